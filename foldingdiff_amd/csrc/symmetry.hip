// Cyclic oligomers (fd_symmetry_energy, fd_symmetry_dock, fd_scaffold_guide_step_sym; include/fdmi.h): a chain
// scored against its own C_n copies about z, and the rigid descent on its pose.  fp64, no floating-point atomics, every sum in an
// order fixed by (length, order, lane) through block_sum.h.
//
// symmetry_pair_kernel.  soft_clash_kernel's shape (relax.hip): one 256-lane workgroup per chain, the outer loop walks the chain
// in blocks of 256 atoms, one atom per lane; for each copy k = 1 .. n - 1 the inner loop walks the whole chain in LDS tiles of
// 1024 atoms (fp64: 24 KiB).  A tile holds the PARTNERS R_k (Q p_b + t): placed and rotated once while loading, never per pair.
// Every lane reads the same partner; partners are taken four at a time and the square roots and the divisions sit behind a test
// of the squared distance against a limit widened by (1 + 2^-40): max(d_off, the clash limit) for a CA lane against a CA partner,
// the lane's widest clash limit otherwise, so that no pair an exact comparison keeps is dropped by the rounding of the square.
// What a pair contributes, and the order of the sums, do not depend on the test.  ALL ordered pairs count, a == b included: the
// partner belongs to another chain.  One lane owns g_a: its terms are summed k ascending, partners in index order; the radial
// term's share goes on top for a CA, then Q^T g_a is ADDED to dcoords (which holds what was launched before, or zeros) or, for
// the descent's last evaluation, stored in a spare buffer that the closing launch adds where that trial became the pose.  The
// energies, the contact count, F = sum g and tau = sum y x g close through fixed trees.  No scratch, no flat access.
//
// symmetry_pose_kernel.  One lane per chain: closes an evaluation of the trial pose -- it == 0: the trial becomes the state;
// it > 0: it does where its energy is not above the state's (false for NaN), and h grows or shrinks -- then, unless it is the
// last, writes the next trial by Rodrigues' formula.  Everything the decision needs lives in SymState.
//
// symmetry_place_kernel.  placed = Q p + t by the pair kernel's own expression, and, for the guided step, the turn of a template
// fit's (R, t_fit) (R placed + t_fit ~ p) into the pose (Q, t) = (R^T, -R^T t_fit) that carries p onto placed.
#include <cstddef>

#include "block_sum.h"
#include "fdmi_kernels.h"

namespace fdmi {

namespace {

constexpr int kTile = 1024;  // atoms per LDS tile

struct Pose {
  double q[9], t[3];
};
__device__ __forceinline__ Pose load_pose(const double* __restrict__ p) {
  Pose r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.q[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) r.t[i] = p[9 + i];
  return r;
}
// y = Q p + t: one expression for every place a chain is put into the assembly frame, so that the bits agree
__device__ __forceinline__ void place(const Pose& P, double px, double py, double pz, double& x, double& y, double& z) {
  x = fma(P.q[2], pz, fma(P.q[1], py, fma(P.q[0], px, P.t[0])));
  y = fma(P.q[5], pz, fma(P.q[4], py, fma(P.q[3], px, P.t[1])));
  z = fma(P.q[8], pz, fma(P.q[7], py, fma(P.q[6], px, P.t[2])));
}

struct SymSum {
  double ec, es, cnt, gx, gy, gz;
};
struct SymLims {
  double lim_n, lim_c;   // the lane's clash limit against an N; against a CA or C
  double d_on, d_off, w_clash, w_contact;
};
// what partner (k, b) adds to atom a's sums; (dx, dy, dz) = y_a - R_k y_b and d2 its squared length; pb = b % 3
__device__ __forceinline__ void sym_pair(SymSum& s, bool lane_ca, int pb, double dx, double dy, double dz, double d2, const SymLims& m) {
  const double d = sqrt(d2);
  const double v = (pb == 0 ? m.lim_n : m.lim_c) - d;
  double k = 0.0;
  if (v > 0.0) {
    s.ec += v * v;
    k = -2.0 * m.w_clash * v;
  }
  if (lane_ca && pb == 1) {
    if (d < m.d_on) s.cnt += 1.0;
    if (d < m.d_off) {
      const double span = m.d_off - m.d_on;
      double u = (m.d_off - d) / span;
      if (u > 1.0) u = 1.0;
      s.es += u * u * (3.0 - 2.0 * u);
      k += 6.0 * m.w_contact * u * (1.0 - u) / span;
    }
  }
  if (k != 0.0 && d > 0.0) {
    k /= d;
    s.gx += k * dx; s.gy += k * dy; s.gz += k * dz;
  }
}

__global__ __launch_bounds__(kChainThreads) void symmetry_pair_kernel(SymPair a) {
  __shared__ double tile[kTile * 3];
  __shared__ double slot[kChainWaves];
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int len = a.lens[chain], n = len * 3, ord = a.order[chain];
  if (ord < 2) {  // (the whole workgroup leaves together, before any barrier)
    if (tid == 0) {
      for (int i = 0; i < 3; ++i) a.energy[(size_t)chain * 3 + i] = 0.0;
      a.contacts[chain] = 0;
      if (a.wrench)
        for (int i = 0; i < 6; ++i) a.wrench[(size_t)chain * 6 + i] = 0.0;
    }
    return;
  }
  if (a.reuse && a.reuse[chain].reuse) {  // the descent's last evaluation was at this pose: its values, its stored gradient
    const SymState& st = a.reuse[chain];
    if (tid == 0) {
      for (int i = 0; i < 3; ++i) a.energy[(size_t)chain * 3 + i] = st.e[i];
      a.contacts[chain] = st.contacts;
    }
    if (a.dcoords)
      for (int i = tid; i < n * 3; i += kChainThreads) {
        const size_t o = (size_t)chain * 3 * a.L * 3 + i;
        a.dcoords[o] += a.spare[o];
      }
    return;
  }
  const double* __restrict__ x = a.coords + (size_t)chain * 3 * a.L * 3;
  const Pose P = load_pose(a.pose + (size_t)chain * a.pose_stride);
  // the radial term: the centroid of the placed CA atoms
  double cx = 0.0, cy = 0.0;
  for (int i = tid; i < len; i += kChainThreads) {
    double yx, yy, yz;
    place(P, x[(size_t)i * 9 + 3], x[(size_t)i * 9 + 4], x[(size_t)i * 9 + 5], yx, yy, yz);
    cx += yx; cy += yy;
  }
  cx = block_sum(cx, slot) / len;
  cy = block_sum(cy, slot) / len;
  const double rho = sqrt(cx * cx + cy * cy);
  const double ex = rho - a.r_max > 0.0 ? rho - a.r_max : 0.0;
  const double e_radial = a.w_radial * ex * ex;
  const double rad = rho > 0.0 ? 2.0 * a.w_radial * ex / (rho * len) : 0.0;
  const double* __restrict__ rot = a.rot + (size_t)ord * 24;  // (cos, sin) of 2 pi k / ord at [2 k]

  double ec = 0.0, es = 0.0, cnt = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
  for (int a0 = 0; a0 < n; a0 += kChainThreads) {
    const int at = a0 + tid;
    const bool live = at < n;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (live) place(P, x[(size_t)at * 3], x[(size_t)at * 3 + 1], x[(size_t)at * 3 + 2], ax, ay, az);
    const bool lane_ca = at % 3 == 1;
    const double ra = at % 3 == 0 ? 1.55 : 1.7;
    const SymLims lm = {a.clash_alpha * (ra + 1.55) + a.clash_margin, a.clash_alpha * (ra + 1.7) + a.clash_margin, a.d_on, a.d_off,
                        a.w_clash, a.w_contact};
    const double wide = lm.lim_c * (1.0 + 0x1p-40), near2 = wide * wide;
    const double wide_ca = (lm.lim_c > a.d_off ? lm.lim_c : a.d_off) * (1.0 + 0x1p-40);
    const double near2_ca = lane_ca ? wide_ca * wide_ca : near2;
    SymSum acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 1; k < ord; ++k) {
      const double c = rot[2 * k], s = rot[2 * k + 1];
      for (int t0 = 0; t0 < n; t0 += kTile) {
        const int m = min(kTile, n - t0);
        __syncthreads();  // the tile before is read to its end
        for (int j = tid; j < m; j += kChainThreads) {
          const size_t o = (size_t)(t0 + j) * 3;
          double yx, yy, yz;
          place(P, x[o], x[o + 1], x[o + 2], yx, yy, yz);
          tile[j * 3] = c * yx - s * yy;
          tile[j * 3 + 1] = s * yx + c * yy;
          tile[j * 3 + 2] = yz;
        }
        __syncthreads();
        if (live) {
          int pb = t0 % 3;  // the kind of partner j, kept without a division
          int j = 0;
          for (; j + 4 <= m; j += 4) {
            double dx[4], dy[4], dz[4], d2[4];
            bool near = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              dx[u] = ax - tile[(j + u) * 3]; dy[u] = ay - tile[(j + u) * 3 + 1]; dz[u] = az - tile[(j + u) * 3 + 2];
              d2[u] = dx[u] * dx[u] + dy[u] * dy[u] + dz[u] * dz[u];
              int q = pb + u;
              q = q >= 3 ? q - 3 : q;
              q = q >= 3 ? q - 3 : q;
              near |= d2[u] < (q == 1 ? near2_ca : near2);
            }
            if (near) {
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                int q = pb + u;
                q = q >= 3 ? q - 3 : q;
                q = q >= 3 ? q - 3 : q;
                sym_pair(acc, lane_ca, q, dx[u], dy[u], dz[u], d2[u], lm);
              }
            }
            pb = pb == 2 ? 0 : pb + 1;  // (j advances by 4: the kind by 1)
          }
          for (; j < m; ++j) {
            const double dx = ax - tile[j * 3], dy = ay - tile[j * 3 + 1], dz = az - tile[j * 3 + 2];
            sym_pair(acc, lane_ca, pb, dx, dy, dz, dx * dx + dy * dy + dz * dz, lm);
            pb = pb == 2 ? 0 : pb + 1;
          }
        }
      }
    }
    if (live) {
      double gx = acc.gx, gy = acc.gy;
      const double gz = acc.gz;
      if (lane_ca) {
        gx += rad * cx;
        gy += rad * cy;
      }
      ec += acc.ec; es += acc.es; cnt += acc.cnt;
      fx += gx; fy += gy; fz += gz;
      tx += ay * gz - az * gy;
      ty += az * gx - ax * gz;
      tz += ax * gy - ay * gx;
      if (a.dcoords) {
        double* __restrict__ g = a.dcoords + ((size_t)chain * 3 * a.L + at) * 3;
        const double d0 = P.q[0] * gx + P.q[3] * gy + P.q[6] * gz, d1 = P.q[1] * gx + P.q[4] * gy + P.q[7] * gz,
                     d2 = P.q[2] * gx + P.q[5] * gy + P.q[8] * gz;
        if (a.store) {
          g[0] = d0; g[1] = d1; g[2] = d2;
        } else {
          g[0] += d0; g[1] += d1; g[2] += d2;
        }
      }
    }
  }
  ec = block_sum(ec, slot); es = block_sum(es, slot); cnt = block_sum(cnt, slot);
  fx = block_sum(fx, slot); fy = block_sum(fy, slot); fz = block_sum(fz, slot);
  tx = block_sum(tx, slot); ty = block_sum(ty, slot); tz = block_sum(tz, slot);
  if (tid == 0) {
    a.energy[(size_t)chain * 3] = 0.5 * a.w_clash * ec;
    a.energy[(size_t)chain * 3 + 1] = -0.5 * a.w_contact * es;
    a.energy[(size_t)chain * 3 + 2] = e_radial;
    a.contacts[chain] = (int)cnt;  // (a sum of ones below 2^53: exact)
    if (a.wrench) {
      double* w = a.wrench + (size_t)chain * 6;
      w[0] = fx; w[1] = fy; w[2] = fz; w[3] = tx; w[4] = ty; w[5] = tz;
    }
  }
}

__global__ void symmetry_pose_kernel(SymDock a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  SymState& st = a.state[b];
  const double* et = a.e_trial + (size_t)b * 3;
  const double e_trial = et[0] + et[1] + et[2];
  const bool accept = a.it == 0 || e_trial <= st.e_total;  // false for NaN
  const bool symmetric = a.order[b] >= 2;
  if (accept) {
    for (int i = 0; i < 12; ++i) st.pose[i] = st.trial[i];
    for (int i = 0; i < 3; ++i) st.e[i] = et[i];
    for (int i = 0; i < 6; ++i) st.wrench[i] = a.wrench_trial[(size_t)b * 6 + i];
    st.e_total = e_trial;
    st.contacts = a.contacts_trial[b];
    if (a.it > 0 && symmetric) st.accepted += 1;
  }
  if (a.it > 0 && symmetric) st.h *= accept ? a.grow : a.shrink;  // (a chain of order 1 has nothing to descend: h and accepted stay)
  if (a.trace) a.trace[(size_t)a.it * a.B + b] = st.e_total;
  st.reuse = a.last && accept && symmetric ? 1 : 0;
  if (a.last) return;
  const double h = st.h;
  double w[3], dt[3];
  for (int i = 0; i < 3; ++i) {
    dt[i] = -h * st.wrench[i];
    w[i] = -h * st.wrench[3 + i] / (a.lever * a.lever);
  }
  const double nd = sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
  const double nw = a.lever * sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double m = nd > nw ? nd : nw;
  const double k = m > a.max_shift ? a.max_shift / m : 1.0;
  for (int i = 0; i < 3; ++i) {
    dt[i] *= k;
    w[i] *= k;
  }
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (!(theta > 0.0)) {  // no turn: Q keeps its bits, and so does t where F == 0 too
    for (int i = 0; i < 9; ++i) st.trial[i] = st.pose[i];
    for (int i = 0; i < 3; ++i) st.trial[9 + i] = dt[i] != 0.0 ? st.pose[9 + i] + dt[i] : st.pose[9 + i];
    return;
  }
  const double ux = w[0] / theta, uy = w[1] / theta, uz = w[2] / theta;
  const double c = cos(theta), s = sin(theta), v = 1.0 - c;
  const double R[9] = {c + v * ux * ux,      v * ux * uy - s * uz, v * ux * uz + s * uy,
                       v * uy * ux + s * uz, c + v * uy * uy,      v * uy * uz - s * ux,
                       v * uz * ux - s * uy, v * uz * uy + s * ux, c + v * uz * uz};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      st.trial[i * 3 + j] = R[i * 3] * st.pose[j] + R[i * 3 + 1] * st.pose[3 + j] + R[i * 3 + 2] * st.pose[6 + j];
    st.trial[9 + i] = R[i * 3] * st.pose[9] + R[i * 3 + 1] * st.pose[10] + R[i * 3 + 2] * st.pose[11] + dt[i];
  }
}

// fit != null: state[b].trial <- (R^T, -R^T t_fit) of fit[b] = (R | t_fit) where order[b] >= 2, before anything else
// placed != null: placed[b][a] <- Q p_a + t with the chain's pose at pose + b * pose_stride, atoms below 3 lens[b]
__global__ __launch_bounds__(kChainThreads) void symmetry_place_kernel(const double* __restrict__ coords, const int* __restrict__ lens,
                                                                       const int* __restrict__ order, int L, const double* __restrict__ fit,
                                                                       SymState* __restrict__ state, const double* __restrict__ pose,
                                                                       int pose_stride, double* __restrict__ placed,
                                                                       const int* __restrict__ offsets, double* __restrict__ packed) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (fit) {
    if (tid == 0 && order[b] >= 2) {
      const double* T = fit + (size_t)b * 12;
      double* o = state[b].trial;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = T[j * 3 + i];
        o[9 + i] = -(T[i] * T[9] + T[3 + i] * T[10] + T[6 + i] * T[11]);
      }
    }
    return;
  }
  const Pose P = load_pose(pose + (size_t)b * pose_stride);
  const int n = lens[b] * 3;
  const double* __restrict__ x = coords + (size_t)b * 3 * L * 3;
  double* __restrict__ y = placed ? placed + (size_t)b * 3 * L * 3 : nullptr;
  double* __restrict__ yp = packed && offsets[b + 1] > offsets[b] ? packed + (size_t)offsets[b] * 3 : nullptr;
  for (int at = tid; at < n; at += kChainThreads) {
    double yx, yy, yz;
    place(P, x[(size_t)at * 3], x[(size_t)at * 3 + 1], x[(size_t)at * 3 + 2], yx, yy, yz);
    if (y) {
      y[(size_t)at * 3] = yx; y[(size_t)at * 3 + 1] = yy; y[(size_t)at * 3 + 2] = yz;
    }
    if (yp) {
      yp[(size_t)at * 3] = yx; yp[(size_t)at * 3 + 1] = yy; yp[(size_t)at * 3 + 2] = yz;
    }
  }
}

}  // namespace

void launch_symmetry_pair(const SymPair& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(symmetry_pair_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, s, a);
}

void launch_symmetry_pose(const SymDock& a, hipStream_t s) {
  hipLaunchKernelGGL(symmetry_pose_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, s, a);
}

void launch_symmetry_fit_pose(const double* fit, const int* order, SymState* state, int B, hipStream_t s) {
  hipLaunchKernelGGL(symmetry_place_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, s, nullptr, nullptr, order, 0, fit, state, nullptr,
                     0, nullptr, nullptr, nullptr);
}

void launch_symmetry_place(const double* coords, const int* lens, int B, int L, const double* pose, int pose_stride, double* placed,
                           const int* offsets, double* packed, hipStream_t s) {
  hipLaunchKernelGGL(symmetry_place_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, s, coords, lens, nullptr, L, nullptr, nullptr, pose,
                     pose_stride, placed, offsets, packed);
}

void launch_symmetry_guide(const SymGuide& g, double* gc, hipStream_t s) {
  const int B = g.dock.B, L = g.pair.L;
  const int stride = (int)(sizeof(SymState) / 8);
  const double* state = reinterpret_cast<const double*>(g.dock.state);
  if (g.fit.xyz) {
    launch_template_energy(g.pair.coords, B, L, g.fit, g.fit_energy, g.fit_rmsd, g.fit_transform, nullptr, s);
    launch_symmetry_fit_pose(g.fit_transform, g.pair.order, g.dock.state, B, s);
  }
  SymPair sp = g.pair;
  sp.pose = state + offsetof(SymState, trial) / 8;
  sp.pose_stride = stride;
  sp.energy = g.e_trial;
  sp.contacts = g.contacts_trial;
  sp.wrench = g.wrench_trial;
  sp.dcoords = nullptr;
  SymDock sd = g.dock;
  sd.e_trial = g.e_trial;
  sd.contacts_trial = g.contacts_trial;
  sd.wrench_trial = g.wrench_trial;
  sd.trace = nullptr;
  for (int it = 0; it <= g.pose_iters; ++it) {
    sd.it = it;
    sd.last = it == g.pose_iters;
    if (sd.last && gc) {  // stored, not added: the closing launch adds it where this trial becomes the pose
      sp.dcoords = g.g_spare;
      sp.store = 1;
    }
    launch_symmetry_pair(sp, B, s);
    launch_symmetry_pose(sd, s);
  }
  sp.pose = state + offsetof(SymState, pose) / 8;
  sp.energy = g.energy;
  sp.contacts = g.contacts;
  sp.wrench = nullptr;
  sp.dcoords = gc;
  sp.store = 0;
  sp.reuse = g.dock.state;
  sp.spare = g.g_spare;
  launch_symmetry_pair(sp, B, s);
  if (g.placed || g.placed_packed) launch_symmetry_place(g.pair.coords, g.pair.lens, B, L, sp.pose, stride, g.placed, g.fit.offsets, g.placed_packed, s);
}

void symmetry_rotations(double* rot) {
  const double two_pi = 6.283185307179586476925286766559;
  for (int n = 0; n <= kSymMaxOrder; ++n)
    for (int k = 0; k < 12; ++k) {
      const double ang = n ? two_pi * k / n : 0.0;
      rot[(n * 12 + k) * 2] = cos(ang);
      rot[(n * 12 + k) * 2 + 1] = sin(ang);
    }
}

}  // namespace fdmi
