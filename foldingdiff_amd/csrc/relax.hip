// Relaxing backbones in torsion space (fd_relax_energy, fd_relax; include/fdmi.h): the soft clash term on fp64
// coordinates and the kernel that closes an evaluation of the energy and carries the descent.  Both: one 256-lane workgroup per
// chain, no floating-point atomics, every sum in an order fixed by the chain's length.
//
// soft_clash_kernel.  The integer rule of clash_kernel (clash_lddt.hip) made soft: atoms a, b with |a - b| >= 2,
// t = alpha (r_a + r_b) + margin, v = max(0, t - d); E = w sum_{a < b} v^2, and on atom a with partner b
// -2 w v (p_a - p_b) / d where v > 0 and d > 0 (the same expression from either end of a pair).  Layout as clash_kernel: the outer
// loop walks the chain in blocks of 256 atoms, one atom per lane, the inner loop walks the whole chain in LDS tiles of 1024 atoms
// (fp64 here: 24 KiB) in index order, every lane reading the same partner; partners are taken four at a time and the square roots
// and the division are behind a test of the squared distances that nearly every group of four fails.  An atom's gradient is the sum of its terms in index
// order of the partner; the energy is each lane's sum over its partners b > a, reduced through a fixed tree.  The gradient is
// ADDED to dcoords, which launch_restraint_energy has written before (the restraints' term, zeros on the padding).
//
// relax_step_kernel.  Closes the evaluation of a trial state xt whose raw derivative launch_nerf_vjp left in Gt -- adds the
// tether's gradient, zeroes what may not move, takes the norm and the three energies -- then, for the descent, decides whether
// the trial replaces the chain's state and writes the next trial.  The decision and everything it needs live in RelaxState.
#include "fdmi_kernels.h"
#include "wrap_pi.h"

namespace fdmi {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 1024;  // atoms per LDS tile

// the sum of v over the workgroup in a fixed tree, the same bits in every lane; `slot` holds kWaves doubles
__device__ __forceinline__ double block_sum(double v, double* slot) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();  // slot may still be read from the call before
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = slot[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) total += slot[w];
  return total;
}

struct ClashSum {
  double e, gx, gy, gz;
};
__device__ __forceinline__ double dist2(double dx, double dy, double dz) { return dx * dx + dy * dy + dz * dz; }
// what partner b adds to atom a's sums; (dx, dy, dz) = p_a - p_b and d2 its squared length
__device__ __forceinline__ void clash_pair(ClashSum& s, int a, int b, double dx, double dy, double dz, double d2, double lim_n,
                                           double lim_c, double w) {
  if (!(b - a >= 2 || a - b >= 2)) return;
  const double d = sqrt(d2);
  const double v = (b % 3 == 0 ? lim_n : lim_c) - d;
  if (v > 0.0) {
    if (b > a) s.e += v * v;
    if (d > 0.0) {
      const double k = -2.0 * w * v / d;
      s.gx += k * dx; s.gy += k * dy; s.gz += k * dz;
    }
  }
}

__global__ __launch_bounds__(kThreads) void soft_clash_kernel(const double* __restrict__ coords, const int* __restrict__ lens, int L,
                                                              double alpha, double margin, double w, double* __restrict__ energy,
                                                              double* __restrict__ dcoords) {
  __shared__ double tile[kTile * 3];
  __shared__ double slot[kWaves];
  const int chain = blockIdx.x, tid = threadIdx.x, n = lens[chain] * 3;  // atoms
  const double* __restrict__ x = coords + (size_t)chain * 3 * L * 3;
  double* __restrict__ g = dcoords + (size_t)chain * 3 * L * 3;
  double e = 0.0;
  for (int a0 = 0; a0 < n; a0 += kThreads) {
    const int a = a0 + tid;
    const bool live = a < n;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (live) {
      ax = x[(size_t)a * 3];
      ay = x[(size_t)a * 3 + 1];
      az = x[(size_t)a * 3 + 2];
    }
    const double ra = a % 3 == 0 ? 1.55 : 1.7;
    const double lim_n = alpha * (ra + 1.55) + margin, lim_c = alpha * (ra + 1.7) + margin;  // against an N; against a CA or C
    // nearly every pair is far apart: partners are taken four at a time, and the square roots and the division only where one of
    // the four is below a squared limit a little wider than the widest exact one, so that no pair the exact comparison keeps is
    // dropped by the rounding of the square.  What a pair contributes, and the order of the sums, do not depend on the test.
    const double wide = lim_c * (1.0 + 0x1p-40), near2 = wide * wide;
    ClashSum acc = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < n; t0 += kTile) {
      const int m = min(kTile, n - t0);
      __syncthreads();  // the tile before is read to its end
      for (int k = tid; k < m * 3; k += kThreads) tile[k] = x[(size_t)t0 * 3 + k];
      __syncthreads();
      if (live) {
        int j = 0;
        for (; j + 4 <= m; j += 4) {
          double dx[4], dy[4], dz[4], d2[4];
          bool near = false;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            dx[u] = ax - tile[(j + u) * 3]; dy[u] = ay - tile[(j + u) * 3 + 1]; dz[u] = az - tile[(j + u) * 3 + 2];
            d2[u] = dist2(dx[u], dy[u], dz[u]);
            near |= d2[u] < near2;
          }
          if (!near) continue;
#pragma unroll
          for (int u = 0; u < 4; ++u) clash_pair(acc, a, t0 + j + u, dx[u], dy[u], dz[u], d2[u], lim_n, lim_c, w);
        }
        for (; j < m; ++j) {
          const double dx = ax - tile[j * 3], dy = ay - tile[j * 3 + 1], dz = az - tile[j * 3 + 2];
          clash_pair(acc, a, t0 + j, dx, dy, dz, dist2(dx, dy, dz), lim_n, lim_c, w);
        }
      }
    }
    e += acc.e;
    const double gx = acc.gx, gy = acc.gy, gz = acc.gz;
    if (live) {
      g[(size_t)a * 3] += gx;
      g[(size_t)a * 3 + 1] += gy;
      g[(size_t)a * 3 + 2] += gz;
    }
  }
  const double total = block_sum(e, slot);
  if (tid == 0) energy[chain] = w * total;
}

// x - y without a contraction into whatever produced y
__device__ __forceinline__ float sub32(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

// v - 2 pi floor((v + pi) / (2 pi)): the difference of two angles on [-pi, pi)
__device__ __forceinline__ double wrap64(double v) {
  const double PI = 3.14159265358979323846;
  return v - 2.0 * PI * floor((v + PI) / (2.0 * PI));
}

__global__ __launch_bounds__(kThreads) void relax_step_kernel(RelaxStep a) {
  __shared__ double slot[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ne = a.lens[b] * a.F;
  const size_t base = (size_t)b * a.L * a.F;
  float* xt = a.xt + base;  // (read here, rewritten below)
  const float* anchor = a.anchor + base;
  const unsigned char* __restrict__ fixed = a.fixed ? a.fixed + (size_t)b * a.L : nullptr;
  double* Gt = a.Gt + base;
  // close the evaluation of the trial
  double et = 0.0, ss = 0.0;
  for (int e = tid; e < ne; e += kThreads) {
    const int l = e / a.F, f = e % a.F;
    const bool movable = (a.move_mask >> f) & 1u;
    double gv = 0.0;
    if (movable) {
      double delta = (double)xt[e] - (double)anchor[e];
      if ((a.angle_mask >> f) & 1u) delta = wrap64(delta);
      et += delta * delta;
      if (!(fixed && fixed[l])) gv = Gt[e] + 2.0 * a.w_tether * delta;
    }
    Gt[e] = gv;
    ss += gv * gv;
  }
  const double e_tether = a.w_tether * block_sum(et, slot);
  const double norm = sqrt(block_sum(ss, slot));
  const double e_clash = a.e_clash[b], e_rst = a.e_rst[b];
  const double e_trial = e_clash + e_rst + e_tether;
  RelaxState* st = a.state + b;
  // every lane reads the state before lane 0 rewrites it
  const double e_cur = st->e_total, n_cur = st->gnorm, h_cur = st->h;
  __syncthreads();
  const bool accept = a.it == 0 || e_trial <= e_cur;  // false for NaN
  double h = h_cur;
  if (a.it > 0) h *= accept ? a.grow : a.shrink;
  const double e_now = accept ? e_trial : e_cur, n_now = accept ? norm : n_cur;
  if (tid == 0) {
    if (accept) {
      st->e[0] = e_clash; st->e[1] = e_rst; st->e[2] = e_tether;
      st->e_total = e_trial;
      st->gnorm = norm;
      if (a.it > 0) st->accepted += 1;
    }
    st->h = h;
    if (a.trace) a.trace[(size_t)a.it * gridDim.x + b] = e_now;
  }
  float* x = a.x + base;
  double* G = a.G + base;
  const double s = h * n_now > a.max_step ? a.max_step / n_now : h;
  for (int e = tid; e < ne; e += kThreads) {
    if (accept) {
      x[e] = xt[e];
      G[e] = Gt[e];
    }
    if (a.last) continue;
    const int f = e % a.F;
    const double gv = G[e];
    float m = x[e];
    if (gv != 0.0) {  // (what may not move has gv == 0 and keeps its bits)
      m = sub32(m, (float)(s * gv));
      if ((a.angle_mask >> f) & 1u) m = wrap_pi(m);
    }
    xt[e] = m;
  }
}

}  // namespace

void launch_soft_clash(const double* coords, const int* lens, int B, int L, double alpha, double margin, double w, double* energy,
                       double* dcoords, hipStream_t s) {
  hipLaunchKernelGGL(soft_clash_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, coords, lens, L, alpha, margin, w, energy, dcoords);
}

void launch_relax_step(const RelaxStep& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(relax_step_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
}

}  // namespace fdmi
