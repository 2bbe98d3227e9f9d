// The derivative of NeRF with respect to its features, distance restraints on backbone atoms, and the guide update that sits
// behind a visit of fd_sample_guided (include/fdmi.h).  Three kernels, each one 256-lane workgroup per chain.
//
// nerf_vjp_kernel.  Atom k >= 3 of a chain was placed from atoms k-3, k-2, k-1 by a torsion about the bond (k-2, k-1), a bond
// angle at atom k-1 and a bond length (k-1, k).  Changing any of the three moves atoms k .. n-1 as a rigid body: a rotation
// about the axis u = unit(c - b) through c (torsion), a rotation about unit(r x u) through c (angle; r = d - c), a translation
// along unit(r) (length).  With g_m the upstream gradient at atom m, the derivative of the function is therefore
//     sum_{m >= k} g_m . (axis x (q_m - c)) = axis . (Tq_k - c x Fs_k),     Fs_k = sum_{m >= k} g_m,  Tq_k = sum_{m >= k} q_m x g_m
// for a rotation and unit(r) . Fs_k for the translation: two suffix sums along the chain and three dot products per atom.
// Positions are relative to atom 0 (q_m = p_m - p_0), which keeps the cancellation in Tq - c x Fs small.
// The coordinates do not decide the sense of the last two: r = bl (-cos(angle) u + sin(angle) w), so unit(r x u) is the angle's
// axis times sign(bl sin(angle)) and unit(r) the bond's direction times sign(bl) -- (angle, torsion) and (-angle, torsion + pi)
// build the same chain.  With `feats`, the float32 rows the forward read (row i for every angle and length of atom 3 i + 3 + j),
// the angle's slot is multiplied by sign(sin((double)angle)) sign(bl) and the length's by sign(bl); the sign of zero and of a
// default counts as +1.  feats == nullptr: every sign +1 (fd_nerf_vjp), right where sin(angle) > 0 and bl > 0.
// Lane t owns atoms [t * per, (t + 1) * per), per = ceil(n / 256): pass 1 sums its own g and q x g (last atom first), a wave
// suffix scan (64-lane shuffles of the fp64 halves, a fixed doubling tree) and four wave totals in LDS give the sum over the
// lanes behind it, pass 2 walks the same atoms again, last first, with the running suffix.  No per-atom array of suffix sums;
// LDS: the four wave totals of one component at a time, 32 bytes.  The order of every sum is fixed by (n, lane), so two calls give the same bits.
//
// restraint_kernel.  Energy and largest violation: lane t takes restraints t, t + 256, ... of the chain's list, then the same
// fixed tree.  Gradient: the kernel gives each atom to a lane that walks the chain's whole list in order and adds the terms
// that name its atom -- no atomics, the sum of an atom is in list order.  (atoms x restraints distance evaluations per chain:
// 384 x 40 at 128 residues; a per-atom index from the host would pay off from a few thousand restraints per chain.)
//
// guide_update_kernel.  |G_b| over the rows below the length (lane-strided squares, the fixed tree), the clip factor, then per
// element x - float32(c k G) where c != 0 and repeat_tie.hip's + s z and wrap of an untied element, with the same draw.
#include "block_sum.h"
#include "fdmi_kernels.h"
#include "guide_element.h"

namespace fdmi {

namespace {

constexpr int kThreads = kChainThreads;
constexpr int kWaves = kChainWaves;

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 unit(V3 a) {
  const double n = sqrt(dot(a, a));
  return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ V3 load3(const double* p, int k) { return {p[3 * k], p[3 * k + 1], p[3 * k + 2]}; }

// (wave_suffix and block_sum, the workgroup's sum in every lane: block_sum.h)

// the sum of v over the lanes BEHIND this one (exclusive suffix over the workgroup)
__device__ __forceinline__ double block_suffix_excl(double v, double* slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double incl = wave_suffix(v);
  double excl = __shfl_down(incl, 1, 64);
  if (lane == 63) excl = 0.0;
  if (lane == 0) slot[wave] = incl;
  __syncthreads();
  for (int w = wave + 1; w < kWaves; ++w) excl += slot[w];
  __syncthreads();
  return excl;
}

// the (row offset, column) of the three features that placed atom k = 3 i + 3 + j; a column < 0: not a feature
struct VjpColumns {
  int tors[3], ang[3], len[3];
};

__global__ __launch_bounds__(kThreads) void nerf_vjp_kernel(const double* __restrict__ coords, const int* __restrict__ lens, int L,
                                                            int F, VjpColumns col, int centered,
                                                            const double* __restrict__ dcoords, const float* __restrict__ feats,
                                                            double* __restrict__ dfeats) {
  __shared__ double slot[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = lens[b], n = 3 * len;
  const double* p = coords + (size_t)b * 3 * L * 3;
  const double* g = dcoords + (size_t)b * 3 * L * 3;
  double* out = dfeats + (size_t)b * L * F;
  const float* rows = feats ? feats + (size_t)b * L * F : nullptr;
  for (int e = tid; e < len * F; e += kThreads) out[e] = 0.0;
  const int per = (n + kThreads - 1) / kThreads;
  const int k0 = min(n, tid * per), k1 = min(n, k0 + per);
  const V3 origin = load3(p, 0);
  V3 mean = {0.0, 0.0, 0.0};
  if (centered) {  // the derivative of subtracting the mean position: the mean upstream gradient goes off every atom
    V3 sum = {0.0, 0.0, 0.0};
    for (int k = k0; k < k1; ++k) sum = sum + load3(g, k);
    mean = {block_sum(sum.x, slot) / n, block_sum(sum.y, slot) / n, block_sum(sum.z, slot) / n};
  }
  // pass 1: this lane's own sums
  V3 Fl = {0.0, 0.0, 0.0}, Tl = {0.0, 0.0, 0.0};
  for (int k = k1 - 1; k >= k0; --k) {
    const V3 gk = load3(g, k) - mean, qk = load3(p, k) - origin;
    Fl = Fl + gk;
    Tl = Tl + cross(qk, gk);
  }
  // the sums of the lanes behind (the barriers inside also put the zeros above in front of the stores below)
  V3 Fs, Tq;
  Fs.x = block_suffix_excl(Fl.x, slot); Fs.y = block_suffix_excl(Fl.y, slot); Fs.z = block_suffix_excl(Fl.z, slot);
  Tq.x = block_suffix_excl(Tl.x, slot); Tq.y = block_suffix_excl(Tl.y, slot); Tq.z = block_suffix_excl(Tl.z, slot);
  // pass 2: the same atoms, last first, with the running suffix
  for (int k = k1 - 1; k >= k0; --k) {
    const V3 gk = load3(g, k) - mean, d = load3(p, k) - origin;
    Fs = Fs + gk;
    Tq = Tq + cross(d, gk);
    if (k < 3) continue;
    const V3 bb = load3(p, k - 2) - origin, c = load3(p, k - 1) - origin;
    const V3 u = unit(c - bb), r = d - c;
    const V3 M = Tq - cross(c, Fs);
    const int i = (k - 3) / 3, j = (k - 3) % 3;
    const int ct = j == 0 ? col.tors[0] : j == 1 ? col.tors[1] : col.tors[2];
    const int ca = j == 0 ? col.ang[0] : j == 1 ? col.ang[1] : col.ang[2];
    const int cl = j == 0 ? col.len[0] : j == 1 ? col.len[1] : col.len[2];
    out[(size_t)(i + (j == 2)) * F + ct] = dot(u, M);  // (phi belongs to the residue the C atom is in)
    const bool flip_l = rows && cl >= 0 && rows[(size_t)i * F + cl] < 0.f;
    const bool flip_a = flip_l != (rows && ca >= 0 && sin((double)rows[(size_t)i * F + ca]) < 0.0);
    if (ca >= 0) {
      const double da = dot(unit(cross(r, u)), M);
      out[(size_t)i * F + ca] = flip_a ? -da : da;
    }
    if (cl >= 0) {
      const double dl = dot(unit(r), Fs);
      out[(size_t)i * F + cl] = flip_l ? -dl : dl;
    }
  }
}

// what restraint r of the list costs and the gradient term on its atom i (atom j gets the opposite)
struct RestraintTerm {
  double v, e;
  V3 grad;
};
__device__ __forceinline__ RestraintTerm restraint_term(const double* p, const Restraints& rs, int r) {
  const V3 diff = load3(p, rs.i[r]) - load3(p, rs.j[r]);
  const double d = sqrt(dot(diff, diff)), dev = d - rs.d0[r], w = rs.w[r];
  const double v = fmax(0.0, fabs(dev) - rs.tol[r]);
  RestraintTerm t;
  t.v = v;
  t.e = w * v * v;
  t.grad = {0.0, 0.0, 0.0};
  if (v > 0.0 && d > 0.0) {
    const double k = 2.0 * w * v * (dev > 0.0 ? 1.0 : -1.0) / d;
    t.grad = {k * diff.x, k * diff.y, k * diff.z};
  }
  return t;
}

__global__ __launch_bounds__(kThreads) void restraint_kernel(const double* __restrict__ coords, const int* __restrict__ lens, int L,
                                                             Restraints rs, double* __restrict__ energy,
                                                             double* __restrict__ max_violation, double* __restrict__ dcoords) {
  __shared__ double slot[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = 3 * lens[b], r0 = rs.offsets[b], r1 = rs.offsets[b + 1];
  const double* p = coords + (size_t)b * 3 * L * 3;
  double e = 0.0, mv = 0.0;
  for (int r = r0 + tid; r < r1; r += kThreads) {
    const RestraintTerm t = restraint_term(p, rs, r);
    e += t.e;
    mv = fmax(mv, t.v);
  }
  const double total = block_sum(e, slot);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mv = fmax(mv, __shfl_xor(mv, d, 64));
  if ((tid & 63) == 0) slot[tid >> 6] = mv;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) mv = fmax(mv, slot[w]);
    energy[b] = total;
    max_violation[b] = mv;
  }
  if (!dcoords) return;
  double* o = dcoords + (size_t)b * 3 * L * 3;
  for (int a = tid; a < 3 * L; a += kThreads) {
    V3 acc = {0.0, 0.0, 0.0};
    if (a < n)
      for (int r = r0; r < r1; ++r) {
        const bool first = rs.i[r] == a;
        if (!first && rs.j[r] != a) continue;
        const RestraintTerm t = restraint_term(p, rs, r);
        acc = first ? acc + t.grad : acc - t.grad;
      }
    o[3 * a] = acc.x; o[3 * a + 1] = acc.y; o[3 * a + 2] = acc.z;
  }
}

__global__ __launch_bounds__(kThreads) void guide_update_kernel(float* __restrict__ x, const double* __restrict__ G,
                                                                const int* __restrict__ lens, int L, int F, unsigned angle_mask,
                                                                float c, double max_norm, float s, const float* __restrict__ z,
                                                                unsigned long long seed, int t, long long seq_offset,
                                                                double* __restrict__ gnorm) {
  __shared__ double slot[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ne = lens[b] * F;
  const size_t base = (size_t)b * L * F;
  double ss = 0.0;
  for (int e = tid; e < ne; e += kThreads) ss += G[base + e] * G[base + e];
  const double norm = sqrt(block_sum(ss, slot));
  const double ck = (double)c * (norm > max_norm ? max_norm / norm : 1.0);
  if (tid == 0) gnorm[b] = norm;
  for (int e = tid; e < ne; e += kThreads) {
    const size_t o = base + e;
    const int l = e / F, f = e % F;
    x[o] = guide_move(x[o], c, ck, G[o], s, z, o, seed, t, seq_offset + b, l, f, angle_mask);
  }
}

}  // namespace

void launch_nerf_vjp(const double* coords, const int* lens, int B, int L, int F, const NerfFeatures& fx, int centered,
                     const double* dcoords, const float* feats, double* dfeats, hipStream_t s) {
  // atom 3 i + 3 (next N): psi, CA:C:1N, 0C:1N;  3 i + 4 (next CA): omega, C:1N:1CA, N:CA;  3 i + 5 (next C): phi of i + 1,
  // N:CA:C at index i (the reference's quirk, nerf.hip), CA:C
  const VjpColumns col{{fx.psi, fx.omega, fx.phi}, {fx.ang_ca_c_n, fx.ang_c_n_ca, fx.ang_n_ca_c}, {fx.len_c_n, fx.len_n_ca, fx.len_ca_c}};
  hipLaunchKernelGGL(nerf_vjp_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, coords, lens, L, F, col, centered ? 1 : 0, dcoords, feats, dfeats);
}

void launch_restraint_energy(const double* coords, const int* lens, int B, int L, const Restraints& r, double* energy,
                             double* max_violation, double* dcoords, hipStream_t s) {
  hipLaunchKernelGGL(restraint_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, coords, lens, L, r, energy, max_violation, dcoords);
}

void launch_guide_update(float* x, const double* G, const int* lens, int B, int L, int F, unsigned angle_mask, float c,
                         double max_norm, float s, const float* z, unsigned long long seed, int t, long long seq_offset,
                         double* gnorm, hipStream_t st) {
  hipLaunchKernelGGL(guide_update_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, x, G, lens, L, F, angle_mask, c, max_norm, s, z,
                     seed, t, seq_offset, gnorm);
}

}  // namespace fdmi
