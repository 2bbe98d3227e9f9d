// NeRF forward with one 256-lane workgroup per chain: fd_nerf_scan (include/fdmi.h).  nerf_kernel (nerf.hip) walks
// a chain with one lane, 3 len placements one after the other; here the chain is a prefix scan over rigid transforms.
//
// place() (nerf_place.h) builds the frame [bc | nbc | n] of the three atoms before atom k and adds frame . (d0, d1, d2) to the
// last of them.  The frame of the NEXT atom follows from this one and the displacement alone: with u = unit(d) and
// m = unit(e_x x u), bc' = R u, n' = R m, nbc' = R (m x u).  So atom k >= 3 is a local transform (M_k, d_k),
// M_k = [u | m x u | m], and with (R, p) the frame and position after atom k - 1
//     p_k = R d_k + p,   R_k = R M_k          i.e. (R, p) o (M, d) = (R M, R d + p),
// which is associative.  (d0, d1, d2) is place_local()'s, the same float32 products and float64 default-angle path as fd_nerf.
//
// Lane t owns atoms [t * per, (t + 1) * per), per = ceil(n / 256), as nerf_vjp_kernel does: walk 1 composes the lane's own run
// left to right, a wave-level inclusive scan (__shfl_up of the 12 doubles, a doubling tree) and the four wave totals in LDS give
// the transform in front of the lane, walk 2 places the atoms.  The seed frame is place()'s frame of the three seed atoms.  The
// tree depends on n alone: two calls give the same bits, and a chain's bits do not depend on the batch it is in.  fp64, no
// atomics; LDS: four transforms and four doubles (416 bytes).
#include "fdmi_kernels.h"
#include "nerf_place.h"

namespace fdmi {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// a rigid transform: the columns of R and the translation
struct Rigid {
  D3 c0, c1, c2, p;
};
__device__ __forceinline__ D3 apply(const Rigid& r, D3 v) {
  return {r.c0.x * v.x + r.c1.x * v.y + r.c2.x * v.z, r.c0.y * v.x + r.c1.y * v.y + r.c2.y * v.z,
          r.c0.z * v.x + r.c1.z * v.y + r.c2.z * v.z};
}
__device__ __forceinline__ D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
// a o b: b happens in a's frame
__device__ __forceinline__ Rigid compose(const Rigid& a, const Rigid& b) {
  return {apply(a, b.c0), apply(a, b.c1), apply(a, b.c2), add(apply(a, b.p), a.p)};
}
__device__ __forceinline__ Rigid identity() { return {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}}; }
__device__ __forceinline__ D3 shfl_up3(D3 v, int d) { return {__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64), __shfl_up(v.z, d, 64)}; }
__device__ __forceinline__ Rigid shfl_up(const Rigid& r, int d) { return {shfl_up3(r.c0, d), shfl_up3(r.c1, d), shfl_up3(r.c2, d), shfl_up3(r.p, d)}; }

// the local transform of atom k >= 3 of a chain whose features are f
__device__ __forceinline__ Rigid local_transform(const float* __restrict__ f, int F, const NerfFeatures& fx, int k) {
  const double PI = 3.14159265358979323846;
  const int i = (k - 3) / 3, j = (k - 3) % 3;
  const float* row = f + (size_t)i * F;
  D3 d;
  // next N: C->N bond, CA:C:1N angle, psi_i;  next CA: N->CA bond, C:1N:1CA angle, omega_i;
  // next C: CA->C bond, N:CA:C angle AT INDEX i (reference quirk, nerf.hip), phi_{i+1}
  if (j == 0)
    d = place_local(fx.ang_ca_c_n >= 0, fx.ang_ca_c_n >= 0 ? row[fx.ang_ca_c_n] : 0.f, 115.0 / 180.0 * PI, fx.len_c_n >= 0,
                    fx.len_c_n >= 0 ? row[fx.len_c_n] : 0.f, 1.34, row[fx.psi]);
  else if (j == 1)
    d = place_local(fx.ang_c_n_ca >= 0, fx.ang_c_n_ca >= 0 ? row[fx.ang_c_n_ca] : 0.f, 121.0 / 180.0 * PI, fx.len_n_ca >= 0,
                    fx.len_n_ca >= 0 ? row[fx.len_n_ca] : 0.f, 1.46, row[fx.omega]);
  else
    d = place_local(fx.ang_n_ca_c >= 0, fx.ang_n_ca_c >= 0 ? row[fx.ang_n_ca_c] : 0.f, 109.0 / 180.0 * PI, fx.len_ca_c >= 0,
                    fx.len_ca_c >= 0 ? row[fx.len_ca_c] : 0.f, 1.54, row[F + fx.phi]);
  const D3 u = unit(d);
  const D3 m = unit(cross(D3{1.0, 0.0, 0.0}, u));
  return {u, cross(m, u), m, d};
}

// the sum of v over the workgroup in a fixed tree, the same bits in every lane; `slot` holds kWaves doubles
__device__ __forceinline__ double block_sum(double v, double* slot) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = slot[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) total += slot[w];
  return total;
}

__global__ __launch_bounds__(kThreads) void nerf_scan_kernel(const float* __restrict__ feats, const int* __restrict__ lens, int L,
                                                             int F, NerfFeatures fx, int center, double* __restrict__ out) {
  __shared__ Rigid wave_total[kWaves];
  __shared__ double slot[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = 3 * lens[b];
  const float* f = feats + (size_t)b * L * F;
  double* o = out + (size_t)b * 3 * L * 3;
  const int per = (n + kThreads - 1) / kThreads;
  const int k0 = min(n, tid * per), k1 = min(n, k0 + per);
  // walk 1: the lane's own run, left to right
  Rigid own = identity();
  for (int k = max(k0, 3); k < k1; ++k) own = compose(own, local_transform(f, F, fx, k));
  // inclusive scan over the wave, then the waves in front
  Rigid incl = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Rigid before = shfl_up(incl, d);
    if (lane >= d) incl = compose(before, incl);
  }
  if (lane == 63) wave_total[wave] = incl;
  Rigid excl = shfl_up(incl, 1);
  if (lane == 0) excl = identity();
  __syncthreads();
  for (int w = wave - 1; w >= 0; --w) excl = compose(wave_total[w], excl);
  // the seed: place()'s frame of the three fixed atoms (nerf.py:22-24)
  const D3 s0 = {17.047, 14.099, 3.625}, s1 = {16.967, 12.784, 4.338}, s2 = {15.685, 12.755, 5.133};
  const D3 bc = unit(sub(s2, s1));
  const D3 nn = unit(cross(sub(s1, s0), bc));
  Rigid cur = compose(Rigid{bc, cross(nn, bc), nn, s2}, excl);
  // walk 2: place the atoms
  D3 sum = {0.0, 0.0, 0.0};
  for (int k = k0; k < k1; ++k) {
    D3 p;
    if (k < 3) {
      p = k == 0 ? s0 : k == 1 ? s1 : s2;
    } else {
      const Rigid t = local_transform(f, F, fx, k);
      p = add(apply(cur, t.p), cur.p);
      cur = {apply(cur, t.c0), apply(cur, t.c1), apply(cur, t.c2), p};
    }
    o[3 * k] = p.x; o[3 * k + 1] = p.y; o[3 * k + 2] = p.z;
    sum = add(sum, p);
  }
  if (center) {  // (workgroup-uniform)
    const double mx = block_sum(sum.x, slot) / n, my = block_sum(sum.y, slot) / n, mz = block_sum(sum.z, slot) / n;
    for (int k = k0; k < k1; ++k) { o[3 * k] -= mx; o[3 * k + 1] -= my; o[3 * k + 2] -= mz; }
  }
  for (int e = 3 * n + tid; e < 9 * L; e += kThreads) o[e] = 0.0;  // padding residues
}

}  // namespace

void launch_nerf_scan(const float* feats, const int* lens, int B, int L, int F, const NerfFeatures& fx, int center, double* out,
                      hipStream_t s) {
  hipLaunchKernelGGL(nerf_scan_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, feats, lens, L, F, fx, center ? 1 : 0, out);
}

}  // namespace fdmi
