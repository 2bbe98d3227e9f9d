// Histogram statistics of angle columns, the device half of custom_metrics.py (foldingdiff/custom_metrics.py:15-78):
//   hist_columns_kernel   np.histogram of every column of values[N][F] against that column's explicit edge array;
//   noise_minmax_kernel   pass 1 of kl_from_dset: per (timestep, feature) the min and max of the noised rows x_t and of
//                         the comparison draw;
//   noise_hist_kernel     pass 2: the same two streams again, histogrammed against edges[t][f][:];
//   noise_draws_kernel    the two streams written out, for a caller that asks for them.
// The rules:
//   bins: numpy's for an explicit edge array e[0..nbins].  Bin i holds e[i] <= x < e[i+1], the last bin also x == e[nbins];
//     everything else (NaN too) is counted in `outside`.  x is the float32 value widened to fp64 and the edges are fp64, so
//     every comparison is exact: it is what searchsorted does after promotion.  One fp64 multiply guesses the bin; the
//     guess is then walked down and up against the edges themselves, so only the comparisons decide.
//   streams: eps = wrap?(scale[f] * z) with z ~ N(0,1) (NoisedAnglesDataset.sample_noise, datasets.py:772-799),
//     x_t = wrap?(keep[t] * x0 + spread[t] * eps), each product and the sum rounded once -- q_sample_kernel's (loss.hip) --
//     and cmp = a second draw treated like eps.  z is Philox (philox_normal.h: sequence = row + row_offset, position 0,
//     step = t, one block for four features) under one seed per stream, or the caller's eps_in and cmp_in taken as they are.
// Every result is an integer count or a min / max, so it does not depend on the grid, the order or the run.  A workgroup
// holds the edges and its 32-bit counts of up to G features in LDS (G chosen by the host so that they fit), counts with
// LDS integer atomics and adds its non-zero counts to the 64-bit totals once, at its end.  Min and max travel as
// order-preserving unsigned keys, so they are integer atomics too.
#include "fdmi_kernels.h"
#include "philox_normal.h"
#include "wrap_pi.h"

// The noising statement must keep its two rounded products and its rounded sum.  hipcc's default lets it contract
// a * b + c into an FMA across statements, and the __f*_rn functions of the HIP headers are plain operators that are
// contracted all the same once they are inlined; so the float32 statements of this file are written with operators, with
// contraction off from here on.
#pragma clang fp contract(off)

namespace fdmi {

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBudget = 65536 - 4 * kThreads * 4 - 64;   // bytes of dynamic LDS a workgroup may ask for without an attribute, less the noise kernels' staged normals

// LDS of a workgroup that holds G features: double e[G][nbins + 1], double per_unit[G], unsigned cnt[G][nbins],
// unsigned outside[G]
__host__ __device__ inline size_t lds_per_feature(int nbins) { return (size_t)(nbins + 2) * 8 + (size_t)(nbins + 1) * 4; }

// unsigned keys ordered as the floats are (NaN aside; -0 sorts below +0, which compare equal)
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the bin of x among the non-decreasing edges e[0..nbins] (LDS), -1 for none; per_unit: bins per unit of x, for the guess
__device__ __forceinline__ int find_bin(double x, const double* __restrict__ e, int nbins, double per_unit) {
  if (!(x >= e[0]) || !(x <= e[nbins])) return -1;
  int i = min(max((int)((x - e[0]) * per_unit), 0), nbins - 1);
  while (i > 0 && x < e[i]) --i;
  while (i < nbins - 1 && x >= e[i + 1]) ++i;
  return i;
}

// (the two later arrays are found from e, G and nbins where they are used: two pointers fewer to hold across the kernels)
struct HistLds {
  double* e;   // [G][nbins + 1]
  int G, nbins;
  __device__ __forceinline__ double* per_unit() const { return e + G * (nbins + 1); }                       // [G]
  __device__ __forceinline__ unsigned* cnt() const { return reinterpret_cast<unsigned*>(per_unit() + G); }   // [G][nbins], then outside[G]
};

__device__ __forceinline__ HistLds hist_lds(unsigned char* lds, int G, int nbins) {
  return HistLds{reinterpret_cast<double*>(lds), G, nbins};
}

// edges of features f0 .. f0 + G - 1 (those below F) into LDS with their bins per unit (0, so guess bin 0, for an empty
// or unbounded range), the counts to 0; every thread calls it, and it ends in a barrier
__device__ __forceinline__ void stage_edges(const double* __restrict__ edges, int f0, int G, int F, int nbins, const HistLds& h) {
  const int per = nbins + 1, live = min(G, F - f0);
  for (int k = threadIdx.x; k < live * per; k += kThreads) h.e[k] = edges[(size_t)f0 * per + k];
  for (int k = threadIdx.x; k < G * nbins + G; k += kThreads) h.cnt()[k] = 0u;
  __syncthreads();
  if ((int)threadIdx.x < G) {
    double v = 0.0;
    if ((int)threadIdx.x < live) {
      const double width = h.e[threadIdx.x * per + nbins] - h.e[threadIdx.x * per];
      if (width > 0.0 && width < 1.7e308) v = (double)nbins / width;
      if (!(v < 1.7e308)) v = 0.0;   // a subnormal width: the quotient is inf
    }
    h.per_unit()[threadIdx.x] = v;
  }
  __syncthreads();
}

// the workgroup's counts into the totals: counts[f][nbins] and outside[f] of the same (timestep, stream)
__device__ __forceinline__ void flush_counts(const unsigned* __restrict__ cnt, int f0, int G, int F, int nbins,
                                             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ outside) {
  const int live = min(G, F - f0);
  for (int k = threadIdx.x; k < live * nbins; k += kThreads)
    if (cnt[k]) atomicAdd(&counts[(size_t)f0 * nbins + k], (unsigned long long)cnt[k]);
  if ((int)threadIdx.x < live && cnt[G * nbins + threadIdx.x])
    atomicAdd(&outside[f0 + threadIdx.x], (unsigned long long)cnt[G * nbins + threadIdx.x]);
}

// grid (row chunk, feature group): thread i of a chunk's pass owns element (row, feature) = (i / g, f0 + i % g)
__global__ __launch_bounds__(kThreads) void hist_columns_kernel(const float* __restrict__ values, long long N, int F,
                                                                const double* __restrict__ edges, int nbins, int G,
                                                                const unsigned char* __restrict__ rows_valid,
                                                                unsigned long long* __restrict__ counts,
                                                                unsigned long long* __restrict__ outside) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  const HistLds h = hist_lds(lds, G, nbins);
  const int f0 = blockIdx.y * G, g = min(G, F - f0);
  stage_edges(edges, f0, G, F, nbins, h);
  const long long n = N * g;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long r = i / g;
    const int fi = (int)(i - r * g);
    if (rows_valid && !rows_valid[r]) continue;
    const int b = find_bin((double)values[(size_t)r * F + f0 + fi], h.e + (size_t)fi * (nbins + 1), nbins, h.per_unit()[fi]);
    atomicAdd(&h.cnt()[b >= 0 ? fi * nbins + b : G * nbins + fi], 1u);
  }
  __syncthreads();
  flush_counts(h.cnt(), f0, G, F, nbins, counts, outside);
}

// The noise kernels come in two instantiations: kGiven = false draws from Philox, kGiven = true reads both streams from
// eps_in / cmp_in (both given).  What a workgroup of them works on: blockIdx.y = the timestep's place in the list, blockIdx.z =
// stream * groups + group; a group is G (1, 2 or 4) features inside one Philox block: features base + k0 .. base + k1 - 1.
struct NoiseSlot {
  int it, t, base, k0, k1;   // base = the first feature of the Philox block
  bool cmp;
  float keep, spread;        // of timestep t
  unsigned long long seed;   // of the slot's stream
  const float* given;        // eps_in / cmp_in moved to the timestep, or null: Philox
};

__device__ __forceinline__ NoiseSlot noise_slot(const NoiseArgs& a) {
  NoiseSlot s;
  const int groups = (a.F + a.G - 1) / a.G, z = blockIdx.z;
  s.it = blockIdx.y;
  s.t = a.timesteps[s.it];
  s.cmp = z >= groups;
  const int f0 = (s.cmp ? z - groups : z) * a.G;
  s.base = f0 & ~3;
  s.k0 = f0 & 3;
  s.k1 = min(s.k0 + a.G, a.F - s.base);
  s.keep = a.keep[s.t];
  s.spread = a.spread[s.t];
  s.seed = s.cmp ? a.seed_cmp : a.seed_eps;
  const float* given = s.cmp ? a.cmp_in : a.eps_in;
  s.given = given ? given + (size_t)s.it * a.N * a.F : nullptr;
  return s;
}

// The four N(0,1) of row r's Philox block into the thread's own LDS places zs[k][thread]: one block serves the up to four
// features of the slot, and the loop over them below stays a loop (one copy of the wrap and of the bin walk in the code,
// not four) without a register array indexed by k.
__device__ __forceinline__ void stage_normals(const NoiseArgs& a, const NoiseSlot& s, long long r, float* __restrict__ zs) {
  philox_normal4(s.seed, s.t, r + a.row_offset, 0, s.base >> 2, zs + threadIdx.x, kThreads);
}

// feature base + k of row r in the slot's stream; *draw = eps (or cmp) itself.  z: the staged normal (unused with given draws)
template <bool kGiven>
__device__ __forceinline__ float noise_value(const NoiseArgs& a, const NoiseSlot& s, long long r, int k, float z, float* draw) {
  const int f = s.base + k;
  const bool angular = (a.angle_mask >> f) & 1u;
  const size_t at = (size_t)r * a.F + f;
  float d;
  if (kGiven) {
    d = s.given[at];
  } else {
    d = z * a.scale[f];
    if (angular) d = wrap_pi(d);
  }
  *draw = d;
  if (s.cmp) return d;
  // sqrt_alphas_cumprod_t * vals + sqrt_one_minus_alphas_cumprod_t * noise: two rounded products, one rounded sum
  float v = s.keep * a.x0[at] + s.spread * d;
  if (angular) v = wrap_pi(v);
  return v;
}

// mins / maxs: keys [nT][2][F]
template <bool kGiven>
__global__ __launch_bounds__(kThreads) void noise_minmax_kernel(NoiseArgs a, unsigned* __restrict__ mins,
                                                                unsigned* __restrict__ maxs) {
  __shared__ float zs[4 * kThreads];
  __shared__ float lo[4 * kThreads];   // the thread's running min / max of feature base + k at [k][thread]
  __shared__ float hi[4 * kThreads];
  const NoiseSlot s = noise_slot(a);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo[k * kThreads + threadIdx.x] = INFINITY;
    hi[k * kThreads + threadIdx.x] = -INFINITY;
  }
  for (unsigned r = blockIdx.x * kThreads + threadIdx.x; r < (unsigned)a.N; r += gridDim.x * kThreads) {   // N < 2^31, the grid far below
    if (!kGiven) stage_normals(a, s, r, zs);
#pragma unroll 1
    for (int k = s.k0; k < s.k1; ++k) {
      const int at = k * kThreads + threadIdx.x;
      float d;
      const float v = noise_value<kGiven>(a, s, r, k, kGiven ? 0.f : zs[at], &d);
      lo[at] = fminf(lo[at], v);
      hi[at] = fmaxf(hi[at], v);
    }
  }
  const size_t out0 = ((size_t)s.it * 2 + (s.cmp ? 1 : 0)) * a.F + s.base;
#pragma unroll 1
  for (int k = s.k0; k < s.k1; ++k) {
    float l = lo[k * kThreads + threadIdx.x], h = hi[k * kThreads + threadIdx.x];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      l = fminf(l, __shfl_xor(l, o, 64));
      h = fmaxf(h, __shfl_xor(h, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && l <= h) {   // l > h: this wave saw no row
      atomicMin(&mins[out0 + k], float_key(l));
      atomicMax(&maxs[out0 + k], float_key(h));
    }
  }
}

// edges [nT][F][nbins + 1]; counts [nT][2][F][nbins], outside [nT][2][F].  The two pointers are needed only by the flush at
// the end, so they wait in LDS rather than in scalar register pairs through the whole kernel (those pairs were the ones
// the compiler had to park in a vector register).
template <bool kGiven>
__global__ __launch_bounds__(kThreads) void noise_hist_kernel(NoiseArgs a, const double* __restrict__ edges, int nbins,
                                                              unsigned long long* __restrict__ counts,
                                                              unsigned long long* __restrict__ outside) {
  extern __shared__ __attribute__((aligned(8))) unsigned char lds[];
  __shared__ float zs[4 * kThreads];
  __shared__ unsigned long long* totals_s[2];
  if (threadIdx.x == 0) {   // stage_edges' barriers come before the read
    totals_s[0] = counts;
    totals_s[1] = outside;
  }
  const HistLds h = hist_lds(lds, a.G, nbins);
  const NoiseSlot s = noise_slot(a);
  const int f0 = s.base + s.k0;
  stage_edges(edges + (size_t)s.it * a.F * (nbins + 1), f0, a.G, a.F, nbins, h);
  for (unsigned r = blockIdx.x * kThreads + threadIdx.x; r < (unsigned)a.N; r += gridDim.x * kThreads) {   // N < 2^31, the grid far below
    if (!kGiven) stage_normals(a, s, r, zs);
#pragma unroll 1
    for (int k = s.k0; k < s.k1; ++k) {
      float d;
      const float v = noise_value<kGiven>(a, s, r, k, kGiven ? 0.f : zs[k * kThreads + threadIdx.x], &d);
      const int fi = k - s.k0;
      const int b = find_bin((double)v, h.e + (size_t)fi * (nbins + 1), nbins, h.per_unit()[fi]);
      atomicAdd(&h.cnt()[b >= 0 ? fi * nbins + b : a.G * nbins + fi], 1u);
    }
  }
  __syncthreads();
  const size_t slab = ((size_t)s.it * 2 + (s.cmp ? 1 : 0)) * a.F;
  flush_counts(h.cnt(), f0, a.G, a.F, nbins, totals_s[0] + slab * nbins, totals_s[1] + slab);
}

// The two streams themselves for a caller that asked for them (small N): the same slots and the same statements as the two
// passes, written out instead of counted.  x_t_out / cmp_out / eps_out: [nT][N][F] or null.
template <bool kGiven>
__global__ __launch_bounds__(kThreads) void noise_draws_kernel(NoiseArgs a, float* __restrict__ x_t_out,
                                                               float* __restrict__ cmp_out, float* __restrict__ eps_out) {
  __shared__ float zs[4 * kThreads];
  const NoiseSlot s = noise_slot(a);
  float* __restrict__ v_out = s.cmp ? cmp_out : x_t_out;
  float* __restrict__ d_out = s.cmp ? nullptr : eps_out;
  for (unsigned r = blockIdx.x * kThreads + threadIdx.x; r < (unsigned)a.N; r += gridDim.x * kThreads) {   // N < 2^31, the grid far below
    if (!kGiven) stage_normals(a, s, r, zs);
#pragma unroll 1
    for (int k = s.k0; k < s.k1; ++k) {
      float d;
      const float v = noise_value<kGiven>(a, s, r, k, kGiven ? 0.f : zs[k * kThreads + threadIdx.x], &d);
      const size_t at = ((size_t)s.it * a.N + r) * a.F + s.base + k;
      if (v_out) v_out[at] = v;
      if (d_out) d_out[at] = d;
    }
  }
}

// row chunks of a launch with `slots` workgroups per chunk: enough workgroups to fill the chip, few enough that the
// flushes at their ends stay a small part of the work
unsigned row_chunks(long long n, long long slots) {
  const long long want = (n + kThreads - 1) / kThreads;
  const long long cap = slots >= 1024 ? 8 : 8192 / slots;
  return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

// features that fit a workgroup's LDS: at least 1 up to nbins = 4096
int hist_features_per_group(int F, int nbins) {
  const int fit = (int)(kLdsBudget / lds_per_feature(nbins));
  return fit < F ? fit : F;
}

}  // namespace

int noise_features_per_group(int nbins) {
  const int fit = hist_features_per_group(4, nbins);
  return fit == 3 ? 2 : fit;   // 1, 2 or 4: a group stays inside one Philox block
}

void launch_hist_columns(const float* values, long long N, int F, const double* edges, int nbins,
                         const unsigned char* rows_valid, unsigned long long* counts, unsigned long long* outside,
                         hipStream_t s) {
  const int G = hist_features_per_group(F, nbins), groups = (F + G - 1) / G;
  const size_t lds = (size_t)G * lds_per_feature(nbins);
  hipLaunchKernelGGL(hist_columns_kernel, dim3(row_chunks(N * G, groups), groups), dim3(kThreads), lds, s, values, N, F, edges,
                     nbins, G, rows_valid, counts, outside);
}

void launch_noise_minmax(const NoiseArgs& a, int nT, unsigned* mins, unsigned* maxs, hipStream_t s) {
  const int slots = 2 * ((a.F + a.G - 1) / a.G);
  const dim3 grid(row_chunks(a.N, (long long)nT * slots), nT, slots);
  if (a.eps_in) hipLaunchKernelGGL(noise_minmax_kernel<true>, grid, dim3(kThreads), 0, s, a, mins, maxs);
  else hipLaunchKernelGGL(noise_minmax_kernel<false>, grid, dim3(kThreads), 0, s, a, mins, maxs);
}

void launch_noise_hist(const NoiseArgs& a, int nT, const double* edges, int nbins, unsigned long long* counts,
                       unsigned long long* outside, float* x_t_out, float* cmp_out, float* eps_out, hipStream_t s) {
  const int slots = 2 * ((a.F + a.G - 1) / a.G);
  const size_t lds = (size_t)a.G * lds_per_feature(nbins);
  const dim3 grid(row_chunks(a.N, (long long)nT * slots), nT, slots);
  if (a.eps_in) hipLaunchKernelGGL(noise_hist_kernel<true>, grid, dim3(kThreads), lds, s, a, edges, nbins, counts, outside);
  else hipLaunchKernelGGL(noise_hist_kernel<false>, grid, dim3(kThreads), lds, s, a, edges, nbins, counts, outside);
  if (!(x_t_out || cmp_out || eps_out)) return;
  if (a.eps_in) hipLaunchKernelGGL(noise_draws_kernel<true>, grid, dim3(kThreads), 0, s, a, x_t_out, cmp_out, eps_out);
  else hipLaunchKernelGGL(noise_draws_kernel<false>, grid, dim3(kThreads), 0, s, a, x_t_out, cmp_out, eps_out);
}

}  // namespace fdmi
