// TM-score of residue-paired CA traces: the maximum over superpositions of
//     TM(R, t) = (1 / Ln) * sum_i 1 / (1 + (|R x_i + t - y_i| / d0)^2),
// found by the seed-and-extend search of Zhang & Skolnick (2004) -- the score tmalign.run_tmalign gives _score_angles
// (foldingdiff/sampling.py:266-284) for chains whose residues already correspond.  The search restated here (and in
// tests/tm_reference.py, DESIGN.md "TM-score"):
//   - seeds: fragment lengths n, n/2, n/4, ... (those > lmin) and lmin = min(n, 4); starts 0, stride, 2 stride, ...
//     <= n - l, plus n - l; ordered by length descending, then start ascending;
//   - from each seed: T_0 = least-squares fit on the fragment; then, for k = 0, 1, ...: score TM(T_k), select the
//     residues with d_i < d_cut (or d_cut + 0.5 j, the smallest j >= 1 that selects min(3, n) of them), stop when the
//     selection repeats or after 20 fits on selections, else fit T_{k+1} on the selection;
//   - result: the largest TM(T_k) over all seeds and iterations; ties go to the first in seed, then iteration order.
//
// tm_score_kernel: one lane per seed, 256 seeds of one pair per workgroup.  The pair's centred traces sit in LDS as
// one 48-byte record per residue, and every lane walks all n residues in the same order, so each read is a broadcast.
// One pass per lane and iteration: apply the lane's own transform, add the TM term, and accumulate over the lane's
// selection the 16 sums its next fit needs -- no cross-lane traffic until the end.  The fit is Horn's (horn_fit.h).
// A repeated selection gives bit-identical sums and so a bit-identical fit: the lane stops when its new fit equals
// the one it has (a different selection with the same fit would repeat that fit's iteration exactly, so the result
// is the same).  Lanes keep their best (TM, transform); the workgroup reduces them to one record per chunk, and
// tm_reduce_kernel picks each pair's best chunk.  Every loop is bounded: 21 passes per seed plus one refill pass per
// short selection, 32 Jacobi sweeps per fit.
#include "fdmi_kernels.h"
#include "tm_search.h"

namespace fdmi {

namespace {

constexpr int kChunk = 256;       // seeds (lanes) per workgroup
constexpr int kRecord = 14;       // workspace record per chunk: TM sum, seed, R[9], t[3]

__global__ void __launch_bounds__(kChunk) tm_score_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                          const double* __restrict__ cent, const int* __restrict__ offsets,
                                                          const int* __restrict__ lens, const int* __restrict__ norm_lens,
                                                          const int* __restrict__ chunk_off, int n_pairs, int stride,
                                                          double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double lds[];   // [n][6]: x, y centred
  __shared__ double best_T[12][kChunk];   // each lane's best transform (R, t), kept out of registers for the fit
  __shared__ double red_s[kChunk / 64];
  __shared__ int red_g[kChunk / 64];
  __shared__ int winner;
  const int chunk = blockIdx.x, tid = threadIdx.x;
  // pair of this chunk: the last pair whose first chunk is <= chunk (pairs with seeds have >= 1 chunk)
  int lo = 0, hi = n_pairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_off[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  const int pair = lo, n = lens[pair];
  const double* pa = a + (size_t)offsets[pair] * 3;
  const double* pb = b + (size_t)offsets[pair] * 3;
  const double* c = cent + (size_t)pair * 6;
  for (int i = tid; i < n; i += kChunk) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lds[i * 6 + d] = pa[(size_t)i * 3 + d] - c[d];
      lds[i * 6 + 3 + d] = pb[(size_t)i * 3 + d] - c[3 + d];
    }
  }
  __syncthreads();

  const int g = (chunk - chunk_off[pair]) * kChunk + tid;
  int l = 0, s = 0;
  const bool active = g < tm_seed_count(n, stride);
  if (active) tm_seed(n, stride, g, l, s);
  const double best = tm_lane_search<kChunk>(lds, n, l, s, active, tm_d0(norm_lens[pair]), &best_T[0][0], tid);

  // the chunk's best (TM sum, seed): wave butterflies, then the waves in order; idle lanes hold (-1, INT_MAX)
  double rs = best;
  int rg = best >= 0.0 ? g : 0x7fffffff;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double os = __shfl_xor(rs, o, 64);
    const int og = __shfl_xor(rg, o, 64);
    if (better(os, og, rs, rg)) { rs = os; rg = og; }
  }
  if ((tid & 63) == 0) { red_s[tid >> 6] = rs; red_g[tid >> 6] = rg; }
  __syncthreads();
  if (tid == 0) {
    double ws_s = red_s[0];
    int ws_g = red_g[0];
    for (int w = 1; w < kChunk / 64; ++w)
      if (better(red_s[w], red_g[w], ws_s, ws_g)) { ws_s = red_s[w]; ws_g = red_g[w]; }
    winner = ws_g;
  }
  __syncthreads();
  if (g == winner && best >= 0.0) {
    double* o = ws + (size_t)chunk * kRecord;
    o[0] = best;
    o[1] = (double)g;
#pragma unroll
    for (int q = 0; q < 12; ++q) o[2 + q] = best_T[q][tid];
  }
}

// one lane per pair: the best chunk (the first on a tie: chunks are in seed order), TM = sum / Ln, and the translation
// of the centred frames folded back: b ~ R a + (t' + cb - R ca)
__global__ void __launch_bounds__(64) tm_reduce_kernel(const double* __restrict__ ws, const double* __restrict__ cent,
                                                       const int* __restrict__ norm_lens, const int* __restrict__ chunk_off,
                                                       int n_pairs, double* __restrict__ tm_out,
                                                       double* __restrict__ transform_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  int bi = chunk_off[p];
  for (int ch = chunk_off[p] + 1; ch < chunk_off[p + 1]; ++ch)
    if (ws[(size_t)ch * kRecord] > ws[(size_t)bi * kRecord]) bi = ch;
  const double* r = ws + (size_t)bi * kRecord;
  const double* c = cent + (size_t)p * 6;
  tm_out[p] = r[0] / norm_lens[p];
  double* o = transform_out + (size_t)p * 12;
#pragma unroll
  for (int q = 0; q < 9; ++q) o[q] = r[2 + q];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    o[9 + i] = r[11 + i] + c[3 + i] - (r[2 + i * 3] * c[0] + r[3 + i * 3] * c[1] + r[4 + i * 3] * c[2]);
}

}  // namespace

int tm_chunk_offsets(const int* lens, int n_pairs, int stride, int* chunk_off) {
  long long at = 0;
  for (int p = 0; p < n_pairs; ++p) {
    chunk_off[p] = (int)at;
    at += (tm_seed_count(lens[p], stride) + kChunk - 1) / kChunk;
    if (at > 0x7fffffffLL) return -1;
  }
  chunk_off[n_pairs] = (int)at;
  return (int)at;
}

size_t tm_workspace_bytes(int n_chunks) { return (size_t)n_chunks * kRecord * sizeof(double); }

hipError_t launch_tm_score(const double* a, const double* b, const double* cent, const int* offsets, const int* lens,
                           const int* norm_lens, const int* chunk_off, int n_pairs, int n_chunks, int stride, int max_len,
                           double* ws, double* tm_out, double* transform_out, hipStream_t s) {
  const size_t lds = (size_t)max_len * 6 * sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tm_score_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tm_score_kernel, dim3(n_chunks), dim3(kChunk), lds, s, a, b, cent, offsets, lens, norm_lens, chunk_off,
                     n_pairs, stride, ws);
  hipLaunchKernelGGL(tm_reduce_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, ws, cent, norm_lens, chunk_off, n_pairs,
                     tm_out, transform_out);
  return hipGetLastError();
}

}  // namespace fdmi
