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
#include "horn_fit.h"

namespace fdmi {

// Number of seeds of an n-residue pair and the (length, start) of seed g; shared by the host's chunk table.
__host__ __device__ inline int tm_seed_count_len(int n, int l, int stride) {
  const int span = n - l;
  return span / stride + 1 + (span % stride != 0 ? 1 : 0);
}

__host__ __device__ inline int tm_seed_count(int n, int stride) {
  const int lmin = n < 4 ? n : 4;
  int total = 0;
  for (int l = n; l > lmin; l /= 2) total += tm_seed_count_len(n, l, stride);
  return total + tm_seed_count_len(n, lmin, stride);
}

namespace {

constexpr int kChunk = 256;       // seeds (lanes) per workgroup
constexpr int kMaxSelFits = 20;   // fits on selections per seed
constexpr int kRecord = 14;       // workspace record per chunk: TM sum, seed, R[9], t[3]

enum LaneMode { SEED = 0, EVAL = 1, REFILL = 2, DONE = 3 };

__device__ inline void tm_seed(int n, int stride, int g, int& l, int& s) {
  const int lmin = n < 4 ? n : 4;
  l = n;
  for (;;) {   // at most log2(n) + 1 lengths
    const int cnt = tm_seed_count_len(n, l, stride);
    if (g < cnt || l == lmin) break;
    g -= cnt;
    l = l / 2 > lmin ? l / 2 : lmin;
  }
  const int span = n - l;
  s = (long long)g * stride <= span ? g * stride : span;   // g = span / stride + 1: the extra start n - l
}

// d0 of the normalisation length and the selection cutoff d_cut = clamp(d0, 4.5, 8)
__device__ inline double tm_d0(int Ln) { return Ln > 21 ? 1.24 * cbrt((double)(Ln - 15)) - 1.8 : 0.5; }

// c^2 for the smallest integer j >= 1 with dn2 < (dcut + 0.5 j)^2, as this lane evaluates it (dn2: the need-th
// smallest squared distance; |coordinates| <= 1e6 keeps j far inside int)
__device__ inline double fallback_cut2(double dn2, double dcut) {
  int j = (int)floor((sqrt(dn2) - dcut) * 2.0) + 1;
  if (j < 1) j = 1;
  for (int it = 0; it < 2 && j > 1; ++it) {
    const double c = dcut + 0.5 * (j - 1);
    if (!(dn2 < c * c)) break;
    --j;
  }
  for (int it = 0; it < 2; ++it) {
    const double c = dcut + 0.5 * j;
    if (dn2 < c * c) break;
    ++j;
  }
  const double c = dcut + 0.5 * j;
  return c * c;
}

// least-squares rigid fit y ~ R x + t from the sums over a selection: m, sum x, sum y, sum x_a y_b
__device__ inline void fit_from_sums(double m, const double sx[3], const double sy[3], const double sxy[9], double R[9],
                                     double t[3]) {
  double cx[3], cy[3], M[3][3], Rm[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { cx[a] = sx[a] / m; cy[a] = sy[a] / m; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) M[a][b] = sxy[a * 3 + b] - sx[a] * cy[b];
  horn_rotation(M, Rm);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) R[a * 3 + b] = Rm[a][b];
    t[a] = cy[a] - (Rm[a][0] * cx[0] + Rm[a][1] * cx[1] + Rm[a][2] * cx[2]);
  }
}

// better (TM sum, seed) pair: larger sum, then smaller seed index
__device__ __forceinline__ bool better(double s, int g, double os, int og) { return s > os || (s == os && g < og); }

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

  const int Ln = norm_lens[pair];
  const double d0 = tm_d0(Ln);
  const double dcut = fmin(fmax(d0, 4.5), 8.0), dcut2 = dcut * dcut, inv_d02 = 1.0 / (d0 * d0);
  const int need = n < 3 ? n : 3;
  const int g = (chunk - chunk_off[pair]) * kChunk + tid;
  int mode = DONE, l = 0, s = 0;
  if (g < tm_seed_count(n, stride)) {
    tm_seed(n, stride, g, l, s);
    mode = SEED;
  }
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  double best = -1.0, c2 = dcut2;
  int k = 0;   // fits on selections so far
  while (mode != DONE) {
    // one pass over the residues under (R, t): TM sum, selection sums, the three smallest squared distances
    double tm = 0.0, m0 = INFINITY, m1 = INFINITY, m2 = INFINITY;
    double sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
    double sxy[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      const double* r = lds + i * 6;
      const double x0 = r[0], x1 = r[1], x2 = r[2], y0 = r[3], y1 = r[4], y2 = r[5];
      const double e0 = R[0] * x0 + R[1] * x1 + R[2] * x2 + t[0] - y0;
      const double e1 = R[3] * x0 + R[4] * x1 + R[5] * x2 + t[1] - y1;
      const double e2 = R[6] * x0 + R[7] * x1 + R[8] * x2 + t[2] - y2;
      const double d2 = e0 * e0 + e1 * e1 + e2 * e2;
      tm += 1.0 / (1.0 + d2 * inv_d02);
      const double lo0 = fmin(m0, d2), hi0 = fmax(m0, d2), lo1 = fmin(m1, hi0), hi1 = fmax(m1, hi0);
      m0 = lo0; m1 = lo1; m2 = fmin(m2, hi1);
      const bool sel = mode == SEED ? (unsigned)(i - s) < (unsigned)l : d2 < c2;
      if (sel) {
        ++cnt;
        sx[0] += x0; sx[1] += x1; sx[2] += x2;
        sy[0] += y0; sy[1] += y1; sy[2] += y2;
        sxy[0] += x0 * y0; sxy[1] += x0 * y1; sxy[2] += x0 * y2;
        sxy[3] += x1 * y0; sxy[4] += x1 * y1; sxy[5] += x1 * y2;
        sxy[6] += x2 * y0; sxy[7] += x2 * y1; sxy[8] += x2 * y2;
      }
    }
    if (mode == EVAL) {
      if (tm > best) {
        best = tm;
#pragma unroll
        for (int q = 0; q < 9; ++q) best_T[q][tid] = R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) best_T[9 + q][tid] = t[q];
      }
      if (k == kMaxSelFits) { mode = DONE; continue; }
      if (cnt < need) {   // widen the cutoff and select again under the same transform
        c2 = fallback_cut2(need == 1 ? m0 : need == 2 ? m1 : m2, dcut);
        mode = REFILL;
        continue;
      }
    }
    double nR[9], nt[3];
    fit_from_sums((double)cnt, sx, sy, sxy, nR, nt);
    if (mode != SEED) {
      bool same = true;
#pragma unroll
      for (int q = 0; q < 9; ++q) same = same && nR[q] == R[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) same = same && nt[q] == t[q];
      if (same) { mode = DONE; continue; }
      ++k;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = nR[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = nt[q];
    c2 = dcut2;
    mode = EVAL;
  }

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
