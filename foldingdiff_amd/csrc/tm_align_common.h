// Device code shared by tm_align_kernel (tm_align.hip: starts 1 and 2) and tm_starts_kernel (tm_align_starts.hip: all five
// starts): the LDS layout, the workgroup's small state, search(map), start 1's threading and the dynamic programme.  The
// rules are in the header of tm_align.hip and in DESIGN.md "TM-align-style alignment".  Everything has internal linkage:
// each of the two sources gets its own copy.
#pragma once
#include "tm_search.h"

namespace fdmi {

namespace {

constexpr int kLanes = 256;
constexpr int kMaxLen = 512;       // FDMI_ALIGN_MAX_LEN
constexpr int kMaxSeeds = kLanes;  // one lane per seed: the search of an alignment is one workgroup's work

struct AlignLds {   // byte offsets of the regions for chains of up to N residues
  int x, y, best_T, overlay, xt, diag, flags, choice, maps, labels, total, W;
  // n_maps int16 arrays of N: a0, cur, prev, best maps and the aligned-residue list; tm_starts_kernel keeps a sixth
  __host__ __device__ explicit AlignLds(int N, int n_maps = 5) {
    N = (N + 3) & ~3;
    W = N / 4;
    x = 0;
    y = x + N * 24;
    best_T = y + N * 24;
    overlay = best_T + 12 * kLanes * 8;
    xt = overlay;                          // DP: transformed x, three diagonals of val, their flags, the choices
    diag = xt + N * 24;
    flags = diag + 3 * (N + 4) * 8;
    choice = flags + 3 * (N + 4);
    const int dp_end = choice + N * W, rec_end = overlay + N * 48;   // search: [n_ali][6] records
    maps = ((dp_end > rec_end ? dp_end : rec_end) + 7) & ~7;
    labels = maps + n_maps * N * 2;
    total = labels + 2 * N;
  }
};

struct AlignShared {
  double T0[12], curT[12], resT[12], bestT[12];
  double res_sum;
  double red_s[kLanes / 64];
  int red_g[kLanes / 64];
  int winner, n_ali, best_n_ali;
};

// the score matrix of a dynamic programme: 1 / (1 + |xt_i - y_j|^2 inv_d02), label equality, or the first plus half the second
enum DpScore { DP_DIST = 0, DP_SS = 1, DP_SS_DIST = 2 };

// the workgroup's best (value, index) -> sh.winner; idle lanes pass (-1, INT_MAX)
__device__ __forceinline__ void reduce_best(double v, int g, AlignShared& sh, int tid) {
  double rs = v;
  int rg = v >= 0.0 ? g : 0x7fffffff;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double os = __shfl_xor(rs, o, 64);
    const int og = __shfl_xor(rg, o, 64);
    if (better(os, og, rs, rg)) { rs = os; rg = og; }
  }
  if ((tid & 63) == 0) { sh.red_s[tid >> 6] = rs; sh.red_g[tid >> 6] = rg; }
  __syncthreads();
  if (tid == 0) {
    double ws_s = sh.red_s[0];
    int ws_g = sh.red_g[0];
    for (int w = 1; w < kLanes / 64; ++w)
      if (better(sh.red_s[w], sh.red_g[w], ws_s, ws_g)) { ws_s = sh.red_s[w]; ws_g = sh.red_g[w]; }
    sh.winner = ws_g;
    sh.res_sum = ws_s;
  }
  __syncthreads();
}

// search(map): sh.res_sum and sh.resT <- the best TM sum and its transform over the aligned pairs of `map`; sh.n_ali
__device__ __forceinline__ void search_map(const short* __restrict__ map, int n1, const double* __restrict__ xc,
                                  const double* __restrict__ yc, double* __restrict__ rec, short* __restrict__ ali,
                                  double* __restrict__ best_T, double d0, AlignShared& sh, int tid) {
  if (tid < 64) {   // the aligned residues in order: ballot compaction on wave 0
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += 64) {
      const int i = i0 + tid;
      const bool has = i < n1 && map[i] >= 0;
      const unsigned long long m = __ballot(has);
      if (has) ali[base + __popcll(m & ((1ull << tid) - 1ull))] = (short)i;
      base += __popcll(m);
    }
    if (tid == 0) sh.n_ali = base;
  }
  __syncthreads();
  const int n = __builtin_amdgcn_readfirstlane(sh.n_ali);   // uniform: the pass loop is scalar control flow
  for (int k = tid; k < n; k += kLanes) {
    const int i = ali[k], j = map[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      rec[k * 6 + d] = xc[i * 3 + d];
      rec[k * 6 + 3 + d] = yc[j * 3 + d];
    }
  }
  __syncthreads();
  int stride = 1;
  while (tm_seed_count(n, stride) > kMaxSeeds) ++stride;   // ends by stride = n (at most 20 seeds)
  int l = 0, s = 0;
  const bool active = tid < tm_seed_count(n, stride);
  if (active) tm_seed(n, stride, tid, l, s);
  const double best = tm_lane_search<kLanes>(rec, n, l, s, active, d0, best_T, tid);
  reduce_best(best, tid, sh, tid);
  if (tid == sh.winner) {
#pragma unroll
    for (int q = 0; q < 12; ++q) sh.resT[q] = best_T[q * kLanes + tid];
  }
  __syncthreads();
}

// start 1: the best gapless threading offset -> a0; its index (offset + n2 - 1) stays in sh.winner and its score in
// sh.res_sum until the next reduce_best
__device__ __forceinline__ void threading_start(int n1, int n2, const double* __restrict__ xc, const double* __restrict__ yc,
                                       double inv_d02, short* __restrict__ a0, AlignShared& sh, int tid) {
  const int m = n1 < n2 ? n1 : n2, m5 = m < 5 ? m : 5, need = m / 2 > m5 ? m / 2 : m5;
  double best = -1.0;
  int best_idx = 0x7fffffff;
  for (int idx = tid; idx < n1 + n2 - 1; idx += kLanes) {   // ascending per lane: the first of a lane's ties stays
    const int k = idx - (n2 - 1);
    const int lo = k > 0 ? k : 0, hi = n1 < n2 + k ? n1 : n2 + k;
    if (hi - lo < need) continue;
    double sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
    double sxy[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lo; i < hi; ++i) {
      const double* px = xc + i * 3;
      const double* py = yc + (i - k) * 3;
      const double x0 = px[0], x1 = px[1], x2 = px[2], y0 = py[0], y1 = py[1], y2 = py[2];
      sx[0] += x0; sx[1] += x1; sx[2] += x2;
      sy[0] += y0; sy[1] += y1; sy[2] += y2;
      sxy[0] += x0 * y0; sxy[1] += x0 * y1; sxy[2] += x0 * y2;
      sxy[3] += x1 * y0; sxy[4] += x1 * y1; sxy[5] += x1 * y2;
      sxy[6] += x2 * y0; sxy[7] += x2 * y1; sxy[8] += x2 * y2;
    }
    double R[9], t[3];
    fit_from_sums((double)(hi - lo), sx, sy, sxy, R, t);
    double tm = 0.0;
    for (int i = lo; i < hi; ++i) {
      const double* px = xc + i * 3;
      const double* py = yc + (i - k) * 3;
      const double x0 = px[0], x1 = px[1], x2 = px[2];
      const double e0 = R[0] * x0 + R[1] * x1 + R[2] * x2 + t[0] - py[0];
      const double e1 = R[3] * x0 + R[4] * x1 + R[5] * x2 + t[1] - py[1];
      const double e2 = R[6] * x0 + R[7] * x1 + R[8] * x2 + t[2] - py[2];
      tm += 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) * inv_d02);
    }
    if (tm > best) { best = tm; best_idx = idx; }
  }
  reduce_best(best, best_idx, sh, tid);   // offset 0 always qualifies, so there is a winner
  const int k = sh.winner - (n2 - 1);
  const int lo = k > 0 ? k : 0, hi = n1 < n2 + k ? n1 : n2 + k;
  for (int i = tid; i < n1; i += kLanes) a0[i] = (short)(i >= lo && i < hi ? i - k : -1);
  __syncthreads();
}

// map <- DP(S, g).  DP_SS: S from the labels; DP_DIST: from |xt_i - y_j|^2 with xt = R x + t already in LDS; DP_SS_DIST: both.
template <DpScore kScore>
__device__ __forceinline__ void dp_align(int n1, int n2, double g, double inv_d02, const double* __restrict__ xt,
                                const double* __restrict__ yc, const signed char* __restrict__ la,
                                const signed char* __restrict__ lb, double* __restrict__ diag,
                                unsigned char* __restrict__ flags, unsigned char* __restrict__ choice, int W, int pitch,
                                short* __restrict__ map, int tid) {
  for (int i = tid; i < n1; i += kLanes) map[i] = -1;
  for (int d = 0; d <= n1 + n2; ++d) {
    const int c0 = d % 3, c1 = (d + 2) % 3, c2 = (d + 1) % 3;   // diagonals d, d - 1, d - 2
    double* cur = diag + c0 * pitch;
    const double* p1 = diag + c1 * pitch;
    const double* p2 = diag + c2 * pitch;
    unsigned char* fcur = flags + c0 * pitch;
    const unsigned char* f1 = flags + c1 * pitch;
    const int ilo = d > n2 ? d - n2 : 0, ihi = d < n1 ? d : n1;
    for (int i = ilo + tid; i <= ihi; i += kLanes) {
      const int j = d - i;
      if (i == 0 || j == 0) {   // border: value 0, not a match
        cur[i] = 0.0;
        fcur[i] = 0;
        continue;
      }
      double S;
      if (kScore == DP_SS) {
        S = la[i - 1] == lb[j - 1] ? 1.0 : 0.0;
      } else {
        const double* px = xt + (i - 1) * 3;
        const double* py = yc + (j - 1) * 3;
        const double e0 = px[0] - py[0], e1 = px[1] - py[1], e2 = px[2] - py[2];
        S = 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) * inv_d02);
        if (kScore == DP_SS_DIST) S += la[i - 1] == lb[j - 1] ? 0.5 : 0.0;
      }
      const double D = p2[i - 1] + S;
      const double H = p1[i - 1] + (f1[i - 1] ? g : 0.0);   // from (i - 1, j)
      const double V = p1[i] + (f1[i] ? g : 0.0);           // from (i, j - 1)
      const bool match = D >= H && D >= V;
      const unsigned c = match ? 0u : H >= V ? 1u : 2u;
      cur[i] = match ? D : H >= V ? H : V;
      fcur[i] = match ? 1 : 0;
      unsigned char* b = choice + (i - 1) * W + ((j - 1) >> 2);
      const int sh = ((j - 1) & 3) * 2;
      *b = (unsigned char)(sh == 0 ? c : *b | (c << sh));   // (i, j - 1) wrote this byte one barrier ago
    }
    __syncthreads();
  }
  if (tid == 0) {
    int i = n1, j = n2;
    while (i > 0 && j > 0) {   // at most n1 + n2 steps
      const unsigned c = (choice[(i - 1) * W + ((j - 1) >> 2)] >> (((j - 1) & 3) * 2)) & 3u;
      if (c == 0u) {
        map[i - 1] = (short)(j - 1);
        --i; --j;
      } else if (c == 1u) {
        --i;
      } else {
        --j;
      }
    }
  }
  __syncthreads();
}

}  // namespace

}  // namespace fdmi
