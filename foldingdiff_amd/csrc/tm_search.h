// The seed-and-extend TM-score search of one lane, shared by tm_score_kernel (tm_score.hip: residue-paired traces) and
// tm_align_kernel and tm_starts_kernel (tm_align.hip, tm_align_starts.hip: the aligned pairs of a residue alignment).  The rules are in the header of
// tm_score.hip and in DESIGN.md "TM-score".
#pragma once
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

constexpr int kTmMaxSelFits = 20;   // fits on selections per seed

enum TmLaneMode { TM_SEED = 0, TM_EVAL = 1, TM_REFILL = 2, TM_DONE = 3 };

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

// The search of one lane from its seed (l, s) over the n records at `rec` (48 bytes each: x then y, in LDS; every lane
// of the workgroup walks them in the same order, so each read is a broadcast).  One pass per iteration: apply the lane's
// own transform, add the TM term, and accumulate over the lane's selection the 16 sums its next fit needs.  Returns the
// lane's best TM sum (-1 for an idle lane) and leaves that transform in best_T[q * kLanes + tid], q < 12 (R, then t).
template <int kLanes>
__device__ __forceinline__ double tm_lane_search(const double* __restrict__ rec, int n, int l, int s, bool active,
                                                 double d0, double* __restrict__ best_T, int tid) {
  const double dcut = fmin(fmax(d0, 4.5), 8.0), dcut2 = dcut * dcut, inv_d02 = 1.0 / (d0 * d0);
  const int need = n < 3 ? n : 3;
  int mode = active ? TM_SEED : TM_DONE;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  double best = -1.0, c2 = dcut2;
  int k = 0;   // fits on selections so far
  while (mode != TM_DONE) {
    // one pass over the residues under (R, t): TM sum, selection sums, the three smallest squared distances
    double tm = 0.0, m0 = INFINITY, m1 = INFINITY, m2 = INFINITY;
    double sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
    double sxy[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      const double* r = rec + i * 6;
      const double x0 = r[0], x1 = r[1], x2 = r[2], y0 = r[3], y1 = r[4], y2 = r[5];
      const double e0 = R[0] * x0 + R[1] * x1 + R[2] * x2 + t[0] - y0;
      const double e1 = R[3] * x0 + R[4] * x1 + R[5] * x2 + t[1] - y1;
      const double e2 = R[6] * x0 + R[7] * x1 + R[8] * x2 + t[2] - y2;
      const double d2 = e0 * e0 + e1 * e1 + e2 * e2;
      tm += 1.0 / (1.0 + d2 * inv_d02);
      const double lo0 = fmin(m0, d2), hi0 = fmax(m0, d2), lo1 = fmin(m1, hi0), hi1 = fmax(m1, hi0);
      m0 = lo0; m1 = lo1; m2 = fmin(m2, hi1);
      const bool sel = mode == TM_SEED ? (unsigned)(i - s) < (unsigned)l : d2 < c2;
      if (sel) {
        ++cnt;
        sx[0] += x0; sx[1] += x1; sx[2] += x2;
        sy[0] += y0; sy[1] += y1; sy[2] += y2;
        sxy[0] += x0 * y0; sxy[1] += x0 * y1; sxy[2] += x0 * y2;
        sxy[3] += x1 * y0; sxy[4] += x1 * y1; sxy[5] += x1 * y2;
        sxy[6] += x2 * y0; sxy[7] += x2 * y1; sxy[8] += x2 * y2;
      }
    }
    if (mode == TM_EVAL) {
      if (tm > best) {
        best = tm;
#pragma unroll
        for (int q = 0; q < 9; ++q) best_T[q * kLanes + tid] = R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) best_T[(9 + q) * kLanes + tid] = t[q];
      }
      if (k == kTmMaxSelFits) { mode = TM_DONE; continue; }
      if (cnt < need) {   // widen the cutoff and select again under the same transform
        c2 = fallback_cut2(need == 1 ? m0 : need == 2 ? m1 : m2, dcut);
        mode = TM_REFILL;
        continue;
      }
    }
    double nR[9], nt[3];
    fit_from_sums((double)cnt, sx, sy, sxy, nR, nt);
    if (mode != TM_SEED) {
      bool same = true;
#pragma unroll
      for (int q = 0; q < 9; ++q) same = same && nR[q] == R[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) same = same && nt[q] == t[q];
      if (same) { mode = TM_DONE; continue; }
      ++k;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = nR[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = nt[q];
    c2 = dcut2;
    mode = TM_EVAL;
  }
  return best;
}

}  // namespace fdmi
