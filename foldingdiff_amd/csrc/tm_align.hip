// TM-align-style comparison of two CA traces whose residues do not correspond: the residue alignment and the
// superposition are searched together -- what tmalign.run_tmalign computes for tmalign.max_tm_across_refs
// (bin/tmscore_training.py) and get_pairwise_tmscores (bin/hclust_structures.py).  It restates the published method
// (Zhang & Skolnick 2005) with two of its starts and is not pinned to the TMalign binary.  The definition restated here
// (and in tests/tmalign_reference.py, DESIGN.md "TM-align-style alignment"), for x with n1 and y with n2 residues and
// a normalisation length Ln >= min(n1, n2):
//   - an alignment is a strictly increasing partial map i -> j; search(map) is the seed-and-extend TM-score search of
//     tm_score.hip over its n_ali pairs (x_i, y_map[i]), normalised by Ln, at the smallest stride s >= 1 with
//     tm_seed_count(n_ali, s) <= 256; it gives (TM, R, t);
//   - DP(S, g): val[i][0] = val[0][j] = 0; D = val[i-1][j-1] + S[i-1][j-1], H = val[i-1][j] + (g if (i-1, j) was a
//     match), V = val[i][j-1] + (g if (i, j-1) was a match); the cell is a match if D >= H and D >= V (value D), else
//     up if H >= V (value H), else left (value V); trace back from (n1, n2) while i > 0 and j > 0, a match cell puts
//     map[i-1] = j-1;
//   - start 1, gapless threading: offset k pairs x_i with y_{i-k}; every k whose overlap is >= max(m / 2, min(m, 5)),
//     m = min(n1, n2), ascending; the score of k is the TM sum under the least-squares fit on its whole overlap; the
//     largest wins, the first on a tie;
//   - start 2, secondary structure: S = 1 where the P-SEA labels (psea.hip) are equal, else 0; DP(S, -1);
//   - refinement of a start map a0: search(a0) is a candidate; for g in (-0.6, 0), from search(a0)'s transform, up to
//     max_iter times: S = 1 / (1 + |R x_i + t - y_j|^2 / d0^2), map = DP(S, g), stop if it equals the map of the
//     iteration before (a0 at first), else search(map) is a candidate and gives the next transform;
//   - result: the candidate with the largest TM, the first on a tie (start 1 before 2, g = -0.6 before 0, iterations
//     in order).
//
// tm_align_kernel: one workgroup of 256 lanes per pair, a persistent grid striding over the pair list.  Both centred
// traces stay in LDS for the whole pair.
//   search     lane per seed over 48-byte aligned-pair records (tm_lane_search, tm_search.h), then the workgroup's best;
//   threading  lane per offset: one pass for the 16 sums of the fit, one for the TM sum;
//   DP         anti-diagonal wavefront, a lane per cell and a barrier per diagonal: three rolling diagonals of val
//              (fp64) and of the match flag, S computed in the cell, one 2-bit choice per cell packed four to a byte
//              (the four cells of a byte lie on four different diagonals, so no two lanes touch a byte between two
//              barriers); the trace-back runs on lane 0.
// The records of the search and the DP's state are never live together and share one region.  Nothing crosses
// workgroups: no flags, no atomics, no global workspace.  Every loop is bounded: max_iter DPs per start and gap
// penalty, n1 + n2 + 1 diagonals per DP, n1 + n2 trace-back steps, tm_lane_search's bounds per search.
#include "fdmi_kernels.h"
#include "launch_common.h"
#include "tm_search.h"

namespace fdmi {

namespace {

constexpr int kLanes = 256;
constexpr int kMaxLen = 512;       // FDMI_ALIGN_MAX_LEN
constexpr int kMaxSeeds = kLanes;  // one lane per seed: the search of an alignment is one workgroup's work

struct AlignLds {   // byte offsets of the regions for chains of up to N residues
  int x, y, best_T, overlay, xt, diag, flags, choice, maps, labels, total, W;
  __host__ __device__ explicit AlignLds(int N) {
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
    labels = maps + 5 * N * 2;             // a0, cur, prev, best maps and the aligned-residue list (int16)
    total = labels + 2 * N;
  }
};

struct AlignArgs {
  const double* ca;        // [n_res][3]
  const double* cent;      // [n_chains][3]
  const int* offsets;      // [n_chains]
  const int* lens;         // [n_chains]
  const signed char* sse;  // [n_res] P-SEA labels
  const int* pair_a;
  const int* pair_b;
  const int* norm_lens;    // [n_pairs]
  const long long* map_offsets;   // [n_pairs] or null
  double* tm_out;          // [n_pairs]
  double* transform_out;   // [n_pairs][12]
  int* n_ali_out;          // [n_pairs]
  int* map_out;            // or null
  int n_pairs, max_iter, max_len;
};

struct AlignShared {
  double T0[12], curT[12], resT[12], bestT[12];
  double res_sum;
  double red_s[kLanes / 64];
  int red_g[kLanes / 64];
  int winner, n_ali, best_n_ali;
};

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

// start 1: the best gapless threading offset -> a0
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

// map <- DP(S, g).  kSS: S from the labels; otherwise from |xt_i - y_j|^2 with xt = R x + t already in LDS.
template <bool kSS>
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
      if (kSS) {
        S = la[i - 1] == lb[j - 1] ? 1.0 : 0.0;
      } else {
        const double* px = xt + (i - 1) * 3;
        const double* py = yc + (j - 1) * 3;
        const double e0 = px[0] - py[0], e1 = px[1] - py[1], e2 = px[2] - py[2];
        S = 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) * inv_d02);
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

__global__ void __launch_bounds__(kLanes) tm_align_kernel(const AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ AlignShared sh;
  const AlignLds L(a.max_len);
  const int N = (a.max_len + 3) & ~3, pitch = N + 4;
  double* xc = reinterpret_cast<double*>(lds_raw + L.x);
  double* yc = reinterpret_cast<double*>(lds_raw + L.y);
  double* best_T = reinterpret_cast<double*>(lds_raw + L.best_T);
  double* rec = reinterpret_cast<double*>(lds_raw + L.overlay);
  double* xt = reinterpret_cast<double*>(lds_raw + L.xt);
  double* diag = reinterpret_cast<double*>(lds_raw + L.diag);
  unsigned char* flags = lds_raw + L.flags;
  unsigned char* choice = lds_raw + L.choice;
  short* a0 = reinterpret_cast<short*>(lds_raw + L.maps);
  short* cur = a0 + N;
  short* prev = cur + N;
  short* best_map = prev + N;
  short* ali = best_map + N;
  signed char* la = reinterpret_cast<signed char*>(lds_raw + L.labels);
  signed char* lb = la + N;
  const int tid = threadIdx.x;

  for (int p = blockIdx.x; p < a.n_pairs; p += gridDim.x) {
    const int ia = a.pair_a[p], ib = a.pair_b[p];
    const int n1 = a.lens[ia], n2 = a.lens[ib], Ln = a.norm_lens[p];
    const size_t ra = (size_t)a.offsets[ia], rb = (size_t)a.offsets[ib];
    const double* ca = a.cent + (size_t)ia * 3;
    const double* cb = a.cent + (size_t)ib * 3;
    for (int k = tid; k < n1 * 3; k += kLanes) xc[k] = a.ca[ra * 3 + k] - ca[k % 3];
    for (int k = tid; k < n2 * 3; k += kLanes) yc[k] = a.ca[rb * 3 + k] - cb[k % 3];
    for (int k = tid; k < n1; k += kLanes) la[k] = a.sse[ra + k];
    for (int k = tid; k < n2; k += kLanes) lb[k] = a.sse[rb + k];
    __syncthreads();

    const double d0 = tm_d0(Ln), inv_d02 = 1.0 / (d0 * d0);
    double best_sum = -1.0;   // uniform over the workgroup
    // candidate (sh.res_sum, sh.resT, map): kept when strictly better, so the first of a tie stays
    auto offer = [&](const short* map) {
      if (sh.res_sum > best_sum) {
        best_sum = sh.res_sum;
        if (tid < 12) sh.bestT[tid] = sh.resT[tid];
        if (tid == 0) sh.best_n_ali = sh.n_ali;
        for (int i = tid; i < n1; i += kLanes) best_map[i] = map[i];
      }
      __syncthreads();
    };

    for (int start = 0; start < 2; ++start) {
      if (start == 0) {
        threading_start(n1, n2, xc, yc, inv_d02, a0, sh, tid);
      } else {
        dp_align<true>(n1, n2, -1.0, inv_d02, xt, yc, la, lb, diag, flags, choice, L.W, pitch, a0, tid);
      }
      for (int gi = 0; gi < 2; ++gi) {
        const double g = gi == 0 ? -0.6 : 0.0;
        // it = -1 (before the first gap penalty only): search(a0) itself, whose transform starts both refinements
        for (int it = gi == 0 ? -1 : 0; it < a.max_iter; ++it) {
          const short* m = a0;
          if (it >= 0) {
            if (it == 0) {
              if (tid < 12) sh.curT[tid] = sh.T0[tid];
              for (int i = tid; i < n1; i += kLanes) prev[i] = a0[i];
              __syncthreads();
            }
            for (int i = tid; i < n1; i += kLanes) {
              const double x0 = xc[i * 3], x1 = xc[i * 3 + 1], x2 = xc[i * 3 + 2];
#pragma unroll
              for (int r = 0; r < 3; ++r)
                xt[i * 3 + r] = sh.curT[r * 3] * x0 + sh.curT[r * 3 + 1] * x1 + sh.curT[r * 3 + 2] * x2 + sh.curT[9 + r];
            }
            __syncthreads();
            dp_align<false>(n1, n2, g, inv_d02, xt, yc, la, lb, diag, flags, choice, L.W, pitch, cur, tid);
            int differs = 0;
            for (int i = tid; i < n1; i += kLanes) differs |= cur[i] != prev[i];
            if (!__syncthreads_or(differs)) break;
            m = cur;
          }
          search_map(m, n1, xc, yc, rec, ali, best_T, d0, sh, tid);
          if (tid < 12) (it < 0 ? sh.T0 : sh.curT)[tid] = sh.resT[tid];
          if (it >= 0)
            for (int i = tid; i < n1; i += kLanes) prev[i] = cur[i];
          offer(m);
        }
      }
    }

    // TM = sum / Ln; the translation of the centred frames folded back: y ~ R x + (t' + cb - R ca)
    if (tid == 0) {
      a.tm_out[p] = best_sum / Ln;
      a.n_ali_out[p] = sh.best_n_ali;
    }
    if (tid < 9) a.transform_out[(size_t)p * 12 + tid] = sh.bestT[tid];
    if (tid < 3)
      a.transform_out[(size_t)p * 12 + 9 + tid] =
          sh.bestT[9 + tid] + cb[tid] - (sh.bestT[tid * 3] * ca[0] + sh.bestT[tid * 3 + 1] * ca[1] + sh.bestT[tid * 3 + 2] * ca[2]);
    if (a.map_out) {
      int* mo = a.map_out + a.map_offsets[p];
      for (int i = tid; i < n1; i += kLanes) mo[i] = best_map[i];
    }
    __syncthreads();   // the next pair overwrites the traces
  }
}

}  // namespace

hipError_t launch_tm_align(const double* ca, const double* cent, const int* offsets, const int* lens, const signed char* sse,
                           const int* pair_a, const int* pair_b, const int* norm_lens, const long long* map_offsets,
                           int n_pairs, int max_iter, int max_len, double* tm_out, double* transform_out, int* n_ali_out,
                           int* map_out, hipStream_t s) {
  static LdsOptIn opt_in;
  if (max_len < 1 || max_len > kMaxLen) return hipErrorInvalidValue;
  if (!opt_in({reinterpret_cast<const void*>(&tm_align_kernel)}, AlignLds(kMaxLen).total)) return hipErrorInvalidValue;
  const int lds = AlignLds(max_len).total;
  // one workgroup per CU: the kernel holds more than 256 registers per lane (tests/test_tmalign.py reads the figure),
  // so a SIMD runs one of its waves at a time whatever LDS is left
  const int grid = n_pairs < cu_count() ? n_pairs : cu_count();
  const AlignArgs a{ca, cent, offsets, lens, sse, pair_a, pair_b, norm_lens, map_offsets, tm_out, transform_out,
                    n_ali_out, map_out, n_pairs, max_iter, max_len};
  hipLaunchKernelGGL(tm_align_kernel, dim3(grid), dim3(kLanes), lds, s, a);
  return hipGetLastError();
}

}  // namespace fdmi
