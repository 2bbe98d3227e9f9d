// TM-align-style comparison of two CA traces whose residues do not correspond: the residue alignment and the
// superposition are searched together -- what tmalign.run_tmalign computes for tmalign.max_tm_across_refs
// (bin/tmscore_training.py) and get_pairwise_tmscores (bin/hclust_structures.py).  It restates the published method
// (Zhang & Skolnick 2005) with two of its starts (tm_align_starts.hip has all five, behind fd_tm_align_ex) and is not pinned
// to the TMalign binary.  The shared device code is tm_align_common.h.  The definition restated here
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
#include "tm_align_common.h"

namespace fdmi {

namespace {

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
        dp_align<DP_SS>(n1, n2, -1.0, inv_d02, xt, yc, la, lb, diag, flags, choice, L.W, pitch, a0, tid);
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
            dp_align<DP_DIST>(n1, n2, g, inv_d02, xt, yc, la, lb, diag, flags, choice, L.W, pitch, cur, tid);
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
