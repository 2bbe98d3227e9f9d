// The alignment search of tm_align.hip with all five starts of the published method (Zhang & Skolnick 2005), behind
// fd_tm_align_ex's `starts` bit set.  Starts 1 and 2, DP(S, g), search(map) and the refinement are those of tm_align.hip's
// header (the shared device code is tm_align_common.h); like them, the three further starts are restated from the paper
// and pinned against tests/tmalign_starts_reference.py, not against the TMalign binary.  With m = min(n1, n2), d0 = d0(Ln)
// and d01 = d0 + 1.5; the "fit of a set of pairs" is the least-squares superposition of fit_from_sums; the "fit score of
// a map" is the TM sum of 1 / (1 + d^2 / d0^2) over the map's pairs under the fit of all its pairs, -1 below 3 pairs:
//   - start 3, secondary structure plus distance: (R1, t1) = the fit of start 1's winning offset on its whole overlap
//     (the fit that scored it; computed even when start 1 is not requested); S[i][j] = 1 / (1 + |R1 x_i + t1 - y_j|^2 /
//     d01^2) + (0.5 if the P-SEA labels of x_i and y_j are equal, else 0); a0 = DP(S, -1);
//   - start 4, local superposition, only for m >= 12 (skipped below): fragment lengths f_a = min(20, m / 3) and
//     f_b = min(100, m / 2), f_b only if f_b > f_a; for a length f and a chain of n residues the fragment positions are
//     0, J, 2J, ... while position + f <= n, J = max(f, ceil((n - f + 1) / 8)): at most 8 per chain, 64 pairs per length;
//     visited f_a before f_b, then the position in x ascending, then the position in y ascending; for each pair (R, t) =
//     the fit of x[i0 : i0 + f] onto y[j0 : j0 + f], S[i][j] = 1 / (1 + |R x_i + t - y_j|^2 / d01^2), map = DP(S, 0),
//     value = the fit score of that map; a0 = the map with the largest value, the first on a tie; at most 128 programmes;
//   - start 5, fragment threading: a chain has a break after residue i if |c_{i+1} - c_i| >= 4.25 A; its longest stretch
//     is the first longest run without a break; if neither chain has a break the start is skipped (it would equal start
//     1); each chain that has a break and whose longest stretch has >= 4 residues has that stretch threaded, as a chain
//     of its own, against the whole other chain by start 1's rule (the same overlap rule with the stretch's length in
//     place of the chain's, scores under d0(Ln)), the indices shifted back; of the up to two maps the one with the higher
//     threading score is a0, x's on a tie; no map, no start;
//   - result: every requested, non-skipped start is refined as in tm_align.hip; the candidate with the largest TM wins,
//     the first on a tie, candidates in start order 1 .. 5, then g = -0.6 before 0, then iterations in order.  Ties keep
//     the first, so more starts never score below fewer and equal them wherever no later start is strictly better.  If
//     every requested start is skipped there is no candidate: TM = -1, the identity transform and an empty map.
//
// tm_starts_kernel: the mapping of tm_align_kernel -- one workgroup of 256 lanes per pair, a persistent grid, both centred
// traces in LDS, fp64 throughout, nothing crosses workgroups.  The maps region holds a sixth int16 array: the running
// best map of start 4 (and the second map of start 5).  The per-fragment fit, the transform of x into xt and the fit
// score of a map are workgroup work with one summation order (wg_sum): lane q adds its terms q, q + 256, ... in ascending
// order, the 64 lanes of a wave are combined by an xor butterfly (offsets 32, 16, ..., 1), and lane 0 adds the four waves'
// sums in wave order.  The order differs from the restatement's; the decision margins of the parity set (every DP cell
// of a traced path, best against second-best fragment pair) are what make that harmless.  Breaks and longest stretches
// are one scan by lane 0 (n1 + n2 steps).  Every loop is bounded: at most 128 programmes in start 4, two threadings in
// start 5, and tm_align_kernel's bounds for the rest.
#include "fdmi_kernels.h"
#include "launch_common.h"
#include "tm_align_common.h"

namespace fdmi {

namespace {

constexpr int kStarts = 5;
constexpr int kFragPositions = 8;   // per chain and fragment length
constexpr double kBreak2 = 4.25 * 4.25;

struct StartsArgs {
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
  double* start_tm_out;    // [n_pairs][5] or null
  int n_pairs, max_iter, max_len;
  unsigned starts;
};

struct StartsShared {
  double part[kLanes / 64][16];
  double sum[16];
  double T[12];       // wg_fit's result: R row-major, then t
  int stretch[2][3];  // per chain: start and length of the longest stretch, whether the chain has a break
};

// st.sum[q] <- the workgroup's sum of v[q], q < K, in the order of the header; all lanes wait for it
template <int K>
__device__ __forceinline__ void wg_sum(double (&v)[K], StartsShared& st, int tid) {
#pragma unroll
  for (int q = 0; q < K; ++q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) st.part[tid >> 6][q] = v[q];
  }
  __syncthreads();
  if (tid < K) {
    double s = st.part[0][tid];
    for (int w = 1; w < kLanes / 64; ++w) s += st.part[w][tid];
    st.sum[tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ void add_pair(const double* __restrict__ px, const double* __restrict__ py, double (&v)[16]) {
  const double x0 = px[0], x1 = px[1], x2 = px[2], y0 = py[0], y1 = py[1], y2 = py[2];
  v[0] += 1.0;
  v[1] += x0; v[2] += x1; v[3] += x2;
  v[4] += y0; v[5] += y1; v[6] += y2;
  v[7] += x0 * y0; v[8] += x0 * y1; v[9] += x0 * y2;
  v[10] += x1 * y0; v[11] += x1 * y1; v[12] += x1 * y2;
  v[13] += x2 * y0; v[14] += x2 * y1; v[15] += x2 * y2;
}

// st.T <- the fit of the pairs whose 16 sums the lanes hold in v (count first); returns the number of pairs
__device__ __forceinline__ int wg_fit(double (&v)[16], StartsShared& st, int tid) {
  wg_sum<16>(v, st, tid);
  const int cnt = (int)st.sum[0];
  if (tid == 0 && cnt >= 1) {
    double R[9], t[3];
    fit_from_sums(st.sum[0], st.sum + 1, st.sum + 4, st.sum + 7, R, t);
#pragma unroll
    for (int q = 0; q < 9; ++q) st.T[q] = R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) st.T[9 + q] = t[q];
  }
  __syncthreads();
  return cnt;
}

// st.T <- the fit of x[i0 : i0 + f] onto y[j0 : j0 + f]
__device__ __forceinline__ void segment_fit(const double* __restrict__ xc, const double* __restrict__ yc, int i0, int j0, int f,
                                            StartsShared& st, int tid) {
  double v[16] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = tid; q < f; q += kLanes) add_pair(xc + (i0 + q) * 3, yc + (j0 + q) * 3, v);
  wg_fit(v, st, tid);
}

// xt <- T x for the n1 residues of x
__device__ __forceinline__ void transform_x(const double* __restrict__ T, const double* __restrict__ xc, double* __restrict__ xt,
                                            int n1, int tid) {
  for (int i = tid; i < n1; i += kLanes) {
    const double x0 = xc[i * 3], x1 = xc[i * 3 + 1], x2 = xc[i * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) xt[i * 3 + r] = T[r * 3] * x0 + T[r * 3 + 1] * x1 + T[r * 3 + 2] * x2 + T[9 + r];
  }
  __syncthreads();
}

// the fit score of `map` (a TM sum, not divided by Ln); -1 below 3 pairs.  Uniform over the workgroup.
__device__ __forceinline__ double map_fit_score(const short* __restrict__ map, int n1, const double* __restrict__ xc,
                                                const double* __restrict__ yc, double inv_d02, StartsShared& st, int tid) {
  double v[16] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n1; i += kLanes) {
    const int j = map[i];
    if (j >= 0) add_pair(xc + i * 3, yc + j * 3, v);
  }
  if (wg_fit(v, st, tid) < 3) return -1.0;
  double tm[1] = {0.0};
  for (int i = tid; i < n1; i += kLanes) {
    const int j = map[i];
    if (j < 0) continue;
    const double* px = xc + i * 3;
    const double* py = yc + j * 3;
    const double x0 = px[0], x1 = px[1], x2 = px[2];
    const double e0 = st.T[0] * x0 + st.T[1] * x1 + st.T[2] * x2 + st.T[9] - py[0];
    const double e1 = st.T[3] * x0 + st.T[4] * x1 + st.T[5] * x2 + st.T[10] - py[1];
    const double e2 = st.T[6] * x0 + st.T[7] * x1 + st.T[8] * x2 + st.T[11] - py[2];
    tm[0] += 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) * inv_d02);
  }
  wg_sum<1>(tm, st, tid);
  return st.sum[0];
}

// lane 0: (start, length) of the first longest run of c[0 .. n) without a break, and whether there is a break
__device__ __forceinline__ void longest_stretch(const double* __restrict__ c, int n, int* __restrict__ out) {
  int best_s = 0, best_l = 0, start = 0, broken = 0;
  for (int i = 0; i < n; ++i) {
    bool brk = i == n - 1;
    if (!brk) {
      const double e0 = c[(i + 1) * 3] - c[i * 3], e1 = c[(i + 1) * 3 + 1] - c[i * 3 + 1], e2 = c[(i + 1) * 3 + 2] - c[i * 3 + 2];
      brk = e0 * e0 + e1 * e1 + e2 * e2 >= kBreak2;
      broken |= brk;
    }
    if (brk) {
      if (i + 1 - start > best_l) { best_l = i + 1 - start; best_s = start; }
      start = i + 1;
    }
  }
  out[0] = best_s;
  out[1] = best_l;
  out[2] = broken;
}

__device__ __forceinline__ int frag_step(int n, int f) {
  const int spread = (n - f + 1 + kFragPositions - 1) / kFragPositions;
  return f > spread ? f : spread;
}

__global__ void __launch_bounds__(kLanes) tm_starts_kernel(const StartsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ AlignShared sh;
  __shared__ StartsShared st;
  const AlignLds L(a.max_len, 6);
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
  short* alt = ali + N;   // start 4's running best map, start 5's second map
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

    const double d0 = tm_d0(Ln), inv_d02 = 1.0 / (d0 * d0), inv_d012 = 1.0 / ((d0 + 1.5) * (d0 + 1.5));
    const int m = n1 < n2 ? n1 : n2;
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

    int k1 = 0;   // start 1's winning offset, for start 3
    for (int start = 0; start < kStarts; ++start) {
      const bool wanted = (a.starts >> start) & 1u;
      bool have = wanted;
      if (start == 0) {
        have = false;
        if (a.starts & 5u) {   // start 3 builds on start 1's winner
          threading_start(n1, n2, xc, yc, inv_d02, a0, sh, tid);
          k1 = sh.winner - (n2 - 1);
          have = wanted;
        }
      } else if (!wanted) {
        // nothing to build
      } else if (start == 1) {
        dp_align<DP_SS>(n1, n2, -1.0, inv_d02, xt, yc, la, lb, diag, flags, choice, L.W, pitch, a0, tid);
      } else if (start == 2) {
        const int lo = k1 > 0 ? k1 : 0, hi = n1 < n2 + k1 ? n1 : n2 + k1;
        segment_fit(xc, yc, lo, lo - k1, hi - lo, st, tid);
        transform_x(st.T, xc, xt, n1, tid);
        dp_align<DP_SS_DIST>(n1, n2, -1.0, inv_d012, xt, yc, la, lb, diag, flags, choice, L.W, pitch, a0, tid);
      } else if (start == 3) {
        have = m >= 12;
        if (have) {
          const int fa = m / 3 < 20 ? m / 3 : 20, fb = m / 2 < 100 ? m / 2 : 100;
          double best_value = -2.0;
          for (int fi = 0; fi < (fb > fa ? 2 : 1); ++fi) {
            const int f = fi == 0 ? fa : fb, J1 = frag_step(n1, f), J2 = frag_step(n2, f);
            for (int i0 = 0; i0 + f <= n1; i0 += J1) {     // at most 8
              for (int j0 = 0; j0 + f <= n2; j0 += J2) {   // at most 8
                segment_fit(xc, yc, i0, j0, f, st, tid);
                transform_x(st.T, xc, xt, n1, tid);
                dp_align<DP_DIST>(n1, n2, 0.0, inv_d012, xt, yc, la, lb, diag, flags, choice, L.W, pitch, cur, tid);
                const double value = map_fit_score(cur, n1, xc, yc, inv_d02, st, tid);
                if (value > best_value) {
                  best_value = value;
                  for (int i = tid; i < n1; i += kLanes) alt[i] = cur[i];
                }
              }
            }
          }
          __syncthreads();
          for (int i = tid; i < n1; i += kLanes) a0[i] = alt[i];
          __syncthreads();
        }
      } else {
        if (tid == 0) {
          longest_stretch(xc, n1, st.stretch[0]);
          longest_stretch(yc, n2, st.stretch[1]);
        }
        __syncthreads();
        const int sx = st.stretch[0][0], lx = st.stretch[0][1], sy = st.stretch[1][0], ly = st.stretch[1][1];
        const bool use_x = st.stretch[0][2] && lx >= 4, use_y = st.stretch[1][2] && ly >= 4;
        have = use_x || use_y;
        double score_x = -1.0;
        if (use_x) {
          for (int i = tid; i < n1; i += kLanes) a0[i] = -1;
          __syncthreads();
          threading_start(lx, n2, xc + sx * 3, yc, inv_d02, a0 + sx, sh, tid);
          score_x = sh.res_sum;
        }
        if (use_y) {
          threading_start(n1, ly, xc, yc + sy * 3, inv_d02, alt, sh, tid);
          if (!use_x || sh.res_sum > score_x) {
            for (int i = tid; i < n1; i += kLanes) a0[i] = (short)(alt[i] >= 0 ? alt[i] + sy : -1);
          }
          __syncthreads();
        }
      }
      double reached = -1.0;
      if (have) {
        for (int gi = 0; gi < 2; ++gi) {
          const double g = gi == 0 ? -0.6 : 0.0;
          // it = -1 (before the first gap penalty only): search(a0) itself, whose transform starts both refinements
          for (int it = gi == 0 ? -1 : 0; it < a.max_iter; ++it) {
            const short* mp = a0;
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
              mp = cur;
            }
            search_map(mp, n1, xc, yc, rec, ali, best_T, d0, sh, tid);
            if (tid < 12) (it < 0 ? sh.T0 : sh.curT)[tid] = sh.resT[tid];
            if (it >= 0)
              for (int i = tid; i < n1; i += kLanes) prev[i] = cur[i];
            reached = sh.res_sum > reached ? sh.res_sum : reached;
            offer(mp);
          }
        }
      }
      if (a.start_tm_out && tid == 0) a.start_tm_out[(size_t)p * kStarts + start] = have ? reached / Ln : -1.0;
    }

    if (best_sum < 0.0) {   // no candidate: every requested start was skipped
      if (tid < 12) sh.bestT[tid] = tid % 4 == 0 && tid < 9 ? 1.0 : 0.0;
      if (tid == 0) sh.best_n_ali = 0;
      for (int i = tid; i < n1; i += kLanes) best_map[i] = -1;
      __syncthreads();
    }
    // TM = sum / Ln; the translation of the centred frames folded back: y ~ R x + (t' + cb - R ca)
    if (tid == 0) {
      a.tm_out[p] = best_sum < 0.0 ? -1.0 : best_sum / Ln;
      a.n_ali_out[p] = sh.best_n_ali;
    }
    if (tid < 9) a.transform_out[(size_t)p * 12 + tid] = sh.bestT[tid];
    if (tid < 3)
      a.transform_out[(size_t)p * 12 + 9 + tid] = best_sum < 0.0 ? 0.0 :
          sh.bestT[9 + tid] + cb[tid] - (sh.bestT[tid * 3] * ca[0] + sh.bestT[tid * 3 + 1] * ca[1] + sh.bestT[tid * 3 + 2] * ca[2]);
    if (a.map_out) {
      int* mo = a.map_out + a.map_offsets[p];
      for (int i = tid; i < n1; i += kLanes) mo[i] = best_map[i];
    }
    __syncthreads();   // the next pair overwrites the traces
  }
}

}  // namespace

hipError_t launch_tm_starts(const double* ca, const double* cent, const int* offsets, const int* lens, const signed char* sse,
                            const int* pair_a, const int* pair_b, const int* norm_lens, const long long* map_offsets,
                            int n_pairs, int max_iter, int max_len, unsigned starts, double* tm_out, double* transform_out,
                            int* n_ali_out, int* map_out, double* start_tm_out, hipStream_t s) {
  static LdsOptIn opt_in;
  if (max_len < 1 || max_len > kMaxLen || starts == 0 || starts >= (1u << kStarts)) return hipErrorInvalidValue;
  if (!opt_in({reinterpret_cast<const void*>(&tm_starts_kernel)}, AlignLds(kMaxLen, 6).total)) return hipErrorInvalidValue;
  const int lds = AlignLds(max_len, 6).total;
  // one workgroup per CU, as for tm_align_kernel: the registers of a lane leave room for one wave per SIMD
  const int grid = n_pairs < cu_count() ? n_pairs : cu_count();
  const StartsArgs a{ca, cent, offsets, lens, sse, pair_a, pair_b, norm_lens, map_offsets, tm_out, transform_out,
                     n_ali_out, map_out, start_tm_out, n_pairs, max_iter, max_len, starts};
  hipLaunchKernelGGL(tm_starts_kernel, dim3(grid), dim3(kLanes), lds, s, a);
  return hipGetLastError();
}

}  // namespace fdmi
