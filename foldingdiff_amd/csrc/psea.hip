// Secondary structure of CA traces by P-SEA (Labesse et al. 1997) as biotite's annotate_sse restates it -- what
// count_structures_in_pdb (bin/annot_secondary_structures.py:64-105) counts.  The definition restated here (and in
// tests/psea_reference.py, DESIGN.md "Secondary structure (P-SEA)"), for the CA atoms x_0 .. x_{n-1} of one chain:
//   d2[i] = |x_{i+1} - x_{i-1}|, d3[i] = |x_{i+2} - x_{i-1}|, d4[i] = |x_{i+3} - x_{i-1}|, r[i] = the angle at x_i,
//   a[i] = the dihedral of x_{i-1} .. x_{i+2} (IUPAC sign); a quantity whose atoms do not all exist fails every test;
//   potential helix:  (d3 in H and d4 in H) or (r in H and a in H); runs of >= 5 are helix;
//   potential strand: (d2 in S and d3 in S and d4 in S) or (r in S and a in S); runs of >= 4 are strand, runs of 3
//     are strand if their residues have >= 5 contacts (4.2 .. 5.2 A to any residue of the chain) between them;
//   labels: 'a' for a helix residue, and for a neighbour of one with d3 in H or r in H; then 'b' for a strand
//     residue, and for a neighbour of one with d3 in S ('b' overwrites 'a');
//   counts: the maximal runs of 'a' and of 'b'.
//
// psea_kernel: one workgroup per chain, the trace in LDS as 24 bytes per residue, lanes striding over the residues.
// Every phase is a gather: a lane writes only the bytes of its own residue and reads its neighbours' bytes of the
// phase before, so the phases need a barrier between them and nothing else.
//   1. the four flag bits of each residue (potential helix / strand, the two extension tests);
//   2. run membership from the flags of the 4 (helix) and 3 (strand) residues on each side -- enough to tell a run of
//      >= 5, >= 4 or exactly 3; a residue of a 3-run counts its contacts in one walk over the chain (every lane reads
//      the same x_j, a broadcast);
//   3. a residue of a 3-run sums the contacts of its run;
//   4. the label from the residue's own and its two neighbours' sets: the two label passes of the definition, which
//      look at the sets and never at labels, folded into one test per residue ('b' tested last, so it wins);
//   5. run starts of 'a' and 'b', summed over the workgroup.
// Every loop is bounded by n or by a constant.
#include "fdmi_kernels.h"

namespace fdmi {

namespace {

constexpr int kThreads = 256;

enum Flag : unsigned char { POT_HELIX = 1, POT_STRAND = 2, EXT_HELIX = 4, EXT_STRAND = 8 };
enum Set : unsigned char { HELIX = 1, STRAND = 2, RUN3 = 4 };
enum Label : signed char { COIL = 0, ALPHA = 1, BETA = 2 };

constexpr double kDeg = 57.295779513082320877;   // 180 / pi

__device__ __forceinline__ bool within(double v, double lo, double hi) { return v >= lo && v <= hi; }   // false for NaN

__device__ inline unsigned char residue_flags(const double* __restrict__ x, int i, int n) {
  if (i < 1 || i > n - 2) return 0;   // no x_{i-1} or no x_{i+1}: nothing is defined
  const double* p = x + (i - 1) * 3;  // x_{i-1}, x_i, x_{i+1} [, x_{i+2} [, x_{i+3}]]
  const double b0[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
  const double b1[3] = {p[6] - p[3], p[7] - p[4], p[8] - p[5]};
  const double e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
  const double d2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
  const double l0 = b0[0] * b0[0] + b0[1] * b0[1] + b0[2] * b0[2], l1 = b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2];
  const double c = -(b0[0] * b1[0] + b0[1] * b1[1] + b0[2] * b1[2]) / sqrt(l0 * l1);
  const double r = acos(fmin(fmax(c, -1.0), 1.0)) * kDeg;   // NaN (coincident atoms) stays NaN
  bool h3 = false, s3 = false, ha = false, sa = false, h4 = false, s4 = false;
  if (i <= n - 3) {
    const double e3[3] = {p[9] - p[0], p[10] - p[1], p[11] - p[2]};
    const double d3 = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
    h3 = within(d3, 4.8, 5.8);
    s3 = within(d3, 9.0, 10.8);
    const double b2[3] = {p[9] - p[6], p[10] - p[7], p[11] - p[8]};
    const double n1[3] = {b0[1] * b1[2] - b0[2] * b1[1], b0[2] * b1[0] - b0[0] * b1[2], b0[0] * b1[1] - b0[1] * b1[0]};
    const double n2[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
    const double y = sqrt(l1) * (b0[0] * n2[0] + b0[1] * n2[1] + b0[2] * n2[2]);
    const double a = atan2(y, n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2]) * kDeg;
    ha = within(a, 30.0, 70.0);
    sa = within(a, -180.0, -125.0) || within(a, 145.0, 180.0);
  }
  if (i <= n - 4) {
    const double e4[3] = {p[12] - p[0], p[13] - p[1], p[14] - p[2]};
    const double d4 = sqrt(e4[0] * e4[0] + e4[1] * e4[1] + e4[2] * e4[2]);
    h4 = within(d4, 5.8, 7.0);
    s4 = within(d4, 11.3, 13.5);
  }
  const bool hr = within(r, 77.0, 101.0), sr = within(r, 110.0, 138.0);
  unsigned char f = 0;
  if ((h3 && h4) || (hr && ha)) f |= POT_HELIX;
  if ((within(d2, 6.1, 7.3) && s3 && s4) || (sr && sa)) f |= POT_STRAND;
  if (h3 || hr) f |= EXT_HELIX;
  if (s3) f |= EXT_STRAND;
  return f;
}

// residues of the run of `bit` around residue i (which has it), looking at most `reach` to each side: back, forward
__device__ inline void run_extent(const unsigned char* __restrict__ flags, int i, int n, unsigned char bit, int reach,
                                  int& back, int& fwd) {
  back = 0;
  while (back < reach && i - back - 1 >= 0 && (flags[i - back - 1] & bit)) ++back;
  fwd = 0;
  while (fwd < reach && i + fwd + 1 < n && (flags[i + fwd + 1] & bit)) ++fwd;
}

__global__ void __launch_bounds__(kThreads) psea_kernel(const double* __restrict__ ca, const int* __restrict__ offsets,
                                                        const int* __restrict__ lens, int max_len,
                                                        signed char* __restrict__ sse_out, int* __restrict__ counts_out) {
  extern __shared__ __attribute__((aligned(16))) double x[];   // [max_len][3]
  unsigned short* contacts = reinterpret_cast<unsigned short*>(x + (size_t)max_len * 3);   // [max_len], 3-runs only
  unsigned char* flags = reinterpret_cast<unsigned char*>(contacts + max_len);             // [max_len]
  unsigned char* sets = flags + max_len;                                                   // [max_len]
  signed char* label = reinterpret_cast<signed char*>(sets + max_len);                     // [max_len]
  __shared__ int red[kThreads / 64];
  const int chain = blockIdx.x, tid = threadIdx.x, n = lens[chain];
  const size_t row0 = (size_t)offsets[chain];
  for (int k = tid; k < n * 3; k += kThreads) x[k] = ca[row0 * 3 + k];
  __syncthreads();

  for (int i = tid; i < n; i += kThreads) flags[i] = residue_flags(x, i, n);
  __syncthreads();

  for (int i = tid; i < n; i += kThreads) {
    const unsigned char f = flags[i];
    unsigned char s = 0;
    int back, fwd;
    if (f & POT_HELIX) {
      run_extent(flags, i, n, POT_HELIX, 4, back, fwd);
      if (back + fwd + 1 >= 5) s |= HELIX;
    }
    if (f & POT_STRAND) {
      run_extent(flags, i, n, POT_STRAND, 3, back, fwd);
      if (back + fwd + 1 >= 4) {
        s |= STRAND;
      } else if (back + fwd + 1 == 3) {
        s |= RUN3;
        const double xi = x[i * 3], yi = x[i * 3 + 1], zi = x[i * 3 + 2];
        int cnt = 0;
        for (int j = 0; j < n; ++j) {
          const double dx = x[j * 3] - xi, dy = x[j * 3 + 1] - yi, dz = x[j * 3 + 2] - zi;
          const double d = dx * dx + dy * dy + dz * dz;
          cnt += (d >= 4.2 * 4.2 && d <= 5.2 * 5.2) ? 1 : 0;
        }
        contacts[i] = (unsigned short)cnt;
      }
    }
    sets[i] = s;
  }
  __syncthreads();

  for (int i = tid; i < n; i += kThreads) {
    if (!(sets[i] & RUN3)) continue;
    int back, fwd;
    run_extent(flags, i, n, POT_STRAND, 3, back, fwd);   // back + fwd == 2
    int sum = 0;
    for (int j = i - back; j <= i + fwd; ++j) sum += contacts[j];
    if (sum >= 5) sets[i] |= STRAND;   // this residue's own byte; the others read contacts only
  }
  __syncthreads();

  for (int i = tid; i < n; i += kThreads) {
    const unsigned char f = flags[i];
    const unsigned char near = (unsigned char)((i > 0 ? sets[i - 1] : 0) | (i + 1 < n ? sets[i + 1] : 0));
    const unsigned char own = sets[i];
    signed char l = COIL;
    if ((own & HELIX) || ((near & HELIX) && (f & EXT_HELIX))) l = ALPHA;
    if ((own & STRAND) || ((near & STRAND) && (f & EXT_STRAND))) l = BETA;
    label[i] = l;
    sse_out[row0 + i] = l;
  }
  __syncthreads();

  int starts = 0;   // run starts of 'a' in the low half, of 'b' in the high half (each <= n / 2 + 1 < 65536)
  for (int i = tid; i < n; i += kThreads) {
    const signed char l = label[i], before = i > 0 ? label[i - 1] : (signed char)COIL;
    if (l != before) starts += l == ALPHA ? 1 : l == BETA ? 0x10000 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) starts += __shfl_xor(starts, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = starts;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += red[w];
    counts_out[chain * 2] = total & 0xffff;
    counts_out[chain * 2 + 1] = total >> 16;
  }
}

}  // namespace

void launch_psea(const double* ca, const int* offsets, const int* lens, int n_chains, int max_len, signed char* sse_out,
                 int* counts_out, hipStream_t s) {
  const size_t lds = (size_t)max_len * (3 * sizeof(double) + sizeof(unsigned short) + 3);   // 58 KiB at 2048
  hipLaunchKernelGGL(psea_kernel, dim3(n_chains), dim3(kThreads), lds, s, ca, offsets, lens, max_len, sse_out, counts_out);
}

}  // namespace fdmi
