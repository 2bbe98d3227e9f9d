// Backbone oxygens and DSSP hydrogen-bond states (Kabsch & Sander 1983) of N / CA / C / O backbones.  The rules, restated
// here, in tests/dssp_reference.py and in DESIGN.md 6t, for the residues 0 .. L-1 of one chain, everything in fp64:
//   oxygen:   psi_i = dihedral(N_i, CA_i, C_i, N_{i+1}); O_i is placed from (N_i, CA_i, C_i) at angle 2.0992622, length
//             1.2359372 and torsion psi_i + pi (trans to the next N; the reference's script uses psi_i itself, which is where the
//             next N sits: reference_torsion).  The last residue has no psi and gets NaN.
//   hydrogen: H_j = N_j + unit(C_{j-1} - O_{j-1}) for j >= 1; no donor: residue 0, flag bit 0, O_{j-1} NaN or on C_{j-1}.
//             no acceptor: flag bit 1, O_i NaN.
//   energy:   E(i, j) = 27.888 (1/d(O_i,N_j) + 1/d(C_i,H_j) - 1/d(O_i,H_j) - 1/d(C_i,N_j)) for i != j, i != j - 1; -9.9 if a
//             distance is below 0.5 A, and never below -9.9.
//   kept:     per donor j the two acceptors of lowest E among E < -0.5, ties to the lower index; hb(i, j) = i is one of them.
//   turn_n(i) = hb(i, i + n), n = 3, 4, 5; a minimal n-helix starts at i (1 <= i <= L-n-1) iff turn_n(i-1) and turn_n(i) and
//             covers i .. i+n-1.
//   bridge (1 <= i, j <= L-2, |i - j| >= 3): parallel (hb(i-1,j) and hb(j,i+1)) or (hb(j-1,i) and hb(i,j+1)); antiparallel
//             (hb(i,j) and hb(j,i)) or (hb(i-1,j+1) and hb(j-1,i+1)).  Residue i of a bridge (i, j) is in a ladder iff (i+1, j+1)
//             or (i-1, j-1) is a parallel bridge too / (i+1, j-1) or (i-1, j+1) an antiparallel one.  No bulges, no sheets.
//   labels, in this order: H minimal 4-helices; E ladder, else B bridge, on residues without H; G minimal 3-helices whose three
//             residues carry no other label; I minimal 5-helices likewise; T unlabelled residues inside a turn; S unlabelled
//             residues 2 .. L-3 whose CA_{i-2} -> CA_i -> CA_{i+2} directions differ by more than 70 degrees.
//
// dssp_kernel: one workgroup per chain.  LDS holds what the O(L^2) pass reads L times -- C and O of every residue, 48 bytes,
// read as a broadcast (every lane of a wave asks for the same acceptor) -- and the per-residue state of the later passes: the
// two kept acceptors (2 x int16) and two label bytes (one doubles as the acceptor mask of the O(L^2) pass), 54 bytes per residue = 54 KiB at the cap of 1024, under the 64 KiB a
// workgroup gets without asking and a third of the CU's 160 KiB, so that two long chains still share a CU.  N, CA and the
// flags are read once or twice per residue and stay in global memory.  A donor lives in one lane's registers (N_j, H_j, the
// two best so far); lanes stride over the donors.
// Every phase after the energy pass is a gather on the kept lists: a lane writes only its own residue's bytes and reads
// bytes of the phase before, with a barrier between phases.  hb(i, j) is two compares, so a helix start, a bridge and a
// ladder test are O(1), and a residue's bridge partners come from kept lists: in each alternative of a bridge (i, j), residue
// i or i + 1 is the donor of a bond whose acceptor names j.  Every loop is bounded by L or by a constant.
#include "fdmi_kernels.h"
#include "nerf_place.h"

namespace fdmi {

namespace {

constexpr int kThreads = 256;
constexpr double kPi = 3.14159265358979323846;
constexpr double kOAngle = 2.0992622, kOLength = 1.2359372;
constexpr double kQ = 27.888, kEMin = -9.9, kECut = -0.5, kDMin = 0.5;
constexpr double kBendCos = 0.34202014332566873304;   // cos(70 degrees): the angle exceeds 70 iff its cosine is below

enum State : signed char { NONE = 0, SH = 1, SB = 2, SE = 3, SG = 4, SI = 5, ST = 6, SS = 7 };

__device__ __forceinline__ D3 load3(const double* __restrict__ p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double dist(D3 a, D3 b) {
  const D3 d = sub(a, b);
  return sqrt(dot(d, d));
}
__device__ __forceinline__ bool any_nan(D3 a) { return a.x != a.x || a.y != a.y || a.z != a.z; }

// ------------------------------------------------------------------------------------------------------------- oxygens
__global__ void __launch_bounds__(kThreads) oxygens_kernel(const double* __restrict__ nca_c, const int* __restrict__ offsets,
                                                           const int* __restrict__ lens, int reference_torsion,
                                                           double* __restrict__ out) {
  const int chain = blockIdx.x, n = lens[chain];
  const size_t row0 = (size_t)offsets[chain];
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const double* r = nca_c + (row0 + i) * 9;
    double* o = out + (row0 + i) * 12;
    for (int k = 0; k < 9; ++k) o[k] = r[k];
    D3 ox = {nan(""), nan(""), nan("")};
    if (i + 1 < n) {
      const D3 a = load3(r), b = load3(r + 3), c = load3(r + 6), d = load3(r + 9);
      // psi: the IUPAC dihedral of a, b, c, d
      const D3 b0 = sub(b, a), b1 = sub(c, b), b2 = sub(d, c);
      const D3 n1 = cross(b0, b1), n2 = cross(b1, b2);
      const double psi = atan2(dot(cross(n1, n2), unit(b1)), dot(n1, n2));
      const double tor = reference_torsion ? psi : psi + kPi;
      // the placement step of nerf_place.h with every factor in fp64
      const D3 bc = unit(b1);
      const D3 nn = unit(cross(b0, bc));
      const D3 m = cross(nn, bc);
      const double d0 = -kOLength * cos(kOAngle), d1 = kOLength * cos(tor) * sin(kOAngle), d2 = kOLength * sin(tor) * sin(kOAngle);
      ox = {bc.x * d0 + m.x * d1 + nn.x * d2 + c.x, bc.y * d0 + m.y * d1 + nn.y * d2 + c.y, bc.z * d0 + m.z * d1 + nn.z * d2 + c.z};
    }
    o[9] = ox.x;
    o[10] = ox.y;
    o[11] = ox.z;
  }
}

// ------------------------------------------------------------------------------------------------------------- states
struct Kept {
  const short* acc;   // [L][2]
  int n;
  __device__ __forceinline__ bool hb(int i, int j) const {   // acceptor i, donor j; false outside the chain
    if (i < 0 || j < 0 || i >= n || j >= n) return false;
    return acc[2 * j] == i || acc[2 * j + 1] == i;
  }
  __device__ __forceinline__ bool helix_start(int i, int len) const {
    return i >= 1 && i <= n - len - 1 && hb(i - 1, i - 1 + len) && hb(i, i + len);
  }
  __device__ __forceinline__ bool in_range(int i, int j) const {
    return i >= 1 && j >= 1 && i <= n - 2 && j <= n - 2 && (i - j >= 3 || j - i >= 3);
  }
  __device__ __forceinline__ bool parallel(int i, int j) const {
    return in_range(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1)));
  }
  __device__ __forceinline__ bool antiparallel(int i, int j) const {
    return in_range(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1)));
  }
};

// bit 0: residue i has a bridge, bit 1: it is in a ladder
__device__ inline int bridge_bits(const Kept& k, int i) {
  if (i < 1 || i > k.n - 2) return 0;
  int bits = 0;
  // the partners j each alternative can name: hb(j, i+1) -> j in acc[i+1]; hb(j-1, i) -> j - 1 in acc[i];
  // hb(j, i) -> j in acc[i]; hb(j-1, i+1) -> j - 1 in acc[i+1]
  for (int s = 0; s < 2; ++s) {
    const int a = k.acc[2 * i + s], b = k.acc[2 * (i + 1) + s];
    const int cand[4] = {a, a + 1, b, b + 1};
    for (int c = 0; c < 4; ++c) {
      const int j = cand[c];
      if ((c & 1) == 0 && j < 0) continue;   // an empty slot (-1); -1 + 1 = 0 fails in_range by itself
      if (k.parallel(i, j)) bits |= 1 | ((k.parallel(i + 1, j + 1) || k.parallel(i - 1, j - 1)) ? 2 : 0);
      if (k.antiparallel(i, j)) bits |= 1 | ((k.antiparallel(i + 1, j - 1) || k.antiparallel(i - 1, j + 1)) ? 2 : 0);
    }
  }
  return bits;
}

__global__ void __launch_bounds__(kThreads) dssp_kernel(const double* __restrict__ bb, const unsigned char* __restrict__ flags,
                                                        const int* __restrict__ offsets, const int* __restrict__ lens, int max_len,
                                                        signed char* __restrict__ state_out, int* __restrict__ acc_out,
                                                        double* __restrict__ energy_out, int* __restrict__ counts_out) {
  extern __shared__ __attribute__((aligned(16))) double co[];                 // [max_len][2][3]: C, O
  short* acc = reinterpret_cast<short*>(co + (size_t)max_len * 6);           // [max_len][2]
  signed char* lab_a = reinterpret_cast<signed char*>(acc + 2 * max_len);    // [max_len]
  signed char* lab_b = lab_a + max_len;                                       // [max_len]
  __shared__ int red[kThreads / 64][3];
  const int chain = blockIdx.x, tid = threadIdx.x, n = lens[chain];
  const size_t row0 = (size_t)offsets[chain];
  const double* x = bb + row0 * 12;
  const unsigned char* fl = flags ? flags + row0 : nullptr;
  signed char* accepts = lab_b;   // the acceptor mask of the energy pass; lab_b is first written two barriers later
  for (int k = tid; k < n * 6; k += kThreads) co[k] = x[(k / 6) * 12 + 6 + k % 6];
  for (int i = tid; i < n; i += kThreads) accepts[i] = !any_nan(load3(x + (size_t)i * 12 + 9)) && !(fl && (fl[i] & 2));
  __syncthreads();

  // ---- the energy pass: donor j against every acceptor
  int bonds = 0;
  for (int j = tid; j < n; j += kThreads) {
    double e0 = kECut, e1 = kECut;   // the two lowest so far, e0 <= e1; a candidate must be strictly below to enter
    int a0 = -1, a1 = -1;
    bool donor = j >= 1 && !(fl && (fl[j] & 1));
    D3 nj = {0.0, 0.0, 0.0}, hj = nj;
    if (donor) {
      const D3 cp = load3(co + (j - 1) * 6), op = load3(co + (j - 1) * 6 + 3);
      const D3 v = sub(cp, op);
      const double len = sqrt(dot(v, v));
      donor = len > 0.0;   // false for a NaN oxygen too
      nj = load3(x + (size_t)j * 12);
      hj = {nj.x + v.x / len, nj.y + v.y / len, nj.z + v.z / len};
    }
    if (donor) {
      for (int i = 0; i < n; ++i) {
        if (i == j || i == j - 1 || !accepts[i]) continue;
        const D3 ci = load3(co + i * 6), oi = load3(co + i * 6 + 3);
        const double d_on = dist(oi, nj), d_ch = dist(ci, hj), d_oh = dist(oi, hj), d_cn = dist(ci, nj);
        double e = kQ * (1.0 / d_on + 1.0 / d_ch - 1.0 / d_oh - 1.0 / d_cn);
        if (e < kEMin) e = kEMin;
        if (d_on < kDMin || d_ch < kDMin || d_oh < kDMin || d_cn < kDMin) e = kEMin;
        if (e < e0) {
          e1 = e0;
          a1 = a0;
          e0 = e;
          a0 = i;
        } else if (e < e1) {
          e1 = e;
          a1 = i;
        }
      }
    }
    acc[2 * j] = (short)a0;
    acc[2 * j + 1] = (short)a1;
    bonds += (a0 >= 0) + (a1 >= 0);
    if (acc_out) {
      acc_out[(row0 + j) * 2] = a0;
      acc_out[(row0 + j) * 2 + 1] = a1;
      energy_out[(row0 + j) * 2] = a0 >= 0 ? e0 : 0.0;
      energy_out[(row0 + j) * 2 + 1] = a1 >= 0 ? e1 : 0.0;
    }
  }
  __syncthreads();
  const Kept k{acc, n};

  // ---- H, then E / B on the residues without H
  for (int i = tid; i < n; i += kThreads) {
    signed char l = NONE;
    for (int s = i - 3; s <= i; ++s)
      if (k.helix_start(s, 4)) l = SH;
    if (l == NONE) {
      const int bits = bridge_bits(k, i);
      l = (bits & 2) ? SE : (bits & 1) ? SB : NONE;
    }
    lab_a[i] = l;
  }
  __syncthreads();

  // ---- G: a minimal 3-helix whose residues carry none of H, B, E
  for (int i = tid; i < n; i += kThreads) {
    signed char l = lab_a[i];
    for (int s = i - 2; s <= i && l == NONE; ++s)
      if (k.helix_start(s, 3) && lab_a[s] == NONE && lab_a[s + 1] == NONE && lab_a[s + 2] == NONE) l = SG;
    lab_b[i] = l;
  }
  __syncthreads();

  // ---- I: a minimal 5-helix whose residues carry none of H, B, E, G; then T and S on what is still unlabelled
  for (int i = tid; i < n; i += kThreads) {
    signed char l = lab_b[i];
    for (int s = i - 4; s <= i && l == NONE; ++s) {
      if (!k.helix_start(s, 5)) continue;
      bool free5 = true;
      for (int r = s; r < s + 5; ++r) free5 = free5 && lab_b[r] == NONE;
      if (free5) l = SI;
    }
    if (l == NONE) {
      for (int len = 3; len <= 5; ++len)
        for (int s = i - len + 1; s <= i - 1; ++s)
          if (k.hb(s, s + len)) l = ST;
    }
    if (l == NONE && i >= 2 && i <= n - 3) {
      const D3 c0 = load3(x + (size_t)(i - 2) * 12 + 3), c1 = load3(x + (size_t)i * 12 + 3), c2 = load3(x + (size_t)(i + 2) * 12 + 3);
      const D3 u = sub(c1, c0), v = sub(c2, c1);
      const double c = dot(u, v) / (sqrt(dot(u, u)) * sqrt(dot(v, v)));   // NaN (coincident atoms) fails the test
      if (c < kBendCos) l = SS;
    }
    lab_a[i] = l;
    state_out[row0 + i] = l;
  }
  __syncthreads();

  // ---- counts: kept bonds, run starts of H and of E
  int h_runs = 0, e_runs = 0;
  for (int i = tid; i < n; i += kThreads) {
    const signed char l = lab_a[i], before = i > 0 ? lab_a[i - 1] : (signed char)NONE;
    if (l != before) {
      h_runs += l == SH;
      e_runs += l == SE;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    bonds += __shfl_xor(bonds, o, 64);
    h_runs += __shfl_xor(h_runs, o, 64);
    e_runs += __shfl_xor(e_runs, o, 64);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = bonds;
    red[tid >> 6][1] = h_runs;
    red[tid >> 6][2] = e_runs;
  }
  __syncthreads();
  if (tid < 3 && counts_out) {
    int total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += red[w][tid];
    counts_out[chain * 3 + tid] = total;
  }
}

}  // namespace

void launch_backbone_oxygens(const double* nca_c, const int* offsets, const int* lens, int n_chains, int reference_torsion,
                             double* out, hipStream_t s) {
  hipLaunchKernelGGL(oxygens_kernel, dim3(n_chains), dim3(kThreads), 0, s, nca_c, offsets, lens, reference_torsion, out);
}

void launch_dssp(const double* bb, const unsigned char* flags, const int* offsets, const int* lens, int n_chains, int max_len,
                 signed char* state_out, int* acc_out, double* energy_out, int* counts_out, hipStream_t s) {
  const size_t lds = (size_t)max_len * (6 * sizeof(double) + 2 * sizeof(short) + 2);   // 54 KiB at 1024
  hipLaunchKernelGGL(dssp_kernel, dim3(n_chains), dim3(kThreads), lds, s, bb, flags, offsets, lens, max_len, state_out, acc_out,
                     energy_out, counts_out);
}

}  // namespace fdmi
