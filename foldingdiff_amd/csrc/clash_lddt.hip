// Two structure scores that are integer counts over all atom pairs of a structure, every structure of a call in one launch:
//   clash_kernel  van der Waals clashes of a backbone -- count_clashes (foldingdiff/vdw_clashes.py:34-68);
//   lddt_kernel   lDDT of a model against a reference of the same residues (Mariani et al. 2013) -- what
//                 lddt_sampled_folded (foldingdiff/lddt.py:59-100) gets from OpenStructure, one container per pair.
// The rules restated here (and in tests/clash_lddt_reference.py, DESIGN.md "Clash counts and lDDT"):
//   clashes: atoms of a chain in file order, 3i = N (r = 1.55), 3i + 1 = CA, 3i + 2 = C (r = 1.7).  a and b clash iff
//     |a - b| >= 2 and d(a, b) <= alpha * (r_a + r_b); the count of a chain = its atoms that clash with at least one other.
//   lDDT: A atoms per residue, residue i of the model corresponds to residue i of the reference.  An unordered pair of
//     atoms of different residues is included iff d_ref < radius; an included pair is conserved at threshold tau iff
//     |d_model - d_ref| < tau.  total = included pairs, conserved = conserved pairs summed over the thresholds; per
//     residue the same two numbers over the included pairs with an atom in it.
// Coordinates arrive as float32 (what a PDB file holds) and are widened to fp64 before the first subtraction; a
// distance is sqrt(dx dx + dy dy + dz dz) in fp64.  Every result is an integer.
//
// Both kernels: one workgroup of 256 threads per structure.  The outer loop walks the structure in blocks of up to 256
// atoms, one atom per thread, its coordinates and counters in registers; the inner loop walks the whole structure again
// in tiles of 1024 atoms staged in LDS as float32 (12 KiB per structure), every lane reading the same atom (a
// broadcast).  So there is no length cap from LDS, no atomic and no floating-point sum: a thread writes its own atom's
// integers, and the totals of a structure are an integer sum over the workgroup, exact in any order.
// lddt_kernel's blocks hold whole residues (256 / A of them), so that the A per-atom counters of a residue meet in one
// block and are summed through LDS.  Every loop that holds a barrier is bounded by workgroup-uniform values.
#include "fdmi_kernels.h"

namespace fdmi {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;   // atoms per LDS tile

// the first min(kTile, n - t0) atoms from t0 on of a structure (x = its first coordinate) into `tile`
__device__ __forceinline__ void stage_tile(const float* __restrict__ x, int t0, int n, float* __restrict__ tile) {
  const int m = min(kTile, n - t0) * 3;
  const float* __restrict__ src = x + (size_t)t0 * 3;
  for (int k = threadIdx.x; k < m; k += kThreads) tile[k] = src[k];
}

__device__ __forceinline__ double dist(double ax, double ay, double az, const float* __restrict__ b) {
  const double dx = ax - (double)b[0], dy = ay - (double)b[1], dz = az - (double)b[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// sum over the workgroup; every thread calls it, thread 0 holds the result
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // red may still be read from the call before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long total = 0;
  for (int w = 0; w < kThreads / 64; ++w) total += red[w];
  return total;
}

__global__ void __launch_bounds__(kThreads) clash_kernel(const float* __restrict__ xyz, const int* __restrict__ offsets,
                                                         const int* __restrict__ lens, double alpha,
                                                         int* __restrict__ counts_out, unsigned char* __restrict__ flags_out) {
  __shared__ float tile[kTile * 3];
  __shared__ long long red[kThreads / 64];
  const int chain = blockIdx.x, tid = threadIdx.x, n = lens[chain] * 3;   // atoms
  const size_t atom0 = (size_t)offsets[chain] * 3;
  const float* __restrict__ x = xyz + atom0 * 3;
  long long clashing = 0;
  for (int a0 = 0; a0 < n; a0 += kThreads) {
    const int a = a0 + tid;
    const bool live = a < n;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (live) {
      ax = (double)x[(size_t)a * 3];
      ay = (double)x[(size_t)a * 3 + 1];
      az = (double)x[(size_t)a * 3 + 2];
    }
    const double ra = a % 3 == 0 ? 1.55 : 1.7;
    const double lim_n = alpha * (ra + 1.55), lim_c = alpha * (ra + 1.7);   // against an N; against a CA or C
    bool hit = false;
    for (int t0 = 0; t0 < n; t0 += kTile) {
      __syncthreads();   // the tile before is read to its end
      stage_tile(x, t0, n, tile);
      __syncthreads();
      if (live) {
        const int m = min(kTile, n - t0);
        for (int j = 0; j < m; ++j) {
          const int b = t0 + j;
          const double d = dist(ax, ay, az, tile + j * 3);
          const bool apart = b - a >= 2 || a - b >= 2;
          hit |= apart && d <= (b % 3 == 0 ? lim_n : lim_c);
        }
      }
    }
    if (live) {
      if (flags_out) flags_out[atom0 + a] = hit ? 1 : 0;
      clashing += hit ? 1 : 0;
    }
  }
  const long long total = block_sum(clashing, red);
  if (tid == 0) counts_out[chain] = (int)total;
}

// thr: the thresholds, 0 in the unused places (|d_model - d_ref| < 0 never holds)
__global__ void __launch_bounds__(kThreads) lddt_kernel(const float* __restrict__ model, const float* __restrict__ ref,
                                                        const int* __restrict__ offsets, const int* __restrict__ lens, int A,
                                                        double radius, LddtThresholds thr, long long* __restrict__ counts_out,
                                                        int* __restrict__ res_counts_out) {
  __shared__ float tile_m[kTile * 3];
  __shared__ float tile_r[kTile * 3];
  __shared__ int atom_total[kThreads];
  __shared__ int atom_cons[kThreads];
  __shared__ long long red[kThreads / 64];
  const int pair = blockIdx.x, tid = threadIdx.x, n_res = lens[pair], n = n_res * A;
  const size_t res0 = (size_t)offsets[pair];
  const float* __restrict__ xm = model + res0 * A * 3;
  const float* __restrict__ xr = ref + res0 * A * 3;
  const int block_res = kThreads / A;   // residues per block; threads block_res * A .. 255 idle
  long long sum_total = 0, sum_cons = 0;
  for (int r0 = 0; r0 < n_res; r0 += block_res) {
    const int a = r0 * A + tid;
    const bool live = tid < block_res * A && a < n;
    const int own = a / A * A;   // the first atom of a's residue
    double mx = 0.0, my = 0.0, mz = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
    if (live) {
      mx = (double)xm[(size_t)a * 3];
      my = (double)xm[(size_t)a * 3 + 1];
      mz = (double)xm[(size_t)a * 3 + 2];
      rx = (double)xr[(size_t)a * 3];
      ry = (double)xr[(size_t)a * 3 + 1];
      rz = (double)xr[(size_t)a * 3 + 2];
    }
    int total = 0, cons = 0;   // ordered pairs of this atom: at most 65535 and 8 * 65535
    for (int t0 = 0; t0 < n; t0 += kTile) {
      __syncthreads();   // the tiles before are read to their end
      stage_tile(xm, t0, n, tile_m);
      stage_tile(xr, t0, n, tile_r);
      __syncthreads();
      if (live) {
        const int m = min(kTile, n - t0);
        for (int j = 0; j < m; ++j) {
          const double d_ref = dist(rx, ry, rz, tile_r + j * 3);
          const bool in = (unsigned)(t0 + j - own) >= (unsigned)A && d_ref < radius;   // another residue, within the radius
          const double delta = fabs(dist(mx, my, mz, tile_m + j * 3) - d_ref);
          int kept = 0;
#pragma unroll
          for (int k = 0; k < kLddtMaxThresholds; ++k) kept += delta < thr.t[k] ? 1 : 0;
          total += in ? 1 : 0;
          cons += in ? kept : 0;
        }
      }
    }
    sum_total += total;
    sum_cons += cons;
    if (res_counts_out) {   // workgroup-uniform
      atom_total[tid] = total;
      atom_cons[tid] = cons;
      __syncthreads();
      if (tid < block_res && r0 + tid < n_res) {
        int t = 0, c = 0;
        for (int k = 0; k < A; ++k) {
          t += atom_total[tid * A + k];
          c += atom_cons[tid * A + k];
        }
        res_counts_out[(res0 + r0 + tid) * 2] = c;
        res_counts_out[(res0 + r0 + tid) * 2 + 1] = t;
      }
      // the next block writes atom_total / atom_cons only after the barriers of its tile loop
    }
  }
  // every unordered pair was counted from both of its atoms
  const long long c = block_sum(sum_cons, red);
  const long long t = block_sum(sum_total, red);
  if (tid == 0) {
    counts_out[(size_t)pair * 2] = c / 2;
    counts_out[(size_t)pair * 2 + 1] = t / 2;
  }
}

}  // namespace

void launch_backbone_clashes(const float* xyz, const int* offsets, const int* lens, int n_chains, double alpha,
                             int* counts_out, unsigned char* flags_out, hipStream_t s) {
  hipLaunchKernelGGL(clash_kernel, dim3(n_chains), dim3(kThreads), 0, s, xyz, offsets, lens, alpha, counts_out, flags_out);
}

void launch_lddt(const float* model, const float* ref, const int* offsets, const int* lens, int n_pairs, int atoms_per_res,
                 double radius, const LddtThresholds& thr, long long* counts_out, int* res_counts_out, hipStream_t s) {
  hipLaunchKernelGGL(lddt_kernel, dim3(n_pairs), dim3(kThreads), 0, s, model, ref, offsets, lens, atoms_per_res, radius, thr,
                     counts_out, res_counts_out);
}

}  // namespace fdmi
