// The inverse of nerf.hip: backbone coordinates -> the nine canonical internal coordinates
// (foldingdiff/angles_and_coords.py:30-109 canonical_distances_and_dihedrals, the featurisation every CATH dataset
// and bin/partial_noise_reconstruct.py start from), and the backbone RMSD after optimal superposition that scores
// a reconstruction against the structure it came from.
//
// internal_coords_kernel: one lane per residue over a ragged batch of chains; fp64 arithmetic on the float32
// coordinates a PDB reader produces, rounded to float32 on output.  Column order and index shifts are the
// reference's (the ones nerf.hip consumes): N:CA:C at index i, and psi_i / omega_i / phi_{i+1}.
//
// superpose_rmsd_kernel: one wave per coordinate pair.  Centroids and the 3x3 covariance are reduced across the
// wave in fp64, the optimal rotation is the eigenvector of the largest eigenvalue of Horn's 4x4 quaternion matrix
// (cyclic Jacobi), and the RMSD is then summed over the superposed atoms directly.  Horn's closed form
// sqrt((Ga + Gb - 2 lambda) / N) would give the same value in exact arithmetic, but its cancellation leaves
// ~sqrt(eps) * radius of gyration (1e-7 A) for an identical pair; the direct sum stays at ~eps * radius.
//
// Both kernels take microseconds next to a sampling run: plain global loads, no LDS.
#include "fdmi_kernels.h"
#include "horn_fit.h"

namespace fdmi {
namespace {

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 load3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(dot(a, a)); }

__device__ __forceinline__ double dist(V3 a, V3 b) { return norm(sub(a, b)); }
// angle at b of a-b-c, in [0, pi]; atan2 keeps full precision near 0 and pi, where acos does not
__device__ __forceinline__ double angle(V3 a, V3 b, V3 c) {
  const V3 u = sub(a, b), v = sub(c, b);
  return atan2(norm(cross(u, v)), dot(u, v));
}
// IUPAC dihedral of a-b-c-d in (-pi, pi] (biotite.structure.dihedral's sign convention)
__device__ __forceinline__ double dihedral(V3 a, V3 b, V3 c, V3 d) {
  const V3 b1 = sub(b, a), b2 = sub(c, b), b3 = sub(d, c);
  const V3 n1 = cross(b1, b2), n2 = cross(b2, b3);
  return atan2(norm(b2) * dot(b1, n2), dot(n1, n2));
}

__global__ void __launch_bounds__(256) internal_coords_kernel(const float* __restrict__ xyz, const int* __restrict__ offsets,
                                       const int* __restrict__ lens, int n_chains, int n_res, float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_res) return;
  // chain of residue r: the last chain whose offset is <= r (offsets increase strictly: every length >= 1)
  int lo = 0, hi = n_chains - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int i = r - offsets[lo], n = lens[lo];
  const float* res = xyz + (size_t)r * 9;   // N, CA, C of residue r
  const V3 N = load3(res), CA = load3(res + 3), Cc = load3(res + 6);
  const float nan = __builtin_nanf("");
  float f[9];
  // phi: C of the previous residue; NaN for the first residue of a chain
  f[3] = i > 0 ? (float)dihedral(load3(res - 3), N, CA, Cc) : nan;
  if (i + 1 < n) {
    const V3 N1 = load3(res + 9), CA1 = load3(res + 12), C1 = load3(res + 15);
    f[0] = (float)dist(Cc, N1);               // 0C:1N
    f[1] = (float)dist(N1, CA1);              // N:CA of residue i+1
    f[2] = (float)dist(CA1, C1);              // CA:C of residue i+1
    f[4] = (float)dihedral(N, CA, Cc, N1);    // psi
    f[5] = (float)dihedral(CA, Cc, N1, CA1);  // omega
    f[6] = (float)angle(N1, CA1, C1);         // tau of residue i+1 (the reference's r = arange(3, ...))
    f[7] = (float)angle(CA, Cc, N1);          // CA:C:1N
    f[8] = (float)angle(Cc, N1, CA1);         // C:1N:1CA
  } else {
    // last residue: the reference pads distances with 0 and angles / dihedrals with NaN
    f[0] = 0.f; f[1] = 0.f; f[2] = 0.f;
    f[4] = nan; f[5] = nan; f[6] = nan; f[7] = nan; f[8] = nan;
  }
  float* o = out + (size_t)r * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = f[k];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return __shfl(v, 0, 64);   // lane 0's sum on every lane: all lanes then take the same (bitwise) decisions
}

__global__ void __launch_bounds__(64) superpose_rmsd_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                      const int* __restrict__ offsets, const int* __restrict__ lens,
                                      double* __restrict__ rmsd) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int n = lens[pair];
  const double* pa = a + (size_t)offsets[pair] * 3;
  const double* pb = b + (size_t)offsets[pair] * 3;
  // pass 1: centroids
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
  for (int k = lane; k < n; k += 64)
#pragma unroll
    for (int d = 0; d < 3; ++d) { sa[d] += pa[(size_t)k * 3 + d]; sb[d] += pb[(size_t)k * 3 + d]; }
  double ca[3], cb[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) { ca[d] = wave_sum(sa[d]) / n; cb[d] = wave_sum(sb[d]) / n; }
  // pass 2: covariance M[i][j] = sum (a - ca)_i (b - cb)_j of the centred coordinates
  double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int k = lane; k < n; k += 64) {
    double u[3], v[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { u[d] = pa[(size_t)k * 3 + d] - ca[d]; v[d] = pb[(size_t)k * 3 + d] - cb[d]; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[i][j] += u[i] * v[j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = wave_sum(M[i][j]);
  // Horn's quaternion matrix; its top eigenvector is the rotation taking a onto b
  double R[3][3];
  horn_rotation(M, R);
  // pass 3: sum |R (a - ca) - (b - cb)|^2
  double e = 0.0;
  for (int k = lane; k < n; k += 64) {
    double u[3], v[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { u[d] = pa[(size_t)k * 3 + d] - ca[d]; v[d] = pb[(size_t)k * 3 + d] - cb[d]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double r = R[i][0] * u[0] + R[i][1] * u[1] + R[i][2] * u[2] - v[i];
      e += r * r;
    }
  }
  e = wave_sum(e);
  if (lane == 0) rmsd[pair] = sqrt(e / n);
}

}  // namespace

void launch_internal_coords(const float* xyz, const int* offsets, const int* lens, int n_chains, int n_res, float* out,
                            hipStream_t s) {
  hipLaunchKernelGGL(internal_coords_kernel, dim3((n_res + 255) / 256), dim3(256), 0, s, xyz, offsets, lens, n_chains, n_res,
                     out);
}

void launch_superpose_rmsd(const double* a, const double* b, const int* offsets, const int* lens, int n_pairs, double* rmsd,
                           hipStream_t s) {
  hipLaunchKernelGGL(superpose_rmsd_kernel, dim3(n_pairs), dim3(64), 0, s, a, b, offsets, lens, rmsd);
}

}  // namespace fdmi
