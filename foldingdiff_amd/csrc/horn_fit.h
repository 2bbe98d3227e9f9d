// Optimal rotation from a 3x3 covariance by Horn's quaternion method, fp64, one lane: shared by superpose_rmsd_kernel
// (internal_coords.hip) and the TM-score search (tm_score.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

// Largest-eigenvalue eigenvector of the symmetric 4x4 A (cyclic Jacobi; every index is a compile-time constant).
__device__ __forceinline__ void top_eigenvector(double A[4][4], double q[4]) {
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      diag += A[p][p] * A[p][p];
#pragma unroll
      for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
    }
    if (!(off > 1e-34 * diag)) break;   // |off-diagonal| below 1e-17 of the diagonal (also ends an all-zero matrix)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apr = A[p][r];
        if (apr == 0.0) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * apr);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // A <- A J
          const double akp = A[k][p], akr = A[k][r];
          A[k][p] = c * akp - s * akr;
          A[k][r] = s * akp + c * akr;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // A <- J^T A
          const double apk = A[p][k], ark = A[r][k];
          A[p][k] = c * apk - s * ark;
          A[r][k] = s * apk + c * ark;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // V <- V J
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - s * vkr;
          V[k][r] = s * vkp + c * vkr;
        }
      }
    }
  }
  int best = 0;
  double lmax = A[0][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > lmax) { lmax = A[k][k]; best = k; }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
}

// The proper rotation R minimising sum |R u - v|^2, from the covariance M[i][j] = sum u_i v_j of centred coordinates:
// the top eigenvector of Horn's quaternion matrix.  M = 0 (one point) gives the identity.
__device__ __forceinline__ void horn_rotation(const double M[3][3], double R[3][3]) {
  const double Sxx = M[0][0], Sxy = M[0][1], Sxz = M[0][2], Syx = M[1][0], Syy = M[1][1], Syz = M[1][2],
               Szx = M[2][0], Szy = M[2][1], Szz = M[2][2];
  double H[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double q[4];
  top_eigenvector(H, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.0 * (x * y - w * z);         R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);         R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);         R[2][1] = 2.0 * (y * z + w * x);         R[2][2] = w * w - x * x - y * y + z * z;
}

}  // namespace fdmi
