// Superposition restraints (fd_template_energy, fd_scaffold_guide_step_tpl, fd_sample_guided_inpaint_tpl; include/fdmi.h,
// DESIGN.md 6z): the squared deviation of chosen atoms from a template after the optimal fit by a PROPER rotation, and its
// gradient on the coordinates.  One 256-lane workgroup per chain as in nerf_vjp.hip, fp64, no floating-point atomics, no
// scratch; every sum in an order fixed by (entry count, lane) through block_sum.h.
//
// template_kernel.  Three lane-strided passes over the chain's entries k = offsets[b] .. offsets[b + 1] - 1 (atom a_k, target
// m_k, weight w_k): (1) the seven sums W, W cp, W cm; (2) the nine sums of the CENTRED covariance M[i][j] = sum w (m - cm)_i
// (p - cp)_j -- a second pass, not sum-of-products minus product-of-sums, which cancels for a template far from the origin;
// (3) the explicit residuals r = (p - cp) - R (m - cm), E = sum w |r|^2 and 2 w r ADDED to dcoords.  Between (2) and (3) lane 0
// runs horn_rotation (horn_fit.h) and the nine entries of R go to every lane through LDS.  E never comes from the eigenvalue:
// at a perfect fit that form cancels.  The host has checked that a chain's atoms are strictly increasing, so every named atom
// belongs to exactly one entry and its read-modify-write to the one lane that owns the entry.  A chain without entries gets
// E = 0, rmsd = 0, the identity transform, and nothing on dcoords.
#include "block_sum.h"
#include "fdmi_kernels.h"
#include "horn_fit.h"

namespace fdmi {

namespace {

__global__ __launch_bounds__(kChainThreads) void template_kernel(const double* __restrict__ coords, int L, TemplateFit t,
                                                                 double* __restrict__ energy, double* __restrict__ rmsd,
                                                                 double* __restrict__ transform, double* __restrict__ dcoords) {
  __shared__ double slot[kChainWaves];
  __shared__ double rot[9];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int k0 = t.offsets[b], k1 = t.offsets[b + 1];
  if (k1 <= k0) {  // (the whole workgroup leaves together, before any barrier)
    if (tid == 0) {
      energy[b] = 0.0;
      rmsd[b] = 0.0;
      if (transform)
        for (int i = 0; i < 12; ++i) transform[(size_t)b * 12 + i] = i == 0 || i == 4 || i == 8 ? 1.0 : 0.0;
    }
    return;
  }
  const double* __restrict__ x = coords + (size_t)b * 3 * L * 3;
  // 1. the weight and the two weighted centroids
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = k0 + tid; k < k1; k += kChainThreads) {
    const double w = t.w[k];
    const size_t a = (size_t)t.atom[k] * 3, m = (size_t)k * 3;
    s[0] += w;
    s[1] += w * x[a]; s[2] += w * x[a + 1]; s[3] += w * x[a + 2];
    s[4] += w * t.xyz[m]; s[5] += w * t.xyz[m + 1]; s[6] += w * t.xyz[m + 2];
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) s[i] = block_sum(s[i], slot);
  const double W = s[0];
  const double cpx = s[1] / W, cpy = s[2] / W, cpz = s[3] / W, cmx = s[4] / W, cmy = s[5] / W, cmz = s[6] / W;
  // 2. the centred covariance
  double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int k = k0 + tid; k < k1; k += kChainThreads) {
    const double w = t.w[k];
    const size_t a = (size_t)t.atom[k] * 3, m = (size_t)k * 3;
    const double px = x[a] - cpx, py = x[a + 1] - cpy, pz = x[a + 2] - cpz;
    const double ux = w * (t.xyz[m] - cmx), uy = w * (t.xyz[m + 1] - cmy), uz = w * (t.xyz[m + 2] - cmz);
    M[0][0] += ux * px; M[0][1] += ux * py; M[0][2] += ux * pz;
    M[1][0] += uy * px; M[1][1] += uy * py; M[1][2] += uy * pz;
    M[2][0] += uz * px; M[2][1] += uz * py; M[2][2] += uz * pz;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = block_sum(M[i][j], slot);
  if (tid == 0) {
    double R[3][3];
    horn_rotation(M, R);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) rot[i * 3 + j] = R[i][j];
  }
  __syncthreads();
  const double r00 = rot[0], r01 = rot[1], r02 = rot[2], r10 = rot[3], r11 = rot[4], r12 = rot[5], r20 = rot[6], r21 = rot[7], r22 = rot[8];
  // 3. the residuals at the optimal fit: the energy, and twice the weighted residual on each named atom
  double* __restrict__ g = dcoords ? dcoords + (size_t)b * 3 * L * 3 : nullptr;
  double e = 0.0;
  for (int k = k0 + tid; k < k1; k += kChainThreads) {
    const double w = t.w[k];
    const size_t a = (size_t)t.atom[k] * 3, m = (size_t)k * 3;
    const double ux = t.xyz[m] - cmx, uy = t.xyz[m + 1] - cmy, uz = t.xyz[m + 2] - cmz;
    const double rx = (x[a] - cpx) - (r00 * ux + r01 * uy + r02 * uz);
    const double ry = (x[a + 1] - cpy) - (r10 * ux + r11 * uy + r12 * uz);
    const double rz = (x[a + 2] - cpz) - (r20 * ux + r21 * uy + r22 * uz);
    e += w * (rx * rx + ry * ry + rz * rz);
    if (g) {
      g[a] += 2.0 * w * rx;
      g[a + 1] += 2.0 * w * ry;
      g[a + 2] += 2.0 * w * rz;
    }
  }
  const double E = block_sum(e, slot);
  if (tid == 0) {
    energy[b] = E;
    rmsd[b] = sqrt(E / W);
    if (transform) {
      double* T = transform + (size_t)b * 12;
      T[0] = r00; T[1] = r01; T[2] = r02; T[3] = r10; T[4] = r11; T[5] = r12; T[6] = r20; T[7] = r21; T[8] = r22;
      T[9] = cpx - (r00 * cmx + r01 * cmy + r02 * cmz);
      T[10] = cpy - (r10 * cmx + r11 * cmy + r12 * cmz);
      T[11] = cpz - (r20 * cmx + r21 * cmy + r22 * cmz);
    }
  }
}

}  // namespace

void launch_template_energy(const double* coords, int B, int L, const TemplateFit& t, double* energy, double* rmsd,
                            double* transform, double* dcoords, hipStream_t s) {
  hipLaunchKernelGGL(template_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, s, coords, L, t, energy, rmsd, transform, dcoords);
}

}  // namespace fdmi
