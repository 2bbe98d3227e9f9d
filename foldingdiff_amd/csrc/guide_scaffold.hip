// Restraint guidance combined with replacement (fd_scaffold_guide_step, fd_sample_guided_inpaint; include/fdmi.h):
// the two kernels of the scaffold-guide statement that are its own, and the statement's launches in their order.  Both kernels:
// one 256-lane workgroup per chain as in nerf_vjp.hip, `fixed` read as bytes, no floating-point atomics, no scratch.
//
// scaffold_shift_kernel.  p[o] = fixed[o] ? known[o] : x0[o], then steer_shift_kernel's statement on p (guide_element.h), in one
// pass; a position at or beyond the chain's length gets 0.  x0[o] is not read where fixed[o]: update_element writes no x0 there.
//
// scaffold_update_kernel.  guide_update_kernel (nerf_vjp.hip) with a mask: G[o] <- 0 where fixed[o] (in place), |G_b| over the
// rows below the length with the same lane-strided squares and the same tree (block_sum.h), the clip factor, then the free
// elements take guide_update_kernel's three lines (guide_element.h) -- with `fixed` all zero the two kernels give the same
// bits.  A fixed element keeps its bits and neither reads nor draws a z.
//
// launch_scaffold_energy.  shift, launch_nerf_scan, launch_restraint_energy, launch_soft_clash (only where w > 0),
// launch_template_energy (template_fit.hip; only where a chain has a template entry), launch_symmetry_guide (symmetry.hip; only
// where a chain has a symmetry order above 1) and, where a gradient is asked for,
// launch_nerf_vjp on the shifted rows: the restraints before the clashes, relax.hip's order, so that with nothing fixed and no
// template G is fd_relax_energy's gradient bit for bit.
#include "block_sum.h"
#include "fdmi_kernels.h"
#include "guide_element.h"

namespace fdmi {

namespace {

__global__ __launch_bounds__(kChainThreads) void scaffold_shift_kernel(const float* __restrict__ x0, const float* __restrict__ known,
                                                                       const unsigned char* __restrict__ fixed,
                                                                       const int* __restrict__ lens, int L, int F, SteerOffset off,
                                                                       unsigned angle_mask, float* __restrict__ ang) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ne = lens[b] * F, row = L * F;
  const size_t base = (size_t)b * row;
  for (int e = tid; e < row; e += kChainThreads) {
    const size_t o = base + e;
    float v = 0.f;
    if (e < ne) {
      if (fixed[o]) v = known[o];
      else v = x0[o];
      v = steer_shift_value(v, off, angle_mask, e % F);
    }
    ang[o] = v;
  }
}

__global__ __launch_bounds__(kChainThreads) void scaffold_update_kernel(float* __restrict__ x, double* __restrict__ G,
                                                                        const unsigned char* __restrict__ fixed,
                                                                        const int* __restrict__ lens, int L, int F, unsigned angle_mask,
                                                                        float c, double max_norm, float s, const float* __restrict__ z,
                                                                        unsigned long long seed, int t, long long seq_offset,
                                                                        double* __restrict__ gnorm) {
  __shared__ double slot[kChainWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ne = lens[b] * F;
  const size_t base = (size_t)b * L * F;
  double ss = 0.0;
  for (int e = tid; e < ne; e += kChainThreads) {
    double g = G[base + e];
    if (fixed[base + e]) {
      g = 0.0;
      G[base + e] = 0.0;
    }
    ss += g * g;
  }
  const double norm = sqrt(block_sum(ss, slot));
  const double ck = (double)c * (norm > max_norm ? max_norm / norm : 1.0);
  if (tid == 0) gnorm[b] = norm;
  for (int e = tid; e < ne; e += kChainThreads) {  // (a lane reads the entries of G it wrote itself)
    const size_t o = base + e;
    if (fixed[o]) continue;
    x[o] = guide_move(x[o], c, ck, G[o], s, z, o, seed, t, seq_offset + b, e / F, e % F, angle_mask);
  }
}

}  // namespace

void launch_scaffold_shift(const float* x0, const float* known, const unsigned char* fixed, const int* lens, int B, int L, int F,
                           const SteerOffset& off, unsigned angle_mask, float* ang, hipStream_t s) {
  hipLaunchKernelGGL(scaffold_shift_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, s, x0, known, fixed, lens, L, F, off, angle_mask,
                     ang);
}

void launch_scaffold_update(float* x, double* G, const unsigned char* fixed, const int* lens, int B, int L, int F, unsigned angle_mask,
                            float c, double max_norm, float s, const float* z, unsigned long long seed, int t, long long seq_offset,
                            double* gnorm, hipStream_t st) {
  hipLaunchKernelGGL(scaffold_update_kernel, dim3((unsigned)B), dim3(kChainThreads), 0, st, x, G, fixed, lens, L, F, angle_mask, c,
                     max_norm, s, z, seed, t, seq_offset, gnorm);
}

void launch_scaffold_energy(const float* x0, const float* known, const unsigned char* fixed, const int* lens, int B, int L, int F,
                            const SteerOffset& off, unsigned angle_mask, const NerfFeatures& fx, const Restraints& rs,
                            const SoftClash& clash, const TemplateFit* tpl, const ScaffoldWork& wk, double* G, hipStream_t s,
                            const SymGuide* sym) {
  const bool clashes = clash.w > 0.0;
  launch_scaffold_shift(x0, known, fixed, lens, B, L, F, off, angle_mask, wk.ang, s);
  launch_nerf_scan(wk.ang, lens, B, L, F, fx, 0, wk.coords, s);
  launch_restraint_energy(wk.coords, lens, B, L, rs, wk.e_rst, wk.max_violation, G || clashes ? wk.gc : nullptr, s);
  if (clashes) launch_soft_clash(wk.coords, lens, B, L, clash.alpha, clash.margin, clash.w, wk.e_clash, wk.gc, s);
  if (tpl) launch_template_energy(wk.coords, B, L, *tpl, wk.e_tpl, wk.rmsd_tpl, nullptr, G ? wk.gc : nullptr, s);
  if (sym) launch_symmetry_guide(*sym, G ? wk.gc : nullptr, s);
  if (G) launch_nerf_vjp(wk.coords, lens, B, L, F, fx, 0, wk.gc, wk.ang, G, s);
}

}  // namespace fdmi
