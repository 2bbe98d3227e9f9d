// Evaluating a fixed checkpoint: the forward noising q(x_t | x_0) and the denoising loss, as two HBM-trivial row kernels.
//   q_sample     NoisedAnglesDataset.__getitem__'s noising statement (foldingdiff/datasets.py:861-871)
//   loss_terms   the per-feature terms of BertForDiffusion._get_loss_terms (foldingdiff/modelling.py:553-604):
//                losses.radian_smooth_l1_loss (losses.py:29-55) for angular features, F.smooth_l1_loss for the others,
//                over the unmasked positions of each sequence
// Every float32 operation is an explicit __f*_rn (no FMA contraction): the per-position results carry the bits of the
// reference's CPU statements.  The sums are fp64 in a fixed order, so they do not depend on the run or on where a
// sequence sits in the batch; the means over the batch are the host's business (they need the count of all positions).
#include "fdmi_kernels.h"
#include "smooth_l1_term.h"
#include "wrap_pi.h"

namespace fdmi {

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ eps,
                                                       const float* __restrict__ keep, const float* __restrict__ spread,
                                                       float* __restrict__ x_t, long long n, int per_seq, int F,
                                                       unsigned angle_mask) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per_seq), f = (int)(i % F);
    // sqrt_alphas_cumprod_t * vals + sqrt_one_minus_alphas_cumprod_t * noise: two rounded products, one rounded sum
    float v = __fadd_rn(__fmul_rn(keep[b], x0[i]), __fmul_rn(spread[b], eps[i]));
    if ((angle_mask >> f) & 1u) v = wrap_pi(v);
    x_t[i] = v;
  }
}

void launch_q_sample(const float* x0, const float* eps, const float* keep, const float* spread, float* x_t, int B, int L, int F,
                     unsigned angle_mask, hipStream_t s) {
  const long long n = (long long)B * L * F;
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x0, eps, keep, spread, x_t, n, L * F, F,
                     angle_mask);
}

// One workgroup per sequence.  Thread tid owns feature tid % F and the positions tid / F, tid / F + P, ... (P = 256 / F
// threads per feature; the 256 - P F threads left over idle), so consecutive threads touch consecutive floats.  Its fp64
// partial sum goes to LDS, and the P partials of a feature are folded by a fixed binary tree.
__global__ __launch_bounds__(256) void loss_terms_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const int* __restrict__ lens, int L, int F, unsigned angle_mask,
                                                         float beta_ang, float beta_lin, double* __restrict__ sums,
                                                         float* __restrict__ terms) {
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = 256 / F, f = tid % F, p = tid / F;
  const bool active = p < P;
  const int len = min(max(lens[b], 0), L);
  const bool angular = (angle_mask >> f) & 1u;
  const float beta = angular ? beta_ang : beta_lin, half_beta = __fmul_rn(0.5f, beta);
  const size_t base = (size_t)b * L * F;
  double acc = 0.0;
  if (active) {
    for (int l = p; l < L; l += P) {
      const size_t o = base + (size_t)l * F + f;
      float term = 0.f;
      if (l < len) {
        term = smooth_l1_term(pred[o], target[o], angular, beta, half_beta);
        acc += (double)term;
      }
      if (terms) terms[o] = term;
    }
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {  // (P <= 256: partner p + s, when there is one)
    if (active && p < s && p + s < P) part[tid] += part[tid + s * F];
    __syncthreads();
  }
  if (tid < F) sums[(size_t)b * F + tid] = part[tid];
}

void launch_loss_terms(const float* pred, const float* target, const int* lens, int B, int L, int F, unsigned angle_mask,
                       float beta_ang, float beta_lin, double* sums, float* terms, hipStream_t s) {
  hipLaunchKernelGGL(loss_terms_kernel, dim3((unsigned)B), dim3(256), 0, s, pred, target, lens, L, F, angle_mask, beta_ang,
                     beta_lin, sums, terms);
}

}  // namespace fdmi
