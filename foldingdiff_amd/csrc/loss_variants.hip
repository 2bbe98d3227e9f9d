// The rest of BertForDiffusion._get_loss_terms (foldingdiff/modelling.py:553-679), as siblings of loss.hip's kernels:
//   loss_terms_ex   loss_terms_kernel with a loss kind -- 0: the smooth-L1 pair, 1: "l1" = losses.radian_l1_loss
//                   (losses.py:12-26) for angular features and F.l1_loss for the others -- and, optionally, the turn
//                   counts of the circle penalty (losses.py:57-61): sum over the unmasked positions of
//                   trunc(|pred| / pi) for angular features
//   pairwise_dist   the pairwise-distance term (modelling.py:616-677, losses.py:66-149, nerf.py:207-292): the denoised
//                   angles from the predicted noise, the NeRF chains of the clean and of the denoised angles, and the
//                   weighted squared differences of all CA-CA distances of a sequence
// Same rules as loss.hip: every float32 operation is an explicit __f*_rn in the reference's order, the sums are fp64 in
// a fixed order (no atomics: the same bits from run to run and wherever a sequence sits in the batch), and the means
// over the batch are the host's business.
#include "fdmi_kernels.h"
#include "nerf_place.h"
#include "smooth_l1_term.h"
#include "wrap_pi.h"

namespace fdmi {

// torch.remainder(v, f32(2 pi)) on a float32 tensor: fmod, then the divisor's sign
__device__ __forceinline__ float rem_two_pi(float v) {
  const float TWO_PI_F = 6.28318548202514648f;
  float m = fmodf(v, TWO_PI_F);
  if (m != 0.f && m < 0.f) m = __fadd_rn(m, TWO_PI_F);
  return m;
}

// radian_l1_loss: target % 2 pi, input % 2 pi, d = target - input, d = (d + pi) % 2 pi - pi, |d|;  F.l1_loss: |target - pred|
__device__ __forceinline__ float l1_term(float pred, float target, bool angular) {
  if (!angular) return fabsf(__fsub_rn(target, pred));
  return fabsf(wrap_pi(__fsub_rn(rem_two_pi(target), rem_two_pi(pred))));
}

// torch.div(torch.abs(pred), pi, rounding_mode="trunc"): a float32 division by f32(pi), truncated
__device__ __forceinline__ long long turns_of(float pred) {
  const float PI_F = 3.14159274101257324f;
  return (long long)truncf(__fdiv_rn(fabsf(pred), PI_F));
}

// loss_terms_kernel's mapping, partials and tree (loss.hip): one workgroup per sequence, thread tid owns feature
// tid % F and the positions tid / F, tid / F + P, ... (P = 256 / F).  The turn counts are integers: exact in any order.
__global__ __launch_bounds__(256) void loss_terms_ex_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            const int* __restrict__ lens, int L, int F, unsigned angle_mask,
                                                            int kind, float beta_ang, float beta_lin,
                                                            double* __restrict__ sums, float* __restrict__ terms,
                                                            long long* __restrict__ turns) {
  __shared__ double part[256];
  __shared__ long long tpart[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = 256 / F, f = tid % F, p = tid / F;
  const bool active = p < P;
  const int len = min(max(lens[b], 0), L);
  const bool angular = (angle_mask >> f) & 1u;
  const float beta = angular ? beta_ang : beta_lin, half_beta = __fmul_rn(0.5f, beta);
  const size_t base = (size_t)b * L * F;
  double acc = 0.0;
  long long nturn = 0;
  if (active) {
    for (int l = p; l < L; l += P) {
      const size_t o = base + (size_t)l * F + f;
      float term = 0.f;
      if (l < len) {
        const float pr = pred[o];
        term = kind == 1 ? l1_term(pr, target[o], angular) : smooth_l1_term(pr, target[o], angular, beta, half_beta);
        acc += (double)term;
        if (turns && angular) nturn += turns_of(pr);
      }
      if (terms) terms[o] = term;
    }
  }
  part[tid] = acc;
  tpart[tid] = nturn;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {  // (P <= 256: partner p + s, when there is one)
    if (active && p < s && p + s < P) {
      part[tid] += part[tid + s * F];
      tpart[tid] += tpart[tid + s * F];
    }
    __syncthreads();
  }
  if (tid < F) {
    sums[(size_t)b * F + tid] = part[tid];
    if (turns) turns[(size_t)b * F + tid] = tpart[tid];
  }
}

void launch_loss_terms_ex(const float* pred, const float* target, const int* lens, int B, int L, int F, unsigned angle_mask,
                          int kind, float beta_ang, float beta_lin, double* sums, float* terms, long long* turns,
                          hipStream_t s) {
  hipLaunchKernelGGL(loss_terms_ex_kernel, dim3((unsigned)B), dim3(256), 0, s, pred, target, lens, L, F, angle_mask, kind,
                     beta_ang, beta_lin, sums, terms, turns);
}

// One workgroup per sequence, L <= kPairwiseMaxLen.
// Phase 1: lanes 0 and 1 of the first wave run the two chains in lock-step (the same trip count: no divergence) --
//   lane 0 on the clean angles, lane 1 on denoised = (corrupted - spread_b * pred) / keep_b, formed on the fly in float32
//   in that order and not wrapped.  place() with the angle a feature and a default length is nerf_build_batch's
//   statement: (-bl cos th, bl cos tau sin th, bl sin tau sin th) in float32, widened, in float64 frames that start at
//   the float64 seed atoms.  The index quirk is nerf_kernel's: the new C takes tau[i] and phi[i + 1].  The CA atoms (rows
//   1, 4, 7, ... of the chain) go to LDS.
// Phase 2: thread tid takes the pairs k = tid, tid + 256, ... of the len (len - 1) / 2, in F.pdist's order
//   (0,1), (0,2), ..., (1,2), ...: both distances in fp64, STORED AS float32 (the reference copies them into a float32
//   tensor), t = coef_b * (d_in - d_tgt)^2 in float32, summed in fp64; the 256 partials are folded by a fixed binary tree.
__global__ __launch_bounds__(256) void pairwise_dist_kernel(const float* __restrict__ angles, const float* __restrict__ corrupted,
                                                            const float* __restrict__ pred, const float* __restrict__ keep,
                                                            const float* __restrict__ spread, const float* __restrict__ coef,
                                                            const int* __restrict__ lens, int L, int F, PairwiseFeatures fx,
                                                            double* __restrict__ sums, long long* __restrict__ pairs,
                                                            double* __restrict__ ca_out) {
  __shared__ double ca[2][kPairwiseMaxLen][3];
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 1), min(L, kPairwiseMaxLen));
  const size_t base = (size_t)b * L * F;
  if (tid < 2) {
    const float kp = keep[b], sp = spread[b];
    auto val = [&](int i, int col) -> float {
      const size_t o = base + (size_t)i * F + col;
      return tid == 0 ? angles[o] : __fdiv_rn(__fsub_rn(corrupted[o], __fmul_rn(sp, pred[o])), kp);
    };
    D3 p0 = {17.047, 14.099, 3.625}, p1 = {16.967, 12.784, 4.338}, p2 = {15.685, 12.755, 5.133};  // nerf.py:22-24
    ca[tid][0][0] = p1.x; ca[tid][0][1] = p1.y; ca[tid][0][2] = p1.z;
    for (int i = 0; i + 1 < len; ++i) {
      // next N: C->N bond 1.34, CA:C:1N angle, psi_i;  next CA: N->CA bond 1.46, C:1N:1CA angle, omega_i;
      // next C: CA->C bond 1.54, tau AT INDEX i, phi_{i+1}
      const D3 n = place(p0, p1, p2, true, val(i, fx.ang_ca_c_n), 0.0, false, 0.f, 1.34, val(i, fx.psi));
      const D3 a = place(p1, p2, n, true, val(i, fx.ang_c_n_ca), 0.0, false, 0.f, 1.46, val(i, fx.omega));
      const D3 c = place(p2, n, a, true, val(i, fx.tau), 0.0, false, 0.f, 1.54, val(i + 1, fx.phi));
      ca[tid][i + 1][0] = a.x; ca[tid][i + 1][1] = a.y; ca[tid][i + 1][2] = a.z;
      p0 = n; p1 = a; p2 = c;
    }
  }
  __syncthreads();
  if (ca_out) {  // [B][2][L][3]: the clean trace, then the denoised one; zeros past the length
    double* o = ca_out + (size_t)b * 2 * L * 3;
    for (int e = tid; e < 2 * L * 3; e += 256) {
      const int chain = e / (L * 3), r = e % (L * 3), i = r / 3;
      o[e] = i < len ? ca[chain][i][r % 3] : 0.0;
    }
  }
  const int npair = len * (len - 1) / 2;
  const float w = coef ? coef[b] : 1.f;
  auto row_start = [&](int i) { return i * (2 * len - i - 1) / 2; };  // pairs (i', .) with i' < i
  double acc = 0.0;
  for (int k = tid; k < npair; k += 256) {
    const double q = 2.0 * len - 1.0;
    int i = (int)((q - sqrt(q * q - 8.0 * k)) * 0.5);
    i = min(max(i, 0), len - 2);
    while (i + 1 <= len - 2 && row_start(i + 1) <= k) ++i;
    while (i > 0 && row_start(i) > k) --i;
    const int j = k - row_start(i) + i + 1;
    auto dist = [&](int chain) {
      const double dx = ca[chain][i][0] - ca[chain][j][0], dy = ca[chain][i][1] - ca[chain][j][1],
                   dz = ca[chain][i][2] - ca[chain][j][2];
      return (float)sqrt(dx * dx + dy * dy + dz * dz);
    };
    const float d = __fsub_rn(dist(1), dist(0));   // input (denoised) - target (clean)
    acc += (double)__fmul_rn(w, __fmul_rn(d, d));
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    sums[b] = part[0];
    pairs[b] = npair;
  }
}

void launch_pairwise_dist(const float* angles, const float* corrupted, const float* pred, const float* keep, const float* spread,
                          const float* coef, const int* lens, int B, int L, int F, const PairwiseFeatures& fx, double* sums,
                          long long* pairs, double* ca_out, hipStream_t s) {
  hipLaunchKernelGGL(pairwise_dist_kernel, dim3((unsigned)B), dim3(256), 0, s, angles, corrupted, pred, keep, spread, coef, lens,
                     L, F, fx, sums, pairs, ca_out);
}

}  // namespace fdmi
