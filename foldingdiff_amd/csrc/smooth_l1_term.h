// The smooth-L1 term of one position (losses.py:29-55 / F.smooth_l1_loss): the one device definition, shared by
// loss_terms_kernel (loss.hip) and its sibling with the "l1" kind and the turn counts (loss_variants.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "wrap_pi.h"

namespace fdmi {

// d = target - pred (wrapped for an angle);  |d| < beta ? 0.5 * d^2 / beta : |d| - 0.5 * beta.  torch evaluates
// 0.5 * (d ** 2) / beta as ((0.5 * (d * d)) / f32(beta)) and abs_d - 0.5 * beta with the python product rounded to float32;
// F.smooth_l1_loss's 0.5 * z * z / beta differs only in where the exact halving happens.
__device__ __forceinline__ float smooth_l1_term(float pred, float target, bool angular, float beta, float half_beta) {
  float d = __fsub_rn(target, pred);
  if (angular) d = wrap_pi(d);
  const float ad = fabsf(d);
  return ad < beta ? __fdiv_rn(__fmul_rn(0.5f, __fmul_rn(d, d)), beta) : __fsub_rn(ad, half_beta);
}

}  // namespace fdmi
