// The one device definition of utils.modulo_with_wrapped_range(v, -pi, pi) (foldingdiff/utils.py:87-121), shared by the
// update kernels (rowwise.hip, rowwise_img.hip) and the noising / loss kernels (loss.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

// wrap: ((v - lo) % (hi - lo)) + lo with lo = -pi, hi = pi evaluated as torch does on a
// float32 tensor with python-float bounds: v + f32(pi); torch.remainder(., f32(2 pi));
// + f32(-pi).  Explicit __f*_rn keeps the compiler from contracting into FMAs, so for
// identical inputs the result is bit-identical to the reference's CPU arithmetic.
__device__ __forceinline__ float wrap_pi(float v) {
  const float PI_F = 3.14159274101257324f, TWO_PI_F = 6.28318548202514648f;
  const float sft = __fadd_rn(v, PI_F);
  float m = fmodf(sft, TWO_PI_F);
  if (m != 0.f && m < 0.f) m = __fadd_rn(m, TWO_PI_F);
  return __fadd_rn(m, -PI_F);
}

}  // namespace fdmi
