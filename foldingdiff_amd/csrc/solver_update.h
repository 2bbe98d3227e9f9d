// The update of a visit of the second-order multistep solver (include/fdmi.h); its callers are update_element
// (p_sample_update.h) and head_update_img_kernel (rowwise_img.hip).  With the visit's (a, b, c, u, v):
//   m  = a x + b eps                                   strided_update.h's mean
//   x0 = u x + v eps, wrapped where angular            the visit's prediction of the clean state
//   m  = m + c * wrap(x0 - prev)  where c != 0         prev = the prediction of the visit before; the difference of two angles
//                                                      either side of +-pi is about 2 pi as numbers and small on the circle
//   x' = m, wrapped where angular;  prev = x0
// Every product and every sum is rounded once (contraction off, as in strided_update.h).  Where c == 0 prev is NOT read: the
// first visit finds it uninitialised, and 0 * NaN must not reach the state.  One thread per element: the thread that writes
// x' is the only one that touches the element's prev.
#pragma once
#include <hip/hip_runtime.h>

#include "strided_update.h"
#include "wrap_pi.h"

namespace fdmi {

__device__ __forceinline__ float solver_difference(float x0, float prev) {
#pragma clang fp contract(off)
  return x0 - prev;
}

// prev / x0_out: the element's own slots (they may be the same address); returns x'
__device__ __forceinline__ float solver_update(float a, float x, float b, float eps, float c, float u, float v, const float* prev,
                                               float* x0_out, bool angular) {
  float m = strided_mean(a, x, b, eps);
  float x0 = strided_mean(u, x, v, eps);
  if (angular) x0 = wrap_pi(x0);
  if (c != 0.f) {
    float d = solver_difference(x0, *prev);
    if (angular) d = wrap_pi(d);
    m = strided_add_noise(m, c, d);  // m + c d, product and sum rounded once
  }
  if (angular) m = wrap_pi(m);
  *x0_out = x0;
  return m;
}

}  // namespace fdmi
