// The update of a strided (few-step) sampling visit (include/fdmi.h), called by update_element (p_sample_update.h),
// head_update_img_kernel (rowwise_img.hip) and solver_update.h:
//   x' = a x + b eps, then + s z where s != 0 -- every product and every sum rounded once.
// hipcc's default lets a * b + c contract into an FMA, and the __f*_rn functions of the HIP headers are plain operators that
// are contracted all the same once they are inlined (see angle_stats.hip); so the statement is written with operators, in
// blocks with contraction off: its instructions then carry no contract flag wherever they are inlined.
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

__device__ __forceinline__ float strided_mean(float a, float x, float b, float eps) {
#pragma clang fp contract(off)
  const float ax = a * x;
  const float be = b * eps;
  return ax + be;
}

__device__ __forceinline__ float strided_add_noise(float v, float s, float z) {
#pragma clang fp contract(off)
  const float sz = s * z;
  return v + sz;
}

}  // namespace fdmi
