// The fixed-order fp64 sums of the one-workgroup-per-chain kernels (nerf_vjp.hip, guide_scaffold.hip): 256 lanes, four waves.
// The shape of every tree depends on the lane index alone, so two launches on the same input give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

constexpr int kChainThreads = 256;
constexpr int kChainWaves = kChainThreads / 64;

// lane i of a wave ends with v_i + v_{i+1} + ... + v_63, by a doubling tree whose shape does not depend on the data
__device__ __forceinline__ double wave_suffix(double v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_down(v, d, 64);
    if (lane + d < 64) v += o;
  }
  return v;
}

// the sum of v over the workgroup, the same bits in every lane; `slot` holds kChainWaves doubles and is free again on return
__device__ __forceinline__ double block_sum(double v, double* slot) {
  const double s = wave_suffix(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = s;
  __syncthreads();
  double total = slot[0];
#pragma unroll
  for (int w = 1; w < kChainWaves; ++w) total += slot[w];
  __syncthreads();
  return total;
}

}  // namespace fdmi
