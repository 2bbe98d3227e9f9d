// The two per-element statements the guide kernels share, each written once:
//   shift   steer_shift_kernel's (steer.hip) and scaffold_shift_kernel's (guide_scaffold.hip): v + offset[f], rounded once,
//           wrapped where angular; v itself where there is no offset
//   move    guide_update_kernel's (nerf_vjp.hip) and scaffold_update_kernel's: x - float32(ck G) where c != 0, + s z where
//           s != 0 with repeat_tie.hip's draw (z[o], or the Philox word of (seed, t, sequence, l, f)), wrap where angular
// Contraction is off where a product would otherwise fuse into the sum behind it.
#pragma once
#include "fdmi_kernels.h"
#include "philox_normal.h"
#include "strided_update.h"
#include "wrap_pi.h"

namespace fdmi {

__device__ __forceinline__ float shift_add(float v, float off) {
#pragma clang fp contract(off)
  return v + off;
}

__device__ __forceinline__ float steer_shift_value(float v, const SteerOffset& off, unsigned angle_mask, int f) {
  if (off.has_offset) {
    v = shift_add(v, off.offset[f]);
    if ((angle_mask >> f) & 1u) v = wrap_pi(v);
  }
  return v;
}

__device__ __forceinline__ float guide_sub(float x, float step) {
#pragma clang fp contract(off)
  return x - step;
}

// m = x[o]; ck = double(c) * k_b; g = G[o]; seq = seq_offset + b
__device__ __forceinline__ float guide_move(float m, float c, double ck, double g, float s, const float* __restrict__ z, size_t o,
                                            unsigned long long seed, int t, long long seq, int l, int f, unsigned angle_mask) {
  if (c != 0.f) m = guide_sub(m, (float)(ck * g));
  if (s != 0.f) m = strided_add_noise(m, s, z ? z[o] : philox_normal(seed, t, seq, l, f));
  if ((angle_mask >> f) & 1u) m = wrap_pi(m);
  return m;
}

}  // namespace fdmi
