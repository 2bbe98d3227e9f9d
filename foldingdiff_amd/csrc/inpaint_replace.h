// Motif-conditioned sampling ("replacement"): the one device definition of the value a FIXED element of a state
// takes, shared by the p_sample update (update_element in p_sample_update.h for the two fp32 kernels, head_update_img_kernel's
// own copy in rowwise_img.hip) and the kernel that replaces the fixed elements of the start point, so that the statement cannot
// drift between them.
//
// Levels.  A state at level j = 0 .. T has seen j forward-noising steps: the state that enters reverse step t is at level
// t + 1, the state that step t leaves is at level t.  coef = [2][T + 1]: keep[j] then spread[j], keep[0] = 1,
// spread[0] = 0, keep[j] = sqrt_alphas_cumprod[j - 1], spread[j] = sqrt_one_minus_alphas_cumprod[j - 1].
//   level j >= 1: wrap?(keep[j] * known + spread[j] * z), each product and the sum rounded once -- launch_q_sample's
//                 statement (loss.hip); z = known_noise[j][o], or with known_noise null the Philox draw whose step word
//                 is j with the top bit set (a stream disjoint from the update's own draws, whose step word is t < 2^31)
//   level 0:      the bits of known[o]; no arithmetic, no draw
//
// Strided runs: a visit at t lands on the level of the next visit's input, next_t[t] + 1 (0 behind the last
// visit), and that -- not t -- is the level of its fixed elements and of their Philox tag.  An explicit known_noise has one
// row per visit there, not per level, so inpaint_value_row takes the row apart from the level; inpaint_value is the same
// statement with row = level, what every plain caller means.
//
// Resampling: a jump takes a state from level a up to level b > a.  Its fixed elements are inpaint_value at
// level b; a FREE element is wrap?(jk * x + js * z), each product and the sum rounded once, jk = sqrt(acp(b) / acp(a)),
// js = sqrt(1 - acp(b) / acp(a)) made by the host, z = the Philox draw whose step word is b with bit 30 set: a third
// stream, disjoint from the other two while T < 2^30.  jump_value is that statement, shared by the jump kernel and its hook.
#pragma once
#include "philox_normal.h"
#include "wrap_pi.h"

namespace fdmi {

__device__ __forceinline__ float inpaint_value_row(const float* __restrict__ known, const float* __restrict__ known_noise,
                                                   const float* __restrict__ coef, int T, long long noise_stride, int level,
                                                   int noise_row, size_t o, unsigned long long seed, long long seq, int l, int f,
                                                   bool angular) {
  const float kv = known[o];
  if (level <= 0) return kv;
  const float z = known_noise ? known_noise[(size_t)noise_row * (size_t)noise_stride + o]
                              : philox_normal(seed, (int)(0x80000000u | (unsigned)level), seq, l, f);
  float v = __fadd_rn(__fmul_rn(coef[level], kv), __fmul_rn(coef[T + 1 + level], z));
  if (angular) v = wrap_pi(v);
  return v;
}

__device__ __forceinline__ float inpaint_value(const float* __restrict__ known, const float* __restrict__ known_noise,
                                               const float* __restrict__ coef, int T, long long noise_stride, int level,
                                               size_t o, unsigned long long seed, long long seq, int l, int f, bool angular) {
  return inpaint_value_row(known, known_noise, coef, T, noise_stride, level, level, o, seed, seq, l, f, angular);
}

__device__ __forceinline__ float jump_value(float x, float jk, float js, int level_to, unsigned long long seed, long long seq,
                                            int l, int f, bool angular) {
  const float z = philox_normal(seed, (int)(0x40000000u | (unsigned)level_to), seq, l, f);
  float v = __fadd_rn(__fmul_rn(jk, x), __fmul_rn(js, z));
  if (angular) v = wrap_pi(v);
  return v;
}

}  // namespace fdmi
