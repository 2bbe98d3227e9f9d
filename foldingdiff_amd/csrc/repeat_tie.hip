// Tying the angle rows of repeat units (include/fdmi.h): the kernel that sits between two replays of the step
// graph in fd_sample_repeat, and behind fd_tie_repeats.  In place on a [B][L][F] state; sequence b has a tie
// (start, period, units), and row start + k * period + j is copy k of unit row j.  For a tied element with copies x_0 .. x_{R-1}:
//   d_k = x_k - x_0 (wrapped where angular), k = 1 .. R - 1;  m = x_0 + (d_1 + .. + d_{R-1}) / float(R), summed left to right
//   m = m + s * z where s != 0;  m = wrap(m) where angular;  every copy <- m
// A free element of a row below the length: m = x, then the same + s z and wrap.  z is the explicit slab's entry at the copy-0
// position, or philox_normal(seed, t, seq_offset + b, l, f) with l the copy-0 row: the draw the update kernel would have made
// there.  `init`: every copy <- x_0, nothing else.  Every product, sum and quotient is rounded once (strided_update.h).
// One thread per element; the copy-0 thread of a tied element reads and writes all its copies and the threads of the other
// copies return, so in place is safe.  A wave's threads sit on consecutive addresses at every copy.  No LDS, no scratch.
#include "fdmi_kernels.h"
#include "philox_normal.h"
#include "strided_update.h"
#include "wrap_pi.h"

namespace fdmi {

namespace {

__device__ __forceinline__ float tie_diff(float xk, float x0) {
#pragma clang fp contract(off)
  return xk - x0;
}

__device__ __forceinline__ float tie_sum(float acc, float d) {
#pragma clang fp contract(off)
  return acc + d;
}

__device__ __forceinline__ float tie_mean(float x0, float sum, float units) {
#pragma clang fp contract(off)
  const float q = sum / units;
  return x0 + q;
}

__global__ __launch_bounds__(256) void repeat_tie_kernel(float* __restrict__ x, const int* __restrict__ lens,
                                                         const int* __restrict__ tie, long long n, int L, int F, unsigned angle_mask,
                                                         int init, float s, const float* __restrict__ z, unsigned long long seed,
                                                         int t, long long seq_offset) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i % F);
  const long long tok = i / F;
  const int l = (int)(tok % L), b = (int)(tok / L);
  if (l >= lens[b]) return;
  const int start = tie[3 * b], period = tie[3 * b + 1], units = tie[3 * b + 2];
  const bool tied = units > 1 && l >= start && l < start + period * units;
  if (tied && l >= start + period) return;  // a copy k > 0: its copy-0 thread writes it
  if (init && !tied) return;
  const bool angular = (angle_mask >> f) & 1u;
  const long long stride = (long long)period * F;
  const float x0 = x[i];
  float m = x0;
  if (tied && !init) {
    float sum = 0.f;
    for (int k = 1; k < units; ++k) {
      float d = tie_diff(x[i + k * stride], x0);
      if (angular) d = wrap_pi(d);
      sum = k == 1 ? d : tie_sum(sum, d);
    }
    m = tie_mean(x0, sum, (float)units);
  }
  if (!init) {
    if (s != 0.f) m = strided_add_noise(m, s, z ? z[i] : philox_normal(seed, t, seq_offset + b, l, f));
    if (angular) m = wrap_pi(m);
  }
  x[i] = m;
  if (tied)
    for (int k = 1; k < units; ++k) x[i + k * stride] = m;
}

}  // namespace

void launch_repeat_tie(float* x, const int* lens, const int* tie, int B, int L, int F, unsigned angle_mask, int init, float s,
                       const float* z, unsigned long long seed, int t, long long seq_offset, hipStream_t st) {
  const long long n = (long long)B * L * F;
  hipLaunchKernelGGL(repeat_tie_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, lens, tie, n, L, F, angle_mask, init,
                     s, z, seed, t, seq_offset);
}

}  // namespace fdmi
