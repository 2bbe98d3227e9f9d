// The jump of a resampling schedule (inpaint_replace.h): the state of a motif-conditioned run, in place, from
// noise level a up to level b > a.  Elementwise over [B][L][F]; positions at or beyond a sequence's length keep their bits.
#include "fdmi_kernels.h"
#include "inpaint_replace.h"

namespace fdmi {

__global__ __launch_bounds__(256) void inpaint_jump_kernel(float* __restrict__ x, const int* __restrict__ lens,
                                                           const float* __restrict__ known,
                                                           const unsigned char* __restrict__ fixed,
                                                           const float* __restrict__ known_coef, int T, int level_to, float jk,
                                                           float js, unsigned long long seed, long long seq_offset, long long n,
                                                           int L, int F, unsigned angle_mask) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const long long tok = i / F;
    const long long b = tok / L;
    const int l = (int)(tok % L);
    if (l >= lens[b]) continue;
    const bool angular = (angle_mask >> f) & 1u;
    x[i] = fixed[i] ? inpaint_value(known, nullptr, known_coef, T, 0, level_to, (size_t)i, seed, seq_offset + b, l, f, angular)
                    : jump_value(x[i], jk, js, level_to, seed, seq_offset + b, l, f, angular);
  }
}

void launch_inpaint_jump(float* x, const int* lens, const float* known, const unsigned char* fixed, const float* known_coef,
                         int T, int level_to, float jk, float js, unsigned long long seed, long long seq_offset, int B, int L,
                         int F, unsigned angle_mask, hipStream_t s) {
  const long long n = (long long)B * L * F;
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(inpaint_jump_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, lens, known, fixed, known_coef, T, level_to,
                     jk, js, seed, seq_offset, n, L, F, angle_mask);
}

}  // namespace fdmi
