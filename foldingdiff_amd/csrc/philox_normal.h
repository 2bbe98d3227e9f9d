// The one device definition of the perf-mode N(0,1) stream, shared by the update kernels (rowwise.hip, rowwise_img.hip)
// and the noise-by-timestep statistics (angle_stats.hip): Philox4x32-10 (Salmon et al., SC'11; constants as in
// Random123) keyed by the 64-bit seed, counter = (sequence lo, sequence hi, position | (feature / 4) << 24, step), then
// Box-Muller on word pairs.  Restated in numpy: oracle/ref_philox.py.
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// N(0,1) for feature f of token (global sequence `seq`, position l) at step t.
// Counter = (seq lo, seq hi | l << 8 ... ) keeps the stream independent of how the
// batch is sharded across GPUs (the key is the user seed).
__device__ __forceinline__ float philox_normal(unsigned long long seed, int t, long long seq, int l, int f) {
  unsigned o[4];
  philox4x32_10((unsigned)seq, (unsigned)((unsigned long long)seq >> 32), (unsigned)l | ((unsigned)(f >> 2) << 24),
                (unsigned)t, (unsigned)seed, (unsigned)(seed >> 32), o);
  const int pair = (f >> 1) & 1;
  const float u1 = ((float)o[2 * pair] + 0.5f) * 2.3283064365386963e-10f;      // (0, 1]
  const float u2 = ((float)o[2 * pair + 1] + 0.5f) * 2.3283064365386963e-10f;
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (f & 1) ? rad * sn : rad * cs;
}

// The same stream for the four features 4 g .. 4 g + 3 of a token from its one Philox block: out[k * stride] is what
// philox_normal(seed, t, seq, l, 4 g + k) returns.  The two Box-Muller pairs go through one copy of the code (a loop that
// is kept a loop, the pair's words picked by selects), which keeps a caller's scalar registers free.
__device__ __forceinline__ void philox_normal4(unsigned long long seed, int t, long long seq, int l, int g,
                                               float* __restrict__ out, int stride) {
  unsigned o[4];
  philox4x32_10((unsigned)seq, (unsigned)((unsigned long long)seq >> 32), (unsigned)l | ((unsigned)g << 24), (unsigned)t,
                (unsigned)seed, (unsigned)(seed >> 32), o);
#pragma unroll 1
  for (int pair = 0; pair < 2; ++pair) {
    const unsigned w1 = pair ? o[2] : o[0], w2 = pair ? o[3] : o[1];
    const float u1 = ((float)w1 + 0.5f) * 2.3283064365386963e-10f;      // (0, 1]
    const float u2 = ((float)w2 + 0.5f) * 2.3283064365386963e-10f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    out[(2 * pair) * stride] = rad * cs;
    out[(2 * pair + 1) * stride] = rad * sn;
  }
}

}  // namespace fdmi
