// HBM-bound, one-wave-per-token kernels of the reverse-diffusion step:
//   embed        K1  Linear(F->d) + BertEmbeddings LayerNorm + time embedding
//                    (foldingdiff/modelling.py:464-472, :157-170)
//   layernorm        standalone residual LayerNorm (unfused fallback of the GEMM epilogue)
//   head_update  K8 tail + K9: AnglesPredictor.layer_norm + dense2 (modelling.py:206-207),
//                    the p_sample update (foldingdiff/sampling.py:62-75) and the per-feature
//                    wrap to [-pi, pi) (sampling.py:119-130, utils.py:100-106)
//   philox_fill      the perf-mode N(0,1) stream, exposed for tests
// A token's d_model row is spread over the 64 lanes (column = lane + 64*j, coalesced
// 256-byte wave accesses); reductions are xor-shuffle butterflies over the wavefront.
#include <cstdlib>
#include <type_traits>

#include "fdmi_kernels.h"
#include "inpaint_replace.h"
#include "p_sample_update.h"
#include "philox_normal.h"
#include "wrap_pi.h"

namespace fdmi {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// sum over the 16 lanes of a DPP row (result in all 16): quad butterflies + the two mirror steps
__device__ __forceinline__ float row16_sum(float v) {
#define FD_DPP_ADD(ctrl) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false))
  FD_DPP_ADD(0xB1);   // quad_perm [1,0,3,2]
  FD_DPP_ADD(0x4E);   // quad_perm [2,3,0,1]
  FD_DPP_ADD(0x141);  // row_half_mirror
  FD_DPP_ADD(0x140);  // row_mirror
#undef FD_DPP_ADD
  return v;
}

static int rowwise_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---- 16-lanes-per-token layout (d = 64 * NV, the released d = 384 -> NV = 6) ----
// Lane k of a 16-lane group owns the float4 columns k + 16 j (j < NV): 256-byte coalesced group
// accesses, row reductions are 4 DPP steps (no LDS round trips), 16 tokens per workgroup pass and a
// grid-stride loop, so the per-column parameters (LayerNorm gamma / beta, bias, time embedding)
// live in registers and the small weight matrix in LDS for the whole launch.
template <int NV>
__device__ __forceinline__ void row16_layernorm(float4 (&v)[NV], const float4 (&gm)[NV], const float4 (&bt)[NV], int d,
                                                float eps) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  const float mean = row16_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j].x -= mean; v[j].y -= mean; v[j].z -= mean; v[j].w -= mean;
    q += (v[j].x * v[j].x + v[j].y * v[j].y) + (v[j].z * v[j].z + v[j].w * v[j].w);
  }
  const float rstd = 1.0f / sqrtf(row16_sum(q) / (float)d + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j].x = v[j].x * rstd * gm[j].x + bt[j].x;
    v[j].y = v[j].y * rstd * gm[j].y + bt[j].y;
    v[j].z = v[j].z * rstd * gm[j].z + bt[j].z;
    v[j].w = v[j].w * rstd * gm[j].w + bt[j].w;
  }
}

// LayerNorm of a row held as v[j] = row[lane + 64 j]  (biased variance, rstd = 1/sqrt(var+eps))
template <int NJ>
__device__ __forceinline__ void row_layernorm(float (&v)[NJ], int lane, int d, const float* gamma, const float* beta,
                                              float eps) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) s += (lane + 64 * j < d) ? v[j] : 0.f;
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float dl = (lane + 64 * j < d) ? v[j] - mean : 0.f;
    q += dl * dl;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < d) v[j] = (v[j] - mean) * rstd * gamma[c] + beta[c];
  }
}

// ------------------------------------------------------------------ embed (K1)
// PER_SEQ (fd_forward_t, fd_denoise_loss): t_src is t_seq[B], one timestep per sequence, and a token of sequence b = tok / L
// adds time_table[t_seq[b]]; otherwise t_src is the step's t_dev.  A compile-time parameter, so that the single-timestep
// kernels (every sampling step, the captured graph) hold no trace of the other mode.
template <int NJ, bool PER_SEQ>
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ x, const float* __restrict__ w_in,
                                                    const float* __restrict__ b_in, const float* __restrict__ pos_emb,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, const float* __restrict__ time_table,
                                                    const int* __restrict__ t_src, float* __restrict__ h, int M, int L,
                                                    int F, int d) {
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= M) return;
  const int t = PER_SEQ ? t_src[tok / L] : *t_src;
  float xin[kMaxFeat];
#pragma unroll
  for (int f = 0; f < kMaxFeat; ++f) xin[f] = f < F ? x[(size_t)tok * F + f] : 0.f;
  float v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    float a = 0.f;
    if (c < d) {
      a = b_in[c];
      for (int f = 0; f < F; ++f) a += xin[f] * w_in[c * F + f];
      if (pos_emb) a += pos_emb[(size_t)(tok % L) * d + c];  // absolute positions only (modelling.py:164-166)
    }
    v[j] = a;
  }
  row_layernorm<NJ>(v, lane, d, gamma, beta, eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < d) h[(size_t)tok * d + c] = v[j] + time_table[(size_t)t * d + c];  // added AFTER the LayerNorm (:472)
  }
}

template <int NV, bool PER_SEQ>
__global__ __launch_bounds__(256) void embed16_kernel(const float* __restrict__ x, const float* __restrict__ w_in,
                                                      const float* __restrict__ b_in, const float* __restrict__ pos_emb,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float eps, const float* __restrict__ time_table,
                                                      const int* __restrict__ t_src, float* __restrict__ h, int M, int L,
                                                      int F) {
  constexpr int d = 64 * NV;
  extern __shared__ __attribute__((aligned(16))) float wT[];  // [F][d]: w_in transposed
  for (int i = threadIdx.x; i < F * d; i += 256) {
    const int f = i / d, c = i - f * d;
    wT[i] = w_in[c * F + f];
  }
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  [[maybe_unused]] const int t = PER_SEQ ? 0 : *t_src;
  float4 bi[NV], gm[NV], bt[NV], tt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = 4 * (k + 16 * j);
    bi[j] = *reinterpret_cast<const float4*>(b_in + c);
    gm[j] = *reinterpret_cast<const float4*>(gamma + c);
    bt[j] = *reinterpret_cast<const float4*>(beta + c);
    if constexpr (!PER_SEQ) tt[j] = *reinterpret_cast<const float4*>(time_table + (size_t)t * d + c);  // the step's row, once
  }
  __syncthreads();
  for (int tg = blockIdx.x; tg * 16 < M; tg += gridDim.x) {
    const int tok = tg * 16 + g;
    const int tc = tok < M ? tok : M - 1;
    float4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = bi[j];
    for (int f = 0; f < F; ++f) {
      const float xf = x[(size_t)tc * F + f];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float4 w = *reinterpret_cast<const float4*>(wT + f * d + 4 * (k + 16 * j));
        v[j].x += xf * w.x; v[j].y += xf * w.y; v[j].z += xf * w.z; v[j].w += xf * w.w;
      }
    }
    if (pos_emb) {  // absolute positions only (modelling.py:164-166)
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float4 pe = *reinterpret_cast<const float4*>(pos_emb + (size_t)(tc % L) * d + 4 * (k + 16 * j));
        v[j].x += pe.x; v[j].y += pe.y; v[j].z += pe.z; v[j].w += pe.w;
      }
    }
    row16_layernorm<NV>(v, gm, bt, d, eps);
    if constexpr (PER_SEQ) {
      const float* trow = time_table + (size_t)t_src[tc / L] * d;  // the sequence's own row of the table
#pragma unroll
      for (int j = 0; j < NV; ++j) tt[j] = *reinterpret_cast<const float4*>(trow + 4 * (k + 16 * j));
    }
    if (tok < M) {
#pragma unroll
      for (int j = 0; j < NV; ++j)  // time embedding added AFTER the LayerNorm (modelling.py:472)
        *reinterpret_cast<float4*>(h + (size_t)tok * d + 4 * (k + 16 * j)) =
            make_float4(v[j].x + tt[j].x, v[j].y + tt[j].y, v[j].z + tt[j].z, v[j].w + tt[j].w);
    }
  }
}

// FDMI_ROWWISE16=0 keeps the one-wave-per-token kernels (also the generic path for d % 64 != 0 or d > 512)
static bool use_row16(int d) {
  static const int on = rowwise_env_int("FDMI_ROWWISE16", 1);
  return on && d % 64 == 0 && d >= 64 && d <= 512;
}

// The one-wave-per-token kernels exist for 1, 3, 6, 12 and 16 columns per lane: fn(integral_constant NJ) of the smallest that holds d
template <typename Fn>
static void with_row_nj(int d, Fn&& fn) {
  const int nj = (d + 63) / 64;
  if (nj <= 1) fn(std::integral_constant<int, 1>{});
  else if (nj <= 3) fn(std::integral_constant<int, 3>{});
  else if (nj <= 6) fn(std::integral_constant<int, 6>{});
  else if (nj <= 12) fn(std::integral_constant<int, 12>{});
  else fn(std::integral_constant<int, 16>{});
}

template <bool PER_SEQ>
static void launch_embed_as(const float* x, const float* w_in, const float* b_in, const float* pos_emb, const float* gamma,
                            const float* beta, float eps, const float* time_table, const int* t_src, float* h, int M, int L, int F,
                            int d, hipStream_t s) {
  if (use_row16(d)) {
    int grid = (M + 15) / 16;
    if (grid > 2048) grid = 2048;
#define FD_E16(NV)                                                                                                             \
  case NV:                                                                                                                     \
    hipLaunchKernelGGL((embed16_kernel<NV, PER_SEQ>), dim3(grid), dim3(256), (size_t)F * 64 * NV * 4, s, x, w_in, b_in, pos_emb, \
                       gamma, beta, eps, time_table, t_src, h, M, L, F);                                                       \
    return;
    switch (d / 64) { FD_E16(1) FD_E16(2) FD_E16(3) FD_E16(4) FD_E16(5) FD_E16(6) FD_E16(7) FD_E16(8) }
#undef FD_E16
  }
  with_row_nj(d, [&](auto nj) {
    hipLaunchKernelGGL((embed_kernel<decltype(nj)::value, PER_SEQ>), dim3((M + 3) / 4), dim3(256), 0, s, x, w_in, b_in, pos_emb, gamma,
                       beta, eps, time_table, t_src, h, M, L, F, d);
  });
}

void launch_embed(const float* x, const float* w_in, const float* b_in, const float* pos_emb, const float* gamma,
                  const float* beta, float eps, const float* time_table, const int* t_dev, const int* t_seq, float* h, int B,
                  int L, int F, int d, hipStream_t s) {
  if (t_seq) launch_embed_as<true>(x, w_in, b_in, pos_emb, gamma, beta, eps, time_table, t_seq, h, B * L, L, F, d, s);
  else launch_embed_as<false>(x, w_in, b_in, pos_emb, gamma, beta, eps, time_table, t_dev, h, B * L, L, F, d, s);
}

// ------------------------------------------------------------- standalone LN
template <int NJ>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        float* __restrict__ y, int rows, int d) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < d ? x[(size_t)row * d + c] : 0.f;
  }
  row_layernorm<NJ>(v, lane, d, gamma, beta, eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < d) y[(size_t)row * d + c] = v[j];
  }
}

void launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int d,
                      hipStream_t s) {
  with_row_nj(d, [&](auto nj) {
    hipLaunchKernelGGL((layernorm_kernel<decltype(nj)::value>), dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma, beta, eps, y, rows, d);
  });
}

// ---------------------------------------------------------- Philox4x32-10 (philox_normal.h)
__global__ void philox_fill_kernel(float* __restrict__ out, unsigned long long seed, int t, long long seq_offset, int B,
                                   int L, int F) {
  const long long n = (long long)B * L * F;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const long long tok = i / F;
    out[i] = philox_normal(seed, t, seq_offset + tok / L, (int)(tok % L), f);
  }
}

void launch_philox_fill(float* out, unsigned long long seed, int t, long long seq_offset, int B, int L, int F,
                        hipStream_t s) {
  const long long n = (long long)B * L * F;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(philox_fill_kernel, dim3(blocks), dim3(256), 0, s, out, seed, t, seq_offset, B, L, F);
}

// --------------------------------------------- head tail + p_sample update (K8/K9)
// (the wrap to [-pi, pi) of the update: wrap_pi.h)
__global__ void wrap_test_f32_kernel(const float* in, float* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = wrap_pi(in[i]);
}

template <int NJ>
__global__ __launch_bounds__(256) void head_update_kernel(UpdateArgs a) {
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= a.M) return;
  const int d = a.d, F = a.F;
  float v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < d ? a.g[(size_t)tok * d + c] : 0.f;
  }
  if (a.do_ln) row_layernorm<NJ>(v, lane, d, a.gamma, a.beta, a.ln_eps);
  // dense2: F dot products of length d, reduced over the wave; lane f keeps result f
  float mine = 0.f;
  for (int f = 0; f < F; ++f) {
    float partial = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < d) partial += v[j] * a.w2[(size_t)f * d + c];
    }
    partial = wave_sum(partial);
    if (lane == f) mine = partial + a.b2[f];
  }
  if (lane >= F) return;
  const size_t o = (size_t)tok * F + lane;
  if (a.eps_out) a.eps_out[o] = mine;
  if (!a.x_out) return;
  update_element(a, resolve_update(a, *a.t_dev, true), o, mine, tok / a.L, tok % a.L, lane, (size_t)a.M * F);
}

template <int NV>
__global__ __launch_bounds__(256) void head_update16_kernel(UpdateArgs a) {
  constexpr int d = 64 * NV;
  extern __shared__ __attribute__((aligned(16))) float w2s[];  // [F][d]
  const int F = a.F;
  for (int i = threadIdx.x; i < F * d; i += 256) w2s[i] = a.w2[i];
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  float4 gm[NV], bt[NV];
  if (a.do_ln) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      gm[j] = *reinterpret_cast<const float4*>(a.gamma + 4 * (k + 16 * j));
      bt[j] = *reinterpret_cast<const float4*>(a.beta + 4 * (k + 16 * j));
    }
  }
  const float b2k = a.b2[k < F ? k : 0];
  const UpdateVisit m = resolve_update(a, a.x_out ? *a.t_dev : 0, a.x_out != nullptr);  // before the row loop: see p_sample_update.h
  __syncthreads();
  for (int tg = blockIdx.x; tg * 16 < a.M; tg += gridDim.x) {
    const int tok = tg * 16 + g;
    const int tc = tok < a.M ? tok : a.M - 1;
    float4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const float4*>(a.g + (size_t)tc * d + 4 * (k + 16 * j));
    if (a.do_ln) row16_layernorm<NV>(v, gm, bt, d, a.ln_eps);
    // dense2: F dot products of length d; lane f of the group keeps result f
    float mine = 0.f;
    for (int f = 0; f < F; ++f) {
      float partial = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float4 w = *reinterpret_cast<const float4*>(w2s + f * d + 4 * (k + 16 * j));
        partial += (v[j].x * w.x + v[j].y * w.y) + (v[j].z * w.z + v[j].w * w.w);
      }
      partial = row16_sum(partial);
      mine = (k == f) ? partial + b2k : mine;
    }
    if (k < F && tok < a.M) {
      const size_t o = (size_t)tok * F + k;
      if (a.eps_out) a.eps_out[o] = mine;
      if (a.x_out) update_element(a, m, o, mine, tok / a.L, tok % a.L, k, (size_t)a.M * F);
    }
  }
}

template <int NV>
static void launch_head_update16(const UpdateArgs& a, hipStream_t s) {
  int grid = (a.M + 15) / 16;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((head_update16_kernel<NV>), dim3(grid), dim3(256), (size_t)a.F * 64 * NV * 4, s, a);
}

void launch_head_update(const UpdateArgs& a, hipStream_t s) {
  if (use_row16(a.d) && a.F <= 16) {
#define FD_H16(NV) case NV: launch_head_update16<NV>(a, s); return;
    switch (a.d / 64) { FD_H16(1) FD_H16(2) FD_H16(3) FD_H16(4) FD_H16(5) FD_H16(6) FD_H16(7) FD_H16(8) }
#undef FD_H16
  }
  with_row_nj(a.d, [&](auto nj) {
    hipLaunchKernelGGL((head_update_kernel<decltype(nj)::value>), dim3((a.M + 3) / 4), dim3(256), 0, s, a);
  });
}

// ---- the start point of a motif-conditioned run: its fixed elements at level `level` (inpaint_replace.h)
__global__ __launch_bounds__(256) void inpaint_init_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                           const unsigned char* __restrict__ fixed,
                                                           const float* __restrict__ known_noise,
                                                           const float* __restrict__ known_coef, int T, int level,
                                                           unsigned long long seed, long long seq_offset, long long n, int L,
                                                           int F, unsigned angle_mask) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (!fixed[i]) continue;
    const int f = (int)(i % F);
    const long long tok = i / F;
    // known_noise is the slab of this level already: stride 0
    x[i] = inpaint_value(known, known_noise, known_coef, T, 0, level, (size_t)i, seed, seq_offset + tok / L, (int)(tok % L), f,
                         (angle_mask >> f) & 1u);
  }
}

void launch_inpaint_init(float* x, const float* known, const unsigned char* fixed, const float* known_noise,
                         const float* known_coef, int T, int level, unsigned long long seed, long long seq_offset, int B,
                         int L, int F, unsigned angle_mask, hipStream_t s) {
  const long long n = (long long)B * L * F;
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(inpaint_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, known, fixed, known_noise, known_coef, T,
                     level, seed, seq_offset, n, L, F, angle_mask);
}

__global__ void step_advance_kernel(int* t_dev, const UpdateDyn* dyn) {
  if (dyn && dyn->next_t) *t_dev = dyn->next_t[*t_dev];  // a strided run: the next visit's t (-1 behind the last)
  else *t_dev -= 1;
}
void launch_step_advance(int* t_dev, const UpdateDyn* dyn, hipStream_t s) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, t_dev, dyn);
}

void launch_wrap_test_f32(const float* in, float* out, long long n, hipStream_t s) {
  hipLaunchKernelGGL(wrap_test_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}

}  // namespace fdmi
