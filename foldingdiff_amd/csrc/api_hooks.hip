// C-ABI test and measurement hooks: single kernels on host operands, for the parity tests and the GEMM timing scripts.
// None of them sees a model: each takes a device_id and owns its device buffers for the call (host_common.h).
// Boundary: include/fdmi.h.
#include <cmath>
#include <cstring>
#include <vector>

#include "fdmi_kernels.h"
#include "host_common.h"
#include "weight_pack.h"

using namespace fdmi;

namespace {

float max_abs(const float* p, size_t n) {
  float mx = 0.f;
  for (size_t i = 0; i < n; ++i) mx = std::fmax(mx, std::fabs(p[i]));
  return mx;
}

// Test hook plumbing of the row-image GEMM: fp32 host operands -> images (scales chosen from the data exactly as
// fd_finalize chooses them from weight bounds) -> production kernel -> fp32.  The images are zero-filled before the
// conversion kernels write them: their padding rows must hold zeros.
// epilogue: EPI_IMG_BIAS | EPI_IMG_GELU | EPI_IMG_LN; tail: GemmImgArgs::tail (1 = the instantiation that cuts an incomplete last
// round into row slices -- the hook's ragged row counts exercise them; 0 = whole tiles only: valid for every shape, same bits)
int img_gemm_hook(int epilogue, const float* A, const float* W, const float* bias, const float* resid, const float* gamma,
                  const float* beta, float eps, float* C, int M, int N, int K, int tail = 1) {
  if (N % 32 || K % 32) return fail(FD_E_UNSUPPORTED, "row-image GEMM: N=%d and K=%d must be multiples of 32", N, K);
  if (epilogue == EPI_IMG_LN && N > 384) return fail(FD_E_UNSUPPORTED, "LN-fused GEMM: N=%d > 384", N);
  DeviceBufs bufs;
  const long long rows = ((long long)M + 127) / 128 * 128;
  const float *dA, *db;
  float* dC;
  unsigned char *dAi, *dOi, *dtrash;
  const unsigned char* dWi;
  const int* ddims;
  HIP_TRY(bufs.upload(A, (size_t)M * K * 4, &dA));
  HIP_TRY(bufs.upload(bias, (size_t)N * 4, &db));
  HIP_TRY(bufs.zeros((size_t)rows * K * 4, &dAi));
  HIP_TRY(bufs.zeros((size_t)rows * N * 4, &dOi));
  HIP_TRY(bufs.zeros((size_t)rows * N * 4, &dC));
  HIP_TRY(bufs.zeros(1024, &dtrash));
  const int hd[2] = {M, (int)rows};
  HIP_TRY(bufs.upload(hd, sizeof hd, &ddims));
  const Image wimg = pack_weight_tiles(W, N, K);
  const float wscale = wimg.scale;
  HIP_TRY(bufs.upload(wimg.data.data(), wimg.data.size() * 2, &dWi));
  const float a_scale = scale_for(max_abs(A, (size_t)M * K));
  launch_f32_to_img(dA, dAi, rows, K, M, a_scale, nullptr);
  // output bound as fd_finalize derives it: ||row of A||_2 ||row of W||_2 + |bias| (+ residual); LayerNorm: gamma/beta
  float in_l2 = 0.f;
  for (int r = 0; r < M; ++r) {
    double n2 = 0.0;
    for (int k = 0; k < K; ++k) n2 += (double)A[(size_t)r * K + k] * A[(size_t)r * K + k];
    in_l2 = std::fmax(in_l2, (float)std::sqrt(n2));
  }
  GemmImgArgs g;
  memset(&g, 0, sizeof g);
  g.A = dAi;
  g.W = dWi;
  g.bias = db;
  g.out = dOi;
  g.trash = dtrash;
  g.dims = ddims;
  g.N = N;
  g.K = K;
  g.acc_scale = 1.0f / (a_scale * wscale);
  g.eps = eps;
  float out_scale;
  if (epilogue == EPI_IMG_LN) {
    const float *dg, *dbt, *dR;
    unsigned char* dRi;
    HIP_TRY(bufs.upload(gamma, (size_t)N * 4, &dg));
    HIP_TRY(bufs.upload(beta, (size_t)N * 4, &dbt));
    HIP_TRY(bufs.upload(resid, (size_t)M * N * 4, &dR));
    HIP_TRY(bufs.zeros((size_t)rows * N * 4, &dRi));
    const float r_scale = scale_for(max_abs(resid, (size_t)M * N));
    launch_f32_to_img(dR, dRi, rows, N, M, r_scale, nullptr);
    g.resid = dRi;
    g.resid_inv = 1.0f / r_scale;
    g.gamma = dg;
    g.beta = dbt;
    out_scale = scale_for(max_abs(gamma, N) * std::sqrt((float)N) + max_abs(beta, N));
  } else {
    out_scale = scale_for(dense_bound(W, bias, 0, N, K, in_l2));
  }
  g.out_scale = out_scale;
  g.tail = tail;
  launch_gemm_img(epilogue, g, (int)rows, nullptr);
  launch_img_to_f32(dOi, dC, rows, N, out_scale, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  return FD_OK;
}

// an event that lives for one call
struct ScopedEvent {
  hipEvent_t e = nullptr;
  ScopedEvent() = default;
  ScopedEvent(const ScopedEvent&) = delete;
  ScopedEvent& operator=(const ScopedEvent&) = delete;
  ~ScopedEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

extern "C" {

int fd_test_wrap(int device_id, int which, const float* in, int64_t n, float* out) {
  if (!in || !out || n < 1) return fail(FD_E_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(device_id));
  DeviceBufs bufs;
  float *din, *dout;
  HIP_TRY(bufs.alloc((size_t)n * 4, &din));
  HIP_TRY(bufs.alloc((size_t)n * 4, &dout));
  HIP_TRY(hipMemcpy(din, in, (size_t)n * 4, hipMemcpyHostToDevice));
  if (which == 0) launch_wrap_test_f32(din, dout, n, nullptr);
  else launch_wrap_test_img(din, dout, n, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
  return FD_OK;
}

int fd_tie_repeats(int device_id, const float* x, const int32_t* lens, const int32_t* tie, int B, int L, int F,
                   const uint8_t* is_angle, int init, float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* out) {
  if (!x || !lens || !tie || !is_angle || !out) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1 || F < 1) return fail(FD_E_INVALID, "bad argument: B=%d L=%d F=%d must be positive", B, L, F);
  if (F > 32) return fail(FD_E_UNSUPPORTED, "F=%d: at most 32 features", F);
  if ((long long)B * L * F > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * F = %lld elements, at most 2^31 - 1", (long long)B * L * F);
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_tie(tie, lens, B)) return rc;
  if (!std::isfinite(s)) return fail(FD_E_INVALID, "s = %g is not finite", (double)s);
  unsigned angle_mask = 0;
  for (int f = 0; f < F; ++f)
    if (is_angle[f]) angle_mask |= 1u << f;
  const size_t n = (size_t)B * L * F;
  const bool draws = !init && s != 0.f && z;  // (the slab is read only then)
  std::vector<float> state_host(n);  // the rows at or beyond a length are not the kernel's: `out` keeps what it held there
  const int rc = device_roundtrip(device_id, {{x, n * 4}, {lens, (size_t)B * 4}, {tie, (size_t)B * 3 * 4}, {draws ? z : x, draws ? n * 4 : 4}},
                          {{state_host.data(), n * 4}}, [&](const RoundtripBufs& d) -> hipError_t {
                            float* state = d.out(0);
                            const float* x_dev = d.in(0);
                            const float* z_dev = d.in(3);
                            const hipError_t e = hipMemcpyAsync(state, x_dev, n * 4, hipMemcpyDeviceToDevice, nullptr);
                            if (e != hipSuccess) return e;
                            launch_repeat_tie(state, d.in(1), d.in(2), B, L, F, angle_mask, init ? 1 : 0, s, draws ? z_dev : nullptr, seed,
                                              t, seq_offset, nullptr);
                            return hipSuccess;
                          });
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    memcpy(out + (size_t)b * L * F, state_host.data() + (size_t)b * L * F, (size_t)lens[b] * F * 4);
  return FD_OK;
}

int fd_test_gemm(int device_id, int precision, int epilogue, const float* A, const float* W, const float* bias,
                 const float* resid, float* C, int M, int N, int K) {
  if (!A || !W || !bias || !C || M < 1 || N < 1 || K < 16 || K % 32) return fail(FD_E_INVALID, "bad argument");
  const int tail = epilogue & FD_TEST_GEMM_WHOLE_TILES ? 0 : 1;
  epilogue &= ~FD_TEST_GEMM_WHOLE_TILES;
  if (epilogue < EPI_BIAS || epilogue > EPI_BIAS_RESID || (epilogue == EPI_BIAS_RESID && !resid))
    return fail(FD_E_INVALID, "bad epilogue");
  HIP_TRY(hipSetDevice(device_id));
  if (precision == FD_PREC_F16X3) {
    if (epilogue == EPI_BIAS_RESID)
      return fail(FD_E_UNSUPPORTED, "the row-image path has no unfused residual epilogue (LayerNorm is always fused): use fd_test_gemm_ln");
    return img_gemm_hook(epilogue == EPI_BIAS_GELU ? EPI_IMG_GELU : EPI_IMG_BIAS, A, W, bias, nullptr, nullptr, nullptr, 0.f, C, M, N, K, tail);
  }
  DeviceBufs bufs;
  float *dA, *dW, *db, *dC;
  const float* dr = nullptr;
  HIP_TRY(bufs.alloc((size_t)M * K * 4, &dA));
  HIP_TRY(bufs.alloc((size_t)N * K * 4, &dW));
  HIP_TRY(bufs.alloc((size_t)N * 4, &db));
  HIP_TRY(bufs.alloc((size_t)M * N * 4, &dC));
  HIP_TRY(hipMemcpy(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dW, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
  if (resid) HIP_TRY(bufs.upload(resid, (size_t)M * N * 4, &dr));
  if (precision != FD_PREC_F32) return fail(FD_E_INVALID, "precision %d", precision);
  launch_gemm_f32(epilogue, dA, dW, db, dr, dC, M, N, K, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  return FD_OK;
}

int fd_test_gemm_ln(int device_id, int precision, int use_fused, const float* A, const float* W, const float* bias,
                    const float* resid, const float* gamma, const float* beta, float eps, float* C, int M, int N,
                    int K) {
  if (!A || !W || !bias || !resid || !gamma || !beta || !C || M < 1 || N < 1 || K < 32 || K % 32)
    return fail(FD_E_INVALID, "bad argument");
  if (precision != FD_PREC_F32 && precision != FD_PREC_F16X3) return fail(FD_E_INVALID, "precision %d", precision);
  HIP_TRY(hipSetDevice(device_id));
  if (precision == FD_PREC_F16X3) {
    if (!use_fused) return fail(FD_E_UNSUPPORTED, "the row-image path always fuses the LayerNorm into the GEMM");
    return img_gemm_hook(EPI_IMG_LN, A, W, bias, resid, gamma, beta, eps, C, M, N, K);
  }
  DeviceBufs bufs;
  const float *dA, *dW, *db, *dr, *dg, *dbt;
  float *dT, *dC;
  HIP_TRY(bufs.upload(A, (size_t)M * K * 4, &dA));
  HIP_TRY(bufs.upload(W, (size_t)N * K * 4, &dW));
  HIP_TRY(bufs.upload(bias, (size_t)N * 4, &db));
  HIP_TRY(bufs.upload(resid, (size_t)M * N * 4, &dr));
  HIP_TRY(bufs.upload(gamma, (size_t)N * 4, &dg));
  HIP_TRY(bufs.upload(beta, (size_t)N * 4, &dbt));
  HIP_TRY(bufs.alloc((size_t)M * N * 4, &dT));
  HIP_TRY(bufs.alloc((size_t)M * N * 4, &dC));
  if (use_fused) {
    if (!launch_gemm_f32_ln(dA, dW, db, dr, dg, dbt, eps, dC, M, N, K, nullptr))
      return fail(FD_E_UNSUPPORTED, "no LN-fused GEMM for N=%d K=%d in this precision", N, K);
  } else {
    launch_gemm_f32(EPI_BIAS_RESID, dA, dW, db, dr, dT, M, N, K, nullptr);
    launch_layernorm(dT, dg, dbt, eps, dC, M, N, nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  return FD_OK;
}

int fd_test_gemm_time(int device_id, int precision, int M, int N, int K, int reps, double* ms_per_launch) {
  if (!ms_per_launch || M < 1 || N < 1 || K < 32 || K % 32 || reps < 1) return fail(FD_E_INVALID, "bad argument");
  if (precision == FD_PREC_F16X3 && N % 32) return fail(FD_E_UNSUPPORTED, "row-image GEMM: N=%d must be a multiple of 32", N);
  HIP_TRY(hipSetDevice(device_id));
  std::vector<float> hA((size_t)M * K), hW((size_t)N * K), hb(N, 0.1f);
  unsigned st = 12345u;
  auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
  for (auto& v : hA) v = rnd();
  for (auto& v : hW) v = 0.02f * rnd();
  DeviceBufs bufs;
  ScopedEvent e0, e1;
  const long long rows = ((long long)M + 127) / 128 * 128;
  const float *dA, *dW, *db;
  float* dC;
  HIP_TRY(bufs.upload(hA.data(), hA.size() * 4, &dA));
  HIP_TRY(bufs.upload(hW.data(), hW.size() * 4, &dW));
  HIP_TRY(bufs.upload(hb.data(), (size_t)N * 4, &db));
  HIP_TRY(bufs.zeros((size_t)rows * N * 4, &dC));
  GemmImgArgs g;
  memset(&g, 0, sizeof g);
  if (precision == FD_PREC_F16X3) {
    unsigned char *dAi, *dtrash;
    const unsigned char* dWi;
    const int* ddims;
    const Image wimg = pack_weight_tiles(hW.data(), N, K);
    const float wscale = wimg.scale;
    HIP_TRY(bufs.zeros((size_t)rows * K * 4, &dAi));
    HIP_TRY(bufs.upload(wimg.data.data(), wimg.data.size() * 2, &dWi));
    HIP_TRY(bufs.zeros(1024, &dtrash));
    const int hd[2] = {M, (int)rows};
    HIP_TRY(bufs.upload(hd, sizeof hd, &ddims));
    launch_f32_to_img(dA, dAi, rows, K, M, 8192.0f, nullptr);
    g.A = dAi;
    g.W = dWi;
    g.bias = db;
    g.out = reinterpret_cast<unsigned char*>(dC);
    g.trash = dtrash;
    g.dims = ddims;
    g.N = N;
    g.K = K;
    g.acc_scale = 1.0f / (8192.0f * wscale);
    g.out_scale = 1024.0f;
  }
  HIP_TRY(hipEventCreate(&e0.e));
  HIP_TRY(hipEventCreate(&e1.e));
  auto run = [&]() {
    if (precision == FD_PREC_F16X3) launch_gemm_img(EPI_IMG_BIAS, g, (int)rows, nullptr);
    else launch_gemm_f32(EPI_BIAS, dA, dW, db, nullptr, dC, M, N, K, nullptr);
  };
  for (int i = 0; i < 3; ++i) run();
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventRecord(e0.e, nullptr));
  for (int i = 0; i < reps; ++i) run();
  HIP_TRY(hipEventRecord(e1.e, nullptr));
  HIP_TRY(hipEventSynchronize(e1.e));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  *ms_per_launch = ms / reps;
  return FD_OK;
}

}  // extern "C"
