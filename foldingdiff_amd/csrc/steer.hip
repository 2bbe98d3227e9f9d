// Steering a sampling run by particle resampling on device rewards (include/fdmi.h): the kernels that sit
// between two replays of the step graph in fd_sample_steered, and behind fd_steer_rewards / fd_steer_resample.
//   shift     ang = x0 + offset[f], rounded once, wrapped where angular: launch_shift_trim's statement without the trim
//   rewards   launch_nerf, launch_backbone_clashes and launch_psea are called as they are; what is new is the float32 / CA
//             copy of the coordinates between them and, per particle, the radius of gyration, the label fractions and
//             the weighted sum
//   resample  log-weights += lambda * (reward - previous reward), effective sample size, systematic resampling
//   gather    x_new[b] = x[ancestor[b]]
// Every sum is fp64 and runs in a fixed order: the radius of gyration as 64 strided partial sums joined by a butterfly whose
// two operands commute, the weights of a group by one thread in index order.  No floating-point atomics, no scratch of the
// kernels' own; two launches on the same input give the same bits.
#include "fdmi_kernels.h"
#include "guide_element.h"
#include "wrap_pi.h"

namespace fdmi {

namespace {

__global__ __launch_bounds__(256) void steer_shift_kernel(const float* __restrict__ x0, const int* __restrict__ lens, long long n,
                                                          int L, int F, SteerOffset off, unsigned angle_mask,
                                                          float* __restrict__ ang) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const long long tok = i / F;
    const int l = (int)(tok % L), b = (int)(tok / L);
    float v = 0.f;
    if (l < lens[b]) v = steer_shift_value(x0[i], off, angle_mask, f);
    ang[i] = v;
  }
}

// coords [n_res][3 atoms][3] fp64 -> the same as float32, and the CA atoms [n_res][3] fp64
__global__ __launch_bounds__(256) void steer_atoms_kernel(const double* __restrict__ coords, long long n_res, float* __restrict__ xyz,
                                                          double* __restrict__ ca) {
  const long long n = n_res * 9;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double v = coords[i];
    xyz[i] = (float)v;
    const int k = (int)(i % 9);
    if (k >= 3 && k < 6) ca[(i / 9) * 3 + (k - 3)] = v;
  }
}

// the same value on every lane: the two operands of each level are the same pair on both lanes, and a + b == b + a
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double weighted_sum(const SteerWeights& wt, const double t[4]) {
#pragma clang fp contract(off)
  double r = wt.w[0] * t[0];
  r = r + wt.w[1] * t[1];
  r = r + wt.w[2] * t[2];
  r = r + wt.w[3] * t[3];
  return r;
}

// one wave per particle
__global__ __launch_bounds__(64) void steer_terms_kernel(const double* __restrict__ ca, const signed char* __restrict__ sse,
                                                         const int* __restrict__ clashes, const int* __restrict__ offsets,
                                                         const int* __restrict__ lens, SteerWeights wt, double* __restrict__ terms,
                                                         double* __restrict__ reward) {
  const int b = blockIdx.x, lane = threadIdx.x, n = lens[b];
  const size_t row0 = (size_t)offsets[b];
  const double* __restrict__ p = ca + row0 * 3;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int helix = 0, strand = 0;
  for (int i = lane; i < n; i += 64) {
    sx += p[i * 3]; sy += p[i * 3 + 1]; sz += p[i * 3 + 2];
    const signed char l = sse[row0 + i];
    helix += l == 1 ? 1 : 0;
    strand += l == 2 ? 1 : 0;
  }
  const double mx = wave_sum_f64(sx) / n, my = wave_sum_f64(sy) / n, mz = wave_sum_f64(sz) / n;
  double ss = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double dx = p[i * 3] - mx, dy = p[i * 3 + 1] - my, dz = p[i * 3 + 2] - mz;
    ss += dx * dx + dy * dy + dz * dz;
  }
  ss = wave_sum_f64(ss);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    helix += __shfl_xor(helix, o, 64);
    strand += __shfl_xor(strand, o, 64);
  }
  if (lane == 0) {
    const double t[4] = {(double)clashes[b], sqrt(ss / n), (double)helix / (double)n, (double)strand / (double)n};
    for (int k = 0; k < 4; ++k) terms[(size_t)b * 4 + k] = t[k];
    reward[b] = weighted_sum(wt, t);
  }
}

constexpr int kResampleThreads = 256;

__global__ __launch_bounds__(kResampleThreads) void steer_resample_kernel(const double* __restrict__ reward, double* __restrict__ logw,
                                                                          double* __restrict__ r_prev, int P, double lambda,
                                                                          double ess_frac, const double* __restrict__ u,
                                                                          int* __restrict__ ancestors,
                                                                          unsigned char* __restrict__ resampled) {
#pragma clang fp contract(off)
  __shared__ double w[kSteerMaxParticles];    // the new log-weights, then the weights
  __shared__ double cum[kSteerMaxParticles];  // w_0 + .. + w_j
  __shared__ double rp[kSteerMaxParticles];   // the rewards of this event, r_prev's new values before the permutation
  __shared__ double head[2];                  // max log-weight; W
  __shared__ int decide;
  const int g = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)g * P;
  for (int k = tid; k < P; k += kResampleThreads) {
    const double r = reward[base + k];
    const double step = lambda * (r - r_prev[base + k]);
    w[k] = logw[base + k] + step;
    rp[k] = r;
  }
  __syncthreads();
  if (tid == 0) {
    double mx = w[0];
    for (int j = 1; j < P; ++j) mx = w[j] > mx ? w[j] : mx;
    head[0] = mx;
  }
  __syncthreads();
  const double mx = head[0];
  for (int k = tid; k < P; k += kResampleThreads) {
    const double lw = w[k];
    logw[base + k] = lw;
    w[k] = exp(lw - mx);
  }
  __syncthreads();
  if (tid == 0) {
    double W = 0.0, S2 = 0.0;
    for (int j = 0; j < P; ++j) {
      W = W + w[j];
      cum[j] = W;
      S2 = S2 + w[j] * w[j];
    }
    const bool usable = W > 0.0 && W <= 1.7976931348623157e308;  // finite and positive (a NaN fails both)
    const double ess = W * W / S2;
    decide = usable && (ess_frac >= 1.0 || ess < ess_frac * (double)P) ? 1 : 0;
    head[1] = W;
    resampled[g] = (unsigned char)decide;
  }
  __syncthreads();
  const bool go = decide != 0;
  const double W = head[1], ug = u[g];
  for (int k = tid; k < P; k += kResampleThreads) {
    int a = k;
    if (go) {
      const double target = (ug + (double)k) / (double)P * W;
      // cum is non-decreasing (every w_j >= 0): the smallest j with cum[j] > target, P - 1 if none
      int lo = 0, hi = P - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > target) hi = mid;
        else lo = mid + 1;
      }
      a = lo;
      logw[base + k] = 0.0;
    }
    r_prev[base + k] = rp[a];
    ancestors[base + k] = (int)base + a;
  }
}

__global__ __launch_bounds__(256) void steer_gather_kernel(const float* __restrict__ x, const int* __restrict__ ancestors,
                                                           float* __restrict__ x_new, long long row) {
  const int b = blockIdx.x;
  const float* __restrict__ src = x + (size_t)ancestors[b] * row;
  float* __restrict__ dst = x_new + (size_t)b * row;
  for (long long i = threadIdx.x; i < row; i += 256) dst[i] = src[i];
}

unsigned blocks_for(long long n) {
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

}  // namespace

void launch_steer_shift(const float* x0, const int* lens, int B, int L, int F, const SteerOffset& off, unsigned angle_mask,
                        float* ang, hipStream_t s) {
  const long long n = (long long)B * L * F;
  hipLaunchKernelGGL(steer_shift_kernel, dim3(blocks_for(n)), dim3(256), 0, s, x0, lens, n, L, F, off, angle_mask, ang);
}

void launch_steer_rewards(const float* ang, const int* lens, int B, int L, int F, const NerfFeatures& fx, const SteerWeights& wt,
                          double alpha, int max_len, const SteerWork& wk, double* terms, double* reward, hipStream_t s) {
  launch_nerf(ang, lens, B, L, F, fx, 0, wk.coords, s);
  const long long n_res = (long long)B * L;
  hipLaunchKernelGGL(steer_atoms_kernel, dim3(blocks_for(n_res * 9)), dim3(256), 0, s, wk.coords, n_res, wk.xyz, wk.ca);
  launch_backbone_clashes(wk.xyz, wk.offsets, lens, B, alpha, wk.clashes, nullptr, s);
  launch_psea(wk.ca, wk.offsets, lens, B, max_len, wk.sse, wk.sse_runs, s);
  hipLaunchKernelGGL(steer_terms_kernel, dim3(B), dim3(64), 0, s, wk.ca, wk.sse, wk.clashes, wk.offsets, lens, wt, terms, reward);
}

void launch_steer_resample(const double* reward, double* logw, double* r_prev, int G, int P, double lambda, double ess_frac,
                           const double* u, int* ancestors, unsigned char* resampled, hipStream_t s) {
  hipLaunchKernelGGL(steer_resample_kernel, dim3(G), dim3(kResampleThreads), 0, s, reward, logw, r_prev, P, lambda, ess_frac, u,
                     ancestors, resampled);
}

void launch_steer_gather(const float* x, const int* ancestors, float* x_new, int B, long long row, hipStream_t s) {
  hipLaunchKernelGGL(steer_gather_kernel, dim3(B), dim3(256), 0, s, x, ancestors, x_new, row);
}

}  // namespace fdmi
