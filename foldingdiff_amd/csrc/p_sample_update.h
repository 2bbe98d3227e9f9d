// The p_sample update of one element (K9), written once for the two fp32 head + update kernels, head_update_kernel and
// head_update16_kernel (rowwise.hip).  The kernels load a row, normalise it, run dense2 and write eps_out; what happens to the
// prediction after that is here.  head_update_img_kernel (rowwise_img.hip) still carries its own copy of the same statement
// (DESIGN.md 6v says why): a change to the statement is made here AND there, and the bit-for-bit tests of the three kernels
// against each other's hooks (tests/test_feature_sets_gpu.py parts A and C) hold the two together.
//
// A launch runs one of four statements, chosen by UpdateArgs and, where set, the tables of UpdateDyn (fdmi_kernels.h):
//   plain    x' = c1[t] * (x - beta[t] * eps / c3[t]) + (t > 0 ? sigma[t] * z : 0)           foldingdiff/sampling.py:62-75
//            (model_mean = sqrt_recip_alphas_t * (x - betas_t * eps / sqrt_one_minus_alphas_cumprod_t), :62-67)
//   strided  x' = a x + b eps (+ s z where s != 0): strided_update.h; z is neither read nor drawn where s == 0.
//            By value (`strided`, sa, sb, ss: fd_p_sample_step_coef) or dyn's abs at t (fd_sample_strided)
//   steered  the strided statement, and the visit's x0 = u x + v eps (solver_update.h's x0 statement) goes to x0_out; x' does
//            not depend on it.  By value (`strided` == 2: fd_p_sample_step_coef_x0) or dyn's uv and x0_steer (fd_sample_steered)
//   solver   the strided mean, corrected by c * wrap(x0 - prev); no draw: solver_update.h.
//            By value (x0_out set and `strided` == 1: fd_p_sample_step_solver) or dyn's cuv and x0_prev (fd_sample_solver)
// each wrapped to [-pi, pi) where the feature is an angle (sampling.py:119-130, utils.py:100-106; wrap_pi.h).  A FIXED element
// (inpaint_replace.h) takes none of them: it leaves step t at level t, whatever the model predicted -- a strided visit: at the
// level it lands on, next_t[t] + 1, with the known_noise row of the visit, ord[t] + 1.
// z = noise[row][o], row = t (a strided run: the visit's ordinal), or the Philox draw of (seed, t, sequence, position, feature).
// x' goes to x_out and, every hist_every-th state and the last one, to hist: state j of the run goes to row j / hist_every,
// j = t_start - t (a strided run: the visit's ordinal).
#pragma once
#include "fdmi_kernels.h"
#include "inpaint_replace.h"
#include "philox_normal.h"
#include "solver_update.h"
#include "strided_update.h"
#include "wrap_pi.h"

namespace fdmi {

// INVARIANT: every pointer member of UpdateArgs and UpdateDyn (fdmi_kernels.h) is null or points into device (global) memory --
// never LDS, never a kernel's stack.  fill_update and the run entries only ever put hipMalloc'ed buffers there.  A member added
// to either struct must keep to that, because the types below say it to the compiler: an address-space-1 pointer to anything
// else reads the wrong memory.
// Why the types are needed: the compiler works the address space out for itself for a pointer that a kernel's own body reads
// from its arguments, but not for one that reaches its use through UpdateVisit.  Every access through such a pointer then takes
// the generic path (flat loads and stores), and the entries of the step tables are fetched per lane and stay in vector registers
// across a row loop (head_update16_kernel<1>: 73 registers instead of 56, 6 waves per SIMD instead of 8).
// a.coef, a.x, a.x_out, a.eps_out and a.angle_mask are deliberately NOT wrapped: update_element and the kernels read them
// straight from the by-value kernel argument, where the compiler does infer the address space (the kernels hold no flat access).
// The casts back to generic pointers at the calls of inpaint_value_row and solver_update rely on the inliner carrying the address
// space through; nothing but the instruction counts in DESIGN.md 6v guards that, so recount flat_ accesses after touching them.
template <typename T>
using device_ptr_t = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ device_ptr_t<T> device_ptr(T* p) {
  return (device_ptr_t<T>)p;
}

// What a launch does at step t, resolved once per kernel: every member is the same for all threads.
struct UpdateVisit {
  int t;
  bool strided, solver;
  int ord, t_next;       // a strided run: the visit's ordinal and the next visit's t (-1 behind the last)
  int level, known_row;  // what a fixed element leaves at, and its row of known_noise
  device_ptr_t<const float> noise;
  device_ptr_t<float> hist;
  unsigned long long seed;
  long long seq_offset;
  int t_start, hist_every;
  device_ptr_t<const float> known, known_noise, known_coef;
  device_ptr_t<const unsigned char> fixed;
  float c1, bt, c3, sg;          // plain: the rows of coef at t
  float sa, sb, ss, sc, su, sv;  // strided (a, b, s), solver (c, u, v), steered (u, v)
  device_ptr_t<const float> x0_prev;
  device_ptr_t<float> x0_out;
};

// live: x_out is set.  A forward-only launch resolves too where the kernel does so in front of its row loop; it reads
// neither coef nor the step tables.
__device__ __forceinline__ UpdateVisit resolve_update(const UpdateArgs& a, int t, bool live) {
  UpdateVisit m;
  m.t = t;
  m.noise = device_ptr(a.noise); m.hist = device_ptr(a.hist); m.seed = a.seed; m.seq_offset = a.seq_offset;
  m.t_start = a.t_start; m.hist_every = 1;
  m.known = device_ptr(a.known); m.known_noise = device_ptr(a.known_noise); m.known_coef = device_ptr(a.known_coef);
  m.fixed = device_ptr(a.fixed);
  if (a.dyn) {  // the per-call values that a captured graph must not bake in (see UpdateDyn)
    m.noise = device_ptr(a.dyn->noise); m.hist = device_ptr(a.dyn->hist);
    m.seed = a.dyn->seed; m.seq_offset = a.dyn->seq_offset; m.t_start = a.dyn->t_start;
    m.hist_every = a.dyn->hist_every > 1 ? a.dyn->hist_every : 1;
    m.known = device_ptr(a.dyn->known); m.known_noise = device_ptr(a.dyn->known_noise); m.known_coef = device_ptr(a.dyn->known_coef);
    m.fixed = device_ptr(a.dyn->fixed);
  }
  m.strided = a.strided != 0;
  m.sa = a.sa; m.sb = a.sb; m.ss = a.ss;
  m.ord = 0; m.t_next = -1;
  m.solver = a.x0_out != nullptr && a.strided != 2;  // (strided == 2: a steered visit, which only writes x0 to x0_out)
  m.sc = a.sc; m.su = a.su; m.sv = a.sv;
  m.x0_prev = device_ptr(a.x0_prev); m.x0_out = device_ptr(a.x0_out);
  m.level = m.strided ? a.level_out : t; m.known_row = m.level;
  if (live && a.dyn && a.dyn->next_t) {  // a run with step tables
    const int T = a.T;
    m.strided = true;
    m.t_next = device_ptr(a.dyn->next_t)[t]; m.ord = device_ptr(a.dyn->ord)[t];
    m.level = m.t_next + 1; m.known_row = m.ord + 1;
    m.sa = device_ptr(a.dyn->abs)[t]; m.sb = device_ptr(a.dyn->abs)[T + t]; m.ss = device_ptr(a.dyn->abs)[2 * T + t];
    if (a.dyn->cuv) {
      m.solver = true;
      m.sc = device_ptr(a.dyn->cuv)[t]; m.su = device_ptr(a.dyn->cuv)[T + t]; m.sv = device_ptr(a.dyn->cuv)[2 * T + t];
      m.x0_prev = m.x0_out = device_ptr(a.dyn->x0_prev);
    } else if (a.dyn->uv) {  // a steered run: the visit also writes its x0
      m.su = device_ptr(a.dyn->uv)[t]; m.sv = device_ptr(a.dyn->uv)[T + t];
      m.x0_out = device_ptr(a.dyn->x0_steer);
    }
  }
  m.c1 = 0.f; m.bt = 0.f; m.c3 = 1.f; m.sg = 0.f;
  if (live) { m.c1 = a.coef[t]; m.bt = a.coef[a.T + t]; m.c3 = a.coef[2 * a.T + t]; m.sg = a.coef[3 * a.T + t]; }
  return m;
}

// Element o = (sequence b, position l, feature f) of a state of `state_elems` elements, eps = the model's prediction for it:
// computes x' and writes x_out, x0_out where the statement has one, and the hist row.  Only where x_out is set.
__device__ __forceinline__ void update_element(const UpdateArgs& a, const UpdateVisit& m, size_t o, float eps, int b, int l, int f,
                                               size_t state_elems) {
  const int t = m.t;
  const bool angular = (a.angle_mask >> f) & 1u;
  float xn;
  if (m.fixed && m.fixed[o]) {
    // (the shared helpers take generic pointers: cast back, the compiler keeps the address space through the inlined call)
    xn = inpaint_value_row((const float*)m.known, (const float*)m.known_noise, (const float*)m.known_coef, a.T, a.noise_stride, m.level,
                           m.known_row, o, m.seed, m.seq_offset + b, l, f, angular);
  } else if (m.strided && !m.solver) {
    xn = strided_mean(m.sa, a.x[o], m.sb, eps);
    if (m.x0_out) {  // steered: x0 is the prediction, without the draw
      float p0 = strided_mean(m.su, a.x[o], m.sv, eps);
      if (angular) p0 = wrap_pi(p0);
      m.x0_out[o] = p0;
    }
    if (m.ss != 0.f) {
      const float z = m.noise ? m.noise[(size_t)m.ord * a.noise_stride + o] : philox_normal(m.seed, t, m.seq_offset + b, l, f);
      xn = strided_add_noise(xn, m.ss, z);
    }
    if (angular) xn = wrap_pi(xn);
  } else if (m.strided) {
    xn = solver_update(m.sa, a.x[o], m.sb, eps, m.sc, m.su, m.sv, (const float*)m.x0_prev + o, (float*)m.x0_out + o, angular);
  } else {
    xn = __fmul_rn(m.c1, __fsub_rn(a.x[o], __fdiv_rn(__fmul_rn(m.bt, eps), m.c3)));
    if (t > 0) {  // sampling.py:69-75
      const float z = m.noise ? m.noise[(size_t)t * a.noise_stride + o] : philox_normal(m.seed, t, m.seq_offset + b, l, f);
      xn = __fadd_rn(xn, __fmul_rn(m.sg, z));
    }
    if (angular) xn = wrap_pi(xn);
  }
  a.x_out[o] = xn;
  const int state = m.strided ? m.ord : m.t_start - t;  // the state's ordinal in the run
  const bool last = m.strided ? m.t_next < 0 : t == 0;
  if (m.hist && ((state + 1) % m.hist_every == 0 || last)) m.hist[(size_t)(state / m.hist_every) * state_elems + o] = xn;
}

}  // namespace fdmi
