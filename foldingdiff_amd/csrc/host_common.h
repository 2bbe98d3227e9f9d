// Host-only helpers shared by the C-ABI sources (api.hip: the model as it runs; api_weights.hip: its weights; api_comm.hip:
// its RCCL binding; api_run.hip: the entries that run it; api_structures.hip: the structure entries; api_hooks.hip: the test
// hooks): the error string, the owner of device buffers
// that live for one call, the synchronous round trip built on it, and the argument checks of the packed-chain entries and of restraint guidance.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fdmi.h"

namespace fdmi {

// sets the calling thread's error string (fd_last_error) and returns `code`; defined once, in api.hip
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return ::fdmi::fail(FD_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                              __FILE__, __LINE__);                                  \
  } while (0)

// Device buffers that live for one call: freed when the owner goes out of scope, on every path.
class DeviceBufs {
 public:
  DeviceBufs() = default;
  DeviceBufs(const DeviceBufs&) = delete;
  DeviceBufs& operator=(const DeviceBufs&) = delete;
  ~DeviceBufs() {
    for (void* p : bufs_) (void)hipFree(p);
  }
  template <typename T>
  hipError_t alloc(size_t bytes, T** dev) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) bufs_.push_back(p);
    *dev = static_cast<T*>(p);
    return e;
  }
  template <typename T>
  hipError_t upload(const void* host, size_t bytes, T** dev) {
    const hipError_t e = alloc(bytes, dev);
    return e != hipSuccess ? e : hipMemcpy(const_cast<std::remove_const_t<T>*>(*dev), host, bytes, hipMemcpyHostToDevice);
  }
  template <typename T>
  hipError_t zeros(size_t bytes, T** dev) {
    const hipError_t e = alloc(bytes, dev);
    return e != hipSuccess ? e : hipMemset(*dev, 0, bytes);
  }

 private:
  std::vector<void*> bufs_;
};

// the device buffers of a round trip as its launch sees them: in(i) / out(i) convert to the pointer type the launch
// wrapper's parameter asks for (an input to pointers to const only)
struct RoundtripBufs {
  struct In {
    const void* p;
    template <typename T>
    operator const T*() const { return static_cast<const T*>(p); }
  };
  struct Out {
    void* p;
    template <typename T>
    operator T*() const { return static_cast<T*>(p); }
  };
  std::vector<void*> ins, outs;
  In in(size_t i) const { return In{ins[i]}; }
  Out out(size_t i) const { return Out{outs[i]}; }
};

// one synchronous device round trip: inputs up, the launch, the outputs down; an output with a null host pointer is a
// device workspace (or an optional output nobody asked for) that stays there and is not zero-filled.  The launch gets
// the device buffers and may return a hipError_t.
template <typename Launch>
int device_roundtrip(int device_id, std::initializer_list<std::pair<const void*, size_t>> inputs,
                     std::initializer_list<std::pair<void*, size_t>> outputs, Launch launch) {
  HIP_TRY(hipSetDevice(device_id));
  DeviceBufs bufs;
  RoundtripBufs d;
  for (auto& in : inputs) {
    void* p;
    HIP_TRY(bufs.upload(in.first, in.second, &p));
    d.ins.push_back(p);
  }
  for (auto& out : outputs) {
    void* p;
    HIP_TRY(bufs.alloc(out.second, &p));
    d.outs.push_back(p);
  }
  if constexpr (std::is_void_v<decltype(launch(d))>) {
    launch(d);
  } else {
    HIP_TRY(launch(d));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  size_t k = 0;
  for (auto& out : outputs) {
    if (out.first) HIP_TRY(hipMemcpy(out.first, d.outs[k], out.second, hipMemcpyDeviceToHost));
    ++k;
  }
  return FD_OK;
}

// lens[i] in [1, cap] (the padded length of a batch, or the most residues a kernel takes); *max_len = the longest
inline int check_lens(const int32_t* lens, int n, int cap, int* max_len = nullptr) {
  int longest = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] < 1 || lens[i] > cap) return fail(FD_E_INVALID, "lens[%d]=%d outside [1, %d]", i, lens[i], cap);
    if (lens[i] > longest) longest = lens[i];
  }
  if (max_len) *max_len = longest;
  return FD_OK;
}

// chains / pairs packed back to back: offsets[c] = lens[0] + ... + lens[c-1]; *total = the sum of all lengths
inline int check_packed(const int32_t* offsets, const int32_t* lens, int n, long long limit, long long* total) {
  long long sum = 0;
  for (int c = 0; c < n; ++c) sum += lens[c] > 0 ? lens[c] : 0;
  if (sum > limit) return fail(FD_E_UNSUPPORTED, "%lld entries in total, at most %lld", sum, limit);
  long long at = 0;
  for (int c = 0; c < n; ++c) {
    if (lens[c] < 1) return fail(FD_E_INVALID, "lens[%d]=%d must be >= 1", c, lens[c]);
    if (offsets[c] < 0 || (long long)offsets[c] + lens[c] > sum)
      return fail(FD_E_INVALID, "offsets[%d]=%d (length %d) outside the buffer of %lld entries", c, offsets[c], lens[c], sum);
    if (offsets[c] != at)
      return fail(FD_E_INVALID, "offsets[%d]=%d, expected %lld (entries are packed back to back in order)", c, offsets[c], at);
    at += lens[c];
  }
  *total = sum;
  return FD_OK;
}

// packed coordinates [sum lens][3] (check_packed has passed): every one finite and within 1e6 A, so that every squared
// distance stays far from overflow.  With `cent`: chain c's centroid goes to cent[c * cent_stride .. + 2] (the TM kernels
// work on each trace in its own centred frame).
inline int check_coords(const double* xyz, const int32_t* offsets, const int32_t* lens, int n, double* cent = nullptr,
                        int cent_stride = 3) {
  for (int c = 0; c < n; ++c) {
    double sum[3] = {0.0, 0.0, 0.0};
    for (int i = offsets[c]; i < offsets[c] + lens[c]; ++i)
      for (int d = 0; d < 3; ++d) {
        const double u = xyz[(size_t)i * 3 + d];
        if (!(std::fabs(u) <= 1e6))
          return fail(FD_E_INVALID, "coordinate %d of residue %d (chain %d) is not finite or beyond 1e6: %g", d, i, c, u);
        sum[d] += u;
      }
    if (cent)
      for (int d = 0; d < 3; ++d) cent[(size_t)c * cent_stride + d] = sum[d] / lens[c];
  }
  return FD_OK;
}

// packed float64 backbones with `per` atoms to a residue ([sum lens][per][3], check_packed has passed): every coordinate finite
// and within 1e6 A; with nan_atom >= 0 that atom's coordinates may also be NaN (a residue without it)
inline int check_backbone(const double* xyz, const int32_t* offsets, const int32_t* lens, int n, int per, int nan_atom = -1) {
  for (int c = 0; c < n; ++c)
    for (int i = offsets[c]; i < offsets[c] + lens[c]; ++i)
      for (int a = 0; a < per; ++a)
        for (int d = 0; d < 3; ++d) {
          const double u = xyz[((size_t)i * per + a) * 3 + d];
          if (!(std::fabs(u) <= 1e6) && !(a == nan_atom && std::isnan(u)))
            return fail(FD_E_INVALID, "coordinate %d of atom %d of residue %d (chain %d) is not finite or beyond 1e6: %g", d, a, i, c, u);
        }
  return FD_OK;
}

// the same for packed float32 coordinates with `per` atoms to an entry ([sum lens][per][3]); names the atom and its chain
inline int check_coords_f32(const float* xyz, const int32_t* offsets, const int32_t* lens, int n, int per) {
  for (int c = 0; c < n; ++c)
    for (long long i = (long long)offsets[c] * per; i < ((long long)offsets[c] + lens[c]) * per; ++i)
      for (int d = 0; d < 3; ++d) {
        const float u = xyz[(size_t)i * 3 + d];
        if (!(std::fabs(u) <= 1e6f))
          return fail(FD_E_INVALID, "coordinate %d of atom %lld (chain %d) is not finite or beyond 1e6: %g", d, i, c, (double)u);
      }
  return FD_OK;
}

// at most FDMI_PAIRCOUNT_MAX_ATOMS atoms in every structure of a packed call with `per` atoms to an entry
inline int check_atom_cap(const int32_t* lens, int n, int per) {
  for (int c = 0; c < n; ++c)
    if ((long long)lens[c] * per > FDMI_PAIRCOUNT_MAX_ATOMS)
      return fail(FD_E_UNSUPPORTED, "lens[%d]=%d: %lld atoms, at most %d in one structure", c, lens[c], (long long)lens[c] * per,
                  FDMI_PAIRCOUNT_MAX_ATOMS);
  return FD_OK;
}

// the pairwise-distance term's own arguments (fd_pairwise_dist, fd_denoise_loss_ex): the padded length the kernel takes,
// six distinct feature columns, a denoising divisor that is not 0, positive weights
inline int check_pairwise(const float* keep, const float* coef, const int32_t* feat_idx, int B, int L, int F) {
  if (L > FDMI_PAIRWISE_MAX_LEN) return fail(FD_E_UNSUPPORTED, "L=%d: the pairwise-distance term takes L <= %d", L, FDMI_PAIRWISE_MAX_LEN);
  for (int i = 0; i < 6; ++i) {
    if (feat_idx[i] < 0 || feat_idx[i] >= F) return fail(FD_E_INVALID, "feat_idx[%d]=%d outside [0, %d)", i, feat_idx[i], F);
    for (int j = 0; j < i; ++j)
      if (feat_idx[j] == feat_idx[i]) return fail(FD_E_INVALID, "feat_idx[%d]=%d repeats feat_idx[%d]", i, feat_idx[i], j);
  }
  for (int b = 0; b < B; ++b) {
    if (!(keep[b] != 0.f) || !std::isfinite(keep[b])) return fail(FD_E_INVALID, "keep[%d]=%g must be finite and not 0", b, (double)keep[b]);
    if (coef && !(coef[b] > 0.f)) return fail(FD_E_INVALID, "coef[%d]=%g must be > 0", b, (double)coef[b]);
  }
  return FD_OK;
}

// what fd_steer_rewards and fd_sample_steered ask of a rewards pass: lengths the P-SEA kernel takes, a feature count the
// shift kernel takes, fd_nerf's columns, finite weights and offsets, a positive clash factor
inline int check_steer(const int32_t* lens, int B, int L, int F, const int32_t* feat_idx, const double* weights, double clash_alpha,
                       const float* offset) {
  if (F < 3 || F > 16) return fail(FD_E_INVALID, "F=%d outside [3, 16]", F);
  if ((long long)B * L * F > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * F = %lld elements, at most 2^31 - 1", (long long)B * L * F);
  if (int rc = check_lens(lens, B, L < FDMI_SSE_MAX_LEN ? L : FDMI_SSE_MAX_LEN)) return rc;
  for (int i = 0; i < 9; ++i)
    if (feat_idx[i] >= F || (i < 3 && feat_idx[i] < 0)) return fail(FD_E_INVALID, "feat_idx[%d]=%d (F=%d)", i, feat_idx[i], F);
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(weights[k])) return fail(FD_E_INVALID, "weights[%d]=%g must be finite", k, weights[k]);
  if (!(clash_alpha > 0.0) || !std::isfinite(clash_alpha)) return fail(FD_E_INVALID, "clash_alpha=%g must be > 0 and finite", clash_alpha);
  for (int f = 0; offset && f < F; ++f)
    if (!std::isfinite(offset[f])) return fail(FD_E_INVALID, "offset[%d]=%g must be finite", f, (double)offset[f]);
  return FD_OK;
}

// the uniforms of systematic resampling: each in [0, 1)
inline int check_steer_u(const double* u, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(u[i] >= 0.0 && u[i] < 1.0)) return fail(FD_E_INVALID, "u[%zu]=%g outside [0, 1)", i, u[i]);
  return FD_OK;
}

// the ties of fd_tie_repeats and fd_sample_repeat (check_lens has passed): tie[b] = start | period | units with start >= 0,
// period >= 1, units >= 1 and the tied rows [start, start + period * units) below lens[b]
inline int check_tie(const int32_t* tie, const int32_t* lens, int B) {
  for (int b = 0; b < B; ++b) {
    const int32_t start = tie[3 * b], period = tie[3 * b + 1], units = tie[3 * b + 2];
    if (start < 0 || period < 1 || units < 1)
      return fail(FD_E_INVALID, "tie[%d] = (%d, %d, %d): start >= 0, period >= 1 and units >= 1", b, start, period, units);
    if ((long long)start + (long long)period * units > lens[b])
      return fail(FD_E_INVALID, "tie[%d] = (%d, %d, %d) ends at row %lld, beyond lens[%d] = %d", b, start, period, units,
                  (long long)start + (long long)period * units, b, lens[b]);
  }
  return FD_OK;
}

// ---- restraint guidance (fd_nerf_vjp, fd_restraint_energy, fd_guide_step, fd_sample_guided)
// lengths the one-workgroup-per-chain kernels take, a feature count the shift kernel takes, fd_nerf's columns with no column
// named twice (the derivative stores one result per element)
inline int check_guide_shape(const int32_t* lens, int B, int L, int F, const int32_t* feat_idx) {
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (F < 3 || F > 16) return fail(FD_E_INVALID, "F=%d outside [3, 16]", F);
  if ((long long)B * L * F > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * F = %lld elements, at most 2^31 - 1", (long long)B * L * F);
  if (int rc = check_lens(lens, B, L < 2048 ? L : 2048)) return rc;
  for (int i = 0; i < 9; ++i) {
    if (feat_idx[i] >= F || feat_idx[i] < -1 || (i < 3 && feat_idx[i] < 0)) return fail(FD_E_INVALID, "feat_idx[%d]=%d (F=%d)", i, feat_idx[i], F);
    for (int j = 0; j < i; ++j)
      if (feat_idx[i] >= 0 && feat_idx[j] == feat_idx[i]) return fail(FD_E_INVALID, "feat_idx[%d]=%d repeats feat_idx[%d]", i, feat_idx[i], j);
  }
  return FD_OK;
}

// [B][3L][3] doubles (fd_nerf's layout), finite on the atoms below 3 lens[b]; `what` names the array
inline int check_chain_doubles(const char* what, const double* v, const int32_t* lens, int B, int L) {
  for (int b = 0; b < B; ++b)
    for (size_t i = (size_t)b * L * 9; i < ((size_t)b * L + lens[b]) * 9; ++i)
      if (!std::isfinite(v[i])) return fail(FD_E_INVALID, "%s is not finite at chain %d, atom %d", what, b, (int)(i / 3 - (size_t)b * L * 3));
  return FD_OK;
}

// [B][L][F] floats, finite on the rows below lens[b]
inline int check_rows_finite(const char* what, const float* v, const int32_t* lens, int B, int L, int F) {
  for (int b = 0; b < B; ++b)
    for (size_t i = (size_t)b * L * F; i < ((size_t)b * L + lens[b]) * F; ++i)
      if (!std::isfinite(v[i])) return fail(FD_E_INVALID, "%s is not finite at sequence %d, position %d", what, b, (int)(i / F - (size_t)b * L));
  return FD_OK;
}

// a batch's packed distance restraints as the host hands them over (check_lens has passed)
struct RestraintLists {
  int n_chains;
  const int32_t *offsets, *i, *j;
  const double *d0, *tol, *w;
  size_t count() const { return (size_t)offsets[n_chains]; }  // (once check_restraints has passed)
};
inline int check_restraints(const RestraintLists& r, const int32_t* lens) {
  const int B = r.n_chains;
  if (!r.offsets) return fail(FD_E_INVALID, "null argument: rst_offsets");
  if (r.offsets[0] != 0) return fail(FD_E_INVALID, "rst_offsets[0]=%d must be 0", r.offsets[0]);
  for (int b = 0; b < B; ++b)
    if (r.offsets[b + 1] < r.offsets[b]) return fail(FD_E_INVALID, "rst_offsets[%d]=%d is below rst_offsets[%d]=%d", b + 1, r.offsets[b + 1], b, r.offsets[b]);
  if (r.offsets[B] > 0 && (!r.i || !r.j || !r.d0 || !r.tol || !r.w)) return fail(FD_E_INVALID, "null argument: the restraint lists");
  for (int b = 0; b < B; ++b)
    for (int k = r.offsets[b]; k < r.offsets[b + 1]; ++k) {
      const int n = 3 * lens[b];
      if (r.i[k] < 0 || r.i[k] >= n || r.j[k] < 0 || r.j[k] >= n)
        return fail(FD_E_INVALID, "restraint %d = atoms (%d, %d) outside chain %d's [0, %d)", k, r.i[k], r.j[k], b, n);
      if (r.i[k] == r.j[k]) return fail(FD_E_INVALID, "restraint %d names atom %d twice", k, r.i[k]);
      if (!(r.d0[k] >= 0.0) || !std::isfinite(r.d0[k])) return fail(FD_E_INVALID, "restraint %d: d0=%g must be >= 0 and finite", k, r.d0[k]);
      if (!(r.tol[k] >= 0.0) || !std::isfinite(r.tol[k])) return fail(FD_E_INVALID, "restraint %d: tol=%g must be >= 0 and finite", k, r.tol[k]);
      if (!(r.w[k] >= 0.0) || !std::isfinite(r.w[k])) return fail(FD_E_INVALID, "restraint %d: w=%g must be >= 0 and finite", k, r.w[k]);
    }
  return FD_OK;
}

// the guide statement's own scalars and its shift
inline int check_guide_scalars(double max_norm, const float* offset, int F) {
  if (!(max_norm > 0.0) || !std::isfinite(max_norm)) return fail(FD_E_INVALID, "max_norm=%g must be > 0 and finite", max_norm);
  for (int f = 0; offset && f < F; ++f)
    if (!std::isfinite(offset[f])) return fail(FD_E_INVALID, "offset[%d]=%g must be finite", f, (double)offset[f]);
  return FD_OK;
}

// what fd_scaffold_guide_step and fd_sample_guided_inpaint ask beyond fd_guide_step's checks (check_lens has passed; known and
// fixed are not null): the statement's scalars, nothing fixed at or beyond a length, known finite where fixed
inline int check_scaffold_guide(const fd_scaffold_guide_params& p, const float* known, const uint8_t* fixed, const int32_t* lens,
                                int B, int L, int F) {
  if (int rc = check_guide_scalars(p.max_norm, p.has_offset ? p.offset : nullptr, F)) return rc;
  const struct { const char* name; double v; } clash[] = {{"clash_alpha", p.clash_alpha}, {"clash_margin", p.clash_margin}, {"w_clash", p.w_clash}};
  for (const auto& w : clash)
    if (!(w.v >= 0.0) || !std::isfinite(w.v)) return fail(FD_E_INVALID, "%s=%g must be >= 0 and finite", w.name, w.v);
  for (int b = 0; b < B; ++b)
    for (int l = 0; l < L; ++l)
      for (int f = 0; f < F; ++f) {
        const size_t o = ((size_t)b * L + l) * F + f;
        if (!fixed[o]) continue;
        if (l >= lens[b]) return fail(FD_E_INVALID, "fixed element beyond a length: sequence %d position %d feature %d, lens[%d] = %d", b, l, f, b, lens[b]);
        if (!std::isfinite(known[o])) return fail(FD_E_INVALID, "known is not finite at a fixed element: sequence %d position %d feature %d", b, l, f);
      }
  return FD_OK;
}

// ---- superposition restraints (fd_template_energy, fd_scaffold_guide_step_tpl, fd_sample_guided_inpaint_tpl)
// a batch's packed templates as the host hands them over (check_lens has passed); all four null: no template
struct TemplateLists {
  int n_chains;
  const int32_t *offsets, *atom;
  const double *xyz, *w;
  bool none() const { return !offsets; }
  size_t count() const { return none() ? 0 : (size_t)offsets[n_chains]; }  // (once check_template has passed)
};
inline int check_template(const TemplateLists& t, const int32_t* lens) {
  const int B = t.n_chains;
  const int given = (t.offsets ? 1 : 0) + (t.atom ? 1 : 0) + (t.xyz ? 1 : 0) + (t.w ? 1 : 0);
  if (given == 0) return FD_OK;
  if (given != 4) return fail(FD_E_INVALID, "null argument: tpl_offsets, tpl_atom, tpl_xyz and tpl_w are given together or not at all");
  if (t.offsets[0] != 0) return fail(FD_E_INVALID, "tpl_offsets[0]=%d must be 0", t.offsets[0]);
  for (int b = 0; b < B; ++b)
    if (t.offsets[b + 1] < t.offsets[b]) return fail(FD_E_INVALID, "tpl_offsets[%d]=%d is below tpl_offsets[%d]=%d", b + 1, t.offsets[b + 1], b, t.offsets[b]);
  for (int b = 0; b < B; ++b)
    for (int k = t.offsets[b]; k < t.offsets[b + 1]; ++k) {
      const int n = 3 * lens[b];
      if (t.atom[k] < 0 || t.atom[k] >= n) return fail(FD_E_INVALID, "template entry %d = atom %d outside chain %d's [0, %d)", k, t.atom[k], b, n);
      if (k > t.offsets[b] && t.atom[k] <= t.atom[k - 1])
        return fail(FD_E_INVALID, "template entry %d = atom %d after atom %d: a chain's atoms are strictly increasing", k, t.atom[k], t.atom[k - 1]);
      if (!(t.w[k] > 0.0) || !std::isfinite(t.w[k])) return fail(FD_E_INVALID, "template entry %d: w=%g must be > 0 and finite", k, t.w[k]);
      for (int d = 0; d < 3; ++d)
        if (!std::isfinite(t.xyz[(size_t)k * 3 + d])) return fail(FD_E_INVALID, "template entry %d: target coordinate %d is not finite", k, d);
    }
  return FD_OK;
}

// ---- cyclic oligomers (fd_symmetry_energy, fd_symmetry_dock, fd_scaffold_guide_step_sym)
// the statement's scalars, the orders (null: not looked at) and the poses (null: not looked at; only chains with order >= 2 are read)
inline int check_symmetry(const fd_symmetry_params& p, const int32_t* order, const double* pose, int B) {
  const struct { const char* name; double v; } nonneg[] = {{"clash_alpha", p.clash_alpha}, {"clash_margin", p.clash_margin}, {"w_clash", p.w_clash},
                                                           {"w_contact", p.w_contact}, {"w_radial", p.w_radial}, {"r_max", p.r_max}};
  for (const auto& w : nonneg)
    if (!(w.v >= 0.0) || !std::isfinite(w.v)) return fail(FD_E_INVALID, "%s=%g must be >= 0 and finite", w.name, w.v);
  if (!(p.d_on >= 0.0) || !(p.d_on < p.d_off) || !std::isfinite(p.d_off)) return fail(FD_E_INVALID, "d_on=%g, d_off=%g: 0 <= d_on < d_off, both finite", p.d_on, p.d_off);
  const struct { const char* name; double v; } pos[] = {{"lever", p.lever}, {"max_shift", p.max_shift}, {"step0", p.step0}};
  for (const auto& w : pos)
    if (!(w.v > 0.0) || !std::isfinite(w.v)) return fail(FD_E_INVALID, "%s=%g must be > 0 and finite", w.name, w.v);
  if (!(p.grow >= 1.0) || !std::isfinite(p.grow)) return fail(FD_E_INVALID, "grow=%g must be >= 1 and finite", p.grow);
  if (!(p.shrink > 0.0 && p.shrink < 1.0)) return fail(FD_E_INVALID, "shrink=%g outside (0, 1)", p.shrink);
  if (p.pose_iters < 0) return fail(FD_E_INVALID, "pose_iters=%d must be >= 0", p.pose_iters);
  for (int b = 0; order && b < B; ++b)
    if (order[b] < 1 || order[b] > 12) return fail(FD_E_INVALID, "order[%d]=%d outside [1, 12]", b, order[b]);
  for (int b = 0; pose && b < B; ++b)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(pose[(size_t)b * 12 + i])) return fail(FD_E_INVALID, "pose[%d][%d]=%g is not finite", b, i, pose[(size_t)b * 12 + i]);
  return FD_OK;
}

}  // namespace fdmi
