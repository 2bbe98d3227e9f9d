// C-ABI host side of libfdmi.so, the entries that run a model: the forwards, the denoising losses, the autoregressive sampler,
// single reverse steps, the sampling runs (plain, motif-conditioned, resampled, strided, strided and conditioned, solver, steered,
// repeat, guided, guided and conditioned) and their device-buffer pieces.  Host code around api.hip's workspace, launch plan and step (model.h) only: every entry
// checks its arguments before its first HIP call, and the paragraphs the entries share are written once, below: make the
// workspace current and upload (open_call), download and synchronise (finish), the one-copy staging of the loss entries
// (PackedUpload), one reverse step from host arrays (host_step), the owner of a run from host arrays (HostRun: stage, begin,
// the family's own steps, finish), the ONE close of a run (close_run: nothing of a finished run stays on the handle or in the
// device's UpdateDyn, whichever family ran and however it ended) and the ONE stager of the per-timestep tables (stage_tables).
// Boundary: include/fdmi.h (each entry point cites the reference function it replaces).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/fdmi.h"
#include "fdmi_kernels.h"
#include "host_common.h"
#include "model.h"
#include "symmetry_host.h"

using namespace fdmi;

namespace {

hipStream_t stream_of(fd_model* m, void* hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : m->stream; }

// ---- the opening and the close of an entry that works on the current workspace
struct Call {
  Workspace* ws;
  size_t n;  // B * L * F
  hipStream_t s;
};

// the model's device and the (B, L) workspace become current
int open_ws(fd_model* m, int B, int L, void* hip_stream, Call* c) {
  HIP_TRY(hipSetDevice(m->device));
  if (int rc = ensure_ws(m, B, L)) return rc;
  *c = Call{&m->ws, (size_t)B * L * m->cfg.n_features, stream_of(m, hip_stream)};
  return FD_OK;
}

// ... and x, lens and an optional [B] int vector (into t_seq) are on their way into it
int open_call(fd_model* m, const void* x, const void* lens, const int32_t* per_seq, int B, int L, Call* c,
              hipMemcpyKind kind = hipMemcpyHostToDevice, void* hip_stream = nullptr) {
  if (int rc = open_ws(m, B, L, hip_stream, c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->ws->x, x, c->n * 4, kind, c->s));
  HIP_TRY(hipMemcpyAsync(c->ws->lens, lens, (size_t)B * 4, kind, c->s));
  if (per_seq) HIP_TRY(hipMemcpyAsync(c->ws->t_seq, per_seq, (size_t)B * 4, kind, c->s));
  return FD_OK;
}

struct Download {
  void* host;  // null: an optional output nobody asked for
  const void* dev;
  size_t bytes;
};

int download_sync(hipStream_t s, const std::vector<Download>& list) {
  for (const Download& d : list)
    if (d.host) HIP_TRY(hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FD_OK;
}

int finish(fd_model* m, hipStream_t s, const std::vector<Download>& list) {
  if (int rc = download_sync(s, list)) return rc;
  return check_flag(m);
}

// ---- one forward: fd_forward (t), fd_forward_t and fd_ar_forward (per_seq: a timestep or a target length per sequence)
int forward(fd_model* m, const float* x, const int32_t* lens, const int32_t* per_seq, int t, StepMode mode, int B, int L, float* out) {
  Call c;
  if (int rc = open_call(m, x, lens, per_seq, B, L, &c)) return rc;
  if (int rc = prepare_rows(m, c.s, 0)) return rc;  // the forward defines every position, masked ones included
  if (per_seq) mode.t_seq = c.ws->t_seq;
  else if (int rc = set_t(m, c.s, t)) return rc;
  mode.forward_only = true;
  if (int rc = run_step(m, c.s, mode)) return rc;
  return finish(m, c.s, {{out, c.ws->eps, c.n * 4}});
}

// every t[b] of a per-sequence timestep vector lies in [0, T)
int check_t_seq(const fd_model* m, const int32_t* t, int B) {
  for (int b = 0; b < B; ++b)
    if (t[b] < 0 || t[b] >= m->T) return fail(FD_E_INVALID, "timestep t[%d]=%d outside [0, %d)", b, t[b], m->T);
  return FD_OK;
}

// the arguments fd_ar_forward and fd_ar_sample share, all checked before the first HIP call
int check_ar(fd_model* m, const void* x, const int32_t* seq_lengths, const void* out, int B, int L, const char* who) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x || !seq_lengths || !out) return fail(FD_E_INVALID, "null argument");
  if (!m->img)
    return fail(FD_E_UNSUPPORTED, "%s: the autoregressive baseline runs on the row-image kernels only; finalize the model with "
                "FD_PREC_F16X3 (the exact-fp32 mode has no autoregressive embedding)", who);
  for (int b = 0; b < B; ++b)  // the length indexes the table fd_finalize was given in place of a timestep
    if (seq_lengths[b] < 0 || seq_lengths[b] >= m->T)
      return fail(FD_E_INVALID, "seq_lengths[%d]=%d outside [0, %d)", b, seq_lengths[b], m->T);
  return FD_OK;
}

// ---- ONE upload of several host arrays: staged back to back (in 4-byte words) in a pageable vector of the caller's frame and
// sent with a blocking copy, behind whatever an earlier asynchronous entry point left on the stream.  add() hands out the
// segment's device address, good once send() has returned.
class PackedUpload {
 public:
  explicit PackedUpload(float* dev) : dev_(dev) {}
  const float* add(const void* host, size_t words) {  // host null: the segment stays zero
    const size_t at = stage_.size();
    stage_.resize(at + words, 0.f);
    if (host) memcpy(stage_.data() + at, host, words * 4);
    return dev_ + at;
  }
  int send(hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(dev_, stage_.data(), stage_.size() * 4, hipMemcpyHostToDevice));
    return FD_OK;
  }

 private:
  float* dev_;
  std::vector<float> stage_;
};

// What the two loss entries run between their upload and their own kernels: t and lens into place, x_t (x_t_dev; null: q(x_t | x_0)
// on the device, with the wrap flags fd_finalize was given), then the forward with one timestep per sequence
int loss_forward(fd_model* m, const Call& c, int B, int L, const float* x0_dev, const float* noise_dev, const float* keep_dev,
                 const float* spread_dev, const float* x_t_dev, const float* t_dev, const float* lens_dev) {
  Workspace& w = *c.ws;
  HIP_TRY(hipMemcpyAsync(w.t_seq, t_dev, (size_t)B * 4, hipMemcpyDeviceToDevice, c.s));
  HIP_TRY(hipMemcpyAsync(w.lens, lens_dev, (size_t)B * 4, hipMemcpyDeviceToDevice, c.s));
  if (!x_t_dev) {
    launch_q_sample(x0_dev, noise_dev, keep_dev, spread_dev, w.x, B, L, m->cfg.n_features, m->angle_mask, c.s);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(w.x, x_t_dev, c.n * 4, hipMemcpyDeviceToDevice, c.s));
  }
  if (int rc = prepare_rows(m, c.s, 0)) return rc;
  StepMode mode{};
  mode.forward_only = true;
  mode.t_seq = w.t_seq;
  return run_step(m, c.s, mode);
}

// ---- motif-conditioned sampling: argument checks (before the first device call) and the workspace's staging buffer
int check_inpaint(const float* known, const uint8_t* fixed, const float* known_coef, const int32_t* lens, int B, int L, int F) {
  if (!fixed) return fail(FD_E_INVALID, "fixed is null");
  if (!known) return fail(FD_E_INVALID, "known is null (fixed is given)");
  if (!known_coef) return fail(FD_E_INVALID, "known_coef is null");
  for (int b = 0; b < B; ++b)
    for (int l = lens[b]; l < L; ++l)
      for (int f = 0; f < F; ++f)
        if (fixed[((size_t)b * L + l) * F + f])
          return fail(FD_E_INVALID, "fixed element beyond a length: sequence %d position %d feature %d, lens[%d] = %d", b, l, f, b, lens[b]);
  return FD_OK;
}

// the host arrays of a conditioned call (fixed null: not conditioned)
struct InpaintHost {
  const float* known = nullptr;
  const uint8_t* fixed = nullptr;
  const float* known_coef = nullptr;
};

// ... and where they are on the device (all null: not conditioned)
struct InpaintDev {
  float *known = nullptr, *z_known = nullptr, *coef = nullptr;
  unsigned char* fixed = nullptr;
  void apply(StepMode* mode) const {  // one step by value: z_known = the one slab of its level
    mode->known = known; mode->fixed = fixed; mode->known_coef = coef; mode->z_known = z_known;
  }
  void apply(UpdateDyn* dyn, const float* known_noise) const {  // a run: known_noise = every level's slab, or null (Philox)
    dyn->known = known; dyn->fixed = fixed; dyn->known_coef = coef; dyn->known_noise = known_noise;
  }
  static void clear(UpdateDyn* dyn) { InpaintDev().apply(dyn, nullptr); }
};

// uploads known / fixed / known_coef into the current workspace's staging buffer (allocated on first use), stream-ordered on s
int stage_inpaint(fd_model* m, hipStream_t s, const InpaintHost& h, InpaintDev* d) {
  Workspace& w = m->ws;
  const size_t n = (size_t)w.B * w.L * m->cfg.n_features, nc = 2 * ((size_t)m->T + 1);
  if (!w.inpaint) HIP_TRY(hipMalloc((void**)&w.inpaint, (2 * n + nc) * 4 + n));
  d->known = w.inpaint;
  d->z_known = w.inpaint + n;
  d->coef = w.inpaint + 2 * n;
  d->fixed = reinterpret_cast<unsigned char*>(w.inpaint + 2 * n + nc);
  HIP_TRY(hipMemcpyAsync(d->known, h.known, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d->coef, h.known_coef, nc * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d->fixed, h.fixed, n, hipMemcpyHostToDevice, s));
  return FD_OK;
}

// ---- ONE reverse step from host arrays: the six fd_p_sample_step* entries, each of which has checked its arguments, allocated
// its call-lifetime buffers (mode.x0_prev, mode.x0_out) and filled the StepMode fields of its update
struct StepHost {
  const float* x;
  int t;
  const int32_t* lens;
  int B, L, wrap;
  const float* z = nullptr;        // the draw to upload, or null: none is read (t = 0, s = 0)
  bool draws = true;               // the update takes its draw from the workspace's slab (false: it has none, the solver's)
  InpaintHost cond;                // fixed null: not conditioned
  const float* z_known = nullptr;  // the replacement's draw to upload, or null: none is read
};

// x_out, eps_out and x0_out (null: not asked for) are the one download list: the state, the prediction and mode.x0_out
int host_step(fd_model* m, const StepHost& h, StepMode mode, float* x_out, float* eps_out, float* x0_out) {
  Call c;
  if (int rc = open_call(m, h.x, h.lens, nullptr, h.B, h.L, &c)) return rc;
  Workspace& w = *c.ws;
  if (mode.x0_out) HIP_TRY(hipMemsetAsync(mode.x0_out, 0, c.n * 4, c.s));  // (a position the kernel does not take as a row is not written)
  if (h.z) HIP_TRY(hipMemcpyAsync(w.z, h.z, c.n * 4, hipMemcpyHostToDevice, c.s));
  InpaintDev ip;
  if (h.cond.fixed) {
    if (int rc = stage_inpaint(m, c.s, h.cond, &ip)) return rc;
    if (h.z_known) HIP_TRY(hipMemcpyAsync(ip.z_known, h.z_known, c.n * 4, hipMemcpyHostToDevice, c.s));
  }
  if (int rc = prepare_rows(m, c.s, 0)) return rc;
  if (int rc = set_t(m, c.s, h.t)) return rc;
  if (h.draws) mode.noise = w.z;
  mode.t_start = h.t;
  mode.no_wrap = !h.wrap;
  ip.apply(&mode);
  if (int rc = run_step(m, c.s, mode)) return rc;
  return finish(m, c.s, {{x_out, w.x, c.n * 4}, {eps_out, w.eps, c.n * 4}, {x0_out, mode.x0_out, c.n * 4}});
}

// one strided update by value: x' = a x + b eps (+ s z where s != 0)
StepMode strided_mode(float a, float b, float s) {
  StepMode mode{};
  mode.strided = true;
  mode.sa = a; mode.sb = b; mode.ss = s;
  return mode;
}

// the opening checks the step entries share ...
int check_step_call(fd_model* m, const void* x, const void* lens, const void* x_out, int B, int L, int t) {
  if (int rc = check_shape(m, B, L, t)) return rc;
  if (!x || !lens || !x_out) return fail(FD_E_INVALID, "null argument");
  return FD_OK;
}

// ... and the finiteness of the coefficients by value: names = one letter per value
int check_finite_coef(const char* names, std::initializer_list<float> values) {
  bool finite = true;
  for (float v : values) finite = finite && std::isfinite(v);
  if (finite) return FD_OK;
  char list[160];
  int at = 0;
  for (float v : values) at += snprintf(list + at, sizeof list - (size_t)at, "%s%c = %g", at ? ", " : "", *names++, (double)v);
  return fail(FD_E_INVALID, "%s: a coefficient is not finite", list);
}

// ---- resampling schedules: argument checks of fd_sample_inpaint_resample / fd_inpaint_jump
uint64_t segment_seed(uint64_t seed, int s) { return seed + (uint64_t)s * 0x9E3779B97F4A7C15ull; }

int check_jump_coef(float jk, float js, int jump) {
  if (!std::isfinite(jk) || !std::isfinite(js) || jk < 0.f || jk > 1.f || js < 0.f || js > 1.f)
    return fail(FD_E_INVALID, "jump_coef of jump %d: jk = %g, js = %g must be finite and within [0, 1]", jump, (double)jk, (double)js);
  return FD_OK;
}

// the rules of a legal schedule; *n_jumps = the number of jumps in it
int check_visits(const int32_t* visits, int n_visits, int t_start, const float* jump_coef, int* n_jumps) {
  if (!visits) return fail(FD_E_INVALID, "visits is null");
  if (n_visits < 1) return fail(FD_E_INVALID, "n_visits = %d must be positive", n_visits);
  if (visits[0] != t_start) return fail(FD_E_INVALID, "visits[0] = %d, the run starts with step t_start = %d", visits[0], t_start);
  int jumps = 0;
  for (int i = 1; i < n_visits; ++i) {
    if (visits[i] < 0 || visits[i] > t_start) return fail(FD_E_INVALID, "visits[%d] = %d outside [0, %d]", i, visits[i], t_start);
    if (visits[i] == visits[i - 1] - 1) continue;
    if (visits[i] < visits[i - 1])
      return fail(FD_E_INVALID, "visits[%d] = %d follows %d: neither the next step down nor a jump up", i, visits[i], visits[i - 1]);
    ++jumps;
  }
  if (visits[n_visits - 1] != 0) return fail(FD_E_INVALID, "visits[%d] = %d, the run ends with step 0", n_visits - 1, visits[n_visits - 1]);
  if (jumps && !jump_coef) return fail(FD_E_INVALID, "jump_coef is null and the schedule has %d jumps", jumps);
  for (int j = 0; j < jumps; ++j)
    if (int rc = check_jump_coef(jump_coef[2 * j], jump_coef[2 * j + 1], j)) return rc;
  *n_jumps = jumps;
  return FD_OK;
}

// ---- the opening of a sampling run on device arrays: n_steps reverse steps, the first of them step t_first.  The plain run
// (fd_sample_begin_dev) has n_steps = t_first + 1; a strided run counts its visits.  m->run_t = the steps left, minus one --
// in a plain run the next timestep
int begin_run(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, int t_first, int n_steps, uint64_t seed,
              int64_t seq_offset, void* out_dev, int full_history, void* hip_stream) {
  if (int rc = check_shape(m, B, L, t_first)) return rc;
  if (!x_init_dev || !lens_dev || !out_dev) return fail(FD_E_INVALID, "null argument");
  if (full_history < 0) return fail(FD_E_INVALID, "full_history = %d", full_history);
  Call c;
  if (int rc = open_call(m, x_init_dev, lens_dev, nullptr, B, L, &c, hipMemcpyDeviceToDevice, hip_stream)) return rc;
  Workspace& w = *c.ws;
  hipStream_t s = c.s;
  if (m->varlen && full_history)  // packed rows: positions beyond a sequence's length are never written
    HIP_TRY(hipMemsetAsync(out_dev, 0, ((size_t)(n_steps - 1 + full_history) / full_history) * c.n * 4, s));
  if (int rc = prepare_rows(m, s, m->varlen)) return rc;
  if (m->use_graph && !graph_current(m, w)) {
    // first use of this (B, L): the warm-up step and the capture run on the model's stream and need the
    // lengths / row table that were just queued on `s`
    if (s != m->stream) HIP_TRY(hipStreamSynchronize(s));
    if (int rc = ensure_graph(m)) return rc;
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  UpdateDyn& dyn = m->dyn_host;
  memset(&dyn, 0, sizeof dyn);
  dyn.hist = full_history ? static_cast<float*>(out_dev) : nullptr;
  dyn.seed = seed;
  dyn.seq_offset = seq_offset;
  dyn.t_start = t_first;
  dyn.hist_every = full_history;
  m->run_t = n_steps - 1;
  m->run_n = n_steps;
  m->run_open = true;
  m->run_B = B;
  m->run_L = L;
  if (int rc = set_t(m, s, t_first)) return rc;
  return FD_OK;
}

// ---- THE close of a sampling run whose family put pointers into the update kernels' per-run values (every run but the plain
// sampler's device entries): the run is over -- or failed, at any point behind begin_run -- and a later run on this model, of
// whatever family, starts from cleared fields, on the host and on the device.  The device-side UpdateDyn is what the captured
// step graph reads; the buffers those pointers named die with the caller's frame, hence the drain.
int close_run(fd_model* m, hipStream_t s) {
  m->run_open = false;
  m->run_t = -1;
  clear_run_pointers(&m->dyn_host);
  send_dyn(m, s, m->dyn_host);
  HIP_TRY(hipStreamSynchronize(s));
  return FD_OK;
}

// the host arrays every run family takes; the entry has checked every argument
struct RunArrays {
  const float* x_init;
  const int32_t* lens;
  int B, L;
  size_t states;             // the states a run without jumps goes through (plain: t_start + 1, strided: the grid's visits)
  const float* noise;        // [states][B][L][F], or null: Philox
  const float* known_noise;  // [states + 1][B][L][F], or null: Philox (or not conditioned)
  uint64_t seed;
  int64_t seq_offset;
  float* out;                // rows: 1 (final only), every state, or every full_history-th state plus the final one
  int full_history;
};

// ---- THE owner of a sampling run from host arrays, on the model's stream.  stage(): x_init, lens, out and the draws into
// buffers of the call's lifetime, blocking -- as is whatever the family adds to `bufs` (its tables, its work buffers) before
// begin() queues the first copy.  Between begin() and finish() the family sets its fields of m->dyn_host and runs its steps.
// finish(rc) ends the run where rc is FD_OK, closes it (close_run) whatever rc is, and then downloads `out` and the family's
// further outputs and reads the non-finite flag -- in that order for every family, so a run that answers FD_E_NONFINITE has
// written its (unusable, include/fdmi.h) outputs.  A frame left between begin() and finish() is closed by the destructor.
class HostRun {
 public:
  HostRun(fd_model* m, const RunArrays& a) : n((size_t)a.B * a.L * m->cfg.n_features), m_(m), a_(a) {}
  HostRun(const HostRun&) = delete;
  HostRun& operator=(const HostRun&) = delete;
  ~HostRun() {
    if (open_) (void)close_run(m_, m_->stream);
  }
  int stage() {
    HIP_TRY(hipSetDevice(m_->device));
    out_bytes_ = (a_.full_history ? (a_.states + a_.full_history - 1) / a_.full_history : 1) * n * 4;
    HIP_TRY(bufs.upload(a_.x_init, n * 4, &x));
    HIP_TRY(bufs.upload(a_.lens, (size_t)a_.B * 4, &lens));
    HIP_TRY(bufs.alloc(out_bytes_, &out));
    if (a_.noise) HIP_TRY(bufs.upload(a_.noise, a_.states * n * 4, &noise));
    if (a_.known_noise) HIP_TRY(bufs.upload(a_.known_noise, (a_.states + 1) * n * 4, &known_noise));
    return FD_OK;
  }
  int begin(int t_first, int n_steps) {
    if (int rc = begin_run(m_, x, lens, a_.B, a_.L, t_first, n_steps, a_.seed, a_.seq_offset, out, a_.full_history, nullptr)) return rc;
    open_ = true;
    return FD_OK;
  }
  int finish(int rc, std::initializer_list<Download> more = {}) {
    if (!rc) rc = fd_sample_end_dev(m_, out, nullptr);
    open_ = false;
    if (int rc_close = close_run(m_, m_->stream)) return rc_close;
    return rc ? rc : download(more);
  }
  int download(std::initializer_list<Download> more = {}) {  // (on its own: behind a run that strided_run_dev has closed)
    std::vector<Download> list{{a_.out, out, out_bytes_}};
    list.insert(list.end(), more);
    return ::finish(m_, m_->stream, list);
  }

  DeviceBufs bufs;
  const size_t n;  // B * L * F
  float *x = nullptr, *out = nullptr;
  int* lens = nullptr;
  const float *noise = nullptr, *known_noise = nullptr;

 private:
  fd_model* m_;
  const RunArrays a_;
  size_t out_bytes_ = 0;
  bool open_ = false;
};

// the conditioning of a run just begun: the arrays staged, the start point's fixed elements at the level it enters the first
// step with (start_draws: that level's slab, or null: Philox), the fields of the update kernels' per-run values (the captured
// step graph is the plain sampler's)
int begin_conditioning(fd_model* m, hipStream_t s, const InpaintHost& cond, const RunArrays& a, int level, const float* start_draws,
                       const float* d_known_noise, InpaintDev* ip) {
  if (int rc = stage_inpaint(m, s, cond, ip)) return rc;
  launch_inpaint_init(m->ws.x, ip->known, ip->fixed, start_draws, ip->coef, m->T, level, a.seed, a.seq_offset, a.B, a.L,
                      m->cfg.n_features, m->angle_mask, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FD_E_HIP, "launch_inpaint_init: %s", hipGetErrorString(e));
  ip->apply(&m->dyn_host, d_known_noise);
  return FD_OK;
}

// a schedule's visits, one segment per pass: the jump that enters it (none in front of the first), then its descent.  Launches only.
// descends(j): visit j follows visit j - 1 without a jump; steps_left(i): m->run_t once visit i is the next (plain ladder: its t)
template <class Descends, class StepsLeft>
int walk_visits(fd_model* m, hipStream_t s, const int32_t* visits, int n_visits, const float* jump_coef, uint64_t seed,
                int64_t seq_offset, int B, int L, const InpaintDev& ip, Descends descends, StepsLeft steps_left) {
  for (int i = 0, seg = 0; i < n_visits; ++seg) {
    int j = i + 1;
    while (j < n_visits && descends(j)) ++j;
    if (seg > 0) {
      const uint64_t seed_s = segment_seed(seed, seg);
      launch_inpaint_jump(m->ws.x, m->ws.lens, ip.known, ip.fixed, ip.coef, m->T, visits[i] + 1, jump_coef[2 * (seg - 1)],
                          jump_coef[2 * (seg - 1) + 1], seed_s, seq_offset, B, L, m->cfg.n_features, m->angle_mask, s);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return fail(FD_E_HIP, "launch_inpaint_jump: %s", hipGetErrorString(e));
      if (int rc = set_t(m, s, visits[i])) return rc;
      m->run_t = steps_left(i);
      m->dyn_host.seed = seed_s;
    }
    if (int rc = fd_sample_steps_dev(m, j - i, nullptr, 0, nullptr)) return rc;  // (re-sends dyn: the segment's seed)
    i = j;
  }
  return FD_OK;
}

// ---- a whole run down the ladder t_start .. 0 from host arrays (fd_sample_ex, fd_sample_inpaint, fd_sample_inpaint_resample); the
// entry has checked every argument.  A plain run goes through the same close as every other: one more stream-ordered copy of
// the small UpdateDyn, and a drained stream on the error paths too.
struct LadderRun {
  RunArrays arrays;
  int t_start;
  InpaintHost cond;                 // fixed null: a plain run
  const int32_t* visits = nullptr;  // a resampling schedule, or null: the single descent t_start .. 0
  int n_visits = 0;
  const float* jump_coef = nullptr;
};

int host_run(fd_model* m, const LadderRun& a) {
  HostRun r(m, a.arrays);
  if (int rc = r.stage()) return rc;
  if (int rc = r.begin(a.t_start, a.t_start + 1)) return rc;
  hipStream_t s = m->stream;
  InpaintDev ip;
  int rc = FD_OK;
  if (a.cond.fixed)  // the start point enters step t_start, so it is at level t_start + 1
    rc = begin_conditioning(m, s, a.cond, a.arrays, a.t_start + 1,
                            r.known_noise ? r.known_noise + ((size_t)a.t_start + 1) * r.n : nullptr, r.known_noise, &ip);
  if (!rc) {
    if (a.visits)  // a descent goes one step down the ladder
      rc = walk_visits(m, s, a.visits, a.n_visits, a.jump_coef, a.arrays.seed, a.arrays.seq_offset, a.arrays.B, a.arrays.L, ip,
                       [&](int j) { return a.visits[j] == a.visits[j - 1] - 1; }, [&](int i) { return a.visits[i]; });
    else
      rc = fd_sample_steps_dev(m, a.t_start + 1, r.noise, 0, nullptr);
  }
  return r.finish(rc);
}

// ---- strided (few-step) sampling: argument checks, all before the first device call
int check_coef_rows(const float* coef, int n_visits, int r0, int r1) {  // rows r0 .. r1 - 1 of a [.][n_visits] table are finite
  for (int r = r0; r < r1; ++r)
    for (int i = 0; i < n_visits; ++i)
      if (!std::isfinite(coef[(size_t)r * n_visits + i]))
        return fail(FD_E_INVALID, "coef[%d][%d] = %g is not finite", r, i, (double)coef[(size_t)r * n_visits + i]);
  return FD_OK;
}

int check_strided(const fd_model* m, const int32_t* visits, int n_visits, const float* coef) {
  if (!visits) return fail(FD_E_INVALID, "visits is null");
  if (!coef) return fail(FD_E_INVALID, "coef is null");
  if (n_visits < 1) return fail(FD_E_INVALID, "n_visits = %d must be positive", n_visits);
  for (int i = 0; i < n_visits; ++i) {
    if (visits[i] < 0 || visits[i] >= m->T) return fail(FD_E_INVALID, "visits[%d] = %d outside [0, %d)", i, visits[i], m->T);
    if (i > 0 && visits[i] >= visits[i - 1])
      return fail(FD_E_INVALID, "visits[%d] = %d follows %d: a strided schedule is strictly descending", i, visits[i], visits[i - 1]);
  }
  return check_coef_rows(coef, n_visits, 0, 3);
}

// where a strided run's tables are on the device: next_t | ord | the rows it asked for, [T] each
struct VisitTables {
  const int32_t* dev = nullptr;
  size_t T = 0;
  const float* row(size_t r) const { return reinterpret_cast<const float*>(dev + (2 + r) * T); }
  void apply(UpdateDyn* dyn) const {  // rows 0 .. 2 are a | b | s of every family
    dyn->next_t = dev;
    dyn->ord = dev + T;
    dyn->abs = row(0);
  }
};

// THE stager of the tables indexed by timestep, in ONE buffer of the call's lifetime (blocking upload): next_t | ord | one
// [T] row per entry of `rows`, a [K] host row whose element i goes to index visits[i] (null: a row of zeros).  A timestep the
// schedule does not visit holds next_t = -1 and zeros, and is never looked up.
int stage_tables(const fd_model* m, DeviceBufs* bufs, const int32_t* visits, int n_visits, std::initializer_list<const float*> rows,
                 VisitTables* d) {
  const size_t T = (size_t)m->T;
  std::vector<int32_t> tab((2 + rows.size()) * T, 0);
  for (size_t t = 0; t < T; ++t) tab[t] = -1;
  for (int i = 0; i < n_visits; ++i) {
    const size_t t = (size_t)visits[i];
    tab[t] = i + 1 < n_visits ? visits[i + 1] : -1;
    tab[T + t] = i;
    size_t r = 2;
    for (const float* row : rows) {
      if (row) memcpy(&tab[r * T + t], &row[i], 4);
      ++r;
    }
  }
  d->T = T;
  HIP_TRY(bufs->upload(tab.data(), tab.size() * 4, &d->dev));
  return FD_OK;
}

// ---- second-order multistep solver: a strided run with s = 0 whose update also reads the visit's (c, u, v) and
// the previous visit's prediction of the clean state
int check_solver(const fd_model* m, const int32_t* visits, int n_visits, const float* coef) {
  if (int rc = check_strided(m, visits, n_visits, coef)) return rc;  // the visits; rows a | b | c finite
  if (int rc = check_coef_rows(coef, n_visits, 3, 5)) return rc;
  if (coef[(size_t)2 * n_visits] != 0.f)
    return fail(FD_E_INVALID, "coef[2][0] = %g: the first visit has no earlier prediction, its c is 0", (double)coef[(size_t)2 * n_visits]);
  return FD_OK;
}

// A strided run on device arrays (the entry has checked every argument): the plain sampler's steps -- its captured graph
// included -- with the tables in the update kernels' per-run values.  `solver`: coef is [5][K] a | b | c | u | v, the run is the
// solver's and its noise_dev null: the tables hold a | b | 0 and c | u | v, and the [n] previous prediction is a buffer of this
// frame (uninitialised: the first visit's c is 0 and does not read it).  Returns closed (close_run) on every path behind
// begin_run: the tables and the previous prediction die with this frame.
int strided_run_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, const int32_t* visits, int n_visits,
                    const float* coef, bool solver, const void* noise_dev, uint64_t seed, int64_t seq_offset, void* out_dev,
                    int full_history, void* hip_stream) {
  HIP_TRY(hipSetDevice(m->device));
  const size_t K = (size_t)n_visits;
  DeviceBufs bufs;
  VisitTables tb;
  float* x0_prev = nullptr;
  if (solver) {
    if (int rc = stage_tables(m, &bufs, visits, n_visits, {coef, coef + K, nullptr, coef + 2 * K, coef + 3 * K, coef + 4 * K}, &tb)) return rc;
    HIP_TRY(bufs.alloc((size_t)B * L * m->cfg.n_features * 4, &x0_prev));
  } else if (int rc = stage_tables(m, &bufs, visits, n_visits, {coef, coef + K, coef + 2 * K}, &tb)) {
    return rc;
  }
  if (int rc = begin_run(m, x_init_dev, lens_dev, B, L, visits[0], n_visits, seed, seq_offset, out_dev, full_history, hip_stream)) return rc;
  tb.apply(&m->dyn_host);
  if (solver) {
    m->dyn_host.cuv = tb.row(3);
    m->dyn_host.x0_prev = x0_prev;
  }
  int rc = fd_sample_steps_dev(m, n_visits, noise_dev, 0, hip_stream);  // (noise rows are per visit: row 0 = visit 0)
  if (!rc) rc = fd_sample_end_dev(m, out_dev, hip_stream);
  const int rc_close = close_run(m, stream_of(m, hip_stream));
  return rc_close ? rc_close : rc;
}

// the same from host arrays (noise [K][B][L][F] or null)
int strided_run_host(fd_model* m, const RunArrays& a, const int32_t* visits, const float* coef, bool solver) {
  HostRun r(m, a);
  if (int rc = r.stage()) return rc;
  if (int rc = strided_run_dev(m, r.x, r.lens, a.B, a.L, visits, (int)a.states, coef, solver, r.noise, a.seed, a.seq_offset, r.out,
                               a.full_history, nullptr))
    return rc;
  return r.download();
}

// ---- the opening checks the run entries share, in the order the contract tests pin.  The ladder runs ...
int check_run_call(fd_model* m, const void* x_init, const int32_t* lens, const void* out, int B, int L, int t_start, int full_history) {
  if (int rc = check_shape(m, B, L, t_start)) return rc;
  if (!x_init || !lens || !out) return fail(FD_E_INVALID, "null argument");
  if (full_history < 0) return fail(FD_E_INVALID, "full_history = %d", full_history);
  return check_lens(lens, B, L);
}

// ... an entry with jumps ...
int check_jump_tag(const fd_model* m) {
  if (m->T >= (1 << 30)) return fail(FD_E_UNSUPPORTED, "T = %d: the jump's stream is tagged with bit 30 of the step word", m->T);
  return FD_OK;
}

// ... and the strided runs, on host or device arrays (a host entry checks its lengths next)
int check_strided_call(fd_model* m, const void* x_init, const void* lens, const void* out, int B, int L, const int32_t* visits,
                       int n_visits, const float* coef, int full_history, bool solver = false) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x_init || !lens || !out) return fail(FD_E_INVALID, "null argument");
  if (full_history < 0) return fail(FD_E_INVALID, "full_history = %d", full_history);
  return solver ? check_solver(m, visits, n_visits, coef) : check_strided(m, visits, n_visits, coef);
}

// ---- strided runs with motif conditioning: the strided tables and the conditioning in the same per-run values.
// A visit at t then replaces its fixed elements at the level it lands on, next_t[t] + 1 (inpaint_replace.h).

// where each timestep sits on a strided grid: pos[t] = its index, -1 off the grid
std::vector<int> grid_positions(const fd_model* m, const int32_t* grid, int n_grid) {
  std::vector<int> pos((size_t)m->T, -1);
  for (int i = 0; i < n_grid; ++i) pos[(size_t)grid[i]] = i;
  return pos;
}

// the rules of a legal resampled run over a (checked) grid; *n_jumps = the number of jumps in it
int check_strided_visits(const fd_model* m, const int32_t* grid, int n_grid, const int32_t* run, int n_run, const float* jump_coef,
                         int* n_jumps) {
  if (!run) return fail(FD_E_INVALID, "run is null");
  if (n_run < 1) return fail(FD_E_INVALID, "n_run = %d must be positive", n_run);
  const std::vector<int> pos = grid_positions(m, grid, n_grid);
  int jumps = 0;
  for (int i = 0; i < n_run; ++i) {
    if (run[i] < 0 || run[i] >= m->T || pos[(size_t)run[i]] < 0) return fail(FD_E_INVALID, "run[%d] = %d is not on the grid", i, run[i]);
    if (i == 0) {
      if (run[0] != grid[0]) return fail(FD_E_INVALID, "run[0] = %d, the run starts with the grid's first visit %d", run[0], grid[0]);
      continue;
    }
    if (pos[(size_t)run[i]] == pos[(size_t)run[i - 1]] + 1) continue;
    if (run[i] < run[i - 1])
      return fail(FD_E_INVALID, "run[%d] = %d follows %d: neither the grid's next visit nor a jump up", i, run[i], run[i - 1]);
    ++jumps;
  }
  if (run[n_run - 1] != grid[n_grid - 1])
    return fail(FD_E_INVALID, "run[%d] = %d, the run ends with the grid's last visit %d", n_run - 1, run[n_run - 1], grid[n_grid - 1]);
  if (jumps && !jump_coef) return fail(FD_E_INVALID, "jump_coef is null and the run has %d jumps", jumps);
  for (int j = 0; j < jumps; ++j)
    if (int rc = check_jump_coef(jump_coef[2 * j], jump_coef[2 * j + 1], j)) return rc;
  *n_jumps = jumps;
  return FD_OK;
}

// the host arrays of a strided conditioned run; the entry has checked every argument
struct StridedHostRun {
  RunArrays arrays;     // states = n_grid; known_noise row 0: the start point, row i + 1: the state visit i leaves
  const int32_t* grid;  // strictly descending
  const float* coef;    // [3][n_grid]
  InpaintHost cond;
  const int32_t* run = nullptr;  // a resampled run over the grid, or null: the grid once
  int n_run = 0;
  const float* jump_coef = nullptr;
};

int strided_host_run(fd_model* m, const StridedHostRun& a) {
  const RunArrays& h = a.arrays;
  const int n_grid = (int)h.states;
  HostRun r(m, h);
  if (int rc = r.stage()) return rc;
  VisitTables tb;
  if (int rc = stage_tables(m, &r.bufs, a.grid, n_grid, {a.coef, a.coef + n_grid, a.coef + 2 * (size_t)n_grid}, &tb)) return rc;
  if (int rc = r.begin(a.grid[0], a.run ? a.n_run : n_grid)) return rc;
  hipStream_t s = m->stream;
  tb.apply(&m->dyn_host);
  InpaintDev ip;  // the start point enters visit 0, so it is at level grid[0] + 1; its draws are row 0
  int rc = begin_conditioning(m, s, a.cond, h, a.grid[0] + 1, r.known_noise, r.known_noise, &ip);
  if (!rc) {
    if (a.run) {  // a descent goes to the grid's next visit; a jump starts from the level the visit before it landed on
      const std::vector<int> pos = grid_positions(m, a.grid, n_grid);
      rc = walk_visits(m, s, a.run, a.n_run, a.jump_coef, h.seed, h.seq_offset, h.B, h.L, ip,
                       [&](int j) { return pos[(size_t)a.run[j]] == pos[(size_t)a.run[j - 1]] + 1; }, [&](int i) { return a.n_run - 1 - i; });
    } else {
      rc = fd_sample_steps_dev(m, n_grid, r.noise, 0, nullptr);
    }
  }
  return r.finish(rc);
}

// ---- steered sampling: a strided run whose visits also write their prediction of the clean state, with an
// event -- shift, rewards, resample, gather (steer.hip) -- between the step segments, as walk_visits puts jumps between them
struct SteeredHostRun {
  RunArrays arrays;  // states = K, final state only
  const int32_t* visits;
  const float* coef;     // [5][K] a | b | s | u | v
  const uint8_t* event;  // [K]
  int n_events;
  int P;
  const fd_steer_params* params;
  const double* u;  // [n_events][B / P]
  double *terms_out, *reward_out, *logw_out;
  int32_t* ancestors_out;  // [n_events][B], or null
};

// The entry has checked every argument.  The tables, the prediction buffer and the rewards pass's buffers die with this frame.
int steered_host_run(fd_model* m, const SteeredHostRun& a) {
  const RunArrays& h = a.arrays;
  const int F = m->cfg.n_features, B = h.B, L = h.L, K = (int)h.states, G = B / a.P;
  const size_t nr = (size_t)B * L, nb = (size_t)B, Kz = h.states;
  const fd_steer_params& sp = *a.params;
  HostRun r(m, h);
  if (int rc = r.stage()) return rc;
  const size_t n = r.n;
  DeviceBufs& bufs = r.bufs;
  float *d_ang, *d_tmp, *d_x0;
  HIP_TRY(bufs.alloc(n * 4, &d_ang));
  HIP_TRY(bufs.alloc(n * 4, &d_tmp));
  VisitTables tb;
  if (int rc = stage_tables(m, &bufs, a.visits, K, {a.coef, a.coef + Kz, a.coef + 2 * Kz, a.coef + 3 * Kz, a.coef + 4 * Kz}, &tb)) return rc;
  HIP_TRY(bufs.zeros(n * 4, &d_x0));  // (packed rows: a position beyond a length is never written, and never read)
  // the rewards pass's buffers, the weights' state and the uniforms
  SteerWork wk{};
  std::vector<int32_t> offsets(nb);
  int max_len = 0;
  for (int b = 0; b < B; ++b) {
    offsets[(size_t)b] = b * L;
    max_len = h.lens[b] > max_len ? h.lens[b] : max_len;
  }
  HIP_TRY(bufs.alloc(nr * 9 * 8, &wk.coords));
  HIP_TRY(bufs.alloc(nr * 9 * 4, &wk.xyz));
  HIP_TRY(bufs.alloc(nr * 3 * 8, &wk.ca));
  HIP_TRY(bufs.alloc(nr, &wk.sse));
  HIP_TRY(bufs.alloc(nb * 2 * 4, &wk.sse_runs));
  HIP_TRY(bufs.alloc(nb * 4, &wk.clashes));
  HIP_TRY(bufs.upload(offsets.data(), nb * 4, &wk.offsets));
  double *d_terms, *d_reward, *d_logw, *d_rprev;
  const double* d_u = nullptr;
  int* d_anc;
  unsigned char* d_flags;
  const size_t ne = a.n_events > 0 ? (size_t)a.n_events : 1;
  HIP_TRY(bufs.alloc(nb * 4 * 8, &d_terms));
  HIP_TRY(bufs.alloc(nb * 8, &d_reward));
  HIP_TRY(bufs.zeros(nb * 8, &d_logw));
  HIP_TRY(bufs.zeros(nb * 8, &d_rprev));
  HIP_TRY(bufs.alloc(ne * nb * 4, &d_anc));
  HIP_TRY(bufs.alloc((size_t)G, &d_flags));
  if (a.n_events > 0) HIP_TRY(bufs.upload(a.u, ne * (size_t)G * 8, &d_u));
  const NerfFeatures fx{sp.feat_idx[0], sp.feat_idx[1], sp.feat_idx[2], sp.feat_idx[3], sp.feat_idx[4],
                        sp.feat_idx[5], sp.feat_idx[6], sp.feat_idx[7], sp.feat_idx[8]};
  SteerWeights wt{};
  for (int k = 0; k < 4; ++k) wt.w[k] = sp.weights[k];
  SteerOffset off{};
  off.has_offset = sp.has_offset ? 1 : 0;
  for (int f = 0; sp.has_offset && f < F; ++f) off.offset[f] = sp.offset[f];

  if (int rc = r.begin(a.visits[0], K)) return rc;
  hipStream_t s = m->stream;
  Workspace& w = m->ws;
  tb.apply(&m->dyn_host);
  m->dyn_host.uv = tb.row(3);
  m->dyn_host.x0_steer = d_x0;
  auto rewards_of = [&](const float* state) -> int {  // shift + rewards of a [B][L][F] state in model space
    launch_steer_shift(state, w.lens, B, L, F, off, m->angle_mask, d_ang, s);
    launch_steer_rewards(d_ang, w.lens, B, L, F, fx, wt, sp.clash_alpha, max_len, wk, d_terms, d_reward, s);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(FD_E_HIP, "launch_steer_rewards: %s", hipGetErrorString(e)) : FD_OK;
  };
  int rc = FD_OK;
  for (int i = 0, e = 0; !rc && i < K;) {  // a segment ends with a visit that has an event, or with the last visit
    int j = i + 1;
    while (j < K && !a.event[j - 1]) ++j;
    rc = fd_sample_steps_dev(m, j - i, r.noise, 0, nullptr);  // (noise rows are per visit, whatever the segment)
    if (!rc && a.event[j - 1]) {
      rc = rewards_of(d_x0);
      if (!rc) {
        int* anc = d_anc + (size_t)e * nb;
        launch_steer_resample(d_reward, d_logw, d_rprev, G, a.P, sp.lambda, sp.ess_frac, d_u + (size_t)e * G, anc, d_flags, s);
        launch_steer_gather(w.x, anc, d_tmp, B, (long long)L * F, s);
        const hipError_t he = hipGetLastError();
        if (he != hipSuccess) rc = fail(FD_E_HIP, "launch_steer_resample: %s", hipGetErrorString(he));
      }
      if (!rc) {
        const hipError_t he = hipMemcpyAsync(w.x, d_tmp, n * 4, hipMemcpyDeviceToDevice, s);
        if (he != hipSuccess) rc = fail(FD_E_HIP, "hipMemcpyAsync: %s", hipGetErrorString(he));
      }
      ++e;
    }
    i = j;
  }
  if (!rc) rc = rewards_of(w.x);  // the final state's
  return r.finish(rc, {{a.terms_out, d_terms, nb * 4 * 8},
                       {a.reward_out, d_reward, nb * 8},
                       {a.logw_out, d_logw, nb * 8},
                       {a.n_events > 0 ? a.ancestors_out : nullptr, d_anc, ne * nb * 4}});
}

// ---- repeat sampling: a strided run whose visits leave wrap(a x + b eps) -- the tables' row s is zero, the draw
// is the tie launch's -- with one tie launch (repeat_tie.hip) behind every visit, which averages the copies of a unit row and
// adds the visit's draw, the same one to every copy.  The entry has checked every argument; a.states = K, final state only.
int repeat_host_run(fd_model* m, const RunArrays& a, const int32_t* visits, const float* coef, const int32_t* tie) {
  const int F = m->cfg.n_features, B = a.B, L = a.L, K = (int)a.states;
  HostRun r(m, a);
  if (int rc = r.stage()) return rc;
  const int* d_tie;
  HIP_TRY(r.bufs.upload(tie, (size_t)B * 3 * 4, &d_tie));
  VisitTables tb;
  if (int rc = stage_tables(m, &r.bufs, visits, K, {coef, coef + a.states, nullptr}, &tb)) return rc;
  if (int rc = r.begin(visits[0], K)) return rc;
  hipStream_t s = m->stream;
  Workspace& w = m->ws;
  tb.apply(&m->dyn_host);
  auto tie_state = [&](int init, float sz, const float* z, int t) -> int {
    launch_repeat_tie(w.x, w.lens, d_tie, B, L, F, m->angle_mask, init, sz, z, a.seed, t, a.seq_offset, s);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(FD_E_HIP, "launch_repeat_tie: %s", hipGetErrorString(e)) : FD_OK;
  };
  int rc = tie_state(1, 0.f, nullptr, 0);  // the start point: every copy is copy 0
  for (int i = 0; !rc && i < K; ++i) {
    rc = fd_sample_steps_dev(m, 1, nullptr, 0, nullptr);
    if (!rc) rc = tie_state(0, coef[2 * a.states + i], r.noise ? r.noise + (size_t)i * r.n : nullptr, visits[i]);
  }
  return r.finish(rc);
}

// ---- restraint-guided sampling: a strided run whose visits leave wrap(a x + b eps) and their prediction of the
// clean state -- the tables' row s is zero, as in a repeat run; u | v as in a steered run -- with the guide statement's five
// launches (steer.hip's shift, nerf.hip, nerf_vjp.hip) behind every visit.  The entry has checked every argument; a.states = K,
// final state only.  The tables, the restraints and the work buffers die with this frame.
struct GuidedHostRun {
  RunArrays arrays;
  const int32_t* visits;
  const float* coef;   // [5][K] a | b | s | u | v
  const float* guide;  // [K]
  const fd_guide_params* params;
  RestraintLists rst;
  double *energy_out, *max_violation_out;
};

int guided_host_run(fd_model* m, const GuidedHostRun& a) {
  const RunArrays& h = a.arrays;
  const int F = m->cfg.n_features, B = h.B, L = h.L, K = (int)h.states;
  const size_t na = (size_t)B * 3 * L * 3, nb = (size_t)B, Kz = h.states, R = a.rst.count();
  const fd_guide_params& gp = *a.params;
  HostRun r(m, h);
  if (int rc = r.stage()) return rc;
  const size_t n = r.n;
  DeviceBufs& bufs = r.bufs;
  VisitTables tb;
  if (int rc = stage_tables(m, &bufs, a.visits, K, {a.coef, a.coef + Kz, nullptr, a.coef + 3 * Kz, a.coef + 4 * Kz}, &tb)) return rc;
  float *d_x0, *d_ang;
  double *d_coords, *d_gc, *d_G, *d_energy, *d_maxv, *d_gnorm;
  HIP_TRY(bufs.zeros(n * 4, &d_x0));  // (packed rows: a position beyond a length is never written, and never read)
  HIP_TRY(bufs.alloc(n * 4, &d_ang));
  HIP_TRY(bufs.alloc(na * 8, &d_coords));
  HIP_TRY(bufs.alloc(na * 8, &d_gc));
  HIP_TRY(bufs.alloc(n * 8, &d_G));
  HIP_TRY(bufs.alloc(nb * 8, &d_energy));
  HIP_TRY(bufs.alloc(nb * 8, &d_maxv));
  HIP_TRY(bufs.alloc(nb * 8, &d_gnorm));
  Restraints rs{};  // (an empty list: the kernel reads the offsets only)
  HIP_TRY(bufs.upload(a.rst.offsets, (nb + 1) * 4, &rs.offsets));
  if (R) {
    HIP_TRY(bufs.upload(a.rst.i, R * 4, &rs.i));
    HIP_TRY(bufs.upload(a.rst.j, R * 4, &rs.j));
    HIP_TRY(bufs.upload(a.rst.d0, R * 8, &rs.d0));
    HIP_TRY(bufs.upload(a.rst.tol, R * 8, &rs.tol));
    HIP_TRY(bufs.upload(a.rst.w, R * 8, &rs.w));
  }
  const NerfFeatures fx{gp.feat_idx[0], gp.feat_idx[1], gp.feat_idx[2], gp.feat_idx[3], gp.feat_idx[4],
                        gp.feat_idx[5], gp.feat_idx[6], gp.feat_idx[7], gp.feat_idx[8]};
  SteerOffset off{};
  off.has_offset = gp.has_offset ? 1 : 0;
  for (int f = 0; gp.has_offset && f < F; ++f) off.offset[f] = gp.offset[f];

  if (int rc = r.begin(a.visits[0], K)) return rc;
  hipStream_t s = m->stream;
  Workspace& w = m->ws;
  tb.apply(&m->dyn_host);
  m->dyn_host.uv = tb.row(3);
  m->dyn_host.x0_steer = d_x0;
  auto energy_of = [&](const float* state, double* grad) {  // shift, NeRF and the restraints of a [B][L][F] state in model space
    launch_steer_shift(state, w.lens, B, L, F, off, m->angle_mask, d_ang, s);
    launch_nerf(d_ang, w.lens, B, L, F, fx, 0, d_coords, s);
    launch_restraint_energy(d_coords, w.lens, B, L, rs, d_energy, d_maxv, grad, s);
  };
  auto launched = [&]() -> int {
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(FD_E_HIP, "the guide launches: %s", hipGetErrorString(e)) : FD_OK;
  };
  int rc = FD_OK;
  for (int i = 0; !rc && i < K; ++i) {
    rc = fd_sample_steps_dev(m, 1, nullptr, 0, nullptr);
    if (rc) break;
    energy_of(d_x0, d_gc);
    launch_nerf_vjp(d_coords, w.lens, B, L, F, fx, 0, d_gc, d_ang, d_G, s);
    launch_guide_update(w.x, d_G, w.lens, B, L, F, m->angle_mask, a.guide[i], gp.max_norm, a.coef[2 * Kz + i],
                        r.noise ? r.noise + (size_t)i * r.n : nullptr, h.seed, a.visits[i], h.seq_offset, d_gnorm, s);
    rc = launched();
  }
  if (!rc) {
    energy_of(w.x, nullptr);  // the final state's
    rc = launched();
  }
  return r.finish(rc, {{a.energy_out, d_energy, nb * 8}, {a.max_violation_out, d_maxv, nb * 8}});
}

// ---- restraint guidance with replacement: guided_host_run with strided_host_run's conditioning in the same
// per-run values -- a visit's fixed elements take update_element's fixed branch, its free ones leave wrap(a x + b eps) and
// their x0 -- and the scaffold-guide statement's launches (guide_scaffold.hip) behind every visit.  The entry has checked every
// argument; a.states = K, final state only.  The tables, the restraints and the work buffers die with this frame.  With a
// template (fd_sample_guided_inpaint_tpl) the statement has one more launch, template_fit.hip's.
// With symmetry orders (fd_sample_guided_inpaint_sym) launch_symmetry_guide's launches follow the template's, and
// the pose, its step size and the placed atoms stay on the device from visit to visit.
struct ScaffoldGuidedHostRun {
  RunArrays arrays;  // known_noise row 0: the start point, row i + 1: the state visit i leaves
  const int32_t* visits;
  const float* coef;   // [5][K] a | b | s | u | v
  const float* guide;  // [K]
  InpaintHost cond;
  const fd_scaffold_guide_params* params;
  RestraintLists rst;
  TemplateLists tpl;   // none, or a chain's entries
  int n_energies;      // 2: restraint | clash (fd_sample_guided_inpaint); 3: | template, and tpl_rmsd_out
  double *energy_out, *max_violation_out, *tpl_rmsd_out;  // [B][n_energies], [B], [B]
  // cyclic symmetry (fd_sample_guided_inpaint_sym); sym_order null: none, and the rest is not looked at
  const int32_t* sym_order;
  const double* sym_pose0;  // [B][12]
  const fd_symmetry_params* sym_params;
  double* sym_energy_out;   // [B][3]
  int32_t* sym_contacts_out;
  double* sym_pose_out;     // [B][12]
};

int scaffold_guided_host_run(fd_model* m, const ScaffoldGuidedHostRun& a) {
  const RunArrays& h = a.arrays;
  const int F = m->cfg.n_features, B = h.B, L = h.L, K = (int)h.states;
  const size_t na = (size_t)B * 3 * L * 3, nb = (size_t)B, Kz = h.states, R = a.rst.count();
  const fd_scaffold_guide_params& gp = *a.params;
  HostRun r(m, h);
  if (int rc = r.stage()) return rc;
  const size_t n = r.n;
  DeviceBufs& bufs = r.bufs;
  VisitTables tb;
  if (int rc = stage_tables(m, &bufs, a.visits, K, {a.coef, a.coef + Kz, nullptr, a.coef + 3 * Kz, a.coef + 4 * Kz}, &tb)) return rc;
  float* d_x0;
  double *d_G, *d_gnorm;
  ScaffoldWork wk{};
  HIP_TRY(bufs.zeros(n * 4, &d_x0));  // (a fixed element and a position beyond a length are never written, and never read)
  HIP_TRY(bufs.alloc(n * 4, &wk.ang));
  HIP_TRY(bufs.alloc(na * 8, &wk.coords));
  HIP_TRY(bufs.alloc(na * 8, &wk.gc));
  HIP_TRY(bufs.alloc(n * 8, &d_G));
  HIP_TRY(bufs.alloc(nb * 8, &wk.e_rst));
  HIP_TRY(bufs.alloc(nb * 8, &wk.max_violation));
  HIP_TRY(bufs.zeros(nb * 8, &wk.e_clash));  // (stays 0 where there is no clash term)
  HIP_TRY(bufs.zeros(nb * 8, &wk.e_tpl));    // (and these where no chain has a template entry: that launch is skipped)
  HIP_TRY(bufs.zeros(nb * 8, &wk.rmsd_tpl));
  HIP_TRY(bufs.alloc(nb * 8, &d_gnorm));
  TemplateFit tf{};
  const TemplateFit* fit = a.tpl.count() ? &tf : nullptr;
  if (fit) {
    HIP_TRY(bufs.upload(a.tpl.offsets, (nb + 1) * 4, &tf.offsets));
    HIP_TRY(bufs.upload(a.tpl.atom, a.tpl.count() * 4, &tf.atom));
    HIP_TRY(bufs.upload(a.tpl.xyz, a.tpl.count() * 24, &tf.xyz));
    HIP_TRY(bufs.upload(a.tpl.w, a.tpl.count() * 8, &tf.w));
  }
  Restraints rs{};  // (an empty list: the kernel reads the offsets only)
  HIP_TRY(bufs.upload(a.rst.offsets, (nb + 1) * 4, &rs.offsets));
  if (R) {
    HIP_TRY(bufs.upload(a.rst.i, R * 4, &rs.i));
    HIP_TRY(bufs.upload(a.rst.j, R * 4, &rs.j));
    HIP_TRY(bufs.upload(a.rst.d0, R * 8, &rs.d0));
    HIP_TRY(bufs.upload(a.rst.tol, R * 8, &rs.tol));
    HIP_TRY(bufs.upload(a.rst.w, R * 8, &rs.w));
  }
  const NerfFeatures fx{gp.feat_idx[0], gp.feat_idx[1], gp.feat_idx[2], gp.feat_idx[3], gp.feat_idx[4],
                        gp.feat_idx[5], gp.feat_idx[6], gp.feat_idx[7], gp.feat_idx[8]};
  SteerOffset off{};
  off.has_offset = gp.has_offset ? 1 : 0;
  for (int f = 0; gp.has_offset && f < F; ++f) off.offset[f] = gp.offset[f];
  const SoftClash clash{gp.clash_alpha, gp.clash_margin, gp.w_clash};
  // the symmetry lines: the pose, h and the placed atoms are carried on the device from visit to visit (the first visit takes
  // sym_pose0 as it is, every later one fits onto where the visit before placed the chain)
  bool symmetric = false;
  for (int b = 0; a.sym_order && b < B; ++b) symmetric |= a.sym_order[b] >= 2;
  SymGuide sg{};
  if (symmetric)
    if (int rc = stage_symmetry_guide(&bufs, a.sym_order, a.sym_pose0, nullptr, *a.sym_params, h.lens, r.lens, wk.coords, B, L, nullptr, true, &sg))
      return rc;

  if (int rc = r.begin(a.visits[0], K)) return rc;
  hipStream_t s = m->stream;
  Workspace& w = m->ws;
  tb.apply(&m->dyn_host);
  m->dyn_host.uv = tb.row(3);
  m->dyn_host.x0_steer = d_x0;
  InpaintDev ip;  // the start point enters visit 0, so it is at level visits[0] + 1; its draws are row 0
  int rc = begin_conditioning(m, s, a.cond, h, a.visits[0] + 1, r.known_noise, r.known_noise, &ip);
  auto launched = [&]() -> int {
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(FD_E_HIP, "the scaffold-guide launches: %s", hipGetErrorString(e)) : FD_OK;
  };
  for (int i = 0; !rc && i < K; ++i) {
    rc = fd_sample_steps_dev(m, 1, nullptr, 0, nullptr);
    if (rc) break;
    launch_scaffold_energy(d_x0, ip.known, ip.fixed, w.lens, B, L, F, off, m->angle_mask, fx, rs, clash, fit, wk, d_G, s,
                           symmetric ? &sg : nullptr);
    sg.fit.xyz = sg.placed_packed;  // (from the second visit on)
    launch_scaffold_update(w.x, d_G, ip.fixed, w.lens, B, L, F, m->angle_mask, a.guide[i], gp.max_norm, a.coef[2 * Kz + i],
                           r.noise ? r.noise + (size_t)i * r.n : nullptr, h.seed, a.visits[i], h.seq_offset, d_gnorm, s);
    rc = launched();
  }
  if (!rc) {  // the final state's: its fixed elements hold known's bits, so p is the state itself
    launch_scaffold_energy(w.x, ip.known, ip.fixed, w.lens, B, L, F, off, m->angle_mask, fx, rs, clash, fit, wk, nullptr, s,
                           symmetric ? &sg : nullptr);
    rc = launched();
  }
  std::vector<double> e_rst(nb), e_clash(nb), maxv(nb), e_tpl(nb), rmsd_tpl(nb), e_sym(symmetric ? nb * 3 : 0);
  std::vector<int32_t> c_sym(symmetric ? nb : 0);
  std::vector<SymState> st_sym(symmetric ? nb : 0);
  const auto opt = [&](void* host) { return symmetric ? host : nullptr; };  // (a null host pointer: not downloaded)
  rc = r.finish(rc, {{e_rst.data(), wk.e_rst, nb * 8}, {e_clash.data(), wk.e_clash, nb * 8}, {maxv.data(), wk.max_violation, nb * 8},
                     {e_tpl.data(), wk.e_tpl, nb * 8}, {rmsd_tpl.data(), wk.rmsd_tpl, nb * 8}, {opt(e_sym.data()), sg.energy, nb * 24},
                     {opt(c_sym.data()), sg.contacts, nb * 4}, {opt(st_sym.data()), sg.dock.state, nb * sizeof(SymState)}});
  if (rc && rc != FD_E_NONFINITE) return rc;  // (a run that answers FD_E_NONFINITE has written its outputs, as every family's)
  const size_t ne = (size_t)a.n_energies;
  for (size_t b = 0; a.sym_order && b < nb; ++b) {
    for (int k = 0; k < 3; ++k) a.sym_energy_out[3 * b + k] = symmetric ? e_sym[3 * b + k] : 0.0;
    a.sym_contacts_out[b] = symmetric ? c_sym[b] : 0;
    memcpy(a.sym_pose_out + 12 * b, symmetric ? st_sym[b].pose : a.sym_pose0 + 12 * b, 96);
  }
  for (size_t b = 0; b < nb; ++b) {
    a.energy_out[ne * b] = e_rst[b];
    a.energy_out[ne * b + 1] = e_clash[b];
    if (ne == 3) {
      a.energy_out[3 * b + 2] = e_tpl[b];
      a.tpl_rmsd_out[b] = rmsd_tpl[b];
    }
    a.max_violation_out[b] = maxv[b];
  }
  return rc;
}

}  // namespace

// ============================================================================ C ABI
extern "C" {

int fd_forward(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float* eps_out) {
  if (int rc = check_shape(m, B, L, t)) return rc;
  if (!x || !lens || !eps_out) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_lens(lens, B, L)) return rc;
  return forward(m, x, lens, nullptr, t, StepMode{}, B, L, eps_out);
}

int fd_forward_t(fd_model* m, const float* x, const int32_t* t, const int32_t* lens, int B, int L, float* eps_out) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x || !t || !lens || !eps_out) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_t_seq(m, t, B)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  return forward(m, x, lens, t, 0, StepMode{}, B, L, eps_out);
}

int fd_ar_forward(fd_model* m, const float* x, const int32_t* seq_lengths, const int32_t* key_lens, int B, int L, float* out) {
  if (int rc = check_ar(m, x, seq_lengths, out, B, L, "fd_ar_forward")) return rc;
  if (!key_lens) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_lens(key_lens, B, L)) return rc;
  StepMode mode{};
  mode.ar = true;
  return forward(m, x, key_lens, seq_lengths, 0, mode, B, L, out);
}

int fd_ar_sample(fd_model* m, const float* seed, const int32_t* seq_lengths, int B, int L, int num_seed, float* out) {
  if (int rc = check_ar(m, seed, seq_lengths, out, B, L, "fd_ar_sample")) return rc;
  if (num_seed < 1)  // (no seed: the first step's keys would all be masked)
    return fail(FD_E_INVALID, "num_seed=%d must be at least 1", num_seed);
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    if (seq_lengths[b] > L) return fail(FD_E_INVALID, "seq_lengths[%d]=%d exceeds L=%d", b, seq_lengths[b], L);
    longest = seq_lengths[b] > longest ? seq_lengths[b] : longest;
  }
  Call c;
  if (int rc = open_ws(m, B, L, nullptr, &c)) return rc;
  Workspace& w = *c.ws;
  const int F = m->cfg.n_features;
  const size_t n = c.n, nb = (size_t)B;
  hipStream_t s = c.s;
  // ONE upload, seed | seq_lengths, through fd_denoise_loss's staging buffer (allocated at that entry's size, so that either may
  // come first)
  if (!w.loss_in) HIP_TRY(hipMalloc((void**)&w.loss_in, (2 * n + 4 * nb) * 4));
  PackedUpload up(w.loss_in);
  const float *seed_dev = up.add(seed, n), *lengths_dev = up.add(seq_lengths, nb);
  if (int rc = up.send(s)) return rc;
  HIP_TRY(hipMemcpyAsync(w.x, seed_dev, n * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(w.t_seq, lengths_dev, nb * 4, hipMemcpyDeviceToDevice, s));
  // Step i is a forward over the rows 0 .. i of every sequence with the keys 0 .. i-1 unmasked (rows > i are masked keys and
  // queries nobody reads: they can influence nothing); its head writes eps[b][0 .. i], and row i of it becomes x[b][i].  The
  // row count grows on the device, so the GEMMs run their slice-capable instantiation; everything else is plan_step's choice
  const StepPlan plan = plan_step(m, w, false, true);
  StepMode mode{};
  mode.forward_only = true;
  mode.t_seq = w.t_seq;
  mode.ar = true;
  auto tail = [&](int copy_pos, int rows_next) -> int {
    launch_ar_step(w.x, w.eps, B, L, F, copy_pos, rows_next, w.cap, w.lens, w.nrow, w.seq_row0, w.rowinfo, w.dims, s);
    HIP_TRY(hipGetLastError());
    return FD_OK;
  };
  if (num_seed < longest)
    if (int rc = tail(-1, num_seed + 1)) return rc;
  for (int i = num_seed; i < longest; ++i) {
    if (int rc = run_step_img(m, s, mode, plan)) return rc;
    if (int rc = tail(i, i + 1 < longest ? i + 2 : 0)) return rc;
  }
  return finish(m, s, {{out, w.x, n * 4}});
}

int fd_denoise_loss(fd_model* m, const float* x0, const float* noise, const int32_t* t, const float* keep, const float* spread,
                    const int32_t* lens, int B, int L, float beta_ang, float beta_lin, double* sums, float* corrupted_out,
                    float* eps_out) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x0 || !noise || !t || !lens || !sums) return fail(FD_E_INVALID, "null argument");
  if ((keep == nullptr) != (spread == nullptr)) return fail(FD_E_INVALID, "null argument: keep and spread go together");
  if (!(beta_ang > 0.f) || !(beta_lin > 0.f)) return fail(FD_E_INVALID, "beta_ang=%g beta_lin=%g must be > 0", beta_ang, beta_lin);
  if (int rc = check_t_seq(m, t, B)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  Call c;
  if (int rc = open_ws(m, B, L, nullptr, &c)) return rc;
  Workspace& w = *c.ws;
  const int F = m->cfg.n_features;
  const size_t n = c.n, nb = (size_t)B;
  hipStream_t s = c.s;
  // the lazily allocated buffers first: an out-of-memory return must not leave copies from this frame in flight
  if (!w.loss_in) HIP_TRY(hipMalloc((void**)&w.loss_in, (2 * n + 4 * nb) * 4));
  if (!w.loss_sums) HIP_TRY(hipMalloc((void**)&w.loss_sums, nb * F * 8));
  PackedUpload up(w.loss_in);  // x0 | noise | keep | spread | t | lens
  const float *x0_dev = up.add(x0, n), *noise_dev = up.add(noise, n), *keep_dev = up.add(keep, nb), *spread_dev = up.add(spread, nb),
              *t_dev = up.add(t, nb), *lens_dev = up.add(lens, nb);
  if (int rc = up.send(s)) return rc;
  // without keep and spread x0 is x_t already
  if (int rc = loss_forward(m, c, B, L, x0_dev, noise_dev, keep_dev, spread_dev, keep ? nullptr : x0_dev, t_dev, lens_dev)) return rc;
  launch_loss_terms(w.eps, noise_dev, w.lens, B, L, F, m->angle_mask, beta_ang, beta_lin, w.loss_sums, nullptr, s);
  HIP_TRY(hipGetLastError());
  return finish(m, s, {{sums, w.loss_sums, nb * F * 8}, {corrupted_out, w.x, n * 4}, {eps_out, w.eps, n * 4}});
}

int fd_denoise_loss_ex(fd_model* m, const float* x0, const float* corrupted, const float* noise, const int32_t* t,
                       const float* keep, const float* spread, const int32_t* lens, int B, int L, int kind, float beta_ang,
                       float beta_lin, const float* coef, const int32_t* feat_idx, double* sums, int64_t* turns,
                       double* pair_sums, int64_t* pairs, float* corrupted_out, float* eps_out) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x0 || !noise || !t || !lens || !sums) return fail(FD_E_INVALID, "null argument");
  if ((keep == nullptr) != (spread == nullptr)) return fail(FD_E_INVALID, "null argument: keep and spread go together");
  if (!corrupted && !keep) return fail(FD_E_INVALID, "null argument: without corrupted the device noises x0 and needs keep and spread");
  if (kind != 0 && kind != 1) return fail(FD_E_INVALID, "kind=%d: 0 (smooth_l1) or 1 (l1)", kind);
  if (!(beta_ang > 0.f) || !(beta_lin > 0.f)) return fail(FD_E_INVALID, "beta_ang=%g beta_lin=%g must be > 0", beta_ang, beta_lin);
  const int F = m->cfg.n_features;
  if (pair_sums) {
    if (!keep) return fail(FD_E_INVALID, "null argument: the pairwise term needs keep and spread");
    if (!pairs || !feat_idx) return fail(FD_E_INVALID, "null argument: the pairwise term needs pairs and feat_idx");
    if (int rc = check_pairwise(keep, coef, feat_idx, B, L, F)) return rc;
  }
  if (int rc = check_t_seq(m, t, B)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  Call c;
  if (int rc = open_ws(m, B, L, nullptr, &c)) return rc;
  Workspace& w = *c.ws;
  const size_t n = c.n, nb = (size_t)B, nf = nb * F;
  hipStream_t s = c.s;
  // the lazily allocated buffers first: an out-of-memory return must not leave copies from this frame in flight
  if (!w.loss_ex_in) HIP_TRY(hipMalloc((void**)&w.loss_ex_in, (3 * n + 5 * nb) * 4));
  if (!w.loss_ex_out) HIP_TRY(hipMalloc((void**)&w.loss_ex_out, (2 * nf + 2 * nb) * 8));
  PackedUpload up(w.loss_ex_in);  // x0 | noise | corrupted | keep | spread | coef | t | lens
  const float *x0_dev = up.add(x0, n), *noise_dev = up.add(noise, n), *corrupted_dev = up.add(corrupted, n), *keep_dev = up.add(keep, nb),
              *spread_dev = up.add(spread, nb), *coef_dev = up.add(coef, nb), *t_dev = up.add(t, nb), *lens_dev = up.add(lens, nb);
  if (int rc = up.send(s)) return rc;
  if (int rc = loss_forward(m, c, B, L, x0_dev, noise_dev, keep_dev, spread_dev, corrupted ? corrupted_dev : nullptr, t_dev, lens_dev))
    return rc;
  double* sums_dev = w.loss_ex_out;
  long long* turns_dev = (long long*)(w.loss_ex_out + nf);
  double* pair_sums_dev = w.loss_ex_out + 2 * nf;
  long long* pairs_dev = (long long*)(w.loss_ex_out + 2 * nf + nb);
  launch_loss_terms_ex(w.eps, noise_dev, w.lens, B, L, F, m->angle_mask, kind, beta_ang, beta_lin, sums_dev, nullptr,
                       turns ? turns_dev : nullptr, s);
  HIP_TRY(hipGetLastError());
  if (pair_sums) {  // the forward's x_t and prediction stay where they are: w.x, w.eps
    const PairwiseFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5]};
    launch_pairwise_dist(x0_dev, w.x, w.eps, keep_dev, spread_dev, coef ? coef_dev : nullptr, w.lens, B, L, F, fx, pair_sums_dev,
                         pairs_dev, nullptr, s);
    HIP_TRY(hipGetLastError());
  }
  // ONE download of what was asked for: sums [| turns] [| pair_sums | pairs] are contiguous up to the last one wanted
  const size_t words = pair_sums ? 2 * nf + 2 * nb : turns ? 2 * nf : nf;
  std::vector<double> back(words);
  if (int rc = finish(m, s, {{back.data(), w.loss_ex_out, words * 8}, {corrupted_out, w.x, n * 4}, {eps_out, w.eps, n * 4}})) return rc;
  memcpy(sums, back.data(), nf * 8);
  if (turns) memcpy(turns, back.data() + nf, nf * 8);
  if (pair_sums) {
    memcpy(pair_sums, back.data() + 2 * nf, nb * 8);
    memcpy(pairs, back.data() + 2 * nf + nb, nb * 8);
  }
  return FD_OK;
}

int fd_forward_ex(fd_model* m, const float* x, int t, const uint8_t* key_mask, const int32_t* position_ids, int B, int L,
                  float* eps_out) {
  if (int rc = check_shape(m, B, L, t)) return rc;
  if (!x || !eps_out) return fail(FD_E_INVALID, "null argument");
  if (!key_mask && !position_ids) return fail(FD_E_INVALID, "fd_forward_ex without a mask and without position ids: use fd_forward");
  if (!m->img) return fail(FD_E_UNSUPPORTED, "fd_forward_ex (arbitrary key masks / position ids) needs FD_PREC_F16X3");
  const fd_config& cfg = m->cfg;
  if (position_ids && cfg.pos_type == FD_POS_ABSOLUTE)
    for (size_t i = 0; i < (size_t)B * L; ++i)
      if (position_ids[i] < 0 || position_ids[i] >= cfg.max_pos)
        return fail(FD_E_INVALID, "position_ids[%zu]=%d outside [0, %d)", i, position_ids[i], cfg.max_pos);
  Call c;
  if (int rc = open_ws(m, B, L, nullptr, &c)) return rc;
  Workspace& w = *c.ws;
  hipStream_t s = c.s;
  // the lazily allocated buffers first: an out-of-memory return must not leave copies from this frame in flight
  if (key_mask && !w.kmask) HIP_TRY(hipMalloc((void**)&w.kmask, (size_t)B * L));
  if (position_ids && cfg.pos_type == FD_POS_ABSOLUTE && !w.pos_ids) HIP_TRY(hipMalloc((void**)&w.pos_ids, (size_t)B * L * 4));
  std::vector<int32_t> lens(B, L);  // every position is a row and a key; what is attended to is the mask's business
  // `lens` is a pageable vector of this frame, and the early returns below would destroy it under an asynchronous copy: a blocking
  // one -- which goes through the NULL stream and is not ordered against work still queued on the model's non-blocking stream (an
  // earlier asynchronous entry point reading w.lens), so that stream is drained first
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(w.lens, lens.data(), (size_t)B * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpyAsync(w.x, x, c.n * 4, hipMemcpyHostToDevice, s));
  StepMode mode{};
  mode.forward_only = true;
  if (key_mask) {
    HIP_TRY(hipMemcpyAsync(w.kmask, key_mask, (size_t)B * L, hipMemcpyHostToDevice, s));
    mode.kmask = w.kmask;
  }
  // (relative position types: the reference's embeddings add no position embedding and HF's distance uses arange, so
  // position_ids change nothing there -- modelling.py:157-166, BertSelfAttention)
  if (position_ids && cfg.pos_type == FD_POS_ABSOLUTE) {
    HIP_TRY(hipMemcpyAsync(w.pos_ids, position_ids, (size_t)B * L * 4, hipMemcpyHostToDevice, s));
    mode.pos_ids = w.pos_ids;
  }
  if (int rc = prepare_rows(m, s, 0)) return rc;
  if (int rc = set_t(m, s, t)) return rc;
  if (int rc = run_step(m, s, mode)) return rc;
  return finish(m, s, {{eps_out, w.eps, c.n * 4}});
}

int fd_p_sample_step(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, const float* z, int wrap,
                     float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (t > 0 && !z) return fail(FD_E_INVALID, "z is required for t > 0");
  if (int rc = check_lens(lens, B, L)) return rc;
  return host_step(m, StepHost{x, t, lens, B, L, wrap, z}, StepMode{}, x_out, nullptr, nullptr);
}

int fd_p_sample_step_inpaint(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, const float* z, int wrap,
                             const float* known, const uint8_t* fixed, const float* known_coef, const float* z_known,
                             float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (t > 0 && !z) return fail(FD_E_INVALID, "z is required for t > 0");
  if (t > 0 && !z_known) return fail(FD_E_INVALID, "z_known is required for t > 0");
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  return host_step(m, StepHost{x, t, lens, B, L, wrap, z, true, {known, fixed, known_coef}, t > 0 ? z_known : nullptr}, StepMode{}, x_out,
                   nullptr, nullptr);
}

int fd_sample_begin_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, int t_start,
                        uint64_t seed, int64_t seq_offset, void* out_dev, int full_history, void* hip_stream) {
  return begin_run(m, x_init_dev, lens_dev, B, L, t_start, t_start + 1, seed, seq_offset, out_dev, full_history, hip_stream);
}

int fd_sample_steps_dev(fd_model* m, int n_steps, const void* noise_dev, int noise_t0, void* hip_stream) {
  if (!m || !m->finalized || m->ws.B == 0) return fail(FD_E_STATE, "fd_sample_steps_dev without fd_sample_begin_dev");
  if (!m->run_open) return fail(FD_E_STATE, "fd_sample_steps_dev: no sampling run in progress (another call on this model has taken its workspace)");
  if (m->ws.B != m->run_B || m->ws.L != m->run_L)
    return fail(FD_E_STATE, "fd_sample_steps_dev: the workspace now holds B=%d L=%d, the run was begun with B=%d L=%d", m->ws.B, m->ws.L, m->run_B, m->run_L);
  if (n_steps < 0 || n_steps > m->run_t + 1) return fail(FD_E_INVALID, "n_steps = %d with %d steps left", n_steps, m->run_t + 1);
  if (noise_dev && (noise_t0 < 0 || noise_t0 > m->run_t - n_steps + 1))  // (the row of t = 0 is read too, and multiplied by sigma_0 = 0)
    return fail(FD_E_INVALID, "noise rows start at t = %d, the steps run down to t = %d", noise_t0, m->run_t - n_steps + 1);
  HIP_TRY(hipSetDevice(m->device));
  Workspace& w = m->ws;
  hipStream_t s = stream_of(m, hip_stream);
  // the kernel reads the draw of step t at noise + t * (B L F): rebase the chunk (row 0 = step noise_t0)
  const size_t n = (size_t)w.B * w.L * m->cfg.n_features;
  UpdateDyn dyn = m->dyn_host;
  dyn.noise = noise_dev ? static_cast<const float*>(noise_dev) - (ptrdiff_t)noise_t0 * (ptrdiff_t)n : nullptr;
  send_dyn(m, s, dyn);
  for (int i = 0; i < n_steps; ++i) {
    const int done = m->run_n - 1 - m->run_t;  // steps already run
    const bool prof = m->profile_every > 0 && (done % m->profile_every) == m->profile_every / 2;
    if (m->use_graph && !prof) {
      HIP_TRY(hipGraphLaunch(w.graph, s));
    } else {
      StepMode mode{};
      mode.use_dyn = true;
      mode.advance = true;
      mode.profile = prof;
      if (int rc = run_step(m, s, mode)) return rc;
    }
    --m->run_t;
  }
  return FD_OK;
}

int fd_sample_end_dev(fd_model* m, void* out_dev, void* hip_stream) {
  if (!m || !m->finalized || m->ws.B == 0) return fail(FD_E_STATE, "fd_sample_end_dev without fd_sample_begin_dev");
  if (!m->run_open) return fail(FD_E_STATE, "fd_sample_end_dev: no sampling run in progress (another call on this model has taken its workspace)");
  if (m->run_t >= 0) return fail(FD_E_STATE, "%d reverse steps have not been run", m->run_t + 1);
  if (m->ws.B != m->run_B || m->ws.L != m->run_L)
    return fail(FD_E_STATE, "fd_sample_end_dev: the workspace now holds B=%d L=%d, the run was begun with B=%d L=%d", m->ws.B, m->ws.L, m->run_B, m->run_L);
  HIP_TRY(hipSetDevice(m->device));
  Workspace& w = m->ws;
  hipStream_t s = stream_of(m, hip_stream);
  const size_t n = (size_t)w.B * w.L * m->cfg.n_features;
  if (!m->dyn_host.hist_every) HIP_TRY(hipMemcpyAsync(out_dev, w.x, n * 4, hipMemcpyDeviceToDevice, s));
  m->run_open = false;
  return FD_OK;
}

int fd_sample_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, int t_start,
                  const void* noise_dev, uint64_t seed, int64_t seq_offset, void* out_dev, int full_history,
                  void* hip_stream) {
  if (int rc = fd_sample_begin_dev(m, x_init_dev, lens_dev, B, L, t_start, seed, seq_offset, out_dev, full_history, hip_stream))
    return rc;
  if (int rc = fd_sample_steps_dev(m, t_start + 1, noise_dev, 0, hip_stream)) return rc;
  return fd_sample_end_dev(m, out_dev, hip_stream);
}

int fd_sample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
              uint64_t seed, float* out, int full_history) {
  return fd_sample_ex(m, x_init, lens, B, L, t_start, noise, seed, 0, out, full_history);
}

int fd_sample_ex(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
                 uint64_t seed, int64_t seq_offset, float* out, int full_history) {
  if (int rc = check_run_call(m, x_init, lens, out, B, L, t_start, full_history)) return rc;
  return host_run(m, LadderRun{{x_init, lens, B, L, (size_t)t_start + 1, noise, nullptr, seed, seq_offset, out, full_history}, t_start});
}

int fd_sample_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
                      const float* known, const uint8_t* fixed, const float* known_coef, const float* known_noise,
                      uint64_t seed, int64_t seq_offset, float* out, int full_history) {
  if (int rc = check_run_call(m, x_init, lens, out, B, L, t_start, full_history)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  return host_run(m, LadderRun{{x_init, lens, B, L, (size_t)t_start + 1, noise, known_noise, seed, seq_offset, out, full_history},
                               t_start, {known, fixed, known_coef}});
}

int fd_sample_inpaint_resample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start,
                               const float* known, const uint8_t* fixed, const float* known_coef, const int32_t* visits,
                               int n_visits, const float* jump_coef, uint64_t seed, int64_t seq_offset, float* out) {
  if (int rc = check_run_call(m, x_init, lens, out, B, L, t_start, 0)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  if (int rc = check_jump_tag(m)) return rc;
  int n_jumps = 0;
  if (int rc = check_visits(visits, n_visits, t_start, jump_coef, &n_jumps)) return rc;
  return host_run(m, LadderRun{{x_init, lens, B, L, (size_t)t_start + 1, nullptr, nullptr, seed, seq_offset, out, 0}, t_start,
                               {known, fixed, known_coef}, visits, n_visits, jump_coef});
}

int fd_inpaint_jump(fd_model* m, const float* x, const int32_t* lens, int B, int L, int level_to, float jk, float js,
                    const float* known, const uint8_t* fixed, const float* known_coef, uint64_t seed, int64_t seq_offset,
                    float* x_out) {
  if (int rc = check_shape(m, B, L, 0)) return rc;
  if (!x || !lens || !x_out) return fail(FD_E_INVALID, "null argument");
  if (level_to < 1 || level_to > m->T) return fail(FD_E_INVALID, "level_to = %d outside [1, %d]", level_to, m->T);
  if (int rc = check_jump_tag(m)) return rc;
  if (int rc = check_jump_coef(jk, js, 0)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  Call c;
  if (int rc = open_call(m, x, lens, nullptr, B, L, &c)) return rc;
  Workspace& w = *c.ws;
  InpaintDev ip;
  if (int rc = stage_inpaint(m, c.s, InpaintHost{known, fixed, known_coef}, &ip)) return rc;
  launch_inpaint_jump(w.x, w.lens, ip.known, ip.fixed, ip.coef, m->T, level_to, jk, js, seed, seq_offset, B, L, m->cfg.n_features,
                      m->angle_mask, c.s);
  HIP_TRY(hipGetLastError());
  return download_sync(c.s, {{x_out, w.x, c.n * 4}});  // (nothing ran that raises the non-finite flag)
}

int fd_sample_strided_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, const int32_t* visits,
                          int n_visits, const float* coef, const void* noise_dev, uint64_t seed, int64_t seq_offset, void* out_dev,
                          int full_history, void* hip_stream) {
  if (int rc = check_strided_call(m, x_init_dev, lens_dev, out_dev, B, L, visits, n_visits, coef, full_history)) return rc;
  return strided_run_dev(m, x_init_dev, lens_dev, B, L, visits, n_visits, coef, false, noise_dev, seed, seq_offset, out_dev,
                         full_history, hip_stream);
}

int fd_sample_strided(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                      const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, float* out, int full_history) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, full_history)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  return strided_run_host(m, {x_init, lens, B, L, (size_t)n_visits, noise, nullptr, seed, seq_offset, out, full_history}, visits, coef, false);
}

int fd_p_sample_step_coef(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                          const float* z, int wrap, float* eps_out, float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (int rc = check_finite_coef("abs", {a, b, s})) return rc;
  if (s != 0.f && !z) return fail(FD_E_INVALID, "z is required for s != 0");
  if (int rc = check_lens(lens, B, L)) return rc;
  return host_step(m, StepHost{x, t, lens, B, L, wrap, s != 0.f ? z : nullptr}, strided_mode(a, b, s), x_out, eps_out, nullptr);
}

int fd_sample_strided_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                              int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                              const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset, float* out,
                              int full_history) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, full_history)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  return strided_host_run(m, StridedHostRun{{x_init, lens, B, L, (size_t)n_visits, noise, known_noise, seed, seq_offset, out, full_history},
                                            visits, coef, {known, fixed, known_coef}});
}

int fd_sample_strided_inpaint_resample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* grid,
                                       int n_grid, const float* coef, const int32_t* run, int n_run, const float* jump_coef,
                                       const float* known, const uint8_t* fixed, const float* known_coef, uint64_t seed,
                                       int64_t seq_offset, float* out) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, grid, n_grid, coef, 0)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  if (int rc = check_jump_tag(m)) return rc;
  int n_jumps = 0;
  if (int rc = check_strided_visits(m, grid, n_grid, run, n_run, jump_coef, &n_jumps)) return rc;
  return strided_host_run(m, StridedHostRun{{x_init, lens, B, L, (size_t)n_grid, nullptr, nullptr, seed, seq_offset, out, 0}, grid, coef,
                                            {known, fixed, known_coef}, run, n_run, jump_coef});
}

int fd_p_sample_step_coef_inpaint(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                                  const float* z, int wrap, int level_out, const float* known, const uint8_t* fixed,
                                  const float* known_coef, const float* z_known, float* eps_out, float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (int rc = check_finite_coef("abs", {a, b, s})) return rc;
  if (s != 0.f && !z) return fail(FD_E_INVALID, "z is required for s != 0");
  if (level_out < 0 || level_out > m->T) return fail(FD_E_INVALID, "level_out = %d outside [0, %d]", level_out, m->T);
  if (level_out >= 1 && !z_known) return fail(FD_E_INVALID, "z_known is required for level_out >= 1");
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  StepMode mode = strided_mode(a, b, s);
  mode.level_out = level_out;
  return host_step(m, StepHost{x, t, lens, B, L, wrap, s != 0.f ? z : nullptr, true, {known, fixed, known_coef},
                               level_out >= 1 ? z_known : nullptr},
                   mode, x_out, eps_out, nullptr);
}

int fd_sample_solver_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, const int32_t* visits,
                         int n_visits, const float* coef, void* out_dev, int full_history, void* hip_stream) {
  if (int rc = check_strided_call(m, x_init_dev, lens_dev, out_dev, B, L, visits, n_visits, coef, full_history, true)) return rc;
  return strided_run_dev(m, x_init_dev, lens_dev, B, L, visits, n_visits, coef, true, nullptr, 0, 0, out_dev, full_history, hip_stream);
}

int fd_sample_solver(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, float* out, int full_history) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, full_history, true)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  return strided_run_host(m, {x_init, lens, B, L, (size_t)n_visits, nullptr, nullptr, 0, 0, out, full_history}, visits, coef, true);
}

int fd_p_sample_step_solver(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float c, float u,
                            float v, const float* x0_prev, int wrap, float* eps_out, float* x0_out, float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (int rc = check_finite_coef("abcuv", {a, b, c, u, v})) return rc;
  if (c != 0.f && !x0_prev) return fail(FD_E_INVALID, "x0_prev is required for c != 0");
  if (int rc = check_lens(lens, B, L)) return rc;
  HIP_TRY(hipSetDevice(m->device));
  // the previous and the new prediction in buffers of the call, allocated (and the previous one uploaded, blocking) before
  // anything of this frame is queued; a given x0_prev is uploaded whatever c is, and not read where c == 0
  const size_t n = (size_t)B * L * m->cfg.n_features;
  DeviceBufs bufs;
  float *d_prev, *d_x0;
  HIP_TRY(bufs.alloc(n * 4, &d_prev));
  HIP_TRY(bufs.alloc(n * 4, &d_x0));
  if (x0_prev) HIP_TRY(hipMemcpy(d_prev, x0_prev, n * 4, hipMemcpyHostToDevice));
  StepMode mode = strided_mode(a, b, 0.f);
  mode.sc = c; mode.su = u; mode.sv = v;
  mode.x0_prev = d_prev;
  mode.x0_out = d_x0;
  StepHost h{x, t, lens, B, L, wrap};
  h.draws = false;
  return host_step(m, h, mode, x_out, eps_out, x0_out);
}

int fd_p_sample_step_coef_x0(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                             float u, float v, const float* z, int wrap, float* eps_out, float* x0_out, float* x_out) {
  if (int rc = check_step_call(m, x, lens, x_out, B, L, t)) return rc;
  if (!x0_out) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_finite_coef("absuv", {a, b, s, u, v})) return rc;
  if (s != 0.f && !z) return fail(FD_E_INVALID, "z is required for s != 0");
  if (int rc = check_lens(lens, B, L)) return rc;
  HIP_TRY(hipSetDevice(m->device));
  DeviceBufs bufs;
  float* d_x0;
  HIP_TRY(bufs.alloc((size_t)B * L * m->cfg.n_features * 4, &d_x0));  // (before anything of this frame is queued)
  StepMode mode = strided_mode(a, b, s);
  mode.su = u; mode.sv = v;
  mode.x0_out = d_x0;
  mode.x0_only = true;
  return host_step(m, StepHost{x, t, lens, B, L, wrap, s != 0.f ? z : nullptr}, mode, x_out, eps_out, x0_out);
}

int fd_sample_steered(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                      const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const uint8_t* event,
                      int n_particles, const fd_steer_params* params, const double* u, float* out, double* terms_out,
                      double* reward_out, double* logw_out, int32_t* ancestors_out) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, 0)) return rc;  // (rows a | b | s too)
  if (int rc = check_coef_rows(coef, n_visits, 3, 5)) return rc;
  if (!event || !u || !params) return fail(FD_E_INVALID, "null argument: event, u and params are required");
  if (!terms_out || !reward_out || !logw_out) return fail(FD_E_INVALID, "null argument: terms_out, reward_out and logw_out are required");
  if (n_particles < 1 || n_particles > kSteerMaxParticles)
    return fail(FD_E_INVALID, "n_particles = %d outside [1, %d]", n_particles, kSteerMaxParticles);
  if (B % n_particles != 0) return fail(FD_E_INVALID, "B = %d is not a multiple of n_particles = %d", B, n_particles);
  if (int rc = check_lens(lens, B, L)) return rc;
  for (int b = 0; b < B; ++b)
    if (lens[b] != lens[b - b % n_particles])
      return fail(FD_E_INVALID, "lens[%d] = %d, the first particle of its group has %d: a group shares one length", b, lens[b],
                  lens[b - b % n_particles]);
  if (!std::isfinite(params->lambda)) return fail(FD_E_INVALID, "lambda = %g must be finite", params->lambda);
  if (!(params->ess_frac >= 0.0)) return fail(FD_E_INVALID, "ess_frac = %g must be >= 0", params->ess_frac);
  if (int rc = check_steer(lens, B, L, m->cfg.n_features, params->feat_idx, params->weights, params->clash_alpha,
                           params->has_offset ? params->offset : nullptr))
    return rc;
  int n_events = 0;
  for (int i = 0; i < n_visits; ++i) n_events += event[i] ? 1 : 0;
  if (int rc = check_steer_u(u, (size_t)n_events * (size_t)(B / n_particles))) return rc;
  return steered_host_run(m, SteeredHostRun{{x_init, lens, B, L, (size_t)n_visits, noise, nullptr, seed, seq_offset, out, 0}, visits, coef,
                                            event, n_events, n_particles, params, u, terms_out, reward_out, logw_out, ancestors_out});
}

int fd_sample_repeat(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const int32_t* tie, float* out) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, 0)) return rc;
  if (!tie) return fail(FD_E_INVALID, "null argument: tie is required");
  if (int rc = check_lens(lens, B, L)) return rc;
  if (int rc = check_tie(tie, lens, B)) return rc;
  return repeat_host_run(m, {x_init, lens, B, L, (size_t)n_visits, noise, nullptr, seed, seq_offset, out, 0}, visits, coef, tie);
}

int fd_sample_guided(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const float* guide,
                     const fd_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i, const int32_t* rst_j,
                     const double* rst_d0, const double* rst_tol, const double* rst_w, float* out, double* energy_out,
                     double* max_violation_out) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, 0)) return rc;  // (rows a | b | s too)
  if (int rc = check_coef_rows(coef, n_visits, 3, 5)) return rc;
  if (!guide || !params) return fail(FD_E_INVALID, "null argument: guide and params are required");
  if (!energy_out || !max_violation_out) return fail(FD_E_INVALID, "null argument: energy_out and max_violation_out are required");
  for (int i = 0; i < n_visits; ++i)
    if (!std::isfinite(guide[i])) return fail(FD_E_INVALID, "guide[%d] = %g is not finite", i, (double)guide[i]);
  if (int rc = check_guide_shape(lens, B, L, m->cfg.n_features, params->feat_idx)) return rc;
  if (int rc = check_guide_scalars(params->max_norm, params->has_offset ? params->offset : nullptr, m->cfg.n_features)) return rc;
  const RestraintLists rl{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w};
  if (int rc = check_restraints(rl, lens)) return rc;
  return guided_host_run(m, GuidedHostRun{{x_init, lens, B, L, (size_t)n_visits, noise, nullptr, seed, seq_offset, out, 0}, visits, coef,
                                          guide, params, rl, energy_out, max_violation_out});
}

}  // extern "C"

// fd_sample_guided_inpaint (n_energies == 2, no template) and fd_sample_guided_inpaint_tpl (3): the checks, then the run
static int guided_inpaint_entry(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                                const float* coef, const float* noise, const float* known, const uint8_t* fixed, const float* known_coef,
                                const float* known_noise, uint64_t seed, int64_t seq_offset, const float* guide,
                                const fd_scaffold_guide_params* params, const RestraintLists& rl, const TemplateLists& tl, int n_energies,
                                float* out, double* energy_out, double* max_violation_out, double* tpl_rmsd_out,
                                const int32_t* sym_order = nullptr, const double* sym_pose0 = nullptr,
                                const fd_symmetry_params* sym_params = nullptr, double* sym_energy_out = nullptr,
                                int32_t* sym_contacts_out = nullptr, double* sym_pose_out = nullptr) {
  if (int rc = check_strided_call(m, x_init, lens, out, B, L, visits, n_visits, coef, 0)) return rc;  // (rows a | b | s too)
  if (int rc = check_coef_rows(coef, n_visits, 3, 5)) return rc;
  if (!guide || !params) return fail(FD_E_INVALID, "null argument: guide and params are required");
  if (!energy_out || !max_violation_out) return fail(FD_E_INVALID, "null argument: energy_out and max_violation_out are required");
  if (n_energies == 3 && !tpl_rmsd_out) return fail(FD_E_INVALID, "null argument: tpl_rmsd_out is required");
  for (int i = 0; i < n_visits; ++i)
    if (!std::isfinite(guide[i])) return fail(FD_E_INVALID, "guide[%d] = %g is not finite", i, (double)guide[i]);
  if (int rc = check_guide_shape(lens, B, L, m->cfg.n_features, params->feat_idx)) return rc;
  if (int rc = check_inpaint(known, fixed, known_coef, lens, B, L, m->cfg.n_features)) return rc;
  if (int rc = check_scaffold_guide(*params, known, fixed, lens, B, L, m->cfg.n_features)) return rc;
  if (int rc = check_restraints(rl, lens)) return rc;
  if (int rc = check_template(tl, lens)) return rc;
  if (sym_order) {
    if (!sym_pose0 || !sym_params || !sym_energy_out || !sym_contacts_out || !sym_pose_out)
      return fail(FD_E_INVALID, "null argument: the symmetry arrays");
    if (int rc = check_symmetry(*sym_params, sym_order, sym_pose0, B)) return rc;
  }
  return scaffold_guided_host_run(m, ScaffoldGuidedHostRun{{x_init, lens, B, L, (size_t)n_visits, noise, known_noise, seed, seq_offset, out, 0},
                                                           visits, coef, guide, {known, fixed, known_coef}, params, rl, tl, n_energies,
                                                           energy_out, max_violation_out, tpl_rmsd_out, sym_order, sym_pose0, sym_params,
                                                           sym_energy_out, sym_contacts_out, sym_pose_out});
}

extern "C" {

int fd_sample_guided_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                             const float* coef, const float* noise, const float* known, const uint8_t* fixed, const float* known_coef,
                             const float* known_noise, uint64_t seed, int64_t seq_offset, const float* guide,
                             const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                             const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float* out,
                             double* energy_out, double* max_violation_out) {
  return guided_inpaint_entry(m, x_init, lens, B, L, visits, n_visits, coef, noise, known, fixed, known_coef, known_noise, seed, seq_offset,
                              guide, params, RestraintLists{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w},
                              TemplateLists{B, nullptr, nullptr, nullptr, nullptr}, 2, out, energy_out, max_violation_out, nullptr);
}

int fd_sample_guided_inpaint_tpl(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                                 int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                                 const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset,
                                 const float* guide, const fd_scaffold_guide_params* params, const int32_t* rst_offsets,
                                 const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol,
                                 const double* rst_w, const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz,
                                 const double* tpl_w, float* out, double* energy_out, double* max_violation_out, double* tpl_rmsd_out) {
  return guided_inpaint_entry(m, x_init, lens, B, L, visits, n_visits, coef, noise, known, fixed, known_coef, known_noise, seed, seq_offset,
                              guide, params, RestraintLists{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w},
                              TemplateLists{B, tpl_offsets, tpl_atom, tpl_xyz, tpl_w}, 3, out, energy_out, max_violation_out, tpl_rmsd_out);
}

int fd_sample_guided_inpaint_sym(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                                 int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                                 const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset,
                                 const float* guide, const fd_scaffold_guide_params* params, const int32_t* rst_offsets,
                                 const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol,
                                 const double* rst_w, const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz,
                                 const double* tpl_w, const int32_t* sym_order, const double* sym_pose0,
                                 const fd_symmetry_params* sym_params, float* out, double* energy_out, double* max_violation_out,
                                 double* tpl_rmsd_out, double* sym_energy_out, int32_t* sym_contacts_out, double* sym_pose_out) {
  return guided_inpaint_entry(m, x_init, lens, B, L, visits, n_visits, coef, noise, known, fixed, known_coef, known_noise, seed, seq_offset,
                              guide, params, RestraintLists{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w},
                              TemplateLists{B, tpl_offsets, tpl_atom, tpl_xyz, tpl_w}, 3, out, energy_out, max_violation_out, tpl_rmsd_out,
                              sym_order, sym_pose0, sym_params, sym_energy_out, sym_contacts_out, sym_pose_out);
}

int fd_philox_normal_dev(fd_model* m, uint64_t seed, int t, int64_t seq_offset, int B, int L, void* out_dev,
                         void* hip_stream) {
  if (!m || !out_dev) return fail(FD_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(m->device));
  launch_philox_fill(static_cast<float*>(out_dev), seed, t, seq_offset, B, L, m->cfg.n_features, stream_of(m, hip_stream));
  HIP_TRY(hipGetLastError());
  return FD_OK;
}

int fd_shift_trim_dev(fd_model* m, const void* traj_dev, int rows, int B, int L, const void* lens_dev, const void* item_off_dev,
                      const float* offset, void* out_dev, void* hip_stream) {
  if (!m || !traj_dev || !lens_dev || !item_off_dev || !out_dev) return fail(FD_E_INVALID, "null argument");
  if (!m->finalized) return fail(FD_E_STATE, "fd_finalize has not been called");
  if (rows < 1 || B < 1 || L < 1) return fail(FD_E_INVALID, "rows=%d B=%d L=%d must be positive", rows, B, L);
  if ((long long)rows * B > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "rows x B = %lld blocks", (long long)rows * B);
  HIP_TRY(hipSetDevice(m->device));
  ShiftTrimArgs a;
  memset(&a, 0, sizeof a);
  a.traj = static_cast<const float*>(traj_dev); a.lens = static_cast<const int*>(lens_dev);
  a.item_off = static_cast<const long long*>(item_off_dev); a.out = static_cast<float*>(out_dev);
  a.rows = rows; a.B = B; a.L = L; a.F = m->cfg.n_features;
  a.angle_mask = m->angle_mask;
  a.has_offset = offset ? 1 : 0;
  if (offset)
    for (int f = 0; f < a.F; ++f) a.offset[f] = offset[f];
  launch_shift_trim(a, stream_of(m, hip_stream));
  HIP_TRY(hipGetLastError());
  return FD_OK;
}

}  // extern "C"
