// C-ABI host side of libfdmi.so, the part that holds a model as it runs: the error string, workspaces, the launch plan of
// a timestep, the step itself, the captured step graph, and the create / destroy / option / profile / debug entries.  The
// model's weights (fd_set_weight, fd_finalize: packing through weight_pack.h, upload) are api_weights.hip, its RCCL binding
// api_comm.hip, and the entry points that run the model (forward, loss, sampling) api_run.hip; the four see each other through
// model.h.  The entry points that take a device_id instead of an fd_model live beside them: api_structures.hip (fd_nerf,
// fd_internal_coords, fd_superpose_rmsd, fd_tm_score, fd_annotate_sse, fd_tm_align) and api_hooks.hip (the fd_test_* hooks);
// what all of them share -- the error string, HIP_TRY, the owner of call-scoped device buffers -- is host_common.h.
// Boundary: include/fdmi.h (each entry point cites the reference function it replaces).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fdmi.h"
#include "fdmi_kernels.h"
#include "host_common.h"
#include "launch_common.h"
#include "model.h"

using namespace fdmi;

namespace {
thread_local std::string g_err;  // one per thread for the whole library: fail() writes it, fd_last_error() reads it
}

int fdmi::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

// debug cycle stamps (FDMI_STAMPS=1), one table per kernel family back to back (in 8-byte words): the GEMMs' [5][8][64][6] first
constexpr long long kStampAttn = 5 * 8 * 64 * 6;                     // attention [4][64][8]
constexpr long long kStampSeqAttn = kStampAttn + 4 * 64 * 8;          // fused attention [4][64][16] (+ 32 K floats of register dumps, seq_attn.hip FDMI_SA_DUMP)
constexpr long long kStampFfn = kStampSeqAttn + 4 * 64 * 16 + 16384;  // ffn16.hip's [8][16][16]
constexpr long long kStampWords = kStampFfn + 8 * 16 * 16;

size_t kHeadBytes(const fd_config& c) { return (size_t)(c.d_model / c.n_heads) * 4; }  // q / k / v image bytes per position and head

}  // namespace

void fdmi::drop_workspaces(fd_model* m) {
  m->ws.release();
  for (Workspace& w : m->cache) w.release();
  m->cache.clear();
}

int fdmi::ensure_ws(fd_model* m, int B, int L) {
  Workspace& w = m->ws;
  // every entry point that takes a workspace comes through here: a sampling run begun earlier (fd_sample_begin_dev) is over --
  // its state (x, the step counter) is about to be overwritten or parked; fd_sample_begin_dev re-opens one afterwards
  m->run_t = -1;
  m->run_open = false;
  const fd_config& c = m->cfg;
  const size_t M = (size_t)B * L, d = c.d_model, F = c.n_features;
  // algorithmic work per launch: 2*M*N*K for GEMMs, 6*L*d per token for attention
  {
    const double Md = (double)M, dd = (double)d, ff = (double)c.d_ff, Ld = (double)L;
    double* fl = m->prof_flops;
    double* by = m->prof_bytes;
    const bool img = m->img;
    fl[KC_EMBED] = 2 * Md * F * dd;            by[KC_EMBED] = 4 * (Md * F + Md * dd);
    // the row-image path computes V (transposed) in its own launch unless n_heads % 6 == 0 (one q | k | v launch)
    const int qn = (img && !(sub_heads(c) % 6 == 0 && !m->split_qkv)) ? 2 : 3;
    fl[KC_GEMM_QKV] = 2 * Md * qn * dd * dd;
    by[KC_GEMM_QKV] = 4 * (Md * dd + qn * dd * dd + Md * qn * dd);
    fl[KC_GEMM_V] = 2 * Md * dd * dd;          by[KC_GEMM_V] = 4 * (2 * Md * dd + dd * dd);
    fl[KC_ATTN] = 6 * Ld * dd * Md;            by[KC_ATTN] = 4 * (Md * 3 * dd + Md * dd);
    fl[KC_GEMM_OUT] = 2 * Md * dd * dd;        by[KC_GEMM_OUT] = 4 * (3 * Md * dd + dd * dd);
    fl[KC_LN1] = 0;                            by[KC_LN1] = 4 * 2 * Md * dd;
    fl[KC_GEMM_UP] = 2 * Md * ff * dd;         by[KC_GEMM_UP] = 4 * (Md * dd + ff * dd + Md * ff);
    fl[KC_GEMM_DOWN] = 2 * Md * ff * dd;       by[KC_GEMM_DOWN] = 4 * (Md * ff + ff * dd + 2 * Md * dd);
    fl[KC_LN2] = 0;                            by[KC_LN2] = 4 * 2 * Md * dd;
    fl[KC_GEMM_HEAD] = 2 * Md * dd * dd;       by[KC_GEMM_HEAD] = 4 * (2 * Md * dd + dd * dd);
    fl[KC_HEAD_UPDATE] = 2 * Md * dd * F;      by[KC_HEAD_UPDATE] = 4 * (Md * dd + 3 * Md * F);
    fl[KC_ADVANCE] = 0;                        by[KC_ADVANCE] = 4;
    // fused q | k | v projection + attention: h in, ctx out, the weights once (q, k, v stay on chip)
    fl[KC_SEQ_ATTN] = 2 * Md * 3 * dd * dd + 6 * Ld * dd * Md;  by[KC_SEQ_ATTN] = 4 * (2 * Md * dd + 3 * dd * dd);
    // fused BertIntermediate + BertOutput: a in, h out, both weight matrices once (the intermediate stays on chip)
    fl[KC_FFN] = 4 * Md * ff * dd;             by[KC_FFN] = 4 * (2 * Md * dd + 2 * ff * dd);
    // ... with BertSelfOutput in front: ctx and h in, h out, three weight matrices once
    fl[KC_TAIL] = 4 * Md * ff * dd + 2 * Md * dd * dd;  by[KC_TAIL] = 4 * (3 * Md * dd + 2 * ff * dd + dd * dd);
  }
  w.last_use = ++m->use_clock;
  if (w.B == B && w.L == L) return FD_OK;
  // park the current workspace and look for a cached one of this shape
  if (w.B != 0) {
    m->cache.push_back(w);
    w = Workspace();
  }
  for (size_t i = 0; i < m->cache.size(); ++i)
    if (m->cache[i].B == B && m->cache[i].L == L) {
      w = m->cache[i];
      m->cache.erase(m->cache.begin() + i);
      w.last_use = m->use_clock;
      return FD_OK;
    }
  while (m->cache.size() >= 3) {  // keep at most 4 shapes alive (C2-sized workspaces are about 1 GB each)
    HIP_TRY(hipStreamSynchronize(m->stream));
    size_t old = 0;
    for (size_t i = 1; i < m->cache.size(); ++i)
      if (m->cache[i].last_use < m->cache[old].last_use) old = i;
    m->cache[old].release();
    m->cache.erase(m->cache.begin() + old);
  }
  if (m->img) {  // every shape check comes BEFORE the first allocation: an early return must not leave buffers behind
    const int Tt = L > 128 ? 4 : (L + 31) / 32;
    const size_t ltot = (size_t)(L > 128 ? (L + 127) / 128 : 1) * 32 * Tt;
    if ((size_t)B * c.n_heads * ltot * kHeadBytes(c) >= (1ull << 32) - 65536)  // (32-bit offsets, the top bytes mark dropped stores)
      return fail(FD_E_UNSUPPORTED, "B=%lld x heads x L=%d: the q / k / v images of one batch must stay below 4 GiB; use smaller batches",
                  (long long)B, (int)L);
  }
  const int rc_alloc = [&]() -> int {
  auto al = [&](void** p, size_t bytes) -> hipError_t { return hipMalloc(p, bytes); };
  auto alz = [&](void** p, size_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(p, bytes);
    return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes, m->stream);
  };
  HIP_TRY(al((void**)&w.x, M * F * 4));
  HIP_TRY(alz((void**)&w.eps, M * F * 4));
  HIP_TRY(al((void**)&w.z, M * F * 4));
  HIP_TRY(al((void**)&w.lens, (size_t)B * 4));
  HIP_TRY(alz((void**)&w.t_dev, 16));
  HIP_TRY(alz((void**)&w.t_seq, (size_t)B * 4));
  HIP_TRY(al((void**)&w.dyn, sizeof(UpdateDyn)));
  if (m->img) {
    // Row images: sequences start at multiples of 8 rows, the row count is rounded up to whole 128-row tiles.
    // Everything is zeroed here: padding rows and never-written key slots start finite, and stay finite as long as every call's
    // values are.  A call that produced an inf / NaN ends in check_flag, which zeroes them again.
    const size_t Lr = (size_t)(L + 7) / 8 * 8;
    const size_t cap = (B * Lr + 127) / 128 * 128;
    const int T = L > 128 ? 4 : (L + 31) / 32;
    w.LPK = 32 * T;
    w.NKT = L > 128 ? (L + 127) / 128 : 1;
    w.LTOT = w.NKT * w.LPK;
    w.cap = (int)cap;
    const size_t BH = (size_t)B * sub_heads(c), gmax = c.d_ff > c.d_model ? c.d_ff : c.d_model;
    HIP_TRY(alz((void**)&w.himg, cap * d * 4));
    HIP_TRY(alz((void**)&w.aimg, cap * d * 4));
    HIP_TRY(alz((void**)&w.cimg, cap * d * 4));
    HIP_TRY(alz((void**)&w.gimg, cap * gmax * 4));
    if (d > 384) HIP_TRY(alz((void**)&w.tmp, cap * d * 4));  // pre-LayerNorm fp32 rows (un-fused LayerNorm path)
    HIP_TRY(alz((void**)&w.qbuf, BH * w.LTOT * 128));
    HIP_TRY(alz((void**)&w.kbuf, BH * w.LTOT * 128));
    HIP_TRY(alz((void**)&w.vbuf, BH * w.LTOT * 128));
    HIP_TRY(alz((void**)&w.trash, 1024));
    HIP_TRY(alz((void**)&w.rowinfo, cap * sizeof(int2)));
    HIP_TRY(alz((void**)&w.seq_row0, ((size_t)B + 1) * 4));
    HIP_TRY(alz((void**)&w.nrow, (size_t)B * 4));
    HIP_TRY(alz((void**)&w.dims, 16));
    HIP_TRY(alz((void**)&w.flag, 16));
    w.img = true;
  } else {
    const size_t gmax = c.d_ff > c.d_model ? c.d_ff : c.d_model;
    // Token-row buffers that feed or leave the LN-fused GEMMs are padded to whole 128-row tiles and
    // zeroed once: the fused kernels then run on full tiles for any B*L (rows are independent; the
    // padding rows stay finite and are never read back).
    const size_t Mp = (M + 127) / 128 * 128;
    HIP_TRY(alz((void**)&w.h, Mp * d * 4));
    HIP_TRY(alz((void**)&w.qkv, Mp * 3 * d * 4));
    HIP_TRY(alz((void**)&w.ctx, Mp * d * 4));
    HIP_TRY(alz((void**)&w.a, Mp * d * 4));
    HIP_TRY(al((void**)&w.tmp, M * d * 4));
    HIP_TRY(alz((void**)&w.g, Mp * gmax * 4));
  }
    return FD_OK;
  }();
  if (rc_alloc) {  // (out of memory, ...): give back what was allocated; w.B stays 0
    (void)hipStreamSynchronize(m->stream);
    w.release();
    return rc_alloc;
  }
  w.B = B;
  w.L = L;
  w.last_use = m->use_clock;
  // the zero fills ran on the model's stream; the caller may continue on another one
  HIP_TRY(hipStreamSynchronize(m->stream));
  return FD_OK;
}

namespace {

int prof_begin(fd_model* m, int cls, hipStream_t s, bool on) {
  if (!on) return FD_OK;
  hipEvent_t e0, e1;
  for (hipEvent_t* e : {&e0, &e1}) {
    if (!m->event_pool.empty()) {
      *e = m->event_pool.back();
      m->event_pool.pop_back();
    } else {
      HIP_TRY(hipEventCreate(e));
    }
  }
  m->pending.push_back({cls, e0, e1});
  HIP_TRY(hipEventRecord(e0, s));
  return FD_OK;
}
int prof_end(fd_model* m, hipStream_t s, bool on) {
  if (!on) return FD_OK;
  HIP_TRY(hipEventRecord(m->pending.back().e1, s));
  return FD_OK;
}

int harvest(fd_model* m) {
  for (PendingEvent& p : m->pending) {
    HIP_TRY(hipEventSynchronize(p.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.e0, p.e1));
    m->prof_ms[p.cls] += ms;
    m->prof_n[p.cls] += 1;
    m->event_pool.push_back(p.e0);
    m->event_pool.push_back(p.e1);
  }
  m->pending.clear();
  return FD_OK;
}

#define PROF(cls, stmt)                                   \
  do {                                                    \
    int rc_ = prof_begin(m, cls, s, mode.profile);        \
    if (rc_) return rc_;                                  \
    stmt;                                                 \
    rc_ = prof_end(m, s, mode.profile);                   \
    if (rc_) return rc_;                                  \
  } while (0)

// an attempted launch that did not happen has recorded an empty bracket: drop it
void prof_drop(fd_model* m, bool on) {
  if (!on) return;
  const PendingEvent p = m->pending.back();
  m->pending.pop_back();
  m->event_pool.push_back(p.e0);
  m->event_pool.push_back(p.e1);
}

// A/B overrides from the environment, read once: FDMI_FUSE_ATTN / FDMI_FUSE_FFN stand in for the options of the same name while
// those are -1 (auto); FDMI_STAMPS=1 makes the row-image kernels write cycle stamps (fd_model::stamps)
struct EnvOverrides {
  int fuse_attn, fuse_ffn;
  bool stamps;
};
const EnvOverrides& env_overrides() {
  static const EnvOverrides env = [] {
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    return EnvOverrides{num("FDMI_FUSE_ATTN", -1), num("FDMI_FUSE_FFN", -1), num("FDMI_STAMPS", 0) != 0};
  }();
  return env;
}

}  // namespace

// Which kernels make up a timestep on workspace `w` (the model's device is current).  key_mask: fd_forward_ex's arbitrary key mask.
// The weight images every layer has are asked of layer 0 (fd_finalize uploads the same set for every layer).
// dyn_rows: the row count of the launches is decided on the device (fd_ar_sample's growing prefix), as with option "varlen"; it
// changes the GEMM tails only.
StepPlan fdmi::plan_step(const fd_model* m, const Workspace& w, bool key_mask, bool dyn_rows) {
  StepPlan p;
  p.img = w.img;
  if (!p.img) {
    p.fuse_ln = m->fuse_ln > 0;  // fp32 path: the LN-fused fp32 GEMM is slower than GEMM + LayerNorm, off unless asked for
    return p;
  }
  const fd_config& c = m->cfg;
  const LayerDev& lw = m->layers[0];
  const EnvOverrides& env = env_overrides();
  const int B = w.B, L = w.L, d = c.d_model, max_rows = w.cap, ncu = cu_count();
  // the fused kernels are persistent, one workgroup per CU: do `items` of their work fill whole rounds of the CUs?  (512 on 256 CUs
  // are two full rounds, 300 would leave the second round four-fifths empty and 8 would run on 8 CUs)
  auto whole_rounds = [&](int items) {
    const int rounds = (items + ncu - 1) / ncu;
    return (double)items >= 0.94 * (double)rounds * ncu;
  };
  const bool fits_u32 = (size_t)w.cap * d * 4 < (1ull << 32) - 65536;  // (the fused kernels address the row images with 32-bit offsets)
  // q | k | v projection + attention as ONE kernel per sequence: q, k and v never reach HBM.  fuse_attn: 1 = seq_attn16.hip (16-row
  // waves, two per SIMD; any L <= 128, padded or packed rows), 2 = seq_attn.hip (round 5: 32-row waves, 96 < L <= 128), 0 = never.
  // auto: seq_attn16.hip for padded rows of 97..128 positions when the batch (one workgroup = one sequence at a time) fills whole rounds.
  // Measured (profiles/r06_seq_attn16_notes.log): packed rows of BASELINE C3's first chunk (B 512, lengths 50..101) are a tie with
  // the two-kernel path (5.29 against 5.25 ms per step), its second chunk (B 268) and batches of a few sequences lose.
  // (auto never reaches seq_attn.hip: its range and its upload condition are subsets of seq_attn16.hip's)
  const int fuse_attn = m->fuse_attn >= 0 ? m->fuse_attn : env.fuse_attn;
  const bool attn_auto = !m->varlen && L > 96 && whole_rounds(B);
  const bool fused_ok = fuse_attn != 0 && (fuse_attn > 0 || attn_auto) && !key_mask && !m->split_qkv && fits_u32;
  if (fused_ok && fuse_attn != 2 && lw.wsa16_i.p && seq_attn16_supported(d, c.n_heads, L, c.max_pos)) p.attn = StepPlan::ATTN_FUSED16;
  else if (fused_ok && fuse_attn == 2 && lw.wsa_i.p && seq_attn_supported(d, c.n_heads, L, c.max_pos)) p.attn = StepPlan::ATTN_FUSED32;
  // else q | k | v in one launch (the three column tiles of a row panel run side by side on one XCD: h is read from HBM once), or q | k + v^T
  else p.attn = lw.wqkv_i.p && !m->split_qkv ? StepPlan::ATTN_QKV : StepPlan::ATTN_QK_VT;
  // an arbitrary key mask: the general kernel (the tuned one builds its schedule on prefix masks); so do head sizes 64 / 96 / 128
  p.attn_gen = key_mask || head_dim(c) != 32;
  // BertIntermediate + BertOutput as ONE kernel (ffn16.hip): the 2 d wide intermediate never reaches HBM.  fuse_ffn 2 (and auto):
  // BertSelfOutput (attention.output.dense + residual + LayerNorm) in front of it in the same launch, its output on chip too.  Passes
  // of 128 rows: auto = the passes fill whole rounds (315 would leave the second round a quarter full where the tile GEMMs deal 6 + 1
  // column tiles per pass).  Packed rows: by the caller's row count when it gave one -- the bound B * ceil8(L) overstates ragged batches
  const int fuse_ffn = m->fuse_ffn >= 0 ? m->fuse_ffn : env.fuse_ffn;
  const int rows_known = m->varlen && m->rows_hint > 0 && m->rows_hint <= max_rows ? m->rows_hint : max_rows;
  const bool fused_ffn = fuse_ffn != 0 && (fuse_ffn > 0 || whole_rounds((rows_known + 127) / 128)) && lw.wff_i.p &&
                         ffn16_supported(d, c.d_ff) && fits_u32;
  p.ffn = !fused_ffn ? StepPlan::FFN_GEMMS : (fuse_ffn != 1 && lw.wtail_i.p && d <= 384) ? StepPlan::FFN_TAIL : StepPlan::FFN_FUSED;
  p.split_ln = d > 384;
  // do the tiles of an N-column GEMM over this workspace fill whole rounds of the launch's workgroups?  Padded rows: the row count
  // is the workspace's capacity, known here; packed rows (sampling.sample): data dependent -> the slice-capable instantiation
  auto tail_for = [&](int N) {
    if (m->varlen || dyn_rows) return 1;
    const int ntiles = (max_rows / 128) * ((N + 383) / 384);
    return ntiles % gemm_img_grid(max_rows, N) != 0 ? 1 : 0;
  };
  if (!p.fused_attn()) p.tail_qk = tail_for(p.attn == StepPlan::ATTN_QKV ? 3 * d : 2 * d);
  p.tail_d = tail_for(d);
  if (p.ffn == StepPlan::FFN_GEMMS) p.tail_ff = tail_for(c.d_ff);
  return p;
}

namespace {

// the arguments of the head + p_sample update launch that both paths share (the caller adds the head's input)
UpdateArgs fill_update(const fd_model* m, const Workspace& w, const StepMode& mode) {
  UpdateArgs u;
  memset(&u, 0, sizeof u);
  if (m->cfg.decoder == FD_DEC_MLP) {
    u.gamma = m->hd_g;
    u.beta = m->hd_b;
    u.do_ln = 1;
  }
  u.w2 = m->hd_w2;
  u.b2 = m->hd_b2;
  u.x = w.x;
  u.coef = m->coef;
  u.t_dev = w.t_dev;
  u.T = m->T;
  u.M = w.B * w.L;
  u.L = w.L;
  u.F = m->cfg.n_features;
  u.d = m->cfg.d_model;
  u.ln_eps = 1e-12f;  // AnglesPredictor(eps=1e-12)  (modelling.py:187,199)
  u.angle_mask = mode.no_wrap ? 0u : m->angle_mask;
  u.eps_out = w.eps;
  if (!mode.forward_only) {
    u.x_out = w.x;
    if (mode.use_dyn) {
      u.dyn = w.dyn;
    } else {
      u.noise = mode.noise;
      u.t_start = mode.t_start;
      u.known = mode.known; u.fixed = mode.fixed; u.known_noise = mode.z_known; u.known_coef = mode.known_coef;
      u.strided = mode.strided ? (mode.x0_only ? 2 : 1) : 0; u.sa = mode.sa; u.sb = mode.sb; u.ss = mode.ss;
      u.level_out = mode.level_out;
      u.sc = mode.sc; u.su = mode.su; u.sv = mode.sv; u.x0_prev = mode.x0_prev; u.x0_out = mode.x0_out;
    }
  }
  if (mode.use_dyn) u.noise_stride = (long long)u.M * u.F;
  return u;
}

}  // namespace

namespace fdmi {

// One reverse-diffusion step = BertForDiffusionBase.forward (modelling.py:384-484) + the
// p_sample update and wrap (sampling.py:62-75, :119-130), as a fixed kernel sequence.
int run_step(fd_model* m, hipStream_t s, const StepMode& mode) {
  const StepPlan plan = plan_step(m, m->ws, mode.kmask != nullptr);
  if (plan.img) return run_step_img(m, s, mode, plan);
  const fd_config& c = m->cfg;
  Workspace& w = m->ws;
  const int B = w.B, L = w.L, M = B * L, d = c.d_model, ff = c.d_ff, F = c.n_features;
  PROF(KC_EMBED, launch_embed(w.x, m->w_in, m->b_in, m->pos_emb, m->emb_g, m->emb_b, c.ln_eps, m->time_table, w.t_dev,
                              mode.t_seq, w.h, B, L, F, d, s));
  for (int li = 0; li < c.n_layers; ++li) {
    const LayerDev& lw = m->layers[li];
    PROF(KC_GEMM_QKV, launch_gemm_f32(EPI_BIAS, w.h, lw.wqkv, lw.bqkv, nullptr, w.qkv, M, 3 * d, d, s));
    bool ok = true;
    PROF(KC_ATTN, ok = launch_attention_f32(w.qkv, lw.demb, w.lens, w.ctx, B, L, c.n_heads, c.max_pos, s,
                                            c.pos_type == FD_POS_RELATIVE_KEY_QUERY));
    if (!ok) return fail(FD_E_UNSUPPORTED, "attention: sequence length %d not supported by the fp32 kernel (max 128)", L);
    bool fused = false;  // (the LN-fused GEMM refuses the shapes it is not built for: GEMM + LayerNorm then)
    if (plan.fuse_ln) {
      PROF(KC_GEMM_OUT, fused = launch_gemm_f32_ln(w.ctx, lw.wo, lw.bo, w.h, lw.ln1g, lw.ln1b, c.ln_eps, w.a, M, d, d, s));
      if (!fused) prof_drop(m, mode.profile);
    }
    if (!fused) {
      PROF(KC_GEMM_OUT, launch_gemm_f32(EPI_BIAS_RESID, w.ctx, lw.wo, lw.bo, w.h, w.tmp, M, d, d, s));
      PROF(KC_LN1, launch_layernorm(w.tmp, lw.ln1g, lw.ln1b, c.ln_eps, w.a, M, d, s));
    }
    PROF(KC_GEMM_UP, launch_gemm_f32(EPI_BIAS_GELU, w.a, lw.wi, lw.bi, nullptr, w.g, M, ff, d, s));
    fused = false;
    if (plan.fuse_ln) {
      PROF(KC_GEMM_DOWN, fused = launch_gemm_f32_ln(w.g, lw.wd, lw.bd, w.a, lw.ln2g, lw.ln2b, c.ln_eps, w.h, M, d, ff, s));
      if (!fused) prof_drop(m, mode.profile);
    }
    if (!fused) {
      PROF(KC_GEMM_DOWN, launch_gemm_f32(EPI_BIAS_RESID, w.g, lw.wd, lw.bd, w.a, w.tmp, M, d, ff, s));
      PROF(KC_LN2, launch_layernorm(w.tmp, lw.ln2g, lw.ln2b, c.ln_eps, w.h, M, d, s));
    }
  }
  UpdateArgs u = fill_update(m, w, mode);
  u.g = w.h;
  if (c.decoder == FD_DEC_MLP) {
    PROF(KC_GEMM_HEAD, launch_gemm_f32(EPI_BIAS_GELU, w.h, m->hd_w1, m->hd_b1, nullptr, w.g, M, d, d, s));
    u.g = w.g;
  }
  PROF(KC_HEAD_UPDATE, launch_head_update(u, s));
  if (mode.advance) PROF(KC_ADVANCE, launch_step_advance(w.t_dev, mode.use_dyn ? w.dyn : nullptr, s));
  HIP_TRY(hipGetLastError());
  return FD_OK;
}


// The same step on the row-image kernels (FD_PREC_F16X3): 6 launches per layer (QK, V^T, attention, attn-out + LN,
// FFN-up + GELU, FFN-down + LN), every activation an fp16 hi|lo image, no separate step-advance launch.
int run_step_img(fd_model* m, hipStream_t s, const StepMode& mode, const StepPlan& plan) {
  const fd_config& c = m->cfg;
  Workspace& w = m->ws;
  const int B = w.B, L = w.L, d = c.d_model, ff = c.d_ff, F = c.n_features, H = sub_heads(c);  // H: 32-column sub-heads (= heads at head size 32)
  const int max_rows = w.cap;
  // debug_stop counts in launches of the unfused sequence, so that a value means the same place under every plan: a fused launch
  // takes the slots of the launches it stands for (fused attention two, fused feed-forward two, with BertSelfOutput in front three)
  int slots = 0;
  auto stop_after = [&](int n) { return m->debug_stop > 0 && (slots += n) >= m->debug_stop; };
  auto done = [&]() -> int {
    HIP_TRY(hipGetLastError());
    return FD_OK;
  };
  {
    EmbedImgArgs e;
    memset(&e, 0, sizeof e);
    e.x = w.x; e.w_in = m->w_in; e.b_in = m->b_in; e.pos_emb = m->pos_emb; e.gamma = m->emb_g; e.beta = m->emb_b;
    e.time_table = m->time_table; e.tslot = w.t_dev; e.rowinfo = w.rowinfo; e.nrow = w.nrow; e.dims = w.dims;
    e.h = w.himg; e.L = L; e.F = F; e.d = d; e.eps = c.ln_eps; e.out_scale = m->layers[0].s_h;
    e.pos_ids = mode.pos_ids;
    PROF(KC_EMBED, launch_embed_img(e, mode.t_seq, max_rows, s, mode.ar));
    if (stop_after(1)) return done();
  }
  if (env_overrides().stamps && !m->stamps) {
    HIP_TRY(hipMalloc((void**)&m->stamps, kStampWords * 8));
    HIP_TRY(hipMemset(m->stamps, 0, kStampWords * 8));
  }
  auto stamps_at = [&](long long word) { return m->stamps ? m->stamps + word : nullptr; };
  auto base = [&]() {
    GemmImgArgs g;
    memset(&g, 0, sizeof g);
    g.stamps = m->stamps;
    g.trash = w.trash; g.rowinfo = w.rowinfo; g.dims = w.dims;
    g.qkv_bytes = (unsigned)((size_t)w.B * H * w.LTOT * 128);
    g.H = H; g.LPK = w.LPK; g.LTOT = w.LTOT; g.NKT = w.NKT;
    g.eps = c.ln_eps;
    return g;
  };
  // a d_model wide GEMM with residual + LayerNorm behind it: in its epilogue, or (a LayerNorm row does not fit one 384-column tile)
  // as fp32 rows and the LayerNorm kernel
  auto gemm_ln = [&](GemmImgArgs& g, int kc_gemm, int kc_ln) -> int {
    g.N = d;
    g.tail = plan.tail_d;
    if (!plan.split_ln) {
      PROF(kc_gemm, launch_gemm_img(EPI_IMG_LN, g, max_rows, s));
      return FD_OK;
    }
    g.out_f32 = w.tmp;
    PROF(kc_gemm, launch_gemm_img(EPI_IMG_BIAS, g, max_rows, s));
    PROF(kc_ln, launch_ln_f32_img(w.tmp, g.gamma, g.beta, c.ln_eps, w.dims, g.out, d, g.out_scale, max_rows, s));
    return FD_OK;
  };
  for (int li = 0; li < c.n_layers; ++li) {
    const LayerDev& lw = m->layers[li];
    const float s_next = li + 1 < c.n_layers ? m->layers[li + 1].s_h : m->s_hfinal;
    if (plan.fused_attn()) {
      const bool fused16 = plan.attn == StepPlan::ATTN_FUSED16;
      SeqAttnArgs a;
      memset(&a, 0, sizeof a);
      a.himg = w.himg; a.himg_bytes = (unsigned)((size_t)w.cap * d * 4);
      const SplitW& wsa = fused16 ? lw.wsa16_i : lw.wsa_i;
      a.wimg = static_cast<const unsigned char*>(wsa.p); a.bias = lw.bqkv;
      a.demb = static_cast<const u32x4_t*>(lw.demb_s.p);
      a.lens = w.lens; a.nrow = w.nrow; a.seq_row0 = w.seq_row0; a.ctx = w.cimg;
      a.B = B; a.H = H; a.maxpos = c.max_pos;
      a.acc_scale = 1.0f / (lw.s_h * wsa.scale);
      a.q_scale = lw.s_q; a.k_scale = lw.s_k; a.v_scale = lw.s_v; a.ctx_scale = lw.s_v;
      a.r_scale = lw.s_k / lw.demb_s.scale;
      a.stamps = stamps_at(kStampSeqAttn);
      bool launched = false;
      PROF(KC_SEQ_ATTN, launched = fused16 ? launch_seq_attn16(a, s, m->debug_grid, &w.grids[0]) : launch_seq_attn(a, s, m->debug_grid, &w.grids[1]));
      if (!launched)
        return fused16 ? fail(FD_E_HIP, "the fused projection + attention kernel could not be launched (%d bytes of LDS per workgroup)", 160256)
                       : fail(FD_E_HIP, "the 32-row fused projection + attention kernel could not be launched (%d bytes of LDS per workgroup)", 160 * 1024);
      if (stop_after(2)) return done();
    } else {
      if (plan.attn == StepPlan::ATTN_QKV) {
        GemmImgArgs g = base();
        g.A = w.himg; g.W = static_cast<const unsigned char*>(lw.wqkv_i.p); g.bias = lw.bqkv;
        g.qbuf = w.qbuf; g.kbuf = w.kbuf; g.vbuf = w.vbuf; g.N = 3 * d; g.K = d;
        g.acc_scale = 1.0f / (lw.s_h * lw.wqkv_i.scale); g.q_scale = lw.s_q; g.k_scale = lw.s_k; g.v_scale = lw.s_v;
        g.tail = plan.tail_qk;
        PROF(KC_GEMM_QKV, launch_gemm_img(EPI_IMG_QKV, g, max_rows, s));
        if (stop_after(1)) return done();
      } else {
        GemmImgArgs g = base();
        g.A = w.himg; g.W = static_cast<const unsigned char*>(lw.wqk_i.p); g.bias = lw.bqk;
        g.qbuf = w.qbuf; g.kbuf = w.kbuf; g.N = 2 * d; g.K = d;
        g.acc_scale = 1.0f / (lw.s_h * lw.wqk_i.scale); g.q_scale = lw.s_q; g.k_scale = lw.s_k;
        g.tail = plan.tail_qk;
        PROF(KC_GEMM_QKV, launch_gemm_img(EPI_IMG_QK, g, max_rows, s));
        if (stop_after(1)) return done();
        g = base();
        g.A = w.himg; g.W = static_cast<const unsigned char*>(lw.wv_i.p); g.bias = lw.bv;
        g.vbuf = w.vbuf; g.N = d; g.K = d;
        g.acc_scale = 1.0f / (lw.s_h * lw.wv_i.scale); g.v_scale = lw.s_v;
        g.tail = plan.tail_d;
        PROF(KC_GEMM_V, launch_gemm_img(EPI_IMG_VT, g, max_rows, s));
        if (stop_after(1)) return done();
      }
      AttnImgArgs a;
      memset(&a, 0, sizeof a);
      a.qbuf = w.qbuf; a.kbuf = w.kbuf; a.vbuf = w.vbuf;
      a.demb = static_cast<const u32x4_t*>(lw.demb_s.p);
      a.lens = w.lens; a.nrow = w.nrow; a.seq_row0 = w.seq_row0; a.ctx = w.cimg; a.trash = w.trash;
      a.B = B; a.H = H; a.LTOT = w.LTOT; a.NKT = w.NKT; a.maxpos = c.max_pos;
      a.q_scale = lw.s_q; a.k_scale = lw.s_k; a.v_scale = lw.s_v; a.ctx_scale = lw.s_v;
      a.r_scale = lw.demb_s.p ? lw.s_k / lw.demb_s.scale : 1.f;
      a.r_scale_k = lw.demb_s.p ? lw.s_q / lw.demb_s.scale : 1.f;
      a.rkq = c.pos_type == FD_POS_RELATIVE_KEY_QUERY;
      a.stamps = stamps_at(kStampAttn);
      bool ok = true;
      if (plan.attn_gen) {  // indexed by head; the images stay per sub-head
        a.H = c.n_heads;
        a.kmask = mode.kmask;
        a.L = mode.kmask ? L : 0;
        PROF(KC_ATTN, ok = launch_attention_gen(a, head_dim(c) / 32, s));
      } else {
        PROF(KC_ATTN, ok = launch_attention_img(a, L, s));
      }
      if (!ok) return fail(FD_E_UNSUPPORTED, "attention: L=%d, head size %d", L, head_dim(c));
      if (stop_after(1)) return done();
    }
    const bool fused_tail = plan.ffn == StepPlan::FFN_TAIL;
    if (!fused_tail) {
      GemmImgArgs g = base();
      g.A = w.cimg; g.W = static_cast<const unsigned char*>(lw.wo_i.p); g.bias = lw.bo; g.gamma = lw.ln1g; g.beta = lw.ln1b;
      g.resid = w.himg; g.out = w.aimg; g.K = d;
      g.acc_scale = 1.0f / (lw.s_v * lw.wo_i.scale); g.resid_inv = 1.0f / lw.s_h; g.out_scale = lw.s_a;
      if (int rc = gemm_ln(g, KC_GEMM_OUT, KC_LN1)) return rc;
      if (stop_after(1)) return done();
    }
    if (plan.ffn != StepPlan::FFN_GEMMS) {
      FfnArgs a;
      memset(&a, 0, sizeof a);
      a.aimg = w.aimg; a.a_bytes = (unsigned)((size_t)w.cap * d * 4);
      a.wimg = static_cast<const unsigned char*>(fused_tail ? lw.wtail_i.p : lw.wff_i.p);
      if (fused_tail) {
        a.cimg = w.cimg; a.hres = w.himg; a.bo = lw.bo; a.g1 = lw.ln1g; a.b1 = lw.ln1b;
        a.ao_scale = 1.0f / (lw.s_v * lw.wtail_i.scale); a.hres_inv = 1.0f / lw.s_h; a.a_scale = lw.s_a; a.eps1 = c.ln_eps;
      }
      a.bi = lw.bi; a.bd = lw.bd; a.gamma = lw.ln2g; a.beta = lw.ln2b;
      a.out = w.himg; a.out_bytes = a.a_bytes;
      a.panels = max_rows / 128; a.dims = w.dims;
      a.up_scale = 1.0f / (lw.s_a * lw.wff_i.scale); a.g_scale = lw.s_g; a.down_scale = 1.0f / (lw.s_g * lw.wff_scale_dn);
      a.resid_inv = 1.0f / lw.s_a; a.out_scale = s_next; a.eps = c.ln_eps;
      a.stamps = stamps_at(kStampFfn);
      bool launched = false;
      PROF(fused_tail ? KC_TAIL : KC_FFN, launched = launch_ffn16(a, d, s, m->debug_grid, &w.grids[2]));
      if (!launched) return fail(FD_E_HIP, "the fused feed-forward kernel could not be launched");
      if (stop_after(fused_tail ? 3 : 2)) return done();
      continue;
    }
    {
      GemmImgArgs g = base();
      g.A = w.aimg; g.W = static_cast<const unsigned char*>(lw.wi_i.p); g.bias = lw.bi; g.out = w.gimg; g.N = ff; g.K = d;
      g.acc_scale = 1.0f / (lw.s_a * lw.wi_i.scale); g.out_scale = lw.s_g;
      g.tail = plan.tail_ff;
      PROF(KC_GEMM_UP, launch_gemm_img(EPI_IMG_GELU, g, max_rows, s));
      if (stop_after(1)) return done();
    }
    {
      GemmImgArgs g = base();
      g.A = w.gimg; g.W = static_cast<const unsigned char*>(lw.wd_i.p); g.bias = lw.bd; g.gamma = lw.ln2g; g.beta = lw.ln2b;
      g.resid = w.aimg; g.out = w.himg; g.K = ff;
      g.acc_scale = 1.0f / (lw.s_g * lw.wd_i.scale); g.resid_inv = 1.0f / lw.s_a; g.out_scale = s_next;
      if (int rc = gemm_ln(g, KC_GEMM_DOWN, KC_LN2)) return rc;
      if (stop_after(1)) return done();
    }
  }
  UpdateArgs u = fill_update(m, w, mode);
  HeadImgArgs hi;
  memset(&hi, 0, sizeof hi);
  if (c.decoder == FD_DEC_MLP) {
    GemmImgArgs g = base();
    g.A = w.himg; g.W = static_cast<const unsigned char*>(m->hd_w1_i.p); g.bias = m->hd_b1; g.out = w.gimg; g.N = d; g.K = d;
    g.acc_scale = 1.0f / (m->s_hfinal * m->hd_w1_i.scale); g.out_scale = m->s_hg;
    g.tail = plan.tail_d;
    PROF(KC_GEMM_HEAD, launch_gemm_img(EPI_IMG_GELU, g, max_rows, s));
    if (stop_after(1)) return done();
    hi.g = w.gimg; hi.g_inv = 1.0f / m->s_hg;
  } else {
    hi.g = w.himg; hi.g_inv = 1.0f / m->s_hfinal;
  }
  hi.rowinfo = w.rowinfo; hi.nrow = w.nrow; hi.dims = w.dims; hi.tslot = w.t_dev; hi.flag = w.flag;
  hi.advance = mode.advance ? 1 : 0;
  PROF(KC_HEAD_UPDATE, launch_head_update_img(u, hi, max_rows, s));
  return done();
}

// token-row table of the batch (row-image path); `packed`: only the first lens[b] positions are rows
int prepare_rows(fd_model* m, hipStream_t s, int packed) {
  Workspace& w = m->ws;
  if (!w.img) return FD_OK;
  launch_build_rows(w.lens, w.B, w.L, packed, w.cap, w.seq_row0, w.nrow, w.rowinfo, w.dims, s);
  HIP_TRY(hipGetLastError());
  return FD_OK;
}

__global__ void set_int_kernel(int* p, int v) { *p = v; }
__global__ void set_dyn_kernel(UpdateDyn* p, UpdateDyn v) { *p = v; }

void send_dyn(fd_model* m, hipStream_t s, const UpdateDyn& v) { hipLaunchKernelGGL(set_dyn_kernel, dim3(1), dim3(1), 0, s, m->ws.dyn, v); }

int set_t(fd_model* m, hipStream_t s, int t) {
  hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(1), 0, s, m->ws.t_dev, t);
  HIP_TRY(hipGetLastError());
  return FD_OK;
}

int check_shape(fd_model* m, int B, int L, int t) {
  if (!m) return fail(FD_E_INVALID, "null model");
  if (!m->finalized) return fail(FD_E_STATE, "fd_finalize has not been called");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (t < 0 || t >= m->T) return fail(FD_E_INVALID, "timestep %d outside [0, %d)", t, m->T);
  if (L > m->cfg.max_pos)  // (the position table and the distance table alike)
    return fail(FD_E_INVALID, "L=%d exceeds max_position_embeddings=%d", L, m->cfg.max_pos);
  if (L > 128 && !m->img)
    return fail(FD_E_UNSUPPORTED, "L=%d: the exact-fp32 attention kernel handles L <= 128; use FD_PREC_F16X3", L);
  return FD_OK;
}

// the workspace's captured graph still holds the launch sequence the model's options ask for (an option change that leads to
// the same sequence -- another rows_hint on the same side of the automatic choice -- keeps the graph)
bool graph_current(const fd_model* m, const Workspace& w) { return w.graph && w.graph_plan == plan_step(m, w, false); }

int ensure_graph(fd_model* m) {
  Workspace& w = m->ws;
  if (graph_current(m, w)) return FD_OK;  // (a precision change goes through fd_finalize, which drops the workspace)
  if (w.graph) {
    (void)hipGraphExecDestroy(w.graph);
    w.graph = nullptr;
  }
  // one eager step first: loads code objects and sets function attributes outside capture
  int rc = set_t(m, m->stream, 0);
  if (rc) return rc;
  StepMode warm{};
  warm.forward_only = true;
  rc = run_step(m, m->stream, warm);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(m->stream));
  StepMode mode{};
  mode.use_dyn = true;
  mode.advance = true;
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
  rc = run_step(m, m->stream, mode);
  hipError_t e = hipStreamEndCapture(m->stream, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess) return fail(FD_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  e = hipGraphInstantiate(&w.graph, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) return fail(FD_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  w.graph_plan = plan_step(m, w, false);
  return FD_OK;
}

// SURVEY 5 (failure detection): the update kernel raises a device flag when the model output is not finite
// (it would silently poison every later step).  Call with the model's work complete.
int check_flag(fd_model* m) {
  Workspace& w = m->ws;
  if (!w.img || !w.flag) return FD_OK;
  int v = 0;
  HIP_TRY(hipMemcpy(&v, w.flag, 4, hipMemcpyDeviceToHost));
  if (!v) return FD_OK;
  HIP_TRY(hipMemset(w.flag, 0, 4));
  // The inf / NaN may sit where no later call writes: padding rows of the images, key / value slots behind the rows of a
  // sequence that is shorter next time (a masked key's p = 0 still meets the slot in the P V product: 0 * NaN).  Back to
  // the zeros of allocation (ensure_ws), on the error path only.
  {
    const fd_config& c = m->cfg;
    const size_t d = c.d_model, gmax = c.d_ff > c.d_model ? c.d_ff : c.d_model, cap = (size_t)w.cap;
    const size_t qkv = (size_t)w.B * sub_heads(c) * w.LTOT * 128;
    const std::pair<void*, size_t> zero[] = {{w.himg, cap * d * 4}, {w.aimg, cap * d * 4}, {w.cimg, cap * d * 4}, {w.gimg, cap * gmax * 4},
                                             {d > 384 ? (void*)w.tmp : nullptr, cap * d * 4}, {w.qbuf, qkv}, {w.kbuf, qkv}, {w.vbuf, qkv},
                                             {w.eps, (size_t)w.B * w.L * c.n_features * 4}};
    for (const auto& z : zero)
      if (z.first) HIP_TRY(hipMemsetAsync(z.first, 0, z.second, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return fail(FD_E_NONFINITE, "the model produced a non-finite value (inf/NaN in the predicted noise)");
}

}  // namespace fdmi

// ============================================================================ C ABI
extern "C" {

int fd_abi_version(void) { return FDMI_ABI_VERSION; }

const char* fd_last_error(void) { return g_err.c_str(); }

int fd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fd_create(const fd_config* cfg, int device_id, fd_model** out) {
  if (!cfg || !out) return fail(FD_E_INVALID, "null argument");
  *out = nullptr;
  const fd_config& c = *cfg;
  if (c.n_features < 1 || c.n_features > kMaxFeat) return fail(FD_E_INVALID, "n_features=%d outside [1,%d]", c.n_features, kMaxFeat);
  if (c.n_heads < 1 || c.d_model < 32 || c.d_model % c.n_heads != 0)
    return fail(FD_E_INVALID, "d_model=%d is not a multiple of n_heads=%d", c.d_model, c.n_heads);
  {
    const int hd = c.d_model / c.n_heads;
    if (hd != 32 && hd != 64 && hd != 96 && hd != 128)
      return fail(FD_E_UNSUPPORTED, "d_model=%d n_heads=%d: attention head size %d is not one of 32, 64, 96, 128", c.d_model, c.n_heads, hd);
  }
  if (c.d_model > 1024) return fail(FD_E_UNSUPPORTED, "d_model=%d > 1024", c.d_model);
  if (c.d_ff < 32 || c.d_ff % 32) return fail(FD_E_UNSUPPORTED, "d_ff=%d must be a positive multiple of 32", c.d_ff);
  if (c.n_layers < 1 || c.max_pos < 1) return fail(FD_E_INVALID, "n_layers=%d max_pos=%d", c.n_layers, c.max_pos);
  if (c.pos_type != FD_POS_ABSOLUTE && c.pos_type != FD_POS_RELATIVE_KEY && c.pos_type != FD_POS_RELATIVE_KEY_QUERY)
    return fail(FD_E_INVALID, "pos_type=%d", c.pos_type);
  if (c.decoder != FD_DEC_MLP && c.decoder != FD_DEC_LINEAR) return fail(FD_E_INVALID, "decoder=%d", c.decoder);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(FD_E_INVALID, "device %d of %d", device_id, ndev);
  HIP_TRY(hipSetDevice(device_id));
  fd_model* m = new fd_model();
  m->cfg = c;
  m->device = device_id;
  hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete m;
    return fail(FD_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  *out = m;
  return FD_OK;
}

void fd_destroy(fd_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)fd_comm_destroy(m);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  drop_workspaces(m);
  free_weights(m);
  for (PendingEvent& p : m->pending) {
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  for (hipEvent_t e : m->event_pool) (void)hipEventDestroy(e);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

int fd_set_option(fd_model* m, const char* name, int value) {
  if (!m || !name) return fail(FD_E_INVALID, "null argument");
  const std::string n = name;
  if (n == "fuse_ln") m->fuse_ln = value < 0 ? -1 : (value ? 1 : 0);
  else if (n == "use_graph") m->use_graph = value ? 1 : 0;
  else if (n == "varlen") m->varlen = value ? 1 : 0;
  else if (n == "fuse_attn") m->fuse_attn = value < 0 ? -1 : (value > 2 ? 1 : value);
  else if (n == "fuse_ffn") m->fuse_ffn = value < 0 ? -1 : (value > 2 ? 2 : value);
  else if (n == "rows_hint") m->rows_hint = value < 0 ? 0 : value;
  else if (n == "split_qkv") {
    m->split_qkv = value ? 1 : 0;
    drop_workspaces(m);  // captured graphs hold the other launch sequence
  }
  else if (n == "debug_stop") {
    if (m->debug_stop != value) drop_workspaces(m);  // a graph captured with a truncated step must not be replayed afterwards
    m->debug_stop = value;
  }
  else if (n == "debug_layer") m->debug_layer = value;
  else if (n == "debug_grid") {
    const int v = value > 0 ? value : 0;
    if (m->debug_grid != v) drop_workspaces(m);  // captured graphs hold the other grid
    m->debug_grid = v;
  }
  else return fail(FD_E_INVALID, "unknown option '%s'", name);
  return FD_OK;
}

int fd_fused_attn_supported(fd_model* m, int L) {
  if (!m) return fail(FD_E_INVALID, "null argument");
  if (!m->finalized) return fail(FD_E_STATE, "fd_finalize has not been called");
  if (m->precision != FD_PREC_F16X3 || m->layers.empty() || L < 1) return 0;
  const fd_config& c = m->cfg;
  const LayerDev& lw = m->layers[0];
  if (m->fuse_attn == 2) return lw.wsa_i.p && seq_attn_supported(c.d_model, c.n_heads, L, c.max_pos) ? 1 : 0;
  return lw.wsa16_i.p && seq_attn16_supported(c.d_model, c.n_heads, L, c.max_pos) ? 1 : 0;
}

int fd_profile_every(fd_model* m, int n) {
  if (!m || n < 0) return fail(FD_E_INVALID, "bad argument");
  m->profile_every = n;
  return FD_OK;
}

int fd_profile_reset(fd_model* m) {
  if (!m) return fail(FD_E_INVALID, "null model");
  if (int rc = harvest(m)) return rc;
  for (int i = 0; i < KC_COUNT; ++i) {
    m->prof_ms[i] = 0;
    m->prof_n[i] = 0;
  }
  return FD_OK;
}

int fd_profile_count(fd_model* m) { return m ? (int)KC_COUNT : 0; }

int fd_profile_get(fd_model* m, int i, const char** name, double* total_ms, int64_t* launches, double* flops_per_launch,
                   double* bytes_per_launch) {
  if (!m || i < 0 || i >= KC_COUNT) return fail(FD_E_INVALID, "bad argument");
  if (int rc = harvest(m)) return rc;
  if (name) *name = kClassName[i];
  if (total_ms) *total_ms = m->prof_ms[i];
  if (launches) *launches = m->prof_n[i];
  if (flops_per_launch) *flops_per_launch = m->prof_flops[i];
  if (bytes_per_launch) *bytes_per_launch = m->prof_bytes[i];
  return FD_OK;
}

int fd_synchronize(fd_model* m) {
  if (!m) return fail(FD_E_INVALID, "null model");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return FD_OK;
}

int fd_debug_read(fd_model* m, const char* name, float* out, int64_t n_floats) {
  if (!m || !name || !out) return fail(FD_E_INVALID, "null argument");
  if (std::string(name) == "scales") {  // what fd_finalize chose: needs the model, not a workspace
    if (!m->finalized || !m->img || m->layers.empty()) return fail(FD_E_STATE, "fd_debug_read(scales): no model finalized with FD_PREC_F16X3");
    if (m->debug_layer < 0 || m->debug_layer >= m->cfg.n_layers)
      return fail(FD_E_INVALID, "fd_debug_read(scales): debug_layer %d of %d layers", m->debug_layer, m->cfg.n_layers);
    const LayerDev& lw = m->layers[m->debug_layer];
    const float s_next = m->debug_layer + 1 < m->cfg.n_layers ? m->layers[m->debug_layer + 1].s_h : m->s_hfinal;
    auto of = [](const SplitW& w) { return w.p ? w.scale : 0.f; };
    const float v[] = {lw.s_h, lw.s_q, lw.s_k, lw.s_v, lw.s_a, lw.s_g, s_next, m->s_hfinal, m->s_hg,
                       of(lw.wqkv_i), of(lw.wqk_i), of(lw.wv_i), of(lw.wsa16_i), of(lw.wsa_i), of(lw.wo_i), of(lw.wtail_i),
                       of(lw.wi_i), of(lw.wd_i), of(lw.wff_i), lw.wff_i.p ? lw.wff_scale_dn : 0.f, of(lw.demb_s)};
    const long long n = sizeof v / sizeof v[0];
    if (n_floats < n) return fail(FD_E_INVALID, "fd_debug_read(scales): need %lld floats", n);
    memcpy(out, v, sizeof v);
    return FD_OK;
  }
  Workspace& w = m->ws;
  if (!w.img) return fail(FD_E_STATE, "fd_debug_read: the current workspace is not on the row-image path");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  const fd_config& c = m->cfg;
  const std::string nm = name;
  const int li = m->debug_layer < c.n_layers ? m->debug_layer : c.n_layers - 1;
  const LayerDev& lw = m->layers[li];
  const float s_next = li + 1 < c.n_layers ? m->layers[li + 1].s_h : m->s_hfinal;
  const long long BH = (long long)w.B * sub_heads(c);
  long long need = 0;
  DeviceBufs bufs;
  float* tmp = nullptr;
  auto img = [&](const unsigned char* src, int K, float scale) -> int {
    need = (long long)w.cap * K;
    if (n_floats < need) return fail(FD_E_INVALID, "fd_debug_read(%s): need %lld floats", name, need);
    HIP_TRY(bufs.alloc(need * 4, &tmp));
    launch_img_to_f32(src, tmp, w.cap, K, scale, m->stream);
    return FD_OK;
  };
  auto qkv = [&](const unsigned char* src, int rowbytes, int is_vt, float scale) -> int {
    need = BH * w.LTOT * 32;
    if (n_floats < need) return fail(FD_E_INVALID, "fd_debug_read(%s): need %lld floats", name, need);
    HIP_TRY(bufs.alloc(need * 4, &tmp));
    launch_qkv_unpack(src, tmp, BH, w.LTOT, w.LPK, rowbytes, is_vt, scale, m->stream);
    return FD_OK;
  };
  int rc;
  if (nm == "h") rc = img(w.himg, c.d_model, lw.s_h);            // input of layer debug_layer
  else if (nm == "h_out") rc = img(w.himg, c.d_model, s_next);   // output of layer debug_layer
  else if (nm == "a") rc = img(w.aimg, c.d_model, lw.s_a);
  else if (nm == "ctx") rc = img(w.cimg, c.d_model, lw.s_v);
  else if (nm == "g") rc = img(w.gimg, c.d_ff, lw.s_g);
  else if (nm == "g_head") rc = img(w.gimg, c.d_model, m->s_hg);
  else if (nm == "q") rc = qkv(w.qbuf, 128, 0, lw.s_q);
  else if (nm == "k") rc = qkv(w.kbuf, 128, 2, lw.s_k);
  else if (nm == "v") rc = qkv(w.vbuf, 0, 1, lw.s_v);
  else if (nm == "stamps") {
    need = n_floats >= 2 * kStampWords ? kStampWords : 5 * 8 * 64 * 6 + 4 * 64 * 8;  // (older scripts ask for the first two tables only)
    if (n_floats < 2 * need) return fail(FD_E_INVALID, "fd_debug_read(stamps): need %lld floats (uint64 view)", 2 * need);
    if (!m->stamps) return fail(FD_E_STATE, "no stamps were recorded (FDMI_STAMPS=1)");
    HIP_TRY(hipMemcpy(out, m->stamps, need * 8, hipMemcpyDeviceToHost));
    return FD_OK;
  } else if (nm == "grids") {
    if (n_floats < 3) return fail(FD_E_INVALID, "fd_debug_read(grids): need 3 floats");
    for (int i = 0; i < 3; ++i) out[i] = (float)w.grids[i];
    return FD_OK;
  } else if (nm == "rowinfo") {
    need = 2LL * w.cap;
    if (n_floats < need) return fail(FD_E_INVALID, "fd_debug_read(rowinfo): need %lld", need);
    std::vector<int> t(need);
    HIP_TRY(hipMemcpy(t.data(), w.rowinfo, need * 4, hipMemcpyDeviceToHost));
    for (long long i = 0; i < need; ++i) out[i] = (float)t[i];
    return FD_OK;
  } else return fail(FD_E_INVALID, "fd_debug_read: unknown buffer '%s'", name);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipMemcpy(out, tmp, need * 4, hipMemcpyDeviceToHost));
  return FD_OK;
}

int fd_check_finite(fd_model* m) {
  if (!m) return fail(FD_E_INVALID, "null model");
  HIP_TRY(hipSetDevice(m->device));
  return check_flag(m);
}

}  // extern "C"
