// The model behind the C ABI as its sources see it: api.hip (workspaces, the launch plan of a timestep, the step, the captured
// graph) and api_weights.hip (fd_set_weight, fd_finalize) define what is declared here; api_run.hip (the entries that run the
// model) and api_comm.hip (the RCCL binding) call it or use fd_model alone.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/fdmi.h"
#include "fdmi_kernels.h"

namespace fdmi {

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

// split-precision image of one weight matrix (gemm_f16x3.hip)
struct SplitW {
  void* p = nullptr;
  float scale = 1.f;
};

struct LayerDev {
  SplitW demb_s;  // distance table as an fp16 hi|lo row image (row-image attention)
  // row-image path: weight images padded to 384 rows, and the (static, power-of-two) scales of this layer's
  // activation images -- derived from norm bounds of the weights at fd_finalize, so nothing can overflow fp16
  SplitW wqk_i, wv_i, wqkv_i, wo_i, wi_i, wd_i;  // wqkv_i: q | k | v rows in one image (n_heads % 6 == 0: one launch)
  SplitW wsa_i;  // the same q | k | v weights ordered per head for the 32-row fused projection + attention kernel (seq_attn.hip), or null
  SplitW wff_i;    // intermediate.dense + output.dense as ONE stream of ring stages (ffn16.hip), or null; scale = the first dense's
  float wff_scale_dn = 1.f;  // ... the second dense's
  SplitW wtail_i;  // attention.output.dense's stages in front of that stream (ffn16.hip TAIL), or null; scale = attention.output.dense's
  SplitW wsa16_i;  // ... for the 16-row kernel (seq_attn16.hip: rows of a head permuted into its operand tiles), or null
  float *bqk = nullptr, *bv = nullptr;  // bias slices of bqkv
  float s_h = 1.f, s_q = 1.f, s_k = 1.f, s_v = 1.f, s_a = 1.f, s_g = 1.f;
  float *wqkv = nullptr, *bqkv = nullptr, *demb = nullptr;
  float *wo = nullptr, *bo = nullptr, *ln1g = nullptr, *ln1b = nullptr;
  float *wi = nullptr, *bi = nullptr, *wd = nullptr, *bd = nullptr, *ln2g = nullptr, *ln2b = nullptr;
};

enum KClass {
  KC_EMBED = 0, KC_GEMM_QKV, KC_GEMM_V, KC_ATTN, KC_GEMM_OUT, KC_LN1, KC_GEMM_UP, KC_GEMM_DOWN, KC_LN2, KC_GEMM_HEAD,
  KC_HEAD_UPDATE, KC_ADVANCE, KC_SEQ_ATTN, KC_FFN, KC_TAIL, KC_COUNT
};
const char* const kClassName[KC_COUNT] = {
    "embed_ln_time", "gemm_qkv", "gemm_v", "attention", "gemm_attn_out", "layernorm_attn", "gemm_ffn_up",
    "gemm_ffn_down", "layernorm_ffn", "gemm_head_dense1", "head_update_wrap", "step_advance", "qkv_attention_fused", "ffn_fused", "attn_out_ffn_fused"};

// The launch sequence of one timestep: every choice between kernels, made once per step (plan_step) from the model's options,
// the environment overrides and the workspace's shape.  run_step launches from it; a captured graph is current for as long as
// the plan it was captured with is the plan the options lead to (graph_current).
struct StepPlan {
  enum Attn { ATTN_QKV, ATTN_QK_VT, ATTN_FUSED16, ATTN_FUSED32 };  // q | k | v in one launch; q | k + v^T; projection + attention fused:
                                                                   // seq_attn16.hip (16-row waves) / seq_attn.hip (32-row waves)
  enum Ffn { FFN_GEMMS, FFN_FUSED, FFN_TAIL };  // two GEMMs; ffn16.hip; ffn16.hip with BertSelfOutput in front of it in the same launch
  bool img = false;       // the row-image kernels (FD_PREC_F16X3), else the fp32 ones
  bool fuse_ln = false;   // fp32 path: the LN-fused GEMMs
  int attn = ATTN_QKV;
  bool attn_gen = false;  // attention_gen.hip (arbitrary key masks, head sizes 64 / 96 / 128), else attention_img.hip
  int ffn = FFN_GEMMS;
  bool split_ln = false;  // d_model > 384: a LayerNorm row does not fit one 384-column tile -- fp32 rows, then the LayerNorm kernel
  int tail_qk = 0, tail_d = 0, tail_ff = 0;  // GemmImgArgs::tail of the GEMMs of N = 3 d (2 d when v^T is its own launch), d and d_ff
  bool fused_attn() const { return attn == ATTN_FUSED16 || attn == ATTN_FUSED32; }
  bool operator==(const StepPlan& o) const {
    return std::tie(img, fuse_ln, attn, attn_gen, ffn, split_ln, tail_qk, tail_d, tail_ff) ==
           std::tie(o.img, o.fuse_ln, o.attn, o.attn_gen, o.ffn, o.split_ln, o.tail_qk, o.tail_d, o.tail_ff);
  }
};

struct Workspace {
  int B = 0, L = 0;
  float *x = nullptr, *eps = nullptr, *h = nullptr, *qkv = nullptr, *ctx = nullptr, *a = nullptr, *tmp = nullptr,
        *g = nullptr, *z = nullptr;
  int* lens = nullptr;
  int* t_dev = nullptr;  // [0] step index; the row-image kernels also use [1] (see rowwise_img.hip)
  int* t_seq = nullptr;  // [B] one timestep per sequence (fd_forward_t, fd_denoise_loss)
  float* loss_in = nullptr;     // fd_denoise_loss's one upload: x0 | noise ([B][L][F] each) | keep | spread | t | lens ([B] each); allocated on first use
  double* loss_sums = nullptr;  // [B][F], with it
  float* loss_ex_in = nullptr;  // fd_denoise_loss_ex's one upload: x0 | noise | corrupted ([B][L][F] each) | keep | spread | coef | t | lens ([B] each)
  double* loss_ex_out = nullptr;  // its one download, in 8-byte words: sums | turns ([B][F] each) | pair_sums | pairs ([B] each)
  UpdateDyn* dyn = nullptr;
  // motif-conditioned sampling (fd_sample_inpaint, fd_p_sample_step_inpaint), allocated on first use:
  // known | z_known ([B][L][F] floats each) | known_coef ([2][T+1] floats) | fixed ([B][L][F] bytes)
  float* inpaint = nullptr;
  // row-image path (fdmi_kernels.h): images, per-(sequence, head) q / k / v^T, the token-row table
  bool img = false;
  int cap = 0, LPK = 0, LTOT = 0, NKT = 0;  // rows128 capacity = ceil128(B * ceil8(L)); key-tile geometry
  unsigned char *himg = nullptr, *aimg = nullptr, *cimg = nullptr, *gimg = nullptr, *qbuf = nullptr, *kbuf = nullptr,
                *vbuf = nullptr, *trash = nullptr;
  int2* rowinfo = nullptr;
  int *seq_row0 = nullptr, *nrow = nullptr, *dims = nullptr, *flag = nullptr;
  unsigned char* kmask = nullptr;  // [B][L] explicit key mask of fd_forward_ex (allocated on first use)
  int* pos_ids = nullptr;          // [B][L] explicit position ids of fd_forward_ex (allocated on first use)
  int grids[3] = {0, 0, 0};  // x-grid of the latest launch of seq_attn16 | seq_attn | ffn16 on this workspace (fd_debug_read "grids")
  hipGraphExec_t graph = nullptr;
  StepPlan graph_plan;  // the launch sequence `graph` was captured with
  uint64_t last_use = 0;
  void release() {
    if (graph) (void)hipGraphExecDestroy(graph);
    graph = nullptr;
    for (void* p : {(void*)x, (void*)eps, (void*)h, (void*)qkv, (void*)ctx, (void*)a, (void*)tmp, (void*)g, (void*)z,
                    (void*)lens, (void*)t_dev, (void*)t_seq, (void*)loss_in, (void*)loss_sums, (void*)loss_ex_in, (void*)loss_ex_out, (void*)dyn, (void*)inpaint, (void*)himg, (void*)aimg, (void*)cimg, (void*)gimg,
                    (void*)qbuf, (void*)kbuf, (void*)vbuf, (void*)trash, (void*)rowinfo, (void*)seq_row0, (void*)nrow,
                    (void*)dims, (void*)flag, (void*)kmask, (void*)pos_ids})
      if (p) (void)hipFree(p);
    *this = Workspace();
  }
};

struct PendingEvent {
  int cls;
  hipEvent_t e0, e1;
};

}  // namespace fdmi

struct fd_model {
  fd_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;
  std::map<std::string, fdmi::HostTensor> host;
  bool finalized = false;
  int T = 0;
  int precision = 0;
  unsigned angle_mask = 0;
  // device weights
  std::vector<void*> allocs;
  float *w_in = nullptr, *b_in = nullptr, *pos_emb = nullptr, *emb_g = nullptr, *emb_b = nullptr;
  std::vector<fdmi::LayerDev> layers;
  float *hd_w1 = nullptr, *hd_b1 = nullptr, *hd_g = nullptr, *hd_b = nullptr, *hd_w2 = nullptr, *hd_b2 = nullptr;
  fdmi::SplitW hd_w1_i;
  float s_hfinal = 1.f, s_hg = 1.f;  // row-image scales: last hidden state, head activation
  bool img = false;                  // FD_PREC_F16X3 runs on the row-image kernels
  float *coef = nullptr, *time_table = nullptr;
  // options
  int fuse_ln = -1;  // -1 auto: LN-fused GEMMs with fp16x3 (measured 9.37 vs 10.15 ms/step), not with fp32 (slower there)
  int use_graph = 1;
  unsigned long long* stamps = nullptr;  // debug cycle stamps (FDMI_STAMPS=1): gemm [5][8][64][6], attention [4][64][8], fused attention [4][64][16]
  int debug_stop = 0;  // row-image path: stop a step after this many launches (debug dumps; 0 = off)
  int debug_layer = 0; // layer whose scales fd_debug_read uses
  int debug_grid = 0;  // > 0: at most this many workgroups for the persistent fused kernels (tests of their item-to-item code; 0 = off)
  int split_qkv = 0; // row-image path: 1 = q | k and v^T as two launches even when one would do (A/B, tests)
  int varlen = 0;    // row-image path: only the first lens[b] positions of a sequence are token rows
  int fuse_attn = -1;  // row-image path: q | k | v projection + attention as ONE kernel per sequence: -1 auto (seq_attn16.hip for padded rows
                     // of 97 .. 128 positions in whole rounds of the CUs), 0 never, 1 seq_attn16.hip wherever it applies (any L <= 128, packed
                     // rows too), 2 seq_attn.hip (32-row waves) wherever it applies (97 .. 128 positions)
  int fuse_ffn = -1;   // row-image path: BertIntermediate + BertOutput as ONE kernel (ffn16.hip): -1 auto (whole rounds of 128-row passes: 2),
                     // 0 never, 1 wherever the kernel applies, 2 with BertSelfOutput in front of it in the same launch
  int rows_hint = 0;   // packed rows: the caller's exact count of token rows of the next calls (sum of the lengths rounded up to 8), or 0 = unknown;
                     // the auto choices of the fused kernels then go by it instead of the bound B * ceil8(L) (the count itself lives in device memory)
  // workspaces (buffers + captured graph) are kept per (B, L): sample_length()-driven sampling and ragged chunks
  // alternate between a few shapes
  std::vector<fdmi::Workspace> cache;
  uint64_t use_clock = 0;
  fdmi::Workspace ws;      // the current one (moved in and out of `cache`)
  void* comm = nullptr;  // ncclComm_t (fd_comm_init)
  int comm_world = 0, comm_rank = 0;
  fdmi::UpdateDyn dyn_host{};  // per-run values of the sampling loop in progress (fd_sample_begin_dev .. fd_sample_end_dev)
  int run_t = -1;        // next timestep of that run (-1: none left); a strided run: its number of visits left, minus one
  int run_n = 0;         // steps (visits) the run was begun with: the profiling ordinal counts from it
  bool run_open = false; // between fd_sample_begin_dev and fd_sample_end_dev, with no other call on the model in between
  int run_B = 0, run_L = 0;  // its shape: fd_sample_steps_dev / _end_dev refuse to run on another workspace
  // profiling
  int profile_every = 0;
  double prof_ms[fdmi::KC_COUNT] = {0};
  int64_t prof_n[fdmi::KC_COUNT] = {0};
  double prof_flops[fdmi::KC_COUNT] = {0}, prof_bytes[fdmi::KC_COUNT] = {0};
  std::vector<fdmi::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
};

namespace fdmi {

struct StepMode {
  bool forward_only;   // write eps only (fd_forward)
  bool use_dyn;        // read per-call values from ws.dyn (sampling loop)
  bool advance;        // decrement *t_dev at the end
  bool profile;        // bracket every kernel with events
  // by-value per-call values when !use_dyn (fd_p_sample_step)
  const float* noise = nullptr;
  int t_start = 0;
  bool no_wrap = false;  // p_sample alone, without the loop's wrap
  const unsigned char* kmask = nullptr;  // fd_forward_ex: [B][L] key mask of any pattern (device), else null: prefix masks from lens
  const int* pos_ids = nullptr;          // fd_forward_ex: [B][L] position ids of the absolute position embedding (device)
  // fd_p_sample_step_inpaint: the replacement's arrays (device; z_known = the one slab of level t), null otherwise
  const float *known = nullptr, *known_coef = nullptr, *z_known = nullptr;
  const unsigned char* fixed = nullptr;
  // fd_p_sample_step_coef: one strided update x' = sa x + sb eps (+ ss z where ss != 0, z = `noise`) in place of p_sample's
  bool strided = false;
  float sa = 0.f, sb = 0.f, ss = 0.f;
  int level_out = 0;  // fd_p_sample_step_coef_inpaint: the level the update lands on (z_known = the one slab of that level)
  // fd_p_sample_step_solver: one update of the second-order solver (solver_update.h) with (sa, sb, sc, su, sv); x0_out non-null
  // selects it (device; x0_prev is read only where sc != 0)
  float sc = 0.f, su = 0.f, sv = 0.f;
  const float* x0_prev = nullptr;
  float* x0_out = nullptr;
  // fd_p_sample_step_coef_x0: the strided update (sa, sb, ss) of fd_p_sample_step_coef, which also writes the visit's prediction
  // of the clean state su x + sv eps, wrapped where angular, to x0_out (not the solver's update)
  bool x0_only = false;
  const int* t_seq = nullptr;            // fd_forward_t / fd_denoise_loss: [B] one timestep per sequence (device), forward only; null: *t_dev
  bool ar = false;  // fd_ar_forward / fd_ar_sample (row-image path, with t_seq = the target lengths): the autoregressive baseline's embedding
};

// The q | k | v projections are stored per 32-column SUB-HEAD (d_model / 32 of them; a head of size 32 nb is nb consecutive
// sub-heads): head size 32 (every released configuration) runs attention_img.hip, 64 / 96 / 128 the general attention_gen.hip.
inline int head_dim(const fd_config& c) { return c.d_model / c.n_heads; }
inline int sub_heads(const fd_config& c) { return c.d_model / 32; }

// ---- defined in api_weights.hip
void free_weights(fd_model* m);  // frees the device weights; the model is no longer finalized

// ---- defined in api.hip
void drop_workspaces(fd_model* m);  // frees every workspace (and with it every captured graph)
int check_shape(fd_model* m, int B, int L, int t);  // the model is finalized and takes this shape and timestep
// makes the (B, L) workspace current (m->ws), allocating it on first use; ends a sampling run begun earlier
int ensure_ws(fd_model* m, int B, int L);
int prepare_rows(fd_model* m, hipStream_t s, int packed);
int set_t(fd_model* m, hipStream_t s, int t);                   // the step index on the device, stream-ordered
void send_dyn(fd_model* m, hipStream_t s, const UpdateDyn& v);  // the per-run values of the update kernels, stream-ordered
StepPlan plan_step(const fd_model* m, const Workspace& w, bool key_mask, bool dyn_rows = false);
int run_step(fd_model* m, hipStream_t s, const StepMode& mode);
int run_step_img(fd_model* m, hipStream_t s, const StepMode& mode, const StepPlan& plan);
int ensure_graph(fd_model* m);
bool graph_current(const fd_model* m, const Workspace& w);
int check_flag(fd_model* m);

}  // namespace fdmi
