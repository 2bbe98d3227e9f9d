/*
 * fdmi.h -- C ABI of libfdmi.so, the MI355X (gfx950) reverse-diffusion sampler
 * for foldingdiff's BertForDiffusion backbone-angle model.
 *
 * The reference (microsoft/foldingdiff) is 100% Python and has NO FFI / plugin
 * interface of its own; its boundary for this path is the Python API
 *     modelling.BertForDiffusionBase.from_dir / .forward   (foldingdiff/modelling.py:297-484)
 *     sampling.p_sample / p_sample_loop / sample           (foldingdiff/sampling.py:27-224)
 * Each entry point below names the reference function it replaces.  The Python
 * package `foldingdiff_amd` binds these with ctypes and re-exposes the
 * reference's names and signatures.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in signatures (streams and device
 *    buffers cross as void*).
 *  - every function returns FD_OK (0) or a negative FD_E_* code; the message is
 *    available from fd_last_error() (thread local).  Nothing throws across the ABI.
 *  - "host" pointers are ordinary host memory, copied synchronously.  "dev"
 *    pointers are device memory on the model's device (hipMalloc / torch CUDA
 *    tensors), used in place on the given stream.
 *  - one fd_model per device; calls on one model are serialised by the caller.
 *  - all tensors are contiguous row-major float32 unless stated otherwise:
 *    angles x[B][L][F], lengths int32[B], history [T][B][L][F].
 */
#ifndef FDMI_H
#define FDMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: fd_sample_steps_dev / fd_sample_end_dev return FD_E_STATE when another call has taken the run's workspace; history
 *    padding of packed rows is zeroed; head sizes other than 32 (multiples of 32) are accepted */
/* 3: fd_shift_trim_dev, fd_test_wrap, option "fuse_attn" (round 5) */
/* 4: fd_fused_attn_supported; option "fuse_attn" takes 2 (the round-5 kernel) and its default kernel no longer promises the bits of
 *    the two-kernel path; option "fuse_ffn" (round 6) */
/* 5: fd_internal_coords, fd_superpose_rmsd (coordinates -> internal coordinates, superposed RMSD) */
/* 6: fd_tm_score (TM-score of residue-paired CA traces) */
/* 7: fd_annotate_sse (P-SEA secondary structure of CA traces)
 *    fd_tm_align (alignment search of CA traces) came later and is additive: no existing entry changed, so the version
 *    stays 7; a library without it fails the binding's symbol lookup by name */
/*    fd_forward_t (one timestep per sequence), fd_loss_terms and fd_denoise_loss (the denoising loss of a fixed checkpoint)
 *    are additive in the same way: no existing entry or struct changed, the version stays 7 */
/*    fd_backbone_clashes and fd_lddt (integer pair counts over the atoms of a structure) are additive too */
/*    fd_ar_forward and fd_ar_sample (the autoregressive baseline) are additive too */
/*    fd_loss_terms_ex, fd_pairwise_dist and fd_denoise_loss_ex (the "l1" loss, the circle penalty and the pairwise-distance
 *    term of the denoising loss) are additive too */
/*    fd_sample_inpaint and fd_p_sample_step_inpaint (motif-conditioned sampling) are additive too */
/*    fd_sample_inpaint_resample and fd_inpaint_jump (resampling schedules of motif-conditioned sampling) are additive too */
/*    fd_sample_strided, fd_sample_strided_dev and fd_p_sample_step_coef (few-step sampling on a strided schedule) are additive
 *    too: no existing entry or public struct changed, and the tests of the earlier additions pin the value 7 */
/*    fd_sample_solver, fd_sample_solver_dev and fd_p_sample_step_solver (the second-order multistep solver) are additive too */
/*    fd_tm_align_ex (the alignment search from a chosen set of TM-align's five starts) is additive too */
/*    fd_sample_steered, fd_p_sample_step_coef_x0, fd_steer_rewards and fd_steer_resample (steering a few-step run by particle
 *    resampling on device rewards) and the struct fd_steer_params are additive too */
/*    fd_sample_repeat and fd_tie_repeats (few-step sampling with the angle rows tied across repeat units) are additive too */
/*    fd_backbone_oxygens and fd_dssp (backbone oxygens and DSSP hydrogen-bond states) are additive too */
/*    fd_nerf_vjp, fd_restraint_energy, fd_guide_step and fd_sample_guided (the derivative of NeRF and restraint-guided few-step
 *    sampling) and the struct fd_guide_params are additive too */
/*    fd_nerf_scan, fd_relax_energy and fd_relax (relaxing backbones in torsion space) and the struct fd_relax_params are additive
 *    too */
/*    fd_nerf_vjp_feats (the derivative of NeRF with the signs of the features the forward read) is additive too */
/*    fd_symmetry_energy, fd_symmetry_dock, fd_scaffold_guide_step_sym and fd_sample_guided_inpaint_sym (cyclic oligomers: a chain
 *    scored against its own symmetry copies) and the struct fd_symmetry_params are additive too */
#define FDMI_ABI_VERSION 7

enum {
  FD_OK = 0,
  FD_E_INVALID = -1,     /* bad argument / unsupported shape            */
  FD_E_STATE = -2,       /* call order (e.g. sample before finalize)    */
  FD_E_MISSING = -3,     /* a required weight was never set             */
  FD_E_HIP = -4,         /* HIP runtime error (message has hipGetErrorString) */
  FD_E_UNSUPPORTED = -5, /* valid in the reference, not implemented here */
  FD_E_NONFINITE = -6    /* the model produced inf / NaN (e.g. corrupt weights); results are not usable */
};

/* config.position_embedding_type (config.json; modelling.py:138-149, HF BertSelfAttention) */
enum { FD_POS_ABSOLUTE = 0, FD_POS_RELATIVE_KEY = 1, FD_POS_RELATIVE_KEY_QUERY = 2 };
/* training_args.json "decoder" (modelling.py:274-279) */
enum { FD_DEC_MLP = 0, FD_DEC_LINEAR = 1 };
/* arithmetic of the contraction kernels */
enum {
  FD_PREC_F32 = 0,  /* v_mfma_f32_32x32x2_f32: exact fp32 products + fp32 accumulate */
  FD_PREC_F16X3 = 1 /* GEMM operands split into fp16 hi + lo (22 significant bits), three
                       v_mfma_f32_32x32x16_f16 per product, fp32 accumulate: fp32-class error at
                       5.3x the fp32-MFMA rate (GEMMs and the attention contractions).  Softmax,
                       LayerNorm, GELU, residuals and all accumulation stay fp32. */
};

typedef struct fd_model fd_model;

/* Shapes of BertConfig + training_args.json that the hot path reads
 * (bin/train.py:425-435; modelling.py:239-295). */
typedef struct fd_config {
  int32_t n_features; /* F  = len(ft_is_angular)  (modelling.py:255-256) */
  int32_t d_model;    /* config.hidden_size */
  int32_t n_heads;    /* config.num_attention_heads; head size d_model / n_heads: 32 (tuned kernels), 64, 96 or 128 */
  int32_t d_ff;       /* config.intermediate_size */
  int32_t n_layers;   /* config.num_hidden_layers */
  int32_t max_pos;    /* config.max_position_embeddings */
  int32_t pos_type;   /* FD_POS_* */
  int32_t decoder;    /* FD_DEC_* */
  float ln_eps;       /* config.layer_norm_eps (embeddings + encoder LayerNorms);
                         the decoder head LayerNorm always uses 1e-12 (modelling.py:187) */
} fd_config;

/* ---- construction: replaces BertForDiffusionBase.__init__/from_dir (modelling.py:239-382) ---- */

int fd_abi_version(void);

/* Number of visible HIP devices (0 if none / no driver). */
int fd_device_count(void);

/* Create an empty model on HIP device `device_id`. */
int fd_create(const fd_config* cfg, int device_id, fd_model** out);

/* Provide one tensor of the reference state_dict, by its HuggingFace /
 * modelling.py name (e.g. "encoder.layer.3.attention.self.query.weight",
 * "token_decoder.dense2.bias"; full list in DESIGN.md).  Replaces
 * load_state_dict (modelling.py:362-363).  Shape is checked against cfg.
 * Non-parameter buffers ("time_embed.W", "embeddings.position_ids") are accepted
 * and ignored: the time embedding reaches the device as a table (fd_finalize). */
int fd_set_weight(fd_model* m, const char* name, const float* host_data, const int64_t* shape, int ndim);

/* Pack weights, upload the schedule + time-embedding tables, build kernels' state.
 *   T           number of diffusion timesteps (NoisedAnglesDataset.timesteps)
 *   coef        float[4][T] rows: sqrt(1/alpha_t), beta_t, sqrt(1-alphabar_t),
 *               sqrt(posterior_variance_t)  -- from compute_alphas
 *               (beta_schedules.py:45-62) as used by p_sample (sampling.py:41-72)
 *   time_table  float[T][d_model]: time_embed(t) for t = 0..T-1, computed on the
 *               host with the reference's fp32 op order (modelling.py:59-71)
 *   is_angle    uint8[F]: which features are wrapped to [-pi, pi) each step
 *               (sampling.py:119-130)
 *   precision   FD_PREC_*
 * May be called again to change T / tables. */
int fd_finalize(fd_model* m, int T, const float* coef, const float* time_table, const uint8_t* is_angle,
                int precision);

void fd_destroy(fd_model* m);

/* Runtime switches:
 *   "fuse_ln"    FD_PREC_F32 only (FD_PREC_F16X3 always fuses): 1: residual + LayerNorm run in the epilogue of
 *                the attention-output and FFN-down GEMMs (shapes without a fused instantiation fall back);
 *                0 / -1 (default): separate LayerNorm kernel (same arithmetic, faster in that mode on MI355X).
 *   "use_graph"  1 (default): the per-step kernel sequence is replayed from a hipGraph;
 *                0: eager launches.
 *   "varlen"     fd_sample / fd_sample_dev with FD_PREC_F16X3: 1 = positions >= lens[b] are not computed at all
 *                (the reference computes them and sampling.sample cuts them away, sampling.py:56-58, :201-203);
 *                positions < lens[b] are bit-identical either way.  Padded positions of the final `out` then keep x_init;
 *                padded positions of history rows are zero.
 *                0 (default): every position evolves as in the reference's p_sample_loop.
 *   "fuse_attn"  FD_PREC_F16X3, relative_key, head size 32, d_model 384 / 192, L <= 128: BertSelfAttention of a sequence (q | k | v
 *                projection + attention, modelling.py:473-480 -> HF BertSelfAttention.forward) as ONE kernel, q / k / v never
 *                reach HBM.  -1 (default): when the batch fills whole rounds of the device's CUs; 1: whenever the shape allows
 *                (fd_fused_attn_supported); 0: never (the q|k|v GEMM + attention kernels); 2: the round-5 kernel (32-row waves,
 *                96 < L <= 128; kept for A/B measurements).  Every choice meets the same tolerance against the reference
 *                (1e-5 on the forward, 1e-3 rad on a step); 0 and 2 give the same bits as each other, 1 does not (it sums in
 *                another order).
 *   "fuse_ffn"   FD_PREC_F16X3, d_model 384 / 192 with intermediate size 2 d_model: the tail of a BertLayer (modelling.py:473-480 -> HF
 *                BertLayer.forward behind the attention) as ONE kernel over passes of 128 token rows.  2: BertSelfOutput (dense +
 *                residual + LayerNorm), BertIntermediate (dense + GELU) and BertOutput (dense + residual + LayerNorm); neither the
 *                attention block's output nor the intermediate reaches HBM.  1: the feed-forward pair only.  0: never (three GEMM
 *                launches).  -1 (default): 2 when the passes fill whole rounds of the device's CUs.  Every choice meets the same
 *                tolerance against the reference; 1 and 2 sum in another order than 0 (not the same bits).
 *   "rows_hint"  with "varlen" 1: the exact number of token rows of the next sampling calls (sum over the batch of the lengths rounded up
 *                to 8; the library itself only has the lengths in device memory and the bound B * ceil8(L)), 0 (default) = unknown.
 *                It only steers the automatic kernel choices ("fuse_ffn" -1); results are within the same tolerances either way.
 *   "split_qkv"  FD_PREC_F16X3: 1 = project q | k and v^T in two launches even when n_heads % 6 == 0 would allow one
 *                (A/B measurements, tests); 0 (default).
 *   "debug_stop" n > 0: a step returns after its first n launches (FD_PREC_F16X3; stage-by-stage comparison with
 *                fd_debug_read, scripts/debug_img.py); "debug_layer": which encoder layer fd_debug_read sees.
 *   "debug_grid" n > 0: the persistent fused kernels (fused projection + attention, both forms; fused feed-forward / layer tail) run
 *                on at most n workgroups, so that a batch of a few sequences already gives every workgroup several items (tests of
 *                their item-to-item code; the automatic kernel choices do not look at it); <= 0 (default): one per compute unit.
 *                A change drops the workspaces and their captured graphs.  Same bits at every value. */
int fd_set_option(fd_model* m, const char* name, int value);

/* 1 if option "fuse_attn" = 1 (or 2, when that is the current value) runs the fused projection + attention kernel for batches of
 * padded length L on this (finalized) model, 0 if the q|k|v GEMM + attention kernels run instead; negative: FD_E_*.  No reference
 * counterpart (HF BertSelfAttention.forward is one code path); tests use it to know which kernels a gate exercised. */
int fd_fused_attn_supported(fd_model* m, int L);

/* ---- parity hooks ---- */

/* eps = model(x, t, attention_mask(lens)) -- BertForDiffusionBase.forward in eval
 * mode (modelling.py:384-484).  Host buffers.  t is constant over the batch, as
 * p_sample asserts (sampling.py:46-47).
 * Size limit of one call (every entry point that takes B and L): in the default precision the q / k / v images of the batch
 * are addressed with 32-bit offsets, so B * n_heads * ceil(L / 32) * 4096 bytes must stay below 4 GiB (B < 21,845 sequences of
 * L = 128 at 12 heads) -- FD_E_UNSUPPORTED beyond; sampling.sample chunks by batch_size long before that. */
int fd_forward(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float* eps_out);

/* fd_forward with one timestep per sequence, t = int32[B] (host), every t[b] in [0, T): what the reference's forward takes from
 * a training or validation batch (modelling.py:384-484 with batch["t"], :553-566).  A row of sequence b adds time_embed(t[b])
 * behind the embedding LayerNorm (modelling.py:472), the only place the timestep enters; every later launch is the one
 * fd_forward makes for the same (B, L).  With all t[b] equal the result has fd_forward's bits.  Both precisions. */
int fd_forward_t(fd_model* m, const float* x, const int32_t* t, const int32_t* lens, int B, int L, float* eps_out);

/* ---- the autoregressive baseline: BertForAutoregressiveBase.forward / .sample (modelling.py:807-893).  The same network and the
 * same weights; the time embedding is reused as an embedding of the sequence's target LENGTH: the row seq_lengths[b] of the table
 * fd_finalize was given (0 <= seq_lengths[b] < T; the coefficient rows are not read) is added to the input Linear's output BEFORE
 * the position embedding and the embeddings LayerNorm, and nothing is added behind it.  FD_PREC_F16X3 only (FD_E_UNSUPPORTED on an
 * FD_PREC_F32 model).  Host buffers; every argument is checked before the first device call.
 *
 * fd_ar_forward: out[B][L][F] = forward(x, prefix mask of key_lens, seq_lengths), 1 <= key_lens[b] <= L unmasked keys per
 * sequence; the other keys get the additive -10000 and every one of the L positions is computed as a query, like fd_forward_t. */
int fd_ar_forward(fd_model* m, const float* x, const int32_t* seq_lengths, const int32_t* key_lens, int B, int L, float* out);

/* fd_ar_sample: the rollout.  ret = seed[B][L][F]; for i = num_seed .. max(seq_lengths) - 1: the keys 0 .. i-1 of every sequence
 * are unmasked and ret[:, i] = forward(ret, that mask, seq_lengths)[:, i].  out[B][L][F] = the final ret: positions < num_seed
 * come back bit for bit, positions >= max(seq_lengths) keep the seed, and the caller trims sequence b to seq_lengths[b].  Row i
 * enters step i with whatever the seed holds there; nothing is wrapped.  Needs 1 <= num_seed (without a seed the first row would
 * see masked keys only: FD_E_INVALID) and max(seq_lengths) <= L.  Step i runs over the rows 0 .. i only -- later rows are masked
 * keys and unread queries -- so the loop costs half the reference's; one upload, one download, no host synchronisation between. */
int fd_ar_sample(fd_model* m, const float* seed, const int32_t* seq_lengths, int B, int L, int num_seed, float* out);

/* The same forward with what the reference's forward also honours (modelling.py:434-452, :464-467) and the sampler never produces:
 *   key_mask      uint8[B][L], 1 = attend, 0 = masked key, ANY pattern (NULL: every key is attended to); masked keys get the
 *                 additive -10000 of HF's extended attention mask, and every position is computed as a query
 *   position_ids  int32[B][L] rows of the absolute position embedding (NULL: 0 .. L-1); ignored for the relative position
 *                 types, as in the reference (no position embedding is added there and the distance uses arange)
 * FD_PREC_F16X3 only.  Arbitrary masks run on the general attention kernel (attention_gen.hip), not the tuned one. */
int fd_forward_ex(fd_model* m, const float* x, int t, const uint8_t* key_mask, const int32_t* position_ids, int B, int L,
                  float* eps_out);

/* One reverse step: x_out = p_sample(x, t) (sampling.py:27-75); with wrap != 0 the
 * loop's per-feature wrap to [-pi, pi) (sampling.py:119-130) is applied as well, i.e.
 * the result is one iteration of p_sample_loop.  z is the N(0,1) draw the reference
 * takes from torch.randn_like (required for t > 0, ignored at t == 0).  Host buffers. */
int fd_p_sample_step(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, const float* z,
                     int wrap, float* x_out);

/* ---- the sampler: replaces p_sample_loop (sampling.py:78-132) ----
 *   x_init   [B][L][F] start point (already wrapped noise, datasets.py:772-799)
 *   lens     int32[B], 1 <= lens[i] <= L; positions >= lens[i] are masked keys
 *   t_start  first timestep index to run (T-1 for a full run); the loop runs
 *            t = t_start, t_start-1, ..., 0  (t_start+1 steps)
 *   noise    [t_start+1][B][L][F] per-step N(0,1) draws, row i used at t = i
 *            (row 0 unused), or NULL => on-device Philox4x32-10 keyed by
 *            (seed, t, element) -- deterministic, but NOT torch's stream
 *   out      full_history == 0: [B][L][F], the final sample only;
 *            full_history == 1: [t_start+1][B][L][F] (row j = state after step t = t_start - j,
 *            i.e. the reference's stacked `imgs`);
 *            full_history == k > 1: [ceil((t_start+1)/k)][B][L][F] -- every k-th state (j = k-1,
 *            2k-1, ...) and the final one in the last row (strided history)
 * The per-step loop is a captured hipGraph replayed t_start+1 times; the step
 * index lives on the device. */
int fd_sample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
              uint64_t seed, float* out, int full_history);

/* fd_sample for a slice of a larger batch: `seq_offset` is the global index of sequence 0, added to the sequence
 * index in the Philox key (multi-GPU sharding of sampling.sample: every rank draws the noise of the unsharded batch). */
int fd_sample_ex(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
                 uint64_t seed, int64_t seq_offset, float* out, int full_history);

/* Same, with every buffer already resident in device memory, asynchronous on
 * `hip_stream` (a hipStream_t, NULL = the model's own stream).  The caller
 * synchronises.  `seq_offset` is added to the sequence index in the Philox key
 * so a batch sharded over several GPUs draws the noise of the unsharded batch. */
int fd_sample_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, int t_start,
                  const void* noise_dev, uint64_t seed, int64_t seq_offset, void* out_dev, int full_history,
                  void* hip_stream);

/* The same loop in pieces, for callers that stream the per-step noise instead of materialising [T][B][L][F]
 * (sampling.py draws the reference's torch.randn_like sequence chunk by chunk on a host thread and uploads it on a copy
 * stream while the previous chunk is consumed):
 *   fd_sample_begin_dev   everything fd_sample_dev does before its first step (uploads x_init / lens into the workspace,
 *                         row table, graph); `out_dev` receives the history rows as in fd_sample_dev
 *   fd_sample_steps_dev   the next n_steps reverse steps, enqueued on the stream; noise_dev = [rows][B][L][F] device
 *                         buffer whose row i is the draw of step t = noise_t0 + i (it must cover every step of the call,
 *                         t = 0 included -- that row is read and multiplied by sigma_0 = 0), or NULL (Philox)
 *   fd_sample_end_dev     after the last step: copies the final state to out_dev when full_history == 0
 * fd_sample_dev(...) == begin; steps(t_start + 1, noise, 0); end.  Stream-ordered like fd_sample_dev. */
int fd_sample_begin_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, int t_start,
                        uint64_t seed, int64_t seq_offset, void* out_dev, int full_history, void* hip_stream);
int fd_sample_steps_dev(fd_model* m, int n_steps, const void* noise_dev, int noise_t0, void* hip_stream);
int fd_sample_end_dev(fd_model* m, void* out_dev, void* hip_stream);

/* ---- motif-conditioned sampling ("replacement"): chosen elements of the state are held to known values while the rest
 * of the chain is generated around them.
 *
 * Levels.  A state at level j = 0 .. T has seen j forward-noising steps.  The state that ENTERS reverse step t is at level
 * t + 1, the state that step t LEAVES is at level t.  keep[0] = 1, spread[0] = 0; keep[j] = sqrt_alphas_cumprod[j-1] and
 * spread[j] = sqrt_one_minus_alphas_cumprod[j-1] for j >= 1, in float32 (what NoisedAnglesDataset noises with).
 *
 * Replacement.  An element o = (b, l, f) with fixed[o] != 0 of a state at level j is
 *   j >= 1:  keep[j] * known[o] + spread[j] * z, each product and the sum rounded once (fd_denoise_loss's noising
 *            statement), wrapped to [-pi, pi) where the model's feature f is an angle
 *   j == 0:  the bits of known[o]
 * with z = known_noise[j][o], or, known_noise NULL, the Philox draw of (seed, 0x80000000 | j, seq_offset + b, l, f): the
 * sampler's generator with the top bit of its step word set, a stream disjoint from the update's own draws.  It is made
 * once on x_init (level t_start + 1) and at the end of every step t (level t), inside the update kernel: no extra launch.
 * Elements with fixed[o] == 0 go through the plain sampler's arithmetic; the history rows hold the replaced values.
 *
 *   known        [B][L][F] values of the fixed elements, in the model's space (mean offset subtracted); elsewhere unread
 *   fixed        uint8 [B][L][F]; a fixed element at a position >= lens[b] is FD_E_INVALID ("fixed" in fd_last_error())
 *   known_coef   float32 [2][T+1]: keep[0..T], then spread[0..T]
 *   known_noise  [t_start+2][B][L][F], row j = the draws of level j (row 0 is never read), or NULL (Philox)
 * fd_sample_inpaint is fd_sample_ex plus these four (host buffers; `noise` and `known_noise` are given or NULL independently of
 * each other).  known, fixed or known_coef NULL: FD_E_INVALID, before any device call.  A later fd_sample* on the same model
 * is unaffected.  Options "use_graph" and "varlen", both precisions and full_history = 0, 1, k as in fd_sample. */
int fd_sample_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start, const float* noise,
                      const float* known, const uint8_t* fixed, const float* known_coef, const float* known_noise,
                      uint64_t seed, int64_t seq_offset, float* out, int full_history);

/* The parity hook of the above: fd_p_sample_step, then the replacement of the fixed elements at level t with the draws
 * z_known [B][L][F] (required for t > 0; level 0 writes known's bits).  x is taken as given: no initial replacement.
 * With wrap == 0 neither the update nor the replacement wraps. */
int fd_p_sample_step_inpaint(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, const float* z, int wrap,
                             const float* known, const uint8_t* fixed, const float* known_coef, const float* z_known,
                             float* x_out);

/* ---- resampling ("jump") schedules of motif-conditioned sampling: the run goes back up the noise ladder and comes down
 * again, so that the free elements get further chances to agree with the fixed ones (Lugmayr et al. 2022, RePaint).
 *
 * Visits.  visits[0 .. n_visits) is the step index t of every reverse step in the order run.  Legal: visits[0] == t_start,
 * visits[n_visits - 1] == 0, 0 <= visits[i] <= t_start, and for i > 0 either visits[i] == visits[i-1] - 1 (descent) or
 * visits[i] >= visits[i-1] (a JUMP: the state step visits[i-1] left at level a = visits[i-1] is forward-noised to level
 * b = visits[i] + 1 > a before step visits[i] runs).
 *
 * Segments and seeds.  Segment s is the run of visits behind the s-th jump (s = 0 in front of the first).  Every draw of
 * segment s -- the update's, the replacement's, and the jump that enters it -- has the Philox key
 * seed_s = seed + s * 0x9E3779B97F4A7C15 (mod 2^64); seed_0 = seed, so a schedule without a jump is fd_sample_inpaint's run
 * bit for bit, and a step index visited again draws fresh noise.
 *
 * The jump to level b entering segment s, for every element o = (i, l, f) with l < lens[i]:
 *   fixed[o] != 0:  the replacement at level b with seed_s (the known value noised afresh)
 *   otherwise:      jk * x[o] + js * z, each product and the sum rounded once, wrapped to [-pi, pi) where feature f is an
 *                   angle; z = the Philox draw of (seed_s, 0x40000000 | b, seq_offset + i, l, f), a third stream (T < 2^30)
 * Positions l >= lens[i] are left as they are.  jump_coef [n_jumps][2] = (jk, js) per jump in the order met:
 * jk = sqrt(acp(b) / acp(a)), js = sqrt(1 - acp(b) / acp(a)), acp(0) = 1, acp(j) = alphas_cumprod[j-1]; each finite and
 * within [0, 1].  NULL is allowed when the schedule has no jump.
 *
 * Both noise streams come from Philox; `out` [B][L][F] receives the final state only (the history of a non-monotone run is
 * not built).  Between the upload and the download the host issues launches only; the captured step graph is the plain
 * sampler's.  An illegal schedule (fd_last_error() names the index), a NULL visits, n_visits < 1, a NULL jump_coef with a
 * jump, a jk / js outside [0, 1] or anything fd_sample_inpaint rejects: FD_E_INVALID before any device call, `out` untouched.
 * Options "use_graph" and "varlen" and both precisions as in fd_sample_inpaint; a later fd_sample* is unaffected. */
int fd_sample_inpaint_resample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, int t_start,
                               const float* known, const uint8_t* fixed, const float* known_coef, const int32_t* visits,
                               int n_visits, const float* jump_coef, uint64_t seed, int64_t seq_offset, float* out);

/* The parity hook of one jump: x_out = x taken to level level_to (1 .. T) with (jk, js) and the Philox key `seed` (the
 * caller passes the segment's seed).  x is taken as given. */
int fd_inpaint_jump(fd_model* m, const float* x, const int32_t* lens, int B, int L, int level_to, float jk, float js,
                    const float* known, const uint8_t* fixed, const float* known_coef, uint64_t seed, int64_t seq_offset,
                    float* x_out);

/* ---- few-step sampling on a strided schedule: the run visits a SUBSEQUENCE of the timesteps and takes the state from each
 * visit's level straight to the next visit's with the DDIM update (Song et al. 2021) -- K network evaluations instead of T,
 * from the same checkpoint.  The reference has no such sampler; like fd_sample_inpaint this is an extension.
 *
 * Levels are those of the inpainting block above: the state that enters step t is at level t + 1.  Visit i runs the network
 * at t = visits[i] on a state at level p = visits[i] + 1 and leaves it at level q = visits[i+1] + 1 (q = 0 behind the last
 * visit).  The library knows nothing of levels or eta: the caller's coefficients say where each visit lands.
 *
 * The update of visit i, for every element o = (b, l, f) with l < lens[b]:
 *   x' = a[i] * x[o] + b[i] * eps[o]            each product and the sum rounded once, no contraction
 *   x' = x' + s[i] * z                          only where s[i] != 0 (product and sum rounded once)
 *   x' = wrap to [-pi, pi)                      where the model's feature f is an angle
 * z = noise[i][o], or, noise NULL, the Philox draw of (seed, visits[i], seq_offset + b, l, f): the plain sampler's key.
 * Where s[i] == 0 z is neither read nor drawn: a run with every s == 0 (DDIM, eta = 0) is a deterministic map of x_init,
 * evaluates no Philox and needs no noise array.  sampling.ddim_coefficients gives, with acp(0) = 1, acp(j) =
 * alphas_cumprod[j-1] and r = acp(p) / acp(q):
 *   s = eta * sqrt((1 - acp(q)) / (1 - acp(p))) * sqrt(1 - r),  a = sqrt(1 / r),
 *   b = sqrt(max(1 - acp(q) - s^2, 0)) - a * sqrt(1 - acp(p))
 * computed in float64 and rounded once; eta = 1 with all T visits is p_sample's own update (its coefficients to 2.7e-13).
 *
 *   visits   int32[K], strictly descending, 0 <= visits[i] < T (host)
 *   coef     float32 [3][K], rows a | b | s, all finite (host)
 *   x_init   [B][L][F] the state that enters step visits[0]
 *   noise    [K][B][L][F], row i = the draws of visit i (read only where s[i] != 0), or NULL (Philox)
 *   out      full_history == 0: [B][L][F]; 1: [K][B][L][F] (row i = the state after visit i); k > 1: [ceil(K/k)] rows, the
 *            states i = k-1, 2k-1, ... and the final one in the last row
 * The tables live in device buffers of the call; the update kernels look them up by the timestep they hold, and the step
 * counter advances to the next visit on the device.  The captured step graph is the plain sampler's and is not re-captured.
 * A NULL visits or coef, n_visits < 1, a visit outside [0, T), visits[i] >= visits[i-1] or a coefficient that is not finite:
 * FD_E_INVALID before any device call (fd_last_error() names the index), `out` untouched.  Options "use_graph" and "varlen"
 * and both precisions as in fd_sample; a later fd_sample* is unaffected.  With motif conditioning: fd_sample_strided_inpaint. */
int fd_sample_strided(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                      const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, float* out, int full_history);

/* The same with x_init, lens, noise and out already in device memory (visits and coef stay host arrays), on `hip_stream`
 * (NULL = the model's own stream).  Unlike fd_sample_dev it returns with the stream drained: the tables are freed with the
 * call. */
int fd_sample_strided_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, const int32_t* visits,
                          int n_visits, const float* coef, const void* noise_dev, uint64_t seed, int64_t seq_offset, void* out_dev,
                          int full_history, void* hip_stream);

/* The parity hook of the above: ONE update at timestep t with explicit (a, b, s), all finite; z [B][L][F] is required exactly
 * when s != 0.  eps_out (or NULL) receives the network's prediction, the bits of fd_forward's.  With wrap == 0 nothing is
 * wrapped.  Host buffers. */
int fd_p_sample_step_coef(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                          const float* z, int wrap, float* eps_out, float* x_out);

/* ---- few-step motif scaffolding: a strided run with replacement, and resampling jumps over visits.
 *
 * Levels are those of the two blocks above.  Visit i of a grid g_0 > g_1 > ... > g_{K-1} runs the network at t = g_i on a state
 * at level g_i + 1 and leaves it at level q_i = g_{i+1} + 1, q_{K-1} = 0.  An element with fixed[o] != 0 leaves visit i as the
 * replacement AT LEVEL q_i (not g_i: the level the state has just reached): keep[q_i] * known[o] + spread[q_i] * z, wrapped
 * where angular, with z = known_noise[i + 1][o] or the Philox draw of (seed, 0x80000000 | q_i, seq_offset + b, l, f); q_i = 0
 * gives the bits of known[o].  It reads or draws no z of the update's own.  Every other element takes fd_sample_strided's
 * statement unchanged, and so do the history rows and the step counter.  x_init's fixed elements are replaced at level
 * g_0 + 1 first (known_noise row 0).  No launch is added to a step and the captured step graph is the plain sampler's.
 *
 *   visits, coef, noise, out, full_history   as in fd_sample_strided
 *   known, fixed, known_coef                 as in fd_sample_inpaint
 *   known_noise  [n_visits + 1][B][L][F]: row 0 = the draws of the start point, row i + 1 = those of the state visit i leaves
 *                (the last row is never read: level 0), or NULL (Philox).  Rows are per VISIT here, not per level.
 * With fixed all zero the result is fd_sample_strided's.  Everything fd_sample_strided or fd_sample_inpaint rejects:
 * FD_E_INVALID before any device call, `out` untouched.  A later fd_sample* on the same model is unaffected. */
int fd_sample_strided_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                              int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                              const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset, float* out,
                              int full_history);

/* The same over a resampled run.  grid [n_grid] and coef [3][n_grid] are fd_sample_strided's visits and coefficients; run
 * [n_run] is the timestep of every visit in the order run.  Legal: run[0] == grid[0], run[n_run - 1] == grid[n_grid - 1],
 * every entry on the grid, and for i > 0 either run[i] is the grid's successor of run[i-1] (a descent) or run[i] >= run[i-1]
 * (a JUMP: the state visit run[i-1] left at level a -- its q, 0 behind the grid's last visit -- is forward-noised to level
 * b = run[i] + 1 > a).  Segments, their seeds seed + s * 0x9E3779B97F4A7C15, the jump's statement and its streams are
 * fd_sample_inpaint_resample's; jump_coef [n_jumps][2] = (jk, js) between those a and b.  A run without a jump is
 * fd_sample_strided_inpaint's bit for bit.  Philox only, final state only; launches only between upload and download.
 * An illegal run (fd_last_error() names the index), a NULL run, n_run < 1, a NULL jump_coef with a jump, jk / js outside
 * [0, 1] or anything the entry above rejects: FD_E_INVALID; T >= 2^30: FD_E_UNSUPPORTED; before any device call. */
int fd_sample_strided_inpaint_resample(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* grid,
                                       int n_grid, const float* coef, const int32_t* run, int n_run, const float* jump_coef,
                                       const float* known, const uint8_t* fixed, const float* known_coef, uint64_t seed,
                                       int64_t seq_offset, float* out);

/* The parity hook of a conditioned visit: fd_p_sample_step_coef, with the fixed elements replaced at level level_out
 * (0 .. T) with the draws z_known [B][L][F] (required for level_out >= 1; level 0 writes known's bits).  x is taken as given. */
int fd_p_sample_step_coef_inpaint(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                                  const float* z, int wrap, int level_out, const float* known, const uint8_t* fixed,
                                  const float* known_coef, const float* z_known, float* eps_out, float* x_out);

/* ---- few-step sampling with a second-order multistep solver, in the manner of DPM-Solver++(2M) (Lu et al. 2022): a strided
 * run without noise whose update also uses the previous visit's prediction of the clean state.  K network evaluations, one
 * [B][L][F] buffer more.  The reference has no such sampler; like fd_sample_strided this is an extension.
 *
 * Visits and levels are fd_sample_strided's.  The update of visit i with (a, b, c, u, v) = coef[.][i], for every element
 * o = (b, l, f) with l < lens[b]; `angular`: the model's feature f is an angle; every product and every sum rounded once, no
 * contraction:
 *   m  = a * x[o] + b * eps[o]                                   fd_sample_strided's mean
 *   x0 = u * x[o] + v * eps[o];   angular: x0 = wrap(x0)          the prediction of the clean state
 *   c != 0:  d = x0 - prev[o];    angular: d = wrap(d);   m = m + c * d
 *   angular: m = wrap(m)
 *   prev[o] = x0;  x'[o] = m
 * wrap = to [-pi, pi).  The difference is wrapped: two predictions of an angle either side of +-pi are close on the circle and
 * about 2 pi apart as numbers.  Where c == 0, prev[o] is NOT read (the first visit finds it uninitialised).  Nothing is drawn:
 * the run is a deterministic map of x_init.  sampling.solver_coefficients gives a and b of ddim_coefficients(eta = 0),
 * u = 1 / alpha_p, v = -sigma_p / alpha_p and, with lam = log(alpha / sigma), h = lam_q - lam_p, r = (lam_p - lam_p') / h
 * (p' = the level visit i - 1 ran at): c = alpha_q (1 - exp(-h)) / (2 r); c = 0 for the first visit, for the last (level 0
 * has infinite log-SNR) and everywhere at order 1, where the run is fd_sample_strided's with every s == 0, bit for bit.
 *
 *   visits   as in fd_sample_strided
 *   coef     float32 [5][K], rows a | b | c | u | v, all finite, c[0] == 0 (host)
 *   x_init, out, full_history   as in fd_sample_strided
 * prev and the tables live in device buffers of the call.  The captured step graph is the plain sampler's and is not
 * re-captured.  Everything fd_sample_strided rejects, a coefficient that is not finite or c[0] != 0: FD_E_INVALID before any
 * device call (fd_last_error() names the index), `out` untouched.  Options "use_graph" and "varlen" and both precisions as in
 * fd_sample; a later fd_sample* is unaffected.  Not offered with motif conditioning. */
int fd_sample_solver(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, float* out, int full_history);

/* The same with x_init, lens and out already in device memory (visits and coef stay host arrays), on `hip_stream` (NULL = the
 * model's own stream).  Like fd_sample_strided_dev it returns with the stream drained. */
int fd_sample_solver_dev(fd_model* m, const void* x_init_dev, const void* lens_dev, int B, int L, const int32_t* visits,
                         int n_visits, const float* coef, void* out_dev, int full_history, void* hip_stream);

/* The parity hook of the above: ONE update at timestep t with explicit (a, b, c, u, v), all finite.  x0_prev [B][L][F] is
 * required exactly when c != 0 (given with c == 0 it is not read).  eps_out (or NULL) receives the network's prediction, the
 * bits of fd_forward's; x0_out (or NULL) the visit's x0.  With wrap == 0 nothing is wrapped.  Host buffers. */
int fd_p_sample_step_solver(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float c, float u,
                            float v, const float* x0_prev, int wrap, float* eps_out, float* x0_out, float* x_out);

/* ---- steering a few-step run by particle resampling on device rewards, in the manner of Feynman-Kac steering (Singhal et
 * al. 2025) and twisted sequential Monte Carlo: no gradient, no backward pass.  The reference has no such sampler; like
 * fd_sample_strided this is an extension.
 *
 * The run carries P = n_particles particles for each of G = B / P requested backbones; the particles of group g are the
 * sequences g P .. g P + P - 1 and share one length.  Every visit is fd_sample_strided's visit (noise included: with every
 * s == 0 the copies of a particle would stay identical) and also writes its prediction of the clean state, the x0 of
 * fd_sample_solver's statement: x0 = u[i] * x[o] + v[i] * eps[o], product and sum rounded once, wrapped where angular.  A
 * visit with event[i] != 0 is followed by an EVENT, four launches on the state the visit left:
 *   shift     ang = x0 + offset[f] in float32, rounded once, wrapped where the model's feature f is an angle
 *             (fd_shift_trim_dev's statement without the trim; has_offset == 0: ang = x0 as it is)
 *   rewards   fd_nerf's coordinates of ang (center = 0), fp64 [B][3L][3]; per particle b of length len:
 *               terms[b][0] = fd_backbone_clashes' count of the coordinates rounded to float32, with clash_alpha
 *               terms[b][1] = the radius of gyration of the CA atoms in Angstrom, sqrt(sum |ca_i - mean|^2 / len), fp64
 *               terms[b][2], terms[b][3] = the residues fd_annotate_sse labels helix (1) and strand (2), divided by len
 *               reward[b] = w0 terms[b][0] + w1 terms[b][1] + w2 terms[b][2] + w3 terms[b][3], summed left to right, every
 *                           product and sum rounded once
 *   resample  per group, with every sum in index order:
 *               logw[b] += lambda * (reward[b] - r_prev[b]);  r_prev[b] = reward[b]
 *               mx = max logw;  w_j = exp(logw_j - mx);  W = sum w_j;  ESS = W W / sum w_j^2
 *               resample iff ess_frac >= 1, or ESS < ess_frac * P; never if W is not finite or not > 0:
 *                 target_k = (u[g] + k) / P * W, k = 0 .. P - 1
 *                 anc[k] = the smallest j with (w_0 + .. + w_j) > target_k   (P - 1 if none)
 *                 r_prev[k] <- r_prev[anc[k]];  logw[k] <- 0
 *               else anc[k] = k
 *   gather    x[b] <- x[g P + anc[b - g P]], the whole [L][F] block of a sequence
 * r_prev and logw start at 0, so the product of an unresampled particle's potentials telescopes to exp(lambda * reward of its
 * latest event).  After the last visit terms_out and reward_out are the rewards statement on the FINAL state (shifted in the
 * same way) and logw_out is what the last event left.
 *
 *   visits, noise, seed, seq_offset, x_init   as in fd_sample_strided
 *   coef           float32 [5][K], rows a | b | s | u | v, all finite (host): a | b | s are fd_sample_strided's, u | v
 *                  fd_sample_solver's
 *   event          uint8[K]
 *   params         weights, lambda (finite), ess_frac (>= 0), clash_alpha (> 0), feat_idx as in fd_nerf, the offset
 *   u              double [n_events][G], each in [0, 1): row e belongs to the e-th visit with event != 0
 *   out            [B][L][F] the final state
 *   terms_out [B][4], reward_out [B], logw_out [B]   doubles (host)
 *   ancestors_out  int32 [n_events][B] global indices g P + anc, or NULL
 * Only launches happen between the upload and the download; the steps replay the plain sampler's captured graph, which is not
 * captured again.  Everything fd_sample_strided rejects, a NULL event / u / params / terms_out / reward_out / logw_out,
 * n_particles outside [1, 1024], B not a multiple of n_particles, unequal lengths within a group, a length above 2048, fewer
 * than 3 or more than 16 features, a bad feat_idx, a u outside [0, 1) or a u / v / weight / lambda / offset that is not
 * finite, ess_frac < 0, clash_alpha <= 0: FD_E_INVALID before any device call, `out` untouched.  Options "use_graph" and
 * "varlen" and both precisions as in fd_sample_strided; a later fd_sample* is unaffected.  Final state only; not offered with
 * motif conditioning or with the second-order solver. */
typedef struct fd_steer_params {
  double weights[4];   /* clashes | radius of gyration | helix fraction | strand fraction */
  double lambda;
  double ess_frac;
  double clash_alpha;
  int32_t feat_idx[9];
  int32_t has_offset;
  float offset[16];    /* the first F are read, and only where has_offset != 0 */
} fd_steer_params;
int fd_sample_steered(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                      const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const uint8_t* event,
                      int n_particles, const fd_steer_params* params, const double* u, float* out, double* terms_out,
                      double* reward_out, double* logw_out, int32_t* ancestors_out);

/* The parity hook of a steered visit: fd_p_sample_step_coef plus u, v (both finite) and x0_out [B][L][F] (required), which
 * receives the visit's prediction of the clean state.  x_out and eps_out are the bits of fd_p_sample_step_coef's. */
int fd_p_sample_step_coef_x0(fd_model* m, const float* x, int t, const int32_t* lens, int B, int L, float a, float b, float s,
                             float u, float v, const float* z, int wrap, float* eps_out, float* x0_out, float* x_out);

/* The shift and rewards statements above on host arrays, model-free and synchronous like fd_nerf.
 *   x          float32 [B][L][F] (host); finite on the rows l < lens[b]
 *   lens       int32[B], 1 <= lens[b] <= min(L, 2048)
 *   feat_idx   int32[9] as in fd_nerf; 3 <= F <= 16
 *   offset     float32[F], or NULL: x is taken as it is; is_angle uint8[F] (required with an offset): the features to wrap
 *   weights    double[4], finite; clash_alpha > 0
 *   terms_out  double [B][4], reward_out double [B]
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
int fd_steer_rewards(int device_id, const float* x, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                     const float* offset, const uint8_t* is_angle, const double* weights, double clash_alpha,
                     double* terms_out, double* reward_out);

/* The resample statement above on host arrays, model-free and synchronous: G groups of P consecutive particles.
 *   reward         double [G P]
 *   logw, r_prev   double [G P], in and out
 *   lambda finite, ess_frac >= 0, 1 <= P <= 1024, u double[G] each in [0, 1)
 *   ancestors_out  int32 [G P] global indices, resampled_out uint8 [G]
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs and logw / r_prev untouched. */
int fd_steer_resample(int device_id, const double* reward, double* logw, double* r_prev, int G, int P, double lambda,
                      double ess_frac, const double* u, int32_t* ancestors_out, uint8_t* resampled_out);

/* ---- repeat proteins: a few-step run whose angle rows are tied across the units of an internal repeat.  A
 * residue's features are internal angles, so a chain whose rows are periodic has exact screw symmetry (all but residue 0, which
 * NeRF seeds from fixed coordinates).  Sequence b has a tie (start, period, units): the tied region is the rows
 * [start, start + period * units), row start + k * period + j is copy k of unit row j, and units == 1 ties nothing.
 * The tie statement, in place on a [B][L][F] state, every product, sum and quotient rounded once in float32; for a tied element
 * with x_k its value in copy k:
 *     d_k = x_k - x_0, wrapped to [-pi, pi) where the feature is angular            k = 1 .. units - 1
 *     m   = x_0 + (d_1 + d_2 + ... + d_{units-1}) / float(units)                    summed left to right
 *     m   = m + s * z  where s != 0;   m = wrap(m) where angular;   every copy <- m
 * and for an element of a row below lens[b] outside the region: m = x, then the same + s z and wrap.  z is the entry of the
 * visit's draws at the copy-0 position (b, start + j, f), or without draws philox_normal(seed, t, seq_offset + b, start + j, f):
 * what the update kernel would have drawn there (a free element: its own position).  Rows at or beyond lens[b] are neither
 * read nor written.  The `init` statement: every copy <- x_0, nothing else.
 *
 * fd_sample_repeat is fd_sample_strided (final state only) with the ties enforced at every visit: the init statement on the
 * start point, then per visit i the strided update without its draw -- wrap(a x + b eps) -- followed by the tie statement with
 * s = coef[2][i], t = visits[i] and row i of `noise`.  The copies therefore start equal, see the mean of the units'
 * predictions and receive the same draw: they stay bit-identical.
 *   visits, coef [3][K], noise [K][B][L][F] or NULL, seed, seq_offset, x_init, lens   as in fd_sample_strided
 *   tie            int32 [B][3] start | period | units (host): start >= 0, period >= 1, units >= 1,
 *                  start + period * units <= lens[b]
 *   out            [B][L][F] the final state
 * One tie launch sits between two replays of the plain sampler's captured step graph; nothing is asked of the host between the
 * upload and the download.  Everything fd_sample_strided rejects, a NULL tie or a tie outside its sequence: FD_E_INVALID before
 * any device call, `out` untouched.  Options "use_graph" and "varlen" and both precisions as in fd_sample_strided; a later
 * fd_sample* is unaffected.  Not offered with motif conditioning, the second-order solver or steering. */
int fd_sample_repeat(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const int32_t* tie, float* out);

/* The tie statement above on host arrays, model-free and synchronous like fd_nerf.
 *   x          float32 [B][L][F] (host); lens int32[B] in [1, L]; tie int32 [B][3] as above; 1 <= F <= 32
 *   is_angle   uint8[F]: the features to wrap
 *   init       != 0: the init statement (s, z, seed, t and seq_offset are not looked at)
 *   s          finite; z float32 [B][L][F], or NULL: Philox with (seed, t, seq_offset); neither is looked at where s == 0
 *   out        float32 [B][L][F]: the rows below lens[b]; the others keep what they held
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), `out` untouched. */
int fd_tie_repeats(int device_id, const float* x, const int32_t* lens, const int32_t* tie, int B, int L, int F,
                   const uint8_t* is_angle, int init, float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* out);

/* ---- restraint guidance: the derivative of NeRF, distance restraints between backbone atoms, and a few-step run
 * that follows every visit with a step down the gradient of the restraint energy of the visit's predicted structure.
 *
 * fd_nerf_vjp_feats: the gradient with respect to the NeRF features of any function of the coordinates, from the coordinates and
 * the float32 feature rows fd_nerf built them from, model-free and synchronous like fd_nerf, fp64 throughout.  fd_nerf_vjp: the
 * same from the coordinates alone, with every sign below taken as +1 -- right on the rows where every bond-angle feature has
 * sin(angle) > 0 and every bond-length feature is > 0 (a backbone's own), wrong in sign elsewhere: use fd_nerf_vjp_feats there.  Per chain of len residues, n = 3 len atoms; atom k >= 3 was
 * placed from atoms k-3, k-2, k-1, and with i = (k - 3) / 3, j = (k - 3) % 3 its features are
 *     j = 0 (next N):   torsion psi (row i)        angle CA:C:1N (row i)                          length 0C:1N (row i)
 *     j = 1 (next CA):  torsion omega (row i)      angle C:1N:1CA (row i)                         length N:CA (row i)
 *     j = 2 (next C):   torsion phi (row i + 1)    angle N:CA:C (row i: the reference's quirk)    length CA:C (row i)
 *   g_k  = dcoords[k], with centered != 0 minus the mean of dcoords over the chain's atoms (the derivative of fd_nerf's center = 1)
 *   q_k  = p_k - p_0: positions relative to the chain's atom 0
 *   Fs_k = sum_{m >= k} g_m,   Tq_k = sum_{m >= k} q_m x g_m
 *   with b = q_{k-2}, c = q_{k-1}, d = q_k, u = unit(c - b), r = d - c, M = Tq_k - c x Fs_k:
 *     d / d torsion = u . M      d / d angle = sa unit(r x u) . M      d / d length = sl unit(r) . Fs_k
 *   sl = sign(length feature),  sa = sign(sin((double)angle feature)) sl, each feature read from row i as float32, the row the
 *   forward read it from; the sign of zero is +1, and so is the sign of a slot whose feat_idx is -1 (the defaults are positive).
 *   The coordinates cannot decide these signs: with r = bl (-cos(angle) u + sin(angle) w), unit(r x u) is the angle's rotation
 *   axis times sign(bl sin(angle)) and unit(r) the bond's direction times sign(bl); (angle, torsion) and (-angle, torsion + pi)
 *   build the same chain.  sin(angle) == 0 or length == 0 is outside the domain: fd_nerf's next frame is not finite there.
 * each to its (row, column); a slot whose feat_idx is -1 receives nothing, every other element of a row below len is 0 (phi of
 * residue 0, the last residue's psi / omega / angles / lengths, columns that are no NeRF feature), rows at or beyond len are not
 * written, len == 1: all zero.  A torsion, an angle or a length moves everything behind it as a rigid body, hence the suffix
 * sums; one workgroup per chain, every sum in an order fixed by the chain's length: two calls give the same bits.
 *   coords      float64 [B][3L][3] in fd_nerf's layout (host); dcoords the same shape; both finite on the atoms below 3 lens[b]
 *   lens        int32[B], 1 <= lens[b] <= min(L, 2048)
 *   feat_idx    int32[9] as in fd_nerf, and no column named twice; 3 <= F <= 16
 *   feats       (fd_nerf_vjp_feats) float32 [B][L][F], the array fd_nerf was given; finite on the rows below lens[b]
 *   dfeats_out  float64 [B][L][F]
 * Where every sign is +1 fd_nerf_vjp_feats returns fd_nerf_vjp's bits.
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
int fd_nerf_vjp(int device_id, const double* coords, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx, int centered,
                const double* dcoords, double* dfeats_out);
int fd_nerf_vjp_feats(int device_id, const double* coords, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                      int centered, const double* dcoords, const float* feats, double* dfeats_out);

/* Distance restraints, packed per chain: chain b owns entries rst_offsets[b] .. rst_offsets[b + 1] - 1 of the lists
 * (rst_offsets[0] == 0, non-decreasing; R = rst_offsets[B] may be 0, the lists are then not read).
 *   rst_i, rst_j           int32[R] atom indices 3 * residue + {0 N, 1 CA, 2 C} inside the chain's [0, 3 lens[b]), i != j
 *   rst_d0, rst_tol, rst_w double[R], finite, d0 >= 0, tol >= 0, w >= 0
 * Per restraint: d = |p_i - p_j|, v = max(0, |d - d0| - tol), E_b += w v^2, and where v > 0 and d > 0
 * dcoords[i] += 2 w v sign(d - d0) (p_i - p_j) / d, the opposite on j.  tol = 0 is harmonic; d0 = 0, tol = 8 is "within 8 A".
 * Distances do not tell a structure from its mirror image; fd_template_energy's term does.
 *   coords             float64 [B][3L][3] (host), finite on the atoms below 3 lens[b]; lens int32[B] in [1, min(L, 2048)]
 *   energy_out         double[B]; max_violation_out double[B]: the largest v, 0 without restraints
 *   dcoords_out        float64 [B][3L][3] (atoms at or beyond 3 lens[b]: 0), or NULL
 * No floating-point atomics: each atom belongs to a lane that walks the chain's list and sums the terms on its atom in list
 * order; the energy is summed in an order fixed by the list's length.  Two calls give the same bits.
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
int fd_restraint_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* rst_offsets,
                        const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                        double* energy_out, double* max_violation_out, double* dcoords_out);

/* The guide statement.  After a visit, x is the state it left and x0 its prediction of the clean state:
 *     ang    = the shift statement of fd_sample_steered on x0
 *     coords = fd_nerf(ang, center = 0)
 *     E, gc  = the restraint statement on coords
 *     G      = fd_nerf_vjp_feats(coords, gc, centered = 0, feats = ang)                 [B][L][F] fp64
 *     n_b    = sqrt(sum of G^2 over the rows below lens[b]), in a fixed order;   k_b = n_b > max_norm ? max_norm / n_b : 1
 *     x     <- x - float32((double(c) * k_b) * G)   only where c != 0 (c == 0 leaves x's bits alone, whatever G holds)
 *     x     <- x + s z  where s != 0;   x <- wrap(x) where angular
 * the last line being fd_tie_repeats' with units == 1: same draw position, same Philox word, same roundings.
 *
 * fd_guide_step: the statement on host arrays, model-free and synchronous like fd_nerf.
 *   x, x0      float32 [B][L][F] (host), finite on the rows below lens[b]; lens int32[B] in [1, min(L, 2048)]
 *   feat_idx   int32[9] as in fd_nerf_vjp; 3 <= F <= 16
 *   offset     float32[F] finite, or NULL: x0 is taken as it is; is_angle uint8[F]: the features to wrap
 *   rst_*      as in fd_restraint_energy
 *   c, s       finite; max_norm > 0
 *   z          float32 [B][L][F], or NULL: Philox with (seed, t, seq_offset); neither is looked at where s == 0
 *   x_out      float32 [B][L][F]: the rows below lens[b]; the others keep what they held
 *   energy_out double[B]: E of x0's structure; gnorm_out double[B]: n_b
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
int fd_guide_step(int device_id, const float* x, const float* x0, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                  const float* offset, const uint8_t* is_angle, const int32_t* rst_offsets, const int32_t* rst_i,
                  const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float c, double max_norm,
                  float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                  double* gnorm_out);

/* fd_sample_guided is fd_sample_strided (final state only) whose visits write their prediction of the clean state as
 * fd_sample_steered's do, run their update without its draw as fd_sample_repeat's do -- wrap(a x + b eps) -- and are each
 * followed by the guide statement with c = guide[i], s = coef[2][i], t = visits[i] and row i of `noise`: five launches (shift,
 * NeRF, restraints, derivative -- fd_nerf_vjp_feats' on the shifted rows, whose bond angles may lie anywhere on the circle --, update) between two replays of the plain sampler's captured step graph, which is not captured
 * again; nothing is asked of the host between the upload and the download.
 *   visits, noise, seed, seq_offset, x_init, lens   as in fd_sample_strided
 *   coef              float32 [5][K] rows a | b | s | u | v, all finite (host), as in fd_sample_steered
 *   guide             float32 [K], finite, zeros allowed
 *   params            feat_idx as in fd_nerf_vjp, the offset of the shift, max_norm > 0
 *   rst_*             as in fd_restraint_energy
 *   out               [B][L][F] the final state
 *   energy_out, max_violation_out   double[B]: the restraint statement on the FINAL state, shifted in the same way
 * Everything fd_sample_strided rejects, a NULL or non-finite u / v / guide, a NULL params or output, a restraint outside its
 * chain or with i == j, a negative or non-finite d0 / tol / w, max_norm <= 0 or not finite, a non-finite offset, a length above
 * 2048, fewer than 3 or more than 16 features, a bad feat_idx: FD_E_INVALID before any device call, `out` untouched.  Options
 * "use_graph" and "varlen" and both precisions as in fd_sample_strided; a later fd_sample* is unaffected.  Single device, final
 * state only; not offered with the second-order solver, steering or ties; with motif conditioning: fd_sample_guided_inpaint. */
typedef struct fd_guide_params {
  int32_t feat_idx[9];
  int32_t has_offset;
  float offset[16];    /* the first F are read, and only where has_offset != 0 */
  double max_norm;
} fd_guide_params;
int fd_sample_guided(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                     const float* coef, const float* noise, uint64_t seed, int64_t seq_offset, const float* guide,
                     const fd_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i, const int32_t* rst_j,
                     const double* rst_d0, const double* rst_tol, const double* rst_w, float* out, double* energy_out,
                     double* max_violation_out);

/* ---- relaxing backbones in torsion space: a model-free descent on a finished backbone's angles that removes
 * backbone clashes, honours distance restraints and may be tethered to where it started.  Backbone-only repulsion in torsion
 * space is no force field; whether relaxed backbones are more designable is unmeasured.
 *
 * fd_nerf_scan: fd_nerf with one workgroup per chain -- the same arguments, layout, `center`, padding zeros and feat_idx, with
 * 1 <= lens[b] <= min(L, 2048).  The displacement (d0, d1, d2) of atom k >= 3 in the frame of the three atoms before it is
 * exactly fd_nerf's (the same float32 cos / sin products, the same float64 default-angle path); fd_nerf recomputes that frame
 * [bc | nbc | n] from three positions, here it is carried: with u = unit(d), m = unit(e_x x u), M_k = [u | m x u | m],
 *     p_k = R_{k-1} d_k + p_{k-1},   R_k = R_{k-1} M_k,   (R_2, p_2) = fd_nerf's frame of the three seed atoms and the seed C,
 * and since (R, p) o (M, d) = (R M, R d + p) is associative a chain is a prefix scan over rigid transforms, in a tree whose shape
 * depends on the chain's length alone: two calls give the same bits, and a chain's bits do not depend on the batch it is in.
 * Not bit-equal to fd_nerf: per chain max |scan - fd_nerf| <= 1e-9 x the chain's largest |p_k - p_0| (measured: DESIGN.md 6x).
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), the output untouched. */
int fd_nerf_scan(int device_id, const float* feats, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx, int center,
                 double* coords_out);

/* The relax energy of a batch of angle rows x (float32 [B][L][F]) and its gradient in angle space:
 *     coords = fd_nerf_scan(x, center = 0)                                  fp64, never rounded to float32
 *     E_clash, gc: atoms 3 i + {0 N, 1 CA, 2 C}, r = 1.55 for N and 1.7 for CA and C; over the pairs a < b with b - a >= 2:
 *         t_ab = clash_alpha (r_a + r_b) + clash_margin (an fp64 product and sum),  v = max(0, t_ab - d(a, b)),
 *         E_clash = w_clash sum v^2;  on atom a  -2 w_clash v (p_a - p_b) / d where v > 0 and d > 0, the opposite on b
 *         (fd_backbone_clashes' rule made soft); an atom's gradient is summed in index order of the partner
 *     E_rst, gc += the restraint statement of fd_restraint_energy (R = 0 is allowed)
 *     G = fd_nerf_vjp_feats(coords, gc, centered = 0, feats = x)
 *     tether: delta = x - anchor in fp64, and where is_angle[f] delta - 2 pi floor((delta + pi) / (2 pi));
 *         E_tether = w_tether sum delta^2 over the rows below lens[b] and the columns with move[f];  G += 2 w_tether delta
 *     G = 0 where !move[f] or fixed[b][l]
 *     gnorm_b = sqrt(sum G^2) over the rows below lens[b], in a fixed order
 * No floating-point atomics anywhere; two calls give the same bits.
 *   feats        float32 [B][L][F] (host), finite on the rows below lens[b]; lens int32[B] in [1, min(L, 2048)]; 3 <= F <= 16
 *   anchor       the same shape and finite in the same rows, or NULL: the input itself (E_tether = 0, no gradient)
 *   params       feat_idx as in fd_nerf_vjp; is_angle / move: the first F are read; move[f] != 0 only where f is one of
 *                feat_idx's columns; clash_alpha, clash_margin, w_clash, w_tether finite and >= 0; the four step numbers are
 *                fd_relax's and are checked here as there
 *   fixed        uint8 [B][L] or NULL: rows that do not move
 *   rst_*        as in fd_restraint_energy
 *   energy_out   double[B][3] clash | restraint | tether;  gnorm_out double[B]
 *   dfeats_out   double[B][L][F] or NULL; rows at or beyond lens[b] are not written
 * With clash_margin >= 1e-3, E_clash == 0 implies that fd_backbone_clashes on the float32-rounded coordinates returns 0 at the
 * same alpha: rounding to float32 moves a distance by about 1e-5 A.
 * A bad call (the list is under fd_relax): FD_E_INVALID before any device call, the word in fd_last_error(), outputs untouched. */
typedef struct fd_relax_params {
  int32_t feat_idx[9];
  uint8_t is_angle[16], move[16];
  double clash_alpha, clash_margin, w_clash, w_tether;
  double step0, grow, shrink, max_step;
} fd_relax_params;
int fd_relax_energy(int device_id, const float* feats, const float* anchor, const int32_t* lens, int B, int L, int F,
                    const fd_relax_params* params, const uint8_t* fixed, const int32_t* rst_offsets, const int32_t* rst_i,
                    const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, double* energy_out,
                    double* gnorm_out, double* dfeats_out);

/* fd_relax: n_iter steps of a descent with an adaptive step on that energy, per chain, chains independent; E is the sum of the
 * three terms, (E, G, n) = fd_relax_energy's energies, gradient and norm:
 *     x = feats;  (E, G, n) of x;  h = step_io ? step_io[b] : step0;  trace[0] = E
 *     for it = 1 .. n_iter:
 *         s  = (h n > max_step) ? max_step / n : h
 *         x' = x - float32(s G), then wrapped as the samplers wrap where is_angle[f] -- where G != 0; an element with G == 0
 *              (immovable columns, fixed rows, phi of residue 0 ...) keeps its bits, as do the rows at or beyond lens[b]
 *         (E', G', n') of x'
 *         if E' <= E (false for NaN):  x, E, G, n = x', E', G', n';  h *= grow;  accepted += 1
 *         else:                        h *= shrink
 *         trace[it] = E
 *     feats_out = x;  energy_out = the three terms of x;  step_io[b] = h
 * anchor == NULL tethers to `feats`.  Nothing is asked of the host between the upload and the download: h, E, the decision and
 * the trial buffers live on the device; five launches per iteration (scan, restraints, clash, derivative, step).
 * fd_relax(n_iter = N) equals N calls with n_iter = 1 chained through feats_out, step_io and the same non-NULL anchor, bit for
 * bit, and energy_out equals fd_relax_energy(feats_out) with that anchor bit for bit.
 *   n_iter        >= 0; 0 returns the input and its energy
 *   step_io       double[B], each finite and > 0, or NULL
 *   feats_out     float32 [B][L][F]: the rows below lens[b]; the others keep what they held
 *   energy_out    double[B][3];  trace_out double[n_iter + 1][B] or NULL;  accepted_out int32[B]
 * Everything fd_guide_step rejects for shapes, lengths, feat_idx and restraints, a move column that is no NeRF feature of
 * feat_idx, a non-finite or negative weight, alpha or margin, step0 <= 0, grow < 1, shrink outside (0, 1), max_step <= 0,
 * a step_io entry that is not finite and > 0, n_iter < 0, non-finite feats or anchor on the rows below a length, a NULL params
 * or output: FD_E_INVALID before any device call, the word in fd_last_error(), outputs untouched. */
int fd_relax(int device_id, const float* feats, const float* anchor, const int32_t* lens, int B, int L, int F,
             const fd_relax_params* params, const uint8_t* fixed, const int32_t* rst_offsets, const int32_t* rst_i,
             const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, int n_iter, double* step_io,
             float* feats_out, double* energy_out, double* trace_out, int32_t* accepted_out);

/* ---- restraint guidance combined with replacement: discontiguous motifs.  Replacement (fd_sample_inpaint)
 * holds chosen elements of the angle rows, so a held run of residues reproduces that segment's backbone exactly, but says nothing
 * about where two held segments sit relative to each other; distance restraints (fd_sample_guided) place them.  Distances do
 * not tell a structure from its mirror image -- the superposition term below (fd_sample_guided_inpaint_tpl) does -- and whether
 * such scaffolds are designable is unmeasured.
 *
 * The scaffold-guide statement, per element o = (b, l, f) of [B][L][F].  After a visit, x is the state it left and x0 its
 * prediction of the clean state; fixed is uint8 [B][L][F], known float32 [B][L][F] in model space as for fd_sample_inpaint:
 *     p[o]   = fixed[o] ? known[o] : x0[o]        (a held element's clean value is KNOWN; x0[o] is never read where fixed[o])
 *     ang    = the shift statement of fd_sample_steered on p
 *     coords = fd_nerf_scan(ang, center = 0)
 *     E_rst, max_violation, gc = the restraint statement of fd_restraint_energy on coords
 *     E_clash, gc +=             fd_relax_energy's soft clash statement (clash_alpha, clash_margin, w_clash), only where w_clash > 0
 *     G      = fd_nerf_vjp_feats(coords, gc, centered = 0, feats = ang)                 [B][L][F] fp64
 *     G[o]   = 0 where fixed[o]
 *     n_b    = sqrt(sum of G^2 over the rows below lens[b]), in fd_guide_step's fixed order;  k_b = n_b > max_norm ? max_norm / n_b : 1
 *     free element:   x <- x - float32((double(c) * k_b) * G) only where c != 0;  x <- x + s z where s != 0;  x <- wrap(x) where
 *                     angular -- fd_guide_step's three lines: same draw position, same Philox word, same roundings
 *     fixed element:  keeps its bits; neither reads nor draws a z
 * The restraints are evaluated before the clashes, fd_relax_energy's order: with w_tether = 0 and every NeRF column movable,
 * fd_relax_energy's dfeats_out on the same ang is the unmasked G bit for bit.  No floating-point atomics; two calls give the
 * same bits.  With fixed all zero and w_clash = 0 the statement is fd_guide_step's with fd_nerf_scan in place of fd_nerf.
 *
 * fd_scaffold_guide_step: the statement on host arrays, model-free and synchronous like fd_guide_step.
 *   x            float32 [B][L][F] (host), finite on the rows below lens[b]; lens int32[B] in [1, min(L, 2048)]; 3 <= F <= 16
 *   x0           the same shape, finite on the free elements of those rows
 *   known, fixed never NULL; known finite where fixed (not read elsewhere: NaN is allowed there); nothing fixed at or beyond lens[b]
 *   is_angle     uint8[F]: the features to wrap
 *   params       feat_idx as in fd_nerf_vjp, the offset of the shift, max_norm > 0 and finite; clash_alpha, clash_margin and
 *                w_clash finite and >= 0 (w_clash == 0: no clash term)
 *   rst_*        as in fd_restraint_energy;  c, s finite
 *   z            float32 [B][L][F], or NULL: Philox with (seed, t, seq_offset); neither is looked at where s == 0
 *   x_out        float32 [B][L][F]: the rows below lens[b]; the others keep what they held
 *   energy_out   double[B][2] restraint | clash of p's structure (clash: 0 where w_clash == 0); max_violation_out, gnorm_out double[B]
 *   dfeats_out   double[B][L][F] the masked G on the rows below lens[b], or NULL
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
typedef struct fd_scaffold_guide_params {
  int32_t feat_idx[9];
  int32_t has_offset;
  float offset[16];                           /* the first F are read, and only where has_offset != 0 */
  double max_norm;                            /* > 0 */
  double clash_alpha, clash_margin, w_clash;  /* finite, >= 0; w_clash == 0: no clash term, alpha and margin unread */
} fd_scaffold_guide_params;
int fd_scaffold_guide_step(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                           const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                           const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                           const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float c, float s,
                           const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                           double* max_violation_out, double* gnorm_out, double* dfeats_out);

/* fd_sample_guided_inpaint is fd_sample_guided with fd_sample_strided_inpaint's conditioning, final state only.  The start
 * point's fixed elements are replaced at level visits[0] + 1 (known_noise row 0).  Visit i is a replay of the plain sampler's
 * captured step graph, which is not captured again: a fixed element leaves it at the level the visit lands on, next_t + 1, from
 * row i + 1 of known_noise or the Philox draw fd_sample_strided_inpaint takes; a free element leaves as wrap(a x + b eps) with
 * x0 = wrap(u x + v eps).  The scaffold-guide statement follows with c = guide[i], s = coef[2][i], t = visits[i] and row i of
 * `noise`: six launches (shift, scan, restraints, clashes, derivative, update; five where w_clash == 0), all one workgroup per
 * chain.  Behind the last visit the fixed elements hold known's bits.  Nothing is asked of the host between the upload and the
 * download.
 *   visits, coef, noise, seed, seq_offset, guide, rst_*   as in fd_sample_guided
 *   known, fixed, known_coef, known_noise                 as in fd_sample_strided_inpaint (known_noise [K + 1][B][L][F] or NULL)
 *   params            as in fd_scaffold_guide_step
 *   out               [B][L][F] the final state
 *   energy_out        double[B][2] restraint | clash and max_violation_out double[B]: the statement's energies with p = the FINAL state
 * Everything fd_sample_guided and fd_sample_strided_inpaint reject, a NULL known or fixed, a non-finite known[o] where fixed[o]
 * (where nothing is fixed known is not read), a negative or non-finite clash_alpha, clash_margin or w_clash: FD_E_INVALID before
 * any device call, outputs untouched.  Options "use_graph" and "varlen" and both precisions as in fd_sample_guided; a later
 * fd_sample* of any family is unaffected.  Single device; not offered with jumps, the second-order solver, steering or ties. */
int fd_sample_guided_inpaint(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits, int n_visits,
                             const float* coef, const float* noise, const float* known, const uint8_t* fixed, const float* known_coef,
                             const float* known_noise, uint64_t seed, int64_t seq_offset, const float* guide,
                             const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                             const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float* out,
                             double* energy_out, double* max_violation_out);

/* ---- superposition restraints: place chosen atoms in 3D, handedness included.  The squared deviation of chosen
 * atoms from a template after the optimal superposition by a PROPER rotation: a mirror image cannot be superposed, so it costs
 * energy, which no set of distances can make it do.
 *
 * The template statement.  Chain b's entries are k = tpl_offsets[b] .. tpl_offsets[b + 1] - 1: an atom index a_k inside the chain's
 * [0, 3 lens[b]) (3 * residue + {0 N, 1 CA, 2 C}), strictly increasing within the chain, a target m_k and a weight w_k > 0.
 *     W   = sum w_k;   cp = sum w_k p[a_k] / W;   cm = sum w_k m_k / W
 *     M[i][j] = sum w_k (m_k - cm)_i (p[a_k] - cp)_j        centred: a second pass over the entries, so that a template far from
 *                                                           the origin loses nothing
 *     R   = the proper rotation that maximises trace(R^T M) -- R (m - cm) ~ p - cp --, by Horn's quaternion method in fp64
 *     r_k = (p[a_k] - cp) - R (m_k - cm)                    explicit residuals
 *     E_tpl = sum w_k |r_k|^2;   rmsd = sqrt(E_tpl / W);   dE/dp[a_k] = 2 w_k r_k
 *     transform: R (row-major), t = cp - R cm               (R m + t superposes the template on the chain)
 * The gradient is exact by the envelope theorem: R is optimal, so E does not change to first order with R, and sum w_k r_k = 0,
 * so the centroid adds nothing.  E and rmsd come from the explicit residuals, never from the eigenvalue: at a perfect fit the
 * eigenvalue form cancels.  A chain with no entries has E = 0 and rmsd = 0, the identity transform, and receives no gradient.
 * One or two entries, or collinear targets, are allowed: the optimal R is then not unique, but every optimal R gives the same
 * residuals (transform_out then holds one of them).  OUTSIDE THE DOMAIN: where the two largest eigenvalues of Horn's 4x4 matrix
 * coincide with non-collinear points the optimal rotation jumps and the energy is not differentiable; that is a set of measure
 * zero (a structure as close to the template's mirror image as to the template), and what is returned there is one of the
 * optimal fits.  One template per chain.
 * No floating-point atomics: one 256-lane workgroup per chain, three lane-strided passes over the entries, every sum in an order
 * fixed by (entry count, lane); each named atom is written by the one lane that owns its entry.  Two calls give the same bits,
 * and a chain's bits do not depend on the batch it is in.
 *
 * fd_template_energy: the statement on host arrays, model-free and synchronous like fd_restraint_energy.
 *   coords         float64 [B][3L][3] (host), finite on the atoms below 3 lens[b]; lens int32[B] in [1, min(L, 2048)]
 *   tpl_offsets    int32[B + 1], tpl_offsets[0] == 0, non-decreasing; n = tpl_offsets[B] may be 0
 *   tpl_atom       int32[n];  tpl_xyz double[n][3], finite;  tpl_w double[n], finite and > 0
 *                  (all four NULL: no template anywhere; some but not all NULL is an error)
 *   energy_out, rmsd_out   double[B]
 *   transform_out  double[B][12] R row-major then t, or NULL
 *   dcoords_out    float64 [B][3L][3], or NULL: written everywhere, 0 on the atoms that are not named
 * A bad call -- non-monotone offsets or tpl_offsets[0] != 0, an atom outside [0, 3 lens[b]) or atoms not strictly increasing
 * within a chain, a weight that is not finite or <= 0, a non-finite target, some but not all of the four arrays NULL, and what
 * fd_restraint_energy rejects for coords and lens: FD_E_INVALID before any device call, the offending word in fd_last_error(),
 * outputs untouched. */
int fd_template_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* tpl_offsets,
                       const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w, double* energy_out, double* rmsd_out,
                       double* transform_out, double* dcoords_out);

/* fd_scaffold_guide_step_tpl: fd_scaffold_guide_step whose statement gains one line after the clash line,
 *     E_tpl, rmsd, gc += the template statement on coords        (that launch is skipped when no chain has an entry)
 * with fd_scaffold_guide_step's arguments and meaning otherwise.
 *   tpl_*          as in fd_template_energy; all four NULL: no template, and every output fd_scaffold_guide_step shares equals
 *                  that entry's bit for bit
 *   energy_out     double[B][3] restraint | clash | template of p's structure;  tpl_rmsd_out double[B] (0 without entries)
 * Everything fd_scaffold_guide_step and fd_template_energy reject, a NULL tpl_rmsd_out: FD_E_INVALID before any device call,
 * outputs untouched. */
int fd_scaffold_guide_step_tpl(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                               const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                               const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                               const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                               const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w, float c,
                               float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                               double* max_violation_out, double* gnorm_out, double* dfeats_out, double* tpl_rmsd_out);

/* fd_sample_guided_inpaint_tpl: fd_sample_guided_inpaint whose visits are followed by fd_scaffold_guide_step_tpl's statement:
 * seven launches per visit at most (shift, scan, restraints, clashes, template, derivative, update).  The plain sampler's
 * captured step graph is not captured again.
 *   tpl_*          as in fd_scaffold_guide_step_tpl; all four NULL: out, the two energies and max_violation_out are
 *                  fd_sample_guided_inpaint's bit for bit
 *   energy_out     double[B][3] restraint | clash | template and tpl_rmsd_out double[B]: the statement with p = the FINAL state
 * Everything fd_sample_guided_inpaint and fd_template_energy reject, a NULL tpl_rmsd_out: FD_E_INVALID before any device call,
 * outputs untouched.  Not offered in fd_relax, fd_sample_guided or fd_guide_step, nor with jumps, the second-order solver,
 * steering or ties; single device. */
int fd_sample_guided_inpaint_tpl(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                                 int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                                 const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset,
                                 const float* guide, const fd_scaffold_guide_params* params, const int32_t* rst_offsets,
                                 const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol,
                                 const double* rst_w, const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz,
                                 const double* tpl_w, float* out, double* energy_out, double* max_violation_out, double* tpl_rmsd_out);

/* ---- cyclic oligomers: a chain scored against its own C_n copies, and a rigid pose carried relative to the axis.
 * Backbone-only repulsion and a CA contact reward are no force field; whether such assemblies are designable, and what their
 * interfaces are worth, is unmeasured.
 *
 * The symmetry statement, per chain b.  n = order[b]; n == 1: the chain is not symmetric and every output is 0.  The pose
 * (Q, t) is 12 doubles, Q row-major then t (fd_template_energy's transform_out layout); p_a are the fp64 coordinates of the atoms
 * a < 3 lens[b], 3 i + {0 N, 1 CA, 2 C}:
 *     y_a      = Q p_a + t                       the chain in the assembly frame; the axis is z through 0
 *     R_k      = the rotation by 2 pi k / n about z, k = 1 .. n - 1 (cos and sin evaluated in fp64 on the host)
 *     d(a,k,b) = |y_a - R_k y_b|                 ALL ordered atom pairs, a == b included, no |a - b| >= 2 exclusion: other chains
 *     clash:   t_ab = clash_alpha (r_a + r_b) + clash_margin, r = 1.55 for N, 1.7 for CA and C (fd_relax_energy's numbers);
 *              v = max(0, t_ab - d);  phi = w_clash v^2
 *     contact: CA-CA pairs only;  u = clamp((d_off - d) / (d_off - d_on), 0, 1);  s = u^2 (3 - 2 u);  phi = -w_contact s
 *     E_clash  = 1/2 sum_{k,a,b} phi_clash;   E_contact = 1/2 sum_{k,a,b} phi_contact
 *              (per subunit: n (E_clash + E_contact) is the inter-chain energy of the explicit n-mer)
 *     g_a      = sum_{k=1}^{n-1} sum_b phi'(d) (y_a - R_k y_b) / d,  terms with d == 0 dropped.  The 1/2 is gone: the triple
 *              (b, n - k, a) has the same distance and gives y_a the same term.  One lane per atom owns g_a, k ascending and
 *              the partners in index order within k; no atomics.
 *     radial:  c = the mean of the CA y;  rho = sqrt(c_x^2 + c_y^2);  e = max(0, rho - r_max);  E_radial = w_radial e^2;
 *              every CA's g gains 2 w_radial e (c_x, c_y, 0) / (rho lens[b]), nothing where rho == 0
 *     contacts = the number of ordered triples (a CA, k, b CA) with d < d_on, an exact int32
 *     F = sum_a g_a;   tau = sum_a y_a x g_a     (dE/dt, and dE/d(a rotation about the origin applied on the left))
 *     dcoords_a = Q^T g_a
 * F_z and tau_z vanish up to rounding: the energy does not change when the pose turns about z or shifts along it.  Every sum is in
 * an order fixed by (length, order, lane); two calls give the same bits, and a chain's bits do not depend on the batch it is in.
 *
 * fd_symmetry_energy: the statement on host arrays, model-free and synchronous like fd_template_energy.
 *   coords        float64 [B][3L][3] (host), finite on the atoms below 3 lens[b]; lens int32[B] in [1, min(L, 2048)]
 *   order         int32[B], each in [1, 12];  pose double[B][12], every entry finite (Q is taken as given: not re-orthogonalised)
 *   params        clash_alpha, clash_margin, w_clash, w_contact, w_radial, r_max finite and >= 0; 0 <= d_on < d_off, both finite;
 *                 lever, max_shift, step0 > 0 and finite; grow >= 1; shrink in (0, 1); pose_iters >= 0 (read by
 *                 fd_scaffold_guide_step_sym only)
 *   energy_out    double[B][3] clash | contact | radial;  contacts_out int32[B]
 *   wrench_out    double[B][6] F then tau, or NULL
 *   dcoords_out   float64 [B][3L][3], or NULL: written everywhere, 0 where order[b] == 1 and at or beyond 3 lens[b]
 * A bad call: FD_E_INVALID before any device call, the offending word in fd_last_error(), outputs untouched. */
typedef struct fd_symmetry_params {
  double clash_alpha, clash_margin, w_clash, w_contact, d_on, d_off, w_radial, r_max;
  double lever, max_shift, step0, grow, shrink;
  int32_t pose_iters, reserved;
} fd_symmetry_params;
int fd_symmetry_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* order, const double* pose,
                       const fd_symmetry_params* params, double* energy_out, int32_t* contacts_out, double* wrench_out,
                       double* dcoords_out);

/* fd_symmetry_dock: the docking descent, rigid body only -- fd_relax's scheme on the pose, per chain, chains independent, with
 * E = E_clash + E_contact + E_radial and (E, F, tau) the statement's:
 *     h = step_io ? step_io[b] : step0;   (E, F, tau) of the pose;   trace[0] = E
 *     for it = 1 .. n_iter:
 *         w = -h tau / lever^2;   dt = -h F;   m = max(|dt|, lever |w|);   k = m > max_shift ? max_shift / m : 1
 *         Q' = Rot(k w) Q;   t' = Rot(k w) t + k dt        Rodrigues' formula in fp64; F == tau == 0 keeps the pose's bits
 *         (E', F', tau') of the trial
 *         if E' <= E (false for NaN):  the trial becomes the pose, h *= grow, accepted += 1;   else h *= shrink
 *         trace[it] = E
 *     pose_out = the pose;  energy_out, contacts_out = the statement's at it;  step_io[b] = h
 * A chain of order 1 has nothing to descend: its pose, its h and accepted = 0 are returned as given.
 * Nothing is asked of the host between the upload and the download; two launches per evaluation (the energy, then a
 * one-lane-per-chain pose step).  fd_symmetry_dock(n_iter = N) equals N calls with n_iter = 1 chained through pose_out and
 * step_io, bit for bit, and energy_out equals fd_symmetry_energy(pose_out) bit for bit.
 *   n_iter        >= 0; 0 returns the input pose and its energy
 *   step_io       double[B], each finite and > 0, or NULL
 *   pose_out      double[B][12];  energy_out double[B][3];  contacts_out int32[B]
 *   trace_out     double[n_iter + 1][B] or NULL;  accepted_out int32[B]
 * Everything fd_symmetry_energy rejects, n_iter < 0, a step_io entry that is not finite and > 0, a NULL output other than
 * trace_out: FD_E_INVALID before any device call, outputs untouched. */
int fd_symmetry_dock(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* order, const double* pose,
                     const fd_symmetry_params* params, int n_iter, double* step_io, double* pose_out, double* energy_out,
                     int32_t* contacts_out, double* trace_out, int32_t* accepted_out);

/* fd_scaffold_guide_step_sym: fd_scaffold_guide_step_tpl whose statement gains, after the template line, for the chains with
 * sym_order[b] >= 2:
 *     sym_placed_in given:  (Q, t) = the proper rigid fit of coords onto sym_placed_in[b], all atoms below 3 lens[b], unit weights:
 *                           with (R, t_fit) = the template statement's transform for the targets sym_placed_in, Q = R^T, t = -R^T t_fit
 *     sym_placed_in NULL:   (Q, t) = sym_pose_in[b]                                   (the first visit of a run)
 *     pose_iters iterations of the docking descent from (Q, t), h carried in sym_step_io[b] (NULL: step0, not written back;
 *         the entry of a chain of order 1 keeps its value)
 *     E_clash_sym, E_contact, E_radial, contacts at the final pose;   gc += Q^T g
 *     sym_pose_out[b] = (Q, t);   sym_placed_out[b] = Q coords + t
 * The fit re-anchors the pose each visit: NeRF hangs the chain on residue 0, so a torsion change near the N-terminus swings the
 * whole chain in NeRF's frame, and fitting onto where the last visit placed it removes that.  The angle gradient and the pose
 * gradient are exact partial derivatives of one energy (block coordinate descent); no term is differentiated through the fit.
 * Launches: the fit and its turn into a pose (with sym_placed_in), two per evaluation of the descent (1 + pose_iters
 * evaluations), one evaluation at the final pose that writes the gradient, one placement.
 *   tpl_*             as in fd_scaffold_guide_step_tpl, all four may be NULL
 *   sym_order         int32[B] in [1, 12], or NULL.  NULL or all 1: none of these launches run and every output
 *                     fd_scaffold_guide_step_tpl shares equals that entry's bit for bit; with all 1 the energies and contacts are
 *                     0, sym_pose_out = sym_pose_in and sym_placed_out is not written; with NULL no sym_* argument is looked at
 *   sym_pose_in       double[B][12], finite;  sym_placed_in double[B][3L][3] finite on the atoms below 3 lens[b], or NULL
 *   sym_params        as in fd_symmetry_energy;  sym_step_io double[B] finite and > 0, or NULL
 *   sym_energy_out    double[B][3] clash | contact | radial;  sym_contacts_out int32[B];  sym_pose_out double[B][12]
 *   sym_placed_out    double[B][3L][3]: the atoms below 3 lens[b]; the others keep what they held.  A chain with order 1 among
 *                     symmetric ones is placed by its sym_pose_in and scores 0
 * Everything fd_scaffold_guide_step_tpl and fd_symmetry_energy reject, with sym_order given a NULL sym_pose_in, sym_params or
 * sym_*_out: FD_E_INVALID before any device call, outputs untouched. */
int fd_scaffold_guide_step_sym(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                               const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                               const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                               const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                               const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w,
                               const int32_t* sym_order, const double* sym_pose_in, const double* sym_placed_in,
                               const fd_symmetry_params* sym_params, double* sym_step_io, float c, float s, const float* z, uint64_t seed,
                               int t, int64_t seq_offset, float* x_out, double* energy_out, double* max_violation_out, double* gnorm_out,
                               double* dfeats_out, double* tpl_rmsd_out, double* sym_energy_out, int32_t* sym_contacts_out,
                               double* sym_pose_out, double* sym_placed_out);

/* fd_sample_guided_inpaint_sym: fd_sample_guided_inpaint_tpl whose visits are followed by fd_scaffold_guide_step_sym's statement.
 * The first visit takes sym_pose0 as the pose (no fit); every later visit, and the statement on the final state behind the last
 * one, fits onto the placed atoms the statement before it left.  h starts at step0 and is carried; the pose, h and the placed atoms
 * live on the device for the whole run.  The plain sampler's captured step graph is replayed, never captured again; only launches
 * happen between the upload and the download.
 *   tpl_*             as in fd_scaffold_guide_step_sym (all four may be NULL)
 *   sym_order, sym_params   as in fd_scaffold_guide_step_sym;  sym_pose0 double[B][12], finite
 *                     sym_order NULL or all 1: out, energy_out, max_violation_out and tpl_rmsd_out are fd_sample_guided_inpaint_tpl's
 *                     bit for bit (all 1: the symmetry energies and contacts are 0 and sym_pose_out = sym_pose0)
 *   sym_energy_out    double[B][3] clash | contact | radial, sym_contacts_out int32[B], sym_pose_out double[B][12]: the statement
 *                     with p = the FINAL state (its fit and its pose_iters steps included)
 * Everything fd_sample_guided_inpaint_tpl and fd_symmetry_energy reject, with sym_order given a NULL sym_pose0, sym_params or
 * sym_*_out: FD_E_INVALID before any device call, outputs untouched.  Single device; not offered with jumps, the second-order
 * solver, steering or ties. */
int fd_sample_guided_inpaint_sym(fd_model* m, const float* x_init, const int32_t* lens, int B, int L, const int32_t* visits,
                                 int n_visits, const float* coef, const float* noise, const float* known, const uint8_t* fixed,
                                 const float* known_coef, const float* known_noise, uint64_t seed, int64_t seq_offset,
                                 const float* guide, const fd_scaffold_guide_params* params, const int32_t* rst_offsets,
                                 const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol,
                                 const double* rst_w, const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz,
                                 const double* tpl_w, const int32_t* sym_order, const double* sym_pose0,
                                 const fd_symmetry_params* sym_params, float* out, double* energy_out, double* max_violation_out,
                                 double* tpl_rmsd_out, double* sym_energy_out, int32_t* sym_contacts_out, double* sym_pose_out);

/* ---- multi-GPU through the ABI: independent sequences are sharded across the GPUs of a node by the HOST (one
 * model per GPU, each sampling its slice with seq_offset = its first global sequence index; Philox noise is keyed by that
 * index, so results do not depend on the world size) and ONE collective returns the slices: an RCCL all-gather over xGMI.
 * The reference has no multi-GPU sampler (foldingdiff/sampling.py:91 is single-device); the Python package does the same
 * exchange through torch.distributed (foldingdiff_amd/distributed.py).  RCCL is bound at run time (dlopen librccl.so).
 *   fd_comm_unique_id  128 bytes, created by one process and distributed by the host (file, pipe, MPI ...)
 *   fd_comm_init       joins the communicator (collective over all ranks); one communicator per model
 *   fd_gather_dev      out_dev[r * n_floats ...] = rank r's local_dev[0 .. n_floats) for every r; equal counts on every rank
 *                      (pad ragged slices to the largest); stream-ordered on hip_stream (NULL: the model's stream) */
#define FD_COMM_ID_BYTES 128
int fd_comm_unique_id(void* id_out);
int fd_comm_init(fd_model* m, int rank, int world, const void* unique_id);
int fd_gather_dev(fd_model* m, const void* local_dev, int64_t n_floats, void* out_dev, void* hip_stream);
int fd_comm_destroy(fd_model* m);

/* Fill out_dev[n] (device, float32) with the Philox N(0,1) stream used for step
 * t of a [B][L][F] batch -- exposes the perf-mode generator for tests. */
int fd_philox_normal_dev(fd_model* m, uint64_t seed, int t, int64_t seq_offset, int B, int L, void* out_dev,
                         void* hip_stream);

/* ---- post-processing: angles -> backbone coordinates ----
 * Replaces NERFBuilder.cartesian_coords / .centered_cartesian_coords (foldingdiff/nerf.py:78-129,
 * place_dihedral :145-204) as create_new_chain_nerf calls them (foldingdiff/angles_and_coords.py:112-184).
 *   feats     float32 [B][L][F] sampled features (host), lens int32[B] residues per chain
 *   feat_idx  int32[9]: column of phi, psi, omega, N:CA:C ("tau"), CA:C:1N, C:1N:1CA, 0C:1N, N:CA, CA:C;
 *             -1 for an angle / length that is not a feature => the reference's constant
 *             (109, 115, 121 degrees; 1.34, 1.46, 1.54 Angstrom); the three dihedrals are required
 *   center    subtract the mean atom position of each chain (centered_cartesian_coords)
 *   coords_out float64 [B][3*L][3]: N, CA, C of each residue; rows of residues >= lens[b] are 0 */
int fd_nerf(int device_id, const float* feats, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
            int center, double* coords_out);

/* ---- input side: backbone coordinates -> internal coordinates (the inverse of fd_nerf) ----
 * Replaces canonical_distances_and_dihedrals (foldingdiff/angles_and_coords.py:30-109) with every distance and angle
 * (EXHAUSTIVE_DISTS + EXHAUSTIVE_ANGLES), for many chains in one launch.
 *   xyz           float32 [n_res][3][3]: N, CA, C of each residue (host), n_res = sum of chain_lens
 *   chain_offsets int32[n_chains]: first residue of each chain; chains are packed back to back in order
 *                 (chain_offsets[0] = 0, chain_offsets[c + 1] = chain_offsets[c] + chain_lens[c])
 *   chain_lens    int32[n_chains], each >= 1
 *   feats_out     float32 [n_res][9] in the reference's column order 0C:1N, N:CA, CA:C, phi, psi, omega, tau, CA:C:1N,
 *                 C:1N:1CA, computed in fp64.  Index shifts and padding are the reference's: phi of a chain's first residue
 *                 is NaN; on its last residue the three distances are 0 and the six angles NaN; N:CA, CA:C and tau at
 *                 index i are those of residue i + 1. */
int fd_internal_coords(int device_id, const float* xyz, const int32_t* chain_offsets, const int32_t* chain_lens, int n_chains,
                       float* feats_out);

/* Backbone RMSD after optimal superposition, the score of a reconstruction against its source structure (in place of
 * the TM-score of tmalign.run_tmalign that _score_angles computes, foldingdiff/sampling.py:266-284; TM-align is an
 * external binary).  Pair p = atoms offsets[p] .. offsets[p] + lens[p] - 1 of a and of b (host, float64 [n_atoms][3],
 * packed back to back like fd_internal_coords' chains, lens >= 1); rmsd_out float64 [n_pairs] = min over rotations R and
 * translations of sqrt(mean |R a + t - b|^2) (Horn's quaternion method, fp64). */
int fd_superpose_rmsd(int device_id, const double* a, const double* b, const int32_t* offsets, const int32_t* lens, int n_pairs,
                      double* rmsd_out);

/* Longest chain fd_tm_score takes: both traces of a pair sit in one workgroup's LDS (48 B per residue). */
#define FDMI_TM_MAX_LEN 2048

/* TM-score of residue-paired CA traces: what tmalign.run_tmalign gives _score_angles (foldingdiff/sampling.py:266-284)
 * when residue i of one chain corresponds to residue i of the other.  It restates the published seed-and-extend
 * TM-score search (Zhang & Skolnick 2004; DESIGN.md "TM-score" has the exact rules) in fp64 and is not pinned to the
 * TMscore / TMalign binaries; TM-align also searches the residue alignment, so its number is usually the same or higher.
 *   a, b       host float64 [n_res][3] CA traces; pair p = rows offsets[p] .. offsets[p] + lens[p] - 1 of each, packed
 *              back to back like fd_superpose_rmsd's; 1 <= lens[p] <= FDMI_TM_MAX_LEN; finite, |coordinate| <= 1e6
 *   norm_lens  int32 [n_pairs] normalisation lengths Ln >= lens[p], or NULL for Ln = lens[p]
 *   stride     >= 1: seed fragments start every stride residues (1: every start, the published search)
 *   tm_out     float64 [n_pairs]: max over rotations R and translations t found by the search of
 *              (1 / Ln) * sum_i 1 / (1 + (|R a_i + t - b_i| / d0)^2), d0 = 1.24 cbrt(Ln - 15) - 1.8 (0.5 for Ln <= 21)
 *   transform_out  NULL, or float64 [n_pairs][12]: R row-major, then t, with b ~ R a + t at that maximum.
 * Synchronous; the result does not depend on the other pairs of the call. */
int fd_tm_score(int device_id, const double* a, const double* b, const int32_t* offsets, const int32_t* lens,
                const int32_t* norm_lens, int n_pairs, int stride, double* tm_out, double* transform_out);

/* Longest chain fd_annotate_sse takes: the trace and its per-residue state sit in one workgroup's LDS (29 B per residue). */
#define FDMI_SSE_MAX_LEN 2048

/* Secondary structure of CA traces: annotate_sse (biotite) as count_structures_in_pdb uses it
 * (bin/annot_secondary_structures.py:64-105).  It restates the P-SEA algorithm (Labesse et al. 1997; DESIGN.md
 * "Secondary structure (P-SEA)" has the exact rules) in fp64 and is not pinned to biotite.
 *   ca          host float64 [n_res][3] CA traces; chain c = rows offsets[c] .. offsets[c] + lens[c] - 1, packed back to
 *               back like fd_tm_score's; 1 <= lens[c] <= FDMI_SSE_MAX_LEN; finite, |coordinate| <= 1e6
 *   sse_out     int8 [n_res]: 0 coil ('c'), 1 helix ('a'), 2 strand ('b') per residue
 *   counts_out  NULL, or int32 [n_chains][2]: the number of maximal runs of helix and of strand labels per chain
 * Synchronous; the result does not depend on the other chains of the call. */
int fd_annotate_sse(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                    int8_t* sse_out /* [sum lens]: 0 c, 1 a, 2 b */, int32_t* counts_out /* [n_chains][2] or NULL */);

/* Longest chain fd_backbone_oxygens and fd_dssp take: C and O of every residue and the per-residue state of the DSSP passes
 * sit in one workgroup's LDS (54 B per residue). */
#define FDMI_DSSP_MAX_LEN 1024

/* The carbonyl oxygens of N / CA / C backbones: what the reference's bin/add_oxygen_to_backbone.py adds to a generated backbone,
 * every chain of a call in one launch, all of it in fp64.  For a residue i that is not its chain's last,
 * psi = dihedral(N_i, CA_i, C_i, N_{i+1}) and O_i is placed from (N_i, CA_i, C_i) with the CA-C-O angle 2.0992622 rad, the
 * C=O length 1.2359372 A and the torsion psi + pi: trans to the next N, where a carbonyl oxygen sits.  The reference's script
 * passes psi itself, which is the next N's own torsion (DESIGN.md 6t has the measurement).
 *   nca_c       host float64 [n_res][3][3]: N, CA, C of every residue; chain c = residues offsets[c] .. offsets[c] + lens[c] - 1,
 *               packed back to back like fd_annotate_sse's; 1 <= lens[c] <= FDMI_DSSP_MAX_LEN; finite, |coordinate| <= 1e6
 *   reference_torsion  != 0: the torsion is psi, the reference script's literal call
 *   out         float64 [n_res][4][3]: N, CA, C copied, then O; the O of a chain's last residue (it has no psi) is NaN, as the
 *               reference gives it none
 * Synchronous; the result does not depend on the other chains of the call. */
int fd_backbone_oxygens(int device_id, const double* nca_c /* [n_res][3][3] */, const int32_t* offsets, const int32_t* lens,
                        int n_chains, int reference_torsion, double* out /* [n_res][4][3] */);

/* DSSP states of N / CA / C / O backbones (Kabsch & Sander 1983; DESIGN.md 6t has the exact rules) in fp64: the hydrogen of
 * residue j >= 1 at N_j + unit(C_{j-1} - O_{j-1}), the electrostatic energy of every C=O(i) -> H-N(j) without a distance
 * prefilter, per donor the two acceptors of lowest energy below -0.5 kcal/mol, and from those bonds minimal helices (H, G, I),
 * bridges and ladders (B, E), turns (T) and bends (S).  Not built: beta-bulge linking of ladders and sheet labels.  It is not
 * pinned to the mkdssp binary (which also keeps a per-acceptor list and rounds energies to three decimals).
 *   bb          host float64 [n_res][4][3]: N, CA, C, O of every residue, chains packed like fd_backbone_oxygens' (whose output
 *               this is); 1 <= lens[c] <= FDMI_DSSP_MAX_LEN; finite, |coordinate| <= 1e6, except that the coordinates of an O
 *               may be NaN: that residue accepts no bond and the next one has no hydrogen
 *   flags       NULL, or uint8 [n_res]: bit 0 the residue is no donor (proline, or no H), bit 1 it is no acceptor.  A chain's
 *               first residue is never a donor
 *   state_out   int8 [n_res]: 0 '-', 1 'H', 2 'B', 3 'E', 4 'G', 5 'I', 6 'T', 7 'S'
 *   acc_out, energy_out  both NULL, or int32 [n_res][2] and float64 [n_res][2]: per donor the chain-local indices of its kept
 *               acceptors, lowest energy first (-1 where none), and their energies in kcal/mol (0 where none)
 *   counts_out  NULL, or int32 [n_chains][3]: kept hydrogen bonds, maximal runs of 'H', maximal runs of 'E' per chain
 * Synchronous; the result does not depend on the other chains of the call. */
int fd_dssp(int device_id, const double* bb /* [n_res][4][3]: N, CA, C, O */, const uint8_t* flags /* [n_res] or NULL */,
            const int32_t* offsets, const int32_t* lens, int n_chains, int8_t* state_out /* [n_res] */,
            int32_t* acc_out /* [n_res][2] or NULL */, double* energy_out /* [n_res][2] or NULL */,
            int32_t* counts_out /* [n_chains][3] or NULL */);

/* Longest chain fd_tm_align takes: both traces, the search's state and the 2-bit trace-back matrix of the dynamic
 * programme (n1 x n2 / 4 bytes) sit in one workgroup's LDS. */
#define FDMI_ALIGN_MAX_LEN 512

/* TM-score of CA traces whose residues do NOT correspond: the residue alignment and the superposition are searched
 * together, as TM-align does -- what tmalign.run_tmalign computes for tmalign.max_tm_across_refs
 * (bin/tmscore_training.py) and get_pairwise_tmscores (bin/hclust_structures.py).  It restates the published method
 * (Zhang & Skolnick 2005) with two of its five starts (gapless threading; secondary structure from fd_annotate_sse's
 * labels), each refined by dynamic programming with gap-open penalties -0.6 and 0 (DESIGN.md "TM-align-style
 * alignment" has the exact rules), in fp64, and is not pinned to the TMalign binary: the score is a lower bound on the
 * optimum TM-align looks for.
 *   ca, offsets, lens  host float64 [n_res][3] CA traces of n_chains chains packed back to back like
 *              fd_annotate_sse's; 1 <= lens[c] <= FDMI_ALIGN_MAX_LEN; finite, |coordinate| <= 1e6.  Uploaded once.
 *   pair_a, pair_b     int32 [n_pairs] chain indices: pair p aligns chain pair_a[p] (x) to chain pair_b[p] (y)
 *   norm_lens  int32 [n_pairs] normalisation lengths Ln >= min(n1, n2), or NULL for Ln = lens[pair_b[p]] (TM-align's
 *              "normalized by length of Chain_2")
 *   max_iter   >= 1: dynamic-programming refinements per start and gap penalty (TM-align's default is 10)
 *   tm_out     float64 [n_pairs]
 *   transform_out  NULL, or float64 [n_pairs][12]: R row-major, then t, with y ~ R x + t at that score
 *   n_ali_out  NULL, or int32 [n_pairs]: aligned residue pairs
 *   map_offsets, map_out  both NULL, or int64 [n_pairs] and int32 [sum of lens[pair_a[p]]]: map_out[map_offsets[p] + i]
 *              = the residue of y aligned with residue i of x, or -1; map_offsets packed (map_offsets[0] = 0,
 *              map_offsets[p + 1] = map_offsets[p] + lens[pair_a[p]])
 * Synchronous; the result of a pair does not depend on the other pairs of the call. */
int fd_tm_align(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                const int32_t* pair_a, const int32_t* pair_b, const int32_t* norm_lens /* null: lens[pair_b] */,
                int n_pairs, int max_iter, double* tm_out, double* transform_out /* null or [n_pairs][12] */,
                int32_t* n_ali_out /* null ok */, const int64_t* map_offsets, int32_t* map_out /* both null, or
                map_out[map_offsets[p] + i] = j or -1 for i < lens[pair_a[p]] */);

/* The starts of fd_tm_align_ex's search, a bit set.  fd_tm_align searches from the first two. */
#define FDMI_ALIGN_START_THREADING 1u /* the best gapless threading */
#define FDMI_ALIGN_START_SSE 2u       /* a dynamic programme over the P-SEA labels */
#define FDMI_ALIGN_START_SSE_DIST 4u  /* labels plus the distances under start 1's superposition */
#define FDMI_ALIGN_START_LOCAL 8u     /* the best of up to 128 fragment-pair superpositions; chains of >= 12 residues */
#define FDMI_ALIGN_START_FRAGMENT 16u /* threading of the longest stretch without a chain break (CA-CA step >= 4.25 A) */
#define FDMI_ALIGN_STARTS_ALL 31u

/* fd_tm_align from a chosen set of TM-align's five starts (DESIGN.md "TM-align-style alignment" has the exact rules of
 * each; like the first two, the three further ones restate the published method and are not pinned to the TMalign
 * binary).  The first 15 arguments and their checks are fd_tm_align's.
 *   starts        a non-empty set of the FDMI_ALIGN_START_* bits; anything else is FD_E_INVALID.  Every requested start
 *                 that applies to the pair is refined as in fd_tm_align and the best candidate wins, the first on a tie in
 *                 start order: more starts never score lower, and FDMI_ALIGN_START_THREADING | FDMI_ALIGN_START_SSE
 *                 returns bit for bit what fd_tm_align returns.
 *   start_tm_out  NULL, or float64 [n_pairs][5]: the best TM reached from each start, -1 where the start was not
 *                 requested or was skipped (LOCAL below 12 residues, FRAGMENT without a chain break).
 * A pair to which no requested start applies has no candidate: tm_out = -1, the identity transform, n_ali_out = 0 and a
 * map of -1.
 * Synchronous; the result of a pair does not depend on the other pairs of the call. */
int fd_tm_align_ex(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                   const int32_t* pair_a, const int32_t* pair_b, const int32_t* norm_lens /* null: lens[pair_b] */,
                   int n_pairs, int max_iter, double* tm_out, double* transform_out /* null or [n_pairs][12] */,
                   int32_t* n_ali_out /* null ok */, const int64_t* map_offsets, int32_t* map_out /* both null or neither */,
                   uint32_t starts, double* start_tm_out /* null or [n_pairs][5] */);

/* Most atoms of one structure fd_backbone_clashes and fd_lddt take (the per-atom pair counters are 32-bit). */
#define FDMI_PAIRCOUNT_MAX_ATOMS 65536

/* Van der Waals clashes of backbones: count_clashes / count_clashes_parallel (foldingdiff/vdw_clashes.py:34-78), every
 * chain of a call in one launch, one workgroup per chain.  Atoms of a chain in file order: 3i = N (radius 1.55), 3i + 1 =
 * CA and 3i + 2 = C (radius 1.7).  Atoms a and b clash iff |a - b| >= 2 and d(a, b) <= alpha * (r_a + r_b), the distance
 * and the product in fp64 from the float32 coordinates.  Unlike the reference, a neighbouring pair (|a - b| = 1) at
 * distance exactly 0 does not clash (DESIGN.md "Clash counts and lDDT").
 *   xyz           host float32 [n_res][3][3]: N, CA, C of each residue; chains packed back to back like
 *                 fd_internal_coords'; 3 * chain_lens[c] <= FDMI_PAIRCOUNT_MAX_ATOMS; finite, |coordinate| <= 1e6
 *   alpha         > 0 and finite (the reference's default is 0.63)
 *   counts_out    int32 [n_chains]: the atoms of the chain that clash with at least one other atom
 *   flags_out     NULL, or uint8 [3 n_res]: 1 = this atom clashes
 * Synchronous; the result does not depend on the other chains of the call. */
int fd_backbone_clashes(int device_id, const float* xyz, const int32_t* chain_offsets, const int32_t* chain_lens,
                        int n_chains, double alpha, int32_t* counts_out /* [n_chains] */,
                        uint8_t* flags_out /* NULL or [3 n_res]: 1 = this atom clashes */);

/* lDDT of models against references of the same residues: lddt / lddt_sampled_folded (foldingdiff/lddt.py:32-100), which
 * start one OpenStructure container per pair.  It restates Mariani et al. 2013 with the defaults of OpenStructure's
 * compare-structures --lddt (DESIGN.md "Clash counts and lDDT" has the exact rules) and is not pinned to that binary; no
 * stereochemistry checks are made.  Residue i of the model corresponds to residue i of the reference, atoms_per_res atoms
 * per residue in the same order in both.  An unordered pair of atoms of different residues is included iff d_ref <
 * radius, and conserved at threshold tau iff |d_model - d_ref| < tau (fp64 from the float32 coordinates).
 *   model, ref    host float32 [n_res][atoms_per_res][3]; pair p = residues offsets[p] .. offsets[p] + lens[p] - 1 of
 *                 both, packed back to back; 1 <= atoms_per_res <= 8; atoms_per_res * lens[p] <=
 *                 FDMI_PAIRCOUNT_MAX_ATOMS; finite, |coordinate| <= 1e6
 *   radius        > 0 and finite (default 15);  thresholds  float64 [n_thresholds], 1 <= n_thresholds <= 8, each > 0 and
 *                 finite (defaults 0.5, 1, 2, 4)
 *   counts_out    int64 [n_pairs][2]: conserved (summed over the thresholds), total (included pairs); the score is
 *                 conserved / (n_thresholds * total), undefined for total = 0
 *   res_counts_out  NULL, or int32 [n_res][2]: the same two numbers over the included pairs with an atom in the residue
 * Synchronous; the result does not depend on the other pairs of the call. */
int fd_lddt(int device_id, const float* model, const float* ref, const int32_t* offsets, const int32_t* lens, int n_pairs,
            int atoms_per_res, double radius, const double* thresholds, int n_thresholds,
            int64_t* counts_out /* [n_pairs][2]: conserved, total */, int32_t* res_counts_out /* NULL or [n_res][2] */);

/* ---- the denoising loss of a fixed checkpoint (forward only): BertForDiffusion._get_loss_terms / validation_step
 * (foldingdiff/modelling.py:553-604, :720-751) with loss = "smooth_l1", circle_reg = 0 and no pairwise-distance loss; the other
 * settings follow below (fd_loss_terms_ex, fd_pairwise_dist, fd_denoise_loss_ex) ----
 *
 * Per-position terms of pred against target (host float32 [B][L][F]) and their per-sequence sums.  Feature f with
 * is_angle[f] != 0: losses.radian_smooth_l1_loss (losses.py:29-55), d = wrap(target - pred) to [-pi, pi), term =
 * |d| < beta_ang ? 0.5 d^2 / beta_ang : |d| - 0.5 beta_ang (the reference uses beta_ang = pi / 10); other features:
 * F.smooth_l1_loss, the same with the unwrapped d and beta_lin (the reference uses 1).  float32 in the reference's operation
 * order.  1 <= F <= 32, 1 <= lens[b] <= L, both betas > 0.
 *   sums    float64 [B][F]: the sum of the terms over positions l < lens[b], accumulated in fp64 in a fixed order -- the same
 *           bits from run to run and wherever the sequence sits in the batch.  _get_loss_terms' value for feature f is
 *           sum_b sums[b][f] / sum_b lens[b].
 *   terms   NULL, or float32 [B][L][F]: the terms themselves, 0 at positions l >= lens[b]
 * Model-free and synchronous, like fd_nerf. */
int fd_loss_terms(int device_id, const float* pred, const float* target, const int32_t* lens, int B, int L, int F,
                  const uint8_t* is_angle, float beta_ang, float beta_lin, double* sums /* [B][F] */,
                  float* terms /* [B][L][F] or NULL */);

/* Noising, forward and loss of one batch in one call on the model's stream: one upload, one [B][F] download.
 *   x0, noise   host float32 [B][L][F]: the clean features and the N(0,1) draw eps (NoisedAnglesDataset.sample_noise); noise
 *               is also the target of the loss (batch["known_noise"])
 *   t           int32 [B], each in [0, T);  lens int32 [B]
 *   keep, spread  float32 [B]: sqrt_alphas_cumprod[t[b]] and sqrt_one_minus_alphas_cumprod[t[b]].  The device computes
 *               x_t = keep[b] * x0 + spread[b] * noise, wrapped to [-pi, pi) where fd_finalize's is_angle says so, at EVERY
 *               position of the padded length -- the bits of NoisedAnglesDataset.__getitem__ (datasets.py:861-871).
 *               BOTH NULL: x0 is x_t already (batch["corrupted"]) and nothing is noised; noise is still the target.
 *   sums        float64 [B][F] as fd_loss_terms', of pred = model(x_t, t, mask(lens)) against noise; angularity is what
 *               fd_finalize was given
 *   corrupted_out, eps_out  NULL, or float32 [B][L][F]: x_t and the predicted noise */
int fd_denoise_loss(fd_model* m, const float* x0, const float* noise, const int32_t* t, const float* keep, const float* spread,
                    const int32_t* lens, int B, int L, float beta_ang, float beta_lin, double* sums /* [B][F] */,
                    float* corrupted_out /* or NULL */, float* eps_out /* or NULL */);

/* ---- the rest of _get_loss_terms (modelling.py:553-679): loss = "l1", the circle penalty, the pairwise-distance term ----
 *
 * fd_loss_terms with a loss kind and the turn counts of the circle penalty.
 *   kind    0: the smooth-L1 pair, fd_loss_terms' bits.  1: "l1" -- losses.radian_l1_loss (losses.py:12-26) for angular
 *           features: target % 2 pi, pred % 2 pi (torch's remainder: the divisor's sign), d = target - pred,
 *           d = (d + pi) % 2 pi - pi, |d|; F.l1_loss, |target - pred|, for the others.  The betas must be > 0 and are
 *           unused with kind 1.
 *   turns   NULL, or int64 [B][F]: the sum over positions l < lens[b] of trunc(|pred| / pi) (a float32 division) for
 *           angular features, 0 for the others.  radian_smooth_l1_loss's circle penalty (losses.py:57-61) adds
 *           circle_penalty * sum_b turns[b][f] / sum_b lens[b] to feature f's value.
 * Model-free and synchronous, like fd_loss_terms. */
int fd_loss_terms_ex(int device_id, const float* pred, const float* target, const int32_t* lens, int B, int L, int F,
                     const uint8_t* is_angle, int kind, float beta_ang, float beta_lin, double* sums /* [B][F] */,
                     float* terms /* [B][L][F] or NULL */, int64_t* turns /* [B][F] or NULL */);

/* The pairwise-distance term (modelling.py:616-677, losses.pairwise_dist_loss, nerf.nerf_build_batch) of one batch.
 *   angles, corrupted, pred   host float32 [B][L][F]: the clean x_0, x_t and the predicted noise
 *   keep, spread   float32 [B], keep[b] != 0: denoised = (corrupted - spread[b] * pred) / keep[b], float32 in that order,
 *                  not wrapped
 *   coef           NULL (1), or float32 [B], each > 0: the weight of sequence b's pairs
 *   lens           int32 [B], 1 <= lens[b] <= L;  L <= FDMI_PAIRWISE_MAX_LEN
 *   feat_idx       int32 [6]: the columns of phi, psi, omega, tau, CA:C:1N, C:1N:1CA, each in [0, F), no two equal
 * Two chains per sequence, of the clean and of the denoised angles: float32 trigonometry, float64 frames from the float64
 * seed atoms, bond lengths 1.34 / 1.46 / 1.54.  Over the lens[b] (lens[b] - 1) / 2 pairs of the first lens[b] CA atoms:
 * both distances rounded to float32, term = coef[b] * (d_denoised - d_clean)^2 in float32.
 *   sums     float64 [B]: the terms of sequence b summed in fp64 in a fixed order (0 for lens[b] = 1)
 *   pairs    int64 [B]: lens[b] (lens[b] - 1) / 2.  The reference's value is sum_b sums[b] / sum_b pairs[b].
 *   ca_out   NULL, or float64 [B][2][L][3]: the CA traces of the clean ([b][0]) and of the denoised angles, 0 past lens[b]
 * Model-free and synchronous; the result does not depend on the other sequences of the call. */
#define FDMI_PAIRWISE_MAX_LEN 128
int fd_pairwise_dist(int device_id, const float* angles, const float* corrupted, const float* pred, const float* keep,
                     const float* spread, const float* coef, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                     double* sums /* [B] */, int64_t* pairs /* [B] */, double* ca_out /* [B][2][L][3] or NULL */);

/* fd_denoise_loss with the three settings: one upload, the forward with one timestep per sequence, the terms, the turn
 * counts and the pairwise sums where asked for, one small download.
 *   x0          host float32 [B][L][F], the clean features (batch["angles"]), always
 *   corrupted   NULL: the device noises x0 with keep / spread as fd_denoise_loss does;  or float32 [B][L][F], x_t as given
 *   noise, t, lens, beta_ang, beta_lin, sums, corrupted_out, eps_out   as fd_denoise_loss'
 *   keep, spread   float32 [B], both or neither; required with corrupted = NULL and with the pairwise term (keep[b] != 0)
 *   kind, turns    as fd_loss_terms_ex'
 *   pair_sums   NULL (the pairwise term is off), or float64 [B] as fd_pairwise_dist's sums, of the forward's own
 *               prediction; then pairs (int64 [B]) and feat_idx (int32 [6]) are required, coef is optional and L <=
 *               FDMI_PAIRWISE_MAX_LEN
 * With kind 0, turns = NULL and pair_sums = NULL, sums has fd_denoise_loss's bits. */
int fd_denoise_loss_ex(fd_model* m, const float* x0, const float* corrupted, const float* noise, const int32_t* t,
                       const float* keep, const float* spread, const int32_t* lens, int B, int L, int kind, float beta_ang,
                       float beta_lin, const float* coef, const int32_t* feat_idx, double* sums /* [B][F] */,
                       int64_t* turns /* [B][F] or NULL */, double* pair_sums /* [B] or NULL */, int64_t* pairs /* [B] or NULL */,
                       float* corrupted_out /* or NULL */, float* eps_out /* or NULL */);

/* ---- histogram statistics of angle columns: the counts behind custom_metrics.kl_from_empirical / kl_from_dset ----
 *
 * np.histogram of every column of a float32 table against that column's own explicit edges.
 *   values      host float32 [N][F], 1 <= N <= 2^31 - 1, 1 <= F <= 32
 *   edges       host float64 [F][nbins + 1], non-decreasing along a row, no NaN;  1 <= nbins <= FDMI_HIST_MAX_BINS
 *   rows_valid  NULL (every row), or uint8 [N]: rows with 0 are skipped
 *   counts      int64 [F][nbins]: bin i of column f holds edges[f][i] <= x < edges[f][i + 1], the last bin also
 *               x == edges[f][nbins] (numpy's rule); x is widened to float64 first, so every comparison is exact
 *   outside     int64 [F]: the counted rows of column f in no bin (below, above, NaN)
 * Integer results: they do not depend on the run.  Model-free and synchronous. */
#define FDMI_HIST_MAX_BINS 4096
int fd_hist_columns(int device_id, const float* values, int64_t N, int F, const double* edges, int nbins,
                    const uint8_t* rows_valid /* [N] or NULL */, int64_t* counts /* [F][nbins] */, int64_t* outside /* [F] */);

/* The two passes of custom_metrics.kl_from_dset over a list of timesteps, one launch each.  For row r, feature f and
 * timestep t = timesteps[i], two streams:
 *   eps = scale[f] * z, wrapped to [-pi, pi) where is_angle[f] (NoisedAnglesDataset.sample_noise, datasets.py:772-799);
 *   x_t = keep[t] * x0[r][f] + spread[t] * eps, two rounded float32 products and one rounded sum, wrapped where
 *         is_angle[f]: fd_denoise_loss's noising statement (datasets.py:861-871);                          -- stream 0
 *   cmp = a second, independent draw treated like eps: the reference's dset.sample_noise(values).        -- stream 1
 * z is N(0, 1) from Philox4x32-10 as fd_philox_normal_dev draws it with sequence = r + row_offset, position 0, step = t,
 * under seed_eps for eps and seed_cmp for cmp.  With eps_in and cmp_in (float32 [nT][N][F], both or neither) the streams take
 * eps / cmp from there AS GIVEN (scaled and wrapped already) instead: a reference run's recorded draws.
 *   x0          host float32 [N][F], 1 <= N <= 2^31 - 1, 1 <= F <= 32
 *   is_angle    uint8 [F];  scale  float32 [F], finite (angular_variance / nonangular_variance per feature)
 *   keep, spread   float32 [T], finite: sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod
 *   timesteps   int32 [nT], each in [0, T), 1 <= nT <= 65535
 * fd_noise_minmax:  minmax_out  float32 [nT][2][F][2]: per timestep, stream and feature the smallest and largest value.
 * fd_noise_hist:    edges       float64 [nT][F][nbins + 1], rows as fd_hist_columns'; BOTH streams of (i, f) are counted
 *                               against edges[i][f]
 *                   counts      int64 [nT][2][F][nbins], outside int64 [nT][2][F], as fd_hist_columns'.  With edges that
 *                               span fd_noise_minmax's result for the same arguments, outside is 0 and a row of counts
 *                               sums to N: the two passes saw the same streams.
 *                   x_t_out, cmp_out, eps_out   NULL, or float32 [nT][N][F]: stream 0, stream 1 and eps (small N)
 * Integer results and exact min / max: they do not depend on the run.  Model-free and synchronous. */
int fd_noise_minmax(int device_id, const float* x0, int64_t N, int F, const uint8_t* is_angle, const float* scale,
                    const float* keep, const float* spread, int T, const int32_t* timesteps, int nT, uint64_t seed_eps,
                    uint64_t seed_cmp, int64_t row_offset, const float* eps_in /* or NULL */, const float* cmp_in /* or NULL */,
                    float* minmax_out /* [nT][2][F][2] */);
int fd_noise_hist(int device_id, const float* x0, int64_t N, int F, const uint8_t* is_angle, const float* scale,
                  const float* keep, const float* spread, int T, const int32_t* timesteps, int nT, uint64_t seed_eps,
                  uint64_t seed_cmp, int64_t row_offset, const float* eps_in /* or NULL */, const float* cmp_in /* or NULL */,
                  const double* edges /* [nT][F][nbins + 1] */, int nbins, int64_t* counts /* [nT][2][F][nbins] */,
                  int64_t* outside /* [nT][2][F] */, float* x_t_out /* or NULL */, float* cmp_out /* or NULL */,
                  float* eps_out /* or NULL */);

/* ---- test hook ----
 * One token GEMM  C[M,N] = A[M,K] W[N,K]^T + bias (+GELU | +resid) through the production
 * kernels of the given precision (epilogue: 0 bias, 1 bias+GELU, 2 bias+residual).  Host buffers,
 * K % 32 == 0.  Used by tests/ to measure kernel error against fp64 in isolation.
 * FD_PREC_F16X3: epilogue | FD_TEST_GEMM_WHOLE_TILES launches the tile kernel's whole-tiles instantiation (the one a step
 * takes when its tiles fill whole rounds of the workgroups) instead of the row-slice capable one; valid for every shape, same
 * bits.  Ignored by FD_PREC_F32. */
#define FD_TEST_GEMM_WHOLE_TILES 0x100
int fd_test_gemm(int device_id, int precision, int epilogue, const float* A, const float* W, const float* bias,
                 const float* resid, float* C, int M, int N, int K);

/* N2: the post-processing of sampling.sample -- foldingdiff/sampling.py:200-222: cut every item to its length, add the
 * training mean offset (datasets.py get_masked_means), re-wrap the angular features with utils.modulo_with_wrapped_range(., -pi, pi)
 * -- on the device, bit-identical to the reference's float32 numpy arithmetic.  traj_dev: [rows][B][L][F] float32 (the stored states
 * of fd_sample_dev, F = fd_config.n_features); lens_dev: int32 [B]; item_off_dev: int64 [B], element offset of item i's
 * [rows][lens[i]][F] block inside out_dev; offset: HOST float32 [F], or NULL = neither shift nor wrap (what the reference does
 * without an offset).  Angularity is what fd_finalize was given.  Asynchronous on hip_stream (NULL: the model's own stream). */
int fd_shift_trim_dev(fd_model* m, const void* traj_dev, int rows, int B, int L, const void* lens_dev, const void* item_off_dev,
                      const float* offset, void* out_dev, void* hip_stream);

/* Test hook for utils.modulo_with_wrapped_range (foldingdiff/utils.py:87-121): out[i] = the update kernels' own wrap of in[i]
 * (host arrays of n float32).  which: 0 = the FD_PREC_F32 kernels' copy (rowwise.hip), 1 = the default path's (rowwise_img.hip). */
int fd_test_wrap(int device_id, int which, const float* in, int64_t n, float* out);

/* C = LayerNorm(A W^T + bias + resid) * gamma + beta over full rows (HF BertSelfOutput / BertOutput,
 * reached from modelling.py:473-480).  use_fused != 0 asks for the LN-fused GEMM kernel of that precision
 * (FD_E_UNSUPPORTED if the shape has no fused instantiation); 0 runs GEMM(+residual) then the LayerNorm kernel. */
int fd_test_gemm_ln(int device_id, int precision, int use_fused, const float* A, const float* W, const float* bias,
                    const float* resid, const float* gamma, const float* beta, float eps, float* C, int M, int N,
                    int K);

/* Average launch time (ms) of the bias-epilogue token GEMM of the given precision on pseudo-random
 * operands, `reps` back-to-back launches bracketed by hipEvents (kernel micro-benchmark / ablations). */
int fd_test_gemm_time(int device_id, int precision, int M, int N, int K, int reps, double* ms_per_launch);

/* ---- measurement ---- */

/* When n > 0, every n-th reverse step of fd_sample* is launched eagerly with a
 * hipEvent pair around each kernel instead of replaying the graph, and the
 * durations are accumulated per kernel class.  0 disables (default). */
int fd_profile_every(fd_model* m, int n);
int fd_profile_reset(fd_model* m);
/* Number of kernel classes; name / accumulated ms / launch count / algorithmic
 * FLOPs and HBM bytes per launch for class i at the last profiled shape. */
int fd_profile_count(fd_model* m);
int fd_profile_get(fd_model* m, int i, const char** name, double* total_ms, int64_t* launches,
                   double* flops_per_launch, double* bytes_per_launch);

/* Block until all work queued on the model's own stream is done. */
int fd_synchronize(fd_model* m);

/* Failure detection for the asynchronous entry point: FD_E_NONFINITE if any reverse step since the last check
 * predicted a non-finite noise value (the host-buffer entry points check by themselves).  Call after the work
 * has completed (fd_synchronize / the caller's stream sync).  The reference has no such guard: a NaN there
 * silently propagates into the sampled angles (foldingdiff/sampling.py:62-75). */
int fd_check_finite(fd_model* m);

/* Debug / test aid (FD_PREC_F16X3 only): copy an intermediate of the last step back as float32.  `name`: "h", "a",
 * "ctx", "g", "g_head", "h_out" ([rows rounded up to 128][width]) or "q", "k", "v" ([B][H][padded L][32]); scales are
 * those of layer option "debug_layer"; option "debug_stop" = n ends a step after n kernel launches.
 * "grids": 3 floats, the x-grid of the most recent launch of the 16-row fused attention, the 32-row fused attention and the fused
 * feed-forward / layer tail on the current workspace (0: none since the workspace was made); see option "debug_grid".
 * "rowinfo": (sequence, position) of every token row as floats, (-1, -1) for a row that is none ([rows rounded up to 128][2]).
 * "scales": the power-of-two scales fd_finalize chose for layer "debug_layer" (which must name a layer), 21 floats; needs a
 * model finalized with FD_PREC_F16X3 and no workspace:
 *    0..5   s_h, s_q, s_k, s_v, s_a, s_g                  activation images of the layer: input, q, k, v (and context),
 *                                                        attention.output LayerNorm, GELU
 *    6      scale of the layer's output image            (the next layer's s_h; s_hfinal after the last layer)
 *    7, 8   s_hfinal, s_hg                               last hidden state, the head's GELU (the same for every layer)
 *    9..20  wqkv_i, wqk_i, wv_i, wsa16_i, wsa_i, wo_i, wtail_i, wi_i, wd_i, wff_i, wff_scale_dn, demb_s
 *                                                        the layer's weight images; 0 where an image was not uploaded */
int fd_debug_read(fd_model* m, const char* name, float* out, int64_t n_floats);

const char* fd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FDMI_H */
