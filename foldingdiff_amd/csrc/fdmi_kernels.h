// Internal launch interface between the C-ABI host code (api.hip: the model as it runs; api_weights.hip: its weights, packed by
// weight_pack.h; api_run.hip: the entries that run it;
// api_structures.hip: fd_nerf and the structure entries; api_hooks.hip: the fd_test_* hooks) and the gfx950 kernels.  Not installed; include/fdmi.h is the
// public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdmi {

constexpr int kHeadDim = 32;   // head size of the tuned kernels (attention_img.hip, attention_f32.hip); 64 / 96 / 128: attention_gen.hip
constexpr int kMaxFeat = 16;   // F <= 16 (reference feature sets have 3..9)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// ---- epilogues of the token GEMM  C[M,N] = A[M,K] * W[N,K]^T + bias[N] ----
enum GemmEpilogue {
  EPI_BIAS = 0,        // QKV projection
  EPI_BIAS_GELU = 1,   // BertIntermediate / AnglesPredictor.dense1: exact-erf GELU
  EPI_BIAS_RESID = 2   // BertSelfOutput / BertOutput dense: + residual (LayerNorm follows)
};

// fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32).  K % 32 == 0; M, N arbitrary.
void launch_gemm_f32(int epilogue, const float* A, const float* W, const float* bias, const float* resid, float* C,
                     int M, int N, int K, hipStream_t s);

// Fused GEMM + bias + residual + LayerNorm over full rows (N == 384 or 192):
//   C = LN(A * W^T + bias + resid) * gamma + beta.   Returns false if (N) has no instantiation.
bool launch_gemm_f32_ln(const float* A, const float* W, const float* bias, const float* resid, const float* gamma,
                        const float* beta, float eps, float* C, int M, int N, int K, hipStream_t s);

// y[r,:] = LN(x[r,:]) * gamma + beta, rows of length d (d <= 1024), one wave per row.
void launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* y, int rows, int d,
                      hipStream_t s);

// K1: h = LN(x W_in^T + b_in (+ pos_emb[l])) * g + b + time_table[*t_dev]; with t_seq ([B], device) non-null a row of
// sequence b adds time_table[t_seq[b]] instead (one timestep per sequence: the sibling kernels, t_dev is not read)
void launch_embed(const float* x, const float* w_in, const float* b_in, const float* pos_emb /*null unless absolute*/,
                  const float* gamma, const float* beta, float eps, const float* time_table, const int* t_dev,
                  const int* t_seq, float* h, int B, int L, int F, int d, hipStream_t s);

// K4: multi-head self-attention with additive key mask and (optionally) the
// relative_key score term.  qkv: [B*L, 3d] (q | k | v), ctx: [B*L, d].
// dist_emb: [2*maxpos-1, 32] of this layer, or null for absolute positions.
// Returns false when L is beyond what this build tiles (L > 128).
// rkq != 0: relative_key_query (the key term k_r . E[l - r + maxpos - 1] as well)
bool launch_attention_f32(const float* qkv, const float* dist_emb, const int* lens, float* ctx, int B, int L, int H,
                          int maxpos, hipStream_t s, int rkq = 0);

// K8 tail + K9: per token  y = do_ln ? LN(g)*gamma+beta : g ;  eps = y W2^T + b2 ;
//   x' = wrap_if_angle( c1[t] * (x - beta[t]*eps / c3[t]) + (t>0 ? sigma[t]*z : 0) )
// coef: [4][T] (c1, beta, c3, sigma).  t is read from *t_dev.
// z comes from noise[t][...] when noise != null, else Philox(seed, t, element).
// Writes eps_out (if non-null), x_out (may alias x), hist[T_hist_row] (if non-null).
// Per-call values the captured per-step graph must not bake in: they live in a
// small device struct that the host rewrites before each sampling run.
struct UpdateDyn {
  const float* noise;    // [t_start+1, M, F] or null
  float* hist;           // [t_start+1, M, F] or null
  unsigned long long seed;
  long long seq_offset;
  int t_start;
  int hist_every;        // keep every k-th state (and the final one) in `hist`; <= 1: every state
  // motif-conditioned sampling (inpaint_replace.h): all null unless fd_sample_inpaint is running
  const float* known;          // [M, F] values of the fixed elements (model space)
  const unsigned char* fixed;  // [M, F] != 0: the element is replaced after every step instead of updated
  const float* known_noise;    // [t_start+2, M, F] draws of the replacement (row j: level j; a strided run: [K+1, M, F], row i+1 =
                               // the state visit i leaves) or null (Philox, tagged step word)
  const float* known_coef;     // [2, T+1] keep | spread per level
  // strided (few-step) sampling: all null unless fd_sample_strided is running; indexed by the timestep t the kernel holds
  // (a descending schedule visits each t at most once).  `noise` and `hist` rows are then per visit: row ord[t]
  const int* next_t;           // [T] the next visit's t, -1 behind the last visit
  const int* ord;              // [T] the visit's ordinal 0 .. K-1
  const float* abs;            // [3, T] rows a | b | s of the visit:  x' = a x + b eps (+ s z where s != 0)
  // second-order multistep solver (solver_update.h): both null unless fd_sample_solver is running (a strided run with s = 0)
  const float* cuv;            // [3, T] rows c | u | v of the visit, indexed by t like `abs`
  float* x0_prev;              // [M, F] the previous visit's prediction of the clean state, indexed like x (packed rows too)
  // steered sampling (fd_sample_steered): both null otherwise.  A strided visit that is not the solver's then also writes its
  // prediction of the clean state, solver_update.h's x0 = u x + v eps (wrapped where angular); x' is unchanged
  const float* uv;             // [2, T] rows u | v of the visit, indexed by t like `abs`
  float* x0_steer;             // [M, F] the visit's prediction, indexed like x (packed rows too); never set together with cuv
};
// Every pointer member above that a run family sets for one run (`noise` and `hist` are rewritten by every run's opening and
// every step segment): back to null, so that a closed run leaves nothing pointing into its call-lifetime buffers.  A new
// per-run pointer member belongs here.
inline void clear_run_pointers(UpdateDyn* d) {
  d->known = nullptr; d->fixed = nullptr; d->known_noise = nullptr; d->known_coef = nullptr;
  d->next_t = nullptr; d->ord = nullptr; d->abs = nullptr;
  d->cuv = nullptr; d->x0_prev = nullptr;
  d->uv = nullptr; d->x0_steer = nullptr;
}
struct UpdateArgs {
  const UpdateDyn* dyn;  // device pointer; when non-null it overrides noise/hist/seed/seq_offset/t_start
  const float* g;        // [M, d]
  const float* gamma;    // [d] or null
  const float* beta;     // [d] or null
  const float* w2;       // [F, d]
  const float* b2;       // [F]
  const float* x;        // [M, F]
  const float* coef;     // [4, T]
  const float* noise;    // [T, M, F] or null
  long long noise_stride;  // elements between consecutive t rows of `noise` (0: a single [M,F] slab)
  const int* t_dev;      // current step index
  float* eps_out;        // [M, F] or null
  float* x_out;          // [M, F] or null (null => forward only)
  float* hist;           // [(t_start+1), M, F] or null
  unsigned long long seed;
  long long seq_offset;  // global index of sequence 0 (Philox key)
  int t_start;
  int T;
  int M, L, F, d;
  int do_ln;
  float ln_eps;
  unsigned angle_mask;   // bit f set => wrap feature f
  // motif-conditioned sampling without `dyn` (fd_p_sample_step_inpaint); null by default.  known_noise rows are
  // noise_stride apart, like `noise`'s
  const float* known;
  const unsigned char* fixed;
  const float* known_noise;
  const float* known_coef;
  // one strided update by value, without `dyn` (fd_p_sample_step_coef): x' = sa x + sb eps (+ ss z where ss != 0), z = `noise`
  int strided;
  float sa, sb, ss;
  // ... and the level its fixed elements land on (fd_p_sample_step_coef_inpaint; known_noise = the one slab of that level)
  int level_out;
  // one solver update by value, without `dyn` (fd_p_sample_step_solver; x0_out non-null selects it, with `strided` == 1 and
  // ss = 0): solver_update.h with (sa, sb, sc, su, sv); x0_prev [M, F] is read only where sc != 0, x0_out [M, F] receives x0
  float sc, su, sv;
  const float* x0_prev;
  float* x0_out;
  // ... and one strided update by value that also writes the visit's prediction of the clean state (fd_p_sample_step_coef_x0):
  // strided == 2 selects it; (sa, sb, ss) as for strided == 1, x0_out [M, F] = su x + sv eps, wrapped where angular
};
void launch_head_update(const UpdateArgs& a, hipStream_t s);
// The replacement of the start point of a motif-conditioned run (inpaint_replace.h): x[o] = the level-`level` value of
// every element with fixed[o] != 0 (level >= 1); known_noise = the [B][L][F] slab of that level, or null (Philox).
void launch_inpaint_init(float* x, const float* known, const unsigned char* fixed, const float* known_noise,
                         const float* known_coef, int T, int level, unsigned long long seed, long long seq_offset, int B,
                         int L, int F, unsigned angle_mask, hipStream_t s);
// The jump of a resampling schedule (inpaint_jump.hip): x [B][L][F] in place from its level up to `level_to` >= 1 -- fixed
// elements as above (Philox), free ones jk * x + js * z with the draws of the step word 0x40000000 | level_to, both wrapped
// where angular; positions l >= lens[b] are left as they are.
void launch_inpaint_jump(float* x, const int* lens, const float* known, const unsigned char* fixed, const float* known_coef,
                         int T, int level_to, float jk, float js, unsigned long long seed, long long seq_offset, int B, int L,
                         int F, unsigned angle_mask, hipStream_t s);

// N1: NeRF internal -> Cartesian backbone coordinates, one lane per chain, fp64.
// Feature column of each quantity in the [B][L][F] float32 array; -1 => the reference's constant.
struct NerfFeatures {
  int phi, psi, omega;                      // required
  int ang_n_ca_c, ang_ca_c_n, ang_c_n_ca;   // "tau"/"N:CA:C", "CA:C:1N", "C:1N:1CA"
  int len_c_n, len_n_ca, len_ca_c;          // "0C:1N", "N:CA", "CA:C"
};
void launch_nerf(const float* feats, const int* lens, int B, int L, int F, const NerfFeatures& fx, int center,
                 double* out /* [B][3L][3] */, hipStream_t s);

// The inverse of NeRF (internal_coords.hip): float32 N, CA, C coordinates [n_res][3][3] of chains packed back to back
// (chain c = residues offsets[c] .. offsets[c] + lens[c] - 1) -> float32 [n_res][9] canonical features, one lane per residue.
void launch_internal_coords(const float* xyz, const int* offsets, const int* lens, int n_chains, int n_res, float* out,
                            hipStream_t s);
// RMSD after optimal superposition of a[k] onto b[k] for atoms offsets[p] .. offsets[p] + lens[p] - 1 of pair p (fp64
// [n_atoms][3] each), one wave per pair.
void launch_superpose_rmsd(const double* a, const double* b, const int* offsets, const int* lens, int n_pairs, double* rmsd,
                           hipStream_t s);
// TM-score search (tm_score.hip).  tm_chunk_offsets fills chunk_off[n_pairs + 1] (host: pair p's seeds are workgroups
// chunk_off[p] .. chunk_off[p + 1] - 1) and returns the number of workgroups, -1 past INT_MAX.  launch_tm_score: cent =
// [n_pairs][6] centroids of a and b, ws = tm_workspace_bytes(n_chunks), transform_out = [n_pairs][12] (R row-major, t).
int tm_chunk_offsets(const int* lens, int n_pairs, int stride, int* chunk_off);
size_t tm_workspace_bytes(int n_chunks);
hipError_t launch_tm_score(const double* a, const double* b, const double* cent, const int* offsets, const int* lens,
                           const int* norm_lens, const int* chunk_off, int n_pairs, int n_chunks, int stride, int max_len,
                           double* ws, double* tm_out, double* transform_out, hipStream_t s);
// P-SEA secondary structure of CA traces (psea.hip), one workgroup per chain: sse_out [sum lens] (0 coil, 1 helix,
// 2 strand), counts_out [n_chains][2] (runs of helix, runs of strand).  max_len = the longest chain (<= 2048: 29 bytes
// of LDS per residue).
void launch_psea(const double* ca, const int* offsets, const int* lens, int n_chains, int max_len, signed char* sse_out,
                 int* counts_out, hipStream_t s);
// Backbone oxygens (dssp.hip), one workgroup per chain: out [sum lens][4][3] = N, CA, C of nca_c [sum lens][3][3] copied, then O
// (NaN on a chain's last residue); reference_torsion != 0 places O at the next N's torsion instead of trans to it.
void launch_backbone_oxygens(const double* nca_c, const int* offsets, const int* lens, int n_chains, int reference_torsion,
                             double* out, hipStream_t s);
// DSSP states of N / CA / C / O backbones bb [sum lens][4][3] (dssp.hip), one workgroup per chain: state_out [sum lens]
// (0 '-', 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S); acc_out [sum lens][2] and energy_out [sum lens][2] (the kept acceptors of each donor) or
// both null; counts_out [n_chains][3] (kept bonds, runs of H, runs of E) or null; flags [sum lens] (bit 0 no donor, bit 1 no
// acceptor) or null.  max_len = the longest chain (<= 1024: 54 bytes of LDS per residue).
void launch_dssp(const double* bb, const unsigned char* flags, const int* offsets, const int* lens, int n_chains, int max_len,
                 signed char* state_out, int* acc_out, double* energy_out, int* counts_out, hipStream_t s);
// TM-align-style alignment search (tm_align.hip), one workgroup per pair on a persistent grid: pair p = chains pair_a[p],
// pair_b[p] of the packed traces `ca` (cent = [n_chains][3] centroids, sse = launch_psea's labels of the same chains,
// max_len = the longest chain, <= 512).  tm_out [n_pairs], transform_out [n_pairs][12], n_ali_out [n_pairs]; map_out
// (with map_offsets [n_pairs]) or both null.
hipError_t launch_tm_align(const double* ca, const double* cent, const int* offsets, const int* lens, const signed char* sse,
                           const int* pair_a, const int* pair_b, const int* norm_lens, const long long* map_offsets,
                           int n_pairs, int max_iter, int max_len, double* tm_out, double* transform_out, int* n_ali_out,
                           int* map_out, hipStream_t s);
// The same search from the starts of the bit set `starts` (tm_align_starts.hip; 1 threading, 2 secondary structure, 4
// secondary structure plus distance, 8 local superposition, 16 fragment threading); start_tm_out [n_pairs][5] or null: the
// best TM reached from each start, -1 where it was not requested or was skipped.
hipError_t launch_tm_starts(const double* ca, const double* cent, const int* offsets, const int* lens, const signed char* sse,
                            const int* pair_a, const int* pair_b, const int* norm_lens, const long long* map_offsets,
                            int n_pairs, int max_iter, int max_len, unsigned starts, double* tm_out, double* transform_out,
                            int* n_ali_out, int* map_out, double* start_tm_out, hipStream_t s);

// Integer pair counts over all atom pairs of a structure (clash_lddt.hip), one workgroup per structure, float32
// coordinates packed like launch_internal_coords'.  Clashes: xyz [n_res][3][3] -> counts_out [n_chains] (atoms that clash),
// flags_out [3 n_res] or null.  lDDT: model, ref [n_res][A][3], 1 <= A <= 8 -> counts_out [n_pairs][2] (conserved pairs
// summed over the thresholds, included pairs), res_counts_out [n_res][2] or null; the unused places of `thr` hold 0,
// which no pair passes.  At most 65536 atoms per structure (the per-atom counters are 32-bit).
constexpr int kLddtMaxThresholds = 8;
struct LddtThresholds {
  double t[kLddtMaxThresholds];
};
void launch_backbone_clashes(const float* xyz, const int* offsets, const int* lens, int n_chains, double alpha,
                             int* counts_out, unsigned char* flags_out, hipStream_t s);
void launch_lddt(const float* model, const float* ref, const int* offsets, const int* lens, int n_pairs, int atoms_per_res,
                 double radius, const LddtThresholds& thr, long long* counts_out, int* res_counts_out, hipStream_t s);

// ---- steering by particle resampling (steer.hip; the statements are in its header and in include/fdmi.h)
struct SteerOffset {
  int has_offset;              // 0: the values are taken as they are (neither shift nor wrap)
  float offset[kMaxFeat];
};
// ang[b][l][f] = x0 + offset[f], rounded once, wrapped where bit f of angle_mask is set (launch_shift_trim's statement without
// the trim); positions l >= lens[b] get 0
void launch_steer_shift(const float* x0, const int* lens, int B, int L, int F, const SteerOffset& off, unsigned angle_mask,
                        float* ang, hipStream_t s);
// the device buffers of one rewards pass over B particles of padded length L; the caller owns them
struct SteerWork {
  double* coords;              // [B][3L][3] launch_nerf's output
  float* xyz;                  // [B][L][3][3] the same rounded to float32 (launch_backbone_clashes' input)
  double* ca;                  // [B][L][3] the CA atoms (launch_psea's input)
  signed char* sse;            // [B][L] launch_psea's labels
  int* sse_runs;               // [B][2] launch_psea's run counts (not used further)
  int* clashes;                // [B] launch_backbone_clashes' counts
  const int* offsets;          // [B] = b * L: particle b's first residue in xyz / ca / sse
};
struct SteerWeights {
  double w[4];                 // clashes | radius of gyration | helix fraction | strand fraction
};
// terms [B][4] and reward [B] of the backbones of ang [B][L][F] (model features already shifted): launch_nerf (center = 0),
// launch_backbone_clashes and launch_psea as they are, then one wave per particle.  max_len = the longest particle (<= 2048)
void launch_steer_rewards(const float* ang, const int* lens, int B, int L, int F, const NerfFeatures& fx, const SteerWeights& wt,
                          double alpha, int max_len, const SteerWork& wk, double* terms, double* reward, hipStream_t s);
constexpr int kSteerMaxParticles = 1024;
// one workgroup per group of P consecutive particles: the reweighting and the systematic resampling of include/fdmi.h;
// ancestors [G * P] hold global indices, resampled [G] 0 / 1
void launch_steer_resample(const double* reward, double* logw, double* r_prev, int G, int P, double lambda, double ess_frac,
                           const double* u, int* ancestors, unsigned char* resampled, hipStream_t s);
// x_new[b] = x[ancestors[b]], whole [row] blocks (row = L * F floats); x_new must not alias x
void launch_steer_gather(const float* x, const int* ancestors, float* x_new, int B, long long row, hipStream_t s);

// ---- tying the rows of repeat units (repeat_tie.hip; the statement is in its header and in include/fdmi.h).  In place on
// x [B][L][F]; tie int32 [B][3] = start | period | units per sequence, checked by the host: start + period * units <= lens[b].
// init != 0: every copy <- copy 0 and nothing else.  z: the visit's [B][L][F] draws, or null: Philox (seed, t, seq_offset)
void launch_repeat_tie(float* x, const int* lens, const int* tie, int B, int L, int F, unsigned angle_mask, int init, float s,
                       const float* z, unsigned long long seed, int t, long long seq_offset, hipStream_t st);

// ---- the derivative of NeRF and restraint guidance (nerf_vjp.hip; the statements are in its header and in include/fdmi.h).
// One 256-lane workgroup per chain in all three; lens[b] <= kGuideMaxLen and distinct feature columns, checked by the host.
constexpr int kGuideMaxLen = 2048;
// dfeats [B][L][F] fp64 <- the gradient with respect to the NeRF features of a function whose gradient with respect to the
// coordinates [B][3L][3] (launch_nerf's layout) is dcoords; rows at or beyond lens[b] are not written.  feats [B][L][F]: the
// float32 rows the forward built the coordinates from, which give the angle and length slots their signs (sign(sin(angle))
// sign(length) and sign(length); the sign of zero and of a default is +1), or null: every sign +1
void launch_nerf_vjp(const double* coords, const int* lens, int B, int L, int F, const NerfFeatures& fx, int centered,
                     const double* dcoords, const float* feats, double* dfeats, hipStream_t s);
// a batch's distance restraints, packed per chain: chain b owns entries offsets[b] .. offsets[b + 1] - 1
struct Restraints {
  const int* offsets;          // [B + 1]
  const int *i, *j;            // atom indices inside the chain's [0, 3 lens[b])
  const double *d0, *tol, *w;
};
// energy [B], max_violation [B] and, unless null, dcoords [B][3L][3] (atoms at or beyond 3 lens[b]: 0)
void launch_restraint_energy(const double* coords, const int* lens, int B, int L, const Restraints& r, double* energy,
                             double* max_violation, double* dcoords, hipStream_t s);
// the last three lines of the guide statement, in place on x [B][L][F]: gnorm [B] <- |G_b|, x <- x - float32(c k_b G) where
// c != 0, then launch_repeat_tie's + s z and wrap of an untied element
void launch_guide_update(float* x, const double* G, const int* lens, int B, int L, int F, unsigned angle_mask, float c,
                         double max_norm, float s, const float* z, unsigned long long seed, int t, long long seq_offset,
                         double* gnorm, hipStream_t st);

// ---- relaxing backbones in torsion space (nerf_scan.hip, relax.hip; the statements are in their headers and in include/fdmi.h).
// One 256-lane workgroup per chain in all three; lens[b] <= kGuideMaxLen, checked by the host.
// launch_nerf's statement up to the last bits (the frame is composed along the chain, not recomputed from three positions)
void launch_nerf_scan(const float* feats, const int* lens, int B, int L, int F, const NerfFeatures& fx, int center,
                      double* out /* [B][3L][3] */, hipStream_t s);
// energy [B] <- w sum v^2 of the soft clash term on coords [B][3L][3]; its gradient is ADDED to dcoords [B][3L][3], which holds
// launch_restraint_energy's (atoms at or beyond 3 lens[b] are left alone)
void launch_soft_clash(const double* coords, const int* lens, int B, int L, double alpha, double margin, double w, double* energy,
                       double* dcoords, hipStream_t s);
// what the descent keeps of a chain between two launches
struct RelaxState {
  double e[3];                 // clash | restraint | tether of the chain's state
  double e_total, gnorm, h;
  int accepted, pad;
};
// one launch of relax_step_kernel: closes the evaluation of the trial xt (Gt: launch_nerf_vjp's output, rewritten in place with the
// tether's gradient added and what may not move zeroed), then it == 0: the trial becomes the state; it > 0: it does where its
// energy is not above the state's, and h grows or shrinks; !last: xt <- the next trial.  trace [.][B] or null.
struct RelaxStep {
  float* xt;                   // [B][L][F]
  double* Gt;                  // [B][L][F]
  const float* anchor;         // [B][L][F]
  const int* lens;
  const unsigned char* fixed;  // [B][L] or null
  const double *e_clash, *e_rst;  // [B] of the trial
  float* x;                    // [B][L][F] the state
  double* G;                   // [B][L][F] its gradient
  RelaxState* state;           // [B]
  double* trace;
  int L, F, it, last;
  unsigned angle_mask, move_mask;
  double w_tether, grow, shrink, max_step;
};
void launch_relax_step(const RelaxStep& a, int B, hipStream_t s);

// ---- restraint guidance combined with replacement (guide_scaffold.hip; the statement is in its header and in include/fdmi.h).
// One 256-lane workgroup per chain; known / fixed [B][L][F] (fixed: bytes), lens[b] <= kGuideMaxLen, checked by the host.
// ang [B][L][F] <- launch_steer_shift's statement on p = fixed ? known : x0 (x0 is not read where fixed); 0 at or beyond a length
void launch_scaffold_shift(const float* x0, const float* known, const unsigned char* fixed, const int* lens, int B, int L, int F,
                           const SteerOffset& off, unsigned angle_mask, float* ang, hipStream_t s);
// launch_guide_update with a mask: G <- 0 where fixed (in place), gnorm [B] <- |G_b|, and only the free elements move and draw
void launch_scaffold_update(float* x, double* G, const unsigned char* fixed, const int* lens, int B, int L, int F, unsigned angle_mask,
                            float c, double max_norm, float s, const float* z, unsigned long long seed, int t, long long seq_offset,
                            double* gnorm, hipStream_t st);
struct SoftClash {
  double alpha, margin, w;     // launch_soft_clash's; w == 0: no clash launch, alpha and margin unread
};
// ---- superposition restraints (template_fit.hip; the statement is in its header and in include/fdmi.h).  A batch's templates,
// packed per chain: chain b owns entries offsets[b] .. offsets[b + 1] - 1, its atoms strictly increasing inside [0, 3 lens[b])
struct TemplateFit {
  const int* offsets;          // [B + 1]
  const int* atom;             // [n]
  const double* xyz;           // [n][3] the targets
  const double* w;             // [n] > 0
};
// energy [B], rmsd [B] and, unless null, transform [B][12] (R row-major, then t); unless dcoords is null the gradient is ADDED to
// dcoords [B][3L][3] on the named atoms, which holds the terms launched before (a chain without entries: 0, 0, the identity)
void launch_template_energy(const double* coords, int B, int L, const TemplateFit& t, double* energy, double* rmsd,
                            double* transform, double* dcoords, hipStream_t s);

struct ScaffoldWork {
  float* ang;                  // [B][L][F] the shifted rows the structure is built from
  double *coords, *gc;         // [B][3L][3] the structure and the energy's gradient on it
  double *e_rst, *max_violation, *e_clash;  // [B]; e_clash is written only where clash.w > 0
  double *e_tpl, *rmsd_tpl;    // [B]; written only where there is a template
};
// the statement up to G: shift, launch_nerf_scan, launch_restraint_energy, launch_soft_clash (clash.w > 0),
// launch_template_energy (tpl not null) and, unless G is null, launch_nerf_vjp on the shifted rows -> G [B][L][F], unmasked
struct SymGuide;
// sym not null (symmetry.hip): launch_symmetry_guide runs behind the template line, before the derivative
void launch_scaffold_energy(const float* x0, const float* known, const unsigned char* fixed, const int* lens, int B, int L, int F,
                            const SteerOffset& off, unsigned angle_mask, const NerfFeatures& fx, const Restraints& rs,
                            const SoftClash& clash, const TemplateFit* tpl, const ScaffoldWork& wk, double* G, hipStream_t s,
                            const SymGuide* sym = nullptr);

// ---- cyclic oligomers (symmetry.hip; the statements are in its header and in include/fdmi.h).  One 256-lane workgroup per chain
// in the pair and place kernels, one lane per chain in the pose kernel; lens[b] <= kGuideMaxLen, order[b] in [1, kSymMaxOrder].
constexpr int kSymMaxOrder = 12;
// rot [(kSymMaxOrder + 1) * 12][2] <- (cos, sin) of 2 pi k / n at [n * 12 + k], evaluated in fp64 on the host
void symmetry_rotations(double* rot);
struct SymState;
// one evaluation of the symmetry statement with chain b's pose at pose + b * pose_stride (doubles)
struct SymPair {
  const double* coords;        // [B][3L][3] in NeRF's frame
  const int *lens, *order;     // [B]
  const double* pose;          // 12 doubles per chain: Q row-major, then t
  const double* rot;           // symmetry_rotations' table
  double* energy;              // [B][3] clash | contact | radial
  int* contacts;               // [B]
  double* wrench;              // [B][6] F | tau, or null
  double* dcoords;             // [B][3L][3] or null: Q^T g is ADDED on the atoms below 3 lens[b] of the chains with order >= 2
                               // (store != 0: WRITTEN there instead)
  // reuse != null: a chain whose reuse[b].reuse is set is not evaluated again -- its energies and contacts are reuse[b]'s, and
  // spare [B][3L][3], the Q^T g an evaluation at that pose stored, is what is added to dcoords
  const SymState* reuse;
  const double* spare;
  int L, pose_stride, store;
  double clash_alpha, clash_margin, w_clash, w_contact, d_on, d_off, w_radial, r_max;
};
void launch_symmetry_pair(const SymPair& a, int B, hipStream_t s);
// what the docking descent keeps of a chain between two launches
struct SymState {
  double pose[12], trial[12];  // the chain's pose and the pose under evaluation
  double e[3], wrench[6];      // of the chain's pose
  double e_total, h;
  int contacts, accepted;
  int reuse, pad;              // the launch with `last` set took its trial as the pose: that evaluation is the pose's
};
// one launch of symmetry_pose_kernel: closes the evaluation of state[b].trial (e_trial, contacts_trial, wrench_trial: what
// launch_symmetry_pair wrote for it), then it == 0: the trial becomes the pose; it > 0: it does where its energy is not above the
// pose's, and h grows or shrinks; !last: trial <- the next trial.  trace [.][B] or null.
struct SymDock {
  SymState* state;             // [B]
  const int* order;            // [B]: a chain of order 1 keeps h and accepted
  const double* e_trial;       // [B][3]
  const int* contacts_trial;   // [B]
  const double* wrench_trial;  // [B][6]
  double* trace;
  int B, it, last;
  double lever, max_shift, grow, shrink;
};
void launch_symmetry_pose(const SymDock& a, hipStream_t s);
// state[b].trial <- (R^T, -R^T t_fit) of launch_template_energy's transform fit[b] = (R | t_fit), where order[b] >= 2
void launch_symmetry_fit_pose(const double* fit, const int* order, SymState* state, int B, hipStream_t s);
// placed [B][3L][3] <- Q p + t on the atoms below 3 lens[b], by the pair kernel's own expression
// (null: not written), and the same atoms packed at packed + 3 offsets[b] for the chains with offsets[b + 1] > offsets[b] (null: not)
void launch_symmetry_place(const double* coords, const int* lens, int B, int L, const double* pose, int pose_stride, double* placed,
                           const int* offsets, double* packed, hipStream_t s);
// the symmetry lines of the scaffold-guide statement on coords [B][3L][3], every buffer on the device:
//   fit.xyz (the placed coordinates of the visit before, with fit's all-atom lists) not null: state[b].trial <- the pose of the
//   proper rigid fit of coords onto them (launch_template_energy as it is, then launch_symmetry_fit_pose); null: state[b].trial
//   is the caller's;  1 + pose_iters evaluations of the descent (it = 0 takes the trial as the pose) with h = state[b].h, the
//   last of which stores its Q^T g in g_spare;  one more launch that writes energy / contacts at the final pose and ADDS Q^T g
//   to gc (null: no gradient) -- from g_spare and the state where the descent's last trial became the pose, by an evaluation of
//   its own only for the chains whose last trial was dropped;  placed <- Q coords + t
struct SymGuide {
  SymPair pair;                // coords, lens, order, rot, L and the scalars; pose, energy, contacts, wrench, dcoords are set here
  SymDock dock;                // state, B and the scalars; the trial buffers are set here
  TemplateFit fit;             // offsets [B + 1] = 3 lens summed over the chains with order >= 2, atom = 0 .. 3 lens - 1, w = 1
  double *fit_energy, *fit_rmsd, *fit_transform;  // [B], [B], [B][12] workspaces
  double *e_trial, *wrench_trial;                 // [B][3], [B][6] workspaces
  double* g_spare;                                // [B][3L][3] workspace
  int* contacts_trial;                            // [B]
  int pose_iters;
  double* energy;              // [B][3] at the final pose
  int* contacts;               // [B]
  double* placed;              // [B][3L][3], or null
  double* placed_packed;       // null, or the same atoms packed by fit.offsets: the next visit's fit targets
};
void launch_symmetry_guide(const SymGuide& g, double* gc, hipStream_t s);

// *t_dev -= 1, or with a strided run open in `dyn` *t_dev = dyn->next_t[*t_dev]  (last node of the per-step graph)
void launch_step_advance(int* t_dev, const UpdateDyn* dyn, hipStream_t s);

// out[i] = Philox normal for (seed, t, element i of [B][L][F] with seq_offset)
void launch_philox_fill(float* out, unsigned long long seed, int t, long long seq_offset, int B, int L, int F,
                        hipStream_t s);

// ================================================================== row-image path (FD_PREC_F16X3)
// Activations live in HBM as fp16 hi|lo row images (img_common.h); see gemm_img.hip / attention_img.hip /
// rowwise_img.hip.  Token rows: sequences start at multiples of 8 rows; `rowinfo[row]` = (sequence, position)
// or (-1, -1) for padding rows; `dims` (device) = {rows, rows rounded up to 128}.  Every kernel is persistent /
// grid-stride and reads the row counts from `dims`, so a captured graph serves any lengths of one (B, L).
enum GemmImgEpilogue {
  EPI_IMG_GELU = 0, EPI_IMG_LN = 1, EPI_IMG_QK = 2, EPI_IMG_VT = 3, EPI_IMG_BIAS = 4 /* plain bias: test hook */,
  EPI_IMG_QKV = 5  // q | k | v in ONE launch (N = 3 d_model; needs n_heads % 6 == 0 so that v starts on a 384-column tile):
                   // column tiles below 2 d_model take the EPI_QK path, the others the EPI_VT path (stamps share EPI_QK's slot)
};

struct GemmImgArgs {
  const unsigned char* A;      // activation image [rows128][K/32][128 B]
  const unsigned char* W;      // weight image [N rounded up to 384][K/32][128 B] (zero padded)
  const float* bias;           // [N]
  const float* gamma;          // [N]   EPI_IMG_LN
  const float* beta;           // [N]   EPI_IMG_LN
  const unsigned char* resid;  // image [rows128][N/32]   EPI_IMG_LN
  unsigned char* out;          // image [rows128][N/32]   EPI_IMG_GELU / EPI_IMG_LN
  float* out_f32;              // EPI_IMG_BIAS only: when non-null the result (+ residual if `resid`) leaves as fp32 [rows128][N]
  unsigned char* qbuf;         // [B][H][LTOT][128 B]     EPI_IMG_QK
  unsigned char* kbuf;         // [B][H][LTOT][128 B]     EPI_IMG_QK (unit u of row l at u ^ ((l >> 1) & 7))
  unsigned char* vbuf;         // [B][H][LTOT / 32][32 d][128 B]  EPI_IMG_VT (V transposed, swizzled: gemm_img.hip)
  unsigned char* trash;        // >= 256 B scratch line for the stores of padding rows
  unsigned qkv_bytes;          // size of each of qbuf / kbuf / vbuf (< 4 GiB: the q | k | v epilogues address them with 32-bit offsets)
  const int2* rowinfo;
  const int* dims;
  int N, K;                    // valid output columns (multiple of 32), reduction length (multiple of 32)
  int H, LPK, LTOT, NKT;       // heads; keys per key tile; NKT * LPK; key tiles
  float acc_scale;             // 1 / (scale of A * scale of W)
  float out_scale;             // scale of the output image (GELU / LN)
  float resid_inv;             // 1 / scale of the residual image
  float eps;                   // LayerNorm eps
  float q_scale, k_scale, v_scale;
  unsigned long long* stamps;  // null, or [5 epilogues][8 waves][64 slots][6] cycle stamps of workgroup 0 (debug)
  int tail;                    // 1: the rows may not fill whole rounds of tiles -> the slice-capable instantiation (gemm_img.hip); 0: they do
};
// max_rows bounds the grid (B * ceil8(L) of the workspace); the kernel reads the actual count from p.dims.
void launch_gemm_img(int epilogue, const GemmImgArgs& p, int max_rows, hipStream_t s);
int gemm_img_grid(int max_rows, int N);
// weight-stationary variant (gemm_ws.hip): K = 384, GELU / bias epilogue
bool gemm_ws_supported(int epilogue, const GemmImgArgs& p);
void launch_gemm_ws(int epilogue, const GemmImgArgs& p, hipStream_t s);
// few-rows LayerNorm GEMM (gemm_ln_rows.hip): N = 384, K = 384 / 768, one workgroup per 32-row group
bool gemm_ln_rows_supported(const GemmImgArgs& p);
void launch_gemm_ln_rows(const GemmImgArgs& p, int max_rows, hipStream_t s);

struct AttnImgArgs {
  const unsigned char* qbuf;
  const unsigned char* kbuf;
  const unsigned char* vbuf;
  const u32x4_t* demb;         // distance table image [2 maxpos - 1][128 B], or null (absolute positions)
  const int* lens;             // [B] unmasked keys per sequence
  const int* nrow;             // [B] positions that are rows at all (L, or lens[b] when packed)
  const int* seq_row0;         // [B + 1] first token row of each sequence
  unsigned char* ctx;          // image [rows128][H][128 B]
  unsigned char* trash;
  int B, H, LTOT, NKT, maxpos;
  float q_scale, k_scale, v_scale, ctx_scale;
  float r_scale;               // k_scale / scale of the distance table
  float r_scale_k;             // q_scale / scale of the distance table (relative_key_query: the key term)
  int rkq;                     // position_embedding_type == relative_key_query
  const unsigned char* kmask;  // attention_gen.hip only: [B][L] 1 = attend, 0 = masked key (any pattern), or null: keys >= lens[b] are masked
  int L;                       // row stride of kmask
  unsigned long long* stamps;  // null, or [4 waves][64 slots][8] cycle stamps of workgroup 0 (debug)
};
bool launch_attention_img(const AttnImgArgs& p, int L, hipStream_t s);
// head sizes 32 * nb, nb = 1 .. 4 (attention_gen.hip; nb = 1 only for arbitrary key masks, which the tuned kernel does not take): p.H = heads; qbuf / kbuf / vbuf / ctx / demb are indexed by 32-column sub-head
bool launch_attention_gen(const AttnImgArgs& p, int nb, hipStream_t s);

// seq_attn.hip: BertSelfAttention's q | k | v projection AND the attention of a whole sequence in ONE kernel (L <= 128, head size 32,
// relative_key, maxpos <= 128): q, k and v never reach HBM.  One 4-wave workgroup per sequence; the hidden state stays in registers.
struct SeqAttnArgs {
  const unsigned char* himg;   // hidden-state image [rows128][d/32] (grouped, img_common.h)
  unsigned himg_bytes;         // its size (< 4 GiB: 32-bit lane offsets; rows beyond it read as zeros)
  const unsigned char* wimg;   // weight image [head][k-tile][unit 0-7][96 rows: q_h | k_h | v_h][16 B] at the scale of wqkv_i (weight_pack.h: pack_seq_attn)
  const float* bias;           // [3 d]: q | k | v
  const u32x4_t* demb;         // distance table image [2 maxpos - 1][128 B]
  const int* lens;             // [B] unmasked keys per sequence
  const int* nrow;             // [B] positions that are rows at all
  const int* seq_row0;         // [B + 1] first token row of each sequence
  unsigned char* ctx;          // image [rows128][H][128 B]
  int B, H, maxpos;
  float acc_scale;             // 1 / (scale of himg * scale of wimg)
  float q_scale, k_scale, v_scale, ctx_scale;
  float r_scale;               // k_scale / scale of the distance table
  unsigned long long* stamps;  // null, or [4 waves][64 slots][16] cycle stamps of workgroup 0 (debug)
};
bool seq_attn_supported(int d_model, int n_heads, int L, int maxpos);
// grid_cap > 0: at most that many workgroups (launch_common.h persistent_grid; option "debug_grid"); *grid_used: the x-grid launched
bool launch_seq_attn(const SeqAttnArgs& p, hipStream_t s, int grid_cap = 0, int* grid_used = nullptr);   // false: the LDS opt-in or the launch was refused
// seq_attn16.hip (round 6): the same operation with 16-row waves, two per SIMD (v_mfma_f32_16x16x32_f16); wimg = [head][k32 step][tile]
// [unit][row][16 B] (weight_pack.h: pack_seq_attn16); any L <= 128, padded or packed rows.  false: the launch failed.
bool seq_attn16_supported(int d_model, int n_heads, int L, int maxpos);
bool launch_seq_attn16(const SeqAttnArgs& p, hipStream_t s, int grid_cap = 0, int* grid_used = nullptr);

// ffn16.hip (round 6): BertIntermediate + GELU + BertOutput (dense + residual + LayerNorm) of 128 token rows per pass in ONE kernel;
// the intermediate never reaches HBM.  wimg = ONE stream of 16 KiB stages in consumption order (weight_pack.h: pack_ffn16).
struct FfnArgs {
  const unsigned char* aimg;   // input image [rows128][d/32] (BertSelfOutput's LayerNorm output): operand AND residual
  unsigned a_bytes;            // its size (rows beyond it read as zeros)
  const unsigned char* wimg;   // weight stream
  const float* bi;             // [2 d]  intermediate.dense.bias
  const float* bd;             // [d]    output.dense.bias
  const float* gamma;          // [d]    output.LayerNorm
  const float* beta;
  unsigned char* out;          // output image [rows128][d/32] (must not alias aimg)
  unsigned out_bytes;          // its size (stores beyond it are dropped)
  int panels;                  // passes of 128 rows (upper bound)
  const int* dims;             // null, or device {rows, rows rounded up to 128}: passes beyond them are skipped
  float up_scale;              // 1 / (scale of aimg * scale of the first dense's weights)
  float g_scale;               // scale of the intermediate's hi / lo images (a power of two)
  float down_scale;            // 1 / (g_scale * scale of the second dense's weights)
  float resid_inv;             // 1 / scale of aimg
  float out_scale;             // scale of the output image
  float eps;
  // the layer's tail in one launch: cimg != null -> BertSelfOutput (attention.output.dense + residual + LayerNorm) runs in front, on the
  // attention context; aimg is then unused (its rows never reach HBM) and wimg starts with attention.output.dense's stages
  const unsigned char* cimg;   // attention context image [rows128][d/32], a_bytes long
  const unsigned char* hres;   // the layer's input rows (residual of BertSelfOutput), a_bytes long; may alias out (a row is read, then written, by one wave)
  const float* bo;             // [d]  attention.output.dense.bias
  const float* g1;             // [d]  attention.output.LayerNorm
  const float* b1;
  float ao_scale;              // 1 / (scale of cimg * scale of attention.output.dense's weights)
  float hres_inv;              // 1 / scale of hres
  float a_scale;               // scale of BertSelfOutput's output images (= 1 / resid_inv)
  float eps1;
  unsigned long long* stamps;  // null, or [8 waves][16 passes][16] cycle stamps of workgroup 0 (debug)
};
bool ffn16_supported(int d_model, int d_ff);
bool launch_ffn16(const FfnArgs& p, int d_model, hipStream_t s, int grid_cap = 0, int* grid_used = nullptr);   // false: the launch failed (grid_cap, grid_used: as launch_seq_attn)

struct EmbedImgArgs {
  const float* x;              // [B][L][F]
  const float* w_in; const float* b_in; const float* pos_emb; const float* gamma; const float* beta;
  const float* time_table;
  int* tslot;                  // [0]: step index of this step (host / head_update_img write it), [1]: copy for the step's other kernels
  const int2* rowinfo; const int* nrow; const int* dims;
  const int* pos_ids;          // [B][L] position ids of the absolute position embedding, or null = 0 .. L-1 (modelling.py:434-442)
  unsigned char* h;            // image [rows128][d/32]
  int L, F, d;
  float eps, out_scale;
};
// t_seq: null, or [B] (device) one timestep per sequence -- the sibling kernel, which reads neither tslot nor writes it
// ar (needs t_seq): the autoregressive baseline's order -- the row time_table[t_seq[b]] goes in BEFORE the position embedding and
// the LayerNorm and nothing behind it (BertForAutoregressiveBase.forward); pos_ids is not read
void launch_embed_img(const EmbedImgArgs& a, const int* t_seq, int max_rows, hipStream_t s, bool ar = false);
// fd_ar_sample, one launch per step: x[b][copy_pos] = eps[b][copy_pos] for every sequence (copy_pos < 0: no copy), then the row
// table of a step in which every sequence has rows_next token rows and rows_next - 1 unmasked keys (rows_next <= 0: no table).
// cap = the workspace's row capacity, B * ceil8(rows_next) <= cap
void launch_ar_step(float* x, const float* eps, int B, int L, int F, int copy_pos, int rows_next, int cap, int* lens, int* nrow,
                    int* seq_row0, int2* rowinfo, int* dims, hipStream_t s);

struct HeadImgArgs {
  const unsigned char* g;      // image [rows128][d/32]: head activation (mlp decoder) or final hidden state (linear)
  float g_inv;                 // 1 / its scale
  const int2* rowinfo; const int* nrow; const int* dims;
  int* tslot;
  int* flag;                   // bit 0 set when a non-finite prediction was seen
  int advance;                 // write tslot[0] = t - 1 at the end (the sampling loop)
};
// UpdateArgs: M = B * L (elements of one state / F), x / eps / noise / hist in the [B][L][F] layout.
void launch_head_update_img(const UpdateArgs& a, const HeadImgArgs& ia, int max_rows, hipStream_t s);

// y = LayerNorm(fp32 rows [rows128][d]) -> image (d_model > 384: the un-fused BertSelfOutput / BertOutput LayerNorm)
void launch_ln_f32_img(const float* src, const float* gamma, const float* beta, float eps, const int* dims, void* out, int d,
                       float out_scale, int max_rows, hipStream_t s);

// N2: the post-processing of sampling.sample (foldingdiff/sampling.py:200-222) on the device: per item the first lens[i]
// positions of every stored state, shifted by the training mean offset and re-wrapped where the feature is an angle, packed into
// one ragged buffer: item i's [rows][lens[i]][F] block starts at element item_off[i].
struct ShiftTrimArgs {
  const float* traj;           // [rows][B][L][F]
  const int* lens;             // [B]
  const long long* item_off;   // [B]
  float* out;                  // ragged
  int rows, B, L, F;
  unsigned angle_mask;         // bit f: feature f is wrapped to [-pi, pi) after the shift
  int has_offset;              // 0: neither shift nor wrap (the reference only wraps inside `if offset is not None`)
  float offset[kMaxFeat];
};
void launch_shift_trim(const ShiftTrimArgs& a, hipStream_t s);
// test hook: out[i] = wrap_pi(in[i]) through the update kernels' own device function (which: 0 rowwise.hip, 1 rowwise_img.hip)
void launch_wrap_test_f32(const float* in, float* out, long long n, hipStream_t s);
void launch_wrap_test_img(const float* in, float* out, long long n, hipStream_t s);

// ---- forward noising and the denoising loss (loss.hip)
// x_t[b][l][f] = wrap?(keep[b] * x0 + spread[b] * eps), each product and the sum rounded once (datasets.py:861-871): the bits
// of the host's float32 statement; features of angle_mask are wrapped to [-pi, pi).  Every position of the padded length
// is noised, as NoisedAnglesDataset.__getitem__ does.
void launch_q_sample(const float* x0, const float* eps, const float* keep, const float* spread, float* x_t, int B, int L, int F,
                     unsigned angle_mask, hipStream_t s);
// per-position smooth-L1 terms of pred against target (losses.py:29-55 for features of angle_mask, with beta_ang;
// F.smooth_l1_loss with beta_lin for the others) over positions l < lens[b], one workgroup per sequence:
// sums[b][f] (fp64, fixed summation order) and, when non-null, terms[b][l][f] (zeros at l >= lens[b]).  F <= 32.
void launch_loss_terms(const float* pred, const float* target, const int* lens, int B, int L, int F, unsigned angle_mask,
                       float beta_ang, float beta_lin, double* sums, float* terms, hipStream_t s);

// ---- the rest of _get_loss_terms (loss_variants.hip)
// launch_loss_terms with a loss kind (0: the smooth-L1 pair, 1: "l1" -- losses.radian_l1_loss, losses.py:12-26, for the
// features of angle_mask and F.l1_loss for the others; the betas are then unused) and, when non-null, turns[b][f] = the
// sum over l < lens[b] of trunc(|pred| / pi) for the features of angle_mask, 0 for the others (losses.py:57-61).
// kind 0 gives launch_loss_terms' bits.
void launch_loss_terms_ex(const float* pred, const float* target, const int* lens, int B, int L, int F, unsigned angle_mask,
                          int kind, float beta_ang, float beta_lin, double* sums, float* terms, long long* turns,
                          hipStream_t s);
// The pairwise-distance term (modelling.py:616-677), one workgroup per sequence, L <= kPairwiseMaxLen: sums[b] = the fp64
// sum over the lens[b] (lens[b] - 1) / 2 CA pairs of coef[b] * (d_denoised - d_clean)^2 (float32 terms; coef null: 1),
// pairs[b] = their number, ca_out (or null) [B][2][L][3] the CA traces of the clean and of the denoised angles.
constexpr int kPairwiseMaxLen = 128;
struct PairwiseFeatures {
  int phi, psi, omega, tau, ang_ca_c_n, ang_c_n_ca;   // columns of "phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"
};
void launch_pairwise_dist(const float* angles, const float* corrupted, const float* pred, const float* keep, const float* spread,
                          const float* coef, const int* lens, int B, int L, int F, const PairwiseFeatures& fx, double* sums,
                          long long* pairs, double* ca_out, hipStream_t s);

// ---- histogram statistics of angle columns (angle_stats.hip; the rules are in its header)
// counts[F][nbins] / outside[F] += np.histogram of column f of values[N][F] (rows with rows_valid[r] == 0 skipped when
// rows_valid is non-null) against edges[f][0..nbins]; the totals must be zero before the launch.  F <= 32, nbins <= 4096.
void launch_hist_columns(const float* values, long long N, int F, const double* edges, int nbins,
                         const unsigned char* rows_valid, unsigned long long* counts, unsigned long long* outside,
                         hipStream_t s);
// features a workgroup of launch_noise_* holds in LDS at this nbins: 4, 2 or 1
int noise_features_per_group(int nbins);
struct NoiseArgs {
  const float* x0;         // [N][F]
  const float* scale;      // [F]: the variance scale of the draws
  const float* keep;       // [T] sqrt_alphas_cumprod
  const float* spread;     // [T] sqrt_one_minus_alphas_cumprod
  const int* timesteps;    // [nT], each in [0, T)
  const float* eps_in;     // [nT][N][F], the noising draws as given (already scaled and wrapped), or null: Philox
  const float* cmp_in;     // the same for the comparison draws; null exactly when eps_in is
  long long N, row_offset; // Philox sequence of row r = r + row_offset
  int F, G;                // G = noise_features_per_group(nbins) (the min / max pass holds nothing in LDS: 4)
  unsigned angle_mask;
  unsigned long long seed_eps, seed_cmp;
};
// pass 1: mins / maxs [nT][2][F] as order-preserving keys (host: memset to 0xff / 0 before, decode after), [.][0] of x_t,
// [.][1] of the comparison draw
void launch_noise_minmax(const NoiseArgs& a, int nT, unsigned* mins, unsigned* maxs, hipStream_t s);
// pass 2: counts[nT][2][F][nbins] / outside[nT][2][F] += the histograms of the same two streams against
// edges[nT][F][nbins + 1]; x_t_out / cmp_out / eps_out: null, or [nT][N][F]
void launch_noise_hist(const NoiseArgs& a, int nT, const double* edges, int nbins, unsigned long long* counts,
                       unsigned long long* outside, float* x_t_out, float* cmp_out, float* eps_out, hipStream_t s);

void launch_build_rows(const int* lens, int B, int L, int packed, int cap, int* seq_row0, int* nrow, int2* rowinfo,
                       int* dims, hipStream_t s);
// fp32 [src_rows][K] -> image [rows][K/32] (rows >= src_rows are zero rows), value * scale = hi + lo; and back
void launch_f32_to_img(const float* src, void* dst, long long rows, int K, long long src_rows, float scale, hipStream_t s);
void launch_img_to_f32(const void* src, float* dst, long long rows, int K, float scale, hipStream_t s);
// debug: q / k rows or v^T blocks -> fp32 [BH][LTOT][32]
void launch_qkv_unpack(const void* src, float* dst, long long BH, int LTOT, int LP, int rowbytes, int is_vt, float scale,
                       hipStream_t s);

}  // namespace fdmi
