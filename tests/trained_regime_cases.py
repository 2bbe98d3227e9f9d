"""
A trained model's regime for the parity tests: weights, conditions and the operand-rounding restatement (no GPU needed).

oracle.ref_model.synthetic_model gives N(0, 0.02) matrices: |score| <= 1.1, attention almost uniform, GELU close to linear.  Every
exponential, online-softmax rescale, probability split and GELU tail of the kernels then sees one regime only, and a score computed
as plain fp16 x fp16 (a lost lo plane of q, k or of the distance table) moves the model output by less than FWD_TOL.  No trained
weights exist offline, so `trained_gains` multiplies the parameters that feed the scores and the feed-forward
pre-activations by powers of two (exact in every format, the model stays exactly as well conditioned per operation) until

  moderate:  row-maximum probabilities around 0.5 with both tails populated, logit ranges of tens (a trained model's range),
  sharp:     most rows put > 0.9 of their mass on one key, logit ranges of about a hundred, GELU saturated on both sides.

The conditions are asserted on the fp64 oracle by tests/test_trained_regime.py; tests/test_trained_regime_gpu.py runs the kernels
there with the project's own criterion (_rel_gate).  GAINS below were chosen on the CPU by those conditions alone.
"""
import math
import types

import numpy as np
import torch

from oracle import ref_model, ref_sampling

REGIMES = ("moderate", "sharp")

# name: (architecture, {regime: (gq, gk, gd, gi)}).  gd is inert where the model has no distance table (absolute positions).
MODELS = {
    # the two models of every launch plan (_RECIPE_MODELS of tests/test_gpu_parity.py)
    "d384": (dict(hidden=384, heads=12, ff=768, layers=3, pos="relative_key", maxpos=128),
             dict(moderate=(8, 8, 8, 4), sharp=(16, 16, 16, 8))),
    "d192": (dict(hidden=192, heads=6, ff=384, layers=6, pos="relative_key", maxpos=128),
             dict(moderate=(16, 8, 8, 4), sharp=(32, 16, 16, 8))),
    # where no fused attention runs
    "rkq384": (dict(hidden=384, heads=12, ff=768, layers=3, pos="relative_key_query", maxpos=128),
               dict(moderate=(8, 8, 8, 4), sharp=(16, 16, 16, 8))),
    "long384": (dict(hidden=384, heads=12, ff=768, layers=3, pos="relative_key", maxpos=256),
                dict(moderate=(8, 8, 64, 4), sharp=(16, 16, 16, 8))),
    "abs192": (dict(hidden=192, heads=6, ff=384, layers=6, pos="absolute", maxpos=128),
               dict(moderate=(16, 8, 1, 4), sharp=(32, 16, 1, 8))),
    "head64": (dict(hidden=128, heads=2, ff=256, layers=2, pos="relative_key", maxpos=128),
               dict(moderate=(16, 16, 8, 4), sharp=(32, 32, 16, 16))),
    "f32_192": (dict(hidden=192, heads=6, ff=384, layers=6, pos="relative_key", maxpos=128),
                dict(moderate=(16, 8, 8, 4), sharp=(32, 16, 16, 8))),
}

SHAPES_A = ((5, 128, [128, 128, 77, 50, 1]), (7, 101, [101, 50, 99, 100, 64, 3, 77]), (3, 7, [7, 1, 3]))   # _RECIPE_SHAPES
SHAPES = {
    "d384": SHAPES_A,
    "d192": SHAPES_A + ((7, 128, [128, 1, 100, 33, 128, 64, 65]),),   # the last: later items of the persistent kernels
    "rkq384": ((5, 128, [128, 128, 77, 50, 1]),),
    "long384": ((3, 200, [200, 77, 150]),),
    "abs192": ((5, 128, [128, 128, 77, 50, 1]),),
    "head64": ((3, 70, [70, 64, 5]),),
    "f32_192": ((5, 128, [128, 128, 77, 50, 1]), (3, 33, [33, 1, 32])),
}
# The conditions are asserted at the shapes whose longest sequence has at least this many keys and recorded below it: a row of 7
# keys sits higher on the probability conditions and lower on the range conditions whatever the weights.
ASSERT_FROM_L = 64
SEED = 3      # synthetic_model's seed, as _recipe_pair's
T_STATS = 42  # the timestep of the measured tables


def trained_gains(sd, layers, gq, gk, gd, gi):
    """A copy of state dict `sd` with, per layer, attention.self.query x gq, attention.self.key x gk (weight and bias),
    attention.self.distance_embedding x gd (where there is one), intermediate.dense x gi (weight and bias), and the head's
    token_decoder.dense1 x gi (weight and bias).  Nothing else is touched."""
    sd = {k: v.clone() for k, v in sd.items()}
    for li in range(layers):
        p = f"encoder.layer.{li}."
        for name, g in (("attention.self.query", gq), ("attention.self.key", gk), ("intermediate.dense", gi)):
            sd[p + name + ".weight"] *= g
            sd[p + name + ".bias"] *= g
        if p + "attention.self.distance_embedding.weight" in sd:
            sd[p + "attention.self.distance_embedding.weight"] *= gd
    sd["token_decoder.dense1.weight"] *= gi
    sd["token_decoder.dense1.bias"] *= gi
    return sd


def named_by_gains(key, layers):
    """Is state-dict entry `key` one that trained_gains multiplies?"""
    if key in ("token_decoder.dense1.weight", "token_decoder.dense1.bias"):
        return True
    for li in range(layers):
        p = f"encoder.layer.{li}."
        if key in [p + n + s for n in ("attention.self.query", "attention.self.key", "intermediate.dense") for s in (".weight", ".bias")]:
            return True
        if key == p + "attention.self.distance_embedding.weight":
            return True
    return False


def oracle_config(arch):
    return ref_model.OracleConfig(hidden_size=arch["hidden"], num_attention_heads=arch["heads"], intermediate_size=arch["ff"],
                                  num_hidden_layers=arch["layers"], max_position_embeddings=arch["maxpos"],
                                  position_embedding_type=arch["pos"])


def state_dict_for(name, regime):
    """The fp32 state dict of model `name` in `regime` ("plain": synthetic_model's weights as they are)."""
    arch, gains = MODELS[name]
    sd = ref_model.synthetic_model(oracle_config(arch), seed=SEED).state_dict()
    return trained_gains(sd, arch["layers"], *gains[regime]) if regime != "plain" else {k: v.clone() for k, v in sd.items()}


def load_both(o32, o64, sd):
    o32.load_state_dict(sd)
    o64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})


def oracle_pair(name, regime, T=1000, sd=None):
    """(fp32 oracle, fp64 oracle) of model `name` in `regime`, the fp64 one on the fp32 time table (as _share_time_table)."""
    arch, _ = MODELS[name]
    o32 = ref_model.synthetic_model(oracle_config(arch), seed=SEED)
    o64 = ref_model.synthetic_model(oracle_config(arch), seed=SEED).double()
    load_both(o32, o64, state_dict_for(name, regime) if sd is None else sd)
    o64.time_table = o32.time_embed(torch.arange(T)).double()
    return o32, o64


def mask_of(lens, L):
    m = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        m[i, :n] = 1.0
    return m


def inputs(B, L, seed=1):
    g = torch.Generator().manual_seed(seed)   # (test_gpu_parity._inputs)
    return ref_sampling.wrap(torch.randn(B, L, 6, generator=g) * 1.5)


# ------------------------------------------------------------------------------------ the attention, restated once more
def _attention(self, hidden_states, ext_mask, rounded=None, seen=None):
    """BertSelfAttention.forward of oracle/ref_model.py, with one operand optionally replaced by its fp16 rounding ("q", "k",
    "e": the distance table, "p": the probabilities) -- "the lo plane of this operand never reaches the MFMA" -- and, with `seen`,
    the scaled scores before the mask and the probabilities handed out."""
    def r16(x):
        return x.half().to(x.dtype)

    q = self._split(self.query(hidden_states))
    k = self._split(self.key(hidden_states))
    v = self._split(self.value(hidden_states))
    if rounded == "q":
        q = r16(q)
    if rounded == "k":
        k = r16(k)
    scores = torch.matmul(q, k.transpose(-1, -2))
    if self.position_embedding_type in ("relative_key", "relative_key_query"):
        L = hidden_states.shape[1]
        distance = torch.arange(L).view(-1, 1) - torch.arange(L).view(1, -1)
        pe = self.distance_embedding(distance + self.max_position_embeddings - 1).to(q.dtype)
        if rounded == "e":
            pe = r16(pe)
        scores = scores + torch.einsum("bhld,lrd->bhlr", q, pe)
        if self.position_embedding_type == "relative_key_query":
            scores = scores + torch.einsum("bhrd,lrd->bhlr", k, pe)
    scores = scores / math.sqrt(self.attention_head_size)
    probs = torch.softmax(scores + ext_mask, dim=-1)
    if seen is not None:
        seen.append((scores.detach().clone(), probs.detach().clone()))
    if rounded == "p":
        probs = r16(probs)
    ctx = torch.matmul(probs, v).permute(0, 2, 1, 3).contiguous()
    return ctx.view(ctx.shape[0], ctx.shape[1], -1)


def forward_restated(oracle, x, t, mask, rounded=None, seen=None):
    """One forward of `oracle` with every layer's attention replaced by _attention(rounded, seen)."""
    layers = [layer.attention.self for layer in oracle.encoder.layer]
    for att in layers:
        att.forward = types.MethodType(lambda self, h, ext: _attention(self, h, ext, rounded, seen), att)
    try:
        return oracle(x, t, attention_mask=mask)
    finally:
        for att in layers:
            del att.forward


def regime_stats(o64, x, t, mask):
    """(output, per-layer list of dicts) of one fp64 forward.  Per layer, over valid query rows and all heads, scores after the
    1 / sqrt(d_h) scaling and before the mask, keys of the row's own sequence only:
      range_median     median over rows of (largest - smallest score of the row)
      range_max        the largest such range (the f32 kernel clamps exponents at -200)
      score_max        largest |score|
      pmax_median      median row-maximum probability
      pmax_gt_0.9, pmax_lt_0.5, pmax_is_1   fractions of rows (the last: all the mass on one key to the last bit)
      argmax_past_128  of the rows of sequences longer than 128 (the others have one key tile whatever the weights): the fraction
                       whose largest score sits at key 128 or later, so that attention_img.hip's second tile raises the running
                       maximum and alpha < 1 rescales the first tile's sums
      ff_gt_4, ff_gt_3, ff_lt_m3            fractions of the feed-forward pre-activations of valid rows (|x| > 4, x > 3, x < -3)
      ff_max           largest |pre-activation|"""
    seen, pre = [], []
    handles = [layer.intermediate.dense.register_forward_hook(lambda m, a, o: pre.append(o.detach().clone()))
               for layer in o64.encoder.layer]
    try:
        out = forward_restated(o64, x.double(), t, mask.double(), seen=seen)
    finally:
        for h in handles:
            h.remove()
    valid = mask.bool()
    stats = []
    for (s, p), a in zip(seen, pre):
        H = s.shape[1]
        rows = valid[:, None, :].expand(-1, H, -1)                    # [B, H, L] valid query rows
        long_rows = rows & (valid.sum(1) > 128)[:, None, None]        # ... of sequences that have a second 128-key tile
        keys = valid[:, None, None, :].expand_as(s)
        hi = s.masked_fill(~keys, -math.inf).max(-1)
        lo = s.masked_fill(~keys, math.inf).min(-1).values
        rng = (hi.values - lo)[rows]
        pm = p.max(-1).values[rows]
        ffv = a[valid]
        stats.append({
            "range_median": float(rng.median()), "range_max": float(rng.max()),
            "score_max": float(s.abs()[keys & rows[..., None]].max()),
            "pmax_median": float(pm.median()), "pmax_gt_0.9": float((pm > 0.9).double().mean()),
            "pmax_lt_0.5": float((pm < 0.5).double().mean()), "pmax_is_1": float((pm == 1.0).double().mean()),
            "argmax_past_128": float((hi.indices[long_rows] >= 128).double().mean()) if long_rows.any() else 0.0,
            "ff_gt_4": float((ffv.abs() > 4).double().mean()), "ff_gt_3": float((ffv > 3).double().mean()),
            "ff_lt_m3": float((ffv < -3).double().mean()), "ff_max": float(ffv.abs().max()),
        })
    return out, stats


# ------------------------------------------------------------------------------------ the conditions (not tolerances)
def check_conditions(regime, stats):
    """The list of conditions of `regime` that the per-layer `stats` miss (empty: the regime is what it claims to be)."""
    missed = []

    def need(ok, li, what):
        if not ok:
            missed.append(f"layer {li}: {what}")

    for li, s in enumerate(stats):
        if regime == "moderate":
            need(10 <= s["range_median"] <= 60, li, f"median logit range {s['range_median']:.1f} not in [10, 60]")
            need(s["score_max"] <= 100, li, f"largest |score| {s['score_max']:.1f} > 100")
            need(0.3 <= s["pmax_median"] <= 0.9, li, f"median row-max probability {s['pmax_median']:.3f} not in [0.3, 0.9]")
            need(s["pmax_gt_0.9"] >= 0.05, li, f"{s['pmax_gt_0.9']:.3f} of rows with row-max > 0.9, < 0.05")
            need(s["pmax_lt_0.5"] >= 0.05, li, f"{s['pmax_lt_0.5']:.3f} of rows with row-max < 0.5, < 0.05")
        else:
            need(s["pmax_gt_0.9"] >= 0.55, li, f"{s['pmax_gt_0.9']:.3f} of rows with row-max > 0.9, < 0.55")
            need(s["range_median"] >= 80, li, f"median logit range {s['range_median']:.1f} < 80")
            need(s["score_max"] <= 300, li, f"largest |score| {s['score_max']:.1f} > 300")
            need(s["ff_gt_4"] >= 0.05, li, f"{s['ff_gt_4']:.3f} of feed-forward pre-activations beyond |x| = 4, < 0.05")
            need(s["ff_gt_3"] >= 0.01 and s["ff_lt_m3"] >= 0.01, li,
                 f"feed-forward pre-activations above 3: {s['ff_gt_3']:.3f}, below -3: {s['ff_lt_m3']:.3f}, one < 0.01")
    return missed


E_REF_MAX = 3e-6   # both regimes: the fp32 oracle's own relative distance from the fp64 one (the problem stays well posed in fp32)


def rel_gate(got, want32, want64):
    """test_gpu_parity._rel_gate, restated for the CPU tests (that module needs the GPU library to import)."""
    want64 = np.asarray(want64, np.float64)
    scale = np.abs(want64).max()
    e_dev = np.abs(np.asarray(got, np.float64) - want64).max() / scale
    e_ref = np.abs(np.asarray(want32, np.float64) - want64).max() / scale
    return float(e_dev), float(e_ref), max(4 * float(e_ref), 2e-6)


# ------------------------------------------------------------------------------------ one reverse step
def eps_coefficient(betas, t):
    """c(t): the coefficient of the predicted noise in the posterior mean of p_sample at step t,
    beta_t / (sqrt(1 - alphabar_t) * sqrt(alpha_t)) -- the factor by which an error of the forward reaches the step's output."""
    betas = np.asarray(betas, np.float64)
    alphas = 1.0 - betas
    abar = np.cumprod(alphas)
    return float(betas[t] / (np.sqrt(1.0 - abar[t]) * np.sqrt(alphas[t])))
