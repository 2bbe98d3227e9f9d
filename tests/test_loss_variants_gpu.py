"""
The rest of the denoising loss on the device (needs an MI355X: pytest -m gpu): the "l1" terms and the turn counts of the
circle penalty, the pairwise-distance term, and the model entry that runs them behind the forward, against the reference's
golden fixture (tests/golden/ref_loss_variants.npz).

Tolerances:
  * turn counts:            exact (integers)
  * per-position l1 terms:  <= 1e-6 absolute (a term is at most pi and takes a handful of fp32 roundings of 6e-8 relative
                            each); the aim is 0 -- the maximum is printed
  * per-sequence sums:      relative 1e-12 against an fp64 numpy sum of the kernel's own terms
  * CA coordinates and per-sequence pairwise sums against the reference: 10 x the maxima the fp64 host statement of
                            the kernel shows against the same reference on the CPU (test_loss_variants.py: 3.9e-6 A,
                            1.04e-6 relative) -- the device's fp64 sin / cos rounded to float32 differ from torch's
                            vectorised float32 ones in the same last-bit way, and the chain amplifies a flip
  * forward eps:            max|d| <= 1e-5, the project's forward gate
  * loss_terms(batch), "l1" and the circle setting: <= 1.2e-5 against the reference (l1 is 1-Lipschitz in the
                            prediction; no turn count can flip, the fixture keeps |pred| 1e-3 away from the steps);
                            the pairwise entry is printed, not gated: its sensitivity to the forward grows as 1 / keep
  * same bits in, same kernels: bit-exact
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden
from foldingdiff_amd import _binding, beta_schedules, losses, modelling
from oracle import ref_model

pytestmark = pytest.mark.gpu

FWD_TOL, TERM_TOL, SUM_RTOL, LOSS_TOL = 1e-5, 1e-6, 1e-12, 1.2e-5
CA_TOL, SEQ_RTOL = 10 * 3.9e-6, 10 * 1.04e-6
F = 6
SETS = ("s1", "s2")
REPORT = {}


def _record(name, **kw):
    """Every measured figure is printed before its assertion (pytest -s shows them)."""
    REPORT[name] = {k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kw.items()}
    print(name, json.dumps(REPORT[name], sort_keys=True))


@pytest.fixture(scope="module")
def gv():
    return golden("ref_loss_variants.npz")


def _set(gv, tag):
    return {k.split("::", 1)[1]: gv[k] for k in gv.files if k.startswith(tag + "::")}


def _pdist_setting(gv):
    return (float(gv["pdist"][0]), float(gv["pdist"][1]), int(gv["pdist"][2]))


def _check_sums(name, sums, terms):
    want = terms.astype(np.float64).sum(axis=1)
    rel = np.abs(sums - want).max() / max(np.abs(want).max(), 1e-300)
    _record(name + "_sums", max_rel=rel)
    assert np.all(np.abs(sums - want) <= SUM_RTOL * np.maximum(np.abs(want), 1e-300)), rel


def _check_terms(name, terms, want):
    err = np.abs(terms.astype(np.float64) - want).max()
    _record(name, max=err, bit_equal=bool(np.array_equal(terms, want)))
    assert err <= TERM_TOL


# ------------------------------------------------------------ 1. l1 terms and turns
@pytest.mark.parametrize("tag", SETS)
def test_l1_terms_and_turns_on_the_golden_batches(gpu, gv, tag):
    g = _set(gv, tag)
    lens, on = g["lengths"].astype(np.int32), g["attn_mask"][:, :, None] != 0
    sums, terms, turns = losses.loss_terms(g["pred"], g["known_noise"], lens, [True] * F, kind="l1", return_turns=True)
    _check_terms(f"l1_terms_{tag}", terms, g["terms_l1"] * on)
    assert not terms[~np.broadcast_to(on, terms.shape)].any()
    assert turns.dtype == np.int64 and np.array_equal(turns, (g["turns"] * on).sum(axis=1))
    _check_sums(f"l1_terms_{tag}", sums, terms)
    got = sums.sum(axis=0) / lens.sum()        # the reference's six numbers from its own prediction
    assert np.abs(got - g["ref_l1"]).max() <= 2e-6
    # kind 0 through the new entry: fd_loss_terms' bits, with the same counts beside them
    s0, t0, n0 = losses.loss_terms(g["pred"], g["known_noise"], lens, [True] * F, kind=0, return_turns=True)
    s_old, t_old = losses.loss_terms(g["pred"], g["known_noise"], lens, [True] * F)
    assert np.array_equal(s0, s_old) and np.array_equal(t0, t_old) and np.array_equal(n0, turns)
    assert np.array_equal(losses.loss_terms(g["pred"], g["known_noise"], g["attn_mask"], [True] * F, kind=1, return_terms=False), sums)


def test_l1_terms_and_turns_at_the_seams(gpu, gv):
    """The fixture's synthetic set (differences at +-pi, inputs at the remainder's seam, |pred| at the multiples of pi; terms
    and counts by the reference's functions), tiled over sequences of lengths 1, 7, 63, 64, 65, 129 and 300 at L = 300 with
    mixed angular flags."""
    lens = np.array([1, 7, 63, 64, 65, 129, 300], np.int32)
    flags = np.array([True, False, True, True, False, True])
    B, L, n = len(lens), 300, len(gv["syn_pred"])
    idx = (np.arange(L * F).reshape(1, L, F) + 13 * np.arange(B).reshape(B, 1, 1)) % n
    pred, target = gv["syn_pred"][idx], gv["syn_target"][idx]
    on = np.arange(L)[None, :, None] < lens[:, None, None]
    want = np.where(flags[None, None, :], gv["syn_terms_l1_ang"][idx], gv["syn_terms_l1_lin"][idx]).astype(np.float32) * on
    want_turns = (gv["syn_turns"][idx].astype(np.int64) * on * flags[None, None, :]).sum(axis=1)
    sums, terms, turns = losses.loss_terms(pred, target, lens, list(flags), kind=1, return_turns=True)
    _check_terms("l1_terms_synthetic", terms, want)
    assert np.array_equal(turns, want_turns) and turns.max() > 100 and not turns[:, ~flags].any()
    _check_sums("l1_terms_synthetic", sums, terms)
    # run to run, and wherever a sequence sits in the batch: the same bits
    again = losses.loss_terms(pred, target, lens, list(flags), kind=1, return_turns=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (sums, terms, turns)))
    perm = np.array([4, 6, 0, 2, 5, 1, 3])
    s3, n3 = losses.loss_terms(pred[perm], target[perm], lens[perm], list(flags), kind=1, return_terms=False, return_turns=True)
    assert np.array_equal(s3, sums[perm]) and np.array_equal(n3, turns[perm])


@pytest.mark.parametrize("Fn", [1, 32])
def test_l1_terms_feature_counts_at_both_ends(gpu, Fn):
    g = torch.Generator().manual_seed(Fn)
    lens, L = np.array([300, 1, 77], np.int32), 300
    pred, target = torch.randn(3, L, Fn, generator=g) * 4, torch.randn(3, L, Fn, generator=g) * 4
    flags = [f % 3 != 1 for f in range(Fn)]
    on = np.arange(L)[None, :, None] < lens[:, None, None]
    want = losses.host_terms(pred, target, flags, loss="l1").numpy() * on
    want_turns = (losses.circle_turns(pred).numpy().astype(np.int64) * on * np.array(flags)[None, None, :]).sum(axis=1)
    sums, terms, turns = losses.loss_terms(pred, target, lens, flags, kind=1, return_turns=True)
    _check_terms(f"l1_terms_F{Fn}", terms, want)
    assert np.array_equal(turns, want_turns)
    _check_sums(f"l1_terms_F{Fn}", sums, terms)


def test_l1_terms_every_length_up_to_twenty(gpu):
    L = 20
    g = torch.Generator().manual_seed(20)
    lens = np.arange(1, L + 1, dtype=np.int32)
    pred, target = torch.randn(L, L, F, generator=g) * 4, torch.randn(L, L, F, generator=g) * 4
    flags = [True, True, False, True, True, True]
    on = np.arange(L)[None, :, None] < lens[:, None, None]
    want = losses.host_terms(pred, target, flags, loss="l1").numpy() * on
    want_turns = (losses.circle_turns(pred).numpy().astype(np.int64) * on * np.array(flags)[None, None, :]).sum(axis=1)
    sums, terms, turns = losses.loss_terms(pred, target, lens, flags, kind=1, return_turns=True)
    _check_terms("l1_terms_all_lengths", terms, want)
    assert np.array_equal(turns, want_turns)
    _check_sums("l1_terms_all_lengths", sums, terms)


# ------------------------------------------------------------ 2. the pairwise-distance term on the recorded prediction
def _pairwise_args(g):
    return (g["angles"], g["corrupted"], g["pred"], g["sqrt_alphas_cumprod_t"], g["sqrt_one_minus_alphas_cumprod_t"],
            g["lengths"].astype(np.int32), np.arange(6, dtype=np.int32))


@pytest.mark.parametrize("tag", SETS)
def test_pairwise_entry_against_the_reference(gpu, gv, tag):
    g = _set(gv, tag)
    args = _pairwise_args(g)
    lens, L = args[5], g["angles"].shape[1]
    sums, pairs, ca = losses.pairwise_dist_sums(*args, coef=g["coef"], return_ca=True)
    on = np.broadcast_to((np.arange(L)[None, :] < lens[:, None])[:, None, :, None], ca.shape)
    ref_ca = np.stack([g["ca_clean"], g["ca_denoised"]], axis=1)
    ca_err = np.abs((ca - ref_ca) * on).max()
    assert pairs.dtype == np.int64 and np.array_equal(pairs, lens.astype(np.int64) * (lens - 1) // 2)
    has = pairs > 0
    want = g["pd_per_seq"].astype(np.float64) * pairs
    seq_rel = (np.abs(sums[has] - want[has]) / want[has]).max()
    batch = sums.sum() / pairs.sum()
    host_sums, _, host_ca = losses.pairwise_dist_host(*args[:6], range(6), coef=g["coef"])
    _record(f"pairwise_{tag}", ca_max=ca_err, seq_rel=seq_rel, batch=batch, batch_rel=abs(batch - float(g["pd_batch"])) / float(g["pd_batch"]),
            ca_vs_host=np.abs(ca - host_ca).max(), sums_rel_vs_host=(np.abs(sums[has] - host_sums[has]) / host_sums[has]).max())
    assert ca_err <= CA_TOL
    assert seq_rel <= SEQ_RTOL
    assert not ca[~on].any()                                    # zeros past each length
    assert (sums[~has] == 0).all() and (pairs[~has] == 0).all()   # a sequence of one residue: no pairs
    if tag == "s1":
        assert (~has).sum() == 1 and lens[~has][0] == 1
    # the scalar weight (every pair times 0.25) and no weight at all
    s_scalar, _ = losses.pairwise_dist_sums(*args, coef=float(gv["scalar_coef"]))
    want = g["pd_scalar_per_seq"].astype(np.float64) * pairs
    assert (np.abs(s_scalar[has] - want[has]) / want[has]).max() <= SEQ_RTOL
    s_none, _ = losses.pairwise_dist_sums(*args)
    assert np.array_equal(s_none * 0.25, s_scalar)              # (0.25 is a power of two: every float32 term scales exactly)
    # two runs, and the batch reversed: the same bits
    again = losses.pairwise_dist_sums(*args, coef=g["coef"], return_ca=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (sums, pairs, ca)))
    rev = losses.pairwise_dist_sums(*[a[::-1].copy() for a in args[:6]], args[6], coef=g["coef"][::-1].copy(), return_ca=True)
    assert np.array_equal(rev[0][::-1], sums) and np.array_equal(rev[1][::-1], pairs) and np.array_equal(rev[2][::-1], ca)


def test_pairwise_entry_with_the_columns_elsewhere(gpu, gv):
    """F = 9 with the six angles at scattered columns: the same sums as with F = 6."""
    g = _set(gv, "s1")
    args = _pairwise_args(g)
    cols = np.array([7, 0, 5, 2, 8, 3], np.int32)
    wide = []
    for a in args[:3]:
        w = np.full(a.shape[:2] + (9,), 123.0, np.float32)
        w[:, :, cols] = a
        wide.append(w)
    got = losses.pairwise_dist_sums(*wide, *args[3:6], cols, coef=g["coef"])
    want = losses.pairwise_dist_sums(*args, coef=g["coef"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------ 3. the model entry
def _model_for(gv, tag, precision):
    """(product model on cuda:0, oracle or None).  s1: the absolute-position model of ref_abs_model.npz, whose reference
    forward is the fixture's pred; s2: the oracle's synthetic relative_key model the fixture names."""
    names = [str(n) for n in gv["names"]]
    if tag == "s1":
        gm = golden("ref_abs_model.npz")
        cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                   max_position_embeddings=64, position_embedding_type="absolute")
        pm = modelling.BertForDiffusionBase(cfg, [True] * F, ft_names=names)
        pm.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")})
        o32 = None
    else:
        hidden, heads, seed = (int(v) for v in gv["oracle_s2"])
        ocfg = ref_model.OracleConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                      num_hidden_layers=2, max_position_embeddings=128, position_embedding_type="relative_key")
        o32 = ref_model.synthetic_model(ocfg, (True,) * F, "gaussian_fourier", "mlp", seed=seed)
        pcfg = modelling.BertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                    num_hidden_layers=2, max_position_embeddings=128, position_embedding_type="relative_key")
        pm = modelling.BertForDiffusionBase(pcfg, [True] * F, ft_names=names)
        pm.load_state_dict(o32.state_dict())
    pm.to("cuda:0")
    pm.set_precision(precision)
    pm.prepare(beta_schedules.cosine_beta_schedule(int(gv["T"])))
    return pm, o32


def _batch(g):
    return {k: torch.from_numpy(g[k]) for k in ("corrupted", "t", "known_noise", "attn_mask", "angles", "lengths",
                                                "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t")}


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag", SETS)
def test_model_entry_equals_the_model_free_entries_and_the_reference(gpu, gv, tag, precision):
    g = _set(gv, tag)
    pm, o32 = _model_for(gv, tag, precision)
    b = _batch(g)
    lens, idx = g["lengths"].astype(np.int32), np.arange(6, dtype=np.int32)
    keep, spread = b["sqrt_alphas_cumprod_t"], b["sqrt_one_minus_alphas_cumprod_t"]
    coef = losses.pairwise_coef(_pdist_setting(gv), b["t"])
    name = f"model_{tag}_{precision}"
    for kind in (1, 0):
        out = pm.denoise_loss_ex(b["angles"], b["known_noise"], b["t"], b["attn_mask"], corrupted=b["corrupted"], keep=keep, spread=spread,
                                 kind=kind, return_turns=True, pairwise=True, coef=coef, return_corrupted=True, return_eps=True)
        assert np.array_equal(out["corrupted"], g["corrupted"])
        want = o32(b["corrupted"], b["t"], attention_mask=b["attn_mask"]).numpy() if o32 is not None else g["pred"]
        err = np.abs(out["eps"].astype(np.float64) - want).max()
        _record(f"{name}_kind{kind}_eps", max=err, vs_fixture=np.abs(out["eps"].astype(np.float64) - g["pred"]).max())
        assert err <= FWD_TOL
        # the same kernels on the same bits: what the two model-free entries return for this call's x_t and prediction
        s, n = losses.loss_terms(out["eps"], g["known_noise"], lens, [True] * F, kind=kind, return_terms=False, return_turns=True)
        assert np.array_equal(out["sums"], s) and np.array_equal(out["turns"], n)
        ps, pn = losses.pairwise_dist_sums(g["angles"], out["corrupted"], out["eps"], keep, spread, lens, idx, coef=coef)
        assert np.array_equal(out["pair_sums"], ps) and np.array_equal(out["pairs"], pn)
    # all three settings off: fd_denoise_loss's bits; and the device's own noising: its x_t
    plain = pm.denoise_loss_ex(b["corrupted"], b["known_noise"], b["t"], b["attn_mask"], corrupted=b["corrupted"])
    assert set(plain) == {"sums"}
    assert np.array_equal(plain["sums"], pm.denoise_loss_sums(b["corrupted"], b["known_noise"], b["t"], b["attn_mask"]))
    noised = pm.denoise_loss_ex(b["angles"], b["known_noise"], b["t"], b["attn_mask"], keep=keep, spread=spread, return_corrupted=True)
    s_old, extra = pm.denoise_loss_sums(b["angles"], b["known_noise"], b["t"], b["attn_mask"], keep=keep, spread=spread, return_corrupted=True)
    assert np.array_equal(noised["corrupted"], extra["corrupted"]) and np.array_equal(noised["sums"], s_old)
    assert np.array_equal(noised["corrupted"], g["corrupted"])
    # loss_terms(batch) under each setting against the reference's _get_loss_terms
    base = {k: b[k] for k in ("corrupted", "t", "known_noise", "attn_mask")}
    got = pm.set_loss("l1").loss_terms(base)
    err = np.abs(got.numpy() - g["ref_l1"].astype(np.float64)).max()
    _record(f"{name}_loss_l1", max=err)
    assert got.shape == (F,) and got.dtype == torch.float64 and err <= LOSS_TOL
    got = pm.set_loss("smooth_l1", circle_reg=float(gv["circle_lambda"])).loss_terms(base)
    err = np.abs(got.numpy() - g["ref_circle"].astype(np.float64)).max()
    _record(f"{name}_loss_circle", max=err)
    assert got.shape == (F,) and err <= LOSS_TOL
    got = pm.set_loss("smooth_l1", use_pdist_loss=_pdist_setting(gv)).loss_terms(b)
    assert got.shape == (F + 1,) and np.abs(got.numpy()[:F] - g["ref_pdist"][:F].astype(np.float64)).max() <= LOSS_TOL
    ref_pd = float(g["ref_pdist"][F])
    _record(f"{name}_loss_pairwise", got=float(got[F]), want=ref_pd, rel=abs(float(got[F]) - ref_pd) / ref_pd)   # printed, not gated
    assert np.isfinite(float(got[F])) and float(got[F]) > 0
    # the scalar form: every pair times the weight
    got_s = pm.set_loss("smooth_l1", use_pdist_loss=float(gv["scalar_coef"])).loss_terms(b)
    _record(f"{name}_loss_pairwise_scalar", got=float(got_s[F]), want=float(g["pd_scalar"]))
    # the defaults again: what a model without the settings returns, bit for bit
    assert torch.equal(pm.set_loss().loss_terms(base), torch.from_numpy(plain["sums"].sum(axis=0) / int(lens.sum())))


def test_a_batch_without_pairs_gives_nan(gpu, gv):
    g = _set(gv, "s1")
    pm, _ = _model_for(gv, "s1", "f16x3")
    b = {k: v[1:2] for k, v in _batch(g).items()}     # the sequence of one residue
    got = pm.set_loss("smooth_l1", use_pdist_loss=_pdist_setting(gv)).loss_terms(b)
    assert got.shape == (F + 1,) and np.isnan(float(got[F])) and np.isfinite(got[:F].numpy()).all()


# ------------------------------------------------------------ 4. argument errors of the model entry
def test_model_entry_returns_error_codes(gpu, gv):
    g = _set(gv, "s1")
    pm, _ = _model_for(gv, "s1", "f16x3")
    lib, h, P = _binding.load(), pm._ensure_handle(), _binding.ptr
    B, L, _ = g["corrupted"].shape
    x, lens, t = g["corrupted"].copy(), g["lengths"].astype(np.int32), g["t"].reshape(-1).astype(np.int32)
    keep, spread = g["sqrt_alphas_cumprod_t"].copy(), g["sqrt_one_minus_alphas_cumprod_t"].copy()
    idx = np.arange(6, dtype=np.int32)
    ba, bl = C.c_float(losses.ANGULAR_BETA), C.c_float(1.0)

    def call(kind=0, keep=keep, spread=spread, corrupted=x, idx=idx, pairwise=True, pairs="d"):
        sums, ps = np.full((B, F), -7.0), np.full(B, -7.0)
        pairs = np.full(B, -7, np.int64) if isinstance(pairs, str) else pairs
        rc = lib.fd_denoise_loss_ex(h, P(x), P(corrupted), P(x), P(t), P(keep), P(spread), P(lens), B, L, kind, ba, bl, None,
                                    P(idx), P(sums), None, P(ps) if pairwise else None, P(pairs), None, None)
        return [sums, ps] + ([pairs] if pairs is not None else []), rc

    missing, zero = idx.copy(), keep.copy()
    missing[3], zero[2] = 6, 0.0          # the tau column is not among the F = 6 features
    for kw, word in [(dict(keep=None, spread=None), b"keep and spread"), (dict(keep=None), b"keep and spread go together"),
                     (dict(idx=missing), b"feat_idx[3]=6"), (dict(idx=None), b"feat_idx"), (dict(pairs=None), b"pairs"),
                     (dict(kind=2), b"kind=2"), (dict(keep=zero), b"keep[2]"),
                     (dict(corrupted=None, keep=None, spread=None, pairwise=False), b"keep and spread")]:
        outs, rc = call(**kw)
        msg = lib.fd_last_error()
        assert rc != 0 and word in msg, (kw.keys(), word, rc, msg)
        assert all((o == -7).all() for o in outs)
    # the python layer names a feature set without the six angles before any call
    pm.ft_names = ["phi", "psi", "omega", "tau", "CA:C:1N", "d0"]
    with pytest.raises(ValueError, match="C:1N:1CA"):
        pm.set_loss(use_pdist_loss=0.1).loss_terms(_batch(g))
    # the model still works afterwards
    outs, rc = call()
    assert rc == 0 and np.array_equal(outs[2], lens.astype(np.int64) * (lens - 1) // 2)


# ------------------------------------------------------------ 5. the command line's evaluation on a model directory
def test_validation_loss_tool_reports_what_the_directory_was_trained_with(gpu, tmp_path):
    """bin/validation_loss.py's ``evaluate`` on a model directory as training leaves it, whose training_args.json says
    loss "l1" and use_pdist_loss [0.05, 0.5, 1000]: the settings are found, val_loss_pairwise_dist_loss is reported, val_loss
    is over F + 1 values, and the numbers are those of loss_terms on the same noised batch; the command line's overrides
    win over the directory."""
    import sys

    from conftest import GOLDEN, REPO
    from test_gpu_parity import _write_model_dir
    sys.path.insert(0, os.path.join(REPO, "bin"))
    import validation_loss as tool
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * F, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    args_path = os.path.join(mdir, "training_args.json")
    args = json.load(open(args_path))
    args.update(loss="l1", use_pdist_loss=[0.05, 0.5, 1000])
    json.dump(args, open(args_path, "w"))
    pdbs = [os.path.join(GOLDEN, "1CRN.pdb"), os.path.join(GOLDEN, "all_residues.pdb")]
    out = tool.evaluate(mdir, pdbs, seed=11)
    assert out["loss"] == "l1" and out["circle_reg"] == 0.0 and tuple(out["use_pdist_loss"]) == (0.05, 0.5, 1000)
    names = list(losses.PAIRWISE_ANGLES)
    assert len(out["per_batch"]) == 1 and len(out["per_batch"][0]["loss_terms"]) == F + 1
    terms = np.array(out["per_batch"][0]["loss_terms"])
    assert np.isfinite(terms).all() and (terms > 0).all()
    assert out["val_loss"] == pytest.approx(terms.mean(), rel=1e-15)
    assert out["val_loss_pairwise_dist_loss"] == pytest.approx(terms[F], rel=1e-15)
    assert [out[f"val_loss_{n}"] for n in names] == pytest.approx(list(terms[:F]), rel=1e-15)
    # the same noised batch through the model directly
    dset = tool.load_dataset(pdbs, tool.Path(mdir))
    net = modelling.BertForDiffusionBase.from_dir(mdir).to("cuda:0")
    assert net.loss_key == "l1" and net.use_pairwise_dist_loss == (0.05, 0.5, 1000) and net.ft_names == names
    net.prepare(dset.alpha_beta_terms["betas"])
    torch.manual_seed(11)
    items = [dset[i] for i in range(len(dset))]
    batch = {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in
             ("corrupted", "t", "known_noise", "attn_mask", "angles", "lengths", "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t")}
    assert np.array_equal(net.loss_terms(batch).numpy(), terms)
    # overrides: the smooth-L1 pair and no pairwise term, whatever the directory says
    plain = tool.evaluate(mdir, pdbs, seed=11, loss="smooth_l1", pdist_loss=[0.0])
    assert plain["loss"] == "smooth_l1" and plain["use_pdist_loss"] == 0.0 and "val_loss_pairwise_dist_loss" not in plain
    assert len(plain["per_batch"][0]["loss_terms"]) == F
    curve = tool.evaluate(mdir, pdbs, seed=11, timesteps_curve=3)["curve"]
    assert curve["features"] == names + ["pairwise_dist_loss"] and np.array(curve["loss"]).shape == (3, F + 1)
