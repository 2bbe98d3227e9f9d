"""Host side of the rest of the denoising loss (no GPU): "l1", the circle penalty and the pairwise-distance term.  The
torch restatements and the numpy emulation of the kernels' operation order against the reference's golden fixture
(tests/golden/ref_loss_variants.npz), the loss settings of the model, the batch logic of validation.validation_loss
with the extra term, and the new C-ABI entries' declarations and argument checks.

Measured here (printed by the test, recorded in DESIGN 6j), fp64 host statement of the pairwise kernel against the
reference: CA coordinates within 3.9e-6 A (L = 128), a per-sequence value within 1.04e-6 relative, the batch value
within 1.4e-7, the scalar-weight variant within 1.4e-7.  The difference is the reference's float32 sin / cos (torch's
vectorised ones are not correctly rounded, the kernel's are) amplified along the chain.  The gates are 10 x the maxima.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from foldingdiff_amd import _binding, losses, modelling, validation

NEW_ENTRIES = ("fd_loss_terms_ex", "fd_pairwise_dist", "fd_denoise_loss_ex")
SETS = ("s1", "s2")
F = 6
CA_MEASURED, SEQ_REL_MEASURED, BATCH_REL_MEASURED = 3.9e-6, 1.04e-6, 1.4e-7
CA_TOL, SEQ_RTOL, BATCH_RTOL = 10 * CA_MEASURED, 10 * SEQ_REL_MEASURED, 10 * BATCH_REL_MEASURED


@pytest.fixture(scope="module")
def gv():
    return golden("ref_loss_variants.npz")


def _set(gv, tag):
    return {k.split("::", 1)[1]: gv[k] for k in gv.files if k.startswith(tag + "::")}


def _pdist_setting(gv):
    return (float(gv["pdist"][0]), float(gv["pdist"][1]), int(gv["pdist"][2]))


# ------------------------------------------------------------ the kernels' operation order in numpy float32
PI_F, TWO_PI_F = np.float32(3.14159274101257324), np.float32(6.28318548202514648)


def emu_rem_two_pi(v):
    m = np.fmod(v, TWO_PI_F)
    return np.where((m != 0) & (m < 0), m + TWO_PI_F, m).astype(np.float32)


def emu_wrap_pi(v):
    return (emu_rem_two_pi(v + PI_F) + (-PI_F)).astype(np.float32)


def emu_l1_terms(pred, target, angular):
    """l1_term of csrc/loss_variants.hip, one rounded float32 operation per step."""
    pred, target = pred.astype(np.float32), target.astype(np.float32)
    ang = np.abs(emu_wrap_pi(emu_rem_two_pi(target) - emu_rem_two_pi(pred)))
    lin = np.abs(target - pred)
    out = np.where(np.asarray(angular, bool), ang, lin)
    assert out.dtype == np.float32
    return out


def emu_turns(pred):
    q = np.abs(pred.astype(np.float32)) / PI_F
    assert q.dtype == np.float32
    return np.trunc(q).astype(np.int64)


# ------------------------------------------------------------ 1. restatements against the reference
@pytest.mark.parametrize("tag", SETS)
def test_host_restatements_have_the_reference_bits(gv, tag):
    g = _set(gv, tag)
    pred, target = torch.from_numpy(g["pred"]), torch.from_numpy(g["known_noise"])
    got = losses.host_terms(pred, target, [True] * F, loss="l1").numpy()
    assert got.dtype == np.float32 and np.array_equal(got, g["terms_l1"])
    assert np.array_equal(losses.circle_turns(pred).numpy(), g["turns"].astype(np.float32))
    keep, spread = torch.from_numpy(g["sqrt_alphas_cumprod_t"]), torch.from_numpy(g["sqrt_one_minus_alphas_cumprod_t"])
    den = losses.denoised_angles(torch.from_numpy(g["corrupted"]), pred, keep, spread)
    assert den.dtype == torch.float32 and np.array_equal(den.numpy(), g["denoised"])
    coef = losses.pairwise_coef(_pdist_setting(gv), torch.from_numpy(g["t"]))
    assert coef.dtype == torch.float32 and coef.shape == g["coef"].shape and np.array_equal(coef.numpy(), g["coef"])
    # _get_loss_terms' values from the reference's own prediction: masked selection, then the function
    idx = torch.where(torch.from_numpy(g["attn_mask"]))
    for f in range(F):
        p, t = pred[idx[0], idx[1], f], target[idx[0], idx[1], f]
        assert losses.radian_l1_loss(p, t).item() == g["ref_l1"][f]
        assert losses.radian_smooth_l1_circle_loss(p, t, beta=losses.ANGULAR_BETA, circle_penalty=float(gv["circle_lambda"])).item() == g["ref_circle"][f]
        assert losses.radian_smooth_l1_circle_loss(p, t, beta=losses.ANGULAR_BETA).item() == g["ref_plain"][f]
    # pairwise_dist_loss on the reference's own coordinates: the batch, and the scalar weight as a 0-dim tensor
    ca_den, ca_clean, lens = torch.from_numpy(g["ca_denoised"]), torch.from_numpy(g["ca_clean"]), torch.from_numpy(g["lengths"])
    assert losses.pairwise_dist_loss(ca_den, ca_clean, lengths=lens, weights=coef).item() == g["pd_batch"] == g["ref_pdist"][F]
    w0 = losses.pairwise_coef(float(gv["scalar_coef"]), torch.from_numpy(g["t"]))
    assert w0.ndim == 0 and w0.dtype == torch.float32
    assert losses.pairwise_dist_loss(ca_den, ca_clean, lengths=lens, weights=w0).item() == g["pd_scalar"]
    for b in range(len(lens)):
        v = losses.pairwise_dist_loss(ca_den[b:b + 1], ca_clean[b:b + 1], lengths=lens[b:b + 1], weights=coef[b:b + 1]).item()
        assert v == g["pd_per_seq"][b] or (np.isnan(v) and np.isnan(g["pd_per_seq"][b]) and int(lens[b]) == 1)


def test_synthetic_seams_restatement_and_emulation(gv):
    """Differences within 1e-3 of +-pi, inputs at the remainder's seam (0, +-2 pi, +-4 pi), |pred| at the multiples of pi:
    the torch restatement and the numpy emulation of the kernel's order both have the reference's bits."""
    sp, st = gv["syn_pred"], gv["syn_target"]
    tp, tt = torch.from_numpy(sp), torch.from_numpy(st)
    for p, t, a, l in zip(tp, tt, gv["syn_terms_l1_ang"], gv["syn_terms_l1_lin"]):
        assert losses.radian_l1_loss(p.reshape(1), t.reshape(1)).item() == a
        assert torch.nn.functional.l1_loss(p.reshape(1), t.reshape(1)).item() == l
    assert np.array_equal(losses.circle_turns(tp).numpy().astype(np.int32), gv["syn_turns"])
    assert np.array_equal(emu_l1_terms(sp, st, True), gv["syn_terms_l1_ang"])
    assert np.array_equal(emu_l1_terms(sp, st, False), gv["syn_terms_l1_lin"])
    assert np.array_equal(emu_turns(sp), gv["syn_turns"].astype(np.int64))
    # the set does what it is for: turn counts 0 .. 5, terms at both ends of [0, pi], inputs beyond one turn
    assert set(gv["syn_turns"].tolist()) == {0, 1, 2, 3, 4, 5}
    assert (gv["syn_terms_l1_ang"] < 1e-3).any() and (gv["syn_terms_l1_ang"] > np.pi - 1e-3).any()
    assert (np.abs(sp) > 2 * np.pi).any() and (np.abs(st) > 2 * np.pi).any()


@pytest.mark.parametrize("tag", SETS)
def test_kernel_order_emulation_gives_the_golden_terms_and_turns(gv, tag):
    g = _set(gv, tag)
    assert np.array_equal(emu_l1_terms(g["pred"], g["known_noise"], [True] * F), g["terms_l1"])
    assert np.array_equal(emu_turns(g["pred"]), g["turns"].astype(np.int64))
    keep, spread = g["sqrt_alphas_cumprod_t"][:, None, None], g["sqrt_one_minus_alphas_cumprod_t"][:, None, None]
    den = (g["corrupted"] - spread * g["pred"]) / keep    # __fdiv_rn(__fsub_rn(c, __fmul_rn(spread, p)), keep)
    assert den.dtype == np.float32 and np.array_equal(den, g["denoised"])


def test_circle_penalty_zero_keeps_todays_bits():
    gl = golden("ref_loss.npz")
    ang = [bool(a) for a in gl["ft_is_angular"]]
    pred, target = torch.from_numpy(gl["pred"]), torch.from_numpy(gl["known_noise"])
    assert np.array_equal(losses.host_terms(pred, target, ang).numpy(), gl["terms"])
    idx = torch.where(torch.from_numpy(gl["attn_mask"]))
    for f, a in enumerate(ang):
        if a:
            p, t = pred[idx[0], idx[1], f], target[idx[0], idx[1], f]
            assert losses.radian_smooth_l1_loss(p, t, beta=losses.ANGULAR_BETA, circle_penalty=0.0).item() == gl["ref_loss_terms"][f]
            assert losses.radian_smooth_l1_circle_loss(p, t, beta=losses.ANGULAR_BETA, circle_penalty=0.0).item() == gl["ref_loss_terms"][f]
    # and a penalty that bites: the mean of the whole turns of the prediction, weighted
    p = torch.tensor([0.5, -4.0, 7.0, -10.0])
    got = losses.radian_smooth_l1_circle_loss(p, p.clone(), beta=0.3, circle_penalty=0.5).item()
    assert got == pytest.approx(0.5 * (0 + 1 + 2 + 3) / 4, rel=1e-6)


# ------------------------------------------------------------ 2. the fp64 host statement of the pairwise kernel
@pytest.mark.parametrize("tag", SETS)
def test_pairwise_host_statement_against_the_reference(gv, tag):
    """float32 trigonometry (correctly rounded, as on the device), float64 frames, float32 distances: every figure is
    printed before it is asserted; the gates are 10 x the maxima measured over both sets (module docstring)."""
    g = _set(gv, tag)
    lens, L = g["lengths"], g["angles"].shape[1]
    sums, pairs, ca = losses.pairwise_dist_host(g["angles"], g["corrupted"], g["pred"], g["sqrt_alphas_cumprod_t"],
                                                g["sqrt_one_minus_alphas_cumprod_t"], lens, range(6), coef=g["coef"])
    on = (np.arange(L)[None, :] < lens[:, None])[:, :, None]
    ca_err = max(np.abs((ca[:, 0] - g["ca_clean"]) * on).max(), np.abs((ca[:, 1] - g["ca_denoised"]) * on).max())
    assert np.array_equal(pairs, lens * (lens - 1) // 2)
    has = pairs > 0
    want = g["pd_per_seq"].astype(np.float64) * pairs
    seq_rel = (np.abs(sums[has] - want[has]) / want[has]).max()
    batch_rel = abs(sums.sum() / pairs.sum() - float(g["pd_batch"])) / float(g["pd_batch"])
    s2, _, _ = losses.pairwise_dist_host(g["angles"], g["corrupted"], g["pred"], g["sqrt_alphas_cumprod_t"],
                                         g["sqrt_one_minus_alphas_cumprod_t"], lens, range(6), coef=np.float32(gv["scalar_coef"]))
    scalar_rel = abs(s2.sum() / pairs.sum() - float(g["pd_scalar"])) / float(g["pd_scalar"])
    print(f"pairwise host statement {tag}: ca {ca_err:.3e} A, per-sequence rel {seq_rel:.3e}, batch rel {batch_rel:.3e}, "
          f"scalar-weight rel {scalar_rel:.3e}")
    assert ca_err <= CA_TOL
    assert seq_rel <= SEQ_RTOL
    assert batch_rel <= BATCH_RTOL and scalar_rel <= BATCH_RTOL
    assert (sums[~has] == 0).all() and not ca[~np.broadcast_to(on[:, None], ca.shape)].any()


# ------------------------------------------------------------ 3. the model's loss settings
def _toy_model(**kw):
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                               max_position_embeddings=64, position_embedding_type="absolute")
    return modelling.BertForDiffusionBase(cfg, [True] * F, **kw)


def test_from_dir_reads_the_loss_settings(tmp_path):
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                               max_position_embeddings=64, position_embedding_type="absolute")
    cfg.save_pretrained(tmp_path)
    base = {"angles_definitions": "canonical-full-angles", "time_encoding": "gaussian_fourier", "decoder": "mlp"}

    def load(**extra):
        with open(tmp_path / "training_args.json", "w") as fh:
            json.dump({**base, **extra}, fh)
        return modelling.BertForDiffusionBase.from_dir(str(tmp_path), load_weights=False)

    m = load()
    assert (m.loss_key, m.circle_lambda, m.use_pairwise_dist_loss) == ("smooth_l1", 0.0, 0.0)
    assert m.ft_names == [f"ft{i}" for i in range(6)]       # nothing a caller sees changes with the defaults
    m = load(loss="l1", circle_reg=0.25, use_pdist_loss=[0.05, 0.5, 1000])
    assert (m.loss_key, m.circle_lambda, m.use_pairwise_dist_loss) == ("l1", 0.25, (0.05, 0.5, 1000))
    assert list(losses.pairwise_columns(m.ft_names)) == [0, 1, 2, 3, 4, 5]
    assert load(loss="radian_l1_smooth").loss_key == "smooth_l1"       # the reference's autocorrection
    assert load(use_pdist_loss=0.1).use_pairwise_dist_loss == 0.1
    with pytest.raises(ValueError, match="loss="):
        load(loss="huber")
    m.loss_key, m.circle_lambda, m.use_pairwise_dist_loss = "smooth_l1", 0.3, 0.0      # all three are settable
    assert m.set_loss("l1").use_pairwise_dist_loss == 0.0


def test_loss_terms_names_what_is_missing_before_any_device_call(gv):
    g = _set(gv, "s1")
    batch = {k: torch.from_numpy(g[k]) for k in ("corrupted", "t", "known_noise", "attn_mask", "angles", "lengths",
                                                  "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t")}
    m = _toy_model(ft_names=[str(n) for n in gv["names"]]).set_loss(use_pdist_loss=_pdist_setting(gv))
    short = {k: v for k, v in batch.items() if k != "sqrt_alphas_cumprod_t"}
    with pytest.raises(KeyError, match="sqrt_alphas_cumprod_t"):
        m.loss_terms(short)
    with pytest.raises(KeyError, match="known_noise"):
        _toy_model().loss_terms({k: v for k, v in batch.items() if k != "known_noise"})
    unnamed = _toy_model().set_loss(use_pdist_loss=0.1)     # ft0 .. ft5: none of the six angles
    with pytest.raises(ValueError, match="CA:C:1N"):
        unnamed.loss_terms(batch)
    with pytest.raises(ValueError, match="tau"):
        losses.pairwise_columns(["phi", "psi", "omega", "CA:C:1N", "C:1N:1CA", "d0"])
    with pytest.raises(ValueError, match="disagree"):
        m.loss_terms({**batch, "lengths": batch["lengths"] + 1})
    with pytest.raises(AssertionError):
        losses.pairwise_coef((0.5, 0.05, 1000), batch["t"])      # 0 < min < max, as the reference asserts


# ------------------------------------------------------------ 4. validation_loss with the extra term
class _ToyDset:
    """Six items of lengths 1, 1, 3, 4, 2, 6 at pad 8, two features."""
    dset_key = "angles"
    feature_names = {"angles": ["phi", "d0"]}
    alpha_beta_terms = {"betas": torch.linspace(1e-4, 0.02, 10)}
    lengths = [1, 1, 3, 4, 2, 6]

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        mask = torch.zeros(8)
        mask[: self.lengths[i]] = 1.0
        return {"corrupted": torch.full((8, 2), float(i)), "known_noise": torch.full((8, 2), float(-i)), "t": torch.tensor([i]),
                "attn_mask": mask, "angles": torch.zeros(8, 2), "lengths": torch.tensor(self.lengths[i]),
                "sqrt_alphas_cumprod_t": torch.tensor(0.9), "sqrt_one_minus_alphas_cumprod_t": torch.tensor(0.1),
                "position_ids": torch.arange(8)}


class _StubModel:
    """F + 1 canned terms: feature 0 = the mean item index, feature 1 = 10 x the items, the pairwise term = 100 + the first
    item index, NaN for a batch without pairs."""
    use_pairwise_dist_loss = (0.05, 0.5, 1000)

    def __init__(self):
        self.batches = []

    def prepare(self, betas):
        pass

    def loss_terms(self, batch):
        self.batches.append(batch)
        idx = batch["corrupted"][:, 0, 0]
        n = batch["lengths"]
        pd = 100.0 + float(idx[0]) if int((n * (n - 1) // 2).sum()) else float("nan")
        return torch.tensor([idx.double().mean().item(), 10.0 * len(idx), pd], dtype=torch.float64)


def test_validation_loss_pools_the_pairwise_term_by_pairs():
    m = _StubModel()
    out = validation.validation_loss(m, _ToyDset(), batch_size=2)
    assert set(m.batches[0]) == {"corrupted", "t", "known_noise", "attn_mask", "angles", "lengths", "sqrt_alphas_cumprod_t",
                                 "sqrt_one_minus_alphas_cumprod_t"}
    assert tuple(m.batches[0]["sqrt_alphas_cumprod_t"].shape) == (2,) and tuple(m.batches[0]["lengths"].shape) == (2,)
    npairs, npos = [0, 3 + 6, 1 + 15], [2, 7, 8]
    assert [b["n_pairs"] for b in out["per_batch"]] == npairs and [b["n_positions"] for b in out["per_batch"]] == npos
    terms = [[0.5, 20.0, float("nan")], [2.5, 20.0, 102.0], [4.5, 20.0, 104.0]]
    assert np.array_equal(np.array([b["loss_terms"] for b in out["per_batch"]]), np.array(terms), equal_nan=True)
    # the pairwise value: over all pairs of the pass, a batch without pairs has no weight
    assert out["val_loss_pairwise_dist_loss"] == pytest.approx((102.0 * 9 + 104.0 * 16) / 25, rel=1e-15)
    assert out["val_loss_pairwise_dist_loss"] != pytest.approx((102.0 * 7 + 104.0 * 8) / 15)     # (not by positions)
    assert out["val_loss_phi"] == pytest.approx((0.5 * 2 + 2.5 * 7 + 4.5 * 8) / 17, rel=1e-15)
    # val_loss: over F + 1 values per batch; the reference's mean of a NaN term is NaN
    assert np.isnan(out["per_batch"][0]["val_loss"]) and out["per_batch"][1]["val_loss"] == pytest.approx((2.5 + 20 + 102) / 3)
    one = validation.validation_loss(_StubModel(), _ToyDset(), batch_size=512)
    assert one["val_loss"] == pytest.approx((2.5 + 60.0 + 100.0) / 3) and one["val_loss_pairwise_dist_loss"] == 100.0
    # a model without the term: the four keys and F values, as before
    plain = _StubModel()
    plain.use_pairwise_dist_loss = 0.0
    plain.loss_terms = lambda batch: (plain.batches.append(batch), torch.tensor([1.0, 2.0], dtype=torch.float64))[1]
    out = validation.validation_loss(plain, _ToyDset(), batch_size=4)
    assert set(plain.batches[0]) == {"corrupted", "t", "known_noise", "attn_mask"}
    assert "val_loss_pairwise_dist_loss" not in out and "n_pairs" not in out["per_batch"][0] and out["val_loss"] == 1.5


# ------------------------------------------------------------ 5. the C ABI
def test_new_entries_are_declared_and_exported(lib):
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fd_[a-z_0-9]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/fdmi.h"
        assert name in _binding.exported_symbols(), f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported by libfdmi.so"
    assert lib.fd_abi_version() == _binding.ABI_VERSION == 7   # (additive entries: the version did not move)
    assert f"#define FDMI_PAIRWISE_MAX_LEN {losses.PAIRWISE_MAX_LEN}" in src


def test_new_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Every bad call returns an error code with its word in fd_last_error() and leaves the outputs at the sentinel, on a
    machine without a GPU too.  No valid call is made.  B = 2, L = 6, F = 7."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    B, L, Fn = 2, 6, 7
    z = np.zeros((B, L, Fn), np.float32)
    lens, flags = np.array([6, 2], np.int32), np.ones(Fn, np.uint8)
    checked = 0

    def terms(pred=z, target=z, lens=lens, B=B, L=L, F=Fn, flags=flags, kind=1, ba=0.3, bl=1.0, sums="d", turns="d"):
        sums = np.full((2, Fn), -7.0) if isinstance(sums, str) else sums
        turns = np.full((2, Fn), -7, np.int64) if isinstance(turns, str) else turns
        out = np.full((B if B > 0 else 2, 6, Fn), -7, np.float32)
        rc = lib.fd_loss_terms_ex(0, P(pred), P(target), P(lens), B, L, F, P(flags), kind, C.c_float(ba), C.c_float(bl),
                                  P(sums), P(out), P(turns))
        return [sums, out, turns], rc

    for kw, word in [(dict(pred=None), b"null"), (dict(target=None), b"null"), (dict(lens=None), b"null"), (dict(flags=None), b"null"),
                     (dict(sums=None), b"null"), (dict(B=0), b"B=0"), (dict(L=0), b"L=0"), (dict(F=0), b"F=0"), (dict(F=33), b"F=33"),
                     (dict(kind=2), b"kind=2"), (dict(kind=-1), b"kind=-1"), (dict(ba=0.0), b"beta"), (dict(bl=float("nan")), b"beta"),
                     (dict(lens=np.array([6, 0], np.int32)), b"lens[1]=0"), (dict(lens=np.array([7, 2], np.int32)), b"outside [1, 6]")]:
        outs, rc = terms(**kw)
        msg = lib.fd_last_error()
        assert rc != 0 and msg and word in msg, (kw.keys(), word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    keep, spread, coef = np.array([0.9, 0.8], np.float32), np.array([0.1, 0.2], np.float32), np.array([0.5, 0.25], np.float32)
    idx = np.array([0, 1, 2, 3, 4, 6], np.int32)

    def pairwise(angles=z, corrupted=z, pred=z, keep=keep, spread=spread, coef=coef, lens=lens, B=B, L=L, F=Fn, idx=idx,
                 sums="d", pairs="d", shape=None):
        sums = np.full(2, -7.0) if isinstance(sums, str) else sums
        pairs = np.full(2, -7, np.int64) if isinstance(pairs, str) else pairs
        ca = np.full((2, 2, 6, 3), -7.0)
        if shape is not None:       # (a padded length beyond the kernel's: the arrays must exist at that size)
            angles = corrupted = pred = np.zeros(shape, np.float32)
        rc = lib.fd_pairwise_dist(0, P(angles), P(corrupted), P(pred), P(keep), P(spread), P(coef), P(lens), B, L, F, P(idx),
                                  P(sums), P(pairs), P(ca))
        return [sums, pairs, ca], rc

    rep, low, high = idx.copy(), idx.copy(), idx.copy()
    rep[4], low[2], high[5] = 1, -1, 7
    for kw, word in [(dict(angles=None), b"null"), (dict(corrupted=None), b"null"), (dict(pred=None), b"null"), (dict(keep=None), b"null"),
                     (dict(spread=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(sums=None), b"null"),
                     (dict(pairs=None), b"null"), (dict(B=0), b"B=0"), (dict(F=5), b"F=5"),
                     (dict(L=129, shape=(2, 129, Fn)), b"L=129"), (dict(idx=rep), b"repeats"), (dict(idx=low), b"feat_idx[2]=-1"),
                     (dict(idx=high), b"feat_idx[5]=7"), (dict(keep=np.array([0.9, 0.0], np.float32)), b"keep[1]"),
                     (dict(keep=np.array([float("nan"), 0.5], np.float32)), b"keep[0]"),
                     (dict(coef=np.array([0.5, 0.0], np.float32)), b"coef[1]"), (dict(coef=np.array([-1.0, 0.5], np.float32)), b"coef[0]"),
                     (dict(lens=np.array([0, 2], np.int32)), b"lens[0]=0"), (dict(lens=np.array([6, 7], np.int32)), b"outside [1, 6]")]:
        outs, rc = pairwise(**kw)
        msg = lib.fd_last_error()
        assert rc != 0 and msg and word in msg, (kw.keys(), word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1
    assert checked == 36
    # the model entry checks its model first: a null model is an error code, never a fault
    sums, t = np.full((2, Fn), -7.0), np.zeros(2, np.int32)
    rc = lib.fd_denoise_loss_ex(None, P(z), P(z), P(z), P(t), P(keep), P(spread), P(lens), B, L, 0, C.c_float(0.3), C.c_float(1.0),
                                None, None, P(sums), None, None, None, None, None)
    assert rc != 0 and b"null" in lib.fd_last_error() and (sums == -7).all()
