"""
The denoising loss on the device (needs an MI355X: pytest -m gpu): the forward with one timestep per sequence against
the CPU oracle, the noising and loss kernels against the reference's golden fixture (tests/golden/ref_loss.npz), and the
whole of ``BertForDiffusionBase.loss_terms`` against the reference's ``_get_loss_terms``.

Tolerances:
  * forward eps:          max|d| <= 1e-5 against the fp32 oracle, the project's forward gate (test_gpu_parity.py)
  * per-position terms:   <= 1e-6 absolute against the reference's terms (a term is at most about pi and takes five fp32
                          roundings of 6e-8 relative each); the aim is 0 -- the maximum is printed and recorded
  * per-sequence sums:    relative 1e-12 against an fp64 numpy sum of the kernel's own terms (at most 512 fp64 additions
                          of 1.1e-16 relative each, in another order)
  * the six loss terms:   <= 1.2e-5 against the reference: a term is 1-Lipschitz in the predicted noise (both branches,
                          and across the +-pi seam), so the forward's 1e-5 carries over, plus 2e-6 for the loss's own fp32
                          arithmetic and the reference's fp32 mean
  * same bits in, same kernels: bit-exact
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import golden
from foldingdiff_amd import _binding, beta_schedules, datasets, losses, modelling
from oracle import ref_model, ref_sampling

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
TERM_TOL = 1e-6
SUM_RTOL = 1e-12
LOSS_TOL = 1.2e-5
REPORT = {}


def _record(name, **kw):
    """Every measured figure is printed before its assertion (pytest -s shows them)."""
    REPORT[name] = {k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kw.items()}
    print(name, json.dumps(REPORT[name], sort_keys=True))


def _pair(hidden, heads, pos="relative_key", time_encoding="gaussian_fourier", precision="f32", maxpos=128, seed=0,
          ft=(True,) * 6):
    """(fp32 oracle, product model on cuda:0) with identical synthetic weights: 2 layers, intermediate size 2 x hidden."""
    ocfg = ref_model.OracleConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                  num_hidden_layers=2, max_position_embeddings=maxpos, position_embedding_type=pos)
    o32 = ref_model.synthetic_model(ocfg, ft, time_encoding, "mlp", seed=seed)
    pcfg = modelling.BertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                num_hidden_layers=2, max_position_embeddings=maxpos, position_embedding_type=pos)
    pm = modelling.BertForDiffusionBase(pcfg, list(ft), time_encoding=time_encoding, decoder="mlp")
    pm.load_state_dict(o32.state_dict())
    pm.to("cuda:0")
    pm.set_precision(precision)
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    return o32, pm


def _mask(lens, L):
    m = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        m[i, :n] = 1.0
    return m


def _inputs(B, L, F=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ref_sampling.wrap(torch.randn(B, L, F, generator=g) * 1.5)


SHAPES = [(33, [33, 1, 32, 8, 9]), (128, [128, 1, 100, 64, 65])]
T_MIXED = [0, 999, 517, 517, 3]


# ------------------------------------------------------------ 1. one timestep per sequence against the oracle
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("L,lens", SHAPES)
@pytest.mark.parametrize("hidden,heads", [(192, 6), (384, 12)])
def test_forward_mixed_t_against_the_oracle(gpu, hidden, heads, L, lens, precision):
    """L = 33 exercises the 8-row padding of the row image; the repeated timestep and both ends of the table are the
    places an index can go wrong.  f16x3 also with the fused attention (where the kernel takes the shape) and the fused
    layer tail forced on: they must see the same hidden state."""
    o32, pm = _pair(hidden, heads, precision=precision, seed=hidden + L)
    x, mask, t = _inputs(len(lens), L, seed=L), _mask(lens, L), torch.tensor(T_MIXED)
    want = o32(x, t, attention_mask=mask).numpy()
    modes = [{}]
    if precision == "f16x3":
        if _binding.load().fd_fused_attn_supported(pm._ensure_handle(), L):
            modes.append({"fuse_attn": 1})
        modes.append({"fuse_ffn": 2})
    for opts in modes:
        for k, v in opts.items():
            pm.set_option(k, v)
        got = pm.forward_mixed_t(x, t, mask).numpy()
        for k in opts:
            pm.set_option(k, -1)
        err = np.abs(got.astype(np.float64) - want).max()
        _record(f"fwd_t_d{hidden}_L{L}_{precision}_{'_'.join(f'{k}{v}' for k, v in opts.items()) or 'auto'}", max=err)
        assert err <= FWD_TOL, (opts, err)
    # the per-launch path (one forward per distinct timestep) is the same function of the same inputs
    assert np.abs(pm(x, t, attention_mask=mask).numpy().astype(np.float64) - want).max() <= FWD_TOL


@pytest.mark.parametrize("pos,time_encoding", [("absolute", "gaussian_fourier"), ("relative_key", "sinusoidal")])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_forward_mixed_t_absolute_positions_and_sinusoidal_time(gpu, pos, time_encoding, precision):
    L, lens = SHAPES[0]
    o32, pm = _pair(192, 6, pos=pos, time_encoding=time_encoding, precision=precision, seed=7)
    x, mask, t = _inputs(len(lens), L, seed=3), _mask(lens, L), torch.tensor(T_MIXED)
    err = np.abs(pm.forward_mixed_t(x, t, mask).numpy().astype(np.float64) - o32(x, t, attention_mask=mask).numpy()).max()
    _record(f"fwd_t_{pos}_{time_encoding}_{precision}", max=err)
    assert err <= FWD_TOL


# ------------------------------------------------------------ 2. same launches, same bits
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_equal_timesteps_give_forwards_bits_and_reversal_reverses(gpu, precision):
    L, lens = SHAPES[1]
    _, pm = _pair(192, 6, precision=precision, seed=11)
    x, mask = _inputs(len(lens), L, seed=5), _mask(lens, L)
    for tv in (0, 517, 999):
        t = torch.full((len(lens),), tv, dtype=torch.long)
        assert torch.equal(pm.forward_mixed_t(x, t, mask), pm(x, t, attention_mask=mask)), tv
    t = torch.tensor(T_MIXED)
    fwd = pm.forward_mixed_t(x, t, mask)
    rev = pm.forward_mixed_t(x.flip(0), t.flip(0), mask.flip(0))
    assert torch.equal(rev.flip(0), fwd)
    with pytest.raises(ValueError, match="forward"):   # a mask with a hole: forward() takes it, this entry says so
        holed = mask.clone()
        holed[0, 5] = 0.0
        pm.forward_mixed_t(x, t, holed)


# ------------------------------------------------------------ fixtures of the golden batch
@pytest.fixture(scope="module")
def gl():
    return golden("ref_loss.npz")


@pytest.fixture(scope="module")
def abs_model(gl):
    """The absolute-position model of ref_abs_model.npz with the fixture's angular flags, default precision."""
    gm = golden("ref_abs_model.npz")
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                               max_position_embeddings=64, position_embedding_type="absolute")
    pm = modelling.BertForDiffusionBase(cfg, [bool(a) for a in gl["ft_is_angular"]])
    pm.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")})
    pm.to("cuda:0")
    pm.prepare(beta_schedules.cosine_beta_schedule(int(gl["T"])))
    return pm


def _golden_batch(gl):
    return {k: torch.from_numpy(gl[k]) for k in ("corrupted", "t", "known_noise", "attn_mask")}


class _ToyAngles:
    def __init__(self, gl):
        self.angles, self.lengths, self.pad = torch.from_numpy(gl["angles"]), gl["lengths"].tolist(), int(gl["pad"])
        self.feature_names = {"angles": ["phi", "psi", "omega", "tau", "d0", "d1"]}
        self.feature_is_angular = {"angles": [bool(a) for a in gl["ft_is_angular"]]}

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, index, ignore_zero_center=False):
        mask = torch.zeros(self.pad)
        mask[: self.lengths[index]] = 1.0
        return {"angles": self.angles[index].clone(), "attn_mask": mask}


# ------------------------------------------------------------ 3. q_sample
def test_device_noising_has_the_bits_of_the_reference_and_of_the_host_dataset(gpu, gl, abs_model):
    x0, mask = torch.from_numpy(gl["angles"]), torch.from_numpy(gl["attn_mask"])
    keep, spread = torch.from_numpy(gl["sqrt_alphas_cumprod_t"]), torch.from_numpy(gl["sqrt_one_minus_alphas_cumprod_t"])
    _, extra = abs_model.denoise_loss_sums(x0, torch.from_numpy(gl["known_noise"]), torch.from_numpy(gl["t"]), mask,
                                           keep=keep, spread=spread, return_corrupted=True)
    assert extra["corrupted"].dtype == np.float32
    assert np.array_equal(extra["corrupted"], gl["corrupted"])   # every position of the pad, masked ones included
    # ... and the product's own host dataset on the same seed draws the same noise and noises to the same bits
    ds = datasets.NoisedAnglesDataset(_ToyAngles(gl), dset_key="angles", timesteps=int(gl["T"]), beta_schedule="cosine")
    torch.manual_seed(int(gl["seed"]))
    items = [ds.__getitem__(i, use_t_val=int(t)) for i, t in enumerate(gl["timesteps"])]
    noise = torch.stack([it["known_noise"] for it in items])
    assert np.array_equal(noise.numpy(), gl["known_noise"])
    _, again = abs_model.denoise_loss_sums(
        x0, noise, torch.stack([it["t"] for it in items]), mask, keep=torch.stack([it["sqrt_alphas_cumprod_t"] for it in items]),
        spread=torch.stack([it["sqrt_one_minus_alphas_cumprod_t"] for it in items]), return_corrupted=True)
    assert np.array_equal(again["corrupted"], torch.stack([it["corrupted"] for it in items]).numpy())


# ------------------------------------------------------------ 4. the loss arithmetic in isolation
def _check_sums(name, sums, terms):
    want = terms.astype(np.float64).sum(axis=1)
    rel = np.abs(sums - want).max() / max(np.abs(want).max(), 1e-300)
    _record(name + "_sums", max_rel=rel)
    assert np.all(np.abs(sums - want) <= SUM_RTOL * np.maximum(np.abs(want), 1e-300)), rel


def test_loss_terms_on_the_golden_batch(gpu, gl):
    lens, ang = gl["lengths"].astype(np.int32), [bool(a) for a in gl["ft_is_angular"]]
    sums, terms = losses.loss_terms(gl["pred"], gl["known_noise"], lens, ang)
    want = gl["terms"] * gl["attn_mask"][:, :, None]
    err = np.abs(terms.astype(np.float64) - want).max()
    _record("terms_golden", max=err, bit_equal=bool(np.array_equal(terms, want)))
    assert err <= TERM_TOL
    assert not terms[gl["attn_mask"] == 0].any()
    _check_sums("terms_golden", sums, terms)
    # the reference's six numbers from its own predicted noise: only the summation order and the mean's precision differ
    got = sums.sum(axis=0) / lens.sum()
    assert np.abs(got - gl["ref_loss_terms"]).max() <= 2e-6
    # a mask in place of the lengths, and sums alone
    assert np.array_equal(losses.loss_terms(gl["pred"], gl["known_noise"], gl["attn_mask"], ang, return_terms=False), sums)


def test_loss_terms_at_the_seam_and_the_thresholds_all_lengths(gpu, gl):
    """Differences within 1e-3 of +-pi and of +-beta on both sides (the fixture's synthetic set, terms by the reference's
    functions), tiled over sequences of lengths 1, 7, 63, 64, 65, 129 and 512 at L = 512 with mixed angular flags."""
    lens = np.array([1, 7, 63, 64, 65, 129, 512], np.int32)
    flags = [True, False, True, True, False, True]
    B, L, F, n = len(lens), 512, 6, len(gl["syn_pred"])
    idx = (np.arange(L * F).reshape(1, L, F) + 13 * np.arange(B).reshape(B, 1, 1)) % n
    pred, target = gl["syn_pred"][idx], gl["syn_target"][idx]
    want = np.where(np.array(flags)[None, None, :], gl["syn_terms_ang"][idx], gl["syn_terms_lin"][idx]).astype(np.float32)
    want = want * (np.arange(L)[None, :, None] < lens[:, None, None])
    sums, terms = losses.loss_terms(pred, target, lens, flags)
    err = np.abs(terms.astype(np.float64) - want).max()
    _record("terms_synthetic", max=err, bit_equal=bool(np.array_equal(terms, want)))
    assert err <= TERM_TOL
    _check_sums("terms_synthetic", sums, terms)
    # run to run, and wherever a sequence sits in the batch: the same bits
    sums2, terms2 = losses.loss_terms(pred, target, lens, flags)
    assert np.array_equal(sums2, sums) and np.array_equal(terms2, terms)
    perm = np.array([4, 6, 0, 2, 5, 1, 3])
    sums3 = losses.loss_terms(pred[perm], target[perm], lens[perm], flags, return_terms=False)
    assert np.array_equal(sums3, sums[perm])


@pytest.mark.parametrize("F", [1, 32])
def test_loss_terms_feature_counts_at_both_ends(gpu, F):
    """F = 1 (256 lanes on one feature) and F = 32 (8 lanes per feature, the most the entry takes), against the host
    restatement of the reference's functions."""
    g = torch.Generator().manual_seed(F)
    lens, L = np.array([300, 1, 77], np.int32), 300
    pred, target = torch.randn(3, L, F, generator=g) * 2, torch.randn(3, L, F, generator=g) * 2
    flags = [f % 3 != 1 for f in range(F)]
    want = losses.host_terms(pred, target, flags).numpy() * (np.arange(L)[None, :, None] < lens[:, None, None])
    sums, terms = losses.loss_terms(pred, target, lens, flags)
    err = np.abs(terms.astype(np.float64) - want).max()
    _record(f"terms_F{F}", max=err, bit_equal=bool(np.array_equal(terms, want)))
    assert err <= TERM_TOL
    _check_sums(f"terms_F{F}", sums, terms)


# ------------------------------------------------------------ 5. end to end against the reference
def test_loss_terms_of_the_golden_batch_against_the_reference(gpu, gl, abs_model):
    batch = _golden_batch(gl)
    got = abs_model.loss_terms(batch)
    assert got.shape == (6,)
    err = np.abs(got.numpy() - gl["ref_loss_terms"].astype(np.float64)).max()
    _record("loss_terms_vs_reference", max=err, got=[float(v) for v in got], want=[float(v) for v in gl["ref_loss_terms"]])
    assert err <= LOSS_TOL
    # the predicted noise itself, for the record of where the difference comes from
    sums, extra = abs_model.denoise_loss_sums(batch["corrupted"], batch["known_noise"], batch["t"], batch["attn_mask"], return_eps=True)
    _record("loss_batch_eps_vs_reference", max=np.abs(extra["eps"].astype(np.float64) - gl["pred"]).max())
    # the same batch from x0 + noise, noised on the device: the same bits into the same kernels
    keep, spread = torch.from_numpy(gl["sqrt_alphas_cumprod_t"]), torch.from_numpy(gl["sqrt_one_minus_alphas_cumprod_t"])
    sums2 = abs_model.denoise_loss_sums(torch.from_numpy(gl["angles"]), batch["known_noise"], batch["t"], batch["attn_mask"],
                                        keep=keep, spread=spread)
    got2 = sums2.sum(axis=0) / int(gl["lengths"].sum())
    assert np.all(np.abs(got2 - got.numpy()) <= 1e-12 * np.abs(got.numpy()))
    # the forward inside it is forward_mixed_t's
    eps = abs_model.forward_mixed_t(batch["corrupted"], batch["t"], batch["attn_mask"]).numpy()
    assert np.array_equal(eps, extra["eps"])
    want_sums = losses.loss_terms(eps, gl["known_noise"], gl["attn_mask"], [bool(a) for a in gl["ft_is_angular"]], return_terms=False)
    assert np.array_equal(sums, want_sums)


# ------------------------------------------------------------ 6. argument errors
def test_model_entries_return_error_codes_for_bad_timesteps_and_lengths(gpu, gl, abs_model):
    lib, h = _binding.load(), abs_model._ensure_handle()
    P = _binding.ptr
    B, L, F = gl["corrupted"].shape
    x, noise, lens = gl["corrupted"].copy(), gl["known_noise"].copy(), gl["lengths"].astype(np.int32)
    T = int(gl["T"])
    good_t = gl["t"].reshape(-1).astype(np.int32)
    ba, bl = C.c_float(losses.ANGULAR_BETA), C.c_float(1.0)

    def fwd(t=good_t, L=L):
        out = np.full((B, L, F), -7, np.float32)
        xx = np.zeros((B, L, F), np.float32)
        return out, lib.fd_forward_t(h, P(xx), P(t), P(lens), B, L, P(out))

    def loss(t=good_t, L=L, keep=None, spread=None):
        sums = np.full((B, F), -7.0)
        xx = np.zeros((B, L, F), np.float32)
        return sums, lib.fd_denoise_loss(h, P(xx), P(xx), P(t), P(keep), P(spread), P(lens), B, L, ba, bl, P(sums), None, None)

    bad_hi, bad_lo = good_t.copy(), good_t.copy()
    bad_hi[3], bad_lo[1] = T, -1
    for call in (fwd, loss):
        for kw, word in [(dict(t=bad_hi), b"t[3]=1000"), (dict(t=bad_lo), b"t[1]=-1"), (dict(t=None), b"null"),
                         (dict(L=65), b"max_position_embeddings")]:
            out, rc = call(**kw)
            msg = lib.fd_last_error()
            assert rc == -1 and word in msg, (call.__name__, word, rc, msg)
            assert (out == -7).all()
    out, rc = loss(keep=np.ones(B, np.float32))
    assert rc == -1 and b"keep and spread" in lib.fd_last_error() and (out == -7).all()
    # the model still works afterwards
    assert fwd()[1] == 0 and loss()[1] == 0
