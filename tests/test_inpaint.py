"""Motif-conditioned sampling, the parts that need no GPU: the level table, the host preparation of ``sampling.inpaint`` /
``sampling.scaffold`` (the device call replaced by a stand-in) and the invariants of the CPU restatement
(tests/inpaint_reference.py) the GPU tests compare against."""
import numpy as np
import pytest
import torch

import inpaint_reference as ipr
from foldingdiff_amd import beta_schedules, datasets, sampling
from oracle import ref_model, ref_sampling

F = 6
PI32 = np.float32(np.pi)


@pytest.mark.parametrize("schedule", ["cosine", "linear", "quadratic"])
def test_inpaint_levels_are_the_float32_alpha_terms_shifted_by_one(schedule):
    T = 37
    got = sampling.inpaint_levels(beta_schedules.get_variance_schedule(schedule, T))
    terms = ref_sampling.alpha_terms(ref_sampling.beta_schedule(schedule, T))
    assert got.dtype == np.float32 and got.shape == (2, T + 1)
    assert got[0, 0] == 1.0 and got[1, 0] == 0.0
    assert np.array_equal(got[0, 1:].view(np.uint32), terms["sqrt_alphas_cumprod"].numpy().view(np.uint32))
    assert np.array_equal(got[1, 1:].view(np.uint32), terms["sqrt_one_minus_alphas_cumprod"].numpy().view(np.uint32))
    assert np.array_equal(got.view(np.uint32), ipr.levels(ref_sampling.beta_schedule(schedule, T)).view(np.uint32))


class _StubModel:
    """What ``inpaint`` asks of a model besides the device call."""
    n_inputs = F
    device = torch.device("cpu")

    def __init__(self):
        self.options, self.prepared = [], None

    def prepare(self, betas, is_angle=None):
        self.prepared = (len(betas), list(is_angle))
        return 0

    def set_option(self, name, value):
        self.options.append((name, value))
        return 0


def _dset(offset=None, pad=16, T=5):
    return datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=pad, mean_offset=offset),
                                        timesteps=T, beta_schedule="cosine")


@pytest.fixture
def device_call(monkeypatch):
    """Replaces the one device call: records its arguments and returns, in every stored state, the known value where an
    element is fixed and the start point elsewhere (what a run leaves in its last row)."""
    calls = []

    def stand_in(h, x0, lens, t_start, known, fixed, coef, seed, out, full_history):
        calls.append(dict(x0=x0.copy(), lens=lens.copy(), t_start=t_start, known=known.copy(), fixed=fixed.copy(), coef=coef.copy(),
                          seed=seed, rows=out.shape[0], full_history=full_history))
        out[:] = np.where(fixed.astype(bool), known, x0)[None]

    monkeypatch.setattr(sampling, "_run_fd_inpaint", stand_in)
    return calls


def _circ_ulps_of_pi(a, b):
    return ref_sampling.circ_dist(a, b).max() / float(np.spacing(PI32))


def test_inpaint_host_preparation(device_call):
    rng = np.random.default_rng(3)
    offset = np.array([0.3, -0.2, 3.0, 1.9, 2.0, 2.1], dtype=np.float32)
    k0 = rng.uniform(-np.pi, np.pi, (7, F)).astype(np.float32)
    k1 = rng.uniform(-np.pi, np.pi, (5, F)).astype(np.float32)
    f0 = np.zeros(7, dtype=bool)          # a [len] mask: whole rows
    f0[2:5] = True
    f1 = np.zeros((5, F), dtype=bool)     # a [len, F] mask: single elements
    f1[0, 3] = f1[4, 0] = f1[2, 5] = True
    k0[~f0] = np.nan                      # NaN where nothing is fixed
    k1[~f1] = np.nan
    model, ds = _StubModel(), _dset(offset)
    torch.manual_seed(11)
    out = sampling.inpaint(model, ds, [k0, k1], [f0, f1])
    assert len(device_call) == 1
    c = device_call[0]
    # the batch: trimmed to the longest item, padded with zeros, lengths as given, the whole schedule, final state only
    assert c["x0"].shape == (2, 7, F) and c["known"].shape == (2, 7, F) and c["fixed"].shape == (2, 7, F)
    assert c["known"].dtype == np.float32 and c["fixed"].dtype == np.uint8 and c["lens"].tolist() == [7, 5]
    assert c["t_start"] == 4 and c["rows"] == 1 and c["full_history"] == 0
    assert np.array_equal(c["coef"], sampling.inpaint_levels(ds.alpha_beta_terms["betas"]))
    want_fixed = np.zeros((2, 7, F), dtype=bool)
    want_fixed[0, 2:5] = True
    want_fixed[1, :5] = f1
    assert np.array_equal(c["fixed"].astype(bool), want_fixed)
    assert np.isfinite(c["known"]).all() and (c["known"][~want_fixed] == 0).all()
    # model space: minus the mean offset, wrapped (the offset 3.0 pushes some angles across -pi)
    data = np.zeros((2, 7, F), dtype=np.float32)
    data[0, :7], data[1, :5] = np.nan_to_num(k0), np.nan_to_num(k1)
    want_known = ipr.wrap32(data - offset)
    assert np.array_equal(c["known"][want_fixed], want_known[want_fixed])
    assert (np.abs(c["known"]) <= PI32).all() and (np.abs(data - offset) > np.pi)[want_fixed].any()
    # the start point is sample_noise's draw of the padded shape, trimmed: the stream sample() consumes
    torch.manual_seed(11)
    assert np.array_equal(c["x0"], ds.sample_noise(torch.zeros(2, 16, F))[:, :7].numpy())
    assert ("varlen", 1) in model.options and model.options[-1] == ("varlen", 0) and model.prepared == (5, [True] * F)
    # back in data space, trimmed: the fixed elements return within 4 ulp of pi (two roundings in, two out)
    assert [o.shape for o in out] == [(7, F), (5, F)]
    assert _circ_ulps_of_pi(out[0][2:5], k0[2:5]) <= 4 and _circ_ulps_of_pi(out[1][f1], k1[f1]) <= 4
    assert (np.abs(out[0]) <= PI32).all()


def test_inpaint_without_offset_keeps_the_bits_and_returns_the_history(device_call):
    rng = np.random.default_rng(4)
    k = rng.uniform(-np.pi, np.pi, (6, F)).astype(np.float32)
    k[3, 2] = PI32                       # no offset: no wrap either, +pi stays +pi
    f = np.zeros((6, F), dtype=bool)
    f[1:4] = True
    model, ds = _StubModel(), _dset(None)
    out = sampling.inpaint(model, ds, [k, k, k], [f, f[:, 0], f], batch_size=2, t_start=2, final_only=False)
    assert [c["lens"].tolist() for c in device_call] == [[6, 6], [6]]              # two batches
    assert all(c["t_start"] == 2 and c["rows"] == 3 and c["full_history"] == 1 for c in device_call)
    assert device_call[0]["seed"] != device_call[1]["seed"]
    assert np.array_equal(device_call[0]["fixed"][0], device_call[0]["fixed"][1])   # [len] mask == the same rows as [len, F]
    for o in out:
        assert o.shape == (3, 6, F)
        assert np.array_equal(o[:, 1:4].view(np.uint32), np.broadcast_to(k[1:4], (3, 3, F)).view(np.uint32))


def test_inpaint_rejects_what_it_cannot_fix(device_call):
    model, ds = _StubModel(), _dset(None)
    k = np.zeros((4, F), dtype=np.float32)
    f = np.ones(4, dtype=bool)
    k[2, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sampling.inpaint(model, ds, [k], [f])
    with pytest.raises(ValueError, match="pads to"):
        sampling.inpaint(model, ds, [np.zeros((17, F), np.float32)], [np.zeros(17, bool)])
    with pytest.raises(AssertionError):
        sampling.inpaint(model, ds, [np.zeros((4, F), np.float32)], [np.zeros((3, F), bool)])
    assert not device_call


def test_scaffold_places_the_motif(device_call):
    rng = np.random.default_rng(5)
    motif = rng.uniform(-3, 3, (4, F)).astype(np.float32)
    model, ds = _StubModel(), _dset(None)
    names = ds.feature_names["angles"]
    tau = names.index("tau")
    out, offs = sampling.scaffold(model, ds, motif, [9, 10, 4])
    assert offs == [2, 3, 0]                                                        # centred: (length - m) // 2
    fx = device_call[0]["fixed"].astype(bool)
    for i, (l, o) in enumerate(zip([9, 10, 4], offs)):
        want = np.zeros((10, F), dtype=bool)
        want[o: o + 4] = True
        if o >= 1:
            want[o - 1, tau] = True    # the N-CA-C angle of the motif's first residue lives in the row before it
            assert device_call[0]["known"][i, o - 1, tau] == motif[0, tau]
        assert np.array_equal(fx[i], want), i
        assert np.array_equal(out[i][o: o + 4].view(np.uint32), motif.view(np.uint32))
        assert out[i].shape == (l, F)
    _, offs = sampling.scaffold(model, ds, motif, [9, 10], offsets=5, pin_lead_angle=False)
    assert offs == [5, 5] and device_call[-1]["fixed"].sum() == 2 * 4 * F
    _, offs = sampling.scaffold(model, ds, motif, [9, 10], offsets=[0, 6])
    assert offs == [0, 6]
    np.random.seed(8)
    _, offs = sampling.scaffold(model, ds, motif, [12] * 40, offsets="random")
    np.random.seed(8)
    assert offs == [int(np.random.randint(0, 9)) for _ in range(40)] and min(offs) == 0 and max(offs) == 8
    for bad in (dict(total_lengths=[3]), dict(total_lengths=[9], offsets=6), dict(total_lengths=[9], offsets="middle")):
        with pytest.raises(ValueError):
            sampling.scaffold(model, ds, motif, **bad)


# ------------------------------------------------------------------ the restatement's own invariants
def _oracle(T=4):
    cfg = ref_model.OracleConfig(hidden_size=32, num_attention_heads=2, intermediate_size=64, layer_norm_eps=1e-12,
                                 num_hidden_layers=1, max_position_embeddings=16, position_embedding_type="relative_key")
    return ref_model.synthetic_model(cfg, (True,) * F, "gaussian_fourier", "mlp", seed=2), ref_sampling.beta_schedule("cosine", T)


def test_restatement_level_zero_returns_the_known_bits():
    rng = np.random.default_rng(6)
    known = rng.uniform(-4, 4, (2, 8, F)).astype(np.float32)
    known[0, 0, :3] = [PI32, -0.0, 1e-30]           # no arithmetic: +pi is not wrapped, the sign of zero survives
    coef = ipr.levels(ref_sampling.beta_schedule("cosine", 4))
    fixed = rng.random((2, 8, F)) < 0.5
    x = rng.standard_normal((2, 8, F)).astype(np.float32)
    got = ipr.replace(x, known, fixed, 0, coef, None, [True] * F)
    assert np.array_equal(got[fixed].view(np.uint32), known[fixed].view(np.uint32))
    assert np.array_equal(got[~fixed].view(np.uint32), x[~fixed].view(np.uint32))
    # a level above zero is the noising statement: rounded products, rounded sum, wrapped
    z = rng.standard_normal((2, 8, F)).astype(np.float32)
    lv = ipr.known_at_level(known, 3, coef, z, [True] * F)
    want = ipr.wrap32(np.float32(coef[0, 3]) * known + np.float32(coef[1, 3]) * z)
    assert np.array_equal(lv.view(np.uint32), want.view(np.uint32)) and (np.abs(lv) <= PI32).all()
    assert not np.array_equal(ipr.known_at_level(known, 3, coef, z, [False] * F), lv)   # the wrap is per feature


def test_restatement_with_nothing_fixed_is_p_sample_loop():
    T = 4
    model, betas = _oracle(T)
    g = torch.Generator().manual_seed(9)
    x0 = ref_sampling.wrap(torch.randn(2, 8, F, generator=g) * 1.5)
    zs = torch.randn(T, 2, 8, F, generator=g)
    lens = [8, 5]
    want = ref_sampling.p_sample_loop(model, lens, x0, T, betas, [True] * F, step_noise=zs).numpy()
    nothing = np.zeros((2, 8, F), dtype=bool)
    known = np.full((2, 8, F), np.nan, dtype=np.float32)
    kz = np.zeros((T + 1, 2, 8, F), dtype=np.float32)
    got = ipr.loop(model, lens, x0.numpy(), T - 1, betas, [True] * F, known, nothing, ipr.levels(betas), zs.numpy(), kz)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and with something fixed, the last row holds known's bits there and every row its own level
    fixed = np.zeros((2, 8, F), dtype=bool)
    fixed[0, 2:5] = True
    known = np.where(fixed, np.float32(0.7), np.float32(np.nan)).astype(np.float32)
    kz = torch.randn(T + 1, 2, 8, F, generator=g).numpy()
    got = ipr.loop(model, lens, x0.numpy(), T - 1, betas, [True] * F, known, fixed, ipr.levels(betas), zs.numpy(), kz)
    assert (got[-1][fixed] == np.float32(0.7)).all() and np.isfinite(got).all()
    for j in range(T):
        lvl = ipr.known_at_level(np.nan_to_num(known), T - 1 - j, ipr.levels(betas), kz[T - 1 - j], [True] * F)
        assert np.array_equal(got[j][fixed].view(np.uint32), lvl[fixed].view(np.uint32))
    assert not np.array_equal(got[-1][~fixed], want[-1][~fixed])   # the free elements feel the fixed ones through the model
