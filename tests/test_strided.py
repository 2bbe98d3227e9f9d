"""Few-step sampling on a strided schedule, the parts that need no GPU: the schedule, the coefficient table, the exported
entries and the host side of ``sampling.sample`` / ``reverse_from`` with the device call replaced by a stand-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import strided_reference as sref
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling

F = 6


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("T,K,t_first", [(1000, 50, None), (1000, 20, None), (1000, 100, 998), (1000, 2, None), (10, 4, None),
                                         (10, 7, None), (8, 3, 6), (1000, 999, None), (1000, 667, None)])
def test_ddim_visits_are_distinct_and_descending(T, K, t_first):
    v = sampling.ddim_visits(T, K, t_first)
    first = T - 1 if t_first is None else t_first
    assert v.dtype == np.int32 and v.shape == (K,)
    assert v[0] == first and v[-1] == 0 and (np.diff(v) < 0).all()
    want = np.floor(np.linspace(first, 0, K) + 0.5).astype(np.int32)
    assert np.array_equal(v, want)


def test_ddim_visits_edge_cases():
    assert sampling.ddim_visits(10, 10).tolist() == list(range(9, -1, -1))        # K = T: every timestep
    assert sampling.ddim_visits(1000, 1000).tolist() == list(range(999, -1, -1))
    assert sampling.ddim_visits(10, 1).tolist() == [9]                            # one visit: straight to level 0
    assert sampling.ddim_visits(10, 1, t_first=0).tolist() == [0]
    # spacing 1 with half-integers in between cannot happen (linspace of integers at spacing 1 is exact), but a spacing
    # just above 1 puts values near x.5: np.round's half-to-even would give 2 for 1.5 and for 2.5
    assert np.round(1.5) == np.round(2.5) == 2
    for T, K in [(4, 3), (6, 3), (6, 5), (8, 5), (12, 9)]:
        v = sampling.ddim_visits(T, K)
        assert len(set(v.tolist())) == K, (T, K, v)
    assert sampling.ddim_visits(4, 3).tolist() == [3, 2, 0]                        # 3, 1.5, 0: floor(1.5 + 0.5) = 2
    for T, K, tf in [(10, 0, None), (10, 11, None), (10, -1, None), (10, 8, 6), (10, 3, 10), (10, 3, -1)]:
        with pytest.raises(ValueError):
            sampling.ddim_visits(T, K, tf)


# ------------------------------------------------------------------ the coefficients
@pytest.mark.parametrize("T", [1000, 10])
@pytest.mark.parametrize("schedule", ["cosine", "linear", "quadratic"])
def test_all_visits_with_eta_one_is_the_ancestral_update(schedule, T):
    """The float64 intermediates against p_sample's own coefficients from the same float64 products."""
    betas = beta_schedules.get_variance_schedule(schedule, T)
    visits = sampling.ddim_visits(T, T)
    got = sampling._ddim_coefficients64(betas, visits, 1.0)
    b = torch.as_tensor(betas).numpy().astype(np.float64)[::-1]                    # visit order: t = T-1 .. 0
    acp = np.concatenate([[1.0], np.cumprod(1.0 - torch.as_tensor(betas).numpy().astype(np.float64))])
    t = visits.astype(np.int64)
    alpha, acp_t, acp_prev = 1.0 - b, acp[t + 1], acp[t]
    want_a = 1.0 / np.sqrt(alpha)
    want_b = -b / (np.sqrt(alpha) * np.sqrt(1.0 - acp_t))
    want_s = np.sqrt(b * (1.0 - acp_prev) / (1.0 - acp_t))
    rel = lambda g, w: float(np.max(np.abs(g - w) / np.abs(w)))   # noqa: E731
    worst = max(rel(got[0], want_a), rel(got[1], want_b), rel(got[2][:-1], want_s[:-1]))
    print(f"{schedule} T={T}: worst relative difference {worst:.2e}")
    np.testing.assert_allclose(got[0], want_a, rtol=1e-10, atol=0)
    np.testing.assert_allclose(got[1], want_b, rtol=1e-10, atol=0)
    np.testing.assert_allclose(got[2][:-1], want_s[:-1], rtol=1e-10, atol=0)
    assert got[2][-1] == 0.0 and want_s[-1] == 0.0                                 # t = 0: posterior_variance_0 = 0


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_coefficient_table_properties_and_bits(eta):
    for T, visits in [(10, [9, 6, 3, 0]), (10, [8, 5, 2, 0]), (8, [7, 4, 2, 0]), (1000, sampling.ddim_visits(1000, 50)),
                      (1000, sampling.ddim_visits(1000, 7, 600)), (10, [5])]:
        betas = beta_schedules.cosine_beta_schedule(T)
        got = sampling.ddim_coefficients(betas, np.asarray(visits, dtype=np.int32), eta)
        assert got.dtype == np.float32 and got.shape == (3, len(visits)) and got.flags["C_CONTIGUOUS"] and np.isfinite(got).all()
        want = sref.coefficients(betas, visits, eta)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (T, visits)
        g64 = sampling._ddim_coefficients64(betas, visits, eta)
        acp = sref.acp_levels(betas)
        assert g64[2, -1] == 0.0                                                   # the last visit lands on level 0: no noise
        np.testing.assert_allclose(g64[0, -1], 1.0 / np.sqrt(acp[int(visits[-1]) + 1]), rtol=1e-14)
        if eta == 0.0:
            assert (g64[2] == 0.0).all() and (got[2] == 0.0).all() and not np.signbit(got[2]).any()
        else:
            assert (g64[2, :-1] > 0).all()
        assert (g64[0] >= 1.0).all() and (g64[1] < 0).all()                        # x is scaled up, the predicted noise taken out


def test_coefficients_reject_bad_input():
    betas = beta_schedules.cosine_beta_schedule(10)
    for visits in ([3, 3, 0], [3, 5], [10, 2], [-1], []):
        with pytest.raises(ValueError):
            sampling.ddim_coefficients(betas, np.asarray(visits, dtype=np.int32), 0.0)
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError):
            sampling.ddim_coefficients(betas, np.asarray([9, 0], dtype=np.int32), eta)


def test_first_visit_conditioning_figures_of_the_design_document():
    """|a| ~ |b| of the visit at t = T - 1 on the cosine schedule, T = 1000: the figures DESIGN.md 6o quotes."""
    betas = beta_schedules.cosine_beta_schedule(1000)
    for K, want in [(20, 5.3e3), (50, 2.0e3), (100, 1.0e3)]:
        c = sampling.ddim_coefficients(betas, sampling.ddim_visits(1000, K), 0.0)
        assert abs(c[0, 0] / want - 1) < 0.02 and abs(-c[1, 0] / want - 1) < 0.02, (K, c[:, 0])
    c = sampling.ddim_coefficients(betas, sampling.ddim_visits(1000, 50, 998), 0.0)  # the lever: start one step lower
    assert c[0, 0] < 200


# ------------------------------------------------------------------ the restatement's own invariants
def test_restatement_update_rounds_once_and_skips_z_where_s_is_zero():
    rng = np.random.default_rng(2)
    x = rng.uniform(-3, 3, (2, 5, F)).astype(np.float32)
    eps = rng.standard_normal((2, 5, F)).astype(np.float32)
    z = rng.standard_normal((2, 5, F)).astype(np.float32)
    a, b, s = np.float32(1.37), np.float32(-0.61), np.float32(0.23)
    got = sref.update(x, eps, a, b, s, z, [False] * F)
    exact = (np.float64(a) * x).astype(np.float32).astype(np.float64) + (np.float64(b) * eps).astype(np.float32)
    want = (exact.astype(np.float32).astype(np.float64) + (np.float64(s) * z).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nan = np.full_like(z, np.nan)
    assert np.array_equal(sref.update(x, eps, a, b, 0.0, nan, [False] * F).view(np.uint32), exact.astype(np.float32).view(np.uint32))
    w = sref.update(x, eps, 4.0, b, s, z, [True, False] * 3)
    assert (np.abs(w[..., 0::2]) <= np.float32(np.pi)).all() and (np.abs(w[..., 1::2]) > np.pi).any()


# ------------------------------------------------------------------ the exported entries
def test_header_binding_and_library_export_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ("fd_sample_strided", "fd_sample_strided_dev", "fd_p_sample_step_coef"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _binding._SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert len(_binding._SIGNATURES["fd_sample_strided"][1]) == 13
    assert len(_binding._SIGNATURES["fd_sample_strided_dev"][1]) == 14
    assert _binding._SIGNATURES["fd_p_sample_step_coef"][1][6:9] == [C.c_float] * 3
    assert lib.fd_abi_version() == _binding.ABI_VERSION
    for name in ("ddim_visits", "ddim_coefficients", "_run_fd_sample_strided"):
        assert hasattr(sampling, name)


def test_null_model_is_an_error_with_a_message(lib):
    x = np.zeros((1, 4, F), dtype=np.float32)
    lens = np.array([4], dtype=np.int32)
    visits = np.array([3, 0], dtype=np.int32)
    coef = np.ones((3, 2), dtype=np.float32)
    out = np.full((1, 4, F), -7.0, dtype=np.float32)
    P = _binding.ptr
    rc = lib.fd_sample_strided(None, P(x), P(lens), 1, 4, P(visits), 2, P(coef), None, C.c_uint64(0), C.c_int64(0), P(out), 0)
    assert rc == -1 and b"null model" in lib.fd_last_error()
    rc = lib.fd_sample_strided_dev(None, P(x), P(lens), 1, 4, P(visits), 2, P(coef), None, C.c_uint64(0), C.c_int64(0), P(out), 0, None)
    assert rc == -1 and b"null model" in lib.fd_last_error()
    rc = lib.fd_p_sample_step_coef(None, P(x), 3, P(lens), 1, 4, 1.0, -1.0, 0.0, None, 1, None, P(out))
    assert rc == -1 and b"null model" in lib.fd_last_error()
    assert (out == -7).all()


# ------------------------------------------------------------------ the host side, the device call replaced
class _StubModel:
    n_inputs = F
    device = torch.device("cpu")

    def __init__(self):
        self.opts = []

    def prepare(self, betas, is_angle=None):
        return 0

    def set_option(self, name, value):
        self.opts.append((name, value))
        return 0


@pytest.fixture
def runners(monkeypatch):
    calls = {"plain": [], "strided": []}

    def plain(h, x0, lens, t_start, zs, seed, seq_offset, out, full_history):
        calls["plain"].append(dict(t_start=t_start, zs=None if zs is None else zs.shape, seed=seed, seq_offset=seq_offset,
                                   rows=out.shape[0], full_history=full_history))
        out[:] = x0[None]

    def strided(h, x0, lens, visits, coef, zs, seed, seq_offset, out, full_history):
        calls["strided"].append(dict(visits=visits.copy(), coef=coef.copy(), zs=None if zs is None else zs.copy(), seed=seed,
                                     seq_offset=seq_offset, rows=out.shape[0], full_history=full_history, lens=lens.copy()))
        out[:] = x0[None]

    monkeypatch.setattr(sampling, "_run_fd_sample", plain)
    monkeypatch.setattr(sampling, "_run_fd_sample_strided", strided)
    return calls


def _dset(T=12, pad=16):
    return datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=pad), timesteps=T, beta_schedule="cosine")


@pytest.mark.parametrize("mode", ["torch", "philox"])
def test_sample_with_num_steps_returns_one_row_per_visit(runners, monkeypatch, mode):
    monkeypatch.setattr(sampling, "NOISE_MODE", mode)
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    torch.manual_seed(5)
    out = sampling.sample(model, ds, n=2, sweep_lengths=(5, 8), final_only=False, num_steps=5, eta=1.0)
    assert [o.shape for o in out] == [(5, l, F) for l in (5, 5, 6, 6, 7, 7)]
    assert len(runners["strided"]) == 1 and not runners["plain"]
    c = runners["strided"][0]
    assert np.array_equal(c["visits"], sampling.ddim_visits(12, 5)) and c["visits"].dtype == np.int32
    assert np.array_equal(c["coef"], sampling.ddim_coefficients(betas, c["visits"], 1.0))
    assert c["rows"] == 5 and c["full_history"] == 1 and c["lens"].tolist() == [5, 5, 6, 6, 7, 7]
    if mode == "torch":
        # one draw of the whole batch shape per visit with s != 0, in visit order, behind the start noise
        torch.manual_seed(5)
        ds.sample_noise(torch.zeros(6, 16, F))
        want = [torch.randn(6, 7, F).numpy() for _ in range(4)]
        assert c["zs"].shape == (5, 6, 7, F) and c["seed"] == 0
        assert all(np.array_equal(c["zs"][i], want[i]) for i in range(4)) and (c["zs"][4] == 0).all()
    else:
        assert c["zs"] is None and c["seed"] > 0
    out = sampling.sample(model, ds, n=1, sweep_lengths=(5, 7), final_only=True, num_steps=5, eta=0.0)
    assert [o.shape for o in out] == [(1, 5, F), (1, 6, F)]
    c = runners["strided"][-1]
    assert c["rows"] == 1 and c["full_history"] == 0 and c["zs"] is None and (c["coef"][2] == 0).all()   # eta = 0 draws nothing
    out = sampling.sample(model, ds, n=1, sweep_lengths=(5, 6), final_only=False, history_every=2, num_steps=5)
    assert out[0].shape == (3, 5, F) and runners["strided"][-1]["full_history"] == 2
    assert ("varlen", 1) in model.opts
    with pytest.raises(ValueError):
        sampling.sample(model, ds, n=1, sweep_lengths=(5, 6), num_steps=13)


def test_num_steps_none_calls_the_old_runner_with_the_old_arguments(runners, monkeypatch):
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    ds, model = _dset(), _StubModel()
    torch.manual_seed(5)
    out = sampling.sample(model, ds, n=1, sweep_lengths=(5, 7), final_only=False)
    assert [o.shape for o in out] == [(12, 5, F), (12, 6, F)]
    assert not runners["strided"] and len(runners["plain"]) == 1
    c = runners["plain"][0]
    assert c["t_start"] == 11 and c["rows"] == 12 and c["full_history"] == 1 and c["zs"] is None and c["seq_offset"] == 0
    x = torch.zeros(2, 6, F)
    sampling.reverse_from(model, x, [6, 4], 6, ds.alpha_beta_terms["betas"])
    assert runners["plain"][-1]["t_start"] == 6 and runners["plain"][-1]["rows"] == 1 and not runners["strided"]


def test_reverse_from_and_p_sample_loop_start_their_schedule_where_the_run_starts(runners, monkeypatch):
    monkeypatch.setattr(sampling, "NOISE_MODE", "torch")
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    x = torch.zeros(2, 6, F)
    got = sampling.reverse_from(model, x, [6, 4], 6, betas, num_steps=3, eta=0.5)
    assert tuple(got.shape) == (2, 6, F)
    c = runners["strided"][-1]
    assert c["visits"].tolist() == [6, 3, 0] and c["rows"] == 1 and c["full_history"] == 0 and c["zs"].shape == (3, 2, 6, F)
    assert np.array_equal(c["coef"], sampling.ddim_coefficients(betas, c["visits"], 0.5))
    traj = sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, num_steps=4)
    assert tuple(traj.shape) == (4, 2, 6, F) and runners["strided"][-1]["visits"].tolist() == [11, 7, 4, 0]
    z = np.zeros((4, 2, 6, F), dtype=np.float32)
    sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, num_steps=4, eta=1.0, step_noise=z, final_only=True)
    assert runners["strided"][-1]["zs"].shape == (4, 2, 6, F) and runners["strided"][-1]["rows"] == 1
    with pytest.raises(AssertionError):
        sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, num_steps=4, step_noise=np.zeros((12, 2, 6, F), np.float32))
    assert not runners["plain"]


def test_scripts_have_the_two_flags():
    import importlib.util
    for script, base in [("sample.py", ["-m", "x"]), ("partial_noise_reconstruct.py", ["a.pdb", "out.json", "-m", "x"])]:
        spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(REPO, "bin", script))
        cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cli)
        args = cli.build_parser().parse_args(base)
        assert args.num_steps is None and args.eta == 0.0
        args = cli.build_parser().parse_args(base + ["--num_steps", "50", "--eta", "0.5"])
        assert args.num_steps == 50 and args.eta == 0.5
