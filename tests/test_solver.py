"""Few-step sampling with the second-order multistep solver, the parts that need no GPU: the log-SNR visit rule, the
coefficient table, the order of the method on an analytic case, the restatement's own invariants, the exported entries and
the host side of the Python samplers with the device call replaced by a stand-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import solver_reference as vref
import strided_reference as sref
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling

F = 6
SCHEDULES = ["cosine", "linear", "quadratic"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the visits
def test_logsnr_visits_pinned_example():
    betas = beta_schedules.cosine_beta_schedule(1000)
    v = sampling.logsnr_visits(betas, 10)
    assert v.dtype == np.int32 and v.tolist() == [999, 925, 830, 639, 376, 174, 71, 24, 4, 0]
    # without the clip four of the ten visits go to t = 999 .. 996: why lambda_min exists
    assert sampling.logsnr_visits(betas, 10, lambda_min=None)[:4].tolist() == [999, 998, 997, 996]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("T,K,t_first,lambda_min", [(1000, 10, None, -3.0), (1000, 20, None, None), (1000, 40, 998, -2.0), (1000, 2, None, -3.0),
                                                    (1000, 999, None, -3.0), (1000, 500, 600, -5.0), (10, 4, None, -3.0), (10, 7, None, None),
                                                    (10, 9, None, 0.5), (8, 3, 6, -4.0), (10, 6, 5, 100.0)])
def test_logsnr_visits_are_strictly_descending_from_t_first_to_zero(schedule, T, K, t_first, lambda_min):
    betas = beta_schedules.get_variance_schedule(schedule, T)
    v = sampling.logsnr_visits(betas, K, t_first, lambda_min)
    first = T - 1 if t_first is None else t_first
    assert v.dtype == np.int32 and v.shape == (K,)
    assert v[0] == first and v[-1] == 0 and (np.diff(v) < 0).all()


def test_logsnr_visits_edge_cases():
    for schedule in SCHEDULES:
        betas = beta_schedules.get_variance_schedule(schedule, 10)
        assert sampling.logsnr_visits(betas, 10).tolist() == list(range(9, -1, -1))          # K = t_first + 1: every timestep
        assert sampling.logsnr_visits(betas, 7, t_first=6).tolist() == list(range(6, -1, -1))
        assert sampling.logsnr_visits(betas, 1).tolist() == [9]                              # one visit: straight to level 0
        assert sampling.logsnr_visits(betas, 1, t_first=0).tolist() == [0]
        assert sampling.logsnr_visits(betas, 1, t_first=4, lambda_min=None).tolist() == [4]
    betas = beta_schedules.cosine_beta_schedule(1000)
    assert sampling.logsnr_visits(betas, 1000).tolist() == list(range(999, -1, -1))
    for K, tf, lm in [(0, None, -3.0), (1001, None, -3.0), (-1, None, -3.0), (8, 6, -3.0), (3, 1000, -3.0), (3, -1, -3.0),
                      (5, None, float("nan")), (5, None, float("inf")), (5, None, float("-inf"))]:
        with pytest.raises(ValueError):
            sampling.logsnr_visits(betas, K, tf, lm)


def test_logsnr_visits_follow_the_stated_rule():
    """The rule of the docstring, written out again: nearest timestep per target, ends pinned, two passes."""
    betas = beta_schedules.get_variance_schedule("linear", 1000)
    acp = np.array(sref.acp_levels(betas))
    lam = 0.5 * (np.log(acp[1:]) - np.log1p(-acp[1:]))
    for K, tf, lm in [(10, 999, -3.0), (25, 700, None), (40, 999, -4.0)]:
        hi = lam[tf] if lm is None else max(lam[tf], lm)
        v = [int(np.argmin(np.abs(lam[: tf + 1] - tg))) for tg in np.linspace(hi, lam[0], K)]
        v[0], v[-1] = tf, 0
        for i in range(1, K):
            v[i] = min(v[i], v[i - 1] - 1)
        v[-1] = max(v[-1], 0)
        for i in range(K - 2, -1, -1):
            v[i] = max(v[i], v[i + 1] + 1)
        assert sampling.logsnr_visits(betas, K, tf, lm).tolist() == v


# ------------------------------------------------------------------ the coefficients
def _visit_sets(betas, T):
    if T == 1000:
        return [sampling.logsnr_visits(betas, 10), sampling.logsnr_visits(betas, 20, lambda_min=None), sampling.ddim_visits(T, 40),
                sampling.logsnr_visits(betas, 7, t_first=600)]
    return [np.array([8, 5, 2, 0], dtype=np.int32), sampling.ddim_visits(T, T), np.array([9, 7, 4, 3, 1, 0], dtype=np.int32),
            np.array([5], dtype=np.int32), np.array([9, 0], dtype=np.int32)]


@pytest.mark.parametrize("T", [1000, 10])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_coefficient_table_properties_and_agreement_with_the_restatement(schedule, T):
    betas = beta_schedules.get_variance_schedule(schedule, T)
    for visits in _visit_sets(betas, T):
        K = len(visits)
        coef = sampling.solver_coefficients(betas, visits)
        assert coef.dtype == np.float32 and coef.shape == (5, K) and coef.flags["C_CONTIGUOUS"] and np.isfinite(coef).all()
        assert np.array_equal(_bits(coef[:2]), _bits(sampling.ddim_coefficients(betas, visits, 0.0)[:2]))   # a | b: DDIM's bits
        assert coef[2, 0] == 0 and coef[2, K - 1] == 0
        assert (coef[2, 1:K - 1] > 0).all()                      # descending visits: h, h_prev > 0
        first = sampling.solver_coefficients(betas, visits, order=1)
        assert (first[2] == 0).all() and np.array_equal(_bits(first[[0, 1, 3, 4]]), _bits(coef[[0, 1, 3, 4]]))
        got, want = sampling._solver_coefficients64(betas, visits), vref.coefficients64(betas, visits)
        assert np.allclose(got, want, rtol=1e-10, atol=0.0), (schedule, T, visits)
        assert np.array_equal(_bits(coef), _bits(got.astype(np.float32)))                                    # rounded once
        assert np.allclose(sampling._solver_coefficients64(betas, visits, 1), vref.coefficients64(betas, visits, 1), rtol=1e-10, atol=0.0)


def test_coefficients_reject_bad_input():
    betas = beta_schedules.cosine_beta_schedule(10)
    for visits in ([], [3, 3, 0], [3, 5, 0], [10, 3, 0], [3, -1]):
        with pytest.raises(ValueError):
            sampling.solver_coefficients(betas, visits)
    for order in (0, 3):
        with pytest.raises(ValueError):
            sampling.solver_coefficients(betas, [8, 5, 2, 0], order=order)


def test_figures_the_documents_quote():
    """the bounds of the free-running GPU test's table, and the conditioning of a cosine T = 1000 run's first visit."""
    betas = beta_schedules.cosine_beta_schedule(10)
    coef = sampling.solver_coefficients(betas, [8, 5, 2, 0])
    assert np.abs(coef).max() <= 6.5 and np.abs(coef[2]).max() <= 0.38
    betas = beta_schedules.cosine_beta_schedule(1000)
    coef = sampling.solver_coefficients(betas, sampling.logsnr_visits(betas, 10))
    assert 1e4 < coef[3, 0] < 1e5 and abs(coef[3, 0] / -coef[4, 0] - 1) < 1e-6       # u ~ -v ~ 1 / alpha_T
    assert 0 < coef[2, 1] < 0.01 and np.abs(coef[2]).max() < 0.3                      # it enters visit 1 through c wrap(d) only


# ------------------------------------------------------------------ the order of the method
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_second_order_on_the_analytic_gaussian_case(schedule):
    """Data that is Gaussian per element (m = 0.3, s0 = 0.5): the optimal eps and the end point of the probability-flow ODE
    are closed forms.  float64, no wrapping, 64 elements drawn at level T = 1000, on logsnr_visits.  The second-order error
    is at most a quarter of the first-order error on the same visits (measured 6.2 x at worst, cosine K = 20 without a
    clip), and below 5e-3 at K = 40 with lambda_min = -3 (measured 1.8e-3 .. 2.0e-3).  A wrong c passes every
    device-against-restatement test; this one it does not pass."""
    T = 1000
    betas = beta_schedules.get_variance_schedule(schedule, T)
    acp = vref.acp_levels(betas)
    rng = np.random.default_rng(0)
    x_start = np.sqrt(acp[T]) * 0.3 + np.sqrt(acp[T] * 0.25 + 1.0 - acp[T]) * rng.standard_normal(64)
    end = np.array([vref.gaussian_ode_end(x, acp[T]) for x in x_start])
    for lambda_min in (None, -3.0):
        for K in (10, 20, 40):
            visits = sampling.logsnr_visits(betas, K, lambda_min=lambda_min)
            e2 = np.abs(vref.gaussian_run(betas, visits, sampling._solver_coefficients64(betas, visits, 2), x_start) - end).max()
            e1 = np.abs(vref.gaussian_run(betas, visits, sampling._solver_coefficients64(betas, visits, 1), x_start) - end).max()
            print(f"{schedule} lambda_min={lambda_min} K={K}: first order {e1:.3g}, second order {e2:.3g}, ratio {e1 / e2:.1f}")
            assert e2 <= e1 / 4, (schedule, lambda_min, K, e1, e2)
            if K == 40 and lambda_min is not None:
                assert e2 < 5e-3, (schedule, e2)
    # the restatement's own table gives the same run (the two tables agree to 1e-10)
    visits = sampling.logsnr_visits(betas, 20)
    r1 = vref.gaussian_run(betas, visits, sampling._solver_coefficients64(betas, visits), x_start)
    r2 = vref.gaussian_run(betas, visits, vref.coefficients64(betas, visits), x_start)
    assert np.abs(r1 - r2).max() < 1e-9


# ------------------------------------------------------------------ the restatement's own invariants
def test_restatement_rounds_once_and_does_not_read_prev_where_c_is_zero():
    rng = np.random.default_rng(2)
    x = rng.uniform(-3, 3, (2, 5, F)).astype(np.float32)
    eps = rng.standard_normal((2, 5, F)).astype(np.float32)
    prev = rng.uniform(-3, 3, (2, 5, F)).astype(np.float32)
    a, b, c, u, v = (np.float32(k) for k in (1.37, -0.61, 0.23, 1.9, -1.1))
    f64, f32 = np.float64, np.float32
    m = ((f64(a) * x).astype(f32).astype(f64) + (f64(b) * eps).astype(f32)).astype(f32)
    x0 = ((f64(u) * x).astype(f32).astype(f64) + (f64(v) * eps).astype(f32)).astype(f32)
    d = (x0.astype(f64) - prev).astype(f32)
    want = (m.astype(f64) + (f64(c) * d).astype(f32)).astype(f32)
    got, got0 = vref.update(x, eps, prev, a, b, c, u, v, [False] * F)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got0), _bits(x0))
    nan = np.full_like(prev, np.nan)
    for p in (nan, None):
        got, got0 = vref.update(x, eps, p, a, b, 0.0, u, v, [True, False] * 3)
        assert np.isfinite(got).all() and np.array_equal(_bits(got0), _bits(vref.update(x, eps, prev, a, b, c, u, v, [True, False] * 3)[1]))
        assert np.array_equal(_bits(got), _bits(sref.update(x, eps, a, b, 0.0, None, [True, False] * 3)))   # the strided statement
    w, w0 = vref.update(x, eps, prev, 4.0, b, c, 3.0, v, [True, False] * 3)
    assert (np.abs(w[..., 0::2]) <= f32(np.pi)).all() and (np.abs(w[..., 1::2]) > np.pi).any()
    assert (np.abs(w0[..., 0::2]) <= f32(np.pi)).all() and (np.abs(w0[..., 1::2]) > np.pi).any()


def test_restatement_wraps_the_difference():
    """x0 = 3.1 and prev = -3.1 are 0.083 apart on the circle and 6.2 apart as numbers: the move is c times the short way round."""
    x = np.full((1, 1, 2), 3.1, dtype=np.float32)
    eps = np.zeros_like(x)
    prev = np.full_like(x, -3.1)
    c = np.float32(0.25)
    out, x0 = vref.update(x, eps, prev, 1.0, 0.0, c, 1.0, 0.0, [True, False])
    short = np.float32(3.1) - np.float32(-3.1) - np.float32(2 * np.pi)
    assert abs(x0[0, 0, 0] - 3.1) < 1e-6 and x0[0, 0, 1] == np.float32(3.1) and abs(short + 0.0832) < 1e-3   # (the wrap itself rounds)
    assert abs(out[0, 0, 0] - (np.float32(3.1) + c * short)) < 1e-6                 # angular: 3.1 - 0.0208
    assert abs(out[0, 0, 1] - (np.float32(3.1) + c * np.float32(6.2))) < 1e-6       # not angular: the difference as it is


# ------------------------------------------------------------------ the exported entries
def test_header_binding_and_library_export_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ("fd_sample_solver", "fd_sample_solver_dev", "fd_p_sample_step_solver"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _binding._SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
        declared = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(declared.split(",")) == len(_binding._SIGNATURES[name][1]), name
    assert len(_binding._SIGNATURES["fd_sample_solver"][1]) == 10
    assert len(_binding._SIGNATURES["fd_sample_solver_dev"][1]) == 11
    assert _binding._SIGNATURES["fd_p_sample_step_solver"][1][6:11] == [C.c_float] * 5
    assert lib.fd_abi_version() == _binding.ABI_VERSION == 7
    for name in ("logsnr_visits", "solver_coefficients", "_run_fd_sample_solver", "_run_fd_sample_solver_device"):
        assert hasattr(sampling, name)


def test_null_model_is_an_error_with_a_message(lib):
    x = np.zeros((1, 4, F), dtype=np.float32)
    lens = np.array([4], dtype=np.int32)
    visits = np.array([3, 0], dtype=np.int32)
    coef = np.ones((5, 2), dtype=np.float32)
    coef[2] = 0
    out = np.full((1, 4, F), -7.0, dtype=np.float32)
    P = _binding.ptr
    rc = lib.fd_sample_solver(None, P(x), P(lens), 1, 4, P(visits), 2, P(coef), P(out), 0)
    assert rc == -1 and b"null model" in lib.fd_last_error()
    rc = lib.fd_sample_solver_dev(None, P(x), P(lens), 1, 4, P(visits), 2, P(coef), P(out), 0, None)
    assert rc == -1 and b"null model" in lib.fd_last_error()
    rc = lib.fd_p_sample_step_solver(None, P(x), 3, P(lens), 1, 4, 1.0, -1.0, 0.0, 1.0, -1.0, None, 1, None, P(out), P(out))
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
    calls = {"plain": [], "strided": [], "solver": []}

    def plain(h, x0, lens, t_start, zs, seed, seq_offset, out, full_history):
        calls["plain"].append(dict(t_start=t_start, zs=None if zs is None else zs.shape, seed=seed, seq_offset=seq_offset,
                                   rows=out.shape[0], full_history=full_history))
        out[:] = x0[None]

    def strided(h, x0, lens, visits, coef, zs, seed, seq_offset, out, full_history):
        calls["strided"].append(dict(visits=visits.copy(), coef=coef.copy(), zs=None if zs is None else zs.copy(), seed=seed,
                                     seq_offset=seq_offset, rows=out.shape[0], full_history=full_history, lens=lens.copy()))
        out[:] = x0[None]

    def solver(h, x0, lens, visits, coef, out, full_history):
        calls["solver"].append(dict(visits=visits.copy(), coef=coef.copy(), rows=out.shape[0], full_history=full_history, lens=lens.copy()))
        out[:] = x0[None]

    monkeypatch.setattr(sampling, "_run_fd_sample", plain)
    monkeypatch.setattr(sampling, "_run_fd_sample_strided", strided)
    monkeypatch.setattr(sampling, "_run_fd_sample_solver", solver)
    return calls


def _dset(T=12, pad=16):
    return datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=pad), timesteps=T, beta_schedule="cosine")


@pytest.mark.parametrize("mode", ["torch", "philox"])
def test_sample_with_the_solver_reaches_the_new_runner(runners, monkeypatch, mode):
    monkeypatch.setattr(sampling, "NOISE_MODE", mode)
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    torch.manual_seed(5)
    out = sampling.sample(model, ds, n=2, sweep_lengths=(5, 8), final_only=False, num_steps=5, solver="dpm2m", spacing="logsnr")
    assert [o.shape for o in out] == [(5, l, F) for l in (5, 5, 6, 6, 7, 7)]
    assert len(runners["solver"]) == 1 and not runners["plain"] and not runners["strided"]
    c = runners["solver"][0]
    assert np.array_equal(c["visits"], sampling.logsnr_visits(betas, 5)) and c["visits"].dtype == np.int32
    assert np.array_equal(_bits(c["coef"]), _bits(sampling.solver_coefficients(betas, c["visits"]))) and c["coef"].shape == (5, 5)
    assert c["rows"] == 5 and c["full_history"] == 1 and c["lens"].tolist() == [5, 5, 6, 6, 7, 7]
    assert ("varlen", 1) in model.opts
    # nothing is drawn: the generator stands where the start noise left it
    state = torch.get_rng_state()
    torch.manual_seed(5)
    ds.sample_noise(torch.zeros(6, 16, F))
    if mode == "torch":
        assert torch.equal(state, torch.get_rng_state())
    # uniform spacing and another lambda_min; final only; thinned history
    sampling.sample(model, ds, n=1, sweep_lengths=(5, 7), final_only=True, num_steps=4, solver="dpm2m")
    c = runners["solver"][-1]
    assert c["visits"].tolist() == sampling.ddim_visits(12, 4).tolist() and c["rows"] == 1 and c["full_history"] == 0
    sampling.sample(model, ds, n=1, sweep_lengths=(5, 6), final_only=False, history_every=2, num_steps=5, solver="dpm2m", spacing="logsnr",
                    lambda_min=-1.0)
    c = runners["solver"][-1]
    assert np.array_equal(c["visits"], sampling.logsnr_visits(betas, 5, lambda_min=-1.0)) and c["rows"] == 3 and c["full_history"] == 2
    # log-SNR visits serve DDIM too, through the strided runner
    sampling.sample(model, ds, n=1, sweep_lengths=(5, 6), final_only=False, num_steps=5, solver="ddim", spacing="logsnr", eta=0.5)
    c = runners["strided"][-1]
    assert np.array_equal(c["visits"], sampling.logsnr_visits(betas, 5))
    assert np.array_equal(_bits(c["coef"]), _bits(sampling.ddim_coefficients(betas, c["visits"], 0.5)))
    assert len(runners["solver"]) == 3 and not runners["plain"]


def test_solver_none_reaches_the_old_runners_unchanged(runners, monkeypatch):
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    for kw in (dict(), dict(solver=None), dict(solver="ddim"), dict(solver="ddim", spacing="uniform")):
        sampling.sample(model, ds, n=1, sweep_lengths=(5, 7), final_only=False, num_steps=5, eta=1.0, **kw)
        c = runners["strided"][-1]
        assert np.array_equal(c["visits"], sampling.ddim_visits(12, 5))
        assert np.array_equal(_bits(c["coef"]), _bits(sampling.ddim_coefficients(betas, c["visits"], 1.0)))
        assert c["rows"] == 5 and c["full_history"] == 1 and c["zs"] is None and c["seed"] > 0 and c["seq_offset"] == 0
        out = sampling.sample(model, ds, n=1, sweep_lengths=(5, 7), final_only=False, **kw)
        assert [o.shape for o in out] == [(12, 5, F), (12, 6, F)]
        c = runners["plain"][-1]
        assert c["t_start"] == 11 and c["rows"] == 12 and c["full_history"] == 1 and c["zs"] is None
    assert not runners["solver"]


def test_reverse_from_p_sample_loop_and_reconstruct_pass_the_arguments_on(runners, monkeypatch):
    monkeypatch.setattr(sampling, "NOISE_MODE", "torch")
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    x = torch.zeros(2, 6, F)
    got = sampling.reverse_from(model, x, [6, 4], 6, betas, num_steps=3, solver="dpm2m", spacing="logsnr", lambda_min=None)
    assert tuple(got.shape) == (2, 6, F)
    c = runners["solver"][-1]
    assert np.array_equal(c["visits"], sampling.logsnr_visits(betas, 3, 6, None)) and c["visits"][0] == 6 and c["rows"] == 1 and c["full_history"] == 0
    traj = sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, num_steps=4, solver="dpm2m")
    assert tuple(traj.shape) == (4, 2, 6, F) and runners["solver"][-1]["visits"].tolist() == [11, 7, 4, 0]
    with pytest.raises(ValueError):   # the solver draws nothing
        sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, num_steps=4, solver="dpm2m", step_noise=np.zeros((4, 2, 6, F), np.float32))
    seen = []
    monkeypatch.setattr(sampling, "reverse_from", lambda *a, **kw: seen.append(kw) or torch.zeros(1, 6, F))

    class _OneItem:
        filenames, alpha_beta_terms = ["a"], {"betas": betas}

        def __len__(self):
            return 1

        def __getitem__(self, idx, use_t_val=None):
            return {"corrupted": torch.zeros(6, F), "lengths": 6, "angles": torch.zeros(6, F)}

    sampling.reconstruct(model, _OneItem(), noise_timesteps=7, num_steps=3, solver="dpm2m", spacing="logsnr", lambda_min=-2.0)
    assert seen[-1]["solver"] == "dpm2m" and seen[-1]["spacing"] == "logsnr" and seen[-1]["lambda_min"] == -2.0 and seen[-1]["num_steps"] == 3
    sampling.reconstruct(model, _OneItem(), noise_timesteps=7, num_steps=3)
    assert set(seen[-1]) == {"is_angle", "num_steps", "eta"}                       # today's call, today's arguments
    scorer = lambda r, t, f: (0.0, 0.0)   # noqa: E731
    sampling.get_reconstruction_error(model, _OneItem(), noise_timesteps=7, scorer=scorer, num_steps=3, solver="dpm2m")
    assert seen[-1]["solver"] == "dpm2m" and seen[-1]["spacing"] == "uniform"
    assert not runners["plain"] and not runners["strided"]


def test_argument_errors_of_the_python_samplers(runners):
    ds, model = _dset(), _StubModel()
    betas = ds.alpha_beta_terms["betas"]
    x = torch.zeros(2, 6, F)
    cases = [dict(num_steps=5, solver="dpm2m", eta=0.5),         # an ODE solver: no noise
             dict(solver="dpm2m"),                               # ... and it needs num_steps
             dict(spacing="logsnr"),
             dict(num_steps=5, solver="heun"),
             dict(num_steps=5, spacing="cosine"),
             dict(num_steps=5, spacing="logsnr", lambda_min=float("nan")),
             dict(num_steps=13, solver="dpm2m")]
    for kw in cases:
        with pytest.raises(ValueError):
            sampling.sample(model, ds, n=1, sweep_lengths=(5, 6), **kw)
        with pytest.raises(ValueError):
            sampling.p_sample_loop(model, [6, 4], x, 12, betas, is_angle=[True] * F, **kw)
        if kw.get("num_steps") != 13:
            with pytest.raises(ValueError):
                sampling.reverse_from(model, x, [6, 4], 11, betas, **kw)
    assert not runners["plain"] and not runners["strided"] and not runners["solver"]
    known = [np.zeros((5, F), dtype=np.float32)]
    fixed = [np.zeros((5, F), dtype=bool)]
    with pytest.raises(ValueError, match="solver"):
        sampling.inpaint(model, ds, known, fixed, num_steps=4, solver="dpm2m")
    with pytest.raises(ValueError, match="solver"):
        sampling.scaffold(model, ds, np.zeros((2, F), dtype=np.float32), [5], num_steps=4, solver="dpm2m")


def test_scripts_have_the_flags_and_record_them_only_when_given():
    import importlib.util
    for script, base in [("sample.py", ["-m", "x"]), ("partial_noise_reconstruct.py", ["a.pdb", "out.json", "-m", "x"])]:
        spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(REPO, "bin", script))
        cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cli)
        args = cli.build_parser().parse_args(base)
        assert args.solver is None and args.spacing is None and args.lambda_min is None
        assert {k: getattr(args, k) for k in cli.FEW_STEP_FLAGS if getattr(args, k) is not None} == {}
        args = cli.build_parser().parse_args(base + ["--num_steps", "20", "--solver", "dpm2m", "--spacing", "logsnr", "--lambda_min", "-4"])
        assert args.num_steps == 20 and args.solver == "dpm2m" and args.spacing == "logsnr" and args.lambda_min == -4.0
        assert {k: getattr(args, k) for k in cli.FEW_STEP_FLAGS if getattr(args, k) is not None} == dict(solver="dpm2m", spacing="logsnr", lambda_min=-4.0)
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + ["--solver", "heun"])
