"""Few-step sampling with the second-order multistep solver on the device (fd_sample_solver, fd_sample_solver_dev,
fd_p_sample_step_solver, sampling.sample(solver="dpm2m")) against the float32 statement of tests/solver_reference.py: the
update BIT FOR BIT in each of the three update kernels, the loop as the chain of hooks, order 1 as the strided run, the
free-running loop with the plain sampler's tolerance (tests/test_gpu_parity.py), the contract and the call history.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import solver_reference as vref
import strided_reference as sref
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling
from test_gpu_parity import FWD_TOL, PRECISIONS, STEP_TOL, _c1_models, _free_running_check, _inputs, _pair, _record, _share_time_table
from test_inpaint_gpu import _masks, _sample_inpaint, _sample_plain
from test_strided_gpu import ANG, C1_LENS, F, SENTINEL, _bits, _forward, _rows, _step_coef, _strided, _valid

pytestmark = pytest.mark.gpu
P = _binding.ptr


def _step_solver(h, x, t, lens, a, b, c, u, v, prev, wrap=1):
    """fd_p_sample_step_solver -> (rc, eps_out, x0_out, x_out); the outputs start at the sentinel."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.float32)
    eps, x0, out = (np.full_like(xs, SENTINEL) for _ in range(3))
    rc = _binding.load().fd_p_sample_step_solver(h, P(xs), int(t), P(ls), B, L, float(a), float(b), float(c), float(u), float(v), P(pv),
                                                 wrap, P(eps), P(x0), P(out))
    return rc, eps, x0, out


def _solver(h, x0, lens, visits, coef, full_history, n_visits=None):
    """fd_sample_solver -> (rc, out); `out` starts at the sentinel."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    vs = None if visits is None else np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    K = n_visits if n_visits is not None else len(vs)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float32)
    out = np.full((_rows(max(K, 1), full_history), B, L, F), SENTINEL, dtype=np.float32)
    rc = _binding.load().fd_sample_solver(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(out), full_history)
    return rc, out


def _solver_dev(h, x0, lens, visits, coef, full_history):
    """fd_sample_solver_dev on device copies -> (rc, out on the host)."""
    dev = "cuda:0"
    x_d = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).to(dev)
    B, L, _ = x_d.shape
    l_d = torch.tensor([int(n) for n in lens], dtype=torch.int32, device=dev)
    vs = np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    cf = np.ascontiguousarray(coef, dtype=np.float32)
    out_d = torch.full((_rows(len(vs), full_history), B, L, F), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = _binding.load().fd_sample_solver_dev(h, C.c_void_p(x_d.data_ptr()), C.c_void_p(l_d.data_ptr()), B, L, P(vs), len(vs), P(cf),
                                              C.c_void_p(out_d.data_ptr()), full_history, None)
    return rc, out_d.cpu().numpy()


# ---------------------------------------------------------------------------------- 1. the three update kernels
@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_solver_statement_bit_for_bit_in_every_update_kernel(gpu, precision, hidden, heads):
    """The row-image kernel (f16x3), the 16-lanes-per-token kernel (f32, d % 64 == 0) and the one-wave-per-token kernel
    (f32, d = 96).  One-layer models, L = 24, B = 3, T = 8, ragged lengths.  x_out and x0_out carry the bits of the float32
    statement applied to the hook's own eps_out, for arbitrary finite (a, b, c, u, v) and a random previous prediction in
    [-pi, pi) that straddles the wrap against x0 somewhere; eps_out carries fd_forward's bits.  No tolerance of its own."""
    o32, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, lens = 8, [24, 17, 9]
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    ok = _valid(lens, 24)
    rng = np.random.default_rng(41)
    x = _inputs(3, 24, seed=5).numpy()
    prev = rng.uniform(-np.pi, np.pi, (3, 24, F)).astype(np.float32)
    prev[prev >= np.float32(np.pi)] = -np.float32(np.pi)
    table = sampling.solver_coefficients(betas, np.array([7, 4, 2, 0], dtype=np.int32))
    sets = [tuple(table[:, 1]), tuple(table[:, 2]), (1.7, -0.9, 0.3, 1.2, -0.8), (-0.25, 3.5, -1.5, 0.9, 2.0 ** -20), (1e-3, 2.0, 0.37, -2.5, 1.0)]
    worst = 0.0
    for t, (a, b, c, u, v) in zip((4, 2, 5, 3, 6), sets):
        assert c != 0
        for wrap in (0, 1):
            ang = ANG if wrap else [False] * F
            rc, eps, x0, out = _step_solver(h, x, t, lens, a, b, c, u, v, prev, wrap)
            assert rc == 0, _binding.load().fd_last_error()
            want, want0 = vref.update(x, eps, prev, a, b, c, u, v, ang)
            assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), (t, wrap)
            assert np.array_equal(_bits(x0)[ok], _bits(want0)[ok]), (t, wrap)
            assert np.array_equal(_bits(eps)[ok], _bits(_forward(h, x, t, lens))[ok]), (t, wrap)
            e = float(np.abs(eps - sref.forward(o32, x, t, lens).numpy())[ok].max())
            worst = max(worst, e)
            assert e <= FWD_TOL, (t, wrap, e)
            if wrap:   # the wrap of the difference is exercised: somewhere x0 and prev are more than pi apart as numbers
                assert (np.abs(want0.astype(np.float64) - prev)[ok] > np.pi).any(), t
                assert (np.abs(out[ok]) <= np.float32(np.pi)).all() and (np.abs(x0[ok]) <= np.float32(np.pi)).all()
                # ... and it matters: without it the statement gives other bits
                with np.errstate(invalid="ignore"):
                    m = ((np.float32(a) * x).astype(np.float32) + (np.float32(b) * eps).astype(np.float32)).astype(np.float32)
                    raw = (m + (np.float32(c) * (want0 - prev).astype(np.float32)).astype(np.float32)).astype(np.float32)
                assert not np.array_equal(vref._wrap_cols(raw, np.arange(F))[ok], want[ok])
            else:      # wrap = 0 wraps nothing: x0 = u x + v eps as it is
                plain0 = ((np.float32(u) * x).astype(np.float32) + (np.float32(v) * eps).astype(np.float32)).astype(np.float32)
                assert np.array_equal(_bits(x0)[ok], _bits(plain0)[ok])
    # c = 0: prev is not read -- NaN-filled, or absent -- and the result is fd_p_sample_step_coef's with s = 0
    nan = np.full_like(prev, np.nan)
    for t, (a, b, _, u, v) in zip((4, 5), (sets[0], sets[2])):
        for wrap in (0, 1):
            rc, eps_s, want = _step_coef(h, x, t, lens, a, b, 0.0, None, wrap)
            assert rc == 0
            for p in (nan, None):
                rc, eps, x0, out = _step_solver(h, x, t, lens, a, b, 0.0, u, v, p, wrap)
                assert rc == 0, _binding.load().fd_last_error()
                assert np.isfinite(out[ok]).all() and np.array_equal(_bits(out)[ok], _bits(want)[ok]), (t, wrap)
                assert np.array_equal(_bits(eps)[ok], _bits(eps_s)[ok])
                assert np.array_equal(_bits(x0)[ok], _bits(vref.update(x, eps, None, a, b, 0.0, u, v, ANG if wrap else [False] * F)[1])[ok])
    _record(f"solver_hook_d{hidden}_{precision}", max_eps=worst)


# ---------------------------------------------------------------------------------- 2. the loop is the chain of hooks
VISIT_SETS = [[8, 5, 2, 0], [9, 7, 4, 3, 1, 0]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_equals_the_chain_of_hooks_bit_for_bit(gpu, precision):
    """C1 (d = 192, 6 layers, L = 64, B = 4, T = 10).  Row i of the full history is the hook applied to row i - 1 (row -1 =
    x_init) with visit i's coefficients and the hook's x0_out of visit i - 1 as the previous prediction, bit for bit: the
    table lookup by timestep, the previous prediction carried from launch to launch, the history ordinal.  The thinned
    history, the final-only run, eager launches, packed rows and the device entry give the same bits below the lengths."""
    g, _, _, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    B, L = 4, 64
    x0 = g["x0"]
    ok = _valid(C1_LENS, L)
    for visits in VISIT_SETS:
        K = len(visits)
        coef = sampling.solver_coefficients(betas, np.asarray(visits, dtype=np.int32))
        assert (coef[2, 1:-1] != 0).all()
        rc, full = _solver(h, x0, C1_LENS, visits, coef, 1)
        assert rc == 0, _binding.load().fd_last_error()
        assert full.shape == (K, B, L, F) and np.isfinite(full[:, ok]).all()
        state, prev = x0, None
        for i, t in enumerate(visits):
            a, b, c, u, v = coef[:, i]
            rc, _, x0_i, want = _step_solver(h, state, t, C1_LENS, a, b, c, u, v, prev)
            assert rc == 0, _binding.load().fd_last_error()
            assert np.array_equal(_bits(full[i])[ok], _bits(want)[ok]), (visits, i)
            state, prev = full[i], x0_i
        rc, final = _solver(h, x0, C1_LENS, visits, coef, 0)
        assert rc == 0 and np.array_equal(_bits(final[0])[ok], _bits(full[-1])[ok])
        rc, every2 = _solver(h, x0, C1_LENS, visits, coef, 2)
        states = [1, 3] if K == 4 else [1, 3, 5]
        assert rc == 0 and every2.shape[0] == len(states)
        assert np.array_equal(_bits(every2)[:, ok], _bits(full[states])[:, ok]), (visits, states)
        pm.set_option("use_graph", 0)
        rc, eager = _solver(h, x0, C1_LENS, visits, coef, 1)
        pm.set_option("use_graph", 1)
        assert rc == 0 and np.array_equal(_bits(eager)[:, ok], _bits(full)[:, ok]), (visits, "eager")
        pm.set_option("varlen", 1)
        rc, packed = _solver(h, x0, C1_LENS, visits, coef, 1)
        rc2, packed_dev = _solver_dev(h, x0, C1_LENS, visits, coef, 1)
        pm.set_option("varlen", 0)
        assert rc == 0 and np.array_equal(_bits(packed)[:, ok], _bits(full)[:, ok]), (visits, "varlen")
        assert rc2 == 0 and np.array_equal(_bits(packed_dev)[:, ok], _bits(full)[:, ok]), (visits, "varlen, dev")
        if precision == "f16x3":                 # packed rows (the row-image path): the history's padding is zeroed, as in fd_sample
            assert (packed[:, ~ok] == 0).all()
        rc, dev = _solver_dev(h, x0, C1_LENS, visits, coef, 1)
        assert rc == 0 and np.array_equal(_bits(dev)[:, ok], _bits(full)[:, ok]), (visits, "dev")
        rc, dev0 = _solver_dev(h, x0, C1_LENS, visits, coef, 0)
        assert rc == 0 and np.array_equal(_bits(dev0[0])[ok], _bits(full[-1])[ok]), (visits, "dev, final only")
        # the second order is in the run: order 1 on the same visits gives other states from visit 1 on
        rc, first = _solver(h, x0, C1_LENS, visits, sampling.solver_coefficients(betas, visits, order=1), 1)
        assert rc == 0 and np.array_equal(_bits(first[0])[ok], _bits(full[0])[ok]) and not np.array_equal(first[1][ok], full[1][ok])


# ---------------------------------------------------------------------------------- 3. order 1 is the strided run
@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_one_gives_the_bits_of_the_strided_run(gpu, precision):
    g, _, _, pm = _c1_models(precision)
    betas = beta_schedules.cosine_beta_schedule(int(g["T"]))
    h = pm.prepare(betas)
    ok = _valid(C1_LENS, 64)
    for visits in VISIT_SETS:
        coef = sampling.solver_coefficients(betas, visits, order=1)
        rc, got = _solver(h, g["x0"], C1_LENS, visits, coef, 1)
        rc2, want = _strided(h, g["x0"], C1_LENS, visits, sampling.ddim_coefficients(betas, visits, 0.0), 0, 1)
        assert rc == 0 and rc2 == 0, _binding.load().fd_last_error()
        assert np.array_equal(_bits(got)[:, ok], _bits(want)[:, ok]), visits


# ---------------------------------------------------------------------------------- 4. against the oracle, free-running
FREE_VISITS = np.array([8, 5, 2, 0], dtype=np.int32)   # every |coefficient| <= 6.5, |c| <= 0.38: below the plain sampler's worst (1.0e2), under which STEP_TOL was set
_FREE_REF = {}


def _free_reference(o32, o64, x0, betas, T):
    """The restatement's loop with the fp32 and the fp64 oracle; computed once, shared by the precisions."""
    if not _FREE_REF:
        coef = sampling.solver_coefficients(betas, FREE_VISITS)
        assert np.abs(coef).max() <= 6.5 and np.abs(coef[2]).max() <= 0.38
        _share_time_table(o64, o32, T)
        _FREE_REF["ref"] = (coef, vref.loop(o32, C1_LENS, x0, FREE_VISITS, coef, ANG), vref.loop(o64, C1_LENS, x0, FREE_VISITS, coef, ANG))
    return _FREE_REF["ref"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_free_running_c1_against_the_oracle(gpu, precision):
    """STEP_TOL on the wrapped difference, 4 of 4 sequences compared over all 4 visits (no sequence is excused by a wrap flip)."""
    g, o32, o64, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef, want32, want64 = _free_reference(o32, o64, g["x0"], betas, T)
    ok = _valid(C1_LENS, 64)
    sel = lambda a: np.where(ok, a, 0.0)   # noqa: E731  (positions beyond a length are nobody's result)
    # the condition on the start: the oracle's own two precisions stay together
    _free_running_check("solver_free_c1_oracle32_vs_64", sel(want32), sel(want64), min_clean=4)
    rc, got = _solver(h, g["x0"], C1_LENS, FREE_VISITS, coef, 1)
    assert rc == 0, _binding.load().fd_last_error()
    _free_running_check(f"solver_free_c1_{precision}", sel(got), sel(want32), tol=STEP_TOL, min_clean=4)


# ---------------------------------------------------------------------------------- 5. the contract
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision="f16x3")
    T = 12
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    lib = _binding.load()
    lens = [50, 33, 64, 12]
    x0 = _inputs(4, 64, seed=4).numpy()
    visits = np.array([11, 7, 3, 0], dtype=np.int32)
    coef = sampling.solver_coefficients(betas, visits)
    dcoef = sampling.ddim_coefficients(betas, visits, 0.5)
    known, fixed = _masks(lens, 64)
    kcoef = sampling.inpaint_levels(betas)
    before = _sample_plain(h, x0, lens, T - 1, 5, 1)
    rc, before_strided = _strided(h, x0, lens, visits, dcoef, 5, 1)
    assert rc == 0
    rc, before_inpaint = _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, 5, 1)
    assert rc == 0
    nan_coef, inf_coef, inf_u, c0 = coef.copy(), coef.copy(), coef.copy(), coef.copy()
    nan_coef[1, 2] = np.nan
    inf_coef[4, 0] = np.inf
    inf_u[3, 3] = -np.inf
    c0[2, 0] = 0.125
    bad = [(dict(visits=None, n_visits=4), b"visits is null"),
           (dict(coef=None), b"coef is null"),
           (dict(n_visits=0), b"n_visits = 0"),
           (dict(visits=[12, 7, 3, 0]), b"visits[0] = 12 outside"),
           (dict(visits=[11, 7, -1, 0]), b"visits[2] = -1 outside"),
           (dict(visits=[11, 7, 7, 0]), b"visits[2] = 7 follows 7"),
           (dict(visits=[11, 3, 7, 0]), b"visits[2] = 7 follows 3"),
           (dict(coef=nan_coef), b"coef[1][2]"),
           (dict(coef=inf_coef), b"coef[4][0]"),
           (dict(coef=inf_u), b"coef[3][3]"),
           (dict(coef=c0), b"coef[2][0]")]
    for kw, word in bad:
        a = dict(visits=visits, coef=coef, n_visits=None)
        a.update(kw)
        rc, out = _solver(h, x0, lens, a["visits"], a["coef"], 1, n_visits=a["n_visits"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all(), word
        after = _sample_plain(h, x0, lens, T - 1, 5, 1)        # a rejected call changes nothing
        assert np.array_equal(_bits(after), _bits(before)), word
    rc, out = _solver(h, x0, [50, 0, 64, 12], visits, coef, 1)
    assert rc == -1 and (out == SENTINEL).all()
    prev = np.zeros((4, 64, F), dtype=np.float32)
    for (a, b, c, u, v, pv), word in [((1.0, -1.0, 0.5, 1.0, -1.0, None), b"x0_prev is required"), ((np.nan, -1.0, 0.0, 1.0, -1.0, prev), b"not finite"),
                                      ((1.0, -1.0, np.inf, 1.0, -1.0, prev), b"not finite"), ((1.0, -1.0, 0.0, -np.inf, -1.0, prev), b"not finite"),
                                      ((1.0, -1.0, 0.0, 1.0, np.nan, prev), b"not finite")]:
        rc, eps, x0_out, out = _step_solver(h, x0, 3, lens, a, b, c, u, v, pv)
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all() and (eps == SENTINEL).all() and (x0_out == SENTINEL).all()
    rc, eps, x0_out, out = _step_solver(h, x0, T, lens, 1.0, -1.0, 0.0, 1.0, -1.0, None)    # the timestep is checked like fd_p_sample_step's
    assert rc == -1 and (out == SENTINEL).all()
    # valid solver runs, host and device entry, and the hook; then the plain, the strided and the conditioned sampler are what
    # they were: the per-run values of the update kernels are clean
    rc, run = _solver(h, x0, lens, visits, coef, 1)
    assert rc == 0 and np.isfinite(run[:, _valid(lens, 64)]).all(), lib.fd_last_error()
    assert not np.array_equal(run[-1], before[-1])
    rc, _ = _solver_dev(h, x0, lens, visits, coef, 0)
    assert rc == 0
    rc, _, _, _ = _step_solver(h, x0, 3, lens, 1.0, -1.0, 0.5, 1.0, -1.0, prev)
    assert rc == 0
    after = _sample_plain(h, x0, lens, T - 1, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))
    rc, after_strided = _strided(h, x0, lens, visits, dcoef, 5, 1)
    assert rc == 0 and np.array_equal(_bits(after_strided), _bits(before_strided))
    rc, after_inpaint = _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, 5, 1)
    assert rc == 0 and np.array_equal(_bits(after_inpaint), _bits(before_inpaint))
    rc, again = _solver(h, x0, lens, visits, coef, 1)                                   # ... and the solver run after them too
    assert rc == 0 and np.array_equal(_bits(again), _bits(run))


# ---------------------------------------------------------------------------------- 6. the call history
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_a_solver_run_does_not_depend_on_the_handle_s_earlier_calls(gpu, precision):
    """A solver run made after a solver run with other lengths and another K, and after a plain run, carries the bits of the
    same call made first on a fresh handle of the same weights: a stale previous prediction or table would show here (the
    earlier run's last visit leaves a previous prediction behind, and its table has entries at timesteps this one visits)."""
    kw = dict(hidden=192 if precision == "f16x3" else 128, heads=6 if precision == "f16x3" else 4, ff=384 if precision == "f16x3" else 256, layers=2, maxpos=128, seed=12,
              precision=precision)
    T = 12
    betas = beta_schedules.cosine_beta_schedule(T)
    lens, x0 = [40, 64, 7, 23], _inputs(4, 64, seed=21).numpy()
    visits = np.array([11, 6, 2, 0], dtype=np.int32)
    coef = sampling.solver_coefficients(betas, visits)
    _, _, fresh = _pair(**kw)
    rc, want = _solver(fresh.prepare(betas), x0, lens, visits, coef, 1)
    assert rc == 0 and np.isfinite(want).all() and not (want == SENTINEL).any(), _binding.load().fd_last_error()
    fresh._invalidate()
    _, _, pm = _pair(**kw)
    h = pm.prepare(betas)
    other = np.array([11, 9, 6, 4, 2, 1, 0], dtype=np.int32)
    rc, _ = _solver(h, _inputs(4, 64, seed=22).numpy(), [64, 12, 50, 33], other, sampling.solver_coefficients(betas, other), 0)
    assert rc == 0
    rc, got = _solver(h, x0, lens, visits, coef, 1)
    assert rc == 0 and np.array_equal(_bits(got), _bits(want))
    _sample_plain(h, x0, [64, 12, 50, 33], T - 1, 5, 0)
    rc, got = _solver(h, x0, lens, visits, coef, 1)
    assert rc == 0 and np.array_equal(_bits(got), _bits(want))
    rc, _ = _solver(h, _inputs(3, 40, seed=23).numpy(), [40, 12, 33], other, sampling.solver_coefficients(betas, other), 2)   # another workspace
    assert rc == 0
    rc, got = _solver_dev(h, x0, lens, visits, coef, 1)
    assert rc == 0 and np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------- 7. Python end to end
def test_sample_end_to_end_on_a_tiny_model(gpu, monkeypatch):
    _, _, pm = _pair(seed=11, precision="f16x3")
    T = 20
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64), timesteps=T, beta_schedule="cosine")
    betas = ds.alpha_beta_terms["betas"]
    runs = []
    for mode in ("philox", "torch", "torch"):
        monkeypatch.setattr(sampling, "NOISE_MODE", mode)
        torch.manual_seed(3)
        runs.append(sampling.sample(pm, ds, n=2, sweep_lengths=(30, 33), final_only=False, num_steps=5, solver="dpm2m", spacing="logsnr"))
    assert [s.shape for s in runs[0]] == [(5, l, F) for l in (30, 30, 31, 31, 32, 32)]
    for s0, s1, s2 in zip(*runs):   # a deterministic map of the start noise: the same across calls and noise modes
        assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(_bits(s1), _bits(s2))
        assert np.isfinite(s0).all() and (s0 >= -np.float32(np.pi)).all() and (s0 < np.float32(np.pi)).all()
    torch.manual_seed(3)
    ddim = sampling.sample(pm, ds, n=2, sweep_lengths=(30, 33), final_only=False, num_steps=5, solver="ddim", spacing="logsnr")
    assert np.array_equal(_bits(ddim[0][0]), _bits(runs[0][0][0])) and not np.array_equal(ddim[0][1], runs[0][0][1])   # c[0] = 0, then second order
    torch.manual_seed(3)
    fin = sampling.sample(pm, ds, n=2, sweep_lengths=(30, 33), final_only=True, num_steps=5, solver="dpm2m", spacing="logsnr")
    assert [s.shape for s in fin] == [(1, l, F) for l in (30, 30, 31, 31, 32, 32)]
    assert all(np.array_equal(_bits(a[0]), _bits(b[-1])) for a, b in zip(fin, runs[0]))
    # reverse_from starts its schedule at t_start: the same states as the C entry on those visits
    x = _inputs(2, 40, seed=8)
    got = sampling.reverse_from(pm, x, [40, 25], 6, betas, is_angle=True, num_steps=3, solver="dpm2m", spacing="logsnr").numpy()
    visits = sampling.logsnr_visits(betas, 3, 6)
    h = pm.prepare(betas, True)
    rc, want = _solver(h, x.numpy(), [40, 25], visits, sampling.solver_coefficients(betas, visits), 0)
    ok = _valid([40, 25], 40)
    assert rc == 0 and np.array_equal(_bits(got)[ok], _bits(want[0])[ok])
    # the device-resident entry of the package
    x_d = x.to("cuda:0")
    l_d = torch.tensor([40, 25], dtype=torch.int32, device="cuda:0")
    out_d = sampling.sample_on_device(pm, x_d, l_d, betas, is_angle=True, t_start=6, num_steps=3, solver="dpm2m", spacing="logsnr", full_history=True)
    assert tuple(out_d.shape) == (3, 2, 40, F) and np.array_equal(_bits(out_d[-1].cpu().numpy())[ok], _bits(got)[ok])
