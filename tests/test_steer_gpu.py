"""Steering by particle resampling on the device (fd_steer_rewards, fd_steer_resample, fd_p_sample_step_coef_x0,
fd_sample_steered, sampling.steer) against the existing entries composed on the host and the numpy statements of
tests/steer_reference.py: integers and bits are compared with ==, the radius of gyration within 1e-12 relative.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import solver_reference as vref
import steer_reference as st
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from test_gpu_parity import PRECISIONS, _inputs, _pair, _record
from test_inpaint_gpu import _sample_plain
from test_solver_gpu import _solver
from test_strided_gpu import ANG, F, SENTINEL, _bits, _step_coef, _strided, _valid

pytestmark = pytest.mark.gpu
P = _binding.ptr
NAMES = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
IDX = np.array([0, 1, 2, 3, 4, 5, -1, -1, -1], dtype=np.int32)
OFFSET = np.array([-1.3, 1.1, 3.0, 1.95, 2.03, 2.12], dtype=np.float32)   # about the training means of the full-angle set
WEIGHTS = np.array([-1.0, -0.5, 1.0, 1.0])
ALPHA = 0.63


def _step_x0(h, x, t, lens, a, b, s, u, v, z, wrap=1):
    """fd_p_sample_step_coef_x0 -> (rc, eps_out, x0_out, x_out); the outputs start at the sentinel."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    zs = None if z is None else np.ascontiguousarray(z, dtype=np.float32)
    eps, x0, out = (np.full_like(xs, SENTINEL) for _ in range(3))
    rc = _binding.load().fd_p_sample_step_coef_x0(h, P(xs), int(t), P(ls), B, L, float(a), float(b), float(s), float(u), float(v), P(zs),
                                                  wrap, P(eps), P(x0), P(out))
    return rc, eps, x0, out


def _rewards(x, lens, offset, weights=WEIGHTS, alpha=ALPHA):
    """fd_steer_rewards -> (rc, terms, reward)."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float32)
    ang = np.ones(F, dtype=np.uint8)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    terms, rew = np.full((B, 4), SENTINEL), np.full(B, SENTINEL)
    rc = _binding.load().fd_steer_rewards(0, P(xs), P(ls), B, L, F, P(IDX), P(off), P(ang), P(w), float(alpha), P(terms), P(rew))
    return rc, terms, rew


def _resample(reward, logw, r_prev, G, P_, lam, ess_frac, u):
    """fd_steer_resample -> (rc, logw, r_prev, ancestors, resampled)."""
    reward = np.ascontiguousarray(reward, dtype=np.float64)
    logw, r_prev = np.array(logw, dtype=np.float64), np.array(r_prev, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    anc, flags = np.full(G * P_, -7, dtype=np.int32), np.full(G, 249, dtype=np.uint8)
    rc = _binding.load().fd_steer_resample(0, P(reward), P(logw), P(r_prev), G, P_, float(lam), float(ess_frac), P(u), P(anc), P(flags))
    return rc, logw, r_prev, anc, flags


def _steered(h, x0, lens, visits, coef, noise, seed, event, P_, params, u, n_visits=None, outs=True):
    """fd_sample_steered -> (rc, out, terms, reward, logw, ancestors); the outputs start at the sentinel."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    vs = None if visits is None else np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    K = n_visits if n_visits is not None else len(vs)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float32)
    zs = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    ev = None if event is None else np.ascontiguousarray(event, dtype=np.uint8)
    us = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    n_ev = int(ev.sum()) if ev is not None else 0
    out = np.full((B, L, F), SENTINEL, dtype=np.float32)
    terms, rew, logw = (np.full((B, 4), SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL)) if outs else (None, None, None)
    anc = np.full((max(n_ev, 1), B), -7, dtype=np.int32)
    rc = _binding.load().fd_sample_steered(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(zs), C.c_uint64(seed), C.c_int64(0), P(ev), int(P_),
                                           None if params is None else C.byref(params), P(us), P(out), P(terms), P(rew), P(logw), P(anc))
    return rc, out, terms, rew, logw, anc[:n_ev]


def _params(weights=WEIGHTS, lam=2.0, ess_frac=1.0, offset=OFFSET, alpha=ALPHA):
    return sampling.steer_params(weights, lam, ess_frac, alpha, NAMES, offset)


def _compose(x, lens, offset, weights=WEIGHTS, alpha=ALPHA):
    """The rewards statement from the existing entries composed on the host: the shift in numpy float32, fd_nerf
    (center = 0), fd_backbone_clashes on the float32 coordinates, fd_annotate_sse on the fp64 CA atoms, numpy fp64 for the
    radius of gyration, the left-to-right sum in Python floats."""
    ang = st.shift(x, offset, ANG)
    coords = nerf.build_backbones([ang[b, :n] for b, n in enumerate(lens)], NAMES, center_coords=False)
    clashes = structures.count_clashes(coords, alpha=alpha)
    sse = structures.annotate_sse([c[1::3] for c in coords])
    terms = np.zeros((len(lens), 4))
    for b, n in enumerate(lens):
        ca = coords[b][1::3]
        terms[b] = [float(clashes[b]), np.sqrt(((ca - ca.mean(axis=0)) ** 2).sum() / n), (sse[b] == "a").sum() / n, (sse[b] == "b").sum() / n]
    return terms, np.array([st.weighted(weights, t) for t in terms])


# ---------------------------------------------------------------------------------- a. rewards
def _reward_chains():
    """B = 6, L = 100, lens (1, 2, 3, 7, 40, 100): compact-random, extended, helical and mixed chains, in model space (the
    offset is subtracted, so that the shifted angles are the intended ones); the first seed whose chains -- by the CPU
    references -- hold a clash, a helix and a strand, with every integer decision at least 1e-6 from its threshold."""
    lens = (1, 2, 3, 7, 40, 100)
    kinds = [["random"], ["random"], ["random"], ["extended"], ["helix"], ["helix", "random", "random", "extended"]]
    for seed in range(20):
        rng = np.random.default_rng(100 + seed)
        x = np.zeros((6, 100, F), dtype=np.float32)
        for b, (n, ks) in enumerate(zip(lens, kinds)):
            parts = np.array_split(np.arange(n), len(ks))
            x[b, :n] = np.concatenate([st.angles_of(k, len(p), rng) for k, p in zip(ks, parts)])
        terms, _, margin = st.rewards(x, lens, IDX, WEIGHTS, ALPHA)
        model_space = st.shift(x, -OFFSET, ANG)
        terms_off, _, margin_off = st.rewards(st.shift(model_space, OFFSET, ANG), lens, IDX, WEIGHTS, ALPHA)
        if min(margin, margin_off) >= 1e-6 and all((t[:, 0] > 0).any() and (t[:, 2] > 0).any() and (t[:, 3] > 0).any() for t in (terms, terms_off)):
            return lens, x, model_space
    raise AssertionError("no seed gave chains with a clash, a helix and a strand")


def test_rewards_equal_the_existing_entries_composed_on_the_host(gpu):
    """300 atoms of the longest chain cross the clash kernel's 256-atom block; lengths 1, 2 and 3 have no dihedral to label."""
    lens, plain, model_space = _reward_chains()
    worst = 0.0
    for x, offset in ((plain, None), (model_space, OFFSET)):
        rc, terms, rew = _rewards(x, lens, offset)
        assert rc == 0, _binding.load().fd_last_error()
        want, want_rew = _compose(x, lens, offset)
        ref_terms, _, _ = st.rewards(st.shift(x, offset, ANG), lens, IDX, WEIGHTS, ALPHA)
        print("terms", terms.tolist(), "composed", want.tolist())
        assert np.array_equal(terms[:, 0], want[:, 0]) and np.array_equal(terms[:, 2:], want[:, 2:])
        assert np.array_equal(terms[:, [0, 2, 3]], ref_terms[:, [0, 2, 3]])       # ... and the numpy references agree
        assert (terms[:, 0] > 0).any() and (terms[:, 2] > 0).any() and (terms[:, 3] > 0).any()
        rel = np.abs(terms[:, 1] - want[:, 1]) / np.maximum(want[:, 1], 1e-300)
        rel[want[:, 1] == 0] = np.abs(terms[:, 1])[want[:, 1] == 0]
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1e-12, rel
        assert np.array_equal(rew.view(np.uint64), np.array([st.weighted(WEIGHTS, t) for t in terms]).view(np.uint64))
        assert np.allclose(rew, want_rew, rtol=1e-12, atol=0)
        rc, terms2, rew2 = _rewards(x, lens, offset)                               # a second launch: the same bits
        assert rc == 0 and np.array_equal(terms2.view(np.uint64), terms.view(np.uint64)) and np.array_equal(rew2.view(np.uint64), rew.view(np.uint64))
    _record("steer_rewards_rg_rel", max=worst)


# ---------------------------------------------------------------------------------- b. resampling
def _resample_cases(G, P_, rng):
    """(reward, logw, r_prev, lam, ess_frac, u) tuples: the CPU test's cases and random ones, with and without a resample."""
    n = G * P_
    dom = np.zeros(n)
    dom[rng.integers(0, P_)] = 80.0
    cases = [(np.full(n, 2.5), np.zeros(n), np.full(n, 2.5), 1.7, 1.0, np.full(G, 0.25)),
             (np.full(n, 2.5), np.full(n, 0.125), np.full(n, 2.5), 1.7, 0.5, np.full(G, 0.5)),
             (dom, np.zeros(n), np.zeros(n), 1.0, 0.9, rng.random(G)),
             (rng.normal(0, 3, n), np.zeros(n), np.zeros(n), 0.75, 0.0, rng.random(G))]
    for k in range(16):
        spread = (0.05, 0.5, 2.0, 6.0)[k % 4]
        cases.append((rng.normal(0, spread, n), rng.normal(0, 0.3, n) * (k % 2), rng.normal(0, spread, n) * (k // 2 % 2),
                      (1.0, -0.6, 2.5)[k % 3], (1.0, 0.5, 0.8, 0.3)[k // 4], rng.random(G)))
    return cases


@pytest.mark.parametrize("G", [1, 3])
def test_resampling_equals_the_reference(gpu, G):
    rng = np.random.default_rng(17 + G)
    made = kept = with_resample = without = 0
    for P_ in (1, 2, 5, 64, 65, 1024):
        for reward, logw, r_prev, lam, ess_frac, u in _resample_cases(G, P_, rng):
            made += 1
            want_logw, want_prev, want_anc, want_flags, margin = st.resample(reward, logw, r_prev, P_, lam, ess_frac, u)
            if margin < 1e-9:   # a decision that the ulps between two exp() could flip
                continue
            kept += 1
            rc, got_logw, got_prev, anc, flags = _resample(reward, logw, r_prev, G, P_, lam, ess_frac, u)
            assert rc == 0, _binding.load().fd_last_error()
            assert np.array_equal(anc, want_anc) and np.array_equal(flags, want_flags), (P_, lam, ess_frac)
            assert np.array_equal(got_logw.view(np.uint64), want_logw.view(np.uint64)), (P_, lam, ess_frac)
            assert np.array_equal(got_prev.view(np.uint64), want_prev.view(np.uint64)), (P_, lam, ess_frac)
            with_resample += int(want_flags.any())
            without += int(not want_flags.all())
    print(f"kept {kept} of {made} generated cases; {with_resample} with a resample, {without} with a group left alone")
    _record(f"steer_resample_kept_G{G}", kept=kept, made=made)
    assert kept >= 0.9 * made and with_resample >= 20 and without >= 20


# ---------------------------------------------------------------------------------- c. the x0 statement
@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_x0_statement_bit_for_bit_in_every_update_kernel(gpu, precision, hidden, heads):
    """The row-image kernel, the 16-lanes-per-token kernel and the one-wave-per-token kernel, as in test_solver_gpu's
    statement test; every visit draws (s != 0).  x' carries fd_p_sample_step_coef's bits, x0 the bits of
    solver_reference.update's x0 on the hook's own eps."""
    _, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, lens = 8, [24, 17, 9]
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    ok = _valid(lens, 24)
    x = _inputs(3, 24, seed=5).numpy()
    z = np.random.default_rng(9).standard_normal((3, 24, F)).astype(np.float32)
    table = sampling.steer_coefficients(betas, np.array([7, 4, 2, 0], dtype=np.int32), 1.0)
    sets = [tuple(table[:, 0]), tuple(table[:, 2]), (1.7, -0.9, 0.3, 1.2, -0.8), (-0.25, 3.5, -1.5, 0.9, 2.0 ** -20), (1e-3, 2.0, 0.37, -2.5, 1.0)]
    for t, (a, b, s, u, v) in zip((7, 2, 5, 3, 6), sets):
        assert s != 0
        for wrap in (0, 1):
            ang = ANG if wrap else [False] * F
            rc, eps, x0, out = _step_x0(h, x, t, lens, a, b, s, u, v, z, wrap)
            assert rc == 0, _binding.load().fd_last_error()
            rc, eps_c, out_c = _step_coef(h, x, t, lens, a, b, s, z, wrap)
            assert rc == 0
            assert np.array_equal(_bits(out)[ok], _bits(out_c)[ok]) and np.array_equal(_bits(eps)[ok], _bits(eps_c)[ok]), (t, wrap)
            want0 = vref.update(x, eps, None, a, b, 0.0, u, v, ang)[1]
            assert np.array_equal(_bits(x0)[ok], _bits(want0)[ok]), (t, wrap)
            if wrap:
                assert (np.abs(x0[ok]) <= np.float32(np.pi)).all()
    rc, eps, x0, out = _step_x0(h, x, 3, lens, 1.0, -1.0, 0.0, 1.2, -0.8, None)      # s == 0: no z needed, x0 all the same
    assert rc == 0 and np.array_equal(_bits(x0)[ok], _bits(vref.update(x, eps, None, 1.0, -1.0, 0.0, 1.2, -0.8, ANG)[1])[ok])


# ---------------------------------------------------------------------------------- d. the run is the chain of its hooks
VISIT_SETS = [[8, 5, 2, 0], [9, 7, 4, 3, 1, 0]]
LENS_D, L_D, P_D, G_D, T_D, LAM_D = [9, 9, 9, 16, 16, 16], 16, 3, 2, 10, 2.0
MODEL_D = dict(hidden=192, heads=6, ff=384, layers=2, maxpos=32, seed=5)
_CHOSEN = {}


def _chosen_run(o32, betas, vi):
    """Start point, draws and uniforms of the run over VISIT_SETS[vi], chosen with the CPU chain over the oracle: of six
    seeds, the one with the largest smallest decision margin among those where an event has a non-identity ancestor vector."""
    if vi not in _CHOSEN:
        visits = VISIT_SETS[vi]
        K = len(visits)
        coef = sampling.steer_coefficients(betas, visits, 1.0)
        event = np.array([0] + [1] * (K - 1), dtype=np.uint8)
        best = None
        for seed in range(6):
            rng = np.random.default_rng(50 + 10 * vi + seed)
            x0 = _inputs(6, L_D, seed=60 + seed).numpy()
            noise = rng.standard_normal((K, 6, L_D, F)).astype(np.float32)
            u = rng.random((K - 1, G_D))
            run = st.chain(o32, LENS_D, x0, visits, coef, noise, event, P_D, u, IDX, WEIGHTS, LAM_D, 1.0, OFFSET, ANG, ALPHA)
            moved = any(not np.array_equal(a, np.arange(6)) for a in run["ancestors"])
            if moved and run["margins"].min() >= 1e-6 and (best is None or run["margins"].min() > best[0]):
                best = (float(run["margins"].min()), x0, noise, u, coef, event)
        assert best is not None, "no seed gave a non-identity resample with every margin >= 1e-6"
        _CHOSEN[vi] = best[1:]
    return _CHOSEN[vi]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 10, G = 2 groups of P = 3 particles of lengths 9 and 16, L = 16; explicit noise and uniforms, ess_frac = 1, an event
    after every visit but the first.  The run's out, terms, rewards, log-weights and ancestors are those of the chain
    fd_p_sample_step_coef_x0 -> fd_steer_rewards -> fd_steer_resample -> a gather on the host."""
    o32, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_D)
    h = pm.prepare(betas)
    ok = _valid(LENS_D, L_D)
    params = _params(lam=LAM_D, ess_frac=1.0)
    for vi, visits in enumerate(VISIT_SETS):
        x0, noise, u, coef, event = _chosen_run(o32, betas, vi)
        rc, out, terms, rew, logw, anc = _steered(h, x0, LENS_D, visits, coef, noise, 0, event, P_D, params, u)
        assert rc == 0, _binding.load().fd_last_error()
        state, lw, rp, e = x0, np.zeros(6), np.zeros(6), 0
        margins, chain_anc = [], []
        for i, t in enumerate(visits):
            a, b, s, cu, cv = coef[:, i]
            rc, _, x0_i, state = _step_x0(h, state, t, LENS_D, a, b, s, cu, cv, noise[i])
            assert rc == 0, _binding.load().fd_last_error()
            if event[i]:
                rc, _, r_i = _rewards(x0_i, LENS_D, OFFSET)
                assert rc == 0, _binding.load().fd_last_error()
                margins.append(st.resample(r_i, lw, rp, P_D, LAM_D, 1.0, u[e])[4])
                rc, lw, rp, a_i, flags = _resample(r_i, lw, rp, G_D, P_D, LAM_D, 1.0, u[e])
                assert rc == 0 and flags.all()
                state = state[a_i]
                chain_anc.append(a_i)
                e += 1
        rc, want_terms, want_rew = _rewards(state, LENS_D, OFFSET)
        assert rc == 0
        print(visits, "ancestors", anc.tolist(), "margins", margins)
        assert np.array_equal(anc, np.array(chain_anc)), visits
        assert np.array_equal(_bits(out)[ok], _bits(state)[ok]), visits
        assert np.array_equal(terms.view(np.uint64), want_terms.view(np.uint64)) and np.array_equal(rew.view(np.uint64), want_rew.view(np.uint64))
        assert np.array_equal(logw.view(np.uint64), lw.view(np.uint64)) and (logw == 0).all()
        # the device's own run resampled for real, and none of its decisions was close
        assert any(not np.array_equal(a_i, np.arange(6)) for a_i in anc), visits
        assert min(margins) >= 1e-6, margins
        assert all((a_i // P_D == np.arange(6) // P_D).all() for a_i in anc)        # ancestors stay within their group
        # eager launches and packed rows give the same bits below the lengths
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            rc, out2, _, rew2, _, anc2 = _steered(h, x0, LENS_D, visits, coef, noise, 0, event, P_D, params, u)
            pm.set_option(option, int(option == "use_graph"))
            assert rc == 0 and np.array_equal(_bits(out2)[ok], _bits(out)[ok]) and np.array_equal(anc2, anc) and np.array_equal(rew2, rew), option


# ---------------------------------------------------------------------------------- e. degenerate runs
@pytest.mark.parametrize("precision", PRECISIONS)
def test_degenerate_runs_are_the_strided_run(gpu, precision):
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_D)
    h = pm.prepare(betas)
    ok = _valid(LENS_D, L_D)
    visits = VISIT_SETS[1]
    K = len(visits)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    x0 = _inputs(6, L_D, seed=71).numpy()
    noise = np.random.default_rng(72).standard_normal((K, 6, L_D, F)).astype(np.float32)
    u = np.random.default_rng(73).random((K, 6))
    every = np.ones(K, dtype=np.uint8)
    for zs, seed in ((noise, 0), (None, 1234)):
        rc, want = _strided(h, x0, LENS_D, visits, coef[:3], seed, 0, noise=zs)
        assert rc == 0, _binding.load().fd_last_error()
        runs = {"one particle": (every, 1, _params(ess_frac=1.0)), "no event": (np.zeros(K, np.uint8), P_D, _params(ess_frac=1.0)),
                "zero weights": (every, P_D, _params(weights=np.zeros(4), ess_frac=0.5))}
        for name, (event, P_, params) in runs.items():
            rc, out, terms, rew, logw, anc = _steered(h, x0, LENS_D, visits, coef, zs, seed, event, P_, params, u)
            assert rc == 0, (name, _binding.load().fd_last_error())
            assert np.array_equal(_bits(out)[ok], _bits(want[0])[ok]), name
            assert all(np.array_equal(a, np.arange(6)) for a in anc) and len(anc) == int(event.sum()), name
            rc, want_terms, want_rew = _rewards(out, LENS_D, OFFSET, weights=np.zeros(4) if name == "zero weights" else WEIGHTS)
            assert rc == 0 and np.array_equal(terms, want_terms) and np.array_equal(rew, want_rew), name
            assert (logw == 0).all(), name   # resampled to 0 (one particle), never touched (no event), or lambda * 0


# ---------------------------------------------------------------------------------- f. errors and the call history
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_D)
    h = pm.prepare(betas)
    lib = _binding.load()
    visits = np.array(VISIT_SETS[0], dtype=np.int32)
    K = len(visits)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    scoef = sampling.solver_coefficients(betas, visits)
    x0 = _inputs(6, L_D, seed=81).numpy()
    event = np.array([0, 1, 1, 1], dtype=np.uint8)
    u = np.random.default_rng(82).random((3, G_D))
    before = _sample_plain(h, x0, LENS_D, T_D - 1, 5, 1)
    rc, before_strided = _strided(h, x0, LENS_D, visits, coef[:3], 5, 1)
    assert rc == 0
    inf_u, nan_b, bad_u, one_u = coef.copy(), coef.copy(), u.copy(), u.copy()
    inf_u[3, 1] = np.inf
    nan_b[1, 2] = np.nan
    bad_u[2, 1] = -0.25
    one_u[0, 0] = 1.0
    bad_idx = _params()
    bad_idx.feat_idx[1] = 6
    bad = [(dict(visits=None, n_visits=4), b"visits is null"), (dict(coef=None), b"coef is null"), (dict(n_visits=0), b"n_visits = 0"),
           (dict(visits=[10, 5, 2, 0]), b"visits[0] = 10 outside"), (dict(visits=[8, 5, 5, 0]), b"visits[2] = 5 follows 5"),
           (dict(coef=nan_b), b"coef[1][2]"), (dict(coef=inf_u), b"coef[3][1]"),
           (dict(event=None), b"null"), (dict(u=None), b"null"), (dict(params=None), b"null"), (dict(outs=False), b"null"),
           (dict(P_=0), b"n_particles = 0"), (dict(P_=1025), b"n_particles = 1025"), (dict(P_=4), b"not a multiple"),
           (dict(lens=[9, 9, 8, 16, 16, 16]), b"a group shares one length"), (dict(lens=[9, 9, 9, 17, 17, 17]), b"lens[3]=17"),
           (dict(params=_params(weights=[1.0, np.nan, 0.0, 0.0])), b"weights[1]"), (dict(params=_params(lam=np.inf)), b"lambda"),
           (dict(params=_params(ess_frac=-1.0)), b"ess_frac"), (dict(params=_params(alpha=0.0)), b"clash_alpha"),
           (dict(params=_params(offset=np.array([0, 0, np.nan, 0, 0, 0], np.float32))), b"offset[2]"), (dict(params=bad_idx), b"feat_idx[1]"),
           (dict(u=bad_u), b"u[5]"), (dict(u=one_u), b"u[0]")]
    for kw, word in bad:
        a = dict(lens=LENS_D, visits=visits, coef=coef, n_visits=None, event=event, P_=P_D, params=_params(), u=u, outs=True)
        a.update(kw)
        rc, out, terms, rew, logw, anc = _steered(h, x0, a["lens"], a["visits"], a["coef"], None, 5, a["event"], a["P_"], a["params"], a["u"],
                                                 n_visits=a["n_visits"], outs=a["outs"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all() and (anc == -7).all(), word
        assert terms is None or ((terms == SENTINEL).all() and (rew == SENTINEL).all() and (logw == SENTINEL).all()), word
    for (a, b, s, cu, cv, z), word in [((1.0, -1.0, 0.5, 1.0, -1.0, None), b"z is required"), ((1.0, -1.0, 0.0, np.inf, -1.0, None), b"not finite"),
                                       ((1.0, -1.0, 0.0, 1.0, np.nan, None), b"not finite")]:
        rc, eps, x0_out, out = _step_x0(h, x0, 3, LENS_D, a, b, s, cu, cv, z)
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all() and (eps == SENTINEL).all() and (x0_out == SENTINEL).all()
    xs, ls, buf = np.ascontiguousarray(x0), np.array(LENS_D, np.int32), np.full_like(x0, SENTINEL)
    rc = lib.fd_p_sample_step_coef_x0(h, P(xs), 3, P(ls), 6, L_D, 1.0, -1.0, 0.0, 1.0, -1.0, None, 1, None, None, P(buf))
    assert rc == -1 and b"null" in lib.fd_last_error() and (buf == SENTINEL).all()      # x0_out is required
    # a steered run, then the plain and the strided sampler are what they were: the per-run values are clean again
    rc, run, _, rew, _, anc = _steered(h, x0, LENS_D, visits, coef, None, 5, event, P_D, _params(), u)
    assert rc == 0 and np.isfinite(run[_valid(LENS_D, L_D)]).all() and np.isfinite(rew).all(), lib.fd_last_error()
    after = _sample_plain(h, x0, LENS_D, T_D - 1, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))
    rc, after_strided = _strided(h, x0, LENS_D, visits, coef[:3], 5, 1)
    assert rc == 0 and np.array_equal(_bits(after_strided), _bits(before_strided))
    # ... and a steered run after a solver run (which leaves a table c | u | v and a previous prediction behind) is its own
    rc, _ = _solver(h, x0, LENS_D, visits, scoef, 1)
    assert rc == 0
    rc, again, _, rew2, _, anc2 = _steered(h, x0, LENS_D, visits, coef, None, 5, event, P_D, _params(), u)
    assert rc == 0 and np.array_equal(_bits(again), _bits(run)) and np.array_equal(anc2, anc) and np.array_equal(rew2, rew)


# ---------------------------------------------------------------------------------- g. Python end to end
def test_steer_end_to_end_on_a_tiny_model(gpu, monkeypatch):
    _, _, pm = _pair(seed=11, precision="f16x3")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64), timesteps=20, beta_schedule="cosine")
    lengths = [30, 41, 30]
    kw = dict(n_particles=4, reward={"clashes": -1.0, "rg": -0.2, "strand": 1.0}, lam=1.5, ess_frac=0.9, num_steps=6, seed=7, batch_size=8)
    torch.manual_seed(3)
    best, info = sampling.steer(pm, ds, lengths, select="best", **kw)
    torch.manual_seed(3)
    every, info_all = sampling.steer(pm, ds, lengths, select="all", **kw)
    assert [s.shape for s in best] == [(l, F) for l in lengths] and [s.shape for s in every] == [(l, F) for l in lengths for _ in range(4)]
    assert info["terms"].shape == (3, 4) and info_all["terms"].shape == (12, 4) and info["events"].sum() >= 1
    assert len(info["ancestors"]) == 2 and info["ancestors"][0].shape == (int(info["events"].sum()), 8)   # batches of two groups, then one
    for g in range(3):
        group = info_all["reward"][4 * g: 4 * g + 4]
        assert info["reward"][g] == group.max() and info["index"][g] == 4 * g + int(np.argmax(group))
        assert np.array_equal(_bits(best[g]), _bits(every[info["index"][g]]))
    for s in every:
        assert np.isfinite(s).all() and (s >= -np.float32(np.pi)).all() and (s < np.float32(np.pi)).all()
    # the returned terms are those of the returned angles (which carry the dataset's offset already: none here)
    terms, rew = structures.steer_terms(every, NAMES, reward=kw["reward"])
    assert np.array_equal(terms, info_all["terms"]) and np.array_equal(rew, info_all["reward"])
    torch.manual_seed(3)
    again, info2 = sampling.steer(pm, ds, lengths, select="best", **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, best)) and np.array_equal(info2["reward"], info["reward"])
    with pytest.raises(ValueError):
        sampling.steer(pm, ds, lengths, n_particles=4, eta=0.0, num_steps=6)
