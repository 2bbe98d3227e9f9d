"""Restraint guidance combined with replacement on the device (fd_scaffold_guide_step, fd_sample_guided_inpaint,
sampling.guide_inpaint / scaffold_segments, bin/sample_restrained.py --hold_motif) against the numpy float64
statement of tests/scaffold_guide_reference.py and against the existing entries composed on the host: bits are compared with
==, everything else with the bound stated at its test."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guide_reference as gr
import inpaint_reference as ipr
import relax_reference as xr
import scaffold_guide_reference as sg
import strided_inpaint_reference as sir
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_model, ref_sampling
from test_gpu_parity import PRECISIONS, _inputs, _pair, _write_model_dir
from test_guide import IDX, random_features
from test_guide_gpu import _ca_restraints, _f64bits, _guide_step, _guided, _nerf, _pack, _scan
from test_inpaint_gpu import _device_draws
from test_repeat_gpu import LENS4, L_R, _tie
from test_steer_gpu import MODEL_D, NAMES, OFFSET, _step_x0
from test_strided_gpu import ANG, SENTINEL, _bits, _strided
from test_strided_inpaint_gpu import _step_coef_inpaint, _strided_inpaint

pytestmark = pytest.mark.gpu
P = _binding.ptr
CLASH = sg.Clash(0.63, 0.15, 1.0)
NO_CLASH = sg.Clash(0.63, 0.15, 0.0)
RAGGED = [1, 2, 3, 7, 12, 12]
OFFSETS = {6: OFFSET, 9: np.concatenate([OFFSET, np.array([0.02, -0.01, 0.03], dtype=np.float32)])}
MIXED9 = [1, 1, 1, 0, 0, 1, 0, 0, 0]


def _err():
    return _binding.load().fd_last_error()


def _valid(lens, L, Fx):
    v = np.zeros((len(lens), L, Fx), dtype=bool)
    for b, n in enumerate(lens):
        v[b, :n] = True
    return v


def _params(Fx=6, offset=None, max_norm=1.0, clash=NO_CLASH, idx=None):
    p = _binding.FdScaffoldGuideParams()
    p.feat_idx[:] = [int(v) for v in (IDX[Fx] if idx is None else idx)]
    p.has_offset = 0 if offset is None else 1
    if offset is not None:
        p.offset[:Fx] = [float(v) for v in offset]
    p.max_norm, p.clash_alpha, p.clash_margin, p.w_clash = max_norm, clash.alpha, clash.margin, clash.w
    return p


def _sg_step(x, x0, known, fixed, lens, packed, c, max_norm=1.0, s=0.0, z=None, seed=0, t=0, seq_offset=0, offset=None, is_angle=None,
             clash=NO_CLASH):
    """fd_scaffold_guide_step -> (rc, x_out, energy [B, 2], max_violation, gnorm, dfeats); the outputs start at the sentinel."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    xs = arr(x)
    B, L, Fx = xs.shape
    ang = arr(np.asarray([True] * Fx if is_angle is None else is_angle, dtype=bool), np.uint8)
    out, e, mv, gn = np.full_like(xs, SENTINEL), np.full((B, 2), SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL)
    G = np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    prm = _params(Fx, offset, max_norm, clash)
    rc = _binding.load().fd_scaffold_guide_step(0, P(xs), P(arr(x0)), P(arr(known)), P(arr(fixed, np.uint8)), P(arr(lens, np.int32)), B, L, Fx, P(ang),
                                                C.byref(prm), *(P(a) for a in packed), C.c_float(c), C.c_float(s), P(arr(z)), C.c_uint64(seed),
                                                int(t), C.c_int64(seq_offset), P(out), P(e), P(mv), P(gn), P(G))
    return rc, out, e, mv, gn, G


def _scan_builder(ang, idx):
    """The statement's coordinates: fd_nerf_scan (center = 0) of one chain's float32 rows."""
    return _scan(np.asarray(ang, dtype=np.float32)[None], [len(ang)], idx, 0)[0]


def _relax_G(ang, lens, packed, Fx, clash):
    """fd_relax_energy's dfeats_out on float32 rows [B, L, F]: no tether, every NeRF column movable, nothing fixed."""
    prm = _binding.FdRelaxParams()
    prm.feat_idx[:] = [int(v) for v in IDX[Fx]]
    for f in range(Fx):
        prm.is_angle[f], prm.move[f] = 1, int(f in set(IDX[Fx].tolist()))
    prm.clash_alpha, prm.clash_margin, prm.w_clash, prm.w_tether = clash.alpha, clash.margin, clash.w, 0.0
    prm.step0, prm.grow, prm.shrink, prm.max_step = 0.01, 1.2, 0.5, 0.5
    feats = np.ascontiguousarray(ang, dtype=np.float32)
    B, L, _ = feats.shape
    e, gn, G = np.empty((B, 3)), np.empty(B), np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    rc = _binding.load().fd_relax_energy(0, P(feats), None, P(np.ascontiguousarray(lens, dtype=np.int32)), B, L, Fx, C.byref(prm), None,
                                         *(P(a) for a in packed), P(e), P(gn), P(G))
    assert rc == 0, _err()
    return e, G


def _step_case(lens, Fx, seed):
    """x (sentinel beyond the lengths), x0, known in model space and a mixed per-element mask: whole rows, a row with ONE fixed
    element, scattered elements; the last chain has nothing fixed.  Restraints between CA atoms where a chain has three
    residues or more, weighted so that the clip is active on some chains and inactive on others."""
    rng = np.random.default_rng(seed)
    B, L = len(lens), max(lens)
    to_model = lambda rows: (rows - OFFSETS[Fx]).astype(np.float32)   # noqa: E731  (any finite value is a model-space value)
    x = np.full((B, L, Fx), SENTINEL, dtype=np.float32)
    x0, known = np.zeros((B, L, Fx), np.float32), np.full((B, L, Fx), np.nan, np.float32)
    fixed = np.zeros((B, L, Fx), np.uint8)
    per = []
    for b, n in enumerate(lens):
        x[b, :n] = _inputs(1, n, Fx, seed=seed + b).numpy()[0]
        x0[b, :n] = to_model(random_features(rng, n, Fx))
        target = np.zeros((L, Fx), np.float32)
        target[:n] = to_model(random_features(rng, n, Fx))
        if b < B - 1 or B == 1:
            if n >= 7:
                fixed[b, 2: n // 2] = 1                       # whole rows
                fixed[b, n // 2 + 1, 3] = 1                   # a row with one fixed element
            fixed[b, :n][rng.random((n, Fx)) < 0.15] = 1      # scattered
            if n <= 3:
                fixed[b, 0, 1] = 1
        known[b][fixed[b] == 1] = target[fixed[b] == 1]
        res = list(range(0, n, max(1, n // 5)))[:5]
        per.append(_ca_restraints(rng, res, n, w=1.0 if b % 2 == 0 else 1e-6) if n >= 3 else ([], [], [], [], []))
    return x, x0, known, fixed, per, _pack(per)


# ---------------------------------------------------------------------------------- 1. the step hook against the statement
@pytest.mark.parametrize("lens,Fx", [(RAGGED, 6), (RAGGED, 9), ([86], 6), ([86], 9)])
def test_step_equals_the_statement_and_leaves_fixed_elements_alone(gpu, lens, Fx):
    """x_out within 2e-6 of the statement (fd_guide_step's gate: G agrees to 1e-9, what remains is five float32 roundings of
    values below 8, each at most a half-ulp step of 2.4e-7 apart), on the circle for wrapped columns; energies, norm and
    violation within 1e-9 relative.  The statement's coordinates are fd_nerf_scan's, as the statement says.  Fixed elements: x_out holds x's bits, dfeats_out is exactly 0; rows at or beyond a length
    are untouched.  86 residues: 258 atoms, the first length with more than one atom per lane."""
    x, x0, known, fixed, per, packed = _step_case(lens, Fx, 40 + Fx + len(lens))
    L = max(lens)
    ok, fx = _valid(lens, L, Fx), fixed.astype(bool)
    x0_poisoned = np.where(fx, np.float32(np.nan), x0)                                      # x0 is not read where fixed
    z = np.random.default_rng(41).standard_normal(x.shape).astype(np.float32)
    is_angle = ANG if Fx == 6 else MIXED9
    clipped, unclipped = 0, 0
    for c, s, clash in ((0.05, 0.0, NO_CLASH), (0.05, 0.3, CLASH), (-0.2, 0.3, CLASH)):
        rc, got, e, mv, gn, G = _sg_step(x, x0_poisoned, known, fixed, lens, packed, c, s=s, z=z, offset=OFFSETS[Fx], is_angle=is_angle, clash=clash)
        assert rc == 0, _err()
        want, we, wmv, wn, clip, Gs = sg.step(np.where(ok, x, 0), x0, np.nan_to_num(known), fx, lens, IDX[Fx], OFFSETS[Fx], is_angle, per, c, 1.0, s=s,
                                              z=z, clash=clash, build=_scan_builder)
        ang = np.asarray(is_angle, dtype=bool)
        dist = np.where(ang, ref_sampling.circ_dist(got, want), np.abs(got.astype(np.float64) - want))[ok]
        rel = lambda a, b: np.abs(a - b) <= 1e-9 * np.abs(b)   # noqa: E731
        print(f"F={Fx} lens={lens} c={c} s={s} w_clash={clash.w}: max distance {dist.max():.2e}; E {e.tolist()}; gnorm {np.round(wn, 4).tolist()}, "
              f"clipped {(clip < 1).tolist()}")
        assert dist.max() <= 2e-6
        assert rel(e[:, 0], we[:, 0]).all() and rel(e[:, 1], we[:, 1]).all() and rel(mv, wmv).all() and rel(gn, wn).all()
        assert (e[:, 1] == 0).all() if clash.w == 0 else (e[:, 1] > 0).any()
        assert np.array_equal(_bits(got)[fx], _bits(x)[fx]) and (G[fx] == 0).all()
        assert (got[~ok] == SENTINEL).all() and (G[~ok] == SENTINEL).all()
        for b, n in enumerate(lens):
            scale = max(np.abs(Gs[b]).max(), 1e-300)
            assert np.abs(G[b, :n] - Gs[b]).max() <= 1e-9 * scale, b
        clipped, unclipped = clipped + int((clip < 1).sum()), unclipped + int((clip == 1).sum())
        free = ok & ~fx
        rc, plain, *_ = _sg_step(x, x0_poisoned, known, fixed, lens, packed, 0.0, s=s, z=z, offset=OFFSETS[Fx], is_angle=is_angle, clash=clash)
        assert rc == 0 and np.abs(got - plain)[free].max() > 1e-4                           # ... and the step was taken
    assert clipped > 0 and (unclipped > 0 or len(lens) == 1)


def test_step_with_c_zero_draws_as_the_tie_statement_and_only_on_free_elements(gpu):
    """c = 0: a free element is fd_tie_repeats' (nothing tied) bit for bit -- the same draw position and Philox word, explicit z
    or not; a fixed one keeps x's bits."""
    x, x0, known, fixed, _, packed = _step_case(RAGGED, 6, 50)
    ok, fx = _valid(RAGGED, 12, 6), fixed.astype(bool)
    z = np.random.default_rng(51).standard_normal(x.shape).astype(np.float32)
    for kw in (dict(), dict(s=0.3, z=z), dict(s=0.3, z=None, seed=(7 << 40) + 99, t=5, seq_offset=1 << 33)):
        rc, got, *_ = _sg_step(x, x0, known, fixed, RAGGED, packed, 0.0, offset=OFFSET, clash=CLASH, **kw)
        assert rc == 0, _err()
        rc, want = _tie(x, RAGGED, [(0, 1, 1)] * 6, ANG, **kw)
        assert rc == 0, _err()
        assert np.array_equal(_bits(got)[ok & ~fx], _bits(want)[ok & ~fx]) and np.array_equal(_bits(got)[fx], _bits(x)[fx]), sorted(kw)
        assert (got[~ok] == SENTINEL).all()


# ---------------------------------------------------------------------------------- 2. against the entries it shares launches with
@pytest.mark.parametrize("Fx", [6, 9])
def test_unmasked_gradient_is_fd_relax_energys_bit_for_bit(gpu, Fx):
    """Nothing fixed: dfeats_out equals fd_relax_energy's dfeats_out on the shifted rows (no tether, every NeRF column movable),
    with and without the clash term, and so do the energies.  (== on the values: where the clash weight is 0 fd_relax_energy
    still adds the clash launch's zeros, which can turn a -0.0 into +0.0.)"""
    for lens in (RAGGED, [86]):
        x, x0, known, fixed, per, packed = _step_case(lens, Fx, 60 + Fx)
        L = max(lens)
        ok = _valid(lens, L, Fx)
        nothing = np.zeros_like(fixed)
        shifted = np.zeros_like(x0)
        for b, n in enumerate(lens):
            shifted[b, :n] = gr.shift(x0[b, :n], OFFSETS[Fx], [True] * Fx)
        for clash in (CLASH, NO_CLASH):
            rc, _, e, _, _, G = _sg_step(x, x0, known, nothing, lens, packed, 0.05, offset=OFFSETS[Fx], clash=clash)
            assert rc == 0, _err()
            e3, G_relax = _relax_G(shifted, lens, packed, Fx, clash)
            assert np.array_equal(G[ok], G_relax[ok]) and np.abs(G[ok]).max() > 0, (lens, clash.w)
            assert np.array_equal(e[:, 0], e3[:, 1]) and np.array_equal(e[:, 1], e3[:, 0]) and (e3[:, 2] == 0).all()


def test_nothing_fixed_and_no_clash_term_is_fd_guide_step_up_to_the_scan(gpu):
    """fixed all zero, w_clash = 0: the statement is fd_guide_step's with fd_nerf_scan in place of fd_nerf.  The scan is within
    1e-9 of the chain's extent of fd_nerf, which moves G by about 1e-6 of itself and a clipped step of at most 0.2 by far less
    than a float32 ulp of pi (2.4e-7): x_out within 2e-6, fd_guide_step's own gate.  Measured: DESIGN.md 6y."""
    worst, worst_scan = 0.0, 0.0
    for lens in (RAGGED, [86]):
        x, x0, known, fixed, per, packed = _step_case(lens, 6, 70)
        ok = _valid(lens, max(lens), 6)
        z = np.random.default_rng(71).standard_normal(x.shape).astype(np.float32)
        shifted = np.zeros_like(x0)
        for b, n in enumerate(lens):
            shifted[b, :n] = gr.shift(x0[b, :n], OFFSET, ANG)
        serial, scan = _nerf(shifted, lens, IDX[6], 0), _scan(shifted, lens, IDX[6], 0)
        for b, n in enumerate(lens):
            d = np.abs(scan[b, : 3 * n] - serial[b, : 3 * n]).max()
            assert d <= xr.scan_gate(serial[b, : 3 * n]), (b, d)
            worst_scan = max(worst_scan, d / (xr.scan_gate(serial[b, : 3 * n]) * 1e9))
        for c, s in ((0.05, 0.0), (-0.2, 0.3)):
            rc, got, e, _, gn, _ = _sg_step(x, x0, known, np.zeros_like(fixed), lens, packed, c, s=s, z=z, offset=OFFSET)
            assert rc == 0, _err()
            rc, want, we, wn = _guide_step(x, x0, lens, packed, c, s=s, z=z, offset=OFFSET)
            assert rc == 0, _err()
            dist = ref_sampling.circ_dist(got, want)[ok].max()
            worst = max(worst, float(dist))
            assert dist <= 2e-6 and (np.abs(e[:, 0] - we) <= 1e-9 * np.abs(we)).all() and (np.abs(gn - wn) <= 1e-6 * np.abs(wn)).all()
    print(f"fd_scaffold_guide_step against fd_guide_step: x_out differs by at most {worst:.2e}; scan against fd_nerf: {worst_scan:.2e} of the extent")


def test_two_calls_give_the_same_bits_and_a_chain_does_not_depend_on_its_batch(gpu):
    x, x0, known, fixed, per, packed = _step_case(RAGGED, 6, 80)
    kw = dict(s=0.3, z=None, seed=12345, t=3, offset=OFFSET, clash=CLASH)
    first = _sg_step(x, x0, known, fixed, RAGGED, packed, 0.05, **kw)
    again = _sg_step(x, x0, known, fixed, RAGGED, packed, 0.05, **kw)
    assert first[0] == 0 and again[0] == 0
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    b, n = 4, RAGGED[4]
    rc, out, e, mv, gn, G = _sg_step(x[b: b + 1, :n], x0[b: b + 1, :n], known[b: b + 1, :n], fixed[b: b + 1, :n], [n], _pack([per[b]]), 0.05,
                                     **dict(kw, seq_offset=b))
    assert rc == 0, _err()
    assert np.array_equal(_bits(out[0]), _bits(first[1][b, :n])) and np.array_equal(_f64bits(G[0]), _f64bits(first[5][b, :n]))
    assert np.array_equal(_f64bits(e[0]), _f64bits(first[2][b])) and gn[0] == first[4][b] and mv[0] == first[3][b]


# ---------------------------------------------------------------------------------- 3. the run
T_S, K_S = 20, 5


def _guided_inpaint(h, x0, lens, visits, coef, noise, known, fixed, kcoef, known_noise, seed, guide, packed, offset=OFFSET, max_norm=1.0,
                    clash=NO_CLASH, idx=None, n_visits=None, out=True, energy=True, params=True):
    """fd_sample_guided_inpaint -> (rc, out, energy [B, 2], max_violation); the outputs start at the sentinel."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    B = len(LENS4)
    vs = arr(visits, np.int32)
    K = n_visits if n_visits is not None else len(vs)
    prm = _params(6, offset, max_norm, clash, idx)
    buf = np.full((B, L_R, 6), SENTINEL, dtype=np.float32) if out else None
    e, mv = (np.full((B, 2), SENTINEL) if energy else None), np.full(B, SENTINEL)
    rc = _binding.load().fd_sample_guided_inpaint(h, P(arr(x0)), P(arr(lens, np.int32)), B, L_R, P(vs), K, P(arr(coef)), P(arr(noise)), P(arr(known)),
                                                  P(arr(fixed, np.uint8)), P(arr(kcoef)), P(arr(known_noise)), C.c_uint64(seed), C.c_int64(0),
                                                  P(arr(guide)), C.byref(prm) if params else None, *(P(a) for a in packed), P(buf), P(e), P(mv))
    return rc, buf, e, mv


def _run_case(betas, seed, eta=1.0, scale=1.0):
    """LENS4 = 16, 13, 9, 14: two held segments and a pinned lead element, scattered elements, nothing fixed, two segments and a
    single element."""
    visits = sampling.ddim_visits(T_S, K_S)
    coef = sampling.steer_coefficients(betas, visits, eta)
    guide = sampling.guidance_coefficients(betas, visits, coef, scale)
    x0 = _inputs(4, L_R, seed=290 + seed).numpy()
    rng = np.random.default_rng(291 + seed)
    noise = rng.standard_normal((K_S, 4, L_R, 6)).astype(np.float32)
    known_noise = rng.standard_normal((K_S + 1, 4, L_R, 6)).astype(np.float32)
    fixed = np.zeros((4, L_R, 6), np.uint8)
    fixed[0, 3:7], fixed[0, 10:14], fixed[0, 2, 3], fixed[0, 9, 3] = 1, 1, 1, 1
    fixed[1, :13][rng.random((13, 6)) < 0.2] = 1
    fixed[3, 2:5], fixed[3, 8:12], fixed[3, 6, 0] = 1, 1, 1
    known = np.where(fixed == 1, rng.uniform(-3.1, 3.1, fixed.shape).astype(np.float32), np.float32(np.nan))   # (not read where free)
    per = [_ca_restraints(rng, [3, 5, 10, 13], 16), _ca_restraints(rng, [0, 6, 12], 13, tol=0.5), ([], [], [], [], []),
           _ca_restraints(rng, [2, 4, 9, 11], 14, w=1e-3)]
    return visits, coef, guide, x0, noise, known_noise, known, fixed, _pack(per)


def _chain_of_hooks(h, x0, visits, coef, guide, noise, known_noise, known, fixed, kcoef, packed, seed, clash):
    """Per visit: fd_p_sample_step_coef_inpaint (s = 0, level_out = the landing level) for x, fd_p_sample_step_coef_x0 on the
    same input for x0, then fd_scaffold_guide_step.  noise None: Philox -- the replacement's draws are the device generator's
    own words, the statement's draw is the hook's own Philox."""
    B = len(LENS4)
    kn = np.nan_to_num(known)
    levels = sir.landing_levels(visits)
    draw = lambda i, q: known_noise[i] if known_noise is not None else _device_draws(h, seed, ipr.TAG | q, B, L_R)   # noqa: E731
    state = ipr.replace(x0, kn, fixed, int(visits[0]) + 1, kcoef, draw(0, int(visits[0]) + 1), ANG)
    for i, (t, q) in enumerate(zip(visits, levels)):
        a, b, s, u, v = coef[:, i]
        rc, _, x = _step_coef_inpaint(h, state, t, LENS4, a, b, 0.0, None, q, kn, fixed, kcoef, None if q == 0 else draw(i + 1, q))
        assert rc == 0, _err()
        rc, _, pred, _ = _step_x0(h, state, t, LENS4, a, b, 0.0, u, v, None)
        assert rc == 0, _err()
        rc, state, *_ = _sg_step(x, pred, known, fixed, LENS4, packed, guide[i], s=s, z=None if noise is None else noise[i], seed=seed, t=int(t),
                                 offset=OFFSET, clash=clash)
        assert rc == 0, _err()
    return state


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 20, K = 5, B = 4, L = 16, eta = 1, with and without the clash term, explicit draws and Philox; eager launches and
    packed rows give the same bits below the lengths; the final state's fixed elements are known's bits and energy_out is the
    hook's on the final state; with nothing fixed the same chain holds."""
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_S)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    ok = _valid(LENS4, L_R, 6)
    visits, coef, guide, x0, noise, known_noise, known, fixed, packed = _run_case(betas, 0)
    fx = fixed.astype(bool)
    assert (guide != 0).all() and (coef[2, :-1] != 0).all()
    for clash, zs, kz, seed in ((CLASH, noise, known_noise, 0), (NO_CLASH, None, None, 977)):
        rc, out, e, mv = _guided_inpaint(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, clash=clash)
        assert rc == 0, _err()
        want = _chain_of_hooks(h, x0, visits, coef, guide, zs, kz, known, fixed, kcoef, packed, seed, clash)
        assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), clash
        assert np.array_equal(_bits(out)[fx], _bits(known)[fx])
        rc, _, e_hook, mv_hook, _, _ = _sg_step(out, out, known, fixed, LENS4, packed, 0.0, offset=OFFSET, clash=clash)
        assert rc == 0 and np.array_equal(_f64bits(e), _f64bits(e_hook)) and np.array_equal(_f64bits(mv), _f64bits(mv_hook))
        assert e[2, 0] == 0 and (e[[0, 1, 3], 0] > 0).all() and ((e[:, 1] == 0).all() if clash.w == 0 else True)
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            rc, out2, e2, _ = _guided_inpaint(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, clash=clash)
            pm.set_option(option, int(option == "use_graph"))
            assert rc == 0 and np.array_equal(_bits(out2)[ok], _bits(out)[ok]) and np.array_equal(_f64bits(e2), _f64bits(e)), option
    nothing = np.zeros_like(fixed)
    rc, free_run, _, _ = _guided_inpaint(h, x0, LENS4, visits, coef, noise, known, nothing, kcoef, known_noise, 0, guide, packed)
    assert rc == 0, _err()
    want = _chain_of_hooks(h, x0, visits, coef, guide, noise, known_noise, known, nothing, kcoef, packed, 0, NO_CLASH)
    assert np.array_equal(_bits(free_run)[ok], _bits(want)[ok]) and not np.array_equal(free_run[ok], out[ok])
    # an all-zero guide table with eta = 0 draws nothing and steers nothing: fd_sample_strided_inpaint
    coef0 = sampling.steer_coefficients(betas, visits, 0.0)
    rc, unguided, _, _ = _guided_inpaint(h, x0, LENS4, visits, coef0, None, known, fixed, kcoef, known_noise, 5, np.zeros_like(guide), packed)
    assert rc == 0, _err()
    rc, plain = _strided_inpaint(h, x0, LENS4, visits, coef0[:3], np.nan_to_num(known), fixed, kcoef, 5, 0, known_noise=known_noise)
    assert rc == 0 and np.array_equal(_bits(unguided)[ok], _bits(plain[0])[ok])


def test_argument_errors_leave_the_outputs_alone(gpu):
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_S)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    visits, coef, guide, x0, _, _, known, fixed, packed = _run_case(betas, 3)
    nan_b, inf_v, nan_g = coef.copy(), coef.copy(), guide.copy()
    nan_b[1, 2], inf_v[4, 1], nan_g[3] = np.nan, np.inf, np.nan
    bad_off = OFFSET.copy()
    bad_off[4] = np.nan
    nan_known, beyond = known.copy(), fixed.copy()
    nan_known[0, 4, 2], beyond[1, 14, 0] = np.nan, 1

    def rst(k, value):
        arrays = [a.copy() for a in packed]
        arrays[k][0] = value
        return tuple(arrays)

    none_at = lambda k: tuple(None if i == k else a for i, a in enumerate(packed))   # noqa: E731
    bad = [(dict(x0=None), b"null"), (dict(lens=None), b"null"), (dict(out=False), b"null"), (dict(guide=None), b"null"), (dict(params=False), b"null"),
           (dict(energy=False), b"null"), (dict(visits=None, n_visits=5), b"visits is null"), (dict(coef=None), b"coef is null"),
           (dict(n_visits=0), b"n_visits = 0"), (dict(visits=[20, 15, 9, 4, 0]), b"visits[0] = 20 outside"), (dict(visits=[19, 15, 15, 4, 0]), b"visits[2] = 15 follows 15"),
           (dict(coef=nan_b), b"coef[1][2]"), (dict(coef=inf_v), b"coef[4][1]"), (dict(guide=nan_g), b"guide[3]"),
           (dict(lens=[16, 13, 0, 14]), b"lens[2]=0"), (dict(lens=[17, 13, 9, 14]), b"lens[0]=17"),
           (dict(max_norm=0.0), b"max_norm=0"), (dict(max_norm=float("inf")), b"max_norm=inf"), (dict(offset=bad_off), b"offset[4]"),
           (dict(idx=[0, 1, 6, 3, 4, 5, -1, -1, -1]), b"feat_idx[2]=6"), (dict(idx=[0, 1, 2, 3, 4, 4, -1, -1, -1]), b"feat_idx[5]=4 repeats"),
           (dict(packed=none_at(0)), b"rst_offsets"), (dict(packed=none_at(2)), b"restraint lists"), (dict(packed=rst(1, 48)), b"restraint 0 = atoms (48, "),
           (dict(packed=rst(3, -0.5)), b"restraint 0: d0"), (dict(packed=rst(4, np.inf)), b"restraint 0: tol"), (dict(packed=rst(5, np.nan)), b"restraint 0: w"),
           (dict(known=None), b"known is null"), (dict(fixed=None), b"fixed is null"), (dict(kcoef=None), b"known_coef is null"),
           (dict(known=nan_known), b"known is not finite at a fixed element: sequence 0 position 4 feature 2"),
           (dict(fixed=beyond), b"fixed element beyond a length: sequence 1 position 14"),
           (dict(clash=sg.Clash(-0.1, 0.15, 1.0)), b"clash_alpha=-0.1"), (dict(clash=sg.Clash(0.63, float("nan"), 1.0)), b"clash_margin="),
           (dict(clash=sg.Clash(0.63, 0.15, -1.0)), b"w_clash=-1"), (dict(clash=sg.Clash(0.63, 0.15, float("inf"))), b"w_clash=inf")]
    for kw, word in bad:
        a = dict(x0=x0, lens=LENS4, visits=visits, coef=coef, guide=guide, packed=packed, n_visits=None, out=True, params=True, energy=True,
                 max_norm=1.0, offset=OFFSET, idx=None, known=known, fixed=fixed, kcoef=kcoef, clash=CLASH)
        a.update(kw)
        rc, out, e, mv = _guided_inpaint(h, a["x0"], a["lens"], a["visits"], a["coef"], None, a["known"], a["fixed"], a["kcoef"], None, 5, a["guide"],
                                         a["packed"], offset=a["offset"], max_norm=a["max_norm"], clash=a["clash"], idx=a["idx"], n_visits=a["n_visits"],
                                         out=a["out"], energy=a["energy"], params=a["params"])
        assert rc == -1 and word in _err(), (word, rc, _err())
        assert (out is None or (out == SENTINEL).all()) and (e is None or (e == SENTINEL).all()) and (mv == SENTINEL).all(), word


def test_other_families_give_their_bits_before_and_after_on_the_same_handle(gpu):
    """tests/call_history_cases.py's pattern: a plain strided, a guided and a conditioned run give, behind an
    fd_sample_guided_inpaint on the same handle, the bits they give first on a fresh handle -- and the new run gives its own
    bits behind them."""
    betas = beta_schedules.cosine_beta_schedule(T_S)
    kcoef = sampling.inpaint_levels(betas)
    visits, coef, guide, x0, _, known_noise, known, fixed, packed = _run_case(betas, 5)
    kn = np.nan_to_num(known)

    def others(h):
        a = _strided(h, x0, LENS4, visits, coef[:3], 11, 0)
        b = _guided(h, x0, LENS4, visits, coef, None, 12, guide, packed)
        c = _strided_inpaint(h, x0, LENS4, visits, coef[:3], kn, fixed, kcoef, 13, 0)
        assert a[0] == 0 and b[0] == 0 and c[0] == 0, _err()
        return a[1], b[1], b[2], c[1]

    def new(h, seed=14):
        rc, out, e, mv = _guided_inpaint(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, seed, guide, packed, clash=CLASH)
        assert rc == 0, _err()
        return out, e, mv

    same = lambda xs, ys: all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(xs, ys))   # noqa: E731
    _, _, pm1 = _pair(precision="f16x3", **MODEL_D)
    h1 = pm1.prepare(betas)
    fresh_others = others(h1)
    after_others = new(h1)
    _, _, pm2 = _pair(precision="f16x3", **MODEL_D)
    h2 = pm2.prepare(betas)
    fresh_new = new(h2)
    assert same(fresh_new, after_others)
    assert same(others(h2), fresh_others)                  # behind the new run: what a fresh handle gives
    assert same(new(h2), fresh_new) and same(others(h1), fresh_others)
    assert not np.array_equal(new(h2, seed=15)[0], fresh_new[0])     # the seed reaches both noise streams


# ---------------------------------------------------------------------------------- 4. Python end to end
def test_scaffold_segments_holds_every_segment_on_a_tiny_model(gpu):
    """Two segments of a 12-residue motif in chains of 30 and 34 residues: each held segment's N / CA / C backbone is within
    1e-3 A of the motif's after superposition (structures.motif_rmsd's usual gate), the returned energies are
    structures.restraint_energy's of the returned backbones, and the run is reproducible.  Nothing is asked of the energy
    itself: the weights are random."""
    _, _, pm = _pair(seed=11, precision="f16x3")
    inner = datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=OFFSET)
    ds = datasets.NoisedAnglesDataset(inner, timesteps=20, beta_schedule="cosine")
    motif_angles = random_features(np.random.default_rng(6), 12, 6)
    motif_xyz = nerf.build_backbones([motif_angles], NAMES, center_coords=False)[0]
    segs = [(1, 5, 4), (7, 11, 20)]
    kw = dict(num_steps=6, scale=1.0, max_norm=1.0, clash_weight=1.0, batch_size=1)   # two calls
    torch.manual_seed(3)
    got, info = sampling.scaffold_segments(pm, ds, motif_angles, motif_xyz, segs, [30, 34], **kw)
    assert [s.shape for s in got] == [(30, 6), (34, 6)] and all(np.isfinite(s).all() for s in got)
    coords = nerf.build_backbones(got, NAMES, center_coords=False)
    for lo, hi, at in segs:
        rmsd = structures.motif_rmsd(coords, motif_xyz[3 * lo: 3 * hi], [at, at])
        print(f"segment [{lo}, {hi}) at {at}: RMSD {rmsd.tolist()}")
        assert (rmsd <= 1e-3).all()
    rst = structures.segment_restraints(motif_xyz, segs)
    e, mv = structures.restraint_energy(nerf.build_backbones(got, NAMES, center_coords=False, method="scan"), rst)
    assert np.allclose(info["energy"], e, rtol=1e-9, atol=0) and np.allclose(info["max_violation"], mv, rtol=1e-9, atol=0)
    assert info["clash_energy"].shape == (2,) and (info["clash_energy"] >= 0).all() and len(rst) == 16
    torch.manual_seed(3)
    again, info2 = sampling.scaffold_segments(pm, ds, motif_angles, motif_xyz, segs, [30, 34], **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, got)) and np.array_equal(info2["energy"], info["energy"])


def test_script_holds_the_motif_and_reports_the_clash_energy(gpu, tmp_path):
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    from foldingdiff_amd.angles_and_coords import write_coords_to_pdb
    motif_pdb = write_coords_to_pdb(gr.build_ref(random_features(np.random.default_rng(4), 30, 6), IDX[6]), str(tmp_path / "motif.pdb"))
    contacts = tmp_path / "contacts.txt"
    contacts.write_text("0 35\n2 30 6.5\n")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_restrained.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "36",
                        "--num_steps", "5", "--seed", "3", "--contacts", str(contacts), "--motif_pdb", motif_pdb, "--motif_residues", "3-6,20-22",
                        "--placed_at", "8,25", "--hold_motif", "--clash_weight", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "restraints.json", "sampled_angles", "sampled_pdb"]
    names = [f"generated_{i}.pdb" for i in range(2)]
    assert sorted(os.listdir(os.path.join(out, "sampled_pdb"))) == names
    with open(os.path.join(out, "restraints.json")) as fh:
        report = json.load(fh)
    assert report["n_restraints"] == 2 + 4 * 3                                             # the contacts and the pairs ACROSS the two ranges
    for key in ("energy", "max_violation", "clash_energy", "motif_ca_rmsd"):
        assert sorted(report[key]) == names and all(np.isfinite(v) and v >= 0 for v in report[key].values()), key
