"""Cyclic oligomers on the device (fd_symmetry_energy, fd_symmetry_dock, fd_scaffold_guide_step_sym, fd_sample_guided_inpaint_sym,
structures.dock_cyclic, sampling.sample_symmetric, bin/sample_symmetric.py) against the numpy float64 statements
of tests/symmetry_reference.py and against the existing entries: bits are compared with ==, everything else with the bound
stated at its test."""
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
import scaffold_guide_reference as sg
import strided_inpaint_reference as sir
import symmetry_reference as sr
import template_reference as tr
from conftest import REPO
from foldingdiff_amd import _binding, angles_and_coords, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_model, ref_sampling
from test_gpu_parity import PRECISIONS, _pair, _write_model_dir
from test_guide import IDX, random_features
from test_guide_gpu import _f64bits, _pack
from test_inpaint_gpu import _device_draws
from test_repeat_gpu import LENS4, L_R
from test_scaffold_guide_gpu import CLASH, NO_CLASH, OFFSETS, T_S, _params, _run_case, _scan_builder, _step_case, _valid
from test_steer_gpu import MODEL_D, NAMES, OFFSET, _step_x0
from test_strided_gpu import ANG, SENTINEL, _bits, _strided
from test_strided_inpaint_gpu import _step_coef_inpaint
from test_template_gpu import NO_TPL, _guided_inpaint_tpl, _pack_tpl, _padded, _run_templates, _sg_step_tpl, _step_templates

pytestmark = pytest.mark.gpu
P = _binding.ptr
# 86 residues: 258 atoms, the first length with two blocks of lanes; 342: 1026 atoms, one more than the LDS tile holds
LENS = [1, 2, 3, 7, 12, 86]
ORDERS = [2, 3, 1, 4, 7, 3]
LONG, LONG_ORDER = 342, 2
PRM = sr.Params(r_max=0.5)       # the radial term is exactly zero on the chain whose centroid lies within 0.5 A of the axis
ON_AXIS = 3                      # that chain


def _err():
    return _binding.load().fd_last_error()


def _sym_params(prm=PRM, **kw):
    p = structures.symmetry_params(alpha=prm.alpha, margin=prm.margin, clash_weight=prm.w_clash, contact_weight=prm.w_contact, d_on=prm.d_on,
                                   d_off=prm.d_off, radial_weight=prm.w_radial, r_max=prm.r_max, lever=prm.lever, max_shift=prm.max_shift,
                                   step0=prm.step0, grow=prm.grow, shrink=prm.shrink, pose_iters=prm.pose_iters)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _poses_near_the_axis(chains, rng, on_axis=None):
    """Random proper rotations; the CA centroid 1.5 to 2.5 A from the axis, so that the copies overlap (``on_axis``: 0.3 A)."""
    poses = []
    for b, c in enumerate(chains):
        Q = tr.random_rotation(rng)
        rho, phi = (0.3 if b == on_axis else rng.uniform(1.5, 2.5)), rng.uniform(0, 2 * np.pi)
        centre = np.array([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(-3, 3)])
        poses.append(np.concatenate([Q.reshape(9), centre - Q @ c[1::3].mean(axis=0)]))
    return np.array(poses)


@pytest.fixture(scope="module")
def batch():
    """The ragged batch with the long chain behind it, the reference's values, and the seed that keeps every CA pair between
    copies at least 1e-6 A from d_on, so that no contact count rests on rounding: walked up from 0, at most 8 tries."""
    for seed in range(8):
        rng = np.random.default_rng(5000 + seed)
        chains = [gr.build_ref(random_features(rng, n, 6), IDX[6]) for n in LENS + [LONG]]
        orders = ORDERS + [LONG_ORDER]
        poses = _poses_near_the_axis(chains, rng, on_axis=ON_AXIS)
        ref = [sr.energy(c, o, p, PRM) for c, o, p in zip(chains, orders, poses)]
        if min(r.min_gap for r in ref) >= 1e-6:
            print(f"seed {seed}: the closest CA pair to d_on is {min(r.min_gap for r in ref):.2e} A from it")
            return dict(chains=chains, orders=np.array(orders, np.int32), poses=poses, ref=ref)
    pytest.fail("no seed below 8 keeps every CA pair 1e-6 A from d_on")


def _energy(chains, orders, poses, prm=None, wrench=True, grad=True):
    """fd_symmetry_energy -> (rc, energy [B, 3], contacts, wrench, dcoords); the outputs start at the sentinel."""
    coords, lens = _padded(chains)
    B, L = coords.shape[0], coords.shape[1] // 3
    e, c = np.full((B, 3), SENTINEL), np.full(B, -7, np.int32)
    w = np.full((B, 6), SENTINEL) if wrench else None
    g = np.full(coords.shape, SENTINEL) if grad else None
    prm = _sym_params() if prm is None else prm
    rc = _binding.load().fd_symmetry_energy(0, P(np.ascontiguousarray(coords)), P(np.asarray(lens, np.int32)), B, L, P(np.ascontiguousarray(orders, dtype=np.int32)),
                                            P(np.ascontiguousarray(poses, dtype=np.float64)), C.byref(prm), P(e), P(c), P(w), P(g))
    return rc, e, c, w, g


def _dock(chains, orders, poses, n_iter, step=None, prm=None, trace=True):
    """fd_symmetry_dock -> (rc, pose, energy, contacts, trace, accepted, step)."""
    coords, lens = _padded(chains)
    B, L = coords.shape[0], coords.shape[1] // 3
    po, e, c, acc = np.full((B, 12), SENTINEL), np.full((B, 3), SENTINEL), np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    tr_ = np.full((n_iter + 1, B), SENTINEL) if trace else None
    h = None if step is None else np.ascontiguousarray(step, dtype=np.float64).copy()
    prm = _sym_params() if prm is None else prm
    rc = _binding.load().fd_symmetry_dock(0, P(np.ascontiguousarray(coords)), P(np.asarray(lens, np.int32)), B, L, P(np.ascontiguousarray(orders, dtype=np.int32)),
                                          P(np.ascontiguousarray(poses, dtype=np.float64)), C.byref(prm), n_iter, P(h), P(po), P(e), P(c), P(tr_), P(acc))
    return rc, po, e, c, tr_, acc, h


# ---------------------------------------------------------------------------------- 1. the statement
def test_symmetry_energy_equals_the_statement(gpu, batch):
    """Energies within 1e-9 relative, F and tau within 1e-9 of their lengths (F_z and tau_z are rounding noise around 0, so a
    gate per component would gate nothing), dcoords within 1e-9 of the chain's largest entry, contacts equal.  The chain of
    order 1 gives zeros everywhere; the chain whose centroid lies within r_max of the axis has E_radial == 0 exactly."""
    chains, orders, poses, ref = batch["chains"], batch["orders"], batch["poses"], batch["ref"]
    rc, e, c, w, g = _energy(chains, orders, poses)
    assert rc == 0, _err()
    nonzero = np.zeros(3, dtype=int)
    for b, (x, r) in enumerate(zip(chains, ref)):
        n = len(x)
        scale = np.abs(r.dcoords).max()
        err_g = np.abs(g[b, :n] - r.dcoords).max() / scale if scale > 0 else np.abs(g[b, :n]).max()
        err_e = np.abs(e[b] - r.e) / np.where(r.e != 0, np.abs(r.e), 1.0)
        nF, nT = np.linalg.norm(r.wrench[:3]), np.linalg.norm(r.wrench[3:])
        err_w = (np.linalg.norm(w[b, :3] - r.wrench[:3]) / max(nF, 1e-300), np.linalg.norm(w[b, 3:] - r.wrench[3:]) / max(nT, 1e-300))
        print(f"len {n // 3} order {orders[b]}: E {e[b].tolist()} contacts {c[b]}; relative errors E {err_e.max():.1e} F {err_w[0]:.1e} tau {err_w[1]:.1e} "
              f"dcoords {err_g:.1e}; |F_z|/|F| {abs(w[b, 2]) / max(nF, 1e-300):.1e}")
        assert (err_e <= 1e-9).all() and c[b] == r.contacts and err_g <= 1e-9
        assert (g[b, n:] == 0).all()
        if orders[b] == 1:
            assert not e[b].any() and c[b] == 0 and not w[b].any() and not g[b].any()
        else:
            assert max(err_w) <= 1e-9 and abs(w[b, 2]) <= 1e-10 * nF and abs(w[b, 5]) <= 1e-10 * nT
        nonzero += (e[b] != 0)
    assert e[ON_AXIS, 2] == 0 and ref[ON_AXIS].e[2] == 0 and nonzero.min() >= 4       # every term is there on most of the seven chains


def test_two_calls_give_the_same_bits_and_a_chain_does_not_depend_on_its_batch(gpu, batch):
    chains, orders, poses = batch["chains"], batch["orders"], batch["poses"]
    first = _energy(chains, orders, poses)
    again = _energy(chains, orders, poses)
    assert first[0] == 0 and again[0] == 0, _err()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first[1:], again[1:]))
    for b in (0, 4, 5, 6):
        n = len(chains[b])
        rc, e, c, w, g = _energy(chains[b: b + 1], orders[b: b + 1], poses[b: b + 1])
        assert rc == 0, _err()
        assert np.array_equal(_f64bits(e[0]), _f64bits(first[1][b])) and c[0] == first[2][b] and np.array_equal(_f64bits(w[0]), _f64bits(first[3][b]))
        assert np.array_equal(_f64bits(g[0]), _f64bits(first[4][b, :n]))
    rc, e, c, w, g = _energy(chains, orders, poses, wrench=False, grad=False)                # the optional outputs
    assert rc == 0 and np.array_equal(_f64bits(e), _f64bits(first[1])) and np.array_equal(c, first[2])


def test_a_contact_limit_below_the_clash_limit(gpu, batch):
    """d_on = 1, d_off = 2, below every clash limit (2.10 to 2.29 A): the squared-distance test of a CA pair is then the clash
    limit's, and the statement's values agree with the reference as at the default limits.  The batch's poses; no CA pair lies
    within 1e-6 A of this d_on either (asserted)."""
    chains, orders, poses = batch["chains"], batch["orders"], batch["poses"]
    narrow = sr.Params(r_max=0.5, d_on=1.0, d_off=2.0)
    ref = [sr.energy(c, int(o), p, narrow) for c, o, p in zip(chains, orders, poses)]
    assert min(r.min_gap for r in ref) >= 1e-6
    rc, e, c, w, g = _energy(chains, orders, poses, prm=_sym_params(narrow))
    assert rc == 0, _err()
    for b, (x, r) in enumerate(zip(chains, ref)):
        n = len(x)
        scale = max(np.abs(r.dcoords).max(), 1e-300)
        assert (np.abs(e[b] - r.e) <= 1e-9 * np.abs(r.e)).all() and c[b] == r.contacts and np.abs(g[b, :n] - r.dcoords).max() <= 1e-9 * scale, b
        assert np.linalg.norm(w[b] - r.wrench) <= 1e-9 * max(np.linalg.norm(r.wrench), 1e-300)
    rc, po, e2, c2, trace, acc, _ = _dock(chains, orders, poses, 10, prm=_sym_params(narrow))
    assert rc == 0 and np.isfinite(po).all() and np.isfinite(trace).all() and (np.diff(trace, axis=0) <= 0).all()
    print(f"d_off = 2: contact energies {e[:, 1].tolist()}, contacts {c.tolist()}; ten steps lower E by {np.round(trace[0] - trace[-1], 3).tolist()}")


# ---------------------------------------------------------------------------------- 2. the docking descent
def test_dock_is_its_own_chain_of_single_steps_and_never_raises_the_energy(gpu, batch):
    """N = 20 against 20 chained calls with n_iter = 1, bit for bit; the trace never rises; energy_out is fd_symmetry_energy's at
    pose_out bit for bit; the first trial agrees with the reference's to 1e-12 (later decisions may flip under rounding and are
    not compared); a chain of order 1 keeps its pose."""
    chains, orders, poses = batch["chains"], batch["orders"], batch["poses"]
    B = len(chains)
    h0 = np.full(B, PRM.step0)
    rc, po, e, c, trace, acc, h = _dock(chains, orders, poses, 20, step=h0)
    assert rc == 0, _err()
    assert (np.diff(trace, axis=0) <= 0).all() and (acc >= 0).all() and (acc <= 20).all()
    assert np.array_equal(trace[-1], (e[:, 0] + e[:, 1]) + e[:, 2])
    rc, e2, c2, _, _ = _energy(chains, orders, po)
    assert rc == 0 and np.array_equal(_f64bits(e2), _f64bits(e)) and np.array_equal(c2, c)
    assert np.array_equal(_f64bits(po[2]), _f64bits(poses[2])) and acc[2] == 0 and h[2] == h0[2]   # order 1: nothing to descend
    cur, step, total = poses, h0, np.zeros(B, dtype=np.int64)
    for it in range(20):
        rc, cur, e1, c1, t1, a1, step = _dock(chains, orders, cur, 1, step=step)
        assert rc == 0, _err()
        total += a1
        assert np.array_equal(_f64bits(t1[1]), _f64bits(trace[it + 1]))
        if it == 0:
            took = 0
            for b in range(B):
                if orders[b] >= 2 and a1[b] == 1:
                    want = sr.trial(poses[b], batch["ref"][b].wrench, PRM.step0, PRM)
                    assert np.abs(cur[b] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), b
                    took += 1
                elif a1[b] == 0:
                    assert np.array_equal(_f64bits(cur[b]), _f64bits(poses[b]))
            assert took >= 4
    assert np.array_equal(_f64bits(cur), _f64bits(po)) and np.array_equal(_f64bits(step), _f64bits(h)) and np.array_equal(total, acc)
    assert np.array_equal(_f64bits(e1), _f64bits(e)) and np.array_equal(c1, c)
    Q = po[:, :9].reshape(B, 3, 3)
    assert np.abs(Q @ Q.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    fell = trace[0] - trace[-1]
    print(f"E falls by {np.round(fell, 4).tolist()} in 20 steps, accepted {acc.tolist()}, contacts {c.tolist()}")
    assert (fell[orders >= 2] > 0).all() and fell[2] == 0
    rc, po0, e0, c0, t0, a0, _ = _dock(chains, orders, poses, 0)                              # n_iter = 0: the input and its energy; no step_io
    assert rc == 0 and np.array_equal(_f64bits(po0), _f64bits(poses)) and np.array_equal(_f64bits(t0[0]), _f64bits(trace[0])) and not a0.any()


def test_dock_cyclic_brings_the_reference_chains_into_contact(gpu):
    """structures.dock_cyclic on tests/test_symmetry.py's chains, orders 2 and 3 as one batch, default parameters, 100 iterations
    from structures.start_pose: that test's gates on the device -- the fall of E at least half the reference's smallest, the hard
    clashes between copies at most double its largest -- and every chain ends in contact."""
    import relax_reference as xr
    from test_symmetry import DOCK_CLASHES_WORST, DOCK_FALL_WORST
    chains = [xr.nerf_scan(ang, xr.IDX3) for ang in xr.device_chains()] * 2
    orders = [2] * 6 + [3] * 6
    res = structures.dock_cyclic(chains, orders, n_iter=100, return_trace=True)
    fell = res.trace[0] - res.trace[-1]
    clashes = [sr.hard_clashes_between(structures.cyclic_assembly(c, p, o)) for c, p, o in zip(chains, res.pose, orders)]
    print(f"E falls by {np.round(fell, 2).tolist()}, accepted {res.accepted.tolist()}, contacts {res.contacts.tolist()}, hard clashes {clashes}")
    assert (np.diff(res.trace, axis=0) <= 0).all() and (res.contacts > 0).all()
    assert fell.min() >= DOCK_FALL_WORST / 2 and max(clashes) <= 2 * DOCK_CLASHES_WORST
    e, c = structures.symmetry_energy(chains, orders, res.pose)
    assert np.array_equal(_f64bits(e), _f64bits(res.energy)) and np.array_equal(c, res.contacts)


# ---------------------------------------------------------------------------------- 3. the step hook against the statement
def _sg_step_sym(x, x0, known, fixed, lens, packed, tpl_packed, orders, pose_in, placed_in, prm, h, c, max_norm=1.0, s=0.0, z=None, seed=0, t=0,
                 seq_offset=0, offset=None, is_angle=None, clash=NO_CLASH):
    """fd_scaffold_guide_step_sym -> (rc, x_out, energy [B, 3], max_violation, gnorm, dfeats, tpl_rmsd, sym_energy, contacts, pose,
    placed, h); sentinels first."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    xs = arr(x)
    B, L, Fx = xs.shape
    ang = arr(np.asarray([True] * Fx if is_angle is None else is_angle, dtype=bool), np.uint8)
    out, e, mv, gn, rm = np.full_like(xs, SENTINEL), np.full((B, 3), SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL)
    G = np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    se, sc, sp, spl = np.full((B, 3), SENTINEL), np.full(B, -7, np.int32), np.full((B, 12), SENTINEL), np.full((B, 3 * L, 3), SENTINEL)
    hh = None if h is None else arr(h, np.float64).copy()
    gp = _params(Fx, offset, max_norm, clash)
    rc = _binding.load().fd_scaffold_guide_step_sym(0, P(xs), P(arr(x0)), P(arr(known)), P(arr(fixed, np.uint8)), P(arr(lens, np.int32)), B, L, Fx,
                                                    P(ang), C.byref(gp), *(P(a) for a in packed), *(P(a) for a in tpl_packed), P(arr(orders, np.int32)),
                                                    P(arr(pose_in, np.float64)), P(arr(placed_in, np.float64)), None if prm is None else C.byref(prm), P(hh),
                                                    C.c_float(c), C.c_float(s), P(arr(z)), C.c_uint64(seed), int(t), C.c_int64(seq_offset), P(out), P(e),
                                                    P(mv), P(gn), P(G), P(rm), P(se), P(sc), P(sp), P(spl))
    return rc, out, e, mv, gn, G, rm, se, sc, sp, spl, hh


def test_step_without_symmetry_is_the_template_step_bit_for_bit(gpu):
    """sym_order NULL (no sym_* argument is looked at) and all ones: every output fd_scaffold_guide_step_tpl shares, bit for bit."""
    x, x0, known, fixed, per, packed = _step_case(LENS, 6, 61)
    tpl_packed = _pack_tpl(_step_templates(LENS, 62))
    x0p = np.where(fixed.astype(bool), np.float32(np.nan), x0)
    z = np.random.default_rng(63).standard_normal(x.shape).astype(np.float32)
    kw = dict(s=0.3, z=z, offset=OFFSETS[6], is_angle=ANG, clash=CLASH)
    rc, *want = _sg_step_tpl(x, x0p, known, fixed, LENS, packed, tpl_packed, -0.2, **kw)
    assert rc == 0, _err()
    poses = np.tile(np.concatenate([np.eye(3).reshape(9), [3.0, 0.0, 0.0]]), (len(LENS), 1))
    for orders, prm, pose_in in ((None, None, None), (np.ones(len(LENS), np.int32), _sym_params(), poses)):
        rc, *got = _sg_step_sym(x, x0p, known, fixed, LENS, packed, tpl_packed, orders, pose_in, None, prm, None, -0.2, **kw)
        assert rc == 0, _err()
        assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(got[:6], want))
        se, sc, sp, spl = got[6:10]
        if orders is None:
            assert (se == SENTINEL).all() and (sc == -7).all() and (sp == SENTINEL).all()
        else:
            assert not se.any() and not sc.any() and np.array_equal(sp, poses)
        assert (spl == SENTINEL).all()


@pytest.mark.parametrize("anchored", [False, True])
def test_step_equals_the_statement_and_leaves_fixed_elements_alone(gpu, anchored):
    """The ragged batch with tests/test_scaffold_guide_gpu.py's masks, distances, clashes and a template, on fd_nerf_scan's own
    coordinates: x_out within 2e-6, the energies (the three of the chain, the three of the symmetry), norm and violation within
    1e-9 relative, contacts equal, the pose within 1e-9, placed_out == Q coords + t to 1e-12; fixed elements keep their bits.
    ``anchored``: with sym_placed_in (a jittered copy of the structure, placed at random), else the first visit's sym_pose_in.
    With pose_iters = 0 the pose is the fit (or sym_pose_in) itself."""
    x, x0, known, fixed, per, packed = _step_case(LENS, 6, 71)
    tpls = _step_templates(LENS, 72)
    L = max(LENS)
    ok, fx = _valid(LENS, L, 6), fixed.astype(bool)
    x0p = np.where(fx, np.float32(np.nan), x0)
    z = np.random.default_rng(73).standard_normal(x.shape).astype(np.float32)
    kn = np.nan_to_num(known)
    structure = [_scan_builder(gr.shift(sg.assemble(x0[b, :n], kn[b, :n], fx[b, :n]), OFFSETS[6], ANG), IDX[6]) for b, n in enumerate(LENS)]
    orders = np.array(ORDERS, np.int32)
    h_in = np.array([0.01, 0.02, 0.01, 0.005, 0.01, 0.03])
    for seed in range(8):     # (contact counts must not rest on rounding: as in the model-free batch)
        rng = np.random.default_rng(7400 + seed)
        pose_in = _poses_near_the_axis(structure, rng)
        placed_in = None
        if anchored:
            placed_in = [sr.place(c + 0.3 * rng.standard_normal(c.shape), p) for c, p in zip(structure, pose_in)]
            pose_in = np.array([sr.random_pose(rng, 9.0) for _ in LENS])            # (not read where a chain is fitted)
        kw = dict(s=0.3, z=z, offset=OFFSETS[6], is_angle=ANG, clash=CLASH)
        want = sr.step(np.where(ok, x, 0), x0, kn, fx, LENS, IDX[6], OFFSETS[6], ANG, per, tpls, orders, pose_in, placed_in, PRM, h_in, -0.2, 1.0,
                       s=0.3, z=z, clash=CLASH, build=_scan_builder)
        gaps = [sr.energy(c, int(o), p, PRM).min_gap for c, o, p in zip(structure, orders, want[7])]
        if min(gaps) >= 1e-6:
            break
    else:
        pytest.fail("no seed below 8 keeps every CA pair 1e-6 A from d_on")
    padded_in = None if placed_in is None else _padded(placed_in)[0]
    rc, got, e, mv, gn, G, rm, se, sc, sp, spl, h = _sg_step_sym(x, x0p, known, fixed, LENS, packed, _pack_tpl(tpls), orders, pose_in, padded_in,
                                                                 _sym_params(), h_in, -0.2, **kw)
    assert rc == 0, _err()
    wx, we, wmv, wn, wrm, wse, wsc, wsp, wpl, wh = want
    dist = ref_sampling.circ_dist(got, wx)[ok]
    rel = lambda a, b: np.abs(a - b) <= 1e-9 * np.abs(b)   # noqa: E731
    print(f"anchored={anchored}: max distance {dist.max():.2e}; symmetry energies {np.round(se, 4).tolist()}; contacts {sc.tolist()}; h {h.tolist()}")
    assert dist.max() <= 2e-6
    assert rel(e, we).all() and rel(mv, wmv).all() and rel(gn, wn).all() and rel(rm, wrm).all() and rel(se, wse).all()
    assert np.array_equal(sc, wsc) and np.abs(sp - wsp).max() <= 1e-9 * max(1.0, np.abs(wsp).max())
    sym = orders >= 2
    assert np.array_equal(h, wh) and not se[~sym].any() and (se[sym, 1] < 0).all()                 # (order 1: h as given)
    for b, n in enumerate(LENS):
        assert np.abs(spl[b, : 3 * n] - sr.place(structure[b], sp[b])).max() <= 1e-12 * max(1.0, np.abs(spl[b, : 3 * n]).max()), b
        assert (spl[b, 3 * n:] == SENTINEL).all()
    assert np.array_equal(_bits(got)[fx], _bits(x)[fx]) and (G[fx] == 0).all() and (got[~ok] == SENTINEL).all()
    # the symmetry moved the step: the same call without it ends elsewhere
    rc, plain, *_ = _sg_step_tpl(x, x0p, known, fixed, LENS, packed, _pack_tpl(tpls), -0.2, **kw)
    assert rc == 0 and np.abs(got - plain)[ok & ~fx].max() > 1e-5
    # pose_iters = 0: the pose is the fit, or the given one bit for bit
    rc, *rest = _sg_step_sym(x, x0p, known, fixed, LENS, packed, _pack_tpl(tpls), orders, pose_in, padded_in, _sym_params(pose_iters=0), h_in, -0.2, **kw)
    assert rc == 0, _err()
    sp0, h0 = rest[8], rest[10]
    assert np.array_equal(h0, h_in)
    for b in range(len(LENS)):
        if anchored and sym[b]:
            fit, _ = sr.fit_pose(structure[b], placed_in[b])
            assert np.abs(sp0[b] - fit).max() <= 1e-9 * max(1.0, np.abs(fit).max()), b
        else:
            assert np.array_equal(_f64bits(sp0[b]), _f64bits(pose_in[b])), b


# ---------------------------------------------------------------------------------- 4. the run
RUN_ORDERS = np.array([3, 2, 1, 4], np.int32)


def _run_poses():
    return structures.start_pose(None, RUN_ORDERS, radius=[4.0, 3.0, 0.0, 5.0], lengths=LENS4)


def _guided_inpaint_sym(h, x0, lens, visits, coef, noise, known, fixed, kcoef, known_noise, seed, guide, packed, tpl_packed, orders, pose0, prm,
                        offset=OFFSET, max_norm=1.0, clash=NO_CLASH, out=True, energy=True, sym_out=(True, True, True)):
    """fd_sample_guided_inpaint_sym -> (rc, out, energy [B, 3], max_violation, tpl_rmsd, sym_energy, contacts, pose); sentinels first."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    B = len(LENS4)
    vs = arr(visits, np.int32)
    gp = _params(6, offset, max_norm, clash)
    buf = np.full((B, L_R, 6), SENTINEL, dtype=np.float32) if out else None
    e, mv, rm = (np.full((B, 3), SENTINEL) if energy else None), np.full(B, SENTINEL), np.full(B, SENTINEL)
    se, sc, sp = (np.full((B, 3), SENTINEL) if sym_out[0] else None), (np.full(B, -7, np.int32) if sym_out[1] else None), (np.full((B, 12), SENTINEL) if sym_out[2] else None)
    rc = _binding.load().fd_sample_guided_inpaint_sym(h, P(arr(x0)), P(arr(lens, np.int32)), B, L_R, P(vs), len(vs), P(arr(coef)), P(arr(noise)),
                                                      P(arr(known)), P(arr(fixed, np.uint8)), P(arr(kcoef)), P(arr(known_noise)), C.c_uint64(seed),
                                                      C.c_int64(0), P(arr(guide)), C.byref(gp), *(P(a) for a in packed), *(P(a) for a in tpl_packed),
                                                      P(arr(orders, np.int32)), P(arr(pose0, np.float64)), None if prm is None else C.byref(prm), P(buf),
                                                      P(e), P(mv), P(rm), P(se), P(sc), P(sp))
    return rc, buf, e, mv, rm, se, sc, sp


def _chain_of_hooks(h, x0, visits, coef, guide, noise, known_noise, known, fixed, kcoef, packed, tpl_packed, seed, clash, prm):
    """Per visit: fd_p_sample_step_coef_inpaint for x, fd_p_sample_step_coef_x0 for x0, then fd_scaffold_guide_step_sym with the
    placed atoms, the pose and h carried; behind the last visit the statement on the final state.  Returns (state, the final
    statement's outputs)."""
    B = len(LENS4)
    kn = np.nan_to_num(known)
    levels = sir.landing_levels(visits)
    draw = lambda i, q: known_noise[i] if known_noise is not None else _device_draws(h, seed, ipr.TAG | q, B, L_R)   # noqa: E731
    state = ipr.replace(x0, kn, fixed, int(visits[0]) + 1, kcoef, draw(0, int(visits[0]) + 1), ANG)
    pose, placed, step = _run_poses(), None, np.full(B, prm.step0)
    for i, (t, q) in enumerate(zip(visits, levels)):
        a, b, s, u, v = coef[:, i]
        rc, _, x = _step_coef_inpaint(h, state, t, LENS4, a, b, 0.0, None, q, kn, fixed, kcoef, None if q == 0 else draw(i + 1, q))
        assert rc == 0, _err()
        rc, _, pred, _ = _step_x0(h, state, t, LENS4, a, b, 0.0, u, v, None)
        assert rc == 0, _err()
        rc, state, _, _, _, _, _, _, _, pose, placed_out, step = _sg_step_sym(x, pred, known, fixed, LENS4, packed, tpl_packed, RUN_ORDERS, pose, placed, prm,
                                                                            step, guide[i], s=s, z=None if noise is None else noise[i], seed=seed,
                                                                            t=int(t), offset=OFFSET, clash=clash)
        assert rc == 0, _err()
        placed = np.where(placed_out == SENTINEL, 0.0, placed_out)
    final = _sg_step_sym(state, state, known, fixed, LENS4, packed, tpl_packed, RUN_ORDERS, pose, placed, prm, step, 0.0, offset=OFFSET, clash=clash)
    assert final[0] == 0, _err()
    return state, final


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 20, K = 5, B = 4, L = 16, eta = 1, orders 3, 2, 1, 4: with clashes, a template and explicit draws, without either and
    with Philox; eager launches and packed rows give the same bits below the lengths; the final state's energies, contacts and
    pose are the hook's on the final state with the carried placement and h."""
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_S)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    ok = _valid(LENS4, L_R, 6)
    visits, coef, guide, x0, noise, known_noise, known, fixed, packed = _run_case(betas, 0)
    fx = fixed.astype(bool)
    prm = _sym_params(sr.Params(pose_iters=2))
    for clash, zs, kz, seed, tpl_packed in ((CLASH, noise, known_noise, 0, _pack_tpl(_run_templates(300))), (NO_CLASH, None, None, 977, NO_TPL)):
        rc, out, e, mv, rm, se, sc, sp = _guided_inpaint_sym(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, tpl_packed,
                                                             RUN_ORDERS, _run_poses(), prm, clash=clash)
        assert rc == 0, _err()
        want, final = _chain_of_hooks(h, x0, visits, coef, guide, zs, kz, known, fixed, kcoef, packed, tpl_packed, seed, clash, prm)
        assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), clash
        assert np.array_equal(_bits(out)[fx], _bits(known)[fx])
        _, _, e_h, mv_h, _, _, rm_h, se_h, sc_h, sp_h, _, _ = final
        assert np.array_equal(_f64bits(e), _f64bits(e_h)) and np.array_equal(_f64bits(mv), _f64bits(mv_h)) and np.array_equal(_f64bits(rm), _f64bits(rm_h))
        assert np.array_equal(_f64bits(se), _f64bits(se_h)) and np.array_equal(sc, sc_h) and np.array_equal(_f64bits(sp), _f64bits(sp_h))
        assert not se[2].any() and sc[2] == 0 and (se[[0, 1, 3], 1] < 0).all()
        print(f"{precision} w_clash={clash.w}: symmetry energies {np.round(se, 3).tolist()}, contacts {sc.tolist()}")
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            got2 = _guided_inpaint_sym(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, tpl_packed, RUN_ORDERS, _run_poses(),
                                       prm, clash=clash)
            pm.set_option(option, int(option == "use_graph"))
            assert got2[0] == 0 and np.array_equal(_bits(got2[1])[ok], _bits(out)[ok]), option
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got2[2:], (e, mv, rm, se, sc, sp))), option
    # the symmetry steers: the same run without it ends elsewhere
    rc, plain, *_ = _guided_inpaint_tpl(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 977, guide, packed, NO_TPL)
    assert rc == 0 and not np.array_equal(plain[ok], out[ok])


def test_the_run_against_its_neighbours(gpu):
    """Orders all 1, or no orders: fd_sample_guided_inpaint_tpl's outputs bit for bit.  Bad calls leave the outputs alone.  A plain
    strided run and a template run give, behind the new run on the same handle, the bits they give first on a fresh handle, and
    the new run its own behind them."""
    betas = beta_schedules.cosine_beta_schedule(T_S)
    kcoef = sampling.inpaint_levels(betas)
    visits, coef, guide, x0, _, _, known, fixed, packed = _run_case(betas, 5)
    tpl_packed = _pack_tpl(_run_templates(301))
    prm = _sym_params()
    same = lambda xs, ys: all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(xs, ys))   # noqa: E731

    def others(h):
        a = _strided(h, x0, LENS4, visits, coef[:3], 11, 0)
        b = _guided_inpaint_tpl(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 12, guide, packed, tpl_packed, clash=CLASH)
        assert a[0] == 0 and b[0] == 0, _err()
        return (a[1],) + tuple(b[1:])

    def new(h, seed=14, orders=RUN_ORDERS, prm=prm, pose0=None):
        got = _guided_inpaint_sym(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, seed, guide, packed, tpl_packed, orders,
                                  _run_poses() if pose0 is None else pose0, prm, clash=CLASH)
        assert got[0] == 0, _err()
        return got[1:]

    _, _, pm1 = _pair(precision="f16x3", **MODEL_D)
    h1 = pm1.prepare(betas)
    fresh_others = others(h1)
    after_others = new(h1)
    _, _, pm2 = _pair(precision="f16x3", **MODEL_D)
    h2 = pm2.prepare(betas)
    fresh_new = new(h2)
    assert same(fresh_new, after_others)
    assert same(others(h2), fresh_others)
    assert same(new(h2), fresh_new) and same(others(h1), fresh_others)
    # no symmetry: the template run, bit for bit
    rc, *tpl_run = _guided_inpaint_tpl(h2, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 14, guide, packed, tpl_packed, clash=CLASH)
    assert rc == 0, _err()
    out, e, mv, rm, se, sc, sp = new(h2, orders=np.ones(4, np.int32))
    assert same((out, e, mv, rm), tpl_run) and not se.any() and not sc.any() and np.array_equal(sp, _run_poses())
    out, e, mv, rm, se, sc, sp = new(h2, orders=None, prm=None)
    assert same((out, e, mv, rm), tpl_run) and (se == SENTINEL).all() and (sc == -7).all() and (sp == SENTINEL).all()
    assert not np.array_equal(out, fresh_new[0])
    # bad calls
    nan_pose = _run_poses()
    nan_pose[3, 10] = np.nan
    bad = [(dict(orders=[3, 2, 0, 4]), b"order[2]=0"), (dict(orders=[3, 13, 1, 4]), b"order[1]=13"), (dict(pose0=nan_pose), b"pose[3][10]"),
           (dict(prm=_sym_params(w_contact=-1.0)), b"w_contact=-1"), (dict(prm=_sym_params(d_off=8.0)), b"d_on=8"), (dict(prm=_sym_params(lever=0.0)), b"lever=0"),
           (dict(prm=_sym_params(shrink=1.5)), b"shrink=1.5"), (dict(prm=_sym_params(pose_iters=-2)), b"pose_iters=-2"), (dict(prm=None), b"symmetry arrays"),
           (dict(pose0=False), b"symmetry arrays"), (dict(sym_out=(False, True, True)), b"symmetry arrays"), (dict(sym_out=(True, False, True)), b"symmetry arrays"),
           (dict(sym_out=(True, True, False)), b"symmetry arrays"), (dict(out=False), b"null"), (dict(energy=False), b"null"),
           (dict(lens=[16, 13, 0, 14]), b"lens[2]=0"), (dict(clash=sg.Clash(0.63, 0.15, -1.0)), b"w_clash=-1"), (dict(max_norm=0.0), b"max_norm=0")]
    for kw, word in bad:
        a = dict(lens=LENS4, orders=RUN_ORDERS, pose0=_run_poses(), prm=prm, out=True, energy=True, sym_out=(True, True, True), clash=CLASH, max_norm=1.0)
        a.update(kw)
        rc, *outs = _guided_inpaint_sym(h2, x0, a["lens"], visits, coef, None, known, fixed, kcoef, None, 5, guide, packed, tpl_packed, a["orders"],
                                        None if a["pose0"] is False else a["pose0"], a["prm"], max_norm=a["max_norm"], clash=a["clash"], out=a["out"],
                                        energy=a["energy"], sym_out=a["sym_out"])
        assert rc == -1 and word in _err(), (word, rc, _err())
        assert all(o is None or (o == (-7 if o.dtype == np.int32 else SENTINEL)).all() for o in outs), word
    assert same(new(h2), fresh_new)


def test_the_run_with_a_contact_limit_below_the_clash_limit_is_its_chain_of_hooks(gpu):
    """d_on = 1, d_off = 2: the run ends finite and is bit for bit the chain of its hooks, as at the default limits."""
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_S)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    ok = _valid(LENS4, L_R, 6)
    visits, coef, guide, x0, _, _, known, fixed, packed = _run_case(betas, 3)
    prm = _sym_params(sr.Params(d_on=1.0, d_off=2.0))
    rc, out, e, mv, rm, se, sc, sp = _guided_inpaint_sym(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 31, guide, packed, NO_TPL, RUN_ORDERS,
                                                         _run_poses(), prm, clash=CLASH)
    assert rc == 0, _err()
    assert np.isfinite(out[ok]).all() and np.isfinite(e).all() and np.isfinite(se).all() and np.isfinite(sp).all()
    want, final = _chain_of_hooks(h, x0, visits, coef, guide, None, None, known, fixed, kcoef, packed, NO_TPL, 31, CLASH, prm)
    assert np.array_equal(_bits(out)[ok], _bits(want)[ok])
    assert np.array_equal(_f64bits(se), _f64bits(final[7])) and np.array_equal(sc, final[8]) and np.array_equal(_f64bits(sp), _f64bits(final[9]))


# ---------------------------------------------------------------------------------- 5. Python end to end
def _recount(backbone, pose, order, d_on=8.0):
    """Ordered (CA, copy, CA) triples below d_on, from the explicit assembly."""
    asm = structures.cyclic_assembly(backbone, pose, order)
    ca = asm[:, 1::3]
    return sum(int((np.sqrt(((ca[0][:, None] - ca[k][None]) ** 2).sum(-1)) < d_on).sum()) for k in range(1, order))


def test_sample_symmetric_reports_the_contacts_of_its_assemblies(gpu):
    _, _, pm = _pair(seed=11, precision="f16x3")
    inner = datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=OFFSET)
    ds = datasets.NoisedAnglesDataset(inner, timesteps=20, beta_schedule="cosine")
    kw = dict(order=[3, 2, 4], num_steps=6, dock_iters=30, batch_size=2)
    torch.manual_seed(3)
    res = sampling.sample_symmetric(pm, ds, [30, 34, 22], **kw)
    assert [s.shape for s in res.angles] == [(30, 6), (34, 6), (22, 6)] and all(np.isfinite(s).all() for s in res.angles)
    assert res.pose.shape == (3, 12) and np.isfinite(res.pose).all() and res.order.tolist() == [3, 2, 4]
    scan = nerf.build_backbones(res.angles, NAMES, center_coords=False, method="scan")
    counted = [_recount(c, p, o) for c, p, o in zip(scan, res.pose, res.order)]
    print(f"contacts {res.contacts.tolist()}, recounted {counted}; energies {np.round(res.energy, 3).tolist()}; the run's own contacts {res.info['symmetry_contacts'].tolist()}")
    assert res.contacts.tolist() == counted
    e, c = structures.symmetry_energy(scan, res.order, res.pose)
    assert np.array_equal(_f64bits(e), _f64bits(res.energy)) and np.array_equal(c, res.contacts)
    start, _ = structures.symmetry_energy(scan, res.order, res.info["symmetry_pose"])
    assert ((res.energy[:, 0] + res.energy[:, 1]) + res.energy[:, 2] <= (start[:, 0] + start[:, 1]) + start[:, 2]).all()   # the dock never raises it
    Q = res.pose[:, :9].reshape(3, 3, 3)
    assert np.abs(Q @ Q.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    torch.manual_seed(3)
    again = sampling.sample_symmetric(pm, ds, [30, 34, 22], **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again.angles, res.angles)) and np.array_equal(_f64bits(again.pose), _f64bits(res.pose))


def test_script_writes_one_chain_per_copy(gpu, tmp_path):
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_symmetric.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "36", "--order", "4",
                        "--num_steps", "5", "--eta", "1.0", "--dock_iters", "10", "--seed", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["assembly_pdb", "model_snapshot", "sampled_angles", "symmetry.json"]
    names = [f"generated_{i}.pdb" for i in range(2)]
    assert sorted(os.listdir(os.path.join(out, "assembly_pdb"))) == names
    assert sorted(os.listdir(os.path.join(out, "sampled_angles"))) == [f"generated_{i}.csv.gz" for i in range(2)]
    with open(os.path.join(out, "symmetry.json")) as fh:
        report = json.load(fh)
    assert sorted(report["samples"]) == names and report["energy_terms"] == ["clash", "contact", "radial"] and report["settings"]["order"] == 4
    for name in names:
        entry = report["samples"][name]
        assert len(entry["pose"]) == 12 and len(entry["energy"]) == 3 and np.isfinite(entry["pose"] + entry["energy"]).all() and entry["contacts"] >= 0
        fname = os.path.join(out, "assembly_pdb", name)
        chains = [angles_and_coords.read_pdb_backbone(fname, chain=ch) for ch in "ABCD"]
        assert all(c.shape == (108, 3) for c in chains) and angles_and_coords.read_pdb_backbone(fname, chain="E").size == 0
        turn = sr.rot_z(1, 4)
        assert np.abs(chains[0] @ turn.T - chains[1]).max() <= 2e-3                       # copies, to the PDB's three decimals
