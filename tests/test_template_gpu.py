"""Superposition restraints on the device (fd_template_energy, fd_scaffold_guide_step_tpl, fd_sample_guided_inpaint_tpl,
structures.template_energy, sampling.scaffold_segments(placement=...), bin/sample_restrained.py --placement) against
the numpy float64 statement of tests/template_reference.py and against the existing entries: bits are compared with ==,
everything else with the bound stated at its test."""
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
import template_reference as tr
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_model, ref_sampling
from test_gpu_parity import PRECISIONS, _pair, _write_model_dir
from test_guide import IDX, random_features
from test_guide_gpu import _f64bits, _guided, _pack
from test_inpaint_gpu import _device_draws
from test_repeat_gpu import LENS4, L_R
from test_scaffold_guide_gpu import (CLASH, K_S, MIXED9, NO_CLASH, OFFSETS, RAGGED, T_S, _guided_inpaint, _params, _run_case, _scan_builder,
                                     _sg_step, _step_case, _valid)
from test_steer_gpu import MODEL_D, NAMES, OFFSET, _step_x0
from test_strided_gpu import ANG, SENTINEL, _bits, _strided
from test_strided_inpaint_gpu import _step_coef_inpaint, _strided_inpaint
from test_template import DESCENT_GATE, moved, template_descent_case

pytestmark = pytest.mark.gpu
P = _binding.ptr
GAP = 1e-3                       # the relative eigen-gap the gates below are derived for
BATCH = RAGGED + [86]            # 86 residues, all atoms: 258 entries, the first count with more than one entry per lane
KINDS = ("none", "one", "two", "collinear", "all", "scattered")


def _err():
    return _binding.load().fd_last_error()


def _pack_tpl(per_chain):
    """Per chain (atoms, xyz [n, 3], w) -> the packed arrays of include/fdmi.h."""
    offs = np.concatenate([[0], np.cumsum([len(t[0]) for t in per_chain])]).astype(np.int32)
    return (offs, np.ascontiguousarray(np.concatenate([np.asarray(t[0], dtype=np.int32) for t in per_chain]).astype(np.int32)),
            np.ascontiguousarray(np.concatenate([np.asarray(t[1], dtype=np.float64).reshape(-1, 3) for t in per_chain])),
            np.ascontiguousarray(np.concatenate([np.asarray(t[2], dtype=np.float64) for t in per_chain]).astype(np.float64)))


def _padded(chains):
    L = max(len(c) for c in chains) // 3
    out = np.zeros((len(chains), 3 * L, 3))
    for b, c in enumerate(chains):
        out[b, : len(c)] = c
    return out, [len(c) // 3 for c in chains]


def _tpl_energy(coords, lens, packed, transform=True, grad=True):
    """fd_template_energy -> (rc, energy, rmsd, transform [B, 12], dcoords); the outputs start at the sentinel."""
    B, L = coords.shape[0], coords.shape[1] // 3
    e, r = np.full(B, SENTINEL), np.full(B, SENTINEL)
    T = np.full((B, 12), SENTINEL) if transform else None
    g = np.full(coords.shape, SENTINEL) if grad else None
    rc = _binding.load().fd_template_energy(0, P(np.ascontiguousarray(coords)), P(np.ascontiguousarray(lens, dtype=np.int32)), B, L,
                                            *(P(a) for a in packed), P(e), P(r), P(T), P(g))
    return rc, e, r, T, g


def _template(kind, rng, xyz):
    """One chain's template of a kind; targets come from another random walk, rotated and 100 A from the origin."""
    n = len(xyz)
    other = moved(rng, np.cumsum(rng.standard_normal((n, 3)) * 1.5, axis=0))
    if kind == "none":
        return tr.NO_TEMPLATE
    if kind in ("one", "two"):
        atoms = np.sort(rng.choice(n, size=1 if kind == "one" else 2, replace=False))
        return atoms, other[atoms], rng.uniform(0.5, 2.0, len(atoms))
    if kind == "collinear":
        atoms = np.sort(rng.choice(n, size=3, replace=False))
        d = rng.standard_normal(3)
        return atoms, other[0] + np.outer([0.0, 1.3, 4.1], d / np.linalg.norm(d)), rng.uniform(0.5, 2.0, 3)
    if kind == "all":
        return np.arange(n), other, np.ones(n)
    atoms = np.sort(rng.choice(n, size=max(3, n // 2), replace=False))
    return atoms, other[atoms], rng.uniform(0.5, 2.0, len(atoms))


def _check_against_reference(coords, lens, per, unique):
    """The gates of DESIGN.md 6z for one batch; returns the measured maxima relative to their gates' scales."""
    rc, e, rmsd, T, g = _tpl_energy(coords, lens, _pack_tpl(per))
    assert rc == 0, _err()
    worst = dict(gradient=0.0, energy=0.0, rotation=0.0, orthonormal=0.0)
    for b, n in enumerate(lens):
        fit = tr.template_energy(coords[b, : 3 * n], per[b])
        R, t = T[b, :9].reshape(3, 3), T[b, 9:]
        assert (g[b, 3 * n:] == 0).all() and (g[b][np.setdiff1d(np.arange(g.shape[1]), per[b][0])] == 0).all()   # written, atoms not named: 0
        ortho = max(np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1))
        assert ortho <= 1e-12, (b, ortho)
        worst["orthonormal"] = max(worst["orthonormal"], ortho)
        if not len(per[b][0]):
            assert e[b] == 0 and rmsd[b] == 0 and np.array_equal(R, np.eye(3)) and (t == 0).all()
            continue
        w = np.asarray(per[b][2], dtype=np.float64)
        W, extent = w.sum(), fit.extent
        if len(w) == 1:   # one entry: nothing to fit; what is left is the rounding of (w p) / w - p, an ulp of 100 A (no extent to scale by)
            assert e[b] <= 1e-20 and rmsd[b] <= 1e-10 and np.abs(g[b]).max() <= 1e-10
            continue
        dg = np.abs(g[b, : 3 * n] - fit.grad).max() / (2 * w.max() * extent)
        de = abs(e[b] - fit.energy) / (W * extent * extent)
        assert dg <= 1e-10 and de <= 1e-10, (b, dg, de)
        assert abs(rmsd[b] - np.sqrt(e[b] / W)) <= 1e-14 * rmsd[b]
        worst["gradient"], worst["energy"] = max(worst["gradient"], dg), max(worst["energy"], de)
        if unique and len(per[b][0]) >= 3:
            assert fit.gap >= GAP, (b, fit.gap)
            cm = (w[:, None] * np.asarray(per[b][1]).reshape(-1, 3)).sum(0) / W
            dr = np.abs(R - fit.R).max()
            assert dr <= 1e-10 and np.abs(t - fit.t).max() <= 1e-10 * (1 + np.linalg.norm(cm)), (b, dr)
            worst["rotation"] = max(worst["rotation"], dr)
    return worst


# ---------------------------------------------------------------------------------- 1. the statement on the device
@pytest.mark.parametrize("kind", KINDS)
def test_template_energy_equals_the_statement(gpu, kind):
    """Ragged lengths 1, 2, 3, 7, 12, 12 and 86, targets 100 A from the origin (a covariance that is not centred would lose
    nine digits there).  Each gradient entry within 1e-10 x 2 max(w) x extent of the reference and E within 1e-10 x W x
    extent^2, extent the largest distance of a named atom from cp: the rotation error is about eps |H| / gap, the reference's
    relative gap is asserted >= 1e-3 where R is unique, so the error is <= 1e-13 of the extent and the gates leave three orders.
    Where R is not unique (one or two entries, collinear targets) every optimal R gives the same residuals and the same gates
    hold; the transform is then only asked to be a proper rotation.  Measured: DESIGN.md 6z."""
    rng = np.random.default_rng(700 + KINDS.index(kind))
    chains = [np.cumsum(rng.standard_normal((3 * n, 3)) * 1.5, axis=0) for n in BATCH]
    coords, lens = _padded(chains)
    per = [_template(kind, rng, c) for c in chains]
    worst = _check_against_reference(coords, lens, per, unique=kind in ("all", "scattered"))
    print(f"{kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_template_energy_on_the_longest_chain(gpu):
    """2048 residues, all 6144 atoms named: 24 entries per lane.  The same gates."""
    rng = np.random.default_rng(720)
    chain = np.cumsum(rng.standard_normal((6144, 3)) * 1.5, axis=0)
    coords, lens = _padded([chain])
    worst = _check_against_reference(coords, lens, [_template("all", rng, chain)], unique=True)
    print("2048 residues: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("n", [7, 24, 40])
def test_mirror_and_copy_on_the_device(gpu, n):
    """tests/test_template.py's copy and mirror statements through structures.template_energy: a rotated and shifted copy fits
    at <= 1e-12 A with a gradient <= 1e-12; the mirror image of the backbone keeps fd_restraint_energy's all-pairs energy to
    the bit, fits the structure's all-atom template at >= 1 A, and fits with mirror=True at <= 1e-12."""
    rng = np.random.default_rng(n)
    xyz = gr.build_ref(random_features(rng, n, 6), IDX[6])
    flipped = xyz * np.array([1.0, 1.0, -1.0])
    copy = structures.Template(np.arange(3 * n), moved(rng, xyz), rng.uniform(0.5, 2.0, 3 * n))
    e, rmsd, grad, (R, t) = structures.template_energy([xyz], copy, return_gradient=True, return_transform=True)
    assert rmsd[0] <= 1e-12 and np.abs(grad[0]).max() <= 1e-12 and np.abs(copy.xyz @ R[0].T + t[0] - xyz).max() <= 1e-11
    i, j = np.triu_indices(3 * n, 1)
    rst = structures.Restraints(i, j, np.linalg.norm(xyz[i] - xyz[j], axis=1) + 0.5, 0.0, 1.0)
    e_rst, _ = structures.restraint_energy([xyz, flipped], rst)
    own = structures.Template(np.arange(3 * n), xyz)
    _, rmsd = structures.template_energy([xyz, flipped], own)
    _, rmsd_mirror = structures.template_energy([xyz, flipped], own, mirror=True)
    print(f"len={n}: copy {rmsd[0]:.1e}; E_rst {e_rst.tolist()}; mirror image {rmsd[1]:.2f} A, against the mirrored template {rmsd_mirror[1]:.1e}")
    assert e_rst[0] > 0 and e_rst[0] == e_rst[1]
    assert rmsd[0] <= 1e-12 and rmsd[1] >= 1.0 and rmsd_mirror[1] <= 1e-12 and abs(rmsd_mirror[0] - rmsd[1]) <= 1e-9


def test_two_calls_give_the_same_bits_and_a_chain_does_not_depend_on_its_batch(gpu):
    rng = np.random.default_rng(730)
    chains = [np.cumsum(rng.standard_normal((3 * n, 3)) * 1.5, axis=0) for n in BATCH]
    coords, lens = _padded(chains)
    per = [_template("scattered" if b % 2 else "all", rng, c) for b, c in enumerate(chains)]
    first, again = _tpl_energy(coords, lens, _pack_tpl(per)), _tpl_energy(coords, lens, _pack_tpl(per))
    assert first[0] == 0 and again[0] == 0, _err()
    for a, b in zip(first[1:], again[1:]):
        assert np.array_equal(_f64bits(a), _f64bits(b))
    for b in (3, 6):
        n = lens[b]
        rc, e, r, T, g = _tpl_energy(coords[b: b + 1, : 3 * n], [n], _pack_tpl([per[b]]))
        assert rc == 0, _err()
        assert e[0] == first[1][b] and r[0] == first[2][b] and np.array_equal(_f64bits(T[0]), _f64bits(first[3][b]))
        assert np.array_equal(_f64bits(g[0]), _f64bits(first[4][b, : 3 * n]))


# ---------------------------------------------------------------------------------- 2. the step hook against the statement
def _sg_step_tpl(x, x0, known, fixed, lens, packed, tpl_packed, c, max_norm=1.0, s=0.0, z=None, seed=0, t=0, seq_offset=0, offset=None,
                 is_angle=None, clash=NO_CLASH):
    """fd_scaffold_guide_step_tpl -> (rc, x_out, energy [B, 3], max_violation, gnorm, dfeats, tpl_rmsd); sentinels first."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    xs = arr(x)
    B, L, Fx = xs.shape
    ang = arr(np.asarray([True] * Fx if is_angle is None else is_angle, dtype=bool), np.uint8)
    out, e, mv, gn, rm = np.full_like(xs, SENTINEL), np.full((B, 3), SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL)
    G = np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    prm = _params(Fx, offset, max_norm, clash)
    rc = _binding.load().fd_scaffold_guide_step_tpl(0, P(xs), P(arr(x0)), P(arr(known)), P(arr(fixed, np.uint8)), P(arr(lens, np.int32)), B, L, Fx,
                                                    P(ang), C.byref(prm), *(P(a) for a in packed), *(P(a) for a in tpl_packed), C.c_float(c),
                                                    C.c_float(s), P(arr(z)), C.c_uint64(seed), int(t), C.c_int64(seq_offset), P(out), P(e), P(mv),
                                                    P(gn), P(G), P(rm))
    return rc, out, e, mv, gn, G, rm


NO_TPL = (None, None, None, None)


def _step_templates(lens, seed):
    """Scattered atoms with random weights per chain, targets another backbone's, moved and jittered by 0.5 A (the first
    residue of every backbone is the same rigid triangle: unjittered, a one-residue chain would fit exactly and its energy be
    rounding noise, which no relative gate can hold); the second chain has none."""
    rng = np.random.default_rng(seed)
    per = []
    for b, n in enumerate(lens):
        target = moved(rng, gr.build_ref(random_features(rng, n, 6), IDX[6]), 30.0) + 0.5 * rng.standard_normal((3 * n, 3))
        atoms = np.sort(rng.choice(3 * n, size=max(3, (3 * n) // 2), replace=False))
        per.append(tr.NO_TEMPLATE if b == 1 else (atoms, target[atoms], rng.uniform(0.5, 2.0, len(atoms))))
    return per


@pytest.mark.parametrize("lens,Fx", [(RAGGED, 6), (RAGGED, 9), ([86], 6), ([86], 9)])
def test_step_equals_the_statement_and_leaves_fixed_elements_alone(gpu, lens, Fx):
    """tests/test_scaffold_guide_gpu.py's masks (whole rows, one fixed element, scattered, nothing fixed; x0 NaN under fixed
    elements) and gates -- x_out 2e-6; energies, norm and violation 1e-9 relative -- with the template alone, with the
    distances, and with distances and clashes; the template energy also within 1e-10 x W x extent^2.  With all tpl_* NULL every
    shared output is fd_scaffold_guide_step's bit for bit."""
    x, x0, known, fixed, per, packed = _step_case(lens, Fx, 40 + Fx + len(lens))
    tpls = _step_templates(lens, 90 + Fx)
    L = max(lens)
    ok, fx = _valid(lens, L, Fx), fixed.astype(bool)
    x0_poisoned = np.where(fx, np.float32(np.nan), x0)
    z = np.random.default_rng(41).standard_normal(x.shape).astype(np.float32)
    is_angle = ANG if Fx == 6 else MIXED9
    none = [([], [], [], [], [])] * len(lens)
    for c, s, clash, rst in ((0.05, 0.0, NO_CLASH, none), (0.05, 0.3, NO_CLASH, per), (-0.2, 0.3, CLASH, per)):
        kw = dict(s=s, z=z, offset=OFFSETS[Fx], is_angle=is_angle, clash=clash)
        rc, got, e, mv, gn, G, rm = _sg_step_tpl(x, x0_poisoned, known, fixed, lens, _pack(rst), _pack_tpl(tpls), c, **kw)
        assert rc == 0, _err()
        want, we, wmv, wn, wrm, Gs = tr.step(np.where(ok, x, 0), x0, np.nan_to_num(known), fx, lens, IDX[Fx], OFFSETS[Fx], is_angle, rst, tpls, c, 1.0,
                                             s=s, z=z, clash=clash, build=_scan_builder)
        ang = np.asarray(is_angle, dtype=bool)
        dist = np.where(ang, ref_sampling.circ_dist(got, want), np.abs(got.astype(np.float64) - want))[ok]
        rel = lambda a, b: np.abs(a - b) <= 1e-9 * np.abs(b)   # noqa: E731
        print(f"F={Fx} lens={lens} c={c} s={s} w_clash={clash.w}: max distance {dist.max():.2e}; E_tpl {e[:, 2].tolist()}; rmsd {np.round(rm, 3).tolist()}")
        assert dist.max() <= 2e-6
        assert all(rel(e[:, k], we[:, k]).all() for k in range(3)) and rel(mv, wmv).all() and rel(gn, wn).all() and rel(rm, wrm).all()
        for b, n in enumerate(lens):
            if len(tpls[b][0]):
                ang_b = gr.shift(sg.assemble(x0[b, :n], np.nan_to_num(known)[b, :n], fx[b, :n]), OFFSETS[Fx], is_angle)
                fit = tr.template_energy(_scan_builder(ang_b, IDX[Fx]), tpls[b])
                assert abs(e[b, 2] - fit.energy) <= 1e-10 * np.sum(tpls[b][2]) * fit.extent ** 2 and e[b, 2] > 0
            else:
                assert e[b, 2] == 0 and rm[b] == 0
            scale = max(np.abs(Gs[b]).max(), 1e-300)
            assert np.abs(G[b, :n] - Gs[b]).max() <= 1e-9 * scale, b
        assert np.array_equal(_bits(got)[fx], _bits(x)[fx]) and (G[fx] == 0).all()
        assert (got[~ok] == SENTINEL).all() and (G[~ok] == SENTINEL).all()
        # no template: the entry it extends, bit for bit
        rc, got0, e0, mv0, gn0, G0, rm0 = _sg_step_tpl(x, x0_poisoned, known, fixed, lens, _pack(rst), NO_TPL, c, **kw)
        assert rc == 0, _err()
        rc, pg, pe, pmv, pgn, pG = _sg_step(x, x0_poisoned, known, fixed, lens, _pack(rst), c, **kw)
        assert rc == 0, _err()
        assert np.array_equal(_bits(got0), _bits(pg)) and np.array_equal(_f64bits(e0[:, :2]), _f64bits(pe)) and np.array_equal(_f64bits(G0), _f64bits(pG))
        assert np.array_equal(_f64bits(mv0), _f64bits(pmv)) and np.array_equal(_f64bits(gn0), _f64bits(pgn)) and (e0[:, 2] == 0).all() and (rm0 == 0).all()
        assert np.abs(got - got0)[ok & ~fx].max() > 1e-4                                    # ... and the template moved the step


def test_fifty_statements_on_the_device_lower_the_template_energy(gpu):
    """tests/test_template.py's descent case, seeds 0 .. 7 as one batch, on the device: the same gate, and the held elements
    keep their bits."""
    cases = [template_descent_case(seed) for seed in range(8)]
    x = np.concatenate([c[0] for c in cases])
    known, fixed = np.concatenate([c[1] for c in cases]), np.concatenate([c[2] for c in cases])
    tpl_packed, no_rst = _pack_tpl([c[3] for c in cases]), _pack([([], [], [], [], [])] * 8)
    start, first = x.copy(), None
    for _ in range(50):
        rc, x, e, _, _, _, rm = _sg_step_tpl(x, x, known, fixed, [24] * 8, no_rst, tpl_packed, 0.05)
        assert rc == 0, _err()
        first = (e[:, 2].copy(), rm.copy()) if first is None else first
    rc, _, e, _, _, _, rm = _sg_step_tpl(x, x, known, fixed, [24] * 8, no_rst, tpl_packed, 0.0)
    assert rc == 0, _err()
    print(f"E_tpl falls by {np.round(first[0] / e[:, 2], 2).tolist()}; CA rmsd {np.round(first[1], 2).tolist()} -> {np.round(rm, 2).tolist()}")
    assert np.array_equal(_bits(x)[fixed], _bits(start)[fixed]) and (first[0] / e[:, 2] >= DESCENT_GATE).all()


# ---------------------------------------------------------------------------------- 3. the run
def _guided_inpaint_tpl(h, x0, lens, visits, coef, noise, known, fixed, kcoef, known_noise, seed, guide, packed, tpl_packed, offset=OFFSET,
                        max_norm=1.0, clash=NO_CLASH, out=True, energy=True, rmsd=True):
    """fd_sample_guided_inpaint_tpl -> (rc, out, energy [B, 3], max_violation, tpl_rmsd); the outputs start at the sentinel."""
    arr = lambda a, dt=np.float32: None if a is None else np.ascontiguousarray(a, dtype=dt)   # noqa: E731
    B = len(LENS4)
    vs = arr(visits, np.int32)
    prm = _params(6, offset, max_norm, clash)
    buf = np.full((B, L_R, 6), SENTINEL, dtype=np.float32) if out else None
    e, mv, rm = (np.full((B, 3), SENTINEL) if energy else None), np.full(B, SENTINEL), (np.full(B, SENTINEL) if rmsd else None)
    rc = _binding.load().fd_sample_guided_inpaint_tpl(h, P(arr(x0)), P(arr(lens, np.int32)), B, L_R, P(vs), len(vs), P(arr(coef)), P(arr(noise)),
                                                      P(arr(known)), P(arr(fixed, np.uint8)), P(arr(kcoef)), P(arr(known_noise)), C.c_uint64(seed),
                                                      C.c_int64(0), P(arr(guide)), C.byref(prm), *(P(a) for a in packed), *(P(a) for a in tpl_packed),
                                                      P(buf), P(e), P(mv), P(rm))
    return rc, buf, e, mv, rm


def _run_templates(seed):
    """LENS4 = 16, 13, 9, 14: the held rows' CA atoms, scattered atoms with weights, none, all atoms."""
    rng = np.random.default_rng(seed)
    target = lambda n: moved(rng, gr.build_ref(random_features(rng, n, 6), IDX[6]), 30.0)   # noqa: E731
    held = np.array([3 * r + 1 for r in list(range(3, 7)) + list(range(10, 14))])
    scattered = np.sort(rng.choice(39, size=11, replace=False))
    return [(held, target(16)[held], np.ones(8)), (scattered, target(13)[scattered], rng.uniform(0.5, 2.0, 11)), tr.NO_TEMPLATE,
            (np.arange(42), target(14), np.full(42, 0.25))]


def _chain_of_hooks(h, x0, visits, coef, guide, noise, known_noise, known, fixed, kcoef, packed, tpl_packed, seed, clash):
    """tests/test_scaffold_guide_gpu.py's chain with fd_scaffold_guide_step_tpl as its last hook."""
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
        rc, state, *_ = _sg_step_tpl(x, pred, known, fixed, LENS4, packed, tpl_packed, guide[i], s=s, z=None if noise is None else noise[i], seed=seed,
                                     t=int(t), offset=OFFSET, clash=clash)
        assert rc == 0, _err()
    return state


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 20, K = 5, B = 4, L = 16, eta = 1: with clashes and explicit draws, without and with Philox; eager launches and packed
    rows give the same bits below the lengths; the final state's three energies and the template rmsd are the hook's on the
    final state."""
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_S)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    ok = _valid(LENS4, L_R, 6)
    visits, coef, guide, x0, noise, known_noise, known, fixed, packed = _run_case(betas, 0)
    tpl_packed = _pack_tpl(_run_templates(300))
    fx = fixed.astype(bool)
    for clash, zs, kz, seed in ((CLASH, noise, known_noise, 0), (NO_CLASH, None, None, 977)):
        rc, out, e, mv, rm = _guided_inpaint_tpl(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, tpl_packed, clash=clash)
        assert rc == 0, _err()
        want = _chain_of_hooks(h, x0, visits, coef, guide, zs, kz, known, fixed, kcoef, packed, tpl_packed, seed, clash)
        assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), clash
        assert np.array_equal(_bits(out)[fx], _bits(known)[fx])
        rc, _, e_hook, mv_hook, _, _, rm_hook = _sg_step_tpl(out, out, known, fixed, LENS4, packed, tpl_packed, 0.0, offset=OFFSET, clash=clash)
        assert rc == 0 and np.array_equal(_f64bits(e), _f64bits(e_hook)) and np.array_equal(_f64bits(mv), _f64bits(mv_hook))
        assert np.array_equal(_f64bits(rm), _f64bits(rm_hook)) and e[2, 2] == 0 and rm[2] == 0 and (e[[0, 1, 3], 2] > 0).all()
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            rc, out2, e2, _, rm2 = _guided_inpaint_tpl(h, x0, LENS4, visits, coef, zs, known, fixed, kcoef, kz, seed, guide, packed, tpl_packed, clash=clash)
            pm.set_option(option, int(option == "use_graph"))
            assert rc == 0 and np.array_equal(_bits(out2)[ok], _bits(out)[ok]) and np.array_equal(_f64bits(e2), _f64bits(e)), option
            assert np.array_equal(_f64bits(rm2), _f64bits(rm))
    # the template steers: the same run without it ends elsewhere
    rc, plain, _, _ = _guided_inpaint(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 977, guide, packed)
    assert rc == 0 and not np.array_equal(plain[ok], out[ok])


def test_the_run_against_its_neighbours(gpu):
    """No template: fd_sample_guided_inpaint's out, energies and violation bit for bit.  Bad calls leave the outputs alone.  A
    plain strided, a guided and a conditioned run give, behind the new run on the same handle, the bits they give first on a
    fresh handle, and the new run its own behind them."""
    betas = beta_schedules.cosine_beta_schedule(T_S)
    kcoef = sampling.inpaint_levels(betas)
    visits, coef, guide, x0, _, _, known, fixed, packed = _run_case(betas, 5)
    tpls = _run_templates(301)
    tpl_packed = _pack_tpl(tpls)
    kn = np.nan_to_num(known)
    same = lambda xs, ys: all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(xs, ys))   # noqa: E731

    def others(h):
        a = _strided(h, x0, LENS4, visits, coef[:3], 11, 0)
        b = _guided(h, x0, LENS4, visits, coef, None, 12, guide, packed)
        c = _strided_inpaint(h, x0, LENS4, visits, coef[:3], kn, fixed, kcoef, 13, 0)
        assert a[0] == 0 and b[0] == 0 and c[0] == 0, _err()
        return a[1], b[1], b[2], c[1]

    def new(h, seed=14, tpl=tpl_packed):
        got = _guided_inpaint_tpl(h, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, seed, guide, packed, tpl, clash=CLASH)
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
    # no template
    out, e, mv, rm = new(h2, tpl=NO_TPL)
    rc, pout, pe, pmv = _guided_inpaint(h2, x0, LENS4, visits, coef, None, known, fixed, kcoef, None, 14, guide, packed, clash=CLASH)
    assert rc == 0 and same((out, e[:, :2], mv), (pout, pe, pmv)) and (e[:, 2] == 0).all() and (rm == 0).all()
    empty = (np.zeros(5, np.int32), np.zeros(1, np.int32), np.zeros((1, 3)), np.ones(1))
    assert same(new(h2, tpl=empty), (out, e, mv, rm))        # offsets that give no chain an entry: that launch is skipped
    assert not np.array_equal(out, fresh_new[0])
    # bad calls
    def tpl(k, value, at=0):
        arrays = [a.copy() for a in tpl_packed]
        arrays[k].reshape(-1)[at] = value
        return tuple(arrays)

    none_at = lambda k: tuple(None if i == k else a for i, a in enumerate(tpl_packed))   # noqa: E731
    bad = [(dict(tpl=none_at(0)), b"given together"), (dict(tpl=none_at(3)), b"given together"), (dict(tpl=tpl(0, 1)), b"tpl_offsets[0]=1"),
           (dict(tpl=tpl(0, 30, 2)), b"tpl_offsets[3]=19 is below"), (dict(tpl=tpl(1, 48, 7)), b"template entry 7 = atom 48 outside chain 0's [0, 48)"),
           (dict(tpl=tpl(1, 10, 1)), b"template entry 1 = atom 10 after atom 10"), (dict(tpl=tpl(3, 0.0, 9)), b"template entry 9: w=0"),
           (dict(tpl=tpl(3, np.inf, 2)), b"template entry 2: w=inf"), (dict(tpl=tpl(2, np.nan, 14)), b"template entry 4: target coordinate 2"),
           (dict(rmsd=False), b"tpl_rmsd_out"), (dict(out=False), b"null"), (dict(energy=False), b"null"), (dict(lens=[16, 13, 0, 14]), b"lens[2]=0"),
           (dict(clash=sg.Clash(0.63, 0.15, -1.0)), b"w_clash=-1"), (dict(max_norm=0.0), b"max_norm=0")]
    for kw, word in bad:
        a = dict(lens=LENS4, tpl=tpl_packed, out=True, energy=True, rmsd=True, clash=CLASH, max_norm=1.0)
        a.update(kw)
        rc, out, e, mv, rm = _guided_inpaint_tpl(h2, x0, a["lens"], visits, coef, None, known, fixed, kcoef, None, 5, guide, packed, a["tpl"],
                                                 max_norm=a["max_norm"], clash=a["clash"], out=a["out"], energy=a["energy"], rmsd=a["rmsd"])
        assert rc == -1 and word in _err(), (word, rc, _err())
        assert all(o is None or (o == SENTINEL).all() for o in (out, e, mv, rm)), word
    assert same(new(h2), fresh_new)


# ---------------------------------------------------------------------------------- 4. Python end to end
def test_scaffold_segments_places_by_template_on_a_tiny_model(gpu):
    """tests/test_scaffold_guide_gpu.py's case with placement="template": each held segment's backbone within 1e-3 A of the
    motif's after superposition, template_energy / template_rmsd are structures.template_energy's of the returned backbones,
    no distance restraint was made, and the run is reproducible.  Nothing is asked of the rmsd itself: the weights are random."""
    _, _, pm = _pair(seed=11, precision="f16x3")
    inner = datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=OFFSET)
    ds = datasets.NoisedAnglesDataset(inner, timesteps=20, beta_schedule="cosine")
    motif_angles = random_features(np.random.default_rng(6), 12, 6)
    motif_xyz = nerf.build_backbones([motif_angles], NAMES, center_coords=False)[0]
    segs = [(1, 5, 4), (7, 11, 20)]
    kw = dict(num_steps=6, scale=1.0, max_norm=1.0, clash_weight=1.0, batch_size=1, placement="template")
    torch.manual_seed(3)
    got, info = sampling.scaffold_segments(pm, ds, motif_angles, motif_xyz, segs, [30, 34], **kw)
    assert [s.shape for s in got] == [(30, 6), (34, 6)] and all(np.isfinite(s).all() for s in got)
    coords = nerf.build_backbones(got, NAMES, center_coords=False)
    for lo, hi, at in segs:
        rmsd = structures.motif_rmsd(coords, motif_xyz[3 * lo: 3 * hi], [at, at])
        assert (rmsd <= 1e-3).all(), rmsd
    scan = nerf.build_backbones(got, NAMES, center_coords=False, method="scan")
    tpl = structures.motif_template(motif_xyz, segs)
    e, rmsd = structures.template_energy(scan, tpl)
    _, mirror = structures.template_energy(scan, tpl, mirror=True)
    print(f"template rmsd {rmsd.tolist()}, against the mirrored template {mirror.tolist()}")
    assert np.allclose(info["template_energy"], e, rtol=1e-9, atol=0) and np.allclose(info["template_rmsd"], rmsd, rtol=1e-9, atol=0)
    assert (info["energy"] == 0).all() and (info["max_violation"] == 0).all() and len(tpl) == 24 and (rmsd > 0).all()
    torch.manual_seed(3)
    again, info2 = sampling.scaffold_segments(pm, ds, motif_angles, motif_xyz, segs, [30, 34], **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, got)) and np.array_equal(info2["template_rmsd"], info["template_rmsd"])


def test_script_places_by_template_and_reports_both_hands(gpu, tmp_path):
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    from foldingdiff_amd.angles_and_coords import write_coords_to_pdb
    motif_pdb = write_coords_to_pdb(gr.build_ref(random_features(np.random.default_rng(4), 30, 6), IDX[6]), str(tmp_path / "motif.pdb"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_restrained.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "36",
                        "--num_steps", "5", "--seed", "3", "--motif_pdb", motif_pdb, "--motif_residues", "3-6,20-22", "--placed_at", "8,25",
                        "--placement", "template", "--template_weight", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "restraints.json", "sampled_angles", "sampled_pdb"]
    names = [f"generated_{i}.pdb" for i in range(2)]
    assert sorted(os.listdir(os.path.join(out, "sampled_pdb"))) == names
    with open(os.path.join(out, "restraints.json")) as fh:
        report = json.load(fh)
    assert report["n_restraints"] == 0                                                     # the template takes the distances' place
    for key in ("energy", "max_violation", "template_energy", "template_rmsd", "template_mirror_rmsd", "motif_ca_rmsd"):
        assert sorted(report[key]) == names and all(np.isfinite(v) and v >= 0 for v in report[key].values()), key
