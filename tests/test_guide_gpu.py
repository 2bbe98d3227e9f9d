"""Restraint guidance on the device (fd_nerf_vjp, fd_restraint_energy, fd_guide_step, fd_sample_guided, nerf.coords_vjp,
nerf.build_backbones_torch, sampling.guide, bin/sample_restrained.py) against the numpy float64 statements of
tests/guide_reference.py and the existing entries composed on the host: bits are compared with ==, everything else with the
bound derived at its test.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guide_reference as gr
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_model, ref_sampling
import relax_reference as rx
from test_gpu_parity import PRECISIONS, _inputs, _pair, _write_model_dir
from test_guide import IDX, NAMES9, descent_case, domain_features, random_features, reparametrise
from test_repeat_gpu import LENS4, LENS5, L_R, T_R, _repeat, _tie
from test_steer_gpu import MODEL_D, NAMES, OFFSET, VISIT_SETS, _step_x0
from test_strided_gpu import ANG, F, SENTINEL, _bits, _strided, _valid

pytestmark = pytest.mark.gpu
P = _binding.ptr
MIXED = [1, 1, 1, 0, 0, 1]


def _err():
    return _binding.load().fd_last_error()


def _f64bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nerf(feats, lens, idx, center):
    """fd_nerf on padded float32 [B, L, F] -> float64 [B, 3L, 3]."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    B, L, Fx = feats.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    out = np.empty((B, 3 * L, 3))
    rc = _binding.load().fd_nerf(0, P(feats), P(ls), B, L, Fx, P(np.ascontiguousarray(idx, dtype=np.int32)), int(center), P(out))
    assert rc == 0, _err()
    return out


def _vjp(coords, lens, idx, Fx, centered, g):
    """fd_nerf_vjp -> (rc, dfeats); `dfeats` starts at the sentinel."""
    B, L = coords.shape[0], coords.shape[1] // 3
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    out = np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    rc = _binding.load().fd_nerf_vjp(0, P(np.ascontiguousarray(coords)), P(ls), B, L, Fx, P(np.ascontiguousarray(idx, dtype=np.int32)), int(centered),
                                     P(np.ascontiguousarray(g)), P(out))
    return rc, out


def _vjp_feats(coords, lens, idx, Fx, centered, g, feats):
    """fd_nerf_vjp_feats -> (rc, dfeats); `dfeats` starts at the sentinel."""
    B, L = coords.shape[0], coords.shape[1] // 3
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    out = np.full((B, L, Fx), SENTINEL, dtype=np.float64)
    rc = _binding.load().fd_nerf_vjp_feats(0, P(np.ascontiguousarray(coords)), P(ls), B, L, Fx, P(np.ascontiguousarray(idx, dtype=np.int32)),
                                           int(centered), P(np.ascontiguousarray(g)), P(np.ascontiguousarray(feats, dtype=np.float32)), P(out))
    return rc, out


def _pack(per_chain):
    """Per chain (i, j, d0, tol, w) lists -> the packed arrays of include/fdmi.h."""
    offs = np.concatenate([[0], np.cumsum([len(r[0]) for r in per_chain])]).astype(np.int32)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(r[k], dtype=dt) for r in per_chain]).astype(dt))   # noqa: E731
    return offs, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64), cat(3, np.float64), cat(4, np.float64)


def _energy(coords, lens, packed, grad=True):
    """fd_restraint_energy -> (rc, energy, max_violation, dcoords or None)."""
    B, L = coords.shape[0], coords.shape[1] // 3
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    e, mv = np.full(B, SENTINEL), np.full(B, SENTINEL)
    g = np.full(coords.shape, SENTINEL) if grad else None
    rc = _binding.load().fd_restraint_energy(0, P(np.ascontiguousarray(coords)), P(ls), B, L, *(P(a) for a in packed), P(e), P(mv), P(g))
    return rc, e, mv, g


def _guide_step(x, x0, lens, packed, c, max_norm=1.0, s=0.0, z=None, seed=0, t=0, seq_offset=0, offset=None, is_angle=ANG, idx=IDX[6]):
    """fd_guide_step -> (rc, x_out, energy, gnorm); the outputs start at the sentinel."""
    xs, x0s = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(x0, dtype=np.float32)
    B, L, Fx = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float32)
    ang = np.ascontiguousarray(np.asarray(is_angle, dtype=bool).astype(np.uint8))
    zs = None if z is None else np.ascontiguousarray(z, dtype=np.float32)
    out, e, gn = np.full_like(xs, SENTINEL), np.full(B, SENTINEL), np.full(B, SENTINEL)
    rc = _binding.load().fd_guide_step(0, P(xs), P(x0s), P(ls), B, L, Fx, P(np.ascontiguousarray(idx, dtype=np.int32)), P(off), P(ang),
                                       *(P(a) for a in packed), C.c_float(c), C.c_double(max_norm), C.c_float(s), P(zs), C.c_uint64(seed), int(t),
                                       C.c_int64(seq_offset), P(out), P(e), P(gn))
    return rc, out, e, gn


def _guided(h, x0, lens, visits, coef, noise, seed, guide, packed, max_norm=1.0, offset=OFFSET, idx=None, n_visits=None, out=True, params=True,
            energy=True):
    """fd_sample_guided -> (rc, out, energy, max_violation); the outputs start at the sentinel."""
    x0 = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float32)
    ls = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    B = len(LENS4)
    vs = None if visits is None else np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    K = n_visits if n_visits is not None else len(vs)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float32)
    zs = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    gt = None if guide is None else np.ascontiguousarray(guide, dtype=np.float32)
    gp = sampling.guide_params(NAMES, offset, 1.0)
    gp.max_norm = max_norm
    if idx is not None:
        gp.feat_idx[:] = [int(v) for v in idx]
    buf = np.full((B, L_R, F), SENTINEL, dtype=np.float32) if out else None
    e, mv = (np.full(B, SENTINEL) if energy else None), np.full(B, SENTINEL)
    rc = _binding.load().fd_sample_guided(h, P(x0), P(ls), B, L_R, P(vs), K, P(cf), P(zs), C.c_uint64(seed), C.c_int64(0), P(gt),
                                          C.byref(gp) if params else None, *(P(a) for a in packed), P(buf), P(e), P(mv))
    return rc, buf, e, mv


def _ca_restraints(rng, residues, n_target, w=1.0, tol=0.0):
    """All CA-CA pairs among `residues` at their distances in a random chain of n_target residues."""
    target = gr.build_ref(random_features(rng, n_target, 6), IDX[6])
    ca = [3 * r + 1 for r in residues]
    pairs = [(a, b) for k, a in enumerate(ca) for b in ca[k + 1:]]
    n = len(pairs)
    return ([p[0] for p in pairs], [p[1] for p in pairs], [float(np.linalg.norm(target[a] - target[b])) for a, b in pairs], [tol] * n, [w] * n)


def _fd_nerf_builder(ang, idx):
    """The guide statement's coordinates: fd_nerf (center = 0) of one chain's float32 rows."""
    return _nerf(np.asarray(ang, dtype=np.float32)[None], [len(ang)], idx, 0)[0]


def _model_space(rng, lens, L):
    """float32 [B, L, 6] whose shift by OFFSET gives plausible backbone angles; rows at or beyond a length at the sentinel."""
    x = np.full((len(lens), L, F), SENTINEL, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = ref_sampling.wrap(torch.from_numpy(random_features(rng, n, 6) - OFFSET)).numpy()
    return x


# ---------------------------------------------------------------------------------- 5. the derivative against the statement
def _check_vjp(feats, lens, idx, Fx, centered, seed):
    B, L = feats.shape[:2]
    coords = _nerf(feats, lens, idx, centered)
    g = np.random.default_rng(seed).standard_normal(coords.shape)
    rc, got = _vjp(coords, lens, idx, Fx, centered, g)
    assert rc == 0, _err()
    worst = 0.0
    for b, n in enumerate(lens):
        want = gr.nerf_vjp(coords[b, : 3 * n], g[b, : 3 * n], idx, Fx, centered)
        assert (got[b, n:] == SENTINEL).all()                                          # rows at or beyond a length: not written
        if n == 1:
            assert (got[b, :1] == 0).all() and not np.signbit(got[b, :1]).any()
            continue
        rel = np.abs(got[b, :n] - want).max() / np.abs(want).max()
        worst = max(worst, rel)
        assert rel <= 1e-9, (b, n, rel)
        assert (got[b, :n][want == 0] == 0).all()                                      # what NeRF does not read stays exactly 0
    rc, again = _vjp(coords, lens, idx, Fx, centered, g)
    assert rc == 0 and np.array_equal(_f64bits(again), _f64bits(got))
    return worst


@pytest.mark.parametrize("Fx", [6, 9, 3])
@pytest.mark.parametrize("centered", [0, 1])
def test_vjp_equals_the_statement_on_fd_nerf_coordinates(gpu, Fx, centered):
    """B = 6, L = 12, lens 1 .. 12, random upstream gradients; gate 1e-9 of the chain's largest entry: fp64, at most 6144
    terms, positions relative to atom 0, a lever-to-result ratio up to about 1e3 -- 1.1e-16 x 6144 x 1e3 = 7e-10."""
    lens = [1, 2, 3, 7, 12, 12]
    rng = np.random.default_rng(50 + Fx)
    feats = np.stack([random_features(rng, 12, Fx) for _ in lens])
    worst = _check_vjp(feats, lens, IDX[Fx], Fx, centered, 60 + Fx)
    print(f"F={Fx} centered={centered}: largest distance to the statement {worst:.2e} of the chain's largest entry")


@pytest.mark.parametrize("n,Fx", [(86, 9), (100, 6), (2048, 6)])
def test_vjp_on_chains_with_more_atoms_than_lanes(gpu, n, Fx):
    """258 atoms: the first chain with more than one atom per lane of the 256-lane workgroup; 100 residues: runs of two with
    idle lanes behind; 2048: every lane owns 24 atoms and every wave boundary carries.  The same gate."""
    rng = np.random.default_rng(n)
    for centered in (0, 1):
        worst = _check_vjp(random_features(rng, n, Fx)[None], [n], IDX[Fx], Fx, centered, n + centered)
        print(f"len={n} F={Fx} centered={centered}: {worst:.2e} of the chain's largest entry")


# ---------------------------------------------------------------------------------- 5b. the whole domain of the forward
DOMAIN_BATCHES = (((1, 2, 3, 7, 12, 12), ("signs", "negative", "backbone", "signs", "negative", "signs")), ((86,), ("signs",)), ((100,), ("negative",)),
                  ((600,), ("signs",)))


@functools.lru_cache(maxsize=None)
def _domain_case(Fx, centered, batches=DOMAIN_BATCHES):
    """Chains of tests/test_guide.py's domain_features (bond angles and lengths of either sign), the coordinates of the float64
    torch restatement on them and autograd's gradient of a random weighting of those coordinates.  Computed once per (F,
    centered) and left unchanged: a list of dicts feats [B, L, F], lens, g [B, 3L, 3], xyz64 [B, 3L, 3], want [B, L, F]."""
    out = []
    for k, (lens, modes) in enumerate(batches):
        rng = np.random.default_rng(9000 + 100 * Fx + 10 * k + centered)
        B, L = len(lens), max(lens)
        feats = np.full((B, L, Fx), SENTINEL, dtype=np.float32)
        g, xyz64, want = rng.standard_normal((B, 3 * L, 3)), np.zeros((B, 3 * L, 3)), np.zeros((B, L, Fx))
        for b, (n, mode) in enumerate(zip(lens, modes)):
            feats[b, :n] = domain_features(rng, n, Fx, mode)
            xyz64[b, : 3 * n], want[b, :n] = gr.autograd_vjp(feats[b, :n], IDX[Fx], g[b, : 3 * n], bool(centered))
        out.append(dict(feats=feats, lens=lens, g=g, xyz64=xyz64, want=want))
    return out


def _check_against_autograd(case, coords, Fx, centered, gate):
    """fd_nerf_vjp_feats on `coords` against the case's autograd gradient, per chain within `gate` of its largest entry."""
    lens = case["lens"]
    rc, got = _vjp_feats(coords, lens, IDX[Fx], Fx, centered, case["g"], case["feats"])
    assert rc == 0, _err()
    worst = 0.0
    for b, n in enumerate(lens):
        assert (got[b, n:] == SENTINEL).all()
        want = case["want"][b, :n]
        if n == 1:
            assert (got[b, :1] == 0).all() and (want == 0).all()
            continue
        rel = np.abs(got[b, :n] - want).max() / np.abs(want).max()
        worst = max(worst, rel)
        assert rel <= gate, (lens, b, n, rel)
        assert (got[b, :n][want == 0] == 0).all()
    return worst, got


@pytest.mark.parametrize("Fx", [3, 6, 9])
@pytest.mark.parametrize("centered", [0, 1])
def test_vjp_feats_against_autograd_on_the_restatements_coordinates(gpu, Fx, centered):
    """The device is given the float64 restatement's coordinates and the rows they were built from; gate 2e-9 of the chain's
    largest entry: the 1e-9 derived for device against statement (test_vjp_equals_the_statement_on_fd_nerf_coordinates) plus the
    statement's 1e-12 against autograd.  Lengths 1 .. 12 in one ragged batch, 86 (258 atoms: more than one per lane), 100, 600."""
    worst = 0.0
    for case in _domain_case(Fx, centered):
        w, got = _check_against_autograd(case, case["xyz64"], Fx, centered, 2e-9)
        worst = max(worst, w)
        rc, again = _vjp_feats(case["xyz64"], case["lens"], IDX[Fx], Fx, centered, case["g"], case["feats"])
        assert rc == 0 and np.array_equal(_f64bits(again), _f64bits(got))                # two calls, the same bits
    print(f"F={Fx} centered={centered}: largest distance to autograd {worst:.2e} of the chain's largest entry")


def test_vjp_feats_against_autograd_at_2048_residues(gpu):
    """Every lane owns 24 atoms and every wave boundary carries.  The same gate."""
    case = _domain_case(6, 1, (((2048,), ("signs",)),))[0]
    worst, _ = _check_against_autograd(case, case["xyz64"], 6, 1, 2e-9)
    print(f"len=2048: {worst:.2e} of the chain's largest entry")


@pytest.mark.parametrize("Fx", [3, 6, 9])
@pytest.mark.parametrize("centered", [0, 1])
def test_vjp_feats_against_autograd_end_to_end(gpu, Fx, centered):
    """fd_nerf's own coordinates (float32 cos / sin products inside), then fd_nerf_vjp_feats: within 1e-5 of autograd's largest
    entry through the float64 restatement -- the statement alone stays within 2.1e-6 at 600 residues (tests/test_guide.py), the
    device adds the last bit of float32 sin and cos."""
    worst = 0.0
    for case in _domain_case(Fx, centered):
        coords = _nerf(case["feats"], case["lens"], IDX[Fx], centered)
        worst = max(worst, _check_against_autograd(case, coords, Fx, centered, 1e-5)[0])
    print(f"F={Fx} centered={centered}: largest distance to autograd {worst:.2e} of the chain's largest entry")


def _scan(feats, lens, idx, center):
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    B, L, Fx = feats.shape
    out = np.empty((B, 3 * L, 3))
    rc = _binding.load().fd_nerf_scan(0, P(feats), P(np.ascontiguousarray(np.asarray(lens, dtype=np.int32))), B, L, Fx,
                                      P(np.ascontiguousarray(idx, dtype=np.int32)), int(center), P(out))
    assert rc == 0, _err()
    return out


@pytest.mark.parametrize("Fx", [3, 6, 9])
def test_forward_against_the_oracle_and_scan_against_serial_on_the_whole_domain(gpu, Fx):
    """fd_nerf against oracle/ref_nerf.build on the same rows.  Per chain d_ref = max |float64 restatement - ref_nerf.build| is
    how far rounding the float32 products alone moves that chain; the device differs from the oracle by last bits of the same
    float32 quantities, so the gate is 4 d_ref and the measured ratio is printed.  fd_nerf_scan against fd_nerf:
    the header's 1e-9 of the chain's extent.  Both centred and not; two calls give the same bits; a chain gives the same bits
    alone and inside the batch."""
    worst_ratio, worst_scan = 0.0, 0.0
    for centered in (0, 1):
        for case in _domain_case(Fx, centered):
            feats, lens = case["feats"], case["lens"]
            serial, scan = _nerf(feats, lens, IDX[Fx], centered), _scan(feats, lens, IDX[Fx], centered)
            assert np.array_equal(_f64bits(serial), _f64bits(_nerf(feats, lens, IDX[Fx], centered)))
            assert np.array_equal(_f64bits(scan), _f64bits(_scan(feats, lens, IDX[Fx], centered)))
            for b, n in enumerate(lens):
                ref = gr.build_ref(feats[b, :n], IDX[Fx])
                gate = rx.scan_gate(ref)
                if centered:
                    ref = ref - ref.mean(axis=0)
                d_ref = np.abs(case["xyz64"][b, : 3 * n] - ref).max()
                err = np.abs(serial[b, : 3 * n] - ref).max()
                if d_ref > 0:
                    worst_ratio = max(worst_ratio, err / d_ref)
                assert err <= 4 * d_ref, (Fx, centered, n, err, d_ref)
                err_scan = np.abs(scan[b, : 3 * n] - serial[b, : 3 * n]).max()
                worst_scan = max(worst_scan, err_scan / gate * 1e-9)
                assert err_scan <= gate, (Fx, centered, n, err_scan, gate)
                assert (serial[b, 3 * n:] == 0).all() and (scan[b, 3 * n:] == 0).all()
            if len(lens) > 1:                                                           # the 12-residue chain at index 4, alone
                alone = feats[4:5].copy()
                assert np.array_equal(_f64bits(_nerf(alone, [12], IDX[Fx], centered)[0]), _f64bits(serial[4]))
                assert np.array_equal(_f64bits(_scan(alone, [12], IDX[Fx], centered)[0]), _f64bits(scan[4]))
                args = (IDX[Fx], Fx, centered, case["g"][4:5], alone)
                rc, one = _vjp_feats(serial[4:5], [12], *args)
                rc2, batch = _vjp_feats(serial, lens, IDX[Fx], Fx, centered, case["g"], feats)
                assert rc == 0 and rc2 == 0 and np.array_equal(_f64bits(one[0]), _f64bits(batch[4]))
    print(f"F={Fx}: |fd_nerf - ref_nerf.build| is at most {worst_ratio:.3f} d_ref; fd_nerf_scan within {worst_scan:.2e} of the chain's extent of fd_nerf")


@pytest.mark.parametrize("Fx", [6, 9])
def test_vjp_feats_returns_fd_nerf_vjp_bits_where_every_sign_is_positive(gpu, Fx):
    """random_features chains (sin(angle) > 0, lengths > 0): the new entry and fd_nerf_vjp agree bit for bit; on domain_features
    they differ in sign exactly where the statement says and nowhere in magnitude."""
    lens = [1, 2, 3, 7, 12, 86]
    rng = np.random.default_rng(70 + Fx)
    feats = np.zeros((len(lens), 86, Fx), dtype=np.float32)
    for b, n in enumerate(lens):
        feats[b, :n] = random_features(rng, n, Fx)
    for centered in (0, 1):
        coords = _nerf(feats, lens, IDX[Fx], centered)
        g = rng.standard_normal(coords.shape)
        rc, plain = _vjp(coords, lens, IDX[Fx], Fx, centered, g)
        rc2, signed = _vjp_feats(coords, lens, IDX[Fx], Fx, centered, g, feats)
        assert rc == 0 and rc2 == 0 and np.array_equal(_f64bits(plain), _f64bits(signed))
    case = _domain_case(Fx, 0)[1]                                                       # 86 residues, signs of either kind
    n = case["lens"][0]
    rc, plain = _vjp(case["xyz64"], [n], IDX[Fx], Fx, 0, case["g"])
    rc2, signed = _vjp_feats(case["xyz64"], [n], IDX[Fx], Fx, 0, case["g"], case["feats"])
    assert rc == 0 and rc2 == 0 and np.array_equal(_f64bits(np.abs(plain)), _f64bits(np.abs(signed)))
    f = case["feats"][0]
    sl = np.where(f[:, 6:9] < 0, -1.0, 1.0) if Fx == 9 else np.ones((n, 3))
    sa = np.where(np.sin(f[:, 3:6].astype(np.float64)) < 0, -1.0, 1.0) * sl[:, [2, 0, 1]]   # columns 3, 4, 5 go with lengths 8, 6, 7
    want = plain[0].copy()
    want[:, 3:6] *= sa
    if Fx == 9:
        want[:, 6:9] *= sl
    assert np.array_equal(_f64bits(want + 0.0), _f64bits(signed[0] + 0.0)) and (sa < 0).sum() > n


def test_python_gradients_on_the_whole_domain(gpu):
    """nerf.coords_vjp with `angles` and build_backbones_torch's backward on chains with bond angles and lengths of either sign:
    both are fd_nerf_vjp_feats' (within 1e-5 of autograd through the float64 restatement, the end-to-end gate)."""
    case = _domain_case(9, 1)[0]
    lens, feats = case["lens"], case["feats"]
    rows = [feats[b, :n] for b, n in enumerate(lens)]
    coords = nerf.build_backbones(rows, NAMES9, center_coords=True)
    got = nerf.coords_vjp(coords, [case["g"][b, : 3 * n] for b, n in enumerate(lens)], NAMES9, centered=True, angles=rows)
    ang = torch.tensor(feats, requires_grad=True)
    xyz = nerf.build_backbones_torch(ang, lens, NAMES9, center_coords=True)
    (xyz * torch.from_numpy(case["g"])).sum().backward()
    for b, n in enumerate(lens):
        want = case["want"][b, :n]
        scale = max(np.abs(want).max(), 1e-300)
        assert np.abs(got[b] - want).max() <= 1e-5 * scale, (b, n)
        assert np.array_equal(_bits(ang.grad.numpy()[b, :n]), _bits(got[b].astype(np.float32))) and (ang.grad.numpy()[b, n:] == 0).all()


# ---------------------------------------------------------------------------------- 6. the torch path
def test_torch_backward_is_coords_vjp_and_agrees_with_autograd(gpu):
    lens, L = [12, 7, 2], 12
    rng = np.random.default_rng(8)
    feats = np.stack([random_features(rng, L, 6) for _ in lens])
    w = rng.standard_normal((3, 3 * L, 3))
    for center in (True, False):
        ang = torch.tensor(feats, requires_grad=True)
        xyz = nerf.build_backbones_torch(ang, lens, NAMES, center_coords=center)
        assert xyz.dtype == torch.float64 and tuple(xyz.shape) == (3, 3 * L, 3)
        plain = nerf.build_backbones([feats[b, :n] for b, n in enumerate(lens)], NAMES, center_coords=center)
        assert all(np.array_equal(xyz[b, : 3 * n].detach().numpy(), plain[b]) for b, n in enumerate(lens))
        ((xyz * torch.from_numpy(w)).sum() ** 2).backward()                             # any torch loss: here the square of a weighted sum
        total = float((xyz.detach() * torch.from_numpy(w)).sum())
        want = nerf.coords_vjp(plain, [2.0 * total * w[b, : 3 * n] for b, n in enumerate(lens)], NAMES, centered=center)
        got = ang.grad.numpy()
        for b, n in enumerate(lens):
            assert np.array_equal(_bits(got[b, :n]), _bits(want[b].astype(np.float32))) and (got[b, n:] == 0).all()
            _, auto = gr.autograd_vjp(feats[b, :n], IDX[6], 2.0 * total * w[b, : 3 * n], center)
            assert np.abs(want[b] - auto).max() <= 1e-5 * np.abs(auto).max()


# ---------------------------------------------------------------------------------- 7. the restraints against the statement
def test_restraint_energy_and_gradient_equal_the_statement(gpu):
    lens, L = [5, 9, 5], 9
    rng = np.random.default_rng(21)
    feats = np.zeros((3, L, 6), dtype=np.float32)
    for b, n in enumerate(lens):
        feats[b, :n] = random_features(rng, n, 6)
    coords = _nerf(feats, lens, IDX[6], 0)
    d = lambda b, i, j: float(np.linalg.norm(coords[b, i] - coords[b, j]))   # noqa: E731
    per = [([1, 4, 13, 0, 13], [10, 13, 7, 14, 2], [d(0, 1, 10) + 0.3, 3.0, d(0, 13, 7) + 2.0, 1.0, 0.0], [0.5, 0.0, 0.25, 0.0, 8.0],
            [1.0, 2.0, 0.5, 0.0, 3.0]),                                    # inside its tolerance | .. | shares atom 13 | w = 0 | a contact
           _ca_restraints(rng, [0, 3, 5, 8], 9, w=0.7),
           ([], [], [], [], [])]                                           # a chain with none
    packed = _pack(per)
    rc, e, mv, g = _energy(coords, lens, packed)
    assert rc == 0, _err()
    for b, n in enumerate(lens):
        we, wv, wg = gr.restraint_energy(coords[b, : 3 * n], per[b])
        assert abs(e[b] - we) <= 1e-12 * abs(we) and abs(mv[b] - wv) <= 1e-12 * wv, (b, e[b], we, mv[b], wv)
        assert np.abs(g[b, : 3 * n] - wg).max() <= 1e-12 * max(np.abs(wg).max(), 1e-300) and (g[b, 3 * n:] == 0).all()
    assert e[2] == 0 and mv[2] == 0 and (g[2] == 0).all() and e[0] > 0 and e[1] > 0
    first = gr.restraint_energy(coords[0, :15], tuple(v[:1] for v in per[0]))
    assert first[0] == 0 and first[1] == 0                                              # (the satisfied one is satisfied)
    rc, e2, mv2, g2 = _energy(coords, lens, packed)
    assert rc == 0 and all(np.array_equal(_f64bits(a), _f64bits(b)) for a, b in ((e, e2), (mv, mv2), (g, g2)))
    rc, e3, mv3, _ = _energy(coords, lens, packed, grad=False)                          # the gradient is optional
    assert rc == 0 and np.array_equal(_f64bits(e3), _f64bits(e)) and np.array_equal(_f64bits(mv3), _f64bits(mv))
    # the Python entry: the same numbers from lists of chains
    sets = [structures.Restraints(*r) for r in per]
    pe, pv, pg = structures.restraint_energy([coords[b, : 3 * n] for b, n in enumerate(lens)], sets, return_gradient=True)
    assert np.array_equal(_f64bits(pe), _f64bits(e)) and np.array_equal(_f64bits(pv), _f64bits(mv))
    assert all(np.array_equal(pg[b], g[b, : 3 * n]) for b, n in enumerate(lens))


# ---------------------------------------------------------------------------------- 8. the hook against the statement
def _step_case():
    rng = np.random.default_rng(31)
    x = _inputs(5, L_R, seed=32).numpy()
    x0 = _model_space(rng, LENS5, L_R)
    for b, n in enumerate(LENS5):
        x[b, n:] = SENTINEL
    weights = [1.0, 1.0, 1e-6, 1.0, 1e-6]                                               # the clip: active | .. | inactive
    per = [_ca_restraints(rng, [1, 3, 5, 7], 8, w=w) for w in weights]
    return x, x0, per, _pack(per)


def test_guide_step_with_c_zero_is_the_tie_statement_bit_for_bit(gpu):
    x, x0, _, packed = _step_case()
    ok = _valid(LENS5, L_R)
    z = np.random.default_rng(33).standard_normal((5, L_R, F)).astype(np.float32)
    untied = [(0, 1, 1)] * 5
    for is_angle in (ANG, MIXED):
        for kw in (dict(), dict(s=0.3, z=z), dict(s=0.3, z=None, seed=(7 << 40) + 99, t=5, seq_offset=1 << 33)):
            rc, got, e, gn = _guide_step(x, x0, LENS5, packed, 0.0, offset=OFFSET, is_angle=is_angle, **kw)
            assert rc == 0, _err()
            rc, want = _tie(x, LENS5, untied, is_angle, **kw)
            assert rc == 0, _err()
            assert np.array_equal(_bits(got)[ok], _bits(want)[ok]) and (got[~ok] == SENTINEL).all(), (is_angle, sorted(kw))
            assert (e > 0).all() and (gn > 0).all()                                     # the energy and the norm are reported all the same


def test_guide_step_equals_the_statement(gpu):
    """c != 0: x_out within 2e-6 of the statement, on the circle for wrapped columns -- G agrees to 1e-9, what remains is
    float32 roundings of values below 8 (the product, the difference, the sum with the draw, the wrap's two sums), each of which
    may fall one half-ulp step of 2.4e-7 apart, five in all.  gnorm and energy to 1e-9 relative.  The statement's coordinates
    are fd_nerf's, as the statement says."""
    x, x0, per, packed = _step_case()
    ok = _valid(LENS5, L_R)
    z = np.random.default_rng(34).standard_normal((5, L_R, F)).astype(np.float32)
    for is_angle, c, s in ((ANG, 0.05, 0.0), (MIXED, 0.05, 0.3), (ANG, -0.2, 0.3)):
        rc, got, e, gn = _guide_step(x, x0, LENS5, packed, c, max_norm=1.0, s=s, z=z, offset=OFFSET, is_angle=is_angle)
        assert rc == 0, _err()
        want, we, wn, clip = gr.guide_step(x, x0, LENS5, IDX[6], OFFSET, is_angle, per, c, 1.0, s=s, z=z, build=_fd_nerf_builder)
        ang = np.asarray(is_angle, dtype=bool)
        dist = np.where(ang, ref_sampling.circ_dist(got, want), np.abs(got.astype(np.float64) - want))[ok]
        print(f"c={c} s={s}: max distance {dist.max():.2e}; energy rel {np.abs(e / we - 1).max():.2e}; gnorm rel {np.abs(gn / wn - 1).max():.2e}; "
              f"gnorm {np.round(wn, 4).tolist()}, clipped {(clip < 1).tolist()}")
        assert dist.max() <= 2e-6 and (got[~ok] == SENTINEL).all()
        assert np.abs(e / we - 1).max() <= 1e-9 and np.abs(gn / wn - 1).max() <= 1e-9
        assert (clip < 1).any() and (clip == 1).any()
        rc, plain, _, _ = _guide_step(x, x0, LENS5, packed, 0.0, s=s, z=z, offset=OFFSET, is_angle=is_angle)
        assert rc == 0 and np.abs(got - plain)[ok].max() > 1e-3                         # ... and the step was taken


def _device_G(x0, lens, per, packed):
    """The G of the guide statement from the device's own entries: the shift on the host (one rounding, tests/guide_reference.py),
    fd_nerf, fd_restraint_energy's gradient, fd_nerf_vjp_feats on the shifted rows."""
    ang = np.zeros_like(x0)
    for b, n in enumerate(lens):
        ang[b, :n] = gr.shift(x0[b, :n], OFFSET, ANG)
    coords = _nerf(ang, lens, IDX[6], 0)
    rc, _, _, gc = _energy(coords, lens, packed)
    assert rc == 0, _err()
    rc, G = _vjp_feats(coords, lens, IDX[6], F, 0, gc, ang)
    assert rc == 0, _err()
    return ang, coords, G


def test_guide_step_where_half_of_the_bond_angles_are_negative(gpu):
    """_step_case with a random half of the rows of the shifted x0 re-parametrised as (-angle, wrap(torsion + pi)): the same
    structures to about 1e-5 A, so the same energies and the same step on the torsions, but the bond-angle entries of G change
    sign exactly in those rows (|dG| <= 1e-4 |G| on entries above 1e-3 of the chain's largest).  fd_guide_step against the
    statement with the gates of test_guide_step_equals_the_statement: 2e-6 on x_out, 1e-9 on gnorm and energy.  A derivative
    from the coordinates alone pushes those bond angles up the gradient."""
    x, x0, per, packed = _step_case()
    ok = _valid(LENS5, L_R)
    rng = np.random.default_rng(35)
    x0_neg, flipped = x0.copy(), np.zeros((5, L_R), dtype=bool)
    for b, n in enumerate(LENS5):
        flipped[b, :n] = rng.random(n) < 0.5
        target = reparametrise(gr.shift(x0[b, :n], OFFSET, ANG), flipped[b, :n])
        x0_neg[b, :n] = ref_sampling.wrap(torch.from_numpy(target - OFFSET)).numpy()
    ang, coords, G = _device_G(x0, LENS5, per, packed)
    ang_neg, coords_neg, G_neg = _device_G(x0_neg, LENS5, per, packed)
    below = ok[:, :, 0]
    share = (ang_neg[below][:, 3:] < 0).mean()
    moved = np.abs(coords_neg - coords).max()
    print(f"{share:.2f} of the bond angles negative; re-parametrising moves the atoms by at most {moved:.2e} A")
    assert 0.3 < share < 0.7 and (ang[below][:, 3:] > 0).all() and moved <= 1e-4
    compared = 0
    for b, n in enumerate(LENS5):
        big = np.abs(G[b, :n]) > 1e-3 * np.abs(G[b, :n]).max()
        sign = np.ones((n, F))
        sign[flipped[b, :n], 3:] = -1.0
        assert (np.abs(G_neg[b, :n] - sign * G[b, :n])[big] <= 1e-4 * np.abs(G[b, :n])[big]).all(), b
        compared += int(big[flipped[b, :n], 3:].sum())
    assert compared >= 30
    z = np.random.default_rng(34).standard_normal((5, L_R, F)).astype(np.float32)
    for is_angle, c, s in ((ANG, 0.05, 0.0), (MIXED, 0.05, 0.3), (ANG, -0.2, 0.3)):
        rc, got, e, gn = _guide_step(x, x0_neg, LENS5, packed, c, max_norm=1.0, s=s, z=z, offset=OFFSET, is_angle=is_angle)
        assert rc == 0, _err()
        want, we, wn, clip = gr.guide_step(x, x0_neg, LENS5, IDX[6], OFFSET, is_angle, per, c, 1.0, s=s, z=z, build=_fd_nerf_builder)
        isang = np.asarray(is_angle, dtype=bool)
        dist = np.where(isang, ref_sampling.circ_dist(got, want), np.abs(got.astype(np.float64) - want))[ok]
        print(f"c={c} s={s}: max distance {dist.max():.2e}; energy rel {np.abs(e / we - 1).max():.2e}; gnorm rel {np.abs(gn / wn - 1).max():.2e}")
        assert dist.max() <= 2e-6 and (got[~ok] == SENTINEL).all()
        assert np.abs(e / we - 1).max() <= 1e-9 and np.abs(gn / wn - 1).max() <= 1e-9
        # ... and the statement without the rows is somewhere else: the test tells the two derivatives apart
        unsigned, *_ = gr.guide_step(x, x0_neg, LENS5, IDX[6], OFFSET, is_angle, per, c, 1.0, s=s, z=z, build=_fd_nerf_builder, signs=False)
        assert np.where(isang, ref_sampling.circ_dist(got, unsigned), np.abs(got.astype(np.float64) - unsigned))[ok].max() > 1e-3


# ---------------------------------------------------------------------------------- 9. descent on the device
def test_fifty_guide_steps_bring_the_energy_to_a_quarter(gpu):
    cases = [descent_case(seed) for seed in range(4)]
    x = np.concatenate([c[0] for c in cases])
    packed = _pack([c[1] for c in cases])
    lens = [24] * 4
    first = None
    for k in range(50):
        rc, x, e, _ = _guide_step(x, x, lens, packed, 0.05, max_norm=1.0)
        assert rc == 0, _err()
        first = e if first is None else first
        if k == 1:
            assert (e < first).all()
    rc, final, _, _ = _energy(_nerf(x, lens, IDX[6], 0), lens, packed, grad=False)
    assert rc == 0, _err()
    print("energy at the start", np.round(first, 2).tolist(), "after 50 steps", np.round(final, 2).tolist())
    assert (final <= 0.25 * first).all()


# ---------------------------------------------------------------------------------- 10. the run is the chain of its hooks
def _run_case(betas, vi, seed, scale=1.0):
    visits = VISIT_SETS[vi]
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    guide = sampling.guidance_coefficients(betas, visits, coef, scale)
    x0 = _inputs(4, L_R, seed=190 + seed).numpy()
    noise = np.random.default_rng(191 + seed).standard_normal((len(visits), 4, L_R, F)).astype(np.float32)
    rng = np.random.default_rng(192 + seed)
    per = [_ca_restraints(rng, [1, 3, 5, 8], 9), _ca_restraints(rng, [0, 6, 12], 13, tol=0.5), ([], [], [], [], []),
           _ca_restraints(rng, [2, 7, 13], 14, w=1e-3)]
    return visits, coef, guide, x0, noise, _pack(per)


def _chain_of_hooks(h, x0, visits, coef, guide, noise, packed):
    state = x0
    for i, t in enumerate(visits):
        a, b, s, u, v = coef[:, i]
        rc, _, pred, state = _step_x0(h, state, t, LENS4, a, b, 0.0, u, v, None)
        assert rc == 0, _err()
        rc, state, _, _ = _guide_step(state, pred, LENS4, packed, guide[i], max_norm=1.0, s=s, z=noise[i], offset=OFFSET)
        assert rc == 0, _err()
    return state


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 10, B = 4, L = 16, explicit noise, eta = 1: fd_sample_guided's out is, per visit, fd_p_sample_step_coef_x0 (s = 0,
    no z) followed by fd_guide_step (the visit's c, s and noise row); eager launches and packed rows give the same bits below
    the lengths; an all-zero guide table is fd_sample_repeat with nothing tied."""
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_R)
    h = pm.prepare(betas)
    ok = _valid(LENS4, L_R)
    for vi in range(len(VISIT_SETS)):
        visits, coef, guide, x0, noise, packed = _run_case(betas, vi, vi)
        assert (guide != 0).all() and (coef[2, :-1] != 0).all()
        rc, out, e, mv = _guided(h, x0, LENS4, visits, coef, noise, 0, guide, packed)
        assert rc == 0, _err()
        want = _chain_of_hooks(h, x0, visits, coef, guide, noise, packed)
        assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), visits
        rc, _, e_hook, _ = _guide_step(out, out, LENS4, packed, 0.0, offset=OFFSET)     # the final state's energy, by the hook
        assert rc == 0 and np.array_equal(_f64bits(e), _f64bits(e_hook)) and e[2] == 0 and mv[2] == 0 and (mv[[0, 1, 3]] > 0).all()
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            rc, out2, e2, _ = _guided(h, x0, LENS4, visits, coef, noise, 0, guide, packed)
            pm.set_option(option, int(option == "use_graph"))
            assert rc == 0 and np.array_equal(_bits(out2)[ok], _bits(out)[ok]) and np.array_equal(_f64bits(e2), _f64bits(e)), (visits, option)
        rc, unguided, _, _ = _guided(h, x0, LENS4, visits, coef, noise, 0, np.zeros_like(guide), packed)
        assert rc == 0, _err()
        rc, rep = _repeat(h, x0, LENS4, visits, coef[:3], noise, 0, [(0, 1, 1)] * 4)
        assert rc == 0, _err()
        assert np.array_equal(_bits(unguided)[ok], _bits(rep)[ok]), visits
        assert not np.array_equal(out[ok], unguided[ok])


# ---------------------------------------------------------------------------------- 11. errors and the call history
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_R)
    h = pm.prepare(betas)
    visits, coef, guide, x0, _, packed = _run_case(betas, 0, 7)
    rc, before = _strided(h, x0, LENS4, visits, coef[:3], 5, 0)
    assert rc == 0, _err()
    nan_b, inf_v, nan_g = coef.copy(), coef.copy(), guide.copy()
    nan_b[1, 2], inf_v[4, 1], nan_g[3] = np.nan, np.inf, np.nan
    bad_off = OFFSET.copy()
    bad_off[4] = np.nan

    def rst(k, value):
        arrays = [a.copy() for a in packed]
        arrays[k][0] = value
        return tuple(arrays)

    none_at = lambda k: tuple(None if i == k else a for i, a in enumerate(packed))   # noqa: E731
    bad = [(dict(x0=None), b"null"), (dict(lens=None), b"null"), (dict(out=False), b"null"), (dict(guide=None), b"null"), (dict(params=False), b"null"),
           (dict(energy=False), b"null"), (dict(visits=None, n_visits=4), b"visits is null"), (dict(coef=None), b"coef is null"),
           (dict(n_visits=0), b"n_visits = 0"), (dict(visits=[10, 5, 2, 0]), b"visits[0] = 10 outside"), (dict(visits=[8, 5, 5, 0]), b"visits[2] = 5 follows 5"),
           (dict(coef=nan_b), b"coef[1][2]"), (dict(coef=inf_v), b"coef[4][1]"), (dict(guide=nan_g), b"guide[3]"),
           (dict(lens=[16, 13, 0, 14]), b"lens[2]=0"), (dict(lens=[17, 13, 9, 14]), b"lens[0]=17"),
           (dict(max_norm=0.0), b"max_norm=0"), (dict(max_norm=-2.0), b"max_norm=-2"), (dict(max_norm=float("inf")), b"max_norm=inf"),
           (dict(offset=bad_off), b"offset[4]"),
           (dict(idx=[0, 1, 6, 3, 4, 5, -1, -1, -1]), b"feat_idx[2]=6"), (dict(idx=[-1, 1, 2, 3, 4, 5, -1, -1, -1]), b"feat_idx[0]=-1"),
           (dict(idx=[0, 1, 2, 3, 4, 4, -1, -1, -1]), b"feat_idx[5]=4 repeats"),
           (dict(packed=none_at(0)), b"rst_offsets"), (dict(packed=none_at(2)), b"restraint lists"),
           (dict(packed=rst(1, 48)), b"restraint 0 = atoms (48, "), (dict(packed=rst(2, -1)), b"restraint 0"), (dict(lens=[8, 13, 9, 14]), b"outside chain 0's [0, 24)"),
           (dict(packed=rst(2, int(packed[1][0]))), b"restraint 0 names atom"),
           (dict(packed=rst(3, -0.5)), b"restraint 0: d0"), (dict(packed=rst(3, np.nan)), b"restraint 0: d0"), (dict(packed=rst(4, -1.0)), b"restraint 0: tol"),
           (dict(packed=rst(4, np.inf)), b"restraint 0: tol"), (dict(packed=rst(5, -1.0)), b"restraint 0: w"), (dict(packed=rst(5, np.nan)), b"restraint 0: w")]
    for kw, word in bad:
        a = dict(x0=x0, lens=LENS4, visits=visits, coef=coef, guide=guide, packed=packed, n_visits=None, out=True, params=True, energy=True,
                 max_norm=1.0, offset=OFFSET, idx=None)
        a.update(kw)
        rc, out, e, mv = _guided(h, a["x0"], a["lens"], a["visits"], a["coef"], None, 5, a["guide"], a["packed"], max_norm=a["max_norm"],
                                 offset=a["offset"], idx=a["idx"], n_visits=a["n_visits"], out=a["out"], params=a["params"], energy=a["energy"])
        assert rc == -1 and word in _err(), (word, rc, _err())
        assert (out is None or (out == SENTINEL).all()) and (e is None or (e == SENTINEL).all()) and (mv == SENTINEL).all(), word
    # after the failed calls the strided sampler is what it was
    rc, after_failed = _strided(h, x0, LENS4, visits, coef[:3], 5, 0)
    assert rc == 0 and np.array_equal(_bits(after_failed), _bits(before))
    # a guided run (Philox draws), then the strided sampler again: the per-run values are clean
    ok = _valid(LENS4, L_R)
    rc, run, e, mv = _guided(h, x0, LENS4, visits, coef, None, 5, guide, packed)
    assert rc == 0 and np.isfinite(run[ok]).all() and np.isfinite(e).all() and (mv >= 0).all(), _err()
    rc, after = _strided(h, x0, LENS4, visits, coef[:3], 5, 0)
    assert rc == 0 and np.array_equal(_bits(after), _bits(before))
    rc, again, e2, _ = _guided(h, x0, LENS4, visits, coef, None, 5, guide, packed)
    assert rc == 0 and np.array_equal(_bits(again), _bits(run)) and np.array_equal(_f64bits(e2), _f64bits(e))
    rc, other, _, _ = _guided(h, x0, LENS4, visits, coef, None, 6, guide, packed)
    assert rc == 0 and not np.array_equal(other[ok], run[ok])                           # the seed reaches the guide launch


# ---------------------------------------------------------------------------------- 12. Python end to end
def test_guide_end_to_end_on_a_tiny_model(gpu):
    """Shapes, range, determinism, and the returned energies against structures.restraint_energy of the NeRF backbones of the
    returned angles.  Nothing is asked of the energy itself: the weights are random."""
    _, _, pm = _pair(seed=11, precision="f16x3")
    inner = datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=np.array([-1.3, 1.1, 3.0, 1.95, 2.03, 2.12], np.float32))
    ds = datasets.NoisedAnglesDataset(inner, timesteps=20, beta_schedule="cosine")
    lengths = [30, 41, 30]
    rng = np.random.default_rng(5)
    motif = gr.build_ref(random_features(rng, 30, 6), IDX[6])[[3 * r + a for r in (4, 5, 6, 20, 21) for a in range(3)]]
    sets = [structures.motif_restraints(motif, [3, 4, 5, 22, 23]) + structures.contact_restraints([(0, 29)]),
            structures.contact_restraints([(2, 40, 6.0), (10, 30)], weight=2.0), None]
    kw = dict(num_steps=6, scale=1.0, max_norm=1.0, batch_size=2)   # two calls: two sequences, then one
    torch.manual_seed(3)
    got, info = sampling.guide(pm, ds, lengths, sets, **kw)
    assert [s.shape for s in got] == [(l, F) for l in lengths] and all(s.dtype == np.float32 for s in got)
    assert all(np.isfinite(s).all() and (s >= -np.float32(np.pi)).all() and (s < np.float32(np.pi)).all() for s in got)
    assert info["energy"].shape == (3,) and info["max_violation"].shape == (3,) and info["energy"][2] == 0 and (info["energy"][:2] > 0).all()
    assert info["guide"].shape == (6,) and (info["guide"] > 0).all()
    coords = nerf.build_backbones(got, NAMES, center_coords=False)
    e, mv = structures.restraint_energy(coords, sets)
    print("energy", info["energy"].tolist(), "largest violation", info["max_violation"].tolist())
    assert np.allclose(info["energy"], e, rtol=1e-12, atol=0) and np.allclose(info["max_violation"], mv, rtol=1e-12, atol=0)
    torch.manual_seed(3)
    again, info2 = sampling.guide(pm, ds, lengths, sets, **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, got)) and np.array_equal(info2["energy"], info["energy"])
    seeded = [sampling.guide(pm, ds, lengths, sets, seed=9, **kw)[0] for _ in range(2)]   # its own generator: the same without manual_seed
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*seeded)) and not np.array_equal(seeded[0][0], got[0])
    torch.manual_seed(3)
    plain, _ = sampling.guide(pm, ds, lengths, sets, **dict(kw, scale=0.0))               # scale 0: the same noise, no guidance
    assert not np.array_equal(plain[0], got[0]) and np.array_equal(_bits(plain[2]), _bits(got[2]))   # (a chain without restraints is not moved)
    with pytest.raises(ValueError):
        sampling.guide(pm, ds, [30, 20], structures.contact_restraints([(0, 29)]), **kw)
    with pytest.raises(ValueError):
        sampling.guide(pm, ds, lengths, sets, **dict(kw, max_norm=0.0))


def test_script_writes_backbones_and_the_restraint_report(gpu, tmp_path):
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    from foldingdiff_amd.angles_and_coords import write_coords_to_pdb
    motif_pdb = write_coords_to_pdb(gr.build_ref(random_features(np.random.default_rng(4), 30, 6), IDX[6]), str(tmp_path / "motif.pdb"))
    contacts = tmp_path / "contacts.txt"
    contacts.write_text("# residue pairs\n0 35\n2 30 6.5\n")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_restrained.py"), "-m", mdir, "-o", out, "-n", "3", "-l", "36",
                        "--num_steps", "5", "--seed", "3", "--contacts", str(contacts), "--motif_pdb", motif_pdb, "--motif_residues", "3-6,20-22",
                        "--placed_at", "8,25", "--scale", "1.0", "--max_norm", "1.0", "--guide_from", "15"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "restraints.json", "sampled_angles", "sampled_pdb"]
    names = [f"generated_{i}.pdb" for i in range(3)]
    assert sorted(os.listdir(os.path.join(out, "sampled_pdb"))) == names
    assert sorted(os.listdir(os.path.join(out, "sampled_angles"))) == [f"generated_{i}.csv.gz" for i in range(3)]
    with open(os.path.join(out, "restraints.json")) as fh:
        report = json.load(fh)
    assert report["length"] == 36 and report["n_restraints"] == 2 + 21
    for key in ("energy", "max_violation", "motif_ca_rmsd"):
        assert sorted(report[key]) == names and all(np.isfinite(v) and v >= 0 for v in report[key].values()), key
    bad = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_restrained.py"), "-m", mdir, "-o", out, "-l", "30", "--contacts", str(contacts)],
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "the restraints need 36 residues" in bad.stderr        # a usage error before the model is loaded
