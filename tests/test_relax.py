"""Relaxation in torsion space without a device: the reference statement (tests/relax_reference.py) against torch autograd and
against oracle/ref_nerf, its chaining, the rejections of the three entries (checked on the host before any device call), the
compiler's metadata of the new kernels, and a check that the device test's chains are worth relaxing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import guide_reference as gr
import relax_reference as rx
from conftest import REPO
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from test_guide import DOMAIN_MODES, domain_features, reparametrise

IDX = {3: np.array([0, 1, 2, -1, -1, -1, -1, -1, -1], np.int32), 6: np.array([0, 1, 2, 3, 4, 5, -1, -1, -1], np.int32),
       9: np.arange(9, dtype=np.int32)}
RST_W = 0.5


def random_features(rng, n, F) -> np.ndarray:
    """float32 [n, F]: torsions anywhere on the circle, bond angles and lengths near a backbone's (as tests/test_guide.py)."""
    cols = [rng.uniform(-np.pi, np.pi, n) for _ in range(3)]
    cols += [m + 0.1 * rng.standard_normal(n) for m in (1.94, 2.03, 2.12)]
    cols += [m + 0.03 * rng.standard_normal(n) for m in (1.33, 1.46, 1.52)]
    return np.stack(cols[:F], axis=1).astype(np.float32)


def energy_case(n, F, seed):
    """A chain with clash, restraints and tether all active: a wide margin (so that even two residues overlap), restraints
    from atom 0 to the last atoms at distances the chain does not have, an anchor a little off the input."""
    rng = np.random.default_rng(seed)
    x = random_features(rng, n, F)
    anchor = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    last = 3 * n - 1
    rst = ([0, 1], [last, last - 1], [1.0, 30.0], [0.1, 0.5], [RST_W, 1.0])
    prm = rx.Params(IDX[F], [True] * 6 + [False] * 3, [f in set(IDX[F][IDX[F] >= 0].tolist()) for f in range(F)], alpha=0.63, margin=1.5,
                    w_clash=0.7, w_tether=0.3)
    fixed = np.zeros(n, dtype=bool)
    if n >= 3:
        fixed[1] = True
    return x, anchor, rst, prm, fixed


def autograd_energy(x32, anchor, rst, prm, fixed, F):
    """(coordinates of the float64 restatement, energies, masked gradient) by torch autograd."""
    feats = torch.tensor(np.asarray(x32, dtype=np.float32).astype(np.float64), requires_grad=True)
    xyz = gr.build_torch(feats, prm.feat_idx, False)
    n = xyz.shape[0]
    idx = torch.arange(n)
    r = torch.tensor(rx.RADII)[idx % 3]
    d = torch.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(dim=2) + torch.eye(n, dtype=torch.float64))
    pair = (idx[None, :] - idx[:, None]) >= 2
    v = torch.clamp(prm.alpha * (r[:, None] + r[None, :]) + prm.margin - d, min=0.0)
    e_clash = prm.w_clash * (v[pair] ** 2).sum()
    e_rst = torch.zeros((), dtype=torch.float64)
    for i, j, d0, tol, w in zip(*rst):
        dist = torch.linalg.norm(xyz[i] - xyz[j])
        e_rst = e_rst + w * torch.clamp(torch.abs(dist - d0) - tol, min=0.0) ** 2
    delta = feats - torch.tensor(np.asarray(anchor, dtype=np.float32).astype(np.float64))
    ang = torch.tensor(np.asarray(prm.is_angle, dtype=bool)[:F])
    delta = torch.where(ang[None, :], delta - 2.0 * np.pi * torch.floor((delta + np.pi) / (2.0 * np.pi)), delta)
    move = torch.tensor(np.asarray(prm.move, dtype=bool)[:F])
    e_tether = prm.w_tether * (delta[:, move] ** 2).sum()
    (e_clash + e_rst + e_tether).backward()
    G = feats.grad.numpy().copy()
    G[:, ~move.numpy()] = 0.0
    G[fixed] = 0.0
    return xyz.detach().numpy(), np.array([e_clash.item(), e_rst.item(), e_tether.item()]), G


# ---------------------------------------------------------------------------------- 1. the gradient against autograd
@pytest.mark.parametrize("F", [3, 6, 9])
def test_energy_gradient_agrees_with_autograd(F):
    """Clash, restraints and tether all active.  As tests/test_guide.py: on ref_nerf.build's coordinates (float32 products
    inside) within 1e-5 of the largest entry, on the float64 restatement's own within 1e-12."""
    for n in (2, 3, 7, 40):
        x, anchor, rst, prm, fixed = energy_case(n, F, 100 * F + n)
        xyz64, e_want, g_want = autograd_energy(x, anchor, rst, prm, fixed, F)
        assert (e_want > 0).all(), (n, e_want)                              # every term is active
        scale = np.abs(g_want).max()
        e_ref, g_ref, gn_ref, _ = rx.relax_energy(x, anchor, prm, fixed, rst, coords=gr.build_ref(x, IDX[F]))
        e_own, g_own, gn_own, _ = rx.relax_energy(x, anchor, prm, fixed, rst, coords=xyz64)
        on_ref, on_own = np.abs(g_ref - g_want).max() / scale, np.abs(g_own - g_want).max() / scale
        print(f"F={F} len={n}: {on_ref:.2e} on ref_nerf's coordinates, {on_own:.2e} on the restatement's; E = {e_want}")
        assert on_ref <= 1e-5 and on_own <= 1e-12
        assert np.allclose(e_own, e_want, rtol=1e-12, atol=0) and gn_own == np.sqrt((g_own * g_own).sum())
        assert (g_own[fixed] == 0).all() and (g_own[:, ~np.asarray(prm.move)[:F]] == 0).all()
    # no anchor: the tether costs nothing and adds nothing
    e0, g0, _, _ = rx.relax_energy(x, None, prm, fixed, rst)
    e1, g1, _, _ = rx.relax_energy(x, None, prm._replace(w_tether=0.0), fixed, rst)
    assert e0[2] == 0 and np.array_equal(g0, g1)


@pytest.mark.parametrize("F", [3, 6, 9])
def test_energy_gradient_agrees_with_autograd_on_the_whole_domain(F):
    """The same check on tests/test_guide.py's domain_features: bond angles of either sign on both sides of pi / 2, lengths of
    either sign.  The same gates.  (Not every term need be active here: chains with obtuse and acute angles do not always clash.)"""
    for n in (2, 3, 7, 40):
        for m, mode in enumerate(DOMAIN_MODES):
            x, anchor, rst, prm, fixed = energy_case(n, F, 100 * F + n)
            rng = np.random.default_rng(7000 * m + 100 * F + n)
            x = domain_features(rng, n, F, mode)
            anchor = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
            xyz64, e_want, g_want = autograd_energy(x, anchor, rst, prm, fixed, F)
            scale = np.abs(g_want).max()
            e_ref, g_ref, _, _ = rx.relax_energy(x, anchor, prm, fixed, rst, coords=gr.build_ref(x, IDX[F]))
            e_own, g_own, gn_own, _ = rx.relax_energy(x, anchor, prm, fixed, rst, coords=xyz64)
            _, g_unsigned, _, _ = rx.relax_energy(x, anchor, prm, fixed, rst, coords=xyz64, signs=False)
            on_ref, on_own = np.abs(g_ref - g_want).max() / scale, np.abs(g_own - g_want).max() / scale
            unsigned = np.abs(g_unsigned - g_want).max() / scale
            print(f"F={F} len={n} {mode}: {on_ref:.2e} on ref_nerf's coordinates, {on_own:.2e} on the restatement's, {unsigned:.2e} without "
                  f"the rows; E = {e_want}")
            assert e_want[1] > 0 and e_want[2] > 0
            assert on_ref <= 1e-5 and on_own <= 1e-12
            assert np.allclose(e_own, e_want, rtol=1e-12, atol=0) and gn_own == np.sqrt((g_own * g_own).sum())
            if F > 3 and mode != "backbone" and n >= 7:
                assert unsigned > 0.1


NEGATED_CHAINS = ((7, 0), (12, 1), (40, 2), (86, 3))     # (residues, seed)
NEGATED_ITERS = 10


def negated_angle_case(n, seed):
    """energy_case's restraints on a backbone-like chain of six features whose every bond angle is negated and its torsion
    moved by pi (the same chain): only the three bond-angle columns move, restraints only (w_clash = 0), no tether."""
    x = reparametrise(random_features(np.random.default_rng(seed), n, 6), np.ones(n, dtype=bool))
    last = 3 * n - 1
    rst = ([0, 1], [last, last - 1], [1.0, 30.0], [0.1, 0.5], [RST_W, 1.0])
    prm = rx.Params(IDX[6], [True] * 6, [False] * 3 + [True] * 3, w_clash=0.0, w_tether=0.0)
    return x, rst, prm


@pytest.mark.parametrize("n,seed", NEGATED_CHAINS)
def test_only_the_signed_gradient_descends_on_negated_bond_angles(n, seed):
    """The chains of tests/test_relax_gpu.py's descent on negated bond angles: within 10 iterations the statement accepts at
    least one step and ends below its start; with every sign taken as +1 (the derivative from the coordinates alone) the
    bond-angle gradient points uphill, every trial rises and nothing is accepted."""
    x, rst, prm = negated_angle_case(n, seed)
    assert (x[:, 3:] < 0).all()
    _, _, trace, accepted, _ = rx.relax(x, None, prm, NEGATED_ITERS, rst=rst)
    _, _, trace_u, accepted_u, h_u = rx.relax(x, None, prm, NEGATED_ITERS, rst=rst, signs=False)
    print(f"{n} residues (seed {seed}): E {trace[0]:.4f} -> {trace[-1]:.4f}, {accepted} accepted; without the signs {accepted_u} accepted")
    assert accepted >= 1 and trace[-1] < trace[0]
    assert accepted_u == 0 and trace_u[-1] == trace_u[0] and h_u == prm.step0 * prm.shrink ** NEGATED_ITERS


# ---------------------------------------------------------------------------------- 2. the scan against the oracle
@pytest.mark.parametrize("F", [3, 6, 9])
def test_composed_frames_agree_with_the_oracle(F):
    """Carrying the frame instead of recomputing it from three positions moves an atom by at most 1e-9 of the chain's extent
    (6144 products x 1.1e-16 x a few roundings each is 1e-11 relative at 2048 residues; measured here: below 1e-13 of it)."""
    worst = 0.0
    for n in (1, 2, 3, 7, 85, 86, 128):
        ang = random_features(np.random.default_rng(10 * n + F), n, F)
        for center in (False, True):
            want = gr.build_ref(ang, IDX[F])
            gate = rx.scan_gate(want)
            if center:
                want = want - want.mean(axis=0)
            err = np.abs(rx.nerf_scan(ang, IDX[F], center) - want).max()
            worst = max(worst, err / gate * 1e-9)
            assert err <= gate, (n, center, err, gate)
    print(f"F={F}: largest error {worst:.2e} of the chain's extent")


# ---------------------------------------------------------------------------------- 3. chaining
def test_the_descent_chained_one_iteration_at_a_time_is_the_descent():
    x, _, _, prm, fixed = energy_case(12, 3, 7)
    prm = prm._replace(margin=0.6, w_tether=0.05)
    rst = ([1, 4], [34, 28], [4.0, 25.0], [0.0, 1.0], [1.0, 0.2])
    whole, e_whole, trace, acc, h = rx.relax(x, None, prm, 8, fixed, rst)
    assert acc >= 2 and trace[-1] < trace[0] and (np.diff(trace) <= 0).all()
    cur, step, n_acc, energies = x, None, 0, [trace[0]]
    for _ in range(8):
        cur, e3, tr, a, step = rx.relax(cur, x, prm, 1, fixed, rst, h=step)
        n_acc += a
        energies.append(tr[-1])
    assert np.array_equal(cur.view(np.uint32), whole.view(np.uint32)) and np.array_equal(e3, e_whole)
    assert n_acc == acc and step == h and np.array_equal(np.array(energies), trace)
    assert np.array_equal(cur[fixed].view(np.uint32), x[fixed].view(np.uint32))   # a fixed row keeps its bits
    same, e_same, tr0, a0, _ = rx.relax(x, None, prm, 0, fixed, rst)              # n_iter = 0: the input and its energy
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32)) and a0 == 0 and len(tr0) == 1


# ---------------------------------------------------------------------------------- 4. the rejections
def test_relax_entries_reject_bad_arguments_before_touching_a_device(lib):
    """fd_nerf_scan, fd_relax_energy and fd_relax: every rejection of include/fdmi.h returns -1 with its word in fd_last_error()
    and leaves the outputs alone, on a machine without a GPU too.  No valid call is made."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    f64 = lambda *v: np.array(v, np.float64)                            # noqa: E731
    B, L, F = 2, 6, 6
    lens, idx = i32(4, 6), IDX[6]
    x = np.random.default_rng(2).standard_normal((B, L, F)).astype(np.float32)
    nan_x = x.copy()
    nan_x[0, 3, 5] = np.nan
    pad_nan = x.copy()
    pad_nan[0, 4:] = np.nan                                              # beyond chain 0's length: not looked at
    rst = dict(offs=i32(0, 1, 3), ri=i32(1, 4, 0), rj=i32(10, 16, 17), d0=f64(5, 6, 7), tol=f64(0, 1, 0), w=f64(1, 0, 2))
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    def scan(feats=x, lens=lens, B=B, F=F, idx=idx, out="default"):
        out = np.full((2, 3 * L, 3), -7.0) if isinstance(out, str) else out
        return [out], lib.fd_nerf_scan(0, P(feats), P(lens), B, L, F, P(idx), 1, P(out))

    for kw, word in [(dict(feats=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=0), b"B=0"), (dict(F=2), b"F=2"), (dict(idx=i32(6, 1, 2, 3, 4, 5, -1, -1, -1)), b"feat_idx[0]=6"),
                     (dict(idx=i32(0, -1, 2, 3, 4, 5, -1, -1, -1)), b"feat_idx[1]=-1"), (dict(lens=i32(4, 0)), b"lens[1]=0"),
                     (dict(lens=i32(4, 7)), b"outside [1, 6]")]:
        expect(word, *scan(**kw))

    def params(idx=idx, move=(1, 1, 1, 0, 0, 0), **kw):
        p = _binding.FdRelaxParams()
        for k in range(9):
            p.feat_idx[k] = int(idx[k])
        for f in range(F):
            p.is_angle[f], p.move[f] = 1, move[f]
        vals = dict(dict(clash_alpha=0.63, clash_margin=0.15, w_clash=1.0, w_tether=0.0, step0=0.01, grow=1.2, shrink=0.5, max_step=0.5), **kw)
        for k, v in vals.items():
            setattr(p, k, v)
        return p

    shape_cases = [(dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"), (dict(B=0), b"B=0"),
                   (dict(F=2), b"F=2 outside [3, 16]"), (dict(F=17), b"F=17 outside [3, 16]"),
                   (dict(prm=params(idx=i32(0, 1, 6, 3, 4, 5, -1, -1, -1))), b"feat_idx[2]=6"),
                   (dict(prm=params(idx=i32(0, -1, 2, 3, 4, 5, -1, -1, -1))), b"feat_idx[1]=-1"),
                   (dict(prm=params(idx=i32(0, 1, 2, 3, 4, 5, -2, -1, -1))), b"feat_idx[6]=-2"),
                   (dict(prm=params(idx=i32(0, 1, 2, 3, 3, 5, -1, -1, -1))), b"feat_idx[4]=3 repeats")]
    rst_cases = [(dict(offs=None), b"rst_offsets"), (dict(offs=i32(1, 1, 3)), b"rst_offsets[0]=1"), (dict(offs=i32(0, 2, 1)), b"rst_offsets[2]=1 is below"),
                 (dict(ri=None), b"restraint lists"), (dict(ri=i32(12, 4, 0)), b"restraint 0 = atoms (12, 10) outside chain 0's [0, 12)"),
                 (dict(rj=i32(10, 4, 17)), b"restraint 1 names atom 4 twice"), (dict(d0=f64(5, -1, 7)), b"restraint 1: d0"),
                 (dict(tol=f64(np.nan, 1, 0)), b"restraint 0: tol"), (dict(w=f64(1, np.inf, 2)), b"restraint 1: w")]
    param_cases = [(dict(prm=None), b"null"), (dict(prm=params(move=(1, 1, 1, 0, 0, 1), idx=i32(0, 1, 2, 3, 4, -1, -1, -1, -1))), b"move[5]"),
                   (dict(prm=params(clash_alpha=-0.1)), b"clash_alpha"), (dict(prm=params(clash_alpha=np.inf)), b"clash_alpha"),
                   (dict(prm=params(clash_margin=np.nan)), b"clash_margin"), (dict(prm=params(clash_margin=-1.0)), b"clash_margin"),
                   (dict(prm=params(w_clash=-1.0)), b"w_clash"), (dict(prm=params(w_tether=np.inf)), b"w_tether"),
                   (dict(prm=params(step0=0.0)), b"step0"), (dict(prm=params(step0=np.nan)), b"step0"), (dict(prm=params(grow=0.99)), b"grow"),
                   (dict(prm=params(shrink=0.0)), b"shrink"), (dict(prm=params(shrink=1.0)), b"shrink"), (dict(prm=params(max_step=0.0)), b"max_step"),
                   (dict(prm=params(max_step=-1.0)), b"max_step"),
                   (dict(feats=nan_x), b"feats is not finite at sequence 0, position 3"), (dict(anchor=nan_x), b"anchor is not finite")]

    def energy(feats=x, anchor=x, lens=lens, B=B, F=F, prm="default", e="default", gn="default", **r):
        a = dict(rst, **r)
        prm = params() if isinstance(prm, str) else prm
        e = np.full((2, 3), -7.0) if isinstance(e, str) else e
        gn = np.full(2, -7.0) if isinstance(gn, str) else gn
        grad = np.full((2, L, 16), -7.0)
        return [e, gn, grad], lib.fd_relax_energy(0, P(feats), P(anchor), P(lens), B, L, F, None if prm is None else C.byref(prm), None,
                                                  P(a["offs"]), P(a["ri"]), P(a["rj"]), P(a["d0"]), P(a["tol"]), P(a["w"]), P(e), P(gn), P(grad))

    for kw, word in [(dict(feats=None), b"null"), (dict(lens=None), b"null"), (dict(e=None), b"null"), (dict(gn=None), b"null")] \
            + shape_cases + rst_cases + param_cases:
        expect(word, *energy(**kw))
    assert energy(feats=pad_nan, lens=i32(4, 0))[1] == -1 and b"lens" in lib.fd_last_error()   # (a length error, not the padding's NaN)

    def relax(feats=x, anchor=None, lens=lens, B=B, F=F, prm="default", n_iter=3, step="default", out="default", e="default", acc="default", **r):
        a = dict(rst, **r)
        prm = params() if isinstance(prm, str) else prm
        out = np.full((2, L, 16), -7, np.float32) if isinstance(out, str) else out
        e = np.full((2, 3), -7.0) if isinstance(e, str) else e
        acc = np.full(2, -7, np.int32) if isinstance(acc, str) else acc
        trace = np.full((4, 2), -7.0)
        step = None if isinstance(step, str) else step
        return [out, e, acc, trace], lib.fd_relax(0, P(feats), P(anchor), P(lens), B, L, F, None if prm is None else C.byref(prm), None,
                                                  P(a["offs"]), P(a["ri"]), P(a["rj"]), P(a["d0"]), P(a["tol"]), P(a["w"]), n_iter, P(step),
                                                  P(out), P(e), P(trace), P(acc))

    for kw, word in [(dict(feats=None), b"null"), (dict(lens=None), b"null"), (dict(out=None), b"null"), (dict(e=None), b"null"),
                     (dict(acc=None), b"null"), (dict(n_iter=-1), b"n_iter=-1"), (dict(step=f64(0.01, 0.0)), b"step_io[1]"),
                     (dict(step=f64(np.nan, 0.01)), b"step_io[0]")] + shape_cases + rst_cases + param_cases:
        expect(word, *relax(**kw))
    assert checked == 10 + (4 + 9 + 9 + 17) + (8 + 9 + 9 + 17)


def test_abi_version_stays_seven(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert "#define FDMI_ABI_VERSION 7" in header and lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7
    for name in ("fd_nerf_scan", "fd_relax_energy", "fd_relax"):
        assert hasattr(lib, name) and re.search(rf"\bint {name}\(", header)
    assert C.sizeof(_binding.FdRelaxParams) == 9 * 4 + 16 + 16 + 4 + 8 * 8       # (4 bytes of padding in front of the doubles)


# ---------------------------------------------------------------------------------- 5. the compiler's metadata
@pytest.mark.parametrize("source,kernels", [("nerf_scan", ["nerf_scan_kernel"]), ("relax", ["soft_clash_kernel", "relax_step_kernel"])])
def test_the_new_kernels_use_no_scratch(source, kernels, tmp_path):
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    out = tmp_path / f"{source}.s"
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S", "--cuda-device-only",
           "-o", str(out), os.path.join(fbuild.CSRC, f"{source}.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    found = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).)*\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S):
        found[m.group(2)] = dict({k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(3))}, group_segment_fixed_size=int(m.group(1)))
    for kernel in kernels:
        md = [v for k, v in found.items() if kernel in k]
        assert len(md) == 1, (kernel, sorted(found))
        assert md[0]["private_segment_fixed_size"] == 0 and md[0]["vgpr_spill_count"] == 0, (kernel, md[0])
        assert md[0]["group_segment_fixed_size"] < 64 * 1024, (kernel, md[0])


# ---------------------------------------------------------------------------------- 6. the device test's inputs are not vacuous
def test_the_device_tests_chains_start_clashing_and_the_statement_clears_them():
    """The six chains of tests/test_relax_gpu.py (torsions only; margin 0.15, weight 1, step0 0.01, grow 1.2, shrink 0.5,
    max_step 0.5): every one starts with three or more clashing atoms, and within the 60 iterations the device test runs the
    statement brings each to E_clash == 0 and zero clashing atoms, with a trace that never rises."""
    prm = rx.Params(rx.IDX3, [True] * 3, [True] * 3)
    chains = rx.device_chains()
    assert [len(c) for c in chains] == [12, 40, 40, 64, 86, 128]
    start = [rx.count_clashes(rx.nerf_scan(c, rx.IDX3)) for c in chains]
    assert sum(s >= 3 for s in start) * 2 >= len(chains), start
    for (kind, n, seed), x, s in zip(rx.DEVICE_CHAINS, chains, start):
        out, e3, trace, accepted, _ = rx.relax(x, None, prm, 60)
        end = rx.count_clashes(rx.nerf_scan(out, rx.IDX3))
        moved = np.abs(rx.wrap64(out.astype(np.float64) - x.astype(np.float64))).max()
        print(f"{kind} {n} (seed {seed}): {s} -> {end} clashing atoms, E {trace[0]:.3f} -> {trace[-1]:.3g}, at 0 from iteration "
              f"{int(np.argmax(trace == 0))}, {accepted} accepted, largest angle change {moved:.3f} rad")
        assert e3[0] == 0 and end == 0 and (np.diff(trace) <= 0).all() and trace[0] > 0
