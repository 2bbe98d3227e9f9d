"""Clash counts and lDDT on the host: the numpy restatement (tests/clash_lddt_reference.py) against the reference's own
counts (tests/golden/ref_clashes.npz) and a hand-worked lDDT case; the C ABI's two entries and their argument checks,
which run before a device is touched; the Python argument checks of ``structures.count_clashes`` / ``structures.lddt``; a
static guard on the kernels.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clash_lddt_reference as cr
from conftest import GOLDEN, REPO, golden
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import structures

FD_E_INVALID, FD_E_UNSUPPORTED = -1, -5


def test_restatement_reproduces_the_reference_counts():
    """The reference's count_clashes gave these counts and flags (make_golden_clashes.py); 1CRN itself has no clash and
    its two shrunk copies clash in every atom."""
    g = golden("ref_clashes.npz")
    names = [str(n) for n in g["names"]]
    assert names == ["1CRN", "1CRN_x0.8", "1CRN_x0.6", "1CRN_jitter", "walk_22", "walk_342"]
    assert g["counts"][:3].tolist() == [0, 138, 138]
    for k, name in enumerate(names):
        xyz = g[f"xyz_{k}"]
        assert xyz.dtype == np.float32 and xyz.shape == (len(g[f"flags_{k}"]), 3)
        count, flags, margin = cr.clashes(xyz, float(g["alpha"]))
        print(name, count, margin)
        assert margin >= cr.MIN_MARGIN
        assert count == int(g["counts"][k]), name
        assert (flags == g[f"flags_{k}"]).all(), name
    crn = structures.read_backbone(os.path.join(GOLDEN, "1CRN.pdb"))[0]
    assert (g["xyz_0"] == crn).all()


def test_lddt_hand_case():
    """Reference CA atoms at x = 0, 10, 20, model at x = 0, 10.4, 23.  Pairs (0, 1) and (1, 2) are within 15 A in the
    reference and (0, 2) is not: total 2.  (0, 1) moves by 0.4 (inside all four thresholds), (1, 2) by 2.6 (inside 4
    only): conserved 5."""
    ref = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0]], np.float32)
    model = np.array([[0, 0, 0], [10.4, 0, 0], [23, 0, 0]], np.float32)
    (cons, total), per_res, margin = cr.lddt_counts(model, ref, atoms_per_res=1)
    assert (cons, total) == (5, 2) and margin >= cr.MIN_MARGIN
    assert cr.score(cons, total) == 0.625
    assert per_res.tolist() == [[4, 1], [5, 2], [1, 1]]
    assert [cr.score(c, t) for c, t in per_res] == [1.0, 0.625, 0.25]
    # one residue: no pair at all
    (cons, total), per_res, _ = cr.lddt_counts(model[:1], ref[:1], atoms_per_res=1)
    assert (cons, total) == (0, 0) and np.isnan(cr.score(cons, total)) and per_res.tolist() == [[0, 0]]


@pytest.mark.parametrize("A", [1, 3])
def test_lddt_of_a_model_equal_to_the_reference_or_rigidly_moved_is_one(A):
    rng = np.random.default_rng(3)
    ref = cr.walk_backbone(rng, 40)[: 40 * A]
    moved = (ref.astype(np.float64) @ cr.rotation(rng).T + rng.uniform(-50, 50, 3)).astype(np.float32)
    for model in (ref, moved):
        (cons, total), per_res, margin = cr.lddt_counts(model, ref, atoms_per_res=A)
        assert margin >= cr.MIN_MARGIN and total > 0
        assert cons == 4 * total and cr.score(cons, total) == 1.0
        assert (per_res[:, 0] == 4 * per_res[:, 1]).all()


def test_entries_are_declared_in_the_header():
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"^int fd_backbone_clashes\(int device_id, const float\* xyz,", src, re.M)
    assert re.search(r"^int fd_lddt\(int device_id, const float\* model, const float\* ref,", src, re.M)
    assert re.search(r"^#define FDMI_PAIRCOUNT_MAX_ATOMS 65536$", src, re.M)
    assert re.search(r"^#define FDMI_ABI_VERSION 7$", src, re.M)
    assert structures.PAIRCOUNT_MAX_ATOMS == 65536


def test_entries_are_bound():
    assert "fd_backbone_clashes" in _binding.exported_symbols()
    assert "fd_lddt" in _binding.exported_symbols()
    assert _binding.ABI_VERSION == 7


def test_entries_are_exported(lib):
    assert lib.fd_abi_version() == 7
    assert hasattr(lib, "fd_backbone_clashes") and hasattr(lib, "fd_lddt")


def test_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Every argument check returns its code with the offending index in fd_last_error() and leaves the outputs alone,
    on a machine without a GPU too.  No valid call is made.  Two structures of 4 and 6 residues."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    rng = np.random.default_rng(5)
    offs, lens = i32(0, 4), i32(4, 6)
    checked = 0

    def expect(code, word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == code and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    xyz = rng.standard_normal((30, 3)).astype(np.float32)   # 10 residues x (N, CA, C)
    bad_nan, bad_inf = xyz.copy(), xyz.copy()
    bad_nan[22, 1] = np.nan    # atom 22 is in chain 1 (atoms 12 .. 29)
    bad_inf[5, 2] = np.inf     # atom 5 is in chain 0
    long_xyz = np.zeros((21846 * 3, 3), np.float32)

    def clashes(xyz=xyz, offs=offs, lens=lens, n=2, alpha=0.63, counts="default"):
        counts = np.full(2, -7, np.int32) if isinstance(counts, str) else counts
        flags = np.full(30, 249, np.uint8)
        rc = lib.fd_backbone_clashes(0, P(xyz), P(offs), P(lens), n, alpha, P(counts), P(flags))
        assert (flags == 249).all()
        return [counts], rc

    for kw, code, word in [
            (dict(xyz=None), FD_E_INVALID, b"null"), (dict(offs=None), FD_E_INVALID, b"null"),
            (dict(lens=None), FD_E_INVALID, b"null"), (dict(counts=None), FD_E_INVALID, b"null"),
            (dict(n=0), FD_E_INVALID, b"n_chains=0"), (dict(n=-3), FD_E_INVALID, b"n_chains=-3"),
            (dict(alpha=0.0), FD_E_INVALID, b"alpha"), (dict(alpha=-0.63), FD_E_INVALID, b"alpha"),
            (dict(alpha=float("nan")), FD_E_INVALID, b"alpha"), (dict(alpha=float("inf")), FD_E_INVALID, b"alpha"),
            (dict(lens=i32(4, 0)), FD_E_INVALID, b"lens[1]=0"), (dict(offs=i32(0, 5)), FD_E_INVALID, b"offsets[1]=5"),
            (dict(offs=i32(1, 4)), FD_E_INVALID, b"offsets[0]=1"),
            (dict(xyz=bad_nan), FD_E_INVALID, b"atom 22 (chain 1) is not finite"),
            (dict(xyz=bad_inf), FD_E_INVALID, b"atom 5 (chain 0) is not finite"),
            (dict(xyz=long_xyz, offs=i32(0), lens=i32(21846), n=1), FD_E_UNSUPPORTED, b"lens[0]=21846: 65538 atoms")]:
        expect(code, word, *clashes(**kw))

    thr = np.array([0.5, 1.0, 2.0, 4.0])
    ca = rng.standard_normal((10, 3)).astype(np.float32)
    ca_nan = ca.copy()
    ca_nan[7, 0] = np.nan
    long_model = np.zeros((8193 * 8, 3), np.float32)

    def lddt(model=ca, ref=ca, offs=offs, lens=lens, n=2, A=1, radius=15.0, thr=thr, n_thr=4, counts="default"):
        counts = np.full((2, 2), -7, np.int64) if isinstance(counts, str) else counts
        res = np.full((10, 2), -7, np.int32)
        return [counts, res], lib.fd_lddt(0, P(model), P(ref), P(offs), P(lens), n, A, radius, P(thr), n_thr, P(counts), P(res))

    for kw, code, word in [
            (dict(model=None), FD_E_INVALID, b"null"), (dict(ref=None), FD_E_INVALID, b"null"),
            (dict(offs=None), FD_E_INVALID, b"null"), (dict(lens=None), FD_E_INVALID, b"null"),
            (dict(thr=None), FD_E_INVALID, b"null"), (dict(counts=None), FD_E_INVALID, b"null"),
            (dict(n=0), FD_E_INVALID, b"n_pairs=0"), (dict(A=0), FD_E_INVALID, b"atoms_per_res=0"),
            (dict(A=9), FD_E_INVALID, b"atoms_per_res=9"), (dict(radius=0.0), FD_E_INVALID, b"radius"),
            (dict(radius=float("nan")), FD_E_INVALID, b"radius"), (dict(radius=float("inf")), FD_E_INVALID, b"radius"),
            (dict(n_thr=0), FD_E_INVALID, b"n_thresholds=0"), (dict(n_thr=9), FD_E_INVALID, b"n_thresholds=9"),
            (dict(thr=np.array([0.5, 1.0, 0.0, 4.0])), FD_E_INVALID, b"thresholds[2]=0"),
            (dict(thr=np.array([0.5, float("nan"), 2.0, 4.0])), FD_E_INVALID, b"thresholds[1]"),
            (dict(thr=np.array([0.5, 1.0, 2.0, -4.0])), FD_E_INVALID, b"thresholds[3]=-4"),
            (dict(lens=i32(4, 0)), FD_E_INVALID, b"lens[1]=0"), (dict(offs=i32(0, 5)), FD_E_INVALID, b"offsets[1]=5"),
            (dict(model=ca_nan), FD_E_INVALID, b"atom 7 (chain 1) is not finite"),
            (dict(ref=ca_nan), FD_E_INVALID, b"atom 7 (chain 1) is not finite"),
            (dict(model=long_model, ref=long_model, offs=i32(0), lens=i32(8193), n=1, A=8), FD_E_UNSUPPORTED,
             b"lens[0]=8193: 65544 atoms")]:
        expect(code, word, *lddt(**kw))
    assert checked == 16 + 22


def test_wrappers_check_their_arguments_in_python():
    """Malformed input raises ValueError before the library is looked for; an empty call returns empty results."""
    ok3, ok1 = np.zeros((12, 3), np.float32), np.zeros((4, 3), np.float32)
    assert structures.count_clashes([]).shape == (0,)
    assert structures.count_clashes([], return_flags=True)[1] == []
    assert structures.lddt([], []).shape == (0,)
    assert structures.lddt([], [], per_residue=True)[1] == []
    for bad in (np.zeros((5, 2)), np.zeros((0, 3)), np.zeros((10, 3)), np.zeros(9), np.zeros((65538, 3))):
        with pytest.raises(ValueError):
            structures.count_clashes([ok3, bad])
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            structures.count_clashes([ok3], alpha=alpha)
    for kw in (dict(models=[ok3], refs=[ok3, ok3]), dict(models=[ok3], refs=[np.zeros((9, 3))]),
               dict(models=[np.zeros((10, 3))], refs=[np.zeros((10, 3))]), dict(models=[ok3], refs=[ok3], atoms_per_res=0),
               dict(models=[ok3], refs=[ok3], atoms_per_res=9), dict(models=[ok3], refs=[ok3], radius=0.0),
               dict(models=[ok3], refs=[ok3], radius=float("nan")), dict(models=[ok3], refs=[ok3], thresholds=()),
               dict(models=[ok3], refs=[ok3], thresholds=(1.0, 0.0)), dict(models=[ok3], refs=[ok3], thresholds=[1.0] * 9),
               dict(models=[np.zeros((4, 2))], refs=[ok1], atoms_per_res=1),
               dict(models=[np.zeros((65537, 3))], refs=[np.zeros((65537, 3))], atoms_per_res=1)):
        with pytest.raises(ValueError):
            structures.lddt(**kw)


def test_count_clashes_parallel_names_a_rejected_file(tmp_path):
    bad = tmp_path / "no_backbone.pdb"
    bad.write_text("REMARK nothing here\n")
    with pytest.raises(ValueError, match="no_backbone.pdb"):
        structures.count_clashes_parallel([str(bad)])


def test_kernels_hold_no_scratch():
    """clash_lddt.hip compiles for the device alone, and both kernels keep an atom's coordinates, limits and counters in
    registers: no private segment."""
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    assert "clash_lddt.hip" in fbuild.SOURCES
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
                        "--cuda-device-only", "-o", "-", os.path.join(fbuild.CSRC, "clash_lddt.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ("clash_kernel", "lddt_kernel"):
        m = re.search(r"\.name:\s+_Z\S*" + kernel + r"\S*\n(.*?)\.wavefront_size", r.stdout, re.S)
        assert m, f"{kernel}'s metadata not found"
        md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(1))}
        print(kernel, md)
        assert md["private_segment_fixed_size"] == 0, md
        assert md["vgpr_spill_count"] == 0, md
