"""Repeat proteins -- angle rows tied across units -- the parts that need no device: the header, the binding and the
library's exports, fd_tie_repeats' argument checks (every one made before the first HIP call), the numpy restatement's own
properties (tests/repeat_reference.py), the Python argument errors, the script's usage errors, the kernel's metadata, and the
symmetry statement itself on the CPU NeRF (oracle/ref_nerf.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repeat_reference as rr
from conftest import REPO
from foldingdiff_amd import _binding, datasets, sampling
from oracle import ref_nerf, ref_sampling

P = _binding.ptr
ENTRIES = ("fd_tie_repeats", "fd_sample_repeat")
i32 = lambda *v: np.array(v, np.int32)   # noqa: E731


def test_entries_are_declared_bound_and_exported(lib):
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _binding.exported_symbols() and hasattr(lib, name)
    assert lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7 and "#define FDMI_ABI_VERSION 7" in src
    from foldingdiff_amd import build
    assert "repeat_tie.hip" in build.SOURCES


def test_tie_repeats_rejects_bad_arguments_before_touching_a_device(lib):
    """Each bad call returns -1 with its word in fd_last_error() and leaves the output at its sentinel, on a machine without
    a GPU too.  No valid call is made."""
    x = np.zeros((2, 8, 6), np.float32)
    ang = np.ones(6, np.uint8)
    checked = 0

    def call(x=x, lens=i32(8, 6), tie=i32(0, 2, 4, 1, 2, 2), B=2, L=8, F=6, ang=ang, init=0, s=0.0, z=None, out="default"):
        out = np.full((2, 8, 6), -7, np.float32) if isinstance(out, str) else out
        rc = lib.fd_tie_repeats(0, P(x), P(lens), P(tie), B, L, F, P(ang), init, C.c_float(s), P(z), C.c_uint64(1), 3, C.c_int64(0), P(out))
        return out, rc

    for kw, word in [(dict(x=None), b"null"), (dict(lens=None), b"null"), (dict(tie=None), b"null"), (dict(ang=None), b"null"),
                     (dict(out=None), b"null"), (dict(B=0), b"bad argument"), (dict(L=0), b"bad argument"), (dict(F=0), b"bad argument"),
                     (dict(B=-1), b"bad argument"), (dict(lens=i32(8, 0)), b"lens"), (dict(lens=i32(9, 6)), b"lens"),
                     (dict(tie=i32(-1, 2, 4, 1, 2, 2)), b"tie"), (dict(tie=i32(0, 0, 4, 1, 2, 2)), b"tie"),
                     (dict(tie=i32(0, 2, 0, 1, 2, 2)), b"tie"), (dict(tie=i32(0, 2, 4, 1, 2, 3)), b"tie"),
                     (dict(tie=i32(1, 2, 4, 1, 2, 2)), b"tie"), (dict(tie=i32(0, 2, 4, 0, 2 ** 30, 4)), b"tie"),
                     (dict(s=float("inf")), b"finite"), (dict(s=float("nan")), b"finite"), (dict(s=float("nan"), init=1), b"finite")]:
        out, rc = call(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (kw, word, rc, msg)
        assert out is None or (out == -7).all(), (kw, msg)
        checked += 1
    assert checked == 20


# ---------------------------------------------------------------------------------- the restatement's own properties
def test_reference_means_across_the_seam_and_plainly_elsewhere():
    """Three copies of one row either side of +-pi: the angular column averages on the circle (within 0.02 of pi), the
    non-angular column takes the plain mean (which is nowhere near)."""
    vals = np.array([3.13, -3.14, 3.12], np.float32)
    x = np.zeros((1, 5, 2), np.float32)
    x[0, 1:4, 0] = vals
    x[0, 1:4, 1] = vals
    x[0, 0] = [0.5, 7.0]            # a free row: the angular column wrapped (0.5 stays), the plain one kept
    x[0, 4] = [-7.0, -7.0]          # beyond the length
    got = rr.tie(x, [4], [(1, 1, 3)], [True, False])
    assert ref_sampling.circ_dist(got[0, 1, 0], np.pi) < 0.02
    assert got[0, 1, 0] == got[0, 2, 0] == got[0, 3, 0] and got[0, 1, 1] == got[0, 2, 1] == got[0, 3, 1]
    d = np.float32(np.float32(vals[1] - vals[0]) + np.float32(vals[2] - vals[0]))
    assert got[0, 1, 1] == np.float32(vals[0] + np.float32(d / np.float32(3))) and abs(got[0, 1, 1] - vals.mean()) < 1e-6
    assert abs(got[0, 0, 0] - 0.5) < 1e-6 and got[0, 0, 1] == np.float32(7.0)
    assert (got[0, 4] == -7.0).all()


def test_reference_free_rows_padding_noise_and_init():
    rng = np.random.default_rng(2)
    lens, ties = [10, 7], [(2, 3, 2), (0, 1, 1)]
    x = rng.uniform(-3, 3, (2, 10, 4)).astype(np.float32)
    x[1, 7:] = -7.0
    z = rng.standard_normal((2, 10, 4)).astype(np.float32)
    ang = [True, True, False, False]
    s = np.float32(0.3)
    got = rr.tie(x, lens, ties, ang, s=s, z=z)
    assert np.array_equal(got[1, 7:], x[1, 7:])                                   # padding keeps its bits
    assert np.array_equal(got[0, 2:5], got[0, 5:8])                               # the copies are equal ...
    want_free = (x[0, [0, 1, 8, 9]] + (s * z[0, [0, 1, 8, 9]]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got[0, [0, 1, 8, 9], 2:], want_free[:, 2:])             # ... a free row is x + s z, its own draw
    assert (np.abs(got[..., :2][_valid2(lens, 10)]) <= np.float32(np.pi)).all()
    assert np.array_equal(got[1, :7, 2:], (x[1, :7, 2:] + (s * z[1, :7, 2:]).astype(np.float32)).astype(np.float32))   # units = 1: all free
    # the tied rows received the draw of the copy-0 position, not their own
    no_noise = rr.tie(x, lens, ties, ang)
    assert np.array_equal(got[0, 5:8, 2:], (no_noise[0, 2:5, 2:] + (s * z[0, 2:5, 2:]).astype(np.float32)).astype(np.float32))
    # s == 0: z is not looked at
    assert np.array_equal(rr.tie(x, lens, ties, ang, s=0.0, z=None), no_noise)
    # init: every copy is copy 0; free rows, padding and the untied sequence keep their bits (no wrap either)
    big = x.copy()
    big[0, 0, 0] = 9.0
    first = rr.tie(big, lens, ties, ang, init=True)
    assert np.array_equal(first[0, 5:8], big[0, 2:5]) and np.array_equal(first[0, 2:5], big[0, 2:5])
    assert np.array_equal(first[0, [0, 1, 8, 9]], big[0, [0, 1, 8, 9]]) and np.array_equal(first[1], big[1])
    # period 1: every row of the region equal
    one = rr.tie(x, [10, 7], [(0, 1, 10), (0, 1, 7)], ang)
    assert (one[0] == one[0, 0]).all() and (one[1, :7] == one[1, 0]).all()


def _valid2(lens, L):
    v = np.zeros((len(lens), L, 2), dtype=bool)
    for b, n in enumerate(lens):
        v[b, :n] = True
    return v


# ---------------------------------------------------------------------------------- Python and the script
def test_python_argument_errors_come_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_binding, "load", no_library)
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64), timesteps=20, beta_schedule="cosine")
    bad = [dict(period=8, units=4, start=1, lengths=[32, 40]),        # 1 + 32 > 32
           dict(period=8, units=8, lengths=[63]), dict(period=0, units=2), dict(period=4, units=0), dict(period=4, units=2, start=-1),
           dict(period=[4, 4, 4], units=2), dict(period=4, units=[2]), dict(period=4, units=2, start=[0, 1, 2]),
           dict(period=4, units=2, spacing="cosine"), dict(period=4, units=2, spacing="logsnr"),   # (logsnr needs num_steps)
           dict(period=4, units=2, lengths=[]), dict(period=4, units=2, lengths=[65])]
    for kw in bad:
        a = dict(lengths=[30, 31])
        a.update(kw)
        with pytest.raises(ValueError):
            sampling.sample_repeats(None, ds, **a)
    assert sampling.repeat_ties([30, 31], 4, [2, 7], start=[0, 3]).tolist() == [[0, 4, 2], [3, 4, 7]]
    assert sampling.repeat_ties([30], 30, 1).dtype == np.int32


def test_script_rejects_a_tie_that_does_not_fit(tmp_path):
    """Exit status 2 (a usage error) and nothing written: a tie that cannot exist without a model directory at all, one
    beyond the padded length with nothing but the directory's training_args.json."""
    import json
    script = os.path.join(REPO, "bin", "sample_repeats.py")
    mdir, out = tmp_path / "model", tmp_path / "out"
    os.makedirs(mdir)
    with open(mdir / "training_args.json", "w") as fh:
        json.dump({"max_seq_len": 64, "angles_definitions": "canonical-full-angles", "timesteps": 20, "variance_schedule": "cosine",
                   "variance_scale": 1.0}, fh)
    for argv in (["-m", str(tmp_path / "nowhere"), "--period", "0", "--units", "4"],
                 ["-m", str(tmp_path / "nowhere"), "--period", "8", "--units", "4", "--flank_n", "-1"],
                 ["-m", str(mdir), "--period", "8", "--units", "8", "--flank_c", "1"],
                 ["-m", str(mdir), "--period", "9", "--units", "8"]):
        r = subprocess.run([sys.executable, script, "-o", str(out), "-n", "2"] + argv, capture_output=True, text=True)
        assert r.returncode == 2, (argv, r.returncode, r.stderr[-500:])
        assert "usage:" in r.stderr and not os.path.exists(out)
    assert sorted(os.listdir(mdir)) == ["training_args.json"]


def test_kernel_holds_no_scratch():
    """repeat_tie.hip compiles for the device alone; the kernel keeps the Philox block and the running sum in registers:
    no private segment, no spill, no LDS."""
    from foldingdiff_amd import build as fbuild
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
                        "--cuda-device-only", "-o", "-", os.path.join(fbuild.CSRC, "repeat_tie.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"\.name:\s+_Z\S*repeat_tie_kernel\S*\n(.*?)\.wavefront_size", r.stdout, re.S)
    assert m, "repeat_tie_kernel's metadata not found"
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(1))}
    print("repeat_tie_kernel:", md)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    desc = re.search(r"\.amdhsa_kernel \S*repeat_tie_kernel\S*\n(.*?)\.end_amdhsa_kernel", r.stdout, re.S)
    assert desc and re.search(r"\.amdhsa_group_segment_fixed_size 0\n", desc.group(1)), "the kernel holds LDS"


# ---------------------------------------------------------------------------------- the symmetry statement
def _unit_rmsd(xyz, start, period, units, first=None):
    """Superposed RMSD (Kabsch, fp64) of the atoms of residues [first, start + (units - 1) period) onto the same range
    shifted by one period; first = start + 1 unless given (structures.repeat_rmsd's range)."""
    lo, hi = start + 1 if first is None else first, start + (units - 1) * period
    a, b = xyz[3 * lo: 3 * hi], xyz[3 * (lo + period): 3 * (hi + period)]
    a, b = a - a.mean(axis=0), b - b.mean(axis=0)
    u, _, vt = np.linalg.svd(a.T @ b)
    d = np.sign(np.linalg.det(u @ vt))
    rot = u @ np.diag([1.0, 1.0, d]) @ vt
    return float(np.sqrt(((a @ rot - b) ** 2).sum() / len(a)))


def test_periodic_angle_rows_give_screw_symmetry_on_the_cpu_nerf():
    """Period 7 x 4 units of random angles through oracle/ref_nerf.build: the units superpose to below 1e-9 A with residue 0
    left out; one angle moved by 0.05 rad costs more than 1e-2 A.  (Residue 0 counted costs about 2e-2: NeRF seeds it from
    fixed coordinates with the seed's own N-CA-C angle.)"""
    rng = np.random.default_rng(7)
    period, units = 7, 4
    unit = np.column_stack([rng.uniform(-np.pi, np.pi, (period, 3)), rng.uniform(1.8, 2.2, (period, 3))])
    rows = np.tile(unit, (units, 1))

    def build(r):
        return ref_nerf.build(r[:, 0], r[:, 1], r[:, 2], tau=r[:, 3], ca_c_n=r[:, 4], c_n_ca=r[:, 5], center=False)

    exact = _unit_rmsd(build(rows), 0, period, units)
    moved = rows.copy()
    moved[period + 3, 1] += 0.05
    off = _unit_rmsd(build(moved), 0, period, units)
    print(f"periodic rows: {exact:.3e} A; one angle off by 0.05 rad: {off:.3e} A")
    assert exact < 1e-9
    assert off > 1e-2
    counted = _unit_rmsd(build(rows), 0, period, units, first=0)
    print(f"residue 0 counted: {counted:.3e} A")
    assert counted > 1e-6
    # free flanks: the first tied residue takes its N-CA-C angle from the free row in front of it, as residue 0 takes the
    # seed's; left out, the units superpose as exactly, and counted it alone is worth more than the 1e-6 A the GPU tests allow
    flank = lambda n: np.column_stack([rng.uniform(-np.pi, np.pi, (n, 3)), rng.uniform(1.8, 2.2, (n, 3))])   # noqa: E731
    flanked = build(np.concatenate([flank(2), rows, flank(3)]))
    inner, with_first = _unit_rmsd(flanked, 2, period, units), _unit_rmsd(flanked, 2, period, units, first=2)
    print(f"two free rows in front: {inner:.3e} A; the first tied residue counted: {with_first:.3e} A")
    assert inner < 1e-9 and with_first > 1e-6
    # the tie statement makes such rows: noisy copies in, periodic rows out
    noisy = (rows + rng.normal(0, 0.02, rows.shape)).astype(np.float32)[None]
    tied = rr.tie(noisy, [period * units], [(0, period, units)], [True] * 3 + [False] * 3)[0].astype(np.float64)
    assert _unit_rmsd(build(noisy[0].astype(np.float64)), 0, period, units) > 1e-2
    assert _unit_rmsd(build(tied), 0, period, units) < 1e-9
