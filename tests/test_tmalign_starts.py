"""The three further starts of the alignment search on the host: the conditions the all-starts parity set has to meet
(asserted by the numpy restatement alone, tests/tmalign_starts_reference.py), the fragment-position rule, the interface
of fd_tm_align_ex (header, binding, exported symbol, argument checks without a device, the Python ValueErrors, the
scripts' --starts) and a static guard on tm_starts_kernel's registers.  No GPU needed."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import psea_reference as pr
import tm_reference as tr
import tmalign_reference as ta
import tmalign_starts_reference as ts
from conftest import REPO
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import structures

BITS = {"THREADING": 1, "SSE": 2, "SSE_DIST": 4, "LOCAL": 8, "FRAGMENT": 16}


def test_parity_set_is_decided_and_the_new_starts_matter():
    """Conditions on the inputs of the GPU parity test: every decision margin and every P-SEA threshold margin is
    >= 1e-9; all starts never score below two; start 3 or 4 is strictly better than starts 1 and 2 on at least 3 pairs
    and start 5 on at least 1; start_tms is -1 exactly where a start is skipped; the set has the agreed shape."""
    cases, res, two = ts.parity_set(), ts.parity_results(), ts.parity_results_two()
    kinds = {c[0] for c in cases}
    assert {"deletion", "insertion", "hinge", "unrelated", "rehinged", "core", "break_x", "break_y", "break_both", "short",
            "unbroken"} == kinds
    assert 28 <= len(cases) <= 32
    small = cases[:-1]
    assert min(min(len(a), len(b)) for _, a, b, _, _ in small) < 12
    assert max(max(len(a), len(b)) for _, a, b, _, _ in small) <= 136
    assert (len(cases[-1][1]), len(cases[-1][2]), cases[-1][4]) == (300, 200, 2)
    worst = min(r["margin"] for r in res)
    print(f"all-starts parity set: {len(cases)} pairs, smallest decision margin {worst:.3e}, "
          f"at most {max(r['programmes'] for r in res)} programmes in start 4")
    n34 = n5 = 0
    for (kind, a, b, _, _), r, w in zip(cases, res, two):
        where = (kind, len(a), len(b))
        assert r["margin"] >= 1e-9 and w["margin"] >= 1e-9, (where, r["margin"], w["margin"])
        assert pr.threshold_margin(a) >= 1e-9 and pr.threshold_margin(b) >= 1e-9, where
        assert r["tm"] >= w["tm"], where
        assert r["programmes"] <= 128
        st = r["start_tms"]
        assert np.array_equal(w["start_tms"][:2], st[:2]) and (w["start_tms"][2:] == -1).all()
        assert r["tm"] == st.max() and (r["tm"] > w["tm"]) == (st[2:].max() > st[:2].max())
        broken = ts.longest_stretch(a)[2] or ts.longest_stretch(b)[2]
        assert (st[:3] >= 0).all() and (st[3] == -1) == (min(len(a), len(b)) < 12), (where, st)
        if not broken:
            assert st[4] == -1, (where, st)
        if kind.startswith("break"):
            assert st[4] >= 0, (where, st)
        if kind == "unbroken":
            assert not broken
        n34 += bool(max(st[2], st[3]) > max(st[0], st[1]))
        n5 += bool(st[4] > max(st[0], st[1]))
        m = r["map"][r["map"] >= 0]
        assert (np.diff(m) > 0).all() and r["n_ali"] == len(m) >= 1
    skipped4 = sum(r["start_tms"][3] == -1 for r in res)
    skipped5 = sum(r["start_tms"][4] == -1 for r in res)
    print(f"start 3 or 4 strictly better than starts 1-2: {n34} pairs; start 5: {n5} pairs; "
          f"start 4 skipped: {skipped4}; start 5 skipped: {skipped5}")
    assert n34 >= 3 and n5 >= 1
    assert skipped4 == 2 and skipped5 >= 2


def test_single_starts_and_selection():
    """A selection is searched in start order whatever order it is given in; one start alone gives that start's
    score; a selection of which no start applies to the pair gives TM -1 and an empty map."""
    k = [c[0] for c in ts.parity_set()].index("break_both")
    _, a, b, Ln, it = ts.parity_set()[k]
    full = ts.parity_results()[k]
    for bit, name in enumerate(ts.START_NAMES[2:], start=2):
        r = ts.tm_align(a, b, Ln=Ln, max_iter=it, starts=1 << bit)
        assert r["tm"] == full["start_tms"][bit] and (np.delete(r["start_tms"], bit) == -1).all()
    none = ts.tm_align(*ts.parity_set()[[c[0] for c in ts.parity_set()].index("short")][1:3], starts=("local",))
    assert none["tm"] == -1.0 and none["n_ali"] == 0 and (none["map"] == -1).all() and (none["start_tms"] == -1).all()
    assert ts.selection(("ss", "threading")) == ("threading", "ss") == ts.selection(3)
    assert ts.selection("all") == ts.START_NAMES == ts.selection(31)
    assert [structures.align_start_bits((n,)) for n in structures.ALIGN_STARTS] == [1, 2, 4, 8, 16]
    assert structures.ALIGN_STARTS == ts.START_NAMES
    assert structures.align_start_bits("all") == 31 and structures.align_start_bits() == 3


def test_fragment_positions_are_bounded():
    """At most 8 positions for every chain of up to 512 residues and every fragment length, the first at 0, every
    fragment inside the chain, no two overlapping."""
    for n in range(1, 513):
        for f in range(1, min(n, 100) + 1):
            pos = ts.fragment_positions(n, f)
            assert 1 <= len(pos) <= 8 and pos[0] == 0 and pos[-1] + f <= n
            assert all(q - p >= f for p, q in zip(pos, pos[1:]))
    for m in range(12, 513):
        fl = ts.fragment_lengths(m)
        assert 4 <= fl[0] <= 20 and len(fl) <= 2 and all(f <= 100 for f in fl) and fl == sorted(set(fl))


def test_longest_stretch():
    x = tr.ca_chain(np.random.default_rng(1), 20)
    assert ts.longest_stretch(x) == (0, 20, False)
    y = x.copy()
    y[7:] += 5.0     # the step 6 -> 7 grows by up to 5 sqrt(3) A
    y[15:] -= 9.0
    assert ts.steps(y)[6] >= 4.25 and ts.steps(y)[14] >= 4.25
    assert ts.longest_stretch(y) == (7, 8, True)        # 7 | 8 | 5 residues
    z = x.copy()
    z[10:] += 5.0
    assert ts.longest_stretch(z) == (0, 10, True)       # 10 | 10: the first of the longest
    assert ts.longest_stretch(x[:1]) == (0, 1, False)


def test_interface():
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"\bint\s+fd_tm_align_ex\s*\(", header)
    for name, bit in BITS.items():
        assert re.search(rf"#define\s+FDMI_ALIGN_START_{name}\s+{bit}u?\b", header), name
    assert re.search(r"#define\s+FDMI_ALIGN_STARTS_ALL\s+31u?\b", header)
    assert re.search(r"#define\s+FDMI_ABI_VERSION\s+7\b", header) and re.search(r"#define\s+FDMI_ALIGN_MAX_LEN\s+512\b", header)
    assert "fd_tm_align_ex" in _binding.exported_symbols()
    sig = _binding._SIGNATURES["fd_tm_align_ex"][1]
    assert len(sig) == 17 and sig[:15] == _binding._SIGNATURES["fd_tm_align"][1] and sig[15] is C.c_uint32
    assert "tm_align_starts.hip" in fbuild.SOURCES and "tm_align.hip" in fbuild.SOURCES
    for fn in (structures.tm_align, structures.pairwise_tm, structures.max_tm_across_refs, structures.pairwise_tmscores,
               structures.training_tm_scores):
        assert inspect.signature(fn).parameters["starts"].default == ("threading", "ss"), fn.__name__
    assert inspect.signature(structures.tm_align).parameters["return_start_tms"].default is False


def test_library_exports_the_entry(lib):
    assert hasattr(lib, "fd_tm_align_ex")


def test_argument_errors_without_a_device(lib):
    """starts = 0 and starts = 32 are refused with "starts", and every null and shape error of fd_tm_align is refused
    in the same words, before any device call and with the outputs untouched.  No valid call is made."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    ca = np.random.default_rng(5).standard_normal((10, 3))
    offs, lens, pa, pb = i32(0, 4), i32(4, 6), i32(0, 1), i32(1, 0)
    bad_nan = ca.copy()
    bad_nan[7, 1] = np.nan

    def align(ca=ca, offs=offs, lens=lens, nc=2, pa=pa, pb=pb, norm=None, n=2, max_iter=3, out="default",
              moff=np.array([0, 4], np.int64), use_map=True, starts=31):
        tm = np.full(2, -7.0) if isinstance(out, str) else out
        T, n_ali, amap, stm = np.full((2, 12), -7.0), np.full(2, -7, np.int32), np.full(10, -7, np.int32), np.full((2, 5), -7.0)
        rc = lib.fd_tm_align_ex(0, P(ca), P(offs), P(lens), nc, P(pa), P(pb), P(norm), n, max_iter, P(tm), P(T), P(n_ali),
                                P(moff), P(amap) if use_map else None, starts, P(stm))
        return rc, lib.fd_last_error(), [x for x in (tm, T, n_ali, amap, stm) if x is not None]

    for kw, word in [(dict(starts=0), b"starts"), (dict(starts=32), b"starts"), (dict(starts=63), b"starts"),
                     (dict(starts=1 << 31), b"starts"),
                     (dict(ca=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(pa=None), b"null"),
                     (dict(pb=None), b"null"), (dict(out=None), b"null"), (dict(use_map=False), b"null"), (dict(moff=None), b"null"),
                     (dict(n=0), b"n_pairs"), (dict(nc=0), b"n_chains"), (dict(max_iter=0), b"max_iter"),
                     (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(513, 4)), b"outside [1, 512]"),
                     (dict(offs=i32(0, 5)), b"offsets"), (dict(pa=i32(0, 2)), b"chain index"),
                     (dict(norm=i32(4, 3)), b"norm_lens"), (dict(moff=np.array([0, 5], np.int64)), b"map_offsets"),
                     (dict(ca=bad_nan), b"finite")]:
        rc, msg, outs = align(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert all((x == -7).all() for x in outs), kw


def test_python_value_errors():
    a, b = np.zeros((5, 3)), np.zeros((8, 3))
    for starts in (("threading", "nope"), "local_fit", (), [], ("ss", "ss"), ("threading", "ss", "threading")):
        for call in (lambda: structures.tm_align([a], [b], starts=starts),
                     lambda: structures.pairwise_tm([a, b], starts=starts),
                     lambda: structures.max_tm_across_refs([a], [b], starts=starts),
                     lambda: structures.pairwise_tmscores([], starts=starts),
                     lambda: structures.training_tm_scores([], [], starts=starts)):
            with pytest.raises(ValueError, match="starts"):
                call()
    # an empty call needs no device: the per-start array has its shape
    out = structures.tm_align([], [], starts="all", return_start_tms=True)
    assert out[0].shape == (0,) and out[1].shape == (0, 5)


@pytest.mark.parametrize("script", ["tmscore_training.py", "hclust_structures.py"])
def test_cli_starts_option(script):
    spec = importlib.util.spec_from_file_location(script[:-3] + "_cli", os.path.join(REPO, "bin", script))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--dirname", "d"] + (["--train", "t"] if "training" in script else [])
    parser = cli.build_parser()
    assert parser.parse_args(base).starts == "two"
    assert parser.parse_args(base + ["--starts", "all"]).starts == "all"
    assert structures.align_start_bits(cli.STARTS["two"]) == 3 and structures.align_start_bits(cli.STARTS["all"]) == 31
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--starts", "five"])


@pytest.fixture(scope="module")
def starts_asm(tmp_path_factory):
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    out = tmp_path_factory.mktemp("isa") / "tm_align_starts.s"
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
           "--cuda-device-only", "-o", str(out), os.path.join(fbuild.CSRC, "tm_align_starts.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_starts_kernel_holds_no_scratch_and_fits_its_occupancy(starts_asm):
    """tm_starts_kernel's budget from its metadata: no scratch, so nothing a lane holds is spilled to memory (the
    compiler parks a few VGPRs in AGPRs and scalar registers in vector lanes; neither touches memory), and VGPRs +
    AGPRs, each rounded up to the allocation granule of 8, within the 512 of a lane: one 256-lane workgroup per CU.
    Its static and dynamic LDS at 512 residues fit the 160 KiB opt-in."""
    blocks = [b for b in re.split(r"\n  - (?=\.\w+:)", starts_asm.split("amdhsa.kernels:")[1])
              if re.search(r"\.name:\s+_Z\S*tm_starts_kernel", b)]
    assert len(blocks) == 1, "tm_starts_kernel not found in the metadata"
    md = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", "\n    " + blocks[0], re.M)}
    regs = -(-md["vgpr_count"] // 8) * 8   # the metadata's vgpr_count is the whole allocation, AGPRs included
    print(f"tm_starts_kernel: {md['vgpr_count']} VGPRs and AGPRs, of them {md['agpr_count']} AGPRs, {md['sgpr_count']} SGPRs, "
          f"{md.get('vgpr_spill_count', 0)} VGPRs parked in AGPRs, {md['private_segment_fixed_size']} bytes of scratch, "
          f"{md['group_segment_fixed_size']} bytes of static LDS")
    assert md["private_segment_fixed_size"] == 0, md
    assert regs <= 512, md
    n = 512   # AlignLds(512, 6) of tm_align_common.h
    dp_end = n * 24 * 2 + 12 * 256 * 8 + n * 24 + 3 * (n + 4) * 8 + 3 * (n + 4) + n * (n // 4)
    dynamic = ((dp_end + 7) & ~7) + 6 * n * 2 + 2 * n
    assert dynamic + md["group_segment_fixed_size"] <= 160 * 1024
