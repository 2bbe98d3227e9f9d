"""The alignment search's definition on the host: properties of the numpy restatement (tests/tmalign_reference.py), the
decision margins of the parity set the GPU tests use, the interface (header, binding, Python argument checks), and a
static guard on the kernel's registers.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import psea_reference as pr
import tm_reference as tr
import tmalign_reference as ta
from conftest import REPO
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import structures


def test_search_stride():
    """The smallest stride with at most 256 seeds, the same number in the package and in the restatement."""
    for n in (1, 4, 5, 60, 64, 100, 128, 300, 512):
        s = ta.search_stride(n)
        assert s == structures.tm_align_stride(n)
        assert ta.seed_count(n, s) <= 256 and (s == 1 or ta.seed_count(n, s - 1) > 256)
    assert ta.search_stride(60) == 1 and ta.search_stride(128) > 1


def test_dp_rules():
    """Hand-checked dynamic programmes: the diagonal of an identity-like matrix, a gap where it pays, match before up
    before left on ties, and the gap penalty charged on opening only."""
    m, _ = ta.dp(np.eye(4), -0.6)
    assert m.tolist() == [0, 1, 2, 3]
    S = np.zeros((3, 4))
    S[0, 0] = S[1, 2] = S[2, 3] = 1.0   # one residue of y is skipped
    assert ta.dp(S, -0.6)[0].tolist() == [0, 2, 3]
    assert ta.dp(np.zeros((2, 2)), 0.0)[0].tolist() == [0, 1]       # all ties: match wins
    assert ta.dp(np.zeros((3, 1)), 0.0)[0].tolist() == [-1, -1, 0]  # cell (1, 1) a match, then up twice, then it
    S = np.zeros((2, 5))
    S[0, 0] = S[1, 4] = 1.0   # a gap of three costs one opening: 2 - 0.6 beats 1
    assert ta.dp(S, -0.6)[0].tolist() == [0, 4]


def test_threading_offsets():
    assert ta.threading_offsets(1, 1) == [0]
    assert ta.threading_offsets(3, 3) == [0]
    assert ta.threading_offsets(6, 6) == [-1, 0, 1]
    ks = ta.threading_offsets(20, 12)   # m = 12: overlaps of at least 6
    assert ks == list(range(-6, 15)) and all(min(20, 12 + k) - max(0, k) >= 6 for k in ks)


def test_self_alignment_scores_one():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 37):
        a = tr.ca_chain(rng, n)
        r = ta.tm_align(a, a @ tr.rotation(rng).T + 5.0)
        assert r["tm"] == pytest.approx(1.0, abs=1e-12)
        assert r["map"].tolist() == list(range(n)) and r["n_ali"] == n


@pytest.mark.parametrize("n", [20, 64, 100])
def test_deletion_scores_one(n):
    """b = a without n // 10 residues, rotated: TM = 1 (normalised by len(b)), every residue of b is aligned and the
    map skips exactly the deleted residues."""
    a, b, cut = ta.deletion_pair(np.random.default_rng(n), n)
    r = ta.tm_align(a, b)
    assert r["tm"] == pytest.approx(1.0, abs=1e-12)
    assert r["n_ali"] == len(b)
    kept = np.delete(np.arange(n), cut)
    want = np.full(n, -1)
    want[kept] = np.arange(len(b))
    assert r["map"].tolist() == want.tolist()
    assert np.abs(a[kept] @ r["R"].T + r["t"] - b).max() < 1e-8


@pytest.mark.parametrize("n,seed", [(64, 0), (100, 0)])
def test_hinge_with_deletion_finds_the_intact_domain(n, seed):
    """A noise-free hinged chain with a deletion in its first domain: at least the intact second domain's share."""
    a, b = ta.hinge_pair(np.random.default_rng(seed), n)
    r = ta.tm_align(a, b)
    assert r["tm"] >= (n // 2) / len(b)
    assert r["tm"] == pytest.approx(ta.tm_of_map(a, b, r["R"], r["t"], r["map"], len(b)), abs=1e-12)


def test_parity_set_is_decided():
    """Every pair of the parity set is far from every decision the search takes (margin >= 1e-9) and from every P-SEA
    threshold, so a kernel that differs by rounding takes the same path; the set has the agreed shape."""
    cases, results = ta.parity_set(), ta.parity_results()
    assert len(cases) == 41
    assert {c[0] for c in cases} == {"deletion", "insertion", "hinge", "unrelated"}
    small = cases[:-1]
    assert min(min(len(a), len(b)) for _, a, b, _, _ in small) == 5
    assert max(max(len(a), len(b)) for _, a, b, _, _ in small) <= 136
    assert (len(cases[-1][1]), len(cases[-1][2]), cases[-1][4]) == (512, 300, 2)
    worst = min(r["margin"] for r in results)
    print(f"parity set: smallest decision margin {worst:.3e}")
    for (kind, a, b, _, _), r in zip(cases, results):
        assert r["margin"] >= 1e-9, (kind, len(a), len(b), r["margin"])
        assert pr.threshold_margin(a) >= 1e-9 and pr.threshold_margin(b) >= 1e-9
        m = r["map"][r["map"] >= 0]
        assert (np.diff(m) > 0).all() and r["n_ali"] == len(m) >= 1
    assert sum(r["start_tms"][1] > r["start_tms"][0] for r in results) >= 4   # the second start earns its keep


def test_interface():
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"#define\s+FDMI_ALIGN_MAX_LEN\s+512\b", header)
    assert re.search(r"\bint\s+fd_tm_align\s*\(", header)
    assert re.search(r"#define\s+FDMI_ABI_VERSION\s+7\b", header)
    assert "fd_tm_align" in _binding.exported_symbols()
    assert len(_binding._SIGNATURES["fd_tm_align"][1]) == 15
    assert _binding.ABI_VERSION == 7
    assert structures.ALIGN_MAX_LEN == 512


def test_argument_errors_are_raised_in_python():
    a, b = np.zeros((5, 3)), np.zeros((8, 3))
    for call in (lambda: structures.tm_align([a], [b, b]),
                 lambda: structures.tm_align([np.zeros((5, 2))], [b]),
                 lambda: structures.tm_align([a], [np.zeros((0, 3))]),
                 lambda: structures.tm_align([np.zeros((513, 3))], [b]),
                 lambda: structures.tm_align([a], [b], norm_lens=[4]),
                 lambda: structures.tm_align([a], [b], norm_lens=[5, 6]),
                 lambda: structures.tm_align([a], [b], max_iter=0),
                 lambda: structures.pairwise_tm([a, b], pairs=[(0, 2)]),
                 lambda: structures.pairwise_tm([a, b], pairs=[(0, 1)], norm_lens=[8, 8]),
                 lambda: structures.pairwise_tm([a, np.zeros((513, 3))]),
                 lambda: structures.pairwise_tm([a, b], chunk=0),
                 lambda: structures.max_tm_across_refs([a], []),
                 lambda: structures.max_tm_across_refs([np.zeros(3)], [b])):
        with pytest.raises(ValueError):
            call()


def test_cli_training_set_argument(tmp_path):
    """--train of bin/tmscore_training.py: a directory gives its .pdb / .pdb.gz files, a text file the paths it lists."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tmscore_training_cli", os.path.join(REPO, "bin", "tmscore_training.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    for name in ("b.pdb", "a.pdb.gz", "notes.txt"):
        (tmp_path / name).write_text("")
    assert cli.training_files(str(tmp_path)) == [str(tmp_path / "a.pdb.gz"), str(tmp_path / "b.pdb")]
    listing = tmp_path / "list.txt"
    listing.write_text("x/1.pdb\n\n  y/2.pdb  \n")
    assert cli.training_files(str(listing)) == ["x/1.pdb", "y/2.pdb"]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-d", "somewhere"])   # --train is required


@pytest.fixture(scope="module")
def align_asm(tmp_path_factory):
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    out = tmp_path_factory.mktemp("isa") / "tm_align.s"
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
           "--cuda-device-only", "-o", str(out), os.path.join(fbuild.CSRC, "tm_align.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_align_kernel_holds_no_scratch_and_fits_its_occupancy(align_asm):
    """No scratch (a spill in the search's pass loop or in a DP cell would dominate it), and registers for the
    occupancy DESIGN.md "TM-align-style alignment" claims: one wave per SIMD, i.e. one 256-lane workgroup per CU --
    VGPRs + AGPRs, each rounded up to the allocation granule of 8, within the 512 per lane."""
    m = re.search(r"\.name:\s+(_Z\S*tm_align_kernel\S*)\n(.*?)\.wavefront_size", align_asm, re.S)
    assert m, "tm_align_kernel not found in the metadata"
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(2))}
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md   # (scalar registers parked in vector lanes touch no memory)
    regs = -(-md["vgpr_count"] // 8) * 8 + -(-md.get("agpr_count", 0) // 8) * 8
    print(f"tm_align_kernel: {md['vgpr_count']} VGPRs, {md.get('agpr_count', 0)} AGPRs, {md['sgpr_count']} SGPRs")
    assert 512 // regs >= 1, md
