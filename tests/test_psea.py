"""The P-SEA annotation's definition on the host: the numpy restatement (tests/psea_reference.py) on the anchors of
DESIGN.md "Secondary structure (P-SEA)", short chains, rigid motion; the C ABI's new entry; the Python argument checks
of ``structures.annotate_sse``; the parser of bin/sample.py; a static guard on the kernel.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import psea_reference as pr
from conftest import GOLDEN, REPO
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import structures


def _fixture_ca(name):
    return structures.read_backbone(os.path.join(GOLDEN, name))[0][1::3]


def test_anchor_1crn():
    """Agrees with the file's own HELIX / SHEET records: helices 7-19 and 23-30, strand 32-35."""
    s = pr.psea(_fixture_ca("1CRN.pdb"))
    assert s == "ccccccaaaaaaaaaaacccccaaaaaaaccbbbbccccccccccc"
    assert pr.counts(s) == (2, 1)


def test_anchor_all_residues():
    s = pr.psea(_fixture_ca("all_residues.pdb"))
    assert s == "cccccccccccaaaaaaaac"
    assert pr.counts(s) == (1, 0)


def test_anchor_ideal_helix():
    """x_i = (2.3 cos 100 i, 2.3 sin 100 i, 1.5 i): right-handed, so the IUPAC dihedral is about +50 degrees."""
    h = pr.ideal_helix(24)
    assert pr.geometry(h)["a"][1] == pytest.approx(50.04, abs=0.01)
    assert pr.psea(h) == "c" + "a" * 22 + "c"
    assert pr.counts(pr.psea(h)) == (1, 0)
    # left-handed: the dihedral changes sign, so only the distance test (blind to the hand, defined up to residue 20)
    # finds potential helix; residue 21 is an extension and residue 22 no longer is
    mirrored = h * np.array([1.0, 1.0, -1.0])
    assert pr.geometry(mirrored)["a"][1] == pytest.approx(-50.04, abs=0.01)
    assert pr.psea(mirrored) == "c" + "a" * 21 + "cc"


def test_anchor_hairpin():
    s = pr.psea(pr.hairpin())
    assert len(s) == 22 and pr.counts(s) == (0, 2)
    assert "a" not in s


def test_undefined_quantities_and_short_chains():
    h = pr.ideal_helix(24)
    q = pr.geometry(h)
    n = len(h)
    for name, last in (("d2", n - 2), ("r", n - 2), ("d3", n - 3), ("a", n - 3), ("d4", n - 4)):
        defined = ~np.isnan(q[name])
        assert defined[1:last + 1].all() and not defined[0] and not defined[last + 1:].any(), name
    for m in range(6):
        assert pr.psea(h[:m]) == "c" * m
        assert pr.psea(pr.hairpin()[:m]) == "c" * m
        assert pr.counts(pr.psea(h[:m])) == (0, 0)


def test_contact_rule_for_runs_of_three():
    """A potential-strand run of exactly three residues (4-6 here) is strand only with >= 5 contacts: a six-residue
    strand alone (sum 0), beside one partner strand 4.8 A away (sum 3), and between two (sum 6)."""
    coil = np.array([[-9.0, 3.0, 4.0], [-6.0, 5.0, 2.5], [-3.0, 4.0, 0.5]])
    short = np.concatenate([coil, pr.wavy_strand(6), coil[::-1] * np.array([-1.0, 1.0, 1.0]) + [16.5, 0.0, 0.0]])

    def partner(y):   # the strand's own wave and zig-zag, two residues longer at each end, moved by y
        j = np.arange(-2, 8)
        return np.stack([3.3 * j, y + 0.3 * np.sin(1.3 * j), 0.9 * (-1.0) ** j], 1)

    one = np.concatenate([short, partner(4.8)[::-1]])
    two = np.concatenate([one, partner(-4.8)])
    for chain, total, label in ((short, 0, "c"), (one, 3, "c"), (two, 6, "b")):
        assert (4, 7) in pr.runs(pr.flags(chain)[1])
        assert pr.three_run_sums(chain) == [total]
        assert pr.contacts(chain)[4:7].tolist() == [total // 3] * 3
        assert pr.sets(chain)[1][4:7].tolist() == [label == "b"] * 3
        assert pr.psea(chain)[4:7] == label * 3
    assert pr.psea(two)[3:8] == "bbbbb"   # residues 3 and 7 are extensions: d3 in the strand range


def test_restatement_is_invariant_under_rigid_motion():
    rng = np.random.default_rng(0)
    for k in range(12):
        ca = pr.segment_chain(rng, 60 + k, [0.1, 0.25, 0.5][k % 3])
        assert pr.threshold_margin(ca) >= 1e-9
        moved = ca @ pr.rotation(rng).T + rng.uniform(-1e3, 1e3, 3)
        assert pr.psea(moved) == pr.psea(ca)


def test_entry_is_declared_in_the_header():
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"^int fd_annotate_sse\(int device_id, const double\* ca,", src, re.M)
    assert re.search(r"^#define FDMI_SSE_MAX_LEN 2048$", src, re.M)
    assert re.search(r"^#define FDMI_ABI_VERSION 7$", src, re.M)


def test_entry_is_bound():
    assert "fd_annotate_sse" in _binding.exported_symbols()
    assert _binding.ABI_VERSION == 7


def test_entry_is_exported(lib):
    assert lib.fd_abi_version() == 7
    assert hasattr(lib, "fd_annotate_sse")


def test_annotate_sse_checks_shapes_in_python():
    assert structures.annotate_sse([]) == []
    assert structures.count_secondary_structures([]).shape == (0, 2)
    for bad in (np.zeros((5, 2)), np.zeros((0, 3)), np.zeros((2049, 3)), np.zeros(6)):
        with pytest.raises(ValueError):
            structures.annotate_sse([bad])
        with pytest.raises(ValueError):
            structures.count_secondary_structures([np.zeros((4, 3)), bad])
    with pytest.raises(ValueError):
        structures.count_structures_in_pdb(os.path.join(GOLDEN, "1CRN.pdb"), backend="dssp")


def test_sample_cli_refuses_psea_with_nopsea(tmp_path):
    """A parser error (exit 2), before the model directory is looked at or a device is touched."""
    cli = os.path.join(REPO, "bin", "sample.py")
    r = subprocess.run([sys.executable, cli, "-m", str(tmp_path / "no_such_model"), "-o", str(tmp_path / "out"), "--psea", "--nopsea"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "not allowed with argument" in r.stderr and "psea" in r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_annot_cli_refuses_what_it_cannot_do(tmp_path):
    cli = os.path.join(REPO, "bin", "annot_secondary_structures.py")
    pdb = os.path.join(GOLDEN, "1CRN.pdb")
    for argv, word in (([pdb, str(tmp_path / "o.pdf"), "--backend", "dssp"], "DSSP"),
                       ([str(tmp_path / "training_args.json"), str(tmp_path / "o.pdf")], "CATH")):
        r = subprocess.run([sys.executable, cli, *argv], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "NotImplementedError" in r.stderr and word in r.stderr, r.stderr[-2000:]
    assert os.listdir(tmp_path) == []


def test_kernel_holds_no_scratch():
    """The per-residue work keeps its vectors in registers: no private segment."""
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
                        "--cuda-device-only", "-o", "-", os.path.join(fbuild.CSRC, "psea.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"\.name:\s+_Z\S*psea_kernel\S*\n(.*?)\.wavefront_size", r.stdout, re.S)
    assert m, "psea_kernel's metadata not found"
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(1))}
    print("psea_kernel:", md)
    assert md["private_segment_fixed_size"] == 0, md
