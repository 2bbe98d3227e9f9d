"""Backbone oxygens and DSSP states without a device: the numpy restatement (tests/dssp_reference.py) against the anchors of
DESIGN.md 6t (crambin's string, ideal helices, the oxygen-torsion finding), the new symbols, the argument checks of
fd_backbone_oxygens and fd_dssp, the PDB reader and writer, and the command lines' parsers.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dssp_reference as dr
from conftest import GOLDEN, REPO
from foldingdiff_amd import _binding, structures
from foldingdiff_amd import angles_and_coords as ac

CRN = os.path.join(GOLDEN, "1CRN.pdb")
CRN_DSSP = "-EE-SSHHHHHHHHHHHTTT--HHHHHHHHS-EE-SSS---GGG--"


@pytest.fixture(scope="module")
def crambin():
    """(float64 [46, 4, 3] N / CA / C / O of the fixture, uint8 [46] flags with PRO as no donor)."""
    xyz, names = structures.read_backbone_atoms(CRN)
    return xyz, np.array([dr.NO_DONOR if n == "PRO" else 0 for n in names], np.uint8)


def test_restatement_gives_crambin_its_known_string(crambin):
    """The two helices, the antiparallel ladder 2-3 / 33-34 and the C-terminal 3-10 turn; 27 kept bonds; no energy within
    0.02 kcal/mol of the cut and no bend within 4 degrees of 70."""
    bb, flags = crambin
    assert bb.shape == (46, 4, 3) and not np.isnan(bb).any() and int(flags.sum()) == 5
    lab, acc, en, counts = dr.dssp(bb, flags)
    assert dr.string(lab) == CRN_DSSP
    assert counts == (27, 2, 2)
    assert dr.bridge_types(acc) == (False, True)
    E = dr.energies(bb, flags)
    assert 0.02 < np.nanmin(np.abs(E + 0.5)) < 0.022
    bend = dr.bend_angles(bb)
    assert 4.0 < np.nanmin(np.abs(bend - 70.0)) < 4.2
    assert 0.02 < dr.threshold_margin(bb, flags) < 0.022
    assert (acc[flags == 1] == -1).all() and (acc[0] == -1).all()


@pytest.mark.parametrize("name, want, energy", [("alpha", "-" + "H" * 18 + "-", -2.94), ("g310", "-" + "G" * 18 + "-", -3.71),
                                                ("pi", "-" + "I" * 18 + "-", -5.93), ("beta", "-" * 20, None)])
def test_restatement_on_ideal_chains(name, want, energy):
    """20 residues of one (phi, psi) built with the reference's NeRF constants, O trans to the next N."""
    bb = dr.ideal_chain(*dr.SEGMENTS[name])
    lab, acc, en, counts = dr.dssp(bb)
    assert dr.string(lab) == want
    if energy is None:
        assert counts[0] == 0
    else:
        n = {"alpha": 4, "g310": 3, "pi": 5}[name]
        donors = np.arange(n, 20)          # every residue from n on gives its hydrogen to the carbonyl n residues back
        assert (acc[donors, 0] == donors - n).all()
        assert np.abs(en[donors, 0] - energy).max() < 0.005


def test_oxygen_torsion_finding(crambin):
    """Placed trans to the next N, the oxygens lie 0.057 A (mean) from crambin's own; at the reference script's torsion they
    lie on the next residue's N instead."""
    bb, _ = crambin
    trans = dr.add_oxygens(bb[:, :3])
    assert np.isnan(trans[-1, 3]).all() and (trans[:, :3] == bb[:, :3]).all()
    d = np.linalg.norm(trans[:-1, 3] - bb[:-1, 3], axis=1)
    assert d.mean() <= 0.1 and d.max() < 0.12
    literal = dr.add_oxygens(bb[:, :3], reference_torsion=True)
    to_next_n = np.linalg.norm(literal[:-1, 3] - bb[1:, 0], axis=1)
    assert to_next_n.max() < 0.3
    assert np.linalg.norm(literal[:-1, 3] - bb[:-1, 3], axis=1).min() > 1.5
    # both obey the bond length and angle they were given
    for o in (trans, literal):
        v, w = o[:-1, 3] - o[:-1, 2], o[:-1, 1] - o[:-1, 2]
        assert np.abs(np.linalg.norm(v, axis=1) - dr.O_LENGTH).max() < 1e-12
        cosang = (v * w).sum(1) / (np.linalg.norm(v, axis=1) * np.linalg.norm(w, axis=1))
        assert np.abs(np.arccos(cosang) - dr.O_ANGLE).max() < 1e-9


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"#define FDMI_DSSP_MAX_LEN 1024\b", header) and structures.DSSP_MAX_LEN == 1024
    assert re.search(r"#define FDMI_ABI_VERSION 7\b", header) and _binding.ABI_VERSION == 7
    for name, n_args in (("fd_backbone_oxygens", 7), ("fd_dssp", 10)):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _binding.exported_symbols() and len(_binding._SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
    for name in ("read_backbone_atoms", "add_oxygens", "dssp", "dssp_counts", "dssp_from_backbones", "dssp_of_pdb"):
        assert callable(getattr(structures, name))
    assert "".join(structures.DSSP_STATES) == dr.STATES


def test_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Every bad call of the two entries returns -1 with its word in fd_last_error() and leaves the outputs alone, on a machine
    without a GPU too.  No valid call is made.  Two chains of 4 and 6 residues."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    rng = np.random.default_rng(5)
    offs, lens = i32(0, 4), i32(4, 6)
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    def spoiled(x, where, value):
        y = x.copy()
        y[where] = value
        return y

    x3 = rng.standard_normal((10, 3, 3))

    def oxygens(x=x3, offs=offs, lens=lens, n=2, out="default"):
        out = np.full((10, 4, 3), -7.0) if isinstance(out, str) else out
        return [out], lib.fd_backbone_oxygens(0, P(x), P(offs), P(lens), n, 0, P(out))

    for kw, word in [(dict(x=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(out=None), b"null"),
                     (dict(n=0), b"n_chains"), (dict(n=-3), b"n_chains"), (dict(lens=i32(4, 0)), b"lens"),
                     (dict(lens=i32(1025, 6)), b"outside [1, 1024]"), (dict(offs=i32(0, 5)), b"offsets"),
                     (dict(offs=i32(1, 5)), b"offsets"), (dict(x=spoiled(x3, (7, 1, 2), np.nan)), b"finite"),
                     (dict(x=spoiled(x3, (0, 0, 0), np.inf)), b"finite"), (dict(x=spoiled(x3, (9, 2, 1), -1.5e6)), b"beyond 1e6")]:
        expect(word, *oxygens(**kw))

    x4 = rng.standard_normal((10, 4, 3))
    x4[[3, 9], 3] = np.nan      # a missing oxygen is allowed and must not be what a call is rejected for
    flags = np.zeros(10, np.uint8)

    def dssp(x=x4, flags=flags, offs=offs, lens=lens, n=2, state="default", acc="default", energy="default"):
        state = np.full(10, -7, np.int8) if isinstance(state, str) else state
        acc = np.full((10, 2), -7, np.int32) if isinstance(acc, str) else acc
        energy = np.full((10, 2), -7.0) if isinstance(energy, str) else energy
        counts = np.full((2, 3), -7, np.int32)
        return [state, acc, energy, counts], lib.fd_dssp(0, P(x), P(flags), P(offs), P(lens), n, P(state), P(acc), P(energy), P(counts))

    for kw, word in [(dict(x=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(state=None), b"null"),
                     (dict(acc=None), b"go together"), (dict(energy=None), b"go together"),
                     (dict(n=0), b"n_chains"), (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(1025, 6)), b"outside [1, 1024]"),
                     (dict(offs=i32(0, 5)), b"offsets"), (dict(x=spoiled(x4, (7, 1, 2), np.nan)), b"finite"),
                     (dict(x=spoiled(x4, (2, 0, 0), np.nan)), b"finite"), (dict(x=spoiled(x4, (5, 3, 1), np.inf)), b"finite"),
                     (dict(x=spoiled(x4, (9, 2, 1), 1.5e6)), b"beyond 1e6"), (dict(flags=None, x=spoiled(x4, (0, 2, 2), -np.inf)), b"finite")]:
        expect(word, *dssp(**kw))
    assert checked == 13 + 15


def test_python_wrappers_check_shapes_before_any_call():
    with pytest.raises(ValueError, match="backbone 0"):
        structures.add_oxygens([np.zeros((4, 3))])
    with pytest.raises(ValueError, match="chain 1"):
        structures.dssp([np.zeros((2, 4, 3)), np.zeros((7, 3))])
    with pytest.raises(ValueError, match="1024"):
        structures.dssp([np.zeros((1025, 4, 3))])
    with pytest.raises(ValueError, match="flags"):
        structures.dssp([np.zeros((2, 4, 3))], flags=[np.zeros(3, np.uint8)])
    assert structures.add_oxygens([]) == [] and structures.dssp([]) == [] and structures.dssp_counts([]).shape == (0, 3)


def test_writer_layout_and_reader_round_trip(tmp_path):
    """write_backbone_with_o_pdb on three residues: four atoms per residue with O after C, no O on the last, the columns
    of write_coords_to_pdb, CONECT between each C and the next N; read_backbone_atoms gives the three decimals back."""
    xyz = np.array([[[-1.0, 2.25, 3.5], [0.4567, -10.0, 100.125], [1.0, 1.0, 1.0], [2.125, 2.0, -2.0]],
                    [[3.0, 3.0, 3.0], [4.0, 4.0, 4.0], [5.0, 5.0, 5.0], [6.0, 6.0, 6.0]],
                    [[7.0, 7.0, 7.0], [8.0, 8.0, 8.0], [9.0, 9.0, 9.0], [np.nan] * 3]])
    out = ac.write_backbone_with_o_pdb(xyz, str(tmp_path / "three.pdb"))
    lines = open(out).read().split("\n")
    assert lines[:4] == [
        "ATOM      1  N   GLY A   1      -1.000   2.250   3.500  1.00  5.00           N  ",
        "ATOM      2  CA  GLY A   1       0.457 -10.000 100.125  1.00  5.00           C  ",
        "ATOM      3  C   GLY A   1       1.000   1.000   1.000  1.00  5.00           C  ",
        "ATOM      4  O   GLY A   1       2.125   2.000  -2.000  1.00  5.00           O  ",
    ]
    assert [l[12:16] + l[22:26] for l in lines[:11]] == [" N     1", " CA    1", " C     1", " O     1", " N     2", " CA    2", " C     2",
                                                          " O     2", " N     3", " CA    3", " C     3"]
    assert lines[11:] == ["CONECT    3    5", "CONECT    5    3", "CONECT    7    9", "CONECT    9    7", ""]
    # the N / CA / C records are write_coords_to_pdb's own, apart from the serial numbers
    plain = open(ac.write_coords_to_pdb(xyz[:, :3].reshape(-1, 3), str(tmp_path / "plain.pdb"))).read().split("\n")
    assert [l[11:] for l in lines[:11] if l[13] != "O"] == [l[11:] for l in plain[:9]]
    back, names = structures.read_backbone_atoms(out)
    assert names == ["GLY"] * 3 and back.shape == (3, 4, 3) and np.isnan(back[2, 3]).all()
    assert np.nanmax(np.abs(back - xyz)) <= 0.00051
    assert (structures.read_backbone(out)[0] == back[:, :3].reshape(-1, 3).astype(np.float32)).all()


def test_read_backbone_atoms_follows_read_backbone(tmp_path):
    xyz, names = structures.read_backbone_atoms(CRN)
    plain, ids = structures.read_backbone(CRN)
    assert len(names) == len(ids) == 46 and names[:5] == ["THR", "THR", "CYS", "CYS", "PRO"]
    assert (xyz[:, :3].reshape(-1, 3).astype(np.float32) == plain).all()
    body = "".join(line for line in open(CRN) if line.startswith("ATOM"))
    two = tmp_path / "two_models.pdb"
    two.write_text(f"MODEL        1\n{body}ENDMDL\nMODEL        2\n{body}ENDMDL\n")
    assert structures.read_backbone_atoms(str(two)) is None and structures.read_backbone(str(two)) is None
    no_ca = tmp_path / "no_ca.pdb"
    no_ca.write_text("".join(l for l in body.splitlines(True) if not (l[12:16].strip() == "CA" and l[22:26].strip() == "7")))
    assert structures.read_backbone_atoms(str(no_ca)) is None and structures.read_backbone(str(no_ca)) is None


def test_dssp_refusals_stay(tmp_path):
    """count_structures_in_pdb(backend="dssp") still raises: the reference's "dssp" is the mkdssp binary."""
    with pytest.raises(ValueError, match="dssp"):
        structures.count_structures_in_pdb(CRN, backend="dssp")


def _script(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name.replace(".py", "_cli"), os.path.join(REPO, "bin", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_parsers():
    """The arguments of the two new scripts and bin/sample.py --dssp, parsed in this process."""
    args = _script("add_oxygen_to_backbone.py").build_parser().parse_args(["in", "out", "--reference_torsion"])
    assert (args.input, args.outdir, args.reference_torsion) == ("in", "out", True)
    assert _script("add_oxygen_to_backbone.py").build_parser().parse_args(["in", "out"]).reference_torsion is False
    parser = _script("dssp_structures.py").build_parser()
    args = parser.parse_args(["a.pdb", "b.pdb", "plot.pdf", "--json", "x.json", "-t", "4", "--title", "t", "--freqlim", "0"])
    assert (args.infiles, args.outpdf, args.json, args.threads) == (["a.pdb", "b.pdb"], "plot.pdf", "x.json", 4)
    with pytest.raises(SystemExit):
        parser.parse_args(["a.pdb", "plot.pdf", "--backend", "psea"])
    sample = _script("sample.py").build_parser()
    assert sample.parse_args(["-m", "model", "--dssp"]).dssp is True and sample.parse_args(["-m", "model"]).dssp is False
    # the P-SEA script still refuses a DSSP backend
    with pytest.raises(NotImplementedError, match="dssp"):
        _script("annot_secondary_structures.py").main(["a.pdb", "plot.pdf", "--backend", "dssp"])
