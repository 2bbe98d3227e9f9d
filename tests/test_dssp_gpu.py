"""fd_backbone_oxygens and fd_dssp on the device: every label, kept bond, energy and count against the numpy restatement
(tests/dssp_reference.py) over the fixtures and a seeded synthetic set, the oxygens in both torsion modes, invariances,
flags, the anchors of DESIGN.md 6t, short chains, NeRF output end to end and the three command lines.
Needs an MI355X:  pytest -m gpu"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dssp_reference as dr
from conftest import REPO
from foldingdiff_amd import nerf, structures
from foldingdiff_amd import angles_and_coords as ac
from test_dssp import CRN_DSSP
from test_structures_gpu import FIXTURES

pytestmark = pytest.mark.gpu

SIZES = list(range(1, 10)) + [20, 46, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512]
NOISE = [0.0, 0.1, 0.25, 0.5]
N_SYNTHETIC = 120


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps(kw, sort_keys=True))


def _fixture_chain(fname):
    xyz, names = structures.read_backbone_atoms(fname)
    return xyz, np.array([dr.NO_DONOR if n == "PRO" else 0 for n in names], np.uint8)


@pytest.fixture(scope="module")
def cases():
    """The test set and the restatement's results on it, computed once and left unchanged: the two fixture files (their
    own O atoms, PRO as no donor), 120 seeded chains whose lengths cycle through SIZES and whose noise cycles through
    NOISE, and one chain of FDMI_DSSP_MAX_LEN residues.  A dict of lists: chains, flags, E (the energy matrices), lab,
    acc, en, counts."""
    chains, flags = map(list, zip(*[_fixture_chain(f) for f in FIXTURES]))
    rng = np.random.default_rng(0)
    chains += [dr.segment_chain(rng, SIZES[k % len(SIZES)], NOISE[k % len(NOISE)]) for k in range(N_SYNTHETIC)]
    chains.append(dr.segment_chain(rng, structures.DSSP_MAX_LEN, 0.25))
    flags += [np.zeros(len(c), np.uint8) for c in chains[2:]]
    out = {"chains": chains, "flags": flags, "E": [dr.energies(c, f) for c, f in zip(chains, flags)]}
    res = [dr.dssp(c, f, E=E) for c, f, E in zip(chains, flags, out["E"])]
    out.update(lab=[r[0] for r in res], acc=[r[1] for r in res], en=[r[2] for r in res], counts=[r[3] for r in res])
    return out


def _assert_same(got_states, got_bonds, got_counts, cases, which=None):
    which = range(len(cases["chains"])) if which is None else which
    worst = 0.0
    for k, idx in enumerate(which):
        want = dr.string(cases["lab"][idx])
        assert "".join(got_states[k]) == want, (idx, len(want))
        acc, en = got_bonds[k]
        assert (acc == cases["acc"][idx]).all(), idx
        ref = cases["en"][idx]
        assert ((en == 0.0) == (ref == 0.0)).all(), idx
        rel = np.abs(en - ref) / np.maximum(np.abs(ref), 1e-300)
        worst = max(worst, float(rel[ref != 0.0].max(initial=0.0)))
        assert tuple(int(v) for v in got_counts[k]) == cases["counts"][idx], idx
    assert worst <= 1e-9, worst
    return worst


def test_against_restatement(gpu, cases):
    """Labels, kept acceptors and counts of all 123 chains, labelled in one call, equal the restatement's; energies agree
    to 1e-9 relative.  The set is checked first, on the restatement alone: no chain within 1e-9 of a threshold, every state
    at least 50 times, both bridge types, donors with three or more acceptors under the cut, energies clamped at -9.9."""
    chains, flags = cases["chains"], cases["flags"]
    assert len(chains) == 2 + N_SYNTHETIC + 1
    assert sorted({len(c) for c in chains[2:]}) == sorted(set(SIZES) | {structures.DSSP_MAX_LEN})
    margin = min(dr.threshold_margin(c, f, E=E) for c, f, E in zip(chains, flags, cases["E"]))
    n_states = np.sum([np.bincount(lab, minlength=8) for lab in cases["lab"]], axis=0)
    kinds = np.array([dr.bridge_types(acc) for acc in cases["acc"]])
    with np.errstate(invalid="ignore"):
        three = sum(int(((E < dr.E_CUT).sum(0) >= 3).sum()) for E in cases["E"])
        clamped = sum(int((E == dr.E_MIN).sum()) for E in cases["E"])
    _record("dssp_set", margin=margin, states=dict(zip(dr.STATES, n_states.tolist())), parallel=int(kinds[:, 0].sum()),
            antiparallel=int(kinds[:, 1].sum()), donors_with_three=three, clamped=clamped)
    assert margin >= 1e-9
    assert (n_states >= 50).all(), n_states
    assert kinds[:, 0].any() and kinds[:, 1].any()
    assert three >= 1 and clamped >= 1

    states, bonds = structures.dssp(chains, flags=flags, device=gpu, return_hbonds=True)
    counts = structures.dssp_counts(chains, flags=flags, device=gpu)
    worst = _assert_same(states, bonds, counts, cases)
    _record("dssp_energy", worst_relative=worst)
    # without the optional outputs the labels are the same
    assert all((a == b).all() for a, b in zip(structures.dssp(chains, flags=flags, device=gpu), states))


@pytest.mark.parametrize("reference_torsion", [False, True])
def test_oxygens_against_restatement(gpu, cases, reference_torsion):
    """fd_backbone_oxygens on the N / CA / C of the whole set: O within 1e-9 A of the restatement, NaN exactly on the last
    residue of every chain, N / CA / C copied bit for bit."""
    nca_c = [c[:, :3] for c in cases["chains"]]
    got = structures.add_oxygens(nca_c, reference_torsion=reference_torsion, device=gpu)
    worst = 0.0
    for k, (x, g) in enumerate(zip(nca_c, got)):
        want = dr.add_oxygens(x, reference_torsion)
        assert g.shape == want.shape == (len(x), 4, 3)
        assert (g[:, :3] == x).all(), k
        assert np.isnan(g[-1, 3]).all() and not np.isnan(g[:-1]).any(), k
        if len(x) > 1:
            worst = max(worst, float(np.linalg.norm(g[:-1, 3] - want[:-1, 3], axis=1).max()))
    _record("oxygens", reference_torsion=reference_torsion, worst_A=worst)
    assert worst <= 1e-9
    if not reference_torsion:   # the synthetic chains carry the restatement's own oxygens
        k = 2 + SIZES.index(46)
        assert np.abs(got[k][:-1, 3] - cases["chains"][k][:-1, 3]).max() <= 1e-9


def test_rigid_motion_leaves_labels_and_bonds(gpu, cases):
    which = [0, 1] + list(range(2 + len(SIZES) - 8, 2 + len(SIZES)))
    rng = np.random.default_rng(11)
    moved = []
    for i in which:
        R, t = dr.rotation(rng), rng.uniform(-50.0, 50.0, 3)
        moved.append(cases["chains"][i] @ R.T + t)
    flags = [cases["flags"][i] for i in which]
    states, bonds = structures.dssp(moved, flags=flags, device=gpu, return_hbonds=True)
    for k, i in enumerate(which):
        assert "".join(states[k]) == dr.string(cases["lab"][i]), i
        assert (bonds[k][0] == cases["acc"][i]).all(), i
        assert np.allclose(bonds[k][1], cases["en"][i], rtol=1e-6, atol=0.0), i


def test_a_chain_alone_in_a_batch_and_in_a_permuted_batch(gpu, cases):
    """Bit-identical results (energies too) whatever else the call holds, and wherever in it the chain sits."""
    which = [0, 1] + list(range(2, 2 + len(SIZES)))
    chains, flags = [cases["chains"][i] for i in which], [cases["flags"][i] for i in which]
    states, bonds = structures.dssp(chains, flags=flags, device=gpu, return_hbonds=True)
    counts = structures.dssp_counts(chains, flags=flags, device=gpu)
    _assert_same(states, bonds, counts, cases, which)
    perm = np.random.default_rng(3).permutation(len(which))
    p_states, p_bonds = structures.dssp([chains[i] for i in perm], flags=[flags[i] for i in perm], device=gpu, return_hbonds=True)
    p_counts = structures.dssp_counts([chains[i] for i in perm], flags=[flags[i] for i in perm], device=gpu)
    for k, i in enumerate(perm):
        assert (p_states[k] == states[i]).all() and (p_counts[k] == counts[i]).all()
        assert (p_bonds[k][0] == bonds[i][0]).all() and (p_bonds[k][1] == bonds[i][1]).all()
    for i in (0, 5, len(which) - 1):
        s, b = structures.dssp([chains[i]], flags=[flags[i]], device=gpu, return_hbonds=True)
        assert (s[0] == states[i]).all() and (b[0][0] == bonds[i][0]).all() and (b[0][1] == bonds[i][1]).all()
        assert (structures.dssp_counts([chains[i]], flags=[flags[i]], device=gpu)[0] == counts[i]).all()


def test_flags_are_honoured(gpu, cases):
    """Marking donors removes exactly their bonds; marking an acceptor removes it from every list; both as the
    restatement has them."""
    bb, flags = cases["chains"][0], cases["flags"][0]
    acc0 = cases["acc"][0]
    donors = np.flatnonzero(acc0[:, 0] >= 0)[::3]
    marked = flags.copy()
    marked[donors] |= dr.NO_DONOR
    (s,), ((acc, en),) = structures.dssp([bb], flags=[marked], device=gpu, return_hbonds=True)
    assert (acc[donors] == -1).all() and (en[donors] == 0.0).all()
    others = np.setdiff1d(np.arange(len(bb)), donors)
    assert (acc[others] == acc0[others]).all()
    want = dr.dssp(bb, marked)
    assert "".join(s) == dr.string(want[0]) and (acc == want[1]).all()
    assert int(structures.dssp_counts([bb], flags=[marked], device=gpu)[0, 0]) == cases["counts"][0][0] - int((acc0[donors] >= 0).sum())

    acceptor = int(np.bincount(acc0[acc0 >= 0]).argmax())
    marked = flags.copy()
    marked[acceptor] |= dr.NO_ACCEPTOR
    (s,), ((acc, en),) = structures.dssp([bb], flags=[marked], device=gpu, return_hbonds=True)
    assert (acc0 == acceptor).any() and not (acc == acceptor).any()
    want = dr.dssp(bb, marked)
    assert "".join(s) == dr.string(want[0]) and (acc == want[1]).all()
    # a missing oxygen: no acceptor, and the next residue no donor
    holed = bb.copy()
    holed[acceptor, 3] = np.nan
    (s,), ((acc, en),) = structures.dssp([holed], flags=[flags], device=gpu, return_hbonds=True)
    assert acceptor + 1 < len(bb) and not (acc == acceptor).any() and (acc[acceptor + 1] == -1).all()
    want = dr.dssp(holed, flags)
    assert "".join(s) == dr.string(want[0]) and (acc == want[1]).all()


def test_anchors(gpu):
    """Crambin's string from the file, and the ideal helices built with the reference's NeRF constants, their oxygens
    placed on the device."""
    assert "".join(structures.dssp_of_pdb(FIXTURES[0], device=gpu)) == CRN_DSSP
    names = ["alpha", "g310", "pi", "beta"]
    ideal = [dr.nerf_chain(np.full(20, np.radians(dr.SEGMENTS[k][0])), np.full(20, np.radians(dr.SEGMENTS[k][1]))) for k in names]
    labels, bonds = structures.dssp_from_backbones(ideal, device=gpu, return_hbonds=True)
    assert ["".join(s) for s in labels] == ["-" + "H" * 18 + "-", "-" + "G" * 18 + "-", "-" + "I" * 18 + "-", "-" * 20]
    for (acc, en), want in zip(bonds[:3], (-2.94, -3.71, -5.93)):
        assert np.abs(en[acc[:, 0] >= 0, 0] - want).max() < 0.005


def test_short_chains(gpu):
    """Chains of 1 to 3 residues have no state but '-' whatever their geometry (a turn needs 4 residues, a bend 5, a bridge
    6); chains of 4 and 5 residues can hold a turn, a 3-10 helix or a bend, and do where the restatement says so."""
    rng = np.random.default_rng(2)
    chains = [dr.ideal_chain(*dr.SEGMENTS[k], n=n) for n in range(1, 6) for k in ("alpha", "g310", "pi", "beta")]
    chains += [dr.add_oxygens(rng.standard_normal((n, 3, 3)) * 2.0) for n in range(1, 6) for _ in range(4)]
    got = ["".join(s) for s in structures.dssp(chains, device=gpu)]
    assert got == [dr.string(dr.dssp(c)[0]) for c in chains]
    assert all(g == "-" * len(g) for g in got if len(g) <= 3)
    by_case = dict(zip([(n, k) for n in range(1, 6) for k in ("alpha", "g310", "pi", "beta")], got))
    assert by_case[(4, "g310")] == "-TT-" and by_case[(5, "g310")] == "-GGG-" and by_case[(5, "alpha")] == "-TTT-"
    assert by_case[(5, "pi")] == "--S--" and by_case[(5, "beta")] == "-----"
    assert (structures.dssp_counts(chains[:4], device=gpu) == 0).all()


def test_nerf_output_end_to_end(gpu):
    """dssp_from_backbones on nerf.build_backbones output for the angle rows an untrained model gives (uniform random
    angles): the restatement's labels on the same coordinates."""
    from foldingdiff_amd.datasets import FEATURE_SET_NAMES_TO_FEATURE_NAMES as NAMES
    rng = np.random.default_rng(4)
    rows = [rng.uniform(-np.pi, np.pi, (n, 6)).astype(np.float32) for n in (12, 33, 64, 100)]
    for r in rows:
        r[:, 3:] = rng.uniform(1.8, 2.2, r[:, 3:].shape)     # bond angles in a chain-like range
    backbones = nerf.build_backbones(rows, NAMES["canonical-full-angles"], device=gpu)
    labels, bonds = structures.dssp_from_backbones(backbones, device=gpu, return_hbonds=True)
    for bb, lab, (acc, _) in zip(backbones, labels, bonds):
        want = dr.dssp(dr.add_oxygens(bb))
        assert dr.threshold_margin(dr.add_oxygens(bb)) >= 1e-9
        assert "".join(lab) == dr.string(want[0]) and (acc == want[1]).all()


def test_oxygen_cli_and_round_trip(gpu, tmp_path):
    """bin/add_oxygen_to_backbone.py on a directory with the two fixtures: four atoms per residue in each output, which read
    back give the device's coordinates to the writer's three decimals."""
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir()
    for f in FIXTURES:
        (indir / os.path.basename(f)).write_text(open(f).read())
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "add_oxygen_to_backbone.py"), str(indir), str(outdir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(outdir)) == sorted(os.path.basename(f) for f in FIXTURES)
    for f in FIXTURES:
        plain = structures.read_backbone(f)[0]
        want = structures.add_oxygens([plain], device=gpu)[0]
        back, names = structures.read_backbone_atoms(str(outdir / os.path.basename(f)))
        assert set(names) == {"GLY"} and back.shape == want.shape
        assert np.isnan(back[-1, 3]).all() and not np.isnan(back[:-1]).any()
        assert np.nanmax(np.abs(back - want)) <= 0.00051
        n_atoms = sum(1 for line in open(outdir / os.path.basename(f)) if line.startswith("ATOM"))
        assert n_atoms == 4 * len(want) - 1


def test_dssp_cli(gpu, tmp_path):
    """bin/dssp_structures.py on the fixtures: exit 0, crambin's string and the counts of structures.dssp_counts."""
    out = tmp_path / "dssp.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "dssp_structures.py"), *FIXTURES, str(tmp_path / "plot.pdf"),
                        "--json", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    assert list(res) == [os.path.basename(f) for f in FIXTURES]
    assert res["1CRN.pdb"] == {"dssp": CRN_DSSP, "n_helix": 2, "n_strand": 2, "n_hbonds": 27}
    other = res["all_residues.pdb"]
    assert other["dssp"] == "".join(structures.dssp_of_pdb(FIXTURES[1], device=gpu))


def test_sample_cli_dssp(gpu, tmp_path):
    """bin/sample.py --dssp on a toy model: dssp.json holds, per written file, the labels and counts of that file's
    coordinates with the oxygens added."""
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "9", "12",
                        "-b", "4", "--seed", "3", "--dssp"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["dssp.json", "model_snapshot", "sampled_angles", "sampled_pdb"]
    res = json.load(open(os.path.join(out, "dssp.json")))
    names = [f"generated_{i}.pdb" for i in range(6)]
    assert list(res) == names
    written = [ac.read_pdb_backbone(os.path.join(out, "sampled_pdb", f)) for f in names]
    assert [len(x) // 3 for x in written] == [9, 9, 10, 10, 11, 11]
    labels = structures.dssp_from_backbones(written, device=gpu)
    counts = structures.dssp_counts(structures.add_oxygens(written, device=gpu), device=gpu)
    for f, lab, c in zip(names, labels, counts):
        assert res[f] == {"dssp": "".join(lab), "n_hbonds": int(c[0]), "n_helix": int(c[1]), "n_strand": int(c[2]),
                          "hbonds_per_residue": int(c[0]) / len(lab)}
