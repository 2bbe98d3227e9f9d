"""fd_annotate_sse and the secondary-structure path of structures.py on the device: every label and count against the
numpy restatement (tests/psea_reference.py) over the fixtures and a seeded synthetic set, invariances, argument
errors, 1CRN rebuilt by NeRF, count_structures_in_pdb / ss_cooccurrence, bin/annot_secondary_structures.py and
bin/sample.py --psea.  Needs an MI355X:  pytest -m gpu"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import psea_reference as pr
from conftest import REPO
from foldingdiff_amd import _binding, nerf, structures
from foldingdiff_amd import angles_and_coords as ac
from test_structures_gpu import FIXTURES

pytestmark = pytest.mark.gpu

SIZES = list(range(1, 10)) + [20, 46, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512]
NOISE = [0.0, 0.1, 0.25, 0.5]
WANT_JSON = {"1CRN.pdb": [2, 1], "all_residues.pdb": [1, 0]}


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps(kw, sort_keys=True))


def _str(labels):
    return "".join(labels)


@pytest.fixture(scope="module")
def cases():
    """(chains, the restatement's label string of each): the two fixture files, then 126 seeded chains whose lengths
    cycle through SIZES and whose noise cycles through NOISE, then one chain of FDMI_SSE_MAX_LEN residues.  Computed
    once; the tests leave it unchanged."""
    assert [os.path.basename(f) for f in FIXTURES] == list(WANT_JSON)
    chains = [structures.read_backbone(f)[0][1::3].astype(np.float64) for f in FIXTURES]
    rng = np.random.default_rng(0)
    chains += [pr.segment_chain(rng, SIZES[k % len(SIZES)], NOISE[k % len(NOISE)]) for k in range(126)]
    chains.append(pr.segment_chain(rng, 2048, 0.25))
    return chains, [pr.psea(c) for c in chains]


def test_against_restatement(gpu, cases):
    """Every label and every count of 129 chains, annotated in one call, equals the restatement's.  The set is checked
    first: no chain within 1e-9 (A or degrees) of a threshold, all three labels in quantity, length-3 potential-strand
    runs on both sides of the contact rule including sums of exactly 4 and 5, and a residue whose 'a' the strand pass
    overwrites."""
    chains, want = cases
    assert len(chains) == 129 and sorted({len(c) for c in chains}) == sorted(set(SIZES) | {46, 20, 2048})
    margin = min(pr.threshold_margin(c) for c in chains)
    sums = [s for c in chains for s in pr.three_run_sums(c)]
    overwritten = sum(1 for c in chains for a, b in zip(*pr.label_passes(c)) if a == "a" and b == "b")
    n_labels = {k: sum(w.count(k) for w in want) for k in "cab"}
    _record("psea_set", margin=margin, labels=n_labels, three_runs_le4=sum(s <= 4 for s in sums),
            three_runs_ge5=sum(s >= 5 for s in sums), overwritten=overwritten)
    assert margin >= 1e-9
    assert min(n_labels.values()) >= 2000
    assert sum(s <= 4 for s in sums) >= 5 and sum(s >= 5 for s in sums) >= 5 and 4 in sums and 5 in sums
    assert overwritten >= 1
    got = structures.annotate_sse(chains)
    got_counts = structures.count_secondary_structures(chains)
    assert len(got) == len(chains) and got_counts.shape == (len(chains), 2)
    wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g.dtype != np.dtype("U1") or _str(g) != w]
    wrong_counts = [i for i, (g, w) in enumerate(zip(got_counts, want)) if tuple(g) != pr.counts(w)]
    _record("psea_vs_restatement", chains=len(chains), wrong=wrong, wrong_counts=wrong_counts)
    assert not wrong and not wrong_counts
    assert _str(got[0]) == "ccccccaaaaaaaaaaacccccaaaaaaaccbbbbccccccccccc" and tuple(got_counts[0]) == (2, 1)
    assert _str(got[1]) == "cccccccccccaaaaaaaac" and tuple(got_counts[1]) == (1, 0)


def test_anchors(gpu):
    """The ideal helix, its mirror image, the hairpin of two flat strands, and chains too short for any structure."""
    h = pr.ideal_helix(24)
    short = [h[:m] for m in range(1, 6)]
    got = structures.annotate_sse([h, h * np.array([1.0, 1.0, -1.0]), pr.hairpin()] + short)
    assert _str(got[0]) == "c" + "a" * 22 + "c"
    assert _str(got[1]) == "c" + "a" * 21 + "cc"
    assert _str(got[2]) == pr.psea(pr.hairpin())
    assert [_str(g) for g in got[3:]] == ["c" * m for m in range(1, 6)]
    counts = structures.count_secondary_structures([h, pr.hairpin()] + short)
    assert counts.tolist() == [[1, 0], [0, 2]] + [[0, 0]] * 5


def test_rigid_motion(gpu, cases):
    """The same chains under a rotation and a translation of up to 1e3 A give identical labels."""
    chains, want = cases
    rng = np.random.default_rng(1)
    moved = [c @ pr.rotation(rng).T + rng.uniform(-1e3, 1e3, 3) for c in chains]
    assert [_str(g) for g in structures.annotate_sse(moved)] == want


def test_deterministic_and_batch_invariant(gpu, cases):
    """Two identical calls are bitwise equal, and each of four chains annotated alone equals its labels in the batch."""
    chains, want = cases
    lib = _binding.load()
    lens = np.array([len(c) for c in chains], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    X = np.ascontiguousarray(np.concatenate(chains))
    P = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    outs = []
    for _ in range(2):
        sse, counts = np.full(len(X), -7, np.int8), np.full((len(chains), 2), -7, np.int32)
        assert lib.fd_annotate_sse(0, P(X), P(offs), P(lens), len(chains), P(sse), P(counts)) == 0
        outs.append((sse, counts))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert set(np.unique(outs[0][0])) == {0, 1, 2} and outs[0][1].min() >= 0
    for i in (0, 37, 100, 128):
        assert _str(structures.annotate_sse([chains[i]])[0]) == want[i]
        assert tuple(structures.count_secondary_structures([chains[i]])[0]) == pr.counts(want[i])


def test_float32_input(gpu, cases):
    """float32 traces give the labels of the restatement on the same rounded coordinates."""
    chains = [c.astype(np.float32) for c in cases[0][:128:3]]
    rounded = [c.astype(np.float64) for c in chains]
    assert min(pr.threshold_margin(c) for c in rounded) >= 1e-9
    assert [_str(g) for g in structures.annotate_sse(chains)] == [pr.psea(c) for c in rounded]


def test_argument_errors(gpu):
    """Each invalid argument returns -1 with its word in the message; nothing is written to the outputs."""
    lib = _binding.load()
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    ca = pr.ideal_helix(10)
    offs, lens = np.array([0, 4], np.int32), np.array([4, 6], np.int32)

    def call(ca=ca, offs=offs, lens=lens, n=2, sse="default", counts="default"):
        sse = np.full(10, -7, np.int8) if isinstance(sse, str) else sse
        counts = np.full((2, 2), -7, np.int32) if isinstance(counts, str) else counts
        rc = lib.fd_annotate_sse(0, P(ca), P(offs), P(lens), n, P(sse), P(counts))
        return rc, lib.fd_last_error(), sse, counts

    rc, _, sse, counts = call()
    assert rc == 0 and (sse == 0).all() and (counts == 0).all()
    rc, _, sse, counts = call(counts=None)   # counts_out = NULL: labels only
    assert rc == 0 and (sse == 0).all()
    rc, _, sse, counts = call(ca=np.ascontiguousarray(pr.ideal_helix(24)), offs=np.array([0], np.int32),
                              lens=np.array([24], np.int32), n=1, sse=np.full(24, -7, np.int8), counts=None)
    assert rc == 0 and sse.tolist() == [0] + [1] * 22 + [0]
    bad_nan, bad_inf, bad_far = ca.copy(), ca.copy(), ca.copy()
    bad_nan[7, 1], bad_inf[0, 0], bad_far[9, 2] = np.nan, -np.inf, 1.5e6
    for kw, word in [(dict(ca=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(sse=None), b"null"),
                     (dict(n=0), b"n_chains"), (dict(n=-3), b"n_chains"),
                     (dict(lens=np.array([4, 0], np.int32)), b"lens"), (dict(lens=np.array([2049, 6], np.int32)), b"lens"),
                     (dict(offs=np.array([0, 3], np.int32)), b"offsets"), (dict(offs=np.array([6, 0], np.int32)), b"offsets"),
                     (dict(offs=np.array([0, 5], np.int32)), b"offsets"),
                     (dict(ca=bad_nan), b"finite"), (dict(ca=bad_inf), b"finite"), (dict(ca=bad_far), b"1e6")]:
        rc, msg, sse, counts = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert sse is None or (sse == -7).all()
        assert (counts == -7).all()


def test_1crn_rebuilt_by_nerf(gpu):
    """1CRN featurised, rebuilt by NeRF and annotated: two helices and one strand."""
    df = structures.featurize([FIXTURES[0]])[0]
    xyz = nerf.build_backbones([df.values], list(df.columns), center_coords=False)[0]
    labels = _str(structures.annotate_sse([xyz[1::3]])[0])
    _record("psea_1crn_rebuilt", labels=labels)
    assert tuple(structures.count_secondary_structures([xyz[1::3]])[0]) == (2, 1)


def test_files_and_cooccurrence(gpu, tmp_path):
    assert structures.count_structures_in_pdb(FIXTURES[0]) == (2, 1)
    assert structures.count_structures_in_pdb(FIXTURES[1]) == (1, 0)
    two_models = tmp_path / "two_models.pdb"
    body = "".join(line for line in open(FIXTURES[1]) if line.startswith("ATOM"))
    two_models.write_text(f"MODEL        1\n{body}ENDMDL\nMODEL        2\n{body}ENDMDL\n")
    assert structures.count_structures_in_pdb(str(two_models)) == (-1, -1)
    out, pdf = tmp_path / "counts.json", tmp_path / "plot.pdf"
    alpha, beta = structures.ss_cooccurrence([FIXTURES[0], str(two_models), FIXTURES[1]], json_file=str(out), outpdf=str(pdf))
    assert alpha.tolist() == [2, 1] and beta.tolist() == [1, 0]
    assert json.load(open(out)) == WANT_JSON
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert not pdf.exists()
    else:
        assert pdf.stat().st_size > 0
    alpha, beta = structures.ss_cooccurrence(FIXTURES, max_seq_len=30)   # 1CRN has 46 residues
    assert alpha.tolist() == [1] and beta.tolist() == [0]


def test_annot_cli(gpu, tmp_path):
    """bin/annot_secondary_structures.py on the fixtures: exit 0 and the JSON of ss_cooccurrence."""
    cli = os.path.join(REPO, "bin", "annot_secondary_structures.py")
    out = tmp_path / "counts.json"
    r = subprocess.run([sys.executable, cli, *FIXTURES, str(tmp_path / "plot.pdf"), "--json", str(out), "--title", "fixtures"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.load(open(out)) == WANT_JSON


def test_sample_cli_psea(gpu, tmp_path):
    """bin/sample.py --psea on the toy model of test_from_dir_lightning_checkpoint_and_cli: exit 0, and
    plots/ss_cooccurrence_sampled.json holds, per written file, the counts of that file's CA atoms."""
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    out = str(tmp_path / "out")
    cli = os.path.join(REPO, "bin", "sample.py")
    r = subprocess.run([sys.executable, cli, "-m", mdir, "-o", out, "-n", "2", "-l", "9", "12", "-b", "4", "--seed", "3", "--psea"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "plots", "sampled_angles", "sampled_pdb"]
    plots = sorted(os.listdir(os.path.join(out, "plots")))
    assert "ss_cooccurrence_sampled.json" in plots and set(plots) <= {"ss_cooccurrence_sampled.json", "ss_cooccurrence_sampled.pdf"}
    res = json.load(open(os.path.join(out, "plots", "ss_cooccurrence_sampled.json")))
    names = [f"generated_{i}.pdb" for i in range(6)]
    assert list(res) == names
    traces = [ac.read_pdb_backbone(os.path.join(out, "sampled_pdb", f))[1::3] for f in names]
    assert [len(t) for t in traces] == [9, 9, 10, 10, 11, 11]
    assert [res[f] for f in names] == structures.count_secondary_structures(traces).tolist()
