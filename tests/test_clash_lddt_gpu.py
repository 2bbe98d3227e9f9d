"""fd_backbone_clashes and fd_lddt on the device: every count and flag against the reference's own clash counts
(tests/golden/ref_clashes.npz) and the numpy restatement (tests/clash_lddt_reference.py), with exact equality of integers
-- every input is first checked to keep each decision at least 1e-9 from its threshold -- then invariances, non-default
parameters, the scorer, and the command lines.  Needs an MI355X:  pytest -m gpu"""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import clash_lddt_reference as cr
from conftest import REPO, golden
from foldingdiff_amd import angles_and_coords as ac
from foldingdiff_amd import datasets, nerf, sampling, structures
from test_structures_gpu import FIXTURES, _toy_model

pytestmark = pytest.mark.gpu

# residues: 3, 6, 63, 66, 255, 258, 1023, 1026 and 2049 atoms -- a block of 256 atoms (85 residues in fd_lddt) and a tile
# of 1024 atoms end inside a residue, and the longest chain needs more than two tiles
BACKBONE_LENS = [1, 2, 21, 22, 85, 86, 341, 342, 683]
CA_LENS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps(kw, sort_keys=True, default=float))


def clash_cases():
    rng = np.random.default_rng(11)
    chains = [cr.walk_backbone(rng, n) for n in BACKBONE_LENS]
    return chains, [cr.clashes(c) for c in chains]


def lddt_cases(A):
    rng = np.random.default_rng(12 + A)
    refs = [cr.walk_backbone(rng, n if A == 3 else (n + 2) // 3)[: n * A] for n in (BACKBONE_LENS if A == 3 else CA_LENS)]
    models = [cr.jittered_model(rng, r) for r in refs]
    return models, refs, [cr.lddt_counts(m, r, atoms_per_res=A) for m, r in zip(models, refs)]


@pytest.fixture(scope="module")
def walks():
    """(chains, the restatement's (count, flags, margin) of each).  Computed once; the tests leave it unchanged."""
    return clash_cases()


@pytest.fixture(scope="module")
def lddt_sets():
    """{A: (models, refs, the restatement's ((conserved, total), per residue, margin) of each pair)}."""
    return {A: lddt_cases(A) for A in (1, 3)}


def test_clashes_on_the_golden_chains(gpu):
    """The six backbones the reference's count_clashes was run on, in one call: its counts and its flags; the same chains
    permuted give the permuted results; a second call gives the same bytes."""
    g = golden("ref_clashes.npz")
    k = len(g["names"])
    chains = [g[f"xyz_{i}"] for i in range(k)]
    counts, flags = structures.count_clashes(chains, alpha=float(g["alpha"]), return_flags=True)
    assert counts.tolist() == g["counts"].tolist()
    for i in range(k):
        assert flags[i].dtype == bool and (flags[i] == g[f"flags_{i}"]).all(), str(g["names"][i])
    perm = [4, 2, 5, 0, 3, 1]
    counts_p, flags_p = structures.count_clashes([chains[i] for i in perm], return_flags=True)
    assert counts_p.tolist() == [int(counts[i]) for i in perm]
    assert all((fp == flags[i]).all() for fp, i in zip(flags_p, perm))
    again, flags_again = structures.count_clashes(chains, return_flags=True)
    assert again.tobytes() == counts.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flags_again, flags))
    assert structures.count_clashes(chains).tolist() == counts.tolist()   # without the flags


def test_clashes_across_block_and_tile_edges(gpu, walks):
    chains, want = walks
    assert [len(c) for c in chains] == [3, 6, 63, 66, 255, 258, 1023, 1026, 2049]
    margin = min(w[2] for w in want)
    _record("clash_walks", margin=margin, counts=[w[0] for w in want])
    assert margin >= cr.MIN_MARGIN
    for c, w in zip(chains, want):
        if len(c) >= 63:
            assert 0 < w[0] < len(c)   # some atoms clash and some do not
    counts, flags = structures.count_clashes(chains, return_flags=True)
    assert counts.tolist() == [w[0] for w in want]
    for f, w in zip(flags, want):
        assert (f == w[1]).all()


@pytest.mark.parametrize("A", [3, 1])
def test_lddt_across_block_and_tile_edges(gpu, lddt_sets, A):
    """Structure counts and per-residue counts equal the restatement's; every threshold decides both ways; the results
    do not depend on the order of the pairs; a model equal to its reference scores exactly 1."""
    models, refs, want = lddt_sets[A]
    assert [len(r) // A for r in refs] == (BACKBONE_LENS if A == 3 else CA_LENS)
    margin = min(w[2] for w in want)
    _record(f"lddt_walks_A{A}", margin=margin, counts=[w[0] for w in want])
    assert margin >= cr.MIN_MARGIN
    for m, r, w in zip(models[2:5], refs[2:5], want[2:5]):   # the jitter is drawn alike for every pair
        per_threshold = [cr.lddt_counts(m, r, atoms_per_res=A, thresholds=(tau,))[0][0] for tau in cr.THRESHOLDS]
        assert 0 < per_threshold[0] < per_threshold[1] < per_threshold[2] < per_threshold[3] < w[0][1]
    counts, res = structures.lddt(models, refs, atoms_per_res=A, per_residue=True, return_counts=True)
    assert counts.dtype == np.int64 and counts.tolist() == [list(w[0]) for w in want]
    for got, w in zip(res, want):
        assert got.shape == w[1].shape and (got == w[1]).all()
    scores, res_scores = structures.lddt(models, refs, atoms_per_res=A, per_residue=True)
    assert np.isnan(scores[0]) and np.isnan(res_scores[0]).all() and counts[0].tolist() == [0, 0]   # one residue
    for s, w in zip(scores[1:], want[1:]):
        assert s == w[0][0] / (4 * w[0][1])
    for rs, w in zip(res_scores[1:], want[1:]):
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.array_equal(rs, np.where(w[1][:, 1] > 0, w[1][:, 0] / (4.0 * w[1][:, 1]), np.nan), equal_nan=True)
    perm = [5, 8, 0, 3, 7, 1, 6, 2, 4]
    counts_p, res_p = structures.lddt([models[i] for i in perm], [refs[i] for i in perm], atoms_per_res=A, per_residue=True,
                                      return_counts=True)
    assert counts_p.tolist() == [counts[i].tolist() for i in perm]
    assert all((rp == res[i]).all() for rp, i in zip(res_p, perm))
    assert structures.lddt(models, refs, atoms_per_res=A, return_counts=True).tolist() == counts.tolist()   # no per-residue output
    same = structures.lddt(refs, refs, atoms_per_res=A)
    assert np.isnan(same[0]) and (same[1:] == 1.0).all()


def test_lddt_hand_case(gpu):
    ref = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0]], np.float32)
    model = np.array([[0, 0, 0], [10.4, 0, 0], [23, 0, 0]], np.float32)
    counts, res = structures.lddt([model], [ref], atoms_per_res=1, per_residue=True, return_counts=True)
    assert counts.tolist() == [[5, 2]] and res[0].tolist() == [[4, 1], [5, 2], [1, 1]]
    scores, res_scores = structures.lddt([model], [ref], atoms_per_res=1, per_residue=True)
    assert scores.tolist() == [0.625] and res_scores[0].tolist() == [1.0, 0.625, 0.25]
    single = structures.lddt([model[:1]], [ref[:1]], atoms_per_res=1, return_counts=True)
    assert single.tolist() == [[0, 0]] and np.isnan(structures.lddt([model[:1]], [ref[:1]], atoms_per_res=1)[0])


def test_non_default_parameters(gpu, walks, lddt_sets):
    chains = walks[0][4:8]
    want = [cr.clashes(c, alpha=0.5) for c in chains]
    assert min(w[2] for w in want) >= cr.MIN_MARGIN
    assert [w[0] for w in want] != [w[0] for w in walks[1][4:8]]
    assert structures.count_clashes(chains, alpha=0.5).tolist() == [w[0] for w in want]
    models, refs = lddt_sets[3][0][4:8], lddt_sets[3][1][4:8]
    for kw in (dict(radius=10.0), dict(thresholds=(1.0, 3.0))):
        want = [cr.lddt_counts(m, r, atoms_per_res=3, **kw) for m, r in zip(models, refs)]
        assert min(w[2] for w in want) >= cr.MIN_MARGIN
        counts, res = structures.lddt(models, refs, atoms_per_res=3, per_residue=True, return_counts=True, **kw)
        assert counts.tolist() == [list(w[0]) for w in want]
        assert all((got == w[1]).all() for got, w in zip(res, want))
        n_thr = len(kw.get("thresholds", cr.THRESHOLDS))
        assert structures.lddt(models, refs, atoms_per_res=3, **kw).tolist() == [w[0][0] / (n_thr * w[0][1]) for w in want]


def test_lddt_scorer_through_reconstruction(gpu):
    """LddtScorer on reconstructions at t = 5 of the fixtures and as the scorer of get_reconstruction_error: the batch
    equals the per-item form and the restatement on the backbones NeRF builds."""
    ds = structures.PdbAnglesOnlyDataset(FIXTURES, pad=32, min_length=0, trim_strategy="leftalign")
    noised = datasets.NoisedAnglesDataset(ds, dset_key="angles", timesteps=1000, beta_schedule="cosine")
    pm = _toy_model()
    torch.manual_seed(7)
    recon, truth, files = sampling.reconstruct(pm, noised, noise_timesteps=5, bs=8)
    s, c = structures.lddt_scorer.score_batch(recon, truth, files)
    assert s.shape == c.shape == (2,) and ((s > 0) & (s <= 1)).all() and ((c > 0) & (c <= 1)).all()
    names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-full-angles"]
    xyz = nerf.build_backbones(list(recon) + list(truth), names)
    for i in range(2):
        assert structures.lddt_scorer(recon[i], truth[i], files[i]) == (s[i], c[i])
        file_bb = structures.read_backbone(files[i])[0][: len(xyz[i])]
        for got, ref in ((s[i], xyz[2 + i]), (c[i], file_bb)):
            (cons, total), _, margin = cr.lddt_counts(xyz[i], ref)
            assert margin >= cr.MIN_MARGIN and got == cons / (4 * total)
    scores, coord = sampling.get_reconstruction_error(pm, noised, noise_timesteps=5, bs=8, scorer=structures.lddt_scorer)
    assert scores.shape == coord.shape == (2,) and ((scores > 0) & (scores <= 1)).all()


def _angle_frames(rng, lens):
    names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-full-angles"]
    return [pd.DataFrame(rng.uniform(-np.pi, np.pi, (n, 6)).astype(np.float32), columns=names) for n in lens]


def test_vdw_clashes_cli(gpu, tmp_path):
    """bin/vdw_clashes.py on files written by write_preds_pdb_folder: the counts of count_clashes on the coordinates
    read back, and their mean on the standard output."""
    files = ac.write_preds_pdb_folder(_angle_frames(np.random.default_rng(2), [9, 14, 23, 40]), str(tmp_path / "pdb"))
    assert all(files)
    want = structures.count_clashes([structures.read_backbone(f)[0] for f in files])
    assert structures.count_clashes_parallel(files, nthreads=3) == {f: int(c) for f, c in zip(files, want)}
    out = tmp_path / "clashes.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "vdw_clashes.py"), *files, "--json", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.load(open(out)) == {f: int(c) for f, c in zip(files, want)}
    assert float(r.stdout.strip().splitlines()[-1]) == float(np.mean(want))


def test_lddt_cli(gpu, tmp_path):
    """bin/lddt.py: <stem>.pdb of the sampled folder against every <stem>_*.pdb of the folded one, the folded file as the
    model; -1.0 for a folded file cut short; a sampled file without folded files does not appear."""
    rng = np.random.default_rng(4)
    sampled_dir, folded_dir = tmp_path / "sampled", tmp_path / "folded"
    files = ac.write_preds_pdb_folder(_angle_frames(rng, [12, 20, 31]), str(sampled_dir))
    os.makedirs(folded_dir)
    want = {}
    for f in files[:2]:
        stem = os.path.splitext(os.path.basename(f))[0]
        ref = structures.read_backbone(f)[0]
        want[stem] = {}
        for k in range(2):
            folded = str(folded_dir / f"{stem}_fold{k}.pdb")
            ac.write_coords_to_pdb(ref.astype(np.float64) + rng.normal(0, 0.8, ref.shape), folded)
            want[stem][f"{stem}_fold{k}"] = float(structures.lddt([structures.read_backbone(folded)[0]], [ref])[0])
    cut = str(folded_dir / "generated_1_short.pdb")
    lines = open(folded_dir / "generated_1_fold0.pdb").read().splitlines(keepends=True)
    open(cut, "w").writelines(lines[:30])
    want["generated_1"]["generated_1_short"] = -1.0
    assert all(0 < v < 1 for s in want.values() for k, v in s.items() if not k.endswith("_short"))
    out = tmp_path / "lddt.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "lddt.py"), str(sampled_dir), str(folded_dir), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.load(open(out)) == want


def _mini_model_dir(tmp_path):
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    return mdir


def test_sample_cli_clashes(gpu, tmp_path):
    """bin/sample.py --clashes on a toy model (T = 20, lengths 9 to 11): clash_counts.json holds, per written file, what
    bin/vdw_clashes.py counts on that file."""
    mdir = _mini_model_dir(tmp_path)
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "9", "12",
                        "-b", "4", "--seed", "3", "--clashes"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["clash_counts.json", "model_snapshot", "sampled_angles", "sampled_pdb"]
    res = json.load(open(os.path.join(out, "clash_counts.json")))
    names = [f"generated_{i}.pdb" for i in range(6)]
    assert list(res) == names
    files = [os.path.join(out, "sampled_pdb", f) for f in names]
    dump = tmp_path / "cli.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "vdw_clashes.py"), *files, "--json", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.load(open(dump)) == {f: res[os.path.basename(f)] for f in files}


def test_partial_noise_reconstruct_cli_lddt(gpu, tmp_path):
    """bin/partial_noise_reconstruct.py --lddt: "lddt" and "lddt_coord" next to the RMSDs, values in (0, 1], and no
    TM-score keys unless asked for."""
    mdir = _mini_model_dir(tmp_path)
    out = str(tmp_path / "scores.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "partial_noise_reconstruct.py"), *FIXTURES, out, "-t", "5", "-m",
                        mdir, "-d", "0", "--lddt"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    assert sorted(res) == ["lddt", "lddt_coord", "model", "rmsd", "rmsd_coord", "timesteps"]
    for key in ("lddt", "lddt_coord"):
        assert sorted(res[key]) == sorted(res["rmsd"]) == sorted(FIXTURES)
        assert all(0 < v <= 1 for v in res[key].values())
