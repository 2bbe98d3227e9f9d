"""fd_tm_align and the alignment path of structures.py on the device: parity with the numpy restatement
(tests/tmalign_reference.py) in score and map, the returned transform and map recomputed on the host, the tie to
fd_tm_score, deletion and hinge cases, invariance, determinism, mixed lengths, argument errors, the Python helpers and
the two CLIs.  Needs an MI355X:  pytest -m gpu"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import tm_reference as tr
import tmalign_reference as ta
from conftest import REPO
from foldingdiff_amd import _binding, structures
from test_structures_gpu import FIXTURES

pytestmark = pytest.mark.gpu


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps({k: float(v) for k, v in kw.items()}, sort_keys=True))


def _norm(case):
    return len(case[2]) if case[3] is None else case[3]


@pytest.fixture(scope="module")
def parity(gpu):
    """The parity set aligned on the device, one call per max_iter: (cases, tm, R, t, maps)."""
    cases = ta.parity_set()
    tm, R, t, maps = np.zeros(len(cases)), [None] * len(cases), [None] * len(cases), [None] * len(cases)
    for it in sorted({c[4] for c in cases}):
        idx = [k for k, c in enumerate(cases) if c[4] == it]
        got = structures.tm_align([cases[k][1] for k in idx], [cases[k][2] for k in idx], norm_lens=[_norm(cases[k]) for k in idx],
                                  max_iter=it, return_transform=True, return_map=True)
        for q, k in enumerate(idx):
            tm[k], R[k], t[k], maps[k] = got[0][q], got[1][q], got[2][q], got[3][q]
    return cases, tm, R, t, maps


def test_against_restatement(parity):
    """The parity set: |TM - restatement| <= 1e-9 and the maps equal element for element."""
    cases, tm, _, _, maps = parity
    want = ta.parity_results()
    dev = np.array([abs(tm[k] - want[k]["tm"]) for k in range(len(cases))])
    wrong = [k for k in range(len(cases)) if not np.array_equal(maps[k], want[k]["map"])]
    _record("tmalign_vs_restatement", max=dev.max(), pairs=len(cases), maps_differ=len(wrong),
            min_margin=min(r["margin"] for r in want))
    assert not wrong, [(k, cases[k][0], len(cases[k][1]), len(cases[k][2])) for k in wrong]
    assert dev.max() <= 1e-9, [(k, cases[k][0], dev[k]) for k in np.flatnonzero(dev > 1e-9)]


def test_result_is_honest(parity):
    """TM recomputed in numpy from the returned R, t and map equals the returned TM within 1e-12; R is a proper
    rotation; the map is strictly increasing and within the second chain."""
    cases, tm, R, t, maps = parity
    worst = 0.0
    for k, c in enumerate(cases):
        worst = max(worst, abs(ta.tm_of_map(c[1], c[2], R[k], t[k], maps[k], _norm(c)) - tm[k]))
        assert np.abs(R[k] @ R[k].T - np.eye(3)).max() < 1e-12 and np.linalg.det(R[k]) > 0
        m = maps[k][maps[k] >= 0]
        assert maps[k].shape == (len(c[1]),) and len(m) >= 1
        assert (np.diff(m) > 0).all() and m.max() < len(c[2]) and maps[k].min() >= -1
    _record("tmalign_honest", max=worst)
    assert worst <= 1e-12


def test_tie_to_tm_score(parity):
    """tm_score of the aligned pairs at the coarse stride equals the returned TM within 1e-9; at stride 1 it is
    >= returned - 1e-12, and polish=True returns that stride-1 value."""
    cases, tm, _, _, maps = parity
    sub = list(range(0, len(cases) - 1, 3)) + [len(cases) - 1]
    xa = [cases[k][1][maps[k] >= 0] for k in sub]
    ya = [cases[k][2][maps[k][maps[k] >= 0]] for k in sub]
    nl = [_norm(cases[k]) for k in sub]
    coarse = np.array([structures.tm_score([x], [y], norm_lens=[n], stride=structures.tm_align_stride(len(x)))[0]
                       for x, y, n in zip(xa, ya, nl)])
    fine = structures.tm_score(xa, ya, norm_lens=nl, stride=1)
    _record("tmalign_vs_tm_score", coarse=np.abs(coarse - tm[sub]).max(), fine_gain=(fine - tm[sub]).max())
    assert np.abs(coarse - tm[sub]).max() <= 1e-9
    assert (fine >= tm[sub] - 1e-12).all()
    ten = [k for k in sub if cases[k][4] == 10]
    polished = structures.tm_align([cases[k][1] for k in ten], [cases[k][2] for k in ten], norm_lens=[_norm(cases[k]) for k in ten],
                                   polish=True)
    assert np.array_equal(polished, fine[[sub.index(k) for k in ten]])


def test_deletion_and_hinge(gpu):
    """As on the host: a deletion scores 1 within 1e-12 with the map skipping exactly the deleted residues; a hinged
    chain with a deletion in its first domain scores at least the intact domain's share."""
    dels = [ta.deletion_pair(np.random.default_rng(n), n) for n in (20, 64, 100)]
    hinges = [ta.hinge_pair(np.random.default_rng(0), n) for n in (64, 100)]
    A = [d[0] for d in dels] + [h[0] for h in hinges]
    B = [d[1] for d in dels] + [h[1] for h in hinges]
    tm, maps = structures.tm_align(A, B, return_map=True)
    for k, (a, b, cut) in enumerate(dels):
        want = np.full(len(a), -1)
        want[np.delete(np.arange(len(a)), cut)] = np.arange(len(b))
        assert abs(tm[k] - 1.0) <= 1e-12 and maps[k].tolist() == want.tolist()
    for k, (a, b) in enumerate(hinges, start=len(dels)):
        _record(f"tmalign_hinge_{len(a)}", tm=tm[k], bar=(len(a) // 2) / len(b))
        assert tm[k] >= (len(a) // 2) / len(b)


def test_invariance(parity):
    """A rigid motion of either chain changes TM by <= 1e-9 and leaves the map unchanged."""
    cases, tm, _, _, maps = parity
    rng = np.random.default_rng(7)
    sub = [k for k in range(len(cases)) if cases[k][4] == 10][::2]
    moved_a = [cases[k][1] @ tr.rotation(rng).T + rng.uniform(-50, 50, 3) for k in sub]
    moved_b = [cases[k][2] @ tr.rotation(rng).T + rng.uniform(-50, 50, 3) for k in sub]
    nl = [_norm(cases[k]) for k in sub]
    worst = 0.0
    for A, B in ((moved_a, [cases[k][2] for k in sub]), ([cases[k][1] for k in sub], moved_b)):
        got, m = structures.tm_align(A, B, norm_lens=nl, return_map=True)
        worst = max(worst, np.abs(got - tm[sub]).max())
        assert all(np.array_equal(x, maps[k]) for x, k in zip(m, sub))
    _record("tmalign_invariance", max=worst)
    assert worst <= 1e-9


def test_deterministic_and_batch_invariant(parity):
    """Two identical calls are bitwise equal; a pair scored alone equals the same pair inside a batch (tm, transform,
    map); pairwise_tm over 12 chains equals 66 single calls."""
    cases, tm, R, t, maps = parity
    ten = [k for k in range(len(cases)) if cases[k][4] == 10]
    A, B, nl = [cases[k][1] for k in ten], [cases[k][2] for k in ten], [_norm(cases[k]) for k in ten]
    again = structures.tm_align(A, B, norm_lens=nl, return_transform=True, return_map=True)
    assert np.array_equal(again[0], tm[ten])
    assert all(np.array_equal(again[1][q], R[k]) and np.array_equal(again[2][q], t[k]) and np.array_equal(again[3][q], maps[k])
               for q, k in enumerate(ten))
    for k in (ten[1], ten[17], ten[38]):
        one = structures.tm_align([cases[k][1]], [cases[k][2]], norm_lens=[_norm(cases[k])], return_transform=True, return_map=True)
        assert one[0][0] == tm[k] and np.array_equal(one[1][0], R[k]) and np.array_equal(one[2][0], t[k])
        assert np.array_equal(one[3][0], maps[k])
    rng = np.random.default_rng(8)
    chains = [tr.ca_chain(rng, int(n)) for n in rng.integers(8, 60, 12)]
    all_pairs = structures.pairwise_tm(chains)
    assert all_pairs.shape == (66,)
    singles = [structures.tm_align([chains[i]], [chains[j]])[0] for i in range(12) for j in range(i + 1, 12)]
    assert np.array_equal(all_pairs, np.array(singles))
    assert np.array_equal(structures.pairwise_tm(chains, chunk=7), all_pairs)   # chunking changes nothing


def test_mixed_lengths(gpu):
    """Chains of 1, 2, 3, 5, 128, 129 and 512 residues in one call, each against a rotated copy of itself: 1 within
    1e-9, every residue aligned with itself."""
    rng = np.random.default_rng(9)
    lens = [1, 2, 3, 5, 128, 129, 512]
    A = [tr.ca_chain(rng, n) + rng.uniform(-20, 20, 3) for n in lens]
    B = [a @ tr.rotation(rng).T + rng.uniform(-60, 60, 3) for a in A]
    tm, maps = structures.tm_align(A, B, max_iter=2, return_map=True)
    _record("tmalign_mixed_lengths", max_deficit=np.abs(tm - 1.0).max())
    assert np.abs(tm - 1.0).max() <= 1e-9
    assert all(m.tolist() == list(range(n)) for m, n in zip(maps, lens))


def test_argument_errors(gpu):
    """Each invalid argument returns -1 with a message; nothing is written to the outputs."""
    lib = _binding.load()
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    ca = np.random.default_rng(5).standard_normal((10, 3))
    offs, lens = np.array([0, 4], np.int32), np.array([4, 6], np.int32)
    pa, pb = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    moff = np.array([0, 4], np.int64)
    long_ca = np.zeros((517, 3))

    def call(ca=ca, offs=offs, lens=lens, nc=2, pa=pa, pb=pb, norm=None, n=2, max_iter=3, out="default", moff=moff, use_map=True):
        tm = np.full(2, -7.0) if isinstance(out, str) else out
        T, n_ali, amap = np.full((2, 12), -7.0), np.full(2, -7, np.int32), np.full(10, -7, np.int32)
        rc = lib.fd_tm_align(0, P(ca), P(offs), P(lens), nc, P(pa), P(pb), P(norm), n, max_iter, P(tm), P(T), P(n_ali), P(moff),
                             P(amap) if use_map else None)
        return rc, lib.fd_last_error(), [x for x in (tm, T, n_ali, amap) if x is not None]

    rc, _, outs = call()
    assert rc == 0 and all((x != -7).all() for x in outs)
    bad_nan = ca.copy()
    bad_nan[7, 1] = np.nan
    bad_inf = ca.copy()
    bad_inf[0, 0] = -np.inf
    for kw, word in [(dict(ca=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(pa=None), b"null"),
                     (dict(pb=None), b"null"), (dict(out=None), b"null"), (dict(use_map=False), b"null"), (dict(moff=None), b"null"),
                     (dict(n=0), b"n_pairs"), (dict(nc=0), b"n_chains"), (dict(max_iter=0), b"max_iter"),
                     (dict(lens=np.array([4, 0], np.int32)), b"lens"),
                     (dict(ca=long_ca, lens=np.array([513, 4], np.int32), offs=np.array([0, 513], np.int32)), b"lens"),
                     (dict(offs=np.array([0, 5], np.int32)), b"offsets"),
                     (dict(pa=np.array([0, 2], np.int32)), b"chain index"), (dict(pb=np.array([-1, 0], np.int32)), b"chain index"),
                     (dict(norm=np.array([4, 3], np.int32)), b"norm_lens"), (dict(moff=np.array([0, 5], np.int64)), b"map_offsets"),
                     (dict(ca=bad_nan), b"finite"), (dict(ca=bad_inf), b"finite")]:
        rc, msg, outs = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert all((x == -7).all() for x in outs), kw


def test_max_tm_across_refs(gpu):
    """6 queries x 9 references: the max and argmax of the 54 tm_align scores (normalised by the reference)."""
    rng = np.random.default_rng(10)
    refs = [tr.ca_chain(rng, int(n)) for n in rng.integers(20, 70, 9)]
    moved = [np.delete(refs[k], [5, 6, 7], axis=0) @ tr.rotation(rng).T + rng.uniform(-30, 30, 3) for k in (4, 0, 7)]
    queries = moved + [tr.ca_chain(rng, int(n)) for n in (15, 40, 66)]
    best, which = structures.max_tm_across_refs(queries, refs)
    table = np.array([[structures.tm_align([q], [r])[0] for r in refs] for q in queries])
    assert np.array_equal(best, table.max(1)) and np.array_equal(which, table.argmax(1))
    assert which[:3].tolist() == [4, 0, 7]   # a reference with three residues deleted finds its origin ...
    assert np.abs(best[:3] - np.array([1 - 3 / len(refs[k]) for k in (4, 0, 7)])).max() <= 1e-9   # ... at (n - 3) / n


def test_cli_tmscore_training(gpu, tmp_path):
    """bin/tmscore_training.py on the two fixture files with --train naming the same two: exit 0, both JSON files with
    the file stems as keys, every score 1 within 1e-9, each file's best match itself."""
    sampled = tmp_path / "sampled"
    sampled.mkdir()
    for f in FIXTURES:
        shutil.copy(f, sampled)
    listing = tmp_path / "train.txt"
    listing.write_text("\n".join(FIXTURES) + "\n")
    cli = os.path.join(REPO, "bin", "tmscore_training.py")
    stems = sorted(os.path.splitext(os.path.basename(f))[0] for f in FIXTURES)
    r = subprocess.run([sys.executable, cli, "-d", str(sampled), "--train", str(listing)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    scores = json.load(open(sampled / "tm_scores.json"))
    refs = json.load(open(sampled / "tm_scores_ref.json"))
    assert sorted(scores) == stems == sorted(refs)
    for k in stems:
        assert abs(scores[k] - 1.0) <= 1e-9
        assert os.path.splitext(os.path.basename(refs[k]))[0] == k


def test_cli_hclust(gpu, tmp_path):
    """bin/hclust_structures.py on the two fixture files: exit 0, a symmetric distance CSV with a zero diagonal and
    the linkage matrix of two leaves."""
    d = tmp_path / "pdbs"
    d.mkdir()
    for k, f in enumerate(FIXTURES):
        shutil.copy(f, d / f"sample_{k}.pdb")
    out = tmp_path / "hclust.pdf"
    cli = os.path.join(REPO, "bin", "hclust_structures.py")
    r = subprocess.run([sys.executable, cli, "--dirname", str(d), "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    dist = pd.read_csv(tmp_path / "hclust_dist.csv", index_col=0)
    assert list(dist.index) == list(dist.columns) == ["sample_0", "sample_1"]
    assert np.array_equal(dist.values, dist.values.T) and (np.diag(dist.values) == 0).all()
    assert 0 < dist.values[0, 1] < 1
    link = np.loadtxt(tmp_path / "hclust_linkage.csv", delimiter=",", ndmin=2)
    assert link.shape == (1, 4) and link[0, 2] == pytest.approx(dist.values[0, 1]) and link[0, 3] == 2
