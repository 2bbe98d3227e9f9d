"""fd_tm_score and the TM-score path of structures.py on the device: invariances, the returned transform, the bound
that ties it to fd_superpose_rmsd, a two-domain case that plain superposition misses, the numpy restatement of the
search (tests/tm_reference.py), determinism, argument errors, 1CRN rebuilt by NeRF, the TmScorer through
get_reconstruction_error and bin/partial_noise_reconstruct.py --tmscore.  Needs an MI355X:  pytest -m gpu"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tm_reference as tr
from conftest import REPO
from foldingdiff_amd import _binding, datasets, nerf, sampling, structures
from test_structures_gpu import FIXTURES, _toy_model

pytestmark = pytest.mark.gpu


def _record(name, **kw):
    """Print a measured value (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps({k: float(v) for k, v in kw.items()}, sort_keys=True))


def _noised(rng, a, sigma):
    return a @ tr.rotation(rng).T + rng.uniform(-40, 40, 3) + rng.standard_normal(a.shape) * sigma


def test_identity_and_invariance(gpu):
    """b = a rotated and translated: TM = 1 within 1e-12 and the transform maps a onto b within 1e-9 A, for ragged
    lengths up to FDMI_TM_MAX_LEN in one call."""
    rng = np.random.default_rng(0)
    lens = [1, 2, 3, 4, 5, 21, 22, 50, 127, 128, 129, 512, 2048]
    a_list = [tr.ca_chain(rng, n) + rng.uniform(-20, 20, 3) for n in lens]
    Rs = [tr.rotation(rng) for _ in lens]
    ts = [rng.uniform(-60, 60, 3) for _ in lens]
    b_list = [a @ R.T + t for a, R, t in zip(a_list, Rs, ts)]
    tm, R, t = structures.tm_score(a_list, b_list, stride=64, return_transform=True)
    assert tm.shape == (len(lens),) and R.shape == (len(lens), 3, 3) and t.shape == (len(lens), 3)
    dev = max(np.abs(a @ R[i].T + t[i] - b).max() for i, (a, b) in enumerate(zip(a_list, b_list)))
    _record("tm_identity", max_tm_deficit=np.abs(tm - 1.0).max(), max_map=dev)
    assert np.abs(tm - 1.0).max() <= 1e-12
    assert dev <= 1e-9
    for Ri in R:   # proper rotations
        assert np.abs(Ri @ Ri.T - np.eye(3)).max() < 1e-12 and np.linalg.det(Ri) > 0


def test_transform_is_honest(gpu):
    """TM recomputed in numpy from the returned R and t reproduces the returned TM within 1e-12 (noised pairs)."""
    rng = np.random.default_rng(1)
    lens = [3, 8, 30, 64, 100, 128, 200]
    a_list = [tr.ca_chain(rng, n) for n in lens]
    b_list = [_noised(rng, a, s) for a, s in zip(a_list, [0.3, 1.0, 2.0, 3.0, 5.0, 8.0, 4.0])]
    norm = [n + k for k, n in enumerate(lens)]
    tm, R, t = structures.tm_score(a_list, b_list, norm_lens=norm, return_transform=True)
    worst = max(abs(tr.tm_of(a, b, R[i], t[i], Ln=norm[i]) - tm[i]) for i, (a, b) in enumerate(zip(a_list, b_list)))
    _record("tm_transform_honest", max=worst)
    assert worst <= 1e-12
    assert ((tm > 0) & (tm <= 1)).all()


def test_search_beats_plain_superposition(gpu):
    """TM >= (n / Ln) / (1 + rmsd^2 / d0^2) with the RMSD from fd_superpose_rmsd: Jensen's inequality at the
    full-length seed, whose fit is the RMSD superposition."""
    rng = np.random.default_rng(2)
    lens = list(rng.integers(3, 300, 40))
    a_list = [tr.ca_chain(rng, n) for n in lens]
    b_list = [_noised(rng, a, rng.uniform(0.3, 10.0)) for a in a_list]
    norm = [n + int(rng.integers(0, 30)) for n in lens]
    rmsd = structures.superposed_rmsd(a_list, b_list)
    tm = structures.tm_score(a_list, b_list, norm_lens=norm)
    bound = np.array([(n / L) / (1 + r * r / structures.tm_d0(L) ** 2) for n, L, r in zip(lens, norm, rmsd)])
    _record("tm_vs_rmsd_bound", min_margin=(tm - bound).min())
    assert (tm >= bound - 1e-12).all()


def test_two_domains(gpu):
    """n = 120, the second half rotated 90 degrees about residue 60 and moved 10 A: the all-residue fit scores below
    0.45 (a score taken at the RMSD superposition fails), the search at least 0.5."""
    a = tr.ca_chain(np.random.default_rng(0), 120)
    b = tr.two_domain(a, 60)
    Rk, tk = tr.kabsch(a, b)
    plain = tr.tm_of(a, b, Rk, tk)
    tm = structures.tm_score([a], [b])[0]
    _record("tm_two_domains", tm=tm, all_residue_fit=plain)
    assert plain < 0.45
    assert tm >= 0.5


def _restatement_cases(rng):
    sizes = [3, 4, 5, 8, 21, 22, 46, 100, 127, 128, 129, 512]
    cases = []
    for k in range(216):
        n = sizes[k % len(sizes)]
        a = tr.ca_chain(rng, n)
        if k % 7 == 3 and n >= 20:
            b = tr.two_domain(a, n // 2, angle_deg=rng.uniform(40, 120), shift=rng.uniform(3, 12), axis=rng.standard_normal(3))
            b = _noised(rng, b, rng.uniform(0.3, 2.0))
        else:
            b = _noised(rng, a, rng.uniform(0.3, 8.0))
        Ln = n + (int(rng.integers(1, 40)) if k % 3 == 0 else 0)
        cases.append((a, b, Ln))
    return cases


def test_against_restatement(gpu):
    """216 seeded pairs (lengths 3..512, noise 0.3-8 A, two-domain cases, Ln > n for a third of them) at stride 5 and
    every length but 512 at stride 1: |TM - restatement| <= 1e-9."""
    cases = _restatement_cases(np.random.default_rng(3))
    worst = 0.0
    for stride in (5, 1):
        sub = [c for c in cases if stride == 5 or len(c[0]) < 512]
        got = structures.tm_score([c[0] for c in sub], [c[1] for c in sub], norm_lens=[c[2] for c in sub], stride=stride)
        want = np.array([tr.tm_search(a, b, Ln=Ln, stride=stride)[0] for a, b, Ln in sub])
        worst = max(worst, np.abs(got - want).max())
        _record(f"tm_vs_restatement_stride{stride}", max=np.abs(got - want).max(), pairs=len(sub))
    assert worst <= 1e-9


def test_deterministic_and_batch_invariant(gpu):
    """Two identical calls are bitwise equal, and so is each pair scored alone and inside the batch."""
    cases = _restatement_cases(np.random.default_rng(4))[:36]
    A, B, L = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    t1, R1, s1 = structures.tm_score(A, B, norm_lens=L, stride=3, return_transform=True)
    t2, R2, s2 = structures.tm_score(A, B, norm_lens=L, stride=3, return_transform=True)
    assert np.array_equal(t1, t2) and np.array_equal(R1, R2) and np.array_equal(s1, s2)
    for i in (0, 5, 17, 35):
        ti, Ri, si = structures.tm_score([A[i]], [B[i]], norm_lens=[L[i]], stride=3, return_transform=True)
        assert ti[0] == t1[i] and np.array_equal(Ri[0], R1[i]) and np.array_equal(si[0], s1[i])


def test_argument_errors(gpu):
    """Each invalid argument returns -1 with a message; nothing is written to the outputs."""
    lib = _binding.load()
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    a = np.random.default_rng(5).standard_normal((10, 3))
    offs, lens = np.array([0, 4], np.int32), np.array([4, 6], np.int32)

    def call(a=a, b=a, offs=offs, lens=lens, norm=None, n=2, stride=1, out="default", transform=None):
        tm = np.full(2, -7.0) if isinstance(out, str) else out
        rc = lib.fd_tm_score(0, P(a), P(b), P(offs), P(lens), P(norm), n, stride, P(tm), P(transform))
        return rc, lib.fd_last_error(), tm

    assert call()[0] == 0
    bad_nan = a.copy()
    bad_nan[7, 1] = np.nan
    bad_inf = a.copy()
    bad_inf[0, 0] = -np.inf
    for kw, word in [(dict(a=None), b"null"), (dict(b=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"),
                     (dict(out=None), b"null"), (dict(n=0), b"n_pairs"), (dict(stride=0), b"stride"),
                     (dict(lens=np.array([4, 0], np.int32)), b"lens"), (dict(lens=np.array([2049, 6], np.int32)), b"lens"),
                     (dict(offs=np.array([0, 5], np.int32)), b"offsets"), (dict(norm=np.array([4, 5], np.int32)), b"norm_lens"),
                     (dict(a=bad_nan), b"finite"), (dict(b=bad_inf), b"finite")]:
        rc, msg, tm = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        if tm is not None:
            assert (tm == -7.0).all()


def test_1crn_round_trip(gpu):
    """The reference's NeRF test (tests/test_nerf.py:89-90, TM-score 1.0): 1CRN featurised, rebuilt by NeRF, its CA
    atoms against the file's CA atoms."""
    df = structures.featurize([FIXTURES[0]])[0]
    xyz = nerf.build_backbones([df.values], list(df.columns), center_coords=False)[0]
    truth = structures.read_backbone(FIXTURES[0])[0]
    tm = structures.tm_score([xyz[1::3]], [truth[1::3]])[0]
    _record("tm_1crn_round_trip", deficit=1.0 - tm)
    assert tm >= 1.0 - 1e-9


def test_tm_scorer_through_reconstruction(gpu):
    """TmScorer on reconstructions at t = 5 of the fixtures and as the scorer of get_reconstruction_error: scores in
    (0, 1], the batch equals the per-item form; 1CRN trimmed to 32 residues has a coordinate score <= 32 / 46, equal to the restatement
    normalised by the file's 46 residues."""
    ds = structures.PdbAnglesOnlyDataset(FIXTURES, pad=32, min_length=0, trim_strategy="leftalign")
    assert sorted(ds.all_lengths) == [20, 46]
    noised = datasets.NoisedAnglesDataset(ds, dset_key="angles", timesteps=1000, beta_schedule="cosine")
    pm = _toy_model()
    torch.manual_seed(7)
    recon, truth, files = sampling.reconstruct(pm, noised, noise_timesteps=5, bs=8)
    s, c = structures.tm_scorer.score_batch(recon, truth, files)
    assert s.shape == c.shape == (2,)
    assert ((s > 0) & (s <= 1)).all() and ((c > 0) & (c <= 1)).all()
    for i in range(2):
        assert structures.tm_scorer(recon[i], truth[i], files[i]) == (s[i], c[i])
    i = files.index(FIXTURES[0])
    assert len(recon[i]) == 32
    names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-full-angles"]
    ca = nerf.build_backbones([recon[i]], names)[0][1::3]
    file_ca = structures.read_backbone(FIXTURES[0])[0][1::3]
    want = tr.tm_search(ca, file_ca[:32], Ln=46)[0]
    _record("tm_scorer_1crn_trimmed", coord=c[i], restatement=want)
    assert c[i] <= 32 / 46 and abs(c[i] - want) <= 1e-9
    scores, coord = sampling.get_reconstruction_error(pm, noised, noise_timesteps=5, bs=8, scorer=structures.tm_scorer)
    assert scores.shape == coord.shape == (2,)
    assert ((scores > 0) & (scores <= 1)).all() and ((coord > 0) & (coord <= 1)).all()


def test_partial_noise_reconstruct_cli_tmscore(gpu, tmp_path):
    """bin/partial_noise_reconstruct.py --tmscore: exit 0; "tmscores" and "tmscores_coord" cover the files of "rmsd",
    with values in (0, 1]."""
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    out = str(tmp_path / "scores.json")
    cli = os.path.join(REPO, "bin", "partial_noise_reconstruct.py")
    r = subprocess.run([sys.executable, cli, *FIXTURES, out, "-t", "5", "-m", mdir, "-d", "0", "--tmscore"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    assert res["timesteps"] == 5 and res["model"] == mdir
    assert sorted(res["rmsd"]) == sorted(FIXTURES) == sorted(res["rmsd_coord"])
    for key in ("tmscores", "tmscores_coord"):
        assert sorted(res[key]) == sorted(res["rmsd"])
        assert all(0 < v <= 1 for v in res[key].values())
