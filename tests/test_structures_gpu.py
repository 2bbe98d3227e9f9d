"""fd_internal_coords / fd_superpose_rmsd and the structures.py path on the device: against fp64 numpy restatements,
against the reference's own NeRF output (tests/golden/ref_nerf.npz), and end to end through reconstruction and the
bin/partial_noise_reconstruct.py command line.  Needs an MI355X:  pytest -m gpu"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, golden
from foldingdiff_amd import datasets, modelling, nerf, sampling, structures

pytestmark = pytest.mark.gpu

FIXTURES = [os.path.join(GOLDEN, "1CRN.pdb"), os.path.join(GOLDEN, "all_residues.pdb")]


def _record(name, **kw):
    """Print a measured error (shown with ``pytest -s``)."""
    print(f"{name}: " + json.dumps({k: float(v) for k, v in kw.items()}, sort_keys=True))


def _np_features(xyz32):
    """fp64 numpy restatement of the feature table (an independent dihedral formula, arccos angles)."""
    X = np.asarray(xyz32, np.float64).reshape(-1, 3, 3)
    N, CA, Cc = X[:, 0], X[:, 1], X[:, 2]
    n = len(X)
    out = np.full((n, 9), np.nan)
    out[-1, :3] = 0.0

    def dist(a, b):
        return np.linalg.norm(a - b, axis=1)

    def ang(a, b, c):
        u, v = a - b, c - b
        return np.arccos(np.clip((u * v).sum(1) / np.linalg.norm(u, axis=1) / np.linalg.norm(v, axis=1), -1, 1))

    def dih(a, b, c, d):
        b0, b1, b2 = a - b, c - b, d - c
        b1 = b1 / np.linalg.norm(b1, axis=1, keepdims=True)
        v = b0 - (b0 * b1).sum(1, keepdims=True) * b1
        w = b2 - (b2 * b1).sum(1, keepdims=True) * b1
        return np.arctan2((np.cross(b1, v) * w).sum(1), (v * w).sum(1))

    if n > 1:
        out[:-1, 0] = dist(Cc[:-1], N[1:])
        out[:-1, 1] = dist(N[1:], CA[1:])
        out[:-1, 2] = dist(CA[1:], Cc[1:])
        out[1:, 3] = dih(Cc[:-1], N[1:], CA[1:], Cc[1:])
        out[:-1, 4] = dih(N[:-1], CA[:-1], Cc[:-1], N[1:])
        out[:-1, 5] = dih(CA[:-1], Cc[:-1], N[1:], CA[1:])
        out[:-1, 6] = ang(N[1:], CA[1:], Cc[1:])
        out[:-1, 7] = ang(CA[:-1], Cc[:-1], N[1:])
        out[:-1, 8] = ang(Cc[:-1], N[1:], CA[1:])
    return out


def _errors(got, want):
    """(max distance error, max circular angle error); NaN and 0.0 must sit exactly where ``want`` has them."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got == 0.0, want == 0.0)
    ok = ~np.isnan(want)
    d = np.abs(got - want)
    d[:, 3:] = np.abs((got[:, 3:] - want[:, 3:] + np.pi) % (2 * np.pi) - np.pi)
    d[~ok] = 0.0
    return d[:, :3].max(), d[:, 3:].max()


def _random_backbones(rng, lengths):
    """Random walks with bond lengths 1.2-1.6 A (so float32 outputs resolve 1e-6) and free bond directions."""
    out = []
    for n in lengths:
        steps = rng.standard_normal((3 * n, 3))
        steps *= rng.uniform(1.2, 1.6, (3 * n, 1)) / np.linalg.norm(steps, axis=1, keepdims=True)
        out.append((np.cumsum(steps, axis=0) + rng.uniform(-50, 50, 3)).astype(np.float32))
    return out


def test_internal_coords_vs_numpy(gpu):
    """Fixture proteins and 2500 random chains of 1..600 residues in ONE launch (ragged offsets) against the fp64
    numpy restatement: <= 1e-6 A / rad, NaN and 0.0 exactly where the reference pads."""
    chains = [structures.read_backbone(f)[0] for f in FIXTURES]
    rng = np.random.default_rng(11)
    lengths = np.concatenate([[1, 2, 3, 600], rng.integers(1, 601, 2496)])
    chains += _random_backbones(rng, lengths)
    got = structures.internal_coords(chains)
    assert len(got) == len(chains) == 2502
    worst_d = worst_a = 0.0
    for c, g in zip(chains, got):
        assert g.dtype == np.float32 and g.shape == (len(c) // 3, 9)
        d, a = _errors(g, _np_features(c))
        worst_d, worst_a = max(worst_d, d), max(worst_a, a)
    _record("internal_coords_vs_numpy", dist=worst_d, angle=worst_a, residues=int(sum(len(c) for c in chains) // 3))
    assert worst_d <= 1e-6 and worst_a <= 1e-6
    # a one-residue chain: no dihedral, no angle, no distance
    one = got[2]
    assert np.isnan(one[0, 3:]).all() and np.all(one[0, :3] == 0.0)


def test_internal_coords_argument_checks(gpu):
    from foldingdiff_amd import _binding
    import ctypes as C
    lib = _binding.load()
    xyz = np.zeros((4, 3, 3), np.float32)
    out = np.zeros((4, 9), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for offs, lens in (([0, 2], [2, 0]), ([0, 3], [2, 2]), ([-1, 1], [1, 3])):
        rc = lib.fd_internal_coords(0, P(xyz), P(np.array(offs, np.int32)), P(np.array(lens, np.int32)), 2, P(out))
        assert rc == -1
        assert lib.fd_last_error()
    rc = lib.fd_superpose_rmsd(0, P(np.zeros(6)), P(np.zeros(6)), P(np.array([0], np.int32)), P(np.array([0], np.int32)), 1,
                               P(np.zeros(1)))
    assert rc == -1 and b"lens" in lib.fd_last_error()


def test_round_trip_with_reference_nerf(gpu):
    """Featurise the reference NeRF's own coordinates (ref_nerf.npz canonical_*_raw): every feature NeRF consumed to
    build them (rows 0..n-2, phi rows 1..n-1) comes back within 1e-5."""
    g = golden("ref_nerf.npz")
    sizes = (2, 37, 128)
    got = structures.internal_coords([g[f"canonical_{n}_raw"].astype(np.float32) for n in sizes])
    assert list(g["names_canonical"]) == structures.CANONICAL
    worst = 0.0
    for n, f in zip(sizes, got):
        want = g[f"canonical_{n}_feats"].astype(np.float64)
        d = f.astype(np.float64) - want
        d[:, 3:] = (d[:, 3:] + np.pi) % (2 * np.pi) - np.pi
        consumed = np.abs(d[:-1])
        consumed[:, 3] = 0.0
        worst = max(worst, consumed.max(), np.abs(d[1:, 3]).max())
    _record("round_trip_ref_nerf", max=worst)
    assert worst <= 1e-5


def test_full_reconstruction_1crn(gpu):
    """The reference's test_full_reconstruction (tests/test_nerf.py:72): 1CRN -> nine features -> NeRF -> the same
    backbone, within 1e-3 A RMSD after superposition."""
    df = structures.featurize([FIXTURES[0]])[0]
    assert list(df.columns) == structures.CANONICAL and len(df) == 46
    xyz = nerf.build_backbones([df.values], list(df.columns), center_coords=False)[0]
    truth = structures.read_backbone(FIXTURES[0])[0]
    r = structures.superposed_rmsd([xyz], [truth])[0]
    _record("full_reconstruction_1crn", rmsd=r, max_abs=np.abs(xyz - truth).max())
    assert r <= 1e-3
    # the single-file form with the reference's defaults: the three dihedrals
    one = structures.canonical_distances_and_dihedrals(FIXTURES[0])
    assert list(one.columns) == ["phi", "psi", "omega"]
    assert np.array_equal(one.values, df[["phi", "psi", "omega"]].values, equal_nan=True)


def _kabsch(a, b):
    u, v = a - a.mean(0), b - b.mean(0)
    U, _, Wt = np.linalg.svd(u.T @ v)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Wt))])
    R = (U @ D @ Wt).T
    return np.sqrt(((u @ R.T - v) ** 2).sum() / len(a))


def _rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_superpose_rmsd_vs_kabsch(gpu):
    """fd_superpose_rmsd against SVD Kabsch in fp64 on rotated, translated and noised pairs of ragged lengths (1, 2,
    collinear, up to 2000 atoms): <= 1e-9 A; an identical pair gives 0."""
    rng = np.random.default_rng(5)
    a_list, b_list = [], []
    for n in [1, 2, 3, 4, 63, 64, 65, 200, 2000] + list(rng.integers(1, 700, 60)):
        a = rng.standard_normal((n, 3)) * 12
        a_list.append(a)
        b_list.append(a @ _rotation(rng).T + rng.uniform(-80, 80, 3) + rng.standard_normal((n, 3)) * rng.choice([0.0, 1e-3, 0.7]))
    line = np.outer(np.linspace(-20, 20, 50), [0.3, -0.5, 0.8])
    a_list += [line, line + 1.0]
    b_list += [line @ _rotation(rng).T + 5.0, (line + rng.standard_normal(line.shape) * 0.1) @ _rotation(rng).T]
    ident = rng.standard_normal((150, 3)) * 10 + 40
    a_list.append(ident)
    b_list.append(ident.copy())
    got = structures.superposed_rmsd(a_list, b_list)
    want = np.array([_kabsch(a, b) for a, b in zip(a_list, b_list)])
    worst = np.abs(got - want).max()
    _record("superpose_rmsd_vs_kabsch", max=worst, identical=got[-1])
    assert got.shape == want.shape and worst <= 1e-9
    assert got[-1] == 0.0 and got[0] == 0.0   # identical pair; a single atom


def _toy_model():
    gm = golden("ref_abs_model.npz")
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                               max_position_embeddings=64, position_embedding_type="absolute")
    pm = modelling.BertForDiffusionBase(cfg, [True] * 6)
    pm.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")})
    return pm.to("cuda:0")


def test_reconstruct_from_pdb_files(gpu):
    """PdbAnglesDataset over the fixtures -> NoisedAnglesDataset -> sampling.reconstruct on the small synthetic model,
    then get_reconstruction_error with the built-in RMSD scorer."""
    ds = structures.PdbAnglesOnlyDataset(FIXTURES, pad=64, min_length=0, trim_strategy="leftalign")
    assert sorted(ds.filenames) == sorted(FIXTURES) and sorted(ds.all_lengths) == [20, 46]
    noised = datasets.NoisedAnglesDataset(ds, dset_key="angles", timesteps=1000, beta_schedule="cosine")
    pm = _toy_model()
    torch.manual_seed(3)
    recon, truth, files = sampling.reconstruct(pm, noised, noise_timesteps=5, bs=8)
    assert files == ds.filenames
    for i, f in enumerate(files):
        n = ds.all_lengths[i]
        assert recon[i].shape == truth[i].shape == (n, 6)
        assert np.array_equal(truth[i], ds[i]["angles"][:n].numpy())
        assert np.isfinite(recon[i]).all() and np.abs(recon[i]).max() <= np.pi + 1e-6
    scores, coord = sampling.get_reconstruction_error(pm, noised, noise_timesteps=5, bs=8, scorer=structures.rmsd_scorer)
    _record("reconstruct_rmsd_t5", max_rmsd=scores.max(), max_rmsd_coord=coord.max())
    assert scores.shape == coord.shape == (2,)
    assert np.isfinite(scores).all() and np.isfinite(coord).all() and (scores >= 0).all() and (coord >= 0).all()
    # the per-item form agrees with the batch
    s1, c1 = structures.rmsd_scorer(recon[0], truth[0], files[0])
    s, c = structures.rmsd_scorer.score_batch(recon, truth, files)
    assert s1 == s[0] and c1 == c[0]
    with pytest.raises(NotImplementedError):
        sampling.get_reconstruction_error(pm, noised, noise_timesteps=5)


def test_partial_noise_reconstruct_cli(gpu, tmp_path):
    """bin/partial_noise_reconstruct.py on the fixtures with a model directory as training leaves it: exit 0, one
    finite RMSD and one finite coordinate RMSD per file."""
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir = str(tmp_path / "model")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    out = str(tmp_path / "scores.json")
    cli = os.path.join(REPO, "bin", "partial_noise_reconstruct.py")
    r = subprocess.run([sys.executable, cli, *FIXTURES, out, "-t", "5", "-m", mdir, "-d", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    assert res["timesteps"] == 5 and res["model"] == mdir and "tmscores" not in res
    for key in ("rmsd", "rmsd_coord"):
        assert sorted(res[key]) == sorted(FIXTURES)
        assert all(np.isfinite(v) and v >= 0 for v in res[key].values())
