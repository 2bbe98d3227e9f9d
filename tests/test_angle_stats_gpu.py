"""The angle-histogram kernels on the device (csrc/angle_stats.hip) against numpy: every count integer-equal, every
min / max and noised value bit-equal, the KL rows against the reference's (tests/golden/ref_angle_stats.npz)."""
import numpy as np
import pytest
import torch

from conftest import golden
from foldingdiff_amd import _binding, beta_schedules, datasets
from foldingdiff_amd import custom_metrics as cm
from oracle import ref_philox

pytestmark = pytest.mark.gpu
P = _binding.ptr


# ---------------------------------------------------------------- fd_hist_columns
def _column(kind, N, nbins, rng):
    """(float32 values [N], edges [nbins + 1] in the dtype numpy gives them) of one column."""
    x = rng.normal(0.3, 1.2, N).astype(np.float32)
    if kind == "normal":        # float32 linspace over the column's own range
        return x, np.linspace(x.min(), x.max(), nbins + 1)
    if kind == "edges":         # values exactly on the min, the max and interior edges of the float32 linspace itself
        e = np.linspace(x.min(), x.max(), nbins + 1)
        assert e.dtype == np.float32
        picks = e[rng.integers(0, nbins + 1, size=min(N, 40))]
        x[rng.permutation(N)[:picks.size]] = picks
        if N >= 3:
            x[0], x[-1] = e[0], e[-1]
        return x, e
    if kind == "const":         # all but two values equal: every lane hits one bin
        x[:] = np.float32(0.7)
        if N >= 3:
            x[N // 3], x[N // 2] = np.float32(-2.5), np.float32(3.25)
        return x, np.linspace(x.min(), x.max(), nbins + 1)
    if kind == "outside":       # genuinely float64 edges narrower than the data: values below and above
        lo, hi = (np.quantile(x, [0.1, 0.9]) if N > 1 else (x[0] + 1.0, x[0] + 2.0))
        e = np.linspace(float(lo) - 1.0 / 3.0, float(hi) + 1.0 / 7.0, nbins + 1)
        assert e.dtype == np.float64 and (e.astype(np.float32).astype(np.float64) != e).any()
        return x, e
    raise AssertionError(kind)


KINDS = ["normal", "edges", "const", "outside"]


@pytest.mark.parametrize("N", [1, 63, 64, 257, 4099, 70001])
def test_hist_columns_equals_numpy(gpu, N):
    """np.histogram, integer-equal, for F in {1, 4, 6, 9} and nbins in {1, 100, 200, 4096}: columns over their own
    float32 linspace, with values exactly on edges, with all but two values equal, and with float64 edges narrower than
    the data (``outside``)."""
    rng = np.random.default_rng(1000 + N)
    seen_outside = 0
    for F in (1, 4, 6, 9):
        for nbins in (1, 100, 200, 4096):
            for shift in range(4 if F == 1 else 1):
                cols = [_column(KINDS[(f + shift) % 4], N, nbins, rng) for f in range(F)]
                values = np.stack([c[0] for c in cols], axis=1)
                edges = np.stack([c[1].astype(np.float64) for c in cols])
                counts, outside = cm.hist_columns(values, edges, device=gpu)
                for f, (x, e) in enumerate(cols):
                    want = np.histogram(x, bins=e)[0]
                    assert np.array_equal(counts[f], want), (N, F, nbins, KINDS[(f + shift) % 4])
                    assert outside[f] == N - want.sum()
                    seen_outside += int(outside[f])
    assert seen_outside > 0 or N == 1


def test_hist_columns_skips_invalid_rows(gpu):
    rng = np.random.default_rng(7)
    values = rng.normal(0, 1, (5000, 6)).astype(np.float32)
    valid = rng.random(5000) < 0.6
    edges = np.stack([np.linspace(values[:, f].min(), values[:, f].max(), 51) for f in range(6)])
    counts, outside = cm.hist_columns(values, edges, device=gpu, rows_valid=valid)
    for f in range(6):
        assert np.array_equal(counts[f], np.histogram(values[valid, f], bins=edges[f])[0])
    assert not outside.any() and counts.sum() == 6 * valid.sum()


def test_kl_from_empirical_on_the_device_equals_the_host_path(gpu):
    """The float32 pairs of the golden file: device counts are numpy's counts, so the same value to the last bit, which
    is the reference's to 1e-12."""
    g = golden("ref_angle_stats.npz")
    done = 0
    for k in range(g["a_kl"].shape[0]):
        u, v = g[f"a_u{k}"], g[f"a_v{k}"]
        if u.dtype != np.float32:
            continue
        for i, nbins in enumerate(g["nbins"]):
            for j, pc in enumerate((False, True)):
                got = cm.kl_from_empirical(u, v, nbins=int(nbins), pseudocount=pc, device=gpu)
                host = cm.kl_from_empirical(u, v, nbins=int(nbins), pseudocount=pc)
                want = g["a_kl"][k, i, j]
                assert got == host
                assert got == want if np.isinf(want) else abs(got - want) <= 1e-12 * abs(want)
                done += 1
    assert done == 4 * 4


# ---------------------------------------------------------------- fd_noise_minmax / fd_noise_hist
def _tables(sched, T):
    terms = beta_schedules.compute_alphas(beta_schedules.get_variance_schedule(sched, T))
    return (np.ascontiguousarray(terms["sqrt_alphas_cumprod"].float().numpy()),
            np.ascontiguousarray(terms["sqrt_one_minus_alphas_cumprod"].float().numpy()))


def _minmax(gpu, x0, angular, scale, keep, spread, ts, seeds=(1, 2), row_offset=0, eps_in=None, cmp_in=None):
    x0, ts = np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(ts, np.int32)
    N, F = x0.shape
    mm = np.empty((ts.size, 2, F, 2), np.float32)
    _binding.check(_binding.load().fd_noise_minmax(gpu, P(x0), N, F, P(angular), P(scale), P(keep), P(spread), keep.size, P(ts),
                                                   ts.size, seeds[0], seeds[1], row_offset, P(eps_in), P(cmp_in), P(mm)))
    return mm


def _hist(gpu, x0, angular, scale, keep, spread, ts, edges, seeds=(1, 2), row_offset=0, eps_in=None, cmp_in=None):
    x0, ts = np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(ts, np.int32)
    N, F = x0.shape
    nT, nbins = ts.size, edges.shape[2] - 1
    counts, outside = np.empty((nT, 2, F, nbins), np.int64), np.empty((nT, 2, F), np.int64)
    x_t, cmp, eps = (np.empty((nT, N, F), np.float32) for _ in range(3))
    _binding.check(_binding.load().fd_noise_hist(gpu, P(x0), N, F, P(angular), P(scale), P(keep), P(spread), keep.size, P(ts), nT,
                                                 seeds[0], seeds[1], row_offset, P(eps_in), P(cmp_in), P(edges), nbins, P(counts),
                                                 P(outside), P(x_t), P(cmp), P(eps)))
    return dict(counts=counts, outside=outside, x_t=x_t, cmp=cmp, eps=eps)


def _edges(mm, nbins):
    """np.linspace per (timestep, feature) over min(x_t, cmp) .. max(x_t, cmp): (native arrays, float64 [nT][F][nbins + 1])"""
    lo, hi = mm[..., 0].min(axis=1), mm[..., 1].max(axis=1)
    native = [[np.linspace(lo[i, f], hi[i, f], nbins + 1) for f in range(mm.shape[2])] for i in range(mm.shape[0])]
    return native, np.ascontiguousarray(np.array(native, np.float64))


def _assert_counts_are_numpys(got, native, N):
    nT, _, F, _ = got["counts"].shape
    assert not got["outside"].any()
    assert (got["counts"].sum(axis=3) == N).all()
    for i in range(nT):
        for f in range(F):
            assert np.array_equal(got["counts"][i, 0, f], np.histogram(got["x_t"][i, :, f], bins=native[i][f])[0]), (i, f)
            assert np.array_equal(got["counts"][i, 1, f], np.histogram(got["cmp"][i, :, f], bins=native[i][f])[0]), (i, f)


class _Toy:
    """Items of zero-padded [pad, F] features, as the golden file's datasets."""

    def __init__(self, angles, lengths, names, angular):
        self.angles, self.lengths, self.pad = torch.from_numpy(angles), [int(l) for l in lengths], angles.shape[1]
        self.feature_names, self.feature_is_angular = {"angles": list(names)}, {"angles": list(angular)}

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, index, ignore_zero_center=False):
        mask = torch.zeros(self.pad)
        mask[:self.lengths[index]] = 1.0
        return {"angles": self.angles[index].clone(), "attn_mask": mask}


NAMES9 = ["0C:1N", "N:CA", "CA:C", "phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
GOLDEN_SETS = {"f6": (NAMES9[3:], [True] * 6, {}), "f9": (NAMES9, [False] * 3 + [True] * 6, {"nonangular_variance": 0.5})}


def _golden_dset(g, tag, sched):
    """The golden file's dataset with the schedule tables of the recorded run: torch's CPU cos and cumprod differ in the
    last bit between machines (keep[0] of the cosine schedule does), and the rows are pinned bit for bit."""
    names, angular, kw = GOLDEN_SETS[tag]
    dset = datasets.NoisedAnglesDataset(_Toy(g[f"b_{tag}_angles"], g["lengths"], names, angular), dset_key="angles",
                                        timesteps=int(g["T"]), beta_schedule=sched, **kw)
    dset.alpha_beta_terms = dict(dset.alpha_beta_terms, sqrt_alphas_cumprod=torch.from_numpy(g[f"b_{sched}_keep"]),
                                 sqrt_one_minus_alphas_cumprod=torch.from_numpy(g[f"b_{sched}_spread"]))
    return dset


@pytest.mark.parametrize("sched", ["cosine", "linear"])
@pytest.mark.parametrize("tag", ["f6", "f9"])
def test_the_references_draws_give_the_references_rows(gpu, tag, sched):
    """The recorded eps / cmp of _kl_helper fed as eps_in / cmp_in: x_t bit-equal to the recorded corrupted rows, min / max
    and counts numpy's, the KL rows the reference's (inf as inf at 100 bins; 1e-12 relative at the coarse bin count)."""
    g = golden("ref_angle_stats.npz")
    dset = _golden_dset(g, tag, sched)
    ts = g["timesteps"].astype(np.int32)
    eps, cmp, want_x_t = (np.ascontiguousarray(g[f"b_{tag}_{sched}_{k}"]) for k in ("eps", "cmp", "corrupted"))
    x0 = cm.stack_unmasked(dset)
    N, F = x0.shape
    assert eps.shape == (3, N, F)
    angular, scale, keep, spread = cm._noise_tables(dset)
    mm = _minmax(gpu, x0, angular, scale, keep, spread, ts, eps_in=eps, cmp_in=cmp)
    assert np.array_equal(mm[:, 0, :, 0], want_x_t.min(axis=1)) and np.array_equal(mm[:, 0, :, 1], want_x_t.max(axis=1))
    assert np.array_equal(mm[:, 1, :, 0], cmp.min(axis=1)) and np.array_equal(mm[:, 1, :, 1], cmp.max(axis=1))
    for nbins, key in ((100, "kl"), (int(g["coarse_nbins"]), "kl_coarse")):
        native, edges = _edges(mm, nbins)
        got = _hist(gpu, x0, angular, scale, keep, spread, ts, edges, eps_in=eps, cmp_in=cmp)
        assert np.array_equal(got["x_t"].view(np.uint32), want_x_t.view(np.uint32))
        assert np.array_equal(got["cmp"].view(np.uint32), cmp.view(np.uint32))
        assert np.array_equal(got["eps"].view(np.uint32), eps.view(np.uint32))
        _assert_counts_are_numpys(got, native, N)
        kl, x_t, cmp_back = cm.kl_from_dset(dset, timesteps=ts, nbins=nbins, device=gpu, noise=(eps, cmp), return_draws=True)
        want = g[f"b_{tag}_{sched}_{key}"]
        assert kl.shape == want.shape and np.array_equal(x_t, want_x_t) and np.array_equal(cmp_back, cmp)
        assert (np.isinf(kl) == np.isinf(want)).all()
        fin = np.isfinite(want)
        assert (np.abs(kl[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])).all(), np.abs(kl[fin] / want[fin] - 1).max()
        assert fin.sum() >= (18 if key == "kl_coarse" else 0)


@pytest.mark.parametrize("N,row_offset,nbins", [(1000, 0, 100), (1000, 1 << 33, 2000), (70001, 0, 4096), (70001, 1 << 33, 100)])
def test_philox_streams(gpu, N, row_offset, nbins):
    """Philox mode over t = 0, 50 and T - 1 (the bin counts 100 / 2000 / 4096 put 4 / 2 / 1 features into a workgroup):
    the two passes see the same streams (nothing outside, sums N), counts are numpy's of the returned draws and those of
    a call that is handed the draws, the stream is the oracle's, seeds and the timestep list behave."""
    T, F = 100, 9
    rng = np.random.default_rng(N + nbins)
    angular = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0], np.uint8)      # plain columns 0, 3, 5, 6, 8: every lane of a Philox block
    scale = np.where(angular != 0, np.float32(0.8), np.float32(1.0)).astype(np.float32)
    x0 = rng.normal(0.0, 1.0, (N, F)).astype(np.float32)
    keep, spread = _tables("cosine", T)
    ts = np.array([0, 50, T - 1], np.int32)
    seeds = ((7 << 40) + 99, 1234)
    common = (gpu, x0, angular, scale, keep, spread)
    mm = _minmax(*common, ts, seeds=seeds, row_offset=row_offset)
    native, edges = _edges(mm, nbins)
    got = _hist(*common, ts, edges, seeds=seeds, row_offset=row_offset)
    _assert_counts_are_numpys(got, native, N)
    assert np.array_equal(mm[:, 0, :, 0], got["x_t"].min(axis=1)) and np.array_equal(mm[:, 0, :, 1], got["x_t"].max(axis=1))
    assert np.array_equal(mm[:, 1, :, 0], got["cmp"].min(axis=1)) and np.array_equal(mm[:, 1, :, 1], got["cmp"].max(axis=1))
    # the draws handed back: the same values and counts
    again = _hist(*common, ts, edges, seeds=(5, 6), row_offset=row_offset, eps_in=got["eps"], cmp_in=got["cmp"])
    assert np.array_equal(again["counts"], got["counts"]) and np.array_equal(again["x_t"], got["x_t"])
    # the stream: the plain columns of cmp (scale 1, no wrap) are the oracle's normals, and eps is the other seed's
    plain = np.flatnonzero(angular == 0)
    for i, t in enumerate(ts):
        for seed, key in ((seeds[1], "cmp"), (seeds[0], "eps")):
            want = ref_philox.philox_normal(seed, int(t), row_offset, N, 1, F).reshape(N, F)
            assert np.abs(got[key][i][:, plain] - want[:, plain]).max() < 2e-5
    # the angular columns: wrap(scale * z) of the oracle's normals for both streams, away from the seam (where a draw that
    # differs in the last bits may land on the other side)
    wrapped = np.flatnonzero(angular != 0)
    for i, t in enumerate(ts):
        for seed, key in ((seeds[1], "cmp"), (seeds[0], "eps")):
            z = ref_philox.philox_normal(seed, int(t), row_offset, N, 1, F).reshape(N, F)[:, wrapped]
            want = (z * scale[wrapped] + np.float32(np.pi)) % np.float32(2 * np.pi) - np.float32(np.pi)
            inner = np.abs(want) < np.pi - 1e-3
            assert inner.mean() > 0.99
            assert np.abs(got[key][i][:, wrapped] - want)[inner].max() < 2e-5
    # x_t is q_sample's statement on eps
    for i, t in enumerate(ts):
        want = torch.from_numpy(x0) * torch.tensor(keep[t]) + torch.from_numpy(got["eps"][i]) * torch.tensor(spread[t])
        assert np.array_equal(got["x_t"][i][:, plain], want.numpy()[:, plain])
    # seeds
    same = _hist(*common, ts, edges, seeds=seeds, row_offset=row_offset)
    assert np.array_equal(same["counts"], got["counts"]) and np.array_equal(same["x_t"], got["x_t"])
    other = _hist(*common, ts, edges, seeds=(seeds[0] + 1, seeds[1] + 1), row_offset=row_offset)
    assert (other["counts"][:, 0] != got["counts"][:, 0]).any() and (other["counts"][:, 1] != got["counts"][:, 1]).any()
    shifted = _hist(*common, ts, edges, seeds=seeds, row_offset=row_offset + 1)
    assert (shifted["cmp"] != got["cmp"]).any()
    # one call per timestep
    for i in range(ts.size):
        one = _hist(*common, ts[i:i + 1], edges[i:i + 1].copy(), seeds=seeds, row_offset=row_offset)
        assert np.array_equal(one["counts"][0], got["counts"][i]) and not one["outside"].any()
        assert np.array_equal(_minmax(*common, ts[i:i + 1], seeds=seeds, row_offset=row_offset)[0], mm[i])


def test_kl_from_dset(gpu):
    """The F = 9 dataset over all 100 timesteps: [T, 9], equal to the host path on the returned draws (inf where that is
    inf), the same whatever the row batches, a different draw under another seed."""
    g = golden("ref_angle_stats.npz")
    dset = _golden_dset(g, "f9", "cosine")
    for nbins in (100, int(g["coarse_nbins"])):
        kl, x_t, cmp = cm.kl_from_dset(dset, nbins=nbins, device=gpu, return_draws=True)
        assert kl.shape == (100, 9) and x_t.shape == cmp.shape == (100, 259, 9)
        host = np.array([[cm.kl_from_empirical(x_t[t, :, f], cmp[t, :, f], nbins=nbins) for f in range(9)] for t in range(100)])
        assert np.array_equal(np.isfinite(kl), np.isfinite(host)) and np.array_equal(kl, host)
        assert np.array_equal(cm.kl_from_dset(dset, nbins=nbins, device=gpu), kl)
        assert np.array_equal(cm.kl_from_dset(dset, nbins=nbins, device=gpu, batch_rows=100), kl)
        # another seed: other draws (the KL itself cannot tell at 100 bins, where 259 rows leave every entry inf)
        _, x_t_other, cmp_other = cm.kl_from_dset(dset, nbins=nbins, device=gpu, seed=1, return_draws=True)
        assert (x_t_other != x_t).any() and (cmp_other != cmp).any()
    sub = cm.kl_from_dset(dset, timesteps=[99, 0], nbins=nbins, device=gpu)
    assert np.array_equal(sub, kl[[99, 0]])


# ---------------------------------------------------------------- the scripts, end to end
def _script(name):
    import importlib.util
    import os

    from conftest import REPO
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "bin", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _two_crambins(tmp_path):
    import os
    import shutil

    from conftest import GOLDEN
    pdbs = tmp_path / "pdbs"
    os.makedirs(pdbs)
    for name in ("a.pdb", "b.pdb"):
        shutil.copy(os.path.join(GOLDEN, "1CRN.pdb"), pdbs / name)
    return pdbs


def test_kl_by_timestep_end_to_end(gpu, tmp_path):
    """bin/kl_by_timestep.py on two copies of crambin (46 residues each): the csv is kl_from_dset of the dataset its
    arguments describe."""
    kbt = _script("kl_by_timestep")
    argv = ["--pdbs", str(_two_crambins(tmp_path)), "--timesteps", "12", "--variance-schedule", "cosine", "--max-seq-len", "64",
            "--nbins", "6", "-o", str(tmp_path / "out")]
    kbt.main(argv)
    dset = kbt.build_dataset(kbt.build_parser().parse_args(argv))
    assert len(dset.dset) == 2 and dset.timesteps == 12 and dset.schedule == "cosine"
    lines = open(tmp_path / "out" / "kl_by_timestep.csv").read().splitlines()
    assert lines[0] == "phi,psi,omega,tau,CA:C:1N,C:1N:1CA" and len(lines) == 13
    back = np.loadtxt(tmp_path / "out" / "kl_by_timestep.csv", delimiter=",", skiprows=1)
    assert np.array_equal(back, cm.kl_from_dset(dset, nbins=6, device=gpu))


def test_sample_plotting_only_end_to_end(gpu, tmp_path):
    """bin/sample_plotting_only.py on a directory laid out as bin/sample.py leaves it, the test set two copies of
    crambin: 92 test residues, a finite KL per angle."""
    import json
    import os

    import pandas as pd

    spo = _script("sample_plotting_only")
    run = tmp_path / "run"
    os.makedirs(run / "model_snapshot")
    os.makedirs(run / "sampled_angles")
    with open(run / "model_snapshot" / "training_args.json", "w") as sink:
        json.dump({"angles_definitions": "canonical-full-angles", "max_seq_len": 64, "min_seq_len": 40}, sink)
    names = NAMES9[3:]
    rng = np.random.default_rng(2)
    for k in range(2):
        pd.DataFrame(rng.normal(0.0, 1.0, (50, 6)), columns=names).to_csv(run / "sampled_angles" / f"generated_{k}.csv.gz")
    spo.main([str(run), "--test-pdbs", str(_two_crambins(tmp_path))])
    written = json.load(open(run / "plots" / "angle_kl.json"))
    assert written["n_generated"] == 100 and written["n_test"] == 92
    assert list(written["kl_generated_test"]) == names and all(np.isfinite(v) for v in written["kl_generated_test"].values())
