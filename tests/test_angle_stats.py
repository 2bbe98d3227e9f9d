"""The angle-distribution KL on the host: ``custom_metrics`` against the reference's own values
(tests/golden/ref_angle_stats.npz, make_golden_angle_stats.py), the properties the reference's tests/test_metrics.py
asks for, the three C entries and their argument checks (which run before a device is touched), a static guard on the
kernels, and the two scripts as far as they go without a device.  No GPU needed."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from foldingdiff_amd import _binding
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import custom_metrics as cm

FD_E_INVALID = -1


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "bin", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(got, want, rel=1e-12):
    """inf as inf, everything else to `rel` relative"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert (np.isinf(got) == np.isinf(want)).all(), (got, want)
    fin = np.isfinite(want)
    assert (got[~fin] == want[~fin]).all()
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert (err <= rel).all(), (err.max(), got, want)
    return err.max() if err.size else 0.0


def test_host_path_reproduces_the_reference():
    """kl_from_empirical(device=None) against the reference's values for every recorded pair, bin count and pseudocount
    setting: the same fp64 statements on the same counts, so 1e-12 relative; inf comes out as inf."""
    g = golden("ref_angle_stats.npz")
    want = g["a_kl"]
    n_inf, worst = 0, 0.0
    for k in range(want.shape[0]):
        u, v = g[f"a_u{k}"], g[f"a_v{k}"]
        for i, nbins in enumerate(g["nbins"]):
            for j, pc in enumerate((False, True)):
                got = cm.kl_from_empirical(u, v, nbins=int(nbins), pseudocount=pc)
                worst = max(worst, _close(got, want[k, i, j]))
                n_inf += int(np.isinf(want[k, i, j]))
    print("worst relative difference", worst, "inf cases", n_inf)
    assert n_inf >= 4 and np.isfinite(want).sum() >= 16
    assert {g[f"a_u{k}"].dtype for k in range(want.shape[0])} == {np.dtype(np.float32), np.dtype(np.float64)}


def test_host_path_reproduces_the_kl_helper_rows():
    """_kl_helper's rows from the recorded corrupted rows and comparison draws: all inf at 100 bins (259 rows), and the
    reference's finite values at the coarse bin count."""
    g = golden("ref_angle_stats.npz")
    coarse = int(g["coarse_nbins"])
    for tag in ("f6", "f9"):
        for sched in ("cosine", "linear"):
            x_t, cmp = g[f"b_{tag}_{sched}_corrupted"], g[f"b_{tag}_{sched}_cmp"]
            for i in range(x_t.shape[0]):
                for f in range(x_t.shape[2]):
                    _close(cm.kl_from_empirical(x_t[i, :, f], cmp[i, :, f]), g[f"b_{tag}_{sched}_kl"][i, f])
                    _close(cm.kl_from_empirical(x_t[i, :, f], cmp[i, :, f], nbins=coarse), g[f"b_{tag}_{sched}_kl_coarse"][i, f])
            assert np.isfinite(g[f"b_{tag}_{sched}_kl_coarse"]).sum() >= 3 * 6


def test_relative_entropy_is_scipys_definition():
    assert cm.relative_entropy([0.5, 0.5], [0.9, 0.1]) == pytest.approx(0.5 * np.log(0.5 / 0.9) + 0.5 * np.log(0.5 / 0.1), rel=1e-15)
    assert cm.relative_entropy([1, 1, 0], [1, 1, 2]) == pytest.approx(np.log(2.0), rel=1e-15)   # normalised first; p = 0 adds 0
    assert cm.relative_entropy([1, 1], [1, 0]) == np.inf
    assert np.isnan(cm.relative_entropy([1, np.nan], [1, 1]))


# ---- the properties of the reference's tests/test_metrics.py
def test_two_gaussians_of_a_thousand_draws_are_infinitely_apart():
    rng = np.random.default_rng(seed=6789)
    u, v = rng.normal(0.0, 1.0, 1000), rng.normal(0.0, 1.0, 1000)
    assert cm.kl_from_empirical(u, v) == np.inf


def test_closer_gaussians_have_the_smaller_divergence():
    rng = np.random.default_rng(seed=6789)
    u, v, w = rng.normal(0.0, 2.0, 1000), rng.normal(0.0, 1.0, 1000), rng.normal(0.0, 0.5, 1000)
    assert cm.kl_from_empirical(v, u) < cm.kl_from_empirical(w, u)


def test_nonoverlapping_samples_are_infinitely_apart():
    rng = np.random.default_rng(seed=6789)
    assert cm.kl_from_empirical(rng.normal(0.0, 1.0, 1000), rng.normal(10.0, 1.0, 1000)) == np.inf


def test_pseudocount_makes_every_divergence_finite():
    rng = np.random.default_rng(seed=1)
    u, v = rng.normal(0.0, 1.0, 500).astype(np.float32), rng.normal(3.0, 1.0, 700).astype(np.float32)
    assert cm.kl_from_empirical(u, v) == np.inf
    assert np.isfinite(cm.kl_from_empirical(u, v, pseudocount=True))


def test_wrapped_mean():
    rng = np.random.default_rng(seed=6489)
    deg = np.array([140.0, 200.0])
    assert np.rad2deg(cm.wrapped_mean(np.deg2rad(deg))) == pytest.approx(170.0, abs=5e-3)
    for loc in (3.0, -3.0, 0.0, 0.5, -0.5):
        assert cm.wrapped_mean(rng.normal(loc, 0.25, 100000)) == pytest.approx(loc, abs=5e-3)
    x = rng.normal(-0.5, 0.25, 100000)
    m = cm.wrapped_mean(x)
    x[:100] = np.nan
    assert np.isfinite(cm.wrapped_mean(x)) and cm.wrapped_mean(x) == pytest.approx(m, abs=5e-3)
    table = rng.normal(1.0, 0.1, (1000, 3))
    assert cm.wrapped_mean(table, axis=0).shape == (3,)


def test_angle_kl_report_names_its_features():
    rng = np.random.default_rng(3)
    sampled, test = rng.normal(0, 1, (400, 2)), rng.normal(0, 1, (600, 2)).astype(np.float32)
    rep = cm.angle_kl_report(sampled, test, ["phi", "psi"])
    assert list(rep) == ["phi", "psi"]
    for i, name in enumerate(rep):
        assert rep[name] == cm.kl_from_empirical(sampled[:, i], test[:, i], nbins=200, pseudocount=True)
        assert np.isfinite(rep[name])
    with pytest.raises(ValueError):
        cm.angle_kl_report(sampled, test, ["phi"])


# ---- the C ABI
def test_entries_are_declared_bound_and_exported(lib):
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert re.search(r"^int fd_hist_columns\(int device_id, const float\* values, int64_t N, int F,", src, re.M)
    assert re.search(r"^int fd_noise_minmax\(int device_id, const float\* x0, int64_t N, int F,", src, re.M)
    assert re.search(r"^int fd_noise_hist\(int device_id, const float\* x0, int64_t N, int F,", src, re.M)
    assert re.search(r"^#define FDMI_HIST_MAX_BINS 4096$", src, re.M) and cm.HIST_MAX_BINS == 4096
    assert re.search(r"^#define FDMI_ABI_VERSION 7$", src, re.M)
    assert _binding.ABI_VERSION == 7 and lib.fd_abi_version() == 7
    for name in ("fd_hist_columns", "fd_noise_minmax", "fd_noise_hist"):
        assert name in _binding.exported_symbols() and hasattr(lib, name)


def test_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Every argument check returns -1 with its word in fd_last_error() and leaves the sentinel-filled outputs alone, on a
    machine without a GPU too.  No valid call is made.  N = 5 rows, F = 3, nbins = 4, T = 10, two timesteps."""
    P = _binding.ptr
    N, F, nbins, T = 5, 3, 4, 10
    rng = np.random.default_rng(5)
    values = rng.standard_normal((N, F)).astype(np.float32)
    edges = np.tile(np.linspace(-4.0, 4.0, nbins + 1), (F, 1))
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == FD_E_INVALID and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    def bad_edges(row, col, value):
        e = edges.copy()
        e[row, col] = value
        return e

    def hist(values=values, N=N, F=F, edges=edges, nbins=nbins, counts="default", outside="default"):
        counts = np.full((3, 4), -7, np.int64) if isinstance(counts, str) else counts
        outside = np.full(3, -7, np.int64) if isinstance(outside, str) else outside
        return [counts, outside], lib.fd_hist_columns(0, P(values), N, F, P(edges), nbins, None, P(counts), P(outside))

    for kw, word in [(dict(values=None), b"null"), (dict(edges=None), b"null"), (dict(counts=None), b"null"),
                     (dict(outside=None), b"null"), (dict(N=0), b"N=0"), (dict(N=-2), b"N=-2"), (dict(N=1 << 31), b"N=2147483648"),
                     (dict(F=0), b"F=0"), (dict(F=33), b"F=33"), (dict(nbins=0), b"nbins=0"), (dict(nbins=4097), b"nbins=4097"),
                     (dict(edges=bad_edges(1, 2, -3.0)), b"edges: row 1 is decreasing or NaN at 2"),
                     (dict(edges=bad_edges(2, 0, np.nan)), b"edges: row 2 is decreasing or NaN at 0")]:
        expect(word, *hist(**kw))

    angular, scale = np.array([1, 0, 1], np.uint8), np.ones(F, np.float32)
    keep, spread = np.linspace(1.0, 0.1, T).astype(np.float32), np.linspace(0.1, 1.0, T).astype(np.float32)
    ts = np.array([0, 9], np.int32)
    edges_t = np.tile(np.linspace(-4.0, 4.0, nbins + 1), (2, F, 1))

    def with_bad(a, i, value):
        a = a.copy()
        a[i] = value
        return a

    draws = np.zeros((2, N, F), np.float32)

    def noise_args(x0=values, N=N, F=F, angular=angular, scale=scale, keep=keep, spread=spread, T=T, ts=ts, nT=2, eps_in=None,
                   cmp_in=None):
        return (0, P(x0), N, F, P(angular), P(scale), P(keep), P(spread), T, P(ts), nT, 11, 12, 0, P(eps_in), P(cmp_in))

    shared = [(dict(x0=None), b"null"), (dict(angular=None), b"null"), (dict(scale=None), b"null"), (dict(keep=None), b"null"),
              (dict(spread=None), b"null"), (dict(ts=None), b"null"), (dict(N=0), b"N=0"), (dict(F=0), b"F=0"), (dict(F=33), b"F=33"),
              (dict(T=0), b"T=0"), (dict(nT=0), b"nT=0"), (dict(nT=65536), b"nT=65536"),
              (dict(ts=np.array([0, 10], np.int32)), b"timesteps[1]=10"), (dict(ts=np.array([-1, 3], np.int32)), b"timesteps[0]=-1"),
              (dict(keep=with_bad(keep, 4, np.nan)), b"keep[4]"), (dict(spread=with_bad(spread, 7, np.inf)), b"spread[7]"),
              (dict(scale=with_bad(scale, 1, np.inf)), b"scale[1]"),
              (dict(eps_in=draws), b"eps_in and cmp_in go together"), (dict(cmp_in=draws), b"eps_in and cmp_in go together")]

    def minmax(out="default", **kw):
        out = np.full((2, 2, 3, 2), -7, np.float32) if isinstance(out, str) else out
        return [out], lib.fd_noise_minmax(*noise_args(**kw), P(out))

    for kw, word in shared + [(dict(out=None), b"null")]:
        expect(word, *minmax(**kw))

    def noise_hist(edges=edges_t, nbins=nbins, counts="default", outside="default", **kw):
        counts = np.full((2, 2, 3, 4), -7, np.int64) if isinstance(counts, str) else counts
        outside = np.full((2, 2, 3), -7, np.int64) if isinstance(outside, str) else outside
        x_t, cmp, eps = (np.full((2, N, F), -7, np.float32) for _ in range(3))
        rc = lib.fd_noise_hist(*noise_args(**kw), P(edges), nbins, P(counts), P(outside), P(x_t), P(cmp), P(eps))
        return [counts, outside, x_t, cmp, eps], rc

    bad_t = edges_t.copy()
    bad_t[1, 2, 3] = -5.0   # row 1 * 3 + 2 = 5
    for kw, word in shared + [(dict(edges=None), b"null"), (dict(counts=None), b"null"), (dict(outside=None), b"null"),
                              (dict(nbins=0), b"nbins=0"), (dict(nbins=4097), b"nbins=4097"),
                              (dict(edges=bad_t), b"edges: row 5 is decreasing or NaN at 3")]:
        expect(word, *noise_hist(**kw))
    assert checked == 13 + 20 + 25


def test_python_wrappers_check_shapes_before_the_library_is_asked():
    with pytest.raises(ValueError):
        cm.hist_columns(np.zeros((4, 2), np.float32), np.zeros((3, 5)))
    with pytest.raises(ValueError):
        cm.hist_columns(np.zeros((4, 2), np.float32), np.zeros((2, 5)), rows_valid=np.ones(3, bool))


def test_kernels_hold_no_scratch():
    """angle_stats.hip compiles for the device alone, and every kernel of it (the noise kernels in both instantiations,
    Philox and given draws) has no private segment and spills neither vector nor scalar registers."""
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    assert "angle_stats.hip" in fbuild.SOURCES
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
                        "--cuda-device-only", "-o", "-", os.path.join(fbuild.CSRC, "angle_stats.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, copies in (("hist_columns_kernel", 1), ("noise_minmax_kernel", 2), ("noise_hist_kernel", 2), ("noise_draws_kernel", 2)):
        found = re.findall(r"\.name:\s+(_Z\S*" + kernel + r"\S*)\n(.*?)\.wavefront_size", r.stdout, re.S)
        assert len(found) == copies, f"{kernel}: {len(found)} instantiations in the metadata"
        for name, body in found:
            md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", body)}
            print(name, md)
            assert md["private_segment_fixed_size"] == 0, (name, md)
            assert md["vgpr_spill_count"] == 0, (name, md)
            assert md["sgpr_spill_count"] == 0, (name, md)


# ---- the scripts
def test_sample_plotting_only_parses_and_reports_on_the_host(tmp_path):
    """Two files of sampled angles in the layout bin/sample.py writes, a synthetic test table: angle_kl.json holds
    kl_from_empirical(sampled, test, 200, pseudocount) per feature, read in the order of the files' numbers."""
    import pandas as pd

    spo = _script("sample_plotting_only")
    args = spo.build_parser().parse_args(["some/dir", "--test-pdbs", "a.pdb", "b.pdb.gz"])
    assert args.dir_name == "some/dir" and args.test_pdbs == ["a.pdb", "b.pdb.gz"]
    assert spo.build_parser().parse_args(["--test-pdbs", "d"]).dir_name == os.getcwd()
    with pytest.raises(SystemExit):
        spo.build_parser().parse_args(["some/dir"])
    listing = tmp_path / "list.txt"
    listing.write_text("x/1.pdb\n\ny/2.pdb.gz\n")
    assert spo.list_test_pdbs([str(listing)]) == ["x/1.pdb", "y/2.pdb.gz"]
    assert spo.list_test_pdbs(["p.pdb", "q.pdb"]) == ["p.pdb", "q.pdb"]

    names = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
    rng = np.random.default_rng(11)
    os.makedirs(tmp_path / "sampled_angles")
    parts = {10: rng.normal(0.0, 1.0, (70, 6)), 9: rng.normal(0.2, 1.0, (50, 6))}
    for k, table in parts.items():
        pd.DataFrame(table, columns=names).to_csv(tmp_path / "sampled_angles" / f"generated_{k}.csv.gz")
    test = rng.normal(0.1, 1.1, (300, 6)).astype(np.float32)
    kl = spo.report(tmp_path, test, names)
    sampled = pd.concat([pd.read_csv(tmp_path / "sampled_angles" / f"generated_{k}.csv.gz", index_col=0) for k in (9, 10)]).values
    written = json.load(open(tmp_path / "plots" / "angle_kl.json"))
    assert written["n_generated"] == 120 and written["n_test"] == 300 and written["nbins"] == 200
    for i, name in enumerate(names):
        want = float(cm.kl_from_empirical(sampled[:, i], test[:, i], nbins=200, pseudocount=True))
        assert np.isfinite(want) and kl[name] == want and written["kl_generated_test"][name] == want


def test_kl_by_timestep_parses_and_writes_its_curve(tmp_path):
    kbt = _script("kl_by_timestep")
    args = kbt.build_parser().parse_args(["--pdbs", "d", "--timesteps", "1000", "--variance-schedule", "cosine"])
    assert (args.pdbs, args.timesteps, args.variance_schedule, args.model_dir, args.nbins, args.seed) == ("d", 1000, "cosine", None, 100, 6489)
    assert kbt.build_parser().parse_args(["--pdbs", "d", "--model-dir", "m"]).model_dir == "m"
    for bad in (["--timesteps", "10"], ["--pdbs", "d", "--variance-schedule", "sigmoid"]):
        with pytest.raises(SystemExit):
            kbt.build_parser().parse_args(bad)
    kl = np.array([[0.5, np.inf], [0.25, 0.125], [0.0, 1e-3]])
    kbt.write_curve(kl, ["phi", "psi"], tmp_path)
    lines = open(tmp_path / "kl_by_timestep.csv").read().splitlines()
    assert lines[0] == "phi,psi" and len(lines) == 4
    back = np.loadtxt(tmp_path / "kl_by_timestep.csv", delimiter=",", skiprows=1)
    assert np.array_equal(back, kl)


def _stub_featurizer(fnames):
    """Stands in for the device featuriser: per file a table of the nine canonical features (50 and 70 rows) and CA atoms."""
    import pandas as pd

    from foldingdiff_amd import structures
    rng = np.random.default_rng(8)
    out = []
    for k, _ in enumerate(fnames):
        n = 50 + 20 * k
        feats = np.concatenate([rng.normal(1.4, 0.02, (n, 3)), rng.uniform(-3.0, 3.0, (n, 6))], axis=1)
        out.append((pd.DataFrame(feats, columns=structures.CANONICAL), rng.normal(0, 5, (n, 3)).astype(np.float32)))
    return out


def _two_files(tmp_path):
    for name in ("a.pdb", "b.pdb"):
        (tmp_path / name).write_text("REMARK stand-in\n")
    return tmp_path


def test_kl_by_timestep_builds_the_dataset_its_arguments_describe(tmp_path, monkeypatch):
    from foldingdiff_amd import structures
    monkeypatch.setattr(structures, "_featurize_for_dataset", _stub_featurizer)
    kbt = _script("kl_by_timestep")
    args = kbt.build_parser().parse_args(["--pdbs", str(_two_files(tmp_path)), "--timesteps", "30", "--variance-schedule", "cosine",
                                          "--max-seq-len", "64", "--variance-scale", "0.5"])
    dset = kbt.build_dataset(args)
    assert (dset.timesteps, dset.schedule, dset.angular_var_scale, dset.nonangular_var_scale) == (30, "cosine", 0.5, 1.0)
    assert len(dset.dset) == 2 and dset.pad == 64 and dset.feature_names["angles"][0] == "phi"
    rows = cm.stack_unmasked(dset)
    assert rows.shape == (50 + 64, 6) and rows.dtype == np.float32   # the 70-residue chain is cut to the padded length
    defaults = kbt.build_dataset(kbt.build_parser().parse_args(["--pdbs", str(tmp_path)]))
    assert (defaults.timesteps, defaults.schedule, defaults.pad) == (250, "linear", 128)


def test_sample_plotting_only_featurises_the_short_test_files(tmp_path, monkeypatch):
    from foldingdiff_amd import structures
    monkeypatch.setattr(structures, "_featurize_for_dataset", _stub_featurizer)
    spo = _script("sample_plotting_only")
    files = spo.list_test_pdbs([str(_two_files(tmp_path))])
    assert [os.path.basename(f) for f in files] == ["a.pdb", "b.pdb"]
    test = spo.featurise_test(files, {"angles_definitions": "canonical-full-angles", "max_seq_len": 64, "min_seq_len": 40})
    assert test.shape == (50, 6) and test.dtype == np.float32          # the 70-residue file is longer than max_seq_len
    want = _stub_featurizer(files)[0][0].values[:, 3:].astype(np.float32)   # not zero-centred
    assert np.array_equal(test, want)
