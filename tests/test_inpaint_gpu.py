"""Motif-conditioned sampling on the device (fd_sample_inpaint, fd_p_sample_step_inpaint, sampling.scaffold) against the
CPU restatement of tests/inpaint_reference.py.  Fixed elements are compared BIT FOR BIT with the float32 statement of
include/fdmi.h; free elements with the tolerances of the plain sampler's tests (tests/test_gpu_parity.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inpaint_reference as ipr
from conftest import GOLDEN
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_sampling
from test_gpu_parity import PRECISIONS, STEP_TOL, _c1_models, _free_running_check, _inputs, _pair, _record, _share_time_table, _step

pytestmark = pytest.mark.gpu
F = 6
ANG = [True] * F
P = _binding.ptr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _masks(lens, L, rows=(10, 30)):
    """One mask per kind: nothing fixed, a run of whole rows, scattered single features, everything below the length
    (cycled over the sequences).  float32 known values in (-pi, pi), NaN-free (the device reads known only where fixed)."""
    B = len(lens)
    rng = np.random.default_rng(17)
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    for b in range(B):
        kind = b % 4
        if kind == 1:
            fixed[b, rows[0]: min(rows[1], lens[b])] = 1
        elif kind == 2:
            pick = rng.random((lens[b], F)) < 0.15
            pick[0, 0] = pick[lens[b] - 1, F - 1] = True     # the first and the last element below the length
            fixed[b, : lens[b]] = pick
        elif kind == 3:
            fixed[b, : lens[b]] = 1
    known = rng.uniform(-3.1, 3.1, (B, L, F)).astype(np.float32)
    return known, fixed


def _step_inpaint(h, x, t, lens, z, known, fixed, coef, zk, wrap=1):
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    zs = None if z is None else np.ascontiguousarray(z, dtype=np.float32)
    zks = None if zk is None else np.ascontiguousarray(zk, dtype=np.float32)
    out = np.empty_like(xs)
    _binding.check(_binding.load().fd_p_sample_step_inpaint(h, P(xs), t, P(ls), B, L, P(zs), wrap, P(known), P(fixed), P(coef), P(zks),
                                                            P(out)))
    return out


def _teacher_forced(name, pm, o32, betas, T, x0, lens, known, fixed, rng_seed=23):
    """Every step t = T-1 .. 0 from the restatement's own state: fixed elements carry the statement's bits (level t; level 0
    included), free elements are within STEP_TOL (circular) of the oracle step, and with an all-zero mask the hook returns
    fd_p_sample_step's bits."""
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    assert np.array_equal(_bits(coef), _bits(ipr.levels(betas)))
    g = torch.Generator().manual_seed(rng_seed)
    B, L, _ = x0.shape
    fx = fixed.astype(bool)
    nothing = np.zeros_like(fixed)
    x = np.asarray(x0, dtype=np.float32)
    worst = 0.0
    for t in range(T - 1, -1, -1):
        z = torch.randn(B, L, F, generator=g).numpy()
        zk = torch.randn(B, L, F, generator=g).numpy()
        want = ipr.step(o32, x, t, lens, betas, z if t > 0 else None, known, fixed, coef, zk if t > 0 else None, ANG)
        got = _step_inpaint(h, x, t, lens, z if t > 0 else None, known, fixed, coef, zk if t > 0 else None)
        assert np.array_equal(_bits(got)[fx], _bits(want)[fx]), (name, t)
        if t == 0:
            assert np.array_equal(_bits(got)[fx], _bits(known)[fx]), name
        valid = np.zeros((B, L, F), dtype=bool)
        for b, n in enumerate(lens):
            valid[b, :n] = True
        free = valid & ~fx
        e = float(ref_sampling.circ_dist(got, want)[free].max())
        print(f"{name} t={t}: free elements max circular error {e:.3e}")
        worst = max(worst, e)
        assert e <= STEP_TOL, (name, t, e)
        plain = _step(pm, h, x, t, lens, z if t > 0 else None)
        empty = _step_inpaint(h, x, t, lens, z if t > 0 else None, known, nothing, coef, zk if t > 0 else None)
        assert np.array_equal(_bits(empty), _bits(plain)), (name, t)
        assert np.array_equal(_bits(got)[free], _bits(plain)[free]), (name, t)   # free elements: the plain step's arithmetic
        x = want
    _record(name, max=worst, steps=T)


C1_LENS = [64, 50, 33, 20]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_teacher_forced_steps_c1(gpu, precision):
    g, o32, _, pm = _c1_models(precision)
    T = int(g["T"])
    known, fixed = _masks(C1_LENS, 64)
    _teacher_forced(f"inpaint_step_c1_{precision}", pm, o32, beta_schedules.cosine_beta_schedule(T), T, g["x0"], C1_LENS, known, fixed)


@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_teacher_forced_steps_every_update_kernel(gpu, precision, hidden, heads):
    """The three update kernels: the row-image kernel (f16x3), the 16-lanes-per-token kernel (f32, d % 64 == 0) and the
    one-wave-per-token kernel (f32, d = 96).  One-layer models, L = 24, B = 3, T = 8, ragged lengths."""
    o32, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, lens = 8, [24, 17, 9]
    known, fixed = _masks([17, 24, 24, 9], 24, rows=(3, 12))
    known, fixed = known[[2, 1, 3]].copy(), fixed[[2, 1, 3]].copy()    # scattered (24), whole rows 3-11 (17), everything below 9
    assert fixed[0].any() and fixed[1, 3:12].all() and not fixed[1, 12:].any() and fixed[2, :9].all() and not fixed[2, 9:].any()
    _teacher_forced(f"inpaint_step_d{hidden}_{precision}", pm, o32, beta_schedules.cosine_beta_schedule(T), T,
                    _inputs(3, 24, seed=5).numpy(), lens, known, fixed)


def _sample_inpaint(h, x0, lens, t_start, known, fixed, coef, seed, full_history, noise=None, known_noise=None, seq_offset=0):
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    nsteps = t_start + 1
    rows = -(-nsteps // full_history) if full_history else 1
    out = np.full((rows, B, L, F), -7.0, dtype=np.float32)
    rc = _binding.load().fd_sample_inpaint(h, P(x0), P(ls), B, L, t_start, P(noise), P(known), P(fixed), P(coef), P(known_noise),
                                           C.c_uint64(seed), C.c_int64(seq_offset), P(out), full_history)
    return rc, out


def _sample_plain(h, x0, lens, t_start, seed, full_history):
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    rows = -(-(t_start + 1) // full_history) if full_history else 1
    out = np.empty((rows, B, L, F), dtype=np.float32)
    _binding.check(_binding.load().fd_sample(h, P(x0), P(ls), B, L, t_start, None, C.c_uint64(seed), P(out), full_history))
    return out


def _device_draws(h, seed, word, B, L):
    """The device's own Philox draws for a step word (two's complement of the tagged word as the C int)."""
    out = torch.empty(B, L, F, device="cuda:0")
    t = word - (1 << 32) if word >= (1 << 31) else word
    _binding.check(_binding.load().fd_philox_normal_dev(h, C.c_uint64(seed), t, C.c_int64(0), B, L, C.c_void_p(out.data_ptr()), None))
    _binding.check(_binding.load().fd_synchronize(h))
    torch.cuda.synchronize()
    return out.cpu().numpy()


FREE_SEED = 20240917   # chosen on the CPU: the oracle's fp32 and fp64 runs of the restatement alone satisfy min_clean (asserted below)


_FREE_REF = {}


def _free_running_reference(o32, o64, x0, betas, T, known, fixed, coef):
    """The restatement's run with the fp32 and the fp64 oracle, both noise streams restated by ref_philox (the update's
    draws with step word t, the replacement's with the tagged word); computed once, shared by the two precisions."""
    if not _FREE_REF:
        B, L = 4, 64
        zero = np.zeros((B, L, F), dtype=np.float32)
        step_noise = np.stack([zero if t == 0 else ipr.ref_philox.philox_normal(FREE_SEED, t, 0, B, L, F) for t in range(T)])
        known_noise = np.stack([zero if j == 0 else ipr.tagged_draw(FREE_SEED, j, 0, B, L, F) for j in range(T + 1)])
        _share_time_table(o64, o32, T)
        _FREE_REF["want32"] = ipr.loop(o32, C1_LENS, x0, T - 1, betas, ANG, known, fixed, coef, step_noise, known_noise)
        _FREE_REF["want64"] = ipr.loop(o64, C1_LENS, x0, T - 1, betas, ANG, known, fixed, coef, step_noise, known_noise)
        _FREE_REF["known_noise"] = known_noise
    return _FREE_REF["want32"], _FREE_REF["want64"], _FREE_REF["known_noise"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_free_running_c1_philox(gpu, precision):
    """Both noise streams from Philox, full history.  In every history row the fixed elements carry the bits of the
    statement at that row's level, with the replacement's draws = the tagged stream (the device's own generator with the
    tagged step word, which is ref_philox's tagged restatement up to the logf / sincosf ulps the plain stream's test
    allows: 2e-5) and, independently of the device's generator, lie within 2.1e-5 of the statement on ref_philox's own
    draws; the last row holds known's bits; the free elements follow the restatement driven by the oracle."""
    g, o32, o64, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    known, fixed = _masks(C1_LENS, 64)
    fx = fixed.astype(bool)
    B, L = 4, 64
    want32, want64, known_noise = _free_running_reference(o32, o64, g["x0"], betas, T, known, fixed, coef)
    valid = np.zeros((B, L, F), dtype=bool)
    for b, n in enumerate(C1_LENS):
        valid[b, :n] = True
    keep = valid & ~fx
    # the condition on the seed: the oracle's own two precisions stay together on the free elements
    # (sequence 3 has no free element and would always count as clean: the check runs over the three that have some)
    has_free = [b for b in range(B) if keep[b].any()]
    assert has_free == [0, 1, 2]
    sel = lambda a: np.where(keep, a, 0.0)[:, has_free]   # noqa: E731
    _free_running_check(f"inpaint_free_c1_oracle32_vs_64_{precision}", sel(want32), sel(want64))
    rc, got = _sample_inpaint(h, g["x0"], C1_LENS, T - 1, known, fixed, coef, FREE_SEED, 1)
    assert rc == 0, _binding.load().fd_last_error()
    assert got.shape == (T, B, L, F)
    for j in range(T):
        level = T - 1 - j
        if level == 0:
            assert np.array_equal(_bits(got[j])[fx], _bits(known)[fx])
            continue
        zk = _device_draws(h, FREE_SEED, ipr.TAG | level, B, L)
        assert np.abs(zk - known_noise[level]).max() < 2e-5, level
        assert not np.array_equal(zk, _device_draws(h, FREE_SEED, level, B, L))      # disjoint from the update's own stream
        lv = ipr.known_at_level(known, level, coef, zk, ANG)
        assert np.array_equal(_bits(got[j])[fx], _bits(lv)[fx]), level
        # ... and against ref_philox's draws alone, with nothing of the device in the expectation: spread <= 1 times the
        # 2e-5 the two generators may differ by, plus the statement's three roundings of values below 2 pi (3 * 2.4e-7)
        ref = ipr.known_at_level(known, level, coef, known_noise[level], ANG)
        assert ref_sampling.circ_dist(got[j], ref)[fx].max() <= 2.1e-5, level
    _free_running_check(f"inpaint_free_c1_{precision}", sel(got), sel(want32))


def test_varlen_rows_leave_positions_below_the_lengths_bit_identical(gpu):
    g, _, _, pm = _c1_models("f16x3")
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    lens = [64, 41, 17, 8]
    known, fixed = _masks(lens, 64, rows=(10, 30))
    fixed[0, 5:9] = 1                        # (the cycle leaves sequence 0 free: fix something in every kind of row)
    outs = []
    for varlen in (0, 1):
        pm.set_option("varlen", varlen)
        rc, out = _sample_inpaint(h, g["x0"], lens, T - 1, known, fixed, coef, 99, 1)
        assert rc == 0, _binding.load().fd_last_error()
        outs.append(out)
    pm.set_option("varlen", 0)
    for b, n in enumerate(lens):
        assert np.array_equal(_bits(outs[0][:, b, :n]), _bits(outs[1][:, b, :n])), b
        assert (outs[1][:, b, n:] == 0).all()   # packed rows: the history's padding is zeroed, as in fd_sample
    assert np.array_equal(_bits(outs[1][-1])[fixed.astype(bool)], _bits(known)[fixed.astype(bool)])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_graph_replay_equals_eager_and_plain_runs_are_unaffected(gpu, precision):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision=precision)
    T = 25
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    lens = [50, 33, 64, 12]
    x0 = _inputs(4, 64, seed=4).numpy()
    known, fixed = _masks(lens, 64)
    before = _sample_plain(h, x0, lens, T - 1, 5, 1)
    runs = {}
    for graph in (1, 0):
        pm.set_option("use_graph", graph)
        rc, runs[graph] = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, 5, 1)
        assert rc == 0, _binding.load().fd_last_error()
    pm.set_option("use_graph", 1)
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    fx = fixed.astype(bool)
    assert np.array_equal(_bits(runs[1][-1])[fx], _bits(known)[fx])
    assert not np.array_equal(runs[1][-1][~fx], before[-1][~fx])        # the run was conditioned ...
    after = _sample_plain(h, x0, lens, T - 1, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))                  # ... and a plain run after it is what it was before
    rc, every3 = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, 5, 3)
    assert rc == 0 and every3.shape[0] == 9
    assert np.array_equal(_bits(every3[:-1]), _bits(runs[1][2::3][:8])) and np.array_equal(_bits(every3[-1]), _bits(runs[1][-1]))
    rc, final = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, 5, 0)
    assert rc == 0 and np.array_equal(_bits(final[0]), _bits(runs[1][-1]))
    # explicit arrays for either stream, independently of each other: the replacement reads row `level` of known_noise
    g = torch.Generator().manual_seed(1)
    kz = torch.randn(T + 1, 4, 64, F, generator=g).numpy()
    rc, mixed = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, 5, 1, known_noise=kz)
    assert rc == 0
    for j in (0, 7, T - 2):
        lv = ipr.known_at_level(known, T - 1 - j, coef, kz[T - 1 - j], ANG)
        assert np.array_equal(_bits(mixed[j])[fx], _bits(lv)[fx]), j
    assert np.array_equal(_bits(mixed[-1])[fx], _bits(known)[fx])


def test_argument_errors_leave_the_output_alone(gpu):
    _, _, pm = _pair(seed=1)
    T = 6
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    lens = [16, 9]
    x0 = _inputs(2, 16, seed=2).numpy()
    known, fixed = _masks(lens, 16, rows=(2, 6))
    lib = _binding.load()
    beyond = fixed.copy()
    beyond[1, 9, 4] = 1                       # the first position past lens[1]
    z = np.zeros((2, 16, F), dtype=np.float32)
    for kw, word in [(dict(fixed=beyond), b"fixed element beyond"), (dict(known=None), b"known is null"), (dict(coef=None), b"known_coef")]:
        a = dict(known=known, fixed=fixed, coef=coef)
        a.update(kw)
        rc, out = _sample_inpaint(h, x0, lens, T - 1, a["known"], a["fixed"], a["coef"], 1, 1)
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == -7).all()
        step_out = np.full((2, 16, F), -7.0, dtype=np.float32)
        rc = lib.fd_p_sample_step_inpaint(h, P(x0), 3, P(np.asarray(lens, np.int32)), 2, 16, P(z), 1, P(a["known"]), P(a["fixed"]),
                                          P(a["coef"]), P(z), P(step_out))
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (step_out == -7).all()
    rc, out = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, 1, 1)      # the same call with nothing wrong
    assert rc == 0 and np.isfinite(out).all()


@pytest.mark.parametrize("with_offset", [False, True])
def test_scaffold_end_to_end_reproduces_the_motif_backbone(gpu, with_offset, monkeypatch):
    """A random-weight canonical-full-angles model scaffolds rows 5-16 of 1CRN's angles to total lengths 30 and 31.  The
    returned fixed rows are the motif's bits (no mean offset) or within 4 ulp of pi of them (a mean offset: two roundings
    of a value below pi on the way in, two on the way out); the motif's residues of the NeRF-built backbones superpose on
    the motif's own NeRF-built backbone within n_angles * 1e-6 * extent (the first-order worst case of that angular
    error: every fixed angle off by 1e-6 rad, each moving an atom by at most the motif's extent).  An unconditional
    sample() of the same lengths is far outside the bound, so the check can fail."""
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    _, _, pm = _pair(seed=11, precision="f16x3")
    offset = np.array([0.11, -0.07, 0.05, 0.02, -0.03, 0.04], dtype=np.float32) if with_offset else None
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=offset), timesteps=20,
                                      beta_schedule="cosine")
    names = ds.feature_names["angles"]
    feats = structures.featurize([os.path.join(GOLDEN, "1CRN.pdb")], distances=[], angles=names)[0]
    motif = feats[names].values[5:17].astype(np.float32)
    assert motif.shape == (12, F) and np.isfinite(motif).all()
    torch.manual_seed(3)
    samples, offs = sampling.scaffold(pm, ds, motif, [30, 31])
    assert offs == [9, 9] and [s.shape for s in samples] == [(30, F), (31, F)]
    for s, o in zip(samples, offs):
        if with_offset:
            ulps = ref_sampling.circ_dist(s[o: o + 12], motif).max() / float(np.spacing(np.float32(np.pi)))
            print(f"offset run: fixed rows within {ulps:.2f} ulp of pi")
            assert ulps <= 4
        else:
            assert np.array_equal(_bits(s[o: o + 12]), _bits(motif))
        assert np.isfinite(s).all() and not np.array_equal(s[:o], np.zeros_like(s[:o]))
    own = structures.motif_backbone(motif, names)
    extent = float(np.sqrt(((own[:, None, :] - own[None, :, :]) ** 2).sum(-1)).max())
    n_angles = 12 * F + 1                                      # the motif's rows and tau of the row before them
    bound = n_angles * 1e-6 * extent
    rmsd = structures.motif_rmsd(nerf.build_backbones(samples, names), own, offs)
    torch.manual_seed(3)
    free = [s[-1] for s in sampling.sample(pm, ds, n=1, sweep_lengths=(30, 32), final_only=True)]
    rmsd_free = structures.motif_rmsd(nerf.build_backbones(free, names), own, offs)
    print(f"motif rmsd {rmsd} (bound {bound:.3e}, extent {extent:.2f} A); unconditional {rmsd_free}")
    _record(f"scaffold_1crn_offset{int(with_offset)}", max=float(rmsd.max()), bound=bound, unconditional=float(rmsd_free.min()))
    assert (rmsd <= bound).all(), (rmsd, bound)
    assert (rmsd_free > bound).all(), (rmsd_free, bound)


def test_sample_scaffold_script_writes_angles_backbones_and_the_rmsd_report(gpu, tmp_path):
    """bin/sample_scaffold.py on a model directory with a mean offset: the output tree, the motif's residues of the written
    angles within 4 ulp of pi of 1CRN's own, and motif_rmsd.json -- within the angular bound of the test above against the
    motif's own NeRF-built backbone, beyond it against the file's coordinates (NeRF's bond lengths are constants)."""
    import importlib.util
    import json

    import pandas as pd
    from conftest import REPO
    from oracle import ref_model
    from test_gpu_parity import _write_model_dir
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 0.05, -0.05, 0.15], dtype=np.float32))
    spec = importlib.util.spec_from_file_location("sample_scaffold", os.path.join(REPO, "bin", "sample_scaffold.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    pdb = os.path.join(GOLDEN, "1CRN.pdb")
    cli.main(["-m", mdir, "--motif", pdb, "--motif_residues", "5", "17", "-l", "30", "32", "-n", "2", "--placement", "random",
              "-o", out, "--seed", "3"])     # (this seed places one motif at offset 0: NeRF's seed residue is its first)
    assert sorted(os.listdir(out)) == ["motif_rmsd.json", "sampled_angles", "sampled_pdb"]
    with open(os.path.join(out, "motif_rmsd.json")) as fh:
        report = json.load(fh)
    assert sorted(report) == [f"scaffold_{i}.pdb" for i in range(4)]
    names = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
    motif = structures.featurize([pdb], distances=[], angles=names)[0][names].values[5:17].astype(np.float32)
    own = structures.motif_backbone(motif, names)
    bound = (12 * F + 1) * 1e-6 * float(np.sqrt(((own[:, None, :] - own[None, :, :]) ** 2).sum(-1)).max())   # as in the test above
    for i in range(4):
        r = report[f"scaffold_{i}.pdb"]
        df = pd.read_csv(os.path.join(out, "sampled_angles", f"scaffold_{i}.csv.gz"), index_col=0)
        assert list(df.columns) == names and len(df) == 30 + i // 2 and 0 <= r["offset"] <= len(df) - 12 and sorted(r) == ["motif_rmsd", "offset", "pdb_rmsd"]
        got = df.values[r["offset"]: r["offset"] + 12].astype(np.float32)
        assert ref_sampling.circ_dist(got, motif).max() <= 4 * float(np.spacing(np.float32(np.pi)))
        assert os.path.isfile(os.path.join(out, "sampled_pdb", f"scaffold_{i}.pdb"))
        assert r["motif_rmsd"] <= bound < r["pdb_rmsd"] < 2.0, (r, bound)
    assert min(r["offset"] for r in report.values()) == 0 < max(r["offset"] for r in report.values())
    with pytest.raises(AssertionError, match="to be empty"):
        cli.main(["-m", mdir, "--motif", pdb, "--motif_residues", "5", "17", "-l", "30", "32", "-o", out])
