"""Resampling schedules of motif-conditioned sampling on the device (fd_sample_inpaint_resample, fd_inpaint_jump,
sampling.scaffold(..., jump_length, n_resample)) against the CPU restatement of tests/resample_reference.py and against the
composition of the entries that existed before them.  Fixed and free elements of a jump are compared BIT FOR BIT with the
float32 statement of include/fdmi.h; free-running runs with the tolerances of the plain sampler's tests."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

import inpaint_reference as ipr
import resample_reference as rsr
from conftest import GOLDEN
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_sampling
from test_gpu_parity import PRECISIONS, _c1_models, _free_running_check, _inputs, _pair, _record, _share_time_table
from test_inpaint_gpu import ANG, C1_LENS, F, _bits, _masks, _sample_inpaint, _sample_plain

pytestmark = pytest.mark.gpu
P = _binding.ptr


def _draws(h, seed, word, B, L, seq_offset=0):
    """The device's own Philox draws for a step word and a sequence offset."""
    out = torch.empty(B, L, F, device="cuda:0")
    _binding.check(_binding.load().fd_philox_normal_dev(h, C.c_uint64(seed), word - (1 << 32) if word >= (1 << 31) else word,
                                                        C.c_int64(seq_offset), B, L, C.c_void_p(out.data_ptr()), None))
    _binding.check(_binding.load().fd_synchronize(h))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _jump(h, x, lens, level_to, jk, js, known, fixed, coef, seed, seq_offset=0, fill=None):
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    out = np.empty_like(xs) if fill is None else np.full_like(xs, fill)
    rc = _binding.load().fd_inpaint_jump(h, P(xs), P(ls), B, L, level_to, C.c_float(jk), C.c_float(js), P(known), P(fixed), P(coef),
                                         C.c_uint64(seed), C.c_int64(seq_offset), P(out))
    return rc, out


def _resample(h, x0, lens, t_start, known, fixed, coef, visits, jump_coef, seed, seq_offset=0, n_visits=None):
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    vs = None if visits is None else np.ascontiguousarray(visits, dtype=np.int32)
    jc = None if jump_coef is None or len(jump_coef) == 0 else np.ascontiguousarray(jump_coef, dtype=np.float32)
    out = np.full((B, L, F), -7.0, dtype=np.float32)
    rc = _binding.load().fd_sample_inpaint_resample(h, P(x0), P(ls), B, L, t_start, P(known), P(fixed), P(coef), P(vs),
                                                    (0 if vs is None else len(vs)) if n_visits is None else n_visits, P(jc),
                                                    C.c_uint64(seed), C.c_int64(seq_offset), P(out))
    return rc, out


def _segments(visits):
    """[(first index, one past the last)] of the descents of a schedule."""
    v = [int(a) for a in visits]
    cuts = [0] + [i for i in range(1, len(v)) if v[i] != v[i - 1] - 1] + [len(v)]
    return list(zip(cuts[:-1], cuts[1:]))


def _compose(h, x0, lens, known, fixed, coef, visits, jump_coef, seed):
    """The resampled run from the entries that existed before it, [n_visits, B, L, F]: per segment fd_sample_inpaint from
    the segment's first step with the segment's seed and the whole history (the rows of the segment's visits are kept),
    then fd_inpaint_jump into the next."""
    x = np.ascontiguousarray(x0, dtype=np.float32)
    rows = []
    for s, (i, j) in enumerate(_segments(visits)):
        key = rsr.seeds(seed, s)
        if s > 0:
            rc, x = _jump(h, x, lens, int(visits[i]) + 1, jump_coef[s - 1][0], jump_coef[s - 1][1], known, fixed, coef, key)
            assert rc == 0, _binding.load().fd_last_error()
        rc, hist = _sample_inpaint(h, x, lens, int(visits[i]), known, fixed, coef, key, 1)
        assert rc == 0, _binding.load().fd_last_error()
        rows.extend(hist[: j - i])
        x = hist[j - i - 1]
    return np.stack(rows)


# ------------------------------------------------------------------ 1. the jump alone
@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_jump_alone(gpu, precision, hidden, heads):
    """fd_inpaint_jump on the one-layer models of the update kernels' test: B = 3, L = 24, T = 8, ragged lengths.  With the
    device's own draws of the two tagged words the restatement's bits, fixed and free; with ref_philox's draws alone within
    2.1e-5 on the circle (js, spread <= 1 times the 2e-5 the two generators may differ by, plus the statement's three
    roundings of values below 2 pi, 3 * 2.4e-7: the bound derived in test_inpaint_gpu.py); positions at or beyond a length
    keep the input's bits."""
    _, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, B, L, lens, seed, off = 8, 3, 24, [24, 17, 9], 0xC0FFEE1234567, 5
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    known, fixed = _masks([17, 24, 24, 9], 24, rows=(3, 12))
    known, fixed = known[[2, 1, 3]].copy(), fixed[[2, 1, 3]].copy()    # scattered (24), whole rows 3-11 (17), everything below 9
    fx = fixed.astype(bool)
    valid = np.zeros((B, L, F), dtype=bool)
    for b, n in enumerate(lens):
        valid[b, :n] = True
    x = _inputs(B, L, seed=5).numpy()
    for a, b in [(0, 1), (0, 8), (3, 5), (7, 8)]:
        jk, js = sampling.resample_jump_coef(betas, [a, b - 1])[0]
        rc, got = _jump(h, x, lens, b, jk, js, known, fixed, coef, seed, off)
        assert rc == 0, _binding.load().fd_last_error()
        zf, zk, zu = (_draws(h, seed, w, B, L, off) for w in (rsr.JUMP_TAG | b, ipr.TAG | b, b))
        assert not np.array_equal(zf, zk) and not np.array_equal(zf, zu) and not np.array_equal(zk, zu)   # three streams
        want = rsr.jump(x, known, fixed, b, jk, js, coef, zf, zk, ANG, lens)
        assert np.array_equal(_bits(got)[fx], _bits(want)[fx]), (a, b)
        assert np.array_equal(_bits(got)[valid & ~fx], _bits(want)[valid & ~fx]), (a, b)
        assert np.array_equal(_bits(got)[~valid], _bits(x)[~valid]), (a, b)
        assert (np.abs(got[valid]) <= np.float32(np.pi)).all()
        ref = rsr.jump(x, known, fixed, b, jk, js, coef, rsr.jump_draw(seed, b, off, B, L, F), ipr.tagged_draw(seed, b, off, B, L, F), ANG, lens)
        e = float(ref_sampling.circ_dist(got, ref)[valid].max())
        print(f"jump {a} -> {b} ({precision}, d = {hidden}): max circular distance to ref_philox's statement {e:.3e}")
        assert e <= 2.1e-5, (a, b, e)
        rc, other = _jump(h, x, lens, b, jk, js, known, fixed, coef, rsr.seeds(seed, 1), off)
        assert rc == 0 and not np.array_equal(other[valid], got[valid])               # another segment: fresh noise


# ------------------------------------------------------------------ 2. one call == the composition of the older entries
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_call_equals_the_composition_of_existing_entries(gpu, precision):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision=precision)
    T, B, L, lens, seed = 25, 4, 64, [50, 33, 64, 12], 5
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    x0 = _inputs(B, L, seed=4).numpy()
    known, fixed = _masks(lens, L)
    fx = fixed.astype(bool)
    visits = sampling.resample_schedule(T - 1, 5, 2)
    jc = sampling.resample_jump_coef(betas, visits)
    assert len(visits) == 45 and jc.shape == (4, 2)
    before = _sample_plain(h, x0, lens, T - 1, seed, 0)
    composed = _compose(h, x0, lens, known, fixed, coef, visits, jc, seed)[-1]
    runs = {}
    for graph, varlen in ((1, 0), (0, 0), (1, 1), (0, 1)):
        pm.set_option("use_graph", graph)
        pm.set_option("varlen", varlen)
        rc, runs[graph, varlen] = _resample(h, x0, lens, T - 1, known, fixed, coef, visits, jc, seed)
        assert rc == 0, _binding.load().fd_last_error()
    pm.set_option("use_graph", 1)
    pm.set_option("varlen", 0)
    assert np.array_equal(_bits(runs[1, 0]), _bits(composed))
    assert np.array_equal(_bits(runs[0, 0]), _bits(composed))
    for b, n in enumerate(lens):
        for graph in (1, 0):
            assert np.array_equal(_bits(runs[graph, 1][b, :n]), _bits(composed[b, :n])), (graph, b)
    assert np.array_equal(_bits(runs[1, 0])[fx], _bits(known)[fx])
    after = _sample_plain(h, x0, lens, T - 1, seed, 0)
    assert np.array_equal(_bits(after), _bits(before))                  # the dyn fields are cleared
    # a schedule without a jump is fd_sample_inpaint's run (jump_coef null)
    rc, plain = _sample_inpaint(h, x0, lens, T - 1, known, fixed, coef, seed, 0)
    assert rc == 0
    rc, flat = _resample(h, x0, lens, T - 1, known, fixed, coef, np.arange(T - 1, -1, -1), None, seed)
    assert rc == 0, _binding.load().fd_last_error()
    assert np.array_equal(_bits(flat), _bits(plain[0]))
    free = ~fx
    for b, n in enumerate(lens):
        free[b, n:] = False
    assert not np.array_equal(runs[1, 0][free], flat[free])             # the jumps change the free elements: the check can fail


# ------------------------------------------------------------------ 3. free-running against the oracle
# chosen on the CPU among forty seeds: the oracle's fp32 and fp64 runs of the restatement stay together on all three sequences
# (min_clean is asserted below) and no free element of the fp32 run comes within 4e-4 of the wrap boundary
RESAMPLE_SEED = 20240931
RESAMPLE_JUMP = 2          # T = 10: jumps from levels 0, 2, 4 and 6, 10 + 4 * 2 = 18 visits <= 2 T
_REF = {}


def _reference(o32, o64, x0, betas, T, known, fixed, coef, visits, jc):
    if not _REF:
        _share_time_table(o64, o32, T)
        _REF["want32"] = rsr.loop(o32, C1_LENS, x0, T - 1, betas, ANG, known, fixed, coef, visits, jc, RESAMPLE_SEED)
        _REF["want64"] = rsr.loop(o64, C1_LENS, x0, T - 1, betas, ANG, known, fixed, coef, visits, jc, RESAMPLE_SEED)
    return _REF["want32"], _REF["want64"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_free_running_c1_resampled(gpu, precision):
    """The C1 golden model over a schedule with n_resample = 2.  fd_sample_inpaint_resample returns the final state only, so
    the device's trajectory (one row per visit) is the composition of the test above, whose last row must be the one call's
    bits; it follows the restatement driven by the fp32 oracle, every draw of which comes from ref_philox."""
    g, o32, o64, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef = sampling.inpaint_levels(betas)
    known, fixed = _masks(C1_LENS, 64)
    fx = fixed.astype(bool)
    B, L = 4, 64
    visits = sampling.resample_schedule(T - 1, RESAMPLE_JUMP, 2)
    jc = sampling.resample_jump_coef(betas, visits)
    assert T < len(visits) <= 2 * T and len(jc) == 4
    want32, want64 = _reference(o32, o64, g["x0"], betas, T, known, fixed, coef, visits, jc)
    keep = ~fx
    for b, n in enumerate(C1_LENS):
        keep[b, n:] = False
    has_free = [b for b in range(B) if keep[b].any()]
    assert has_free == [0, 1, 2]                                # (sequence 3 has no free element and would always count as clean)
    sel = lambda a: np.where(keep, a, 0.0)[:, has_free]   # noqa: E731
    _free_running_check(f"resample_free_c1_oracle32_vs_64_{precision}", sel(want32), sel(want64))
    rc, final = _resample(h, g["x0"], C1_LENS, T - 1, known, fixed, coef, visits, jc, RESAMPLE_SEED)
    assert rc == 0, _binding.load().fd_last_error()
    got = _compose(h, g["x0"], C1_LENS, known, fixed, coef, visits, jc, RESAMPLE_SEED)
    assert got.shape == want32.shape and np.array_equal(_bits(got[-1]), _bits(final))
    assert np.array_equal(_bits(final)[fx], _bits(known)[fx])
    _free_running_check(f"resample_free_c1_{precision}", sel(got), sel(want32))


# ------------------------------------------------------------------ 4. argument errors
def test_new_argument_errors_leave_the_output_alone(gpu):
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
    visits = sampling.resample_schedule(T - 1, 2, 2)           # 5 4 3 2 3 2 1 0 1 0
    jc = sampling.resample_jump_coef(betas, visits)
    assert visits.tolist() == [5, 4, 3, 2, 3, 2, 1, 0, 1, 0] and len(jc) == 2

    def edit(i, v):
        out = visits.copy()
        out[i] = v
        return out

    def coefs(i, k, v):
        out = jc.copy()
        out[i, k] = v
        return out

    cases = [
        (dict(fixed=beyond), b"fixed element beyond"), (dict(known=None), b"known is null"), (dict(coef=None), b"known_coef"),
        (dict(visits=None), b"visits is null"), (dict(n_visits=0), b"n_visits"),
        (dict(visits=edit(0, 4)), b"visits[0]"), (dict(visits=edit(-1, 1)), b"visits[%d]" % (len(visits) - 1)),
        (dict(visits=edit(2, 6)), b"visits[2]"), (dict(visits=edit(2, -1)), b"visits[2]"),
        (dict(visits=edit(3, 1)), b"visits[3]"),                   # two levels down at once: neither a descent nor a jump
        (dict(jc=None), b"jump_coef is null"),
        (dict(jc=coefs(1, 0, np.nan)), b"jump 1"), (dict(jc=coefs(0, 1, 1.5)), b"jump 0"), (dict(jc=coefs(0, 0, -0.25)), b"jump 0"),
        (dict(jc=coefs(1, 1, np.inf)), b"jump 1"),
    ]
    for kw, word in cases:
        a = dict(known=known, fixed=fixed, coef=coef, visits=visits, jc=jc, n_visits=None)
        a.update(kw)
        rc, out = _resample(h, x0, lens, T - 1, a["known"], a["fixed"], a["coef"], a["visits"], a["jc"], 1, n_visits=a["n_visits"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == -7).all(), word
    jk, js = jc[0]
    hook = [
        (dict(level=0), b"level_to"), (dict(level=T + 1), b"level_to"), (dict(jk=np.nan), b"jk"), (dict(js=1.25), b"js"),
        (dict(jk=-0.5), b"jk"), (dict(fixed=beyond), b"fixed element beyond"), (dict(known=None), b"known is null"),
        (dict(coef=None), b"known_coef"),
    ]
    for kw, word in hook:
        a = dict(known=known, fixed=fixed, coef=coef, level=3, jk=jk, js=js)
        a.update(kw)
        rc, out = _jump(h, x0, lens, a["level"], a["jk"], a["js"], a["known"], a["fixed"], a["coef"], 1, fill=-7.0)
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == -7).all(), word
    rc, out = _resample(h, x0, lens, T - 1, known, fixed, coef, visits, jc, 1)      # the same calls with nothing wrong
    assert rc == 0 and np.isfinite(out).all(), lib.fd_last_error()
    rc, out = _jump(h, x0, lens, 3, jk, js, known, fixed, coef, 1, fill=-7.0)
    assert rc == 0 and np.isfinite(out).all() and (out != -7).all(), lib.fd_last_error()


# ------------------------------------------------------------------ 5. scaffold end to end
def test_scaffold_with_a_resampling_schedule_reproduces_the_motif_backbone(gpu, monkeypatch):
    """sampling.scaffold(..., jump_length=5, n_resample=2) on rows 5-16 of 1CRN's angles, T = 20, total lengths 30 and 31: the
    fixed rows are the motif's bits and the motif's residues of the NeRF-built backbones superpose on the motif's own
    backbone within n_angles * 1e-6 * extent, the angular bound of the end-to-end test of tests/test_inpaint_gpu.py.  The
    run differs from the plain descent of the same seed on the free rows."""
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    _, _, pm = _pair(seed=11, precision="f16x3")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=None), timesteps=20,
                                      beta_schedule="cosine")
    names = ds.feature_names["angles"]
    feats = structures.featurize([os.path.join(GOLDEN, "1CRN.pdb")], distances=[], angles=names)[0]
    motif = feats[names].values[5:17].astype(np.float32)
    assert motif.shape == (12, F) and np.isfinite(motif).all()
    calls = []
    real = sampling._run_fd_inpaint_resample

    def spy(*a):
        calls.append(len(a[7]))
        return real(*a)

    monkeypatch.setattr(sampling, "_run_fd_inpaint_resample", spy)
    monkeypatch.setattr(sampling, "_run_fd_inpaint_resample_default", spy)         # (the spy is the device call: rows_hint as usual)
    torch.manual_seed(3)
    samples, offs = sampling.scaffold(pm, ds, motif, [30, 31], jump_length=5, n_resample=2)
    assert calls == [len(sampling.resample_schedule(19, 5, 2))] == [35]
    assert offs == [9, 9] and [s.shape for s in samples] == [(30, F), (31, F)]
    torch.manual_seed(3)
    plain, _ = sampling.scaffold(pm, ds, motif, [30, 31])
    for s, p, o in zip(samples, plain, offs):
        assert np.array_equal(_bits(s[o: o + 12]), _bits(motif))
        assert np.isfinite(s).all() and not np.array_equal(s[:o], np.zeros_like(s[:o]))
        assert not np.array_equal(s[:o - 1], p[:o - 1])
    own = structures.motif_backbone(motif, names)
    extent = float(np.sqrt(((own[:, None, :] - own[None, :, :]) ** 2).sum(-1)).max())
    bound = (12 * F + 1) * 1e-6 * extent                       # the motif's rows and tau of the row before them
    rmsd = structures.motif_rmsd(nerf.build_backbones(samples, names), own, offs)
    print(f"resampled scaffold: motif rmsd {rmsd} (bound {bound:.3e}, extent {extent:.2f} A)")
    _record("scaffold_1crn_resampled", max=float(rmsd.max()), bound=bound)
    assert (rmsd <= bound).all(), (rmsd, bound)


def test_sample_scaffold_script_takes_the_resampling_flags(gpu, tmp_path, caplog):
    import importlib.util
    import json

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
    with caplog.at_level(logging.INFO):
        cli.main(["-m", mdir, "--motif", pdb, "--motif_residues", "5", "17", "-l", "30", "32", "-o", out, "--seed", "3",
                  "--jump_length", "5", "--n_resample", "2"])
    assert "35 reverse steps (visits) per chain" in caplog.text
    with open(os.path.join(out, "motif_rmsd.json")) as fh:
        report = json.load(fh)
    assert sorted(report) == ["scaffold_0.pdb", "scaffold_1.pdb"]
    names = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
    motif = structures.featurize([pdb], distances=[], angles=names)[0][names].values[5:17].astype(np.float32)
    own = structures.motif_backbone(motif, names)
    bound = (12 * F + 1) * 1e-6 * float(np.sqrt(((own[:, None, :] - own[None, :, :]) ** 2).sum(-1)).max())
    for r in report.values():
        assert sorted(r) == ["motif_rmsd", "offset", "pdb_rmsd"] and r["motif_rmsd"] <= bound, (r, bound)
