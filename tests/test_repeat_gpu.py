"""Repeat proteins on the device (fd_tie_repeats, fd_sample_repeat, sampling.sample_repeats, structures.repeat_rmsd,
bin/sample_repeats.py) against the numpy float32 statement of tests/repeat_reference.py and the existing entries composed on
the host: bits are compared with ==; the Philox draws with the bound derived at their test.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import repeat_reference as rr
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_model, ref_philox, ref_sampling
from test_gpu_parity import PRECISIONS, _inputs, _pair, _write_model_dir
from test_steer_gpu import MODEL_D, NAMES, VISIT_SETS
from test_strided_gpu import ANG, F, SENTINEL, _bits, _step_coef, _strided, _valid

pytestmark = pytest.mark.gpu
P = _binding.ptr
L_R = 16
LENS5 = [16, 13, 9, 14, 8]
TIES5 = [(0, 4, 4), (1, 3, 4), (0, 1, 1), (2, 5, 2), (0, 1, 8)]   # whole chain | a lead-in row | untied | flanks either side | period 1
LENS4, TIES4 = LENS5[:4], TIES5[:4]
T_R = 10


def _tie(x, lens, ties, is_angle=ANG, init=0, s=0.0, z=None, seed=0, t=0, seq_offset=0):
    """fd_tie_repeats -> (rc, out); `out` starts at the sentinel."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, Fx = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    ts = np.ascontiguousarray(np.asarray(ties, dtype=np.int32).reshape(B, 3))
    ang = np.ascontiguousarray(np.asarray(is_angle, dtype=bool).astype(np.uint8))
    zs = None if z is None else np.ascontiguousarray(z, dtype=np.float32)
    out = np.full_like(xs, SENTINEL)
    rc = _binding.load().fd_tie_repeats(0, P(xs), P(ls), P(ts), B, L, Fx, P(ang), int(init), C.c_float(s), P(zs), C.c_uint64(seed), int(t),
                                        C.c_int64(seq_offset), P(out))
    return rc, out


def _repeat(h, x0, lens, visits, coef, noise, seed, ties, n_visits=None, out=True):
    """fd_sample_repeat -> (rc, out); `out` starts at the sentinel."""
    x0 = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float32)
    ls = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    B = len(LENS4)
    vs = None if visits is None else np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    K = n_visits if n_visits is not None else len(vs)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float32)
    zs = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    ts = None if ties is None else np.ascontiguousarray(np.asarray(ties, dtype=np.int32).reshape(-1, 3))
    buf = np.full((B, L_R, F), SENTINEL, dtype=np.float32) if out else None
    rc = _binding.load().fd_sample_repeat(h, P(x0), P(ls), B, L_R, P(vs), K, P(cf), P(zs), C.c_uint64(seed), C.c_int64(0), P(ts), P(buf))
    return rc, buf


def _err():
    return _binding.load().fd_last_error()


def _seam_inputs(seed):
    """[5, 16, 6] within +-pi, the rows at or beyond a length at the sentinel; some unit rows have their copies placed
    either side of the +-pi seam, in an angular column of both is_angle runs (0) and in one that only the first wraps (3)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.1, 3.1, (5, L_R, F)).astype(np.float32)
    for b, ((start, period, units), col) in enumerate(zip(TIES5, (0, 3, 0, 0, 3))):
        for k in range(units):
            x[b, start + k * period, col] = np.float32((3.13, -3.14, 3.12, -3.11)[k % 4] + rng.uniform(-0.001, 0.001))
    for b, n in enumerate(LENS5):
        x[b, n:] = SENTINEL
    return x


# ---------------------------------------------------------------------------------- a. the hook against the reference
@pytest.mark.parametrize("is_angle", [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 1]])
def test_hook_equals_the_reference_bit_for_bit(gpu, is_angle):
    x = _seam_inputs(11)
    ok = _valid(LENS5, L_R)
    z = np.random.default_rng(12).standard_normal((5, L_R, F)).astype(np.float32)
    ang = np.array(is_angle, dtype=bool)
    for name, kw in (("s = 0", dict()), ("s = 0.3, explicit z", dict(s=0.3, z=z)), ("init", dict(init=1))):
        rc, got = _tie(x, LENS5, TIES5, is_angle, **kw)
        assert rc == 0, _err()
        want = rr.tie(x, LENS5, TIES5, ang, init=bool(kw.get("init", 0)), s=kw.get("s", 0.0), z=kw.get("z"))
        assert np.array_equal(_bits(got)[ok], _bits(want)[ok]), name
        assert (got[~ok] == SENTINEL).all(), name                                     # rows at or beyond a length: never written
        for b, (start, period, units) in enumerate(TIES5):                            # the copies are each other's bits
            for k in range(1, units):
                assert np.array_equal(_bits(got[b, start + k * period: start + (k + 1) * period]), _bits(got[b, start: start + period])), (name, b, k)
        if name != "init":
            assert (np.abs(got[..., ang][ok[..., ang]]) <= np.float32(np.pi)).all(), name
    # the seam: the circular mean of copies either side of +-pi stays next to it (the plain mean would be near 0)
    rc, got = _tie(x, LENS5, TIES5, is_angle)
    assert rc == 0 and ref_sampling.circ_dist(got[0, 0, 0], np.pi) < 0.05
    if ang[3]:
        assert ref_sampling.circ_dist(got[4, 0, 3], np.pi) < 0.05
    else:
        assert abs(got[4, 0, 3]) < 0.1
    # in place on the same input twice: the same bits
    rc, again = _tie(x, LENS5, TIES5, is_angle, s=0.3, z=z)
    rc2, once = _tie(x, LENS5, TIES5, is_angle, s=0.3, z=z)
    assert rc == 0 and rc2 == 0 and np.array_equal(_bits(again), _bits(once))


def test_hook_draws_the_update_kernels_philox_stream(gpu):
    """z null, s = 0.3: the draw is philox_normal(seed, t, seq_offset + b, l, f) at the copy-0 row.  Against the statement on
    ref_philox's draws: the two generators may differ by 2e-5 (the bound tests/test_gpu_parity.py sets between the device's
    logf / sincosf and numpy's), which s = 0.3 scales to 6e-6; the four roundings behind the draw (the product, the sum, the
    wrap's two sums) are of values below 8 and may each fall one half-ulp step, 2.4e-7, apart: 6e-6 + 4 * 2.4e-7 < 7e-6, on the
    circle for the wrapped columns."""
    x = _seam_inputs(13)
    ok = _valid(LENS5, L_R)
    ang = np.array([1, 1, 1, 0, 0, 1], dtype=bool)
    s = np.float32(0.3)
    for seed, t, seq_offset in ((1234, 5, 0), ((7 << 40) + 99, 0, 1 << 33)):
        rc, got = _tie(x, LENS5, TIES5, ang, s=s, z=None, seed=seed, t=t, seq_offset=seq_offset)
        assert rc == 0, _err()
        zr = ref_philox.philox_normal(seed, t, seq_offset, 5, L_R, F)
        want = rr.tie(x, LENS5, TIES5, ang, s=s, z=zr)
        d = np.where(ang, ref_sampling.circ_dist(got, want), np.abs(got.astype(np.float64) - want))[ok]
        print(f"seed {seed}, t {t}: max distance to the statement on ref_philox's draws {d.max():.3e}")
        assert d.max() < 7e-6
        rc, plain = _tie(x, LENS5, TIES5, ang)
        assert rc == 0 and np.abs(got - plain)[ok].max() > 0.1                        # ... and something was drawn
        for b, (start, period, units) in enumerate(TIES5):
            for k in range(1, units):
                assert np.array_equal(_bits(got[b, start + k * period: start + (k + 1) * period]), _bits(got[b, start: start + period]))
        rc, other = _tie(x, LENS5, TIES5, ang, s=s, z=None, seed=seed, t=t + 1, seq_offset=seq_offset)
        assert rc == 0 and not np.array_equal(other[ok], got[ok])                      # another step word: other draws


# ---------------------------------------------------------------------------------- b. the run is the chain of its hooks
def _run_inputs(betas, vi, seed):
    visits = VISIT_SETS[vi]
    coef = sampling.ddim_coefficients(betas, visits, 1.0)
    x0 = _inputs(4, L_R, seed=90 + seed).numpy()
    noise = np.random.default_rng(91 + seed).standard_normal((len(visits), 4, L_R, F)).astype(np.float32)
    return visits, coef, x0, noise


def _chain_of_hooks(h, x0, visits, coef, noise):
    rc, state = _tie(x0, LENS4, TIES4, init=1)
    assert rc == 0, _err()
    for i, t in enumerate(visits):
        a, b, s = coef[:, i]
        rc, _, state = _step_coef(h, state, t, LENS4, a, b, 0.0, None)
        assert rc == 0, _err()
        rc, state = _tie(state, LENS4, TIES4, s=s, z=noise[i])
        assert rc == 0, _err()
    return state


@pytest.mark.parametrize("precision", PRECISIONS)
def test_run_equals_the_chain_of_its_hooks_bit_for_bit(gpu, precision):
    """T = 10, B = 4, L = 16, explicit noise, eta = 1: fd_sample_repeat's out is the init tie, then per visit
    fd_p_sample_step_coef (s = 0, no z) followed by fd_tie_repeats (the visit's s and noise row); eager launches and packed
    rows give the same bits below the lengths."""
    _, _, pm = _pair(precision=precision, **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_R)
    h = pm.prepare(betas)
    ok = _valid(LENS4, L_R)
    for vi in range(len(VISIT_SETS)):
        visits, coef, x0, noise = _run_inputs(betas, vi, vi)
        assert (coef[2, :-1] != 0).all()
        rc, out = _repeat(h, x0, LENS4, visits, coef, noise, 0, TIES4)
        assert rc == 0, _err()
        want = _chain_of_hooks(h, x0, visits, coef, noise)
        assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), visits
        for option in ("use_graph", "varlen"):
            pm.set_option(option, 1 - (option == "use_graph"))
            rc, out2 = _repeat(h, x0, LENS4, visits, coef, noise, 0, TIES4)
            pm.set_option(option, int(option == "use_graph"))
            assert rc == 0 and np.array_equal(_bits(out2)[ok], _bits(out)[ok]), (visits, option)


# ---------------------------------------------------------------------------------- c. properties of the run's output
def test_run_output_is_periodic_and_its_backbone_has_screw_symmetry(gpu):
    """The tied copies are bit-identical and the free rows are not; the units of the NeRF backbone superpose to at most 1e-6 A
    (NeRF is fp64 and periodic rows give 8.5e-15 on the CPU; one row left untied costs at least 1e-2: the gate is four orders
    of magnitude from either); the untied sequence gets NaN."""
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_R)
    h = pm.prepare(betas)
    visits, coef, x0, noise = _run_inputs(betas, 1, 5)
    rc, out = _repeat(h, x0, LENS4, visits, coef, noise, 0, TIES4)
    assert rc == 0, _err()
    for b, (start, period, units) in enumerate(TIES4):
        first = out[b, start: start + period]
        for k in range(1, units):
            assert np.array_equal(_bits(out[b, start + k * period: start + (k + 1) * period]), _bits(first)), (b, k)
        free = [l for l in range(LENS4[b]) if units > 1 and not start <= l < start + period * units]
        for l in free:
            assert not np.array_equal(out[b, l], first[(l - start) % period]), (b, l)
    assert len([l for l in range(LENS4[3]) if not 2 <= l < 12]) == 4                  # two flank rows either side
    coords = nerf.build_backbones([out[b, :n] for b, n in enumerate(LENS4)], NAMES, center_coords=False)
    cols = [np.array(v) for v in zip(*TIES4)]
    rmsd = structures.repeat_rmsd(coords, *cols)
    print("repeat RMSD per sequence:", rmsd.tolist())
    assert np.isnan(rmsd[2]) and (rmsd[[0, 1, 3]] <= 1e-6).all()
    # the same run without ties: the units do not superpose
    rc, loose = _repeat(h, x0, LENS4, visits, coef, noise, 0, [(0, 1, 1)] * 4)
    assert rc == 0, _err()
    loose_rmsd = structures.repeat_rmsd(nerf.build_backbones([loose[b, :n] for b, n in enumerate(LENS4)], NAMES, center_coords=False), *cols)
    assert (loose_rmsd[[0, 1, 3]] > 1e-2).all(), loose_rmsd


# ---------------------------------------------------------------------------------- d. errors and the call history
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(precision="f16x3", **MODEL_D)
    betas = beta_schedules.cosine_beta_schedule(T_R)
    h = pm.prepare(betas)
    visits, coef, x0, _ = _run_inputs(betas, 0, 7)
    rc, before = _strided(h, x0, LENS4, visits, coef, 5, 0)
    assert rc == 0, _err()
    nan_b, inf_s = coef.copy(), coef.copy()
    nan_b[1, 2] = np.nan
    inf_s[2, 0] = np.inf

    def tie_with(b, row):
        t = [list(r) for r in TIES4]
        t[b] = list(row)
        return t

    bad = [(dict(x0=None), b"null"), (dict(lens=None), b"null"), (dict(out=False), b"null"), (dict(ties=None), b"null"),
           (dict(visits=None, n_visits=4), b"visits is null"), (dict(coef=None), b"coef is null"), (dict(n_visits=0), b"n_visits = 0"),
           (dict(visits=[10, 5, 2, 0]), b"visits[0] = 10 outside"), (dict(visits=[8, 5, 5, 0]), b"visits[2] = 5 follows 5"),
           (dict(coef=nan_b), b"coef[1][2]"), (dict(coef=inf_s), b"coef[2][0]"),
           (dict(lens=[16, 13, 0, 14]), b"lens[2]=0"), (dict(lens=[17, 13, 9, 14]), b"lens[0]=17"),
           (dict(ties=tie_with(0, (-1, 4, 4))), b"tie[0]"), (dict(ties=tie_with(1, (1, 0, 4))), b"tie[1]"),
           (dict(ties=tie_with(2, (0, 1, 0))), b"tie[2]"), (dict(ties=tie_with(3, (2, 5, 3))), b"tie[3]"),
           (dict(ties=tie_with(1, (2, 3, 4))), b"tie[1]"), (dict(lens=[16, 12, 9, 14]), b"tie[1]")]
    for kw, word in bad:
        a = dict(x0=x0, lens=LENS4, visits=visits, coef=coef, ties=TIES4, n_visits=None, out=True)
        a.update(kw)
        rc, out = _repeat(h, a["x0"], a["lens"], a["visits"], a["coef"], None, 5, a["ties"], n_visits=a["n_visits"], out=a["out"])
        assert rc == -1 and word in _err(), (word, rc, _err())
        assert out is None or (out == SENTINEL).all(), word
    # after the failed calls the strided sampler is what it was
    rc, after_failed = _strided(h, x0, LENS4, visits, coef, 5, 0)
    assert rc == 0 and np.array_equal(_bits(after_failed), _bits(before))
    # a repeat run (Philox draws), then the strided sampler again: the per-run values are clean
    rc, run = _repeat(h, x0, LENS4, visits, coef, None, 5, TIES4)
    assert rc == 0 and np.isfinite(run[_valid(LENS4, L_R)]).all(), _err()
    rc, after = _strided(h, x0, LENS4, visits, coef, 5, 0)
    assert rc == 0 and np.array_equal(_bits(after), _bits(before))
    rc, again = _repeat(h, x0, LENS4, visits, coef, None, 5, TIES4)
    assert rc == 0 and np.array_equal(_bits(again), _bits(run))
    rc, other = _repeat(h, x0, LENS4, visits, coef, None, 6, TIES4)
    assert rc == 0 and not np.array_equal(other[_valid(LENS4, L_R)], run[_valid(LENS4, L_R)])   # the seed reaches the tie launch


# ---------------------------------------------------------------------------------- e. Python end to end
def _copies_equal(s, start, period, units):
    return all(np.array_equal(_bits(s[start + k * period: start + (k + 1) * period]), _bits(s[start: start + period])) for k in range(1, units))


def test_sample_repeats_end_to_end_on_a_tiny_model(gpu):
    _, _, pm = _pair(seed=11, precision="f16x3")
    inner = datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=np.array([-1.3, 1.1, 3.0, 1.95, 2.03, 2.12], np.float32))
    ds = datasets.NoisedAnglesDataset(inner, timesteps=20, beta_schedule="cosine")
    lengths, period, units, start = [30, 41, 30], [7, 5, 30], [4, 8, 1], [1, 0, 0]
    kw = dict(start=start, num_steps=6, batch_size=2)   # two calls: two sequences, then one
    torch.manual_seed(3)
    got = sampling.sample_repeats(pm, ds, lengths, period, units, **kw)
    assert [s.shape for s in got] == [(l, F) for l in lengths] and all(s.dtype == np.float32 for s in got)
    for s, p, r, a in zip(got, period, units, start):
        assert np.isfinite(s).all() and (s >= -np.float32(np.pi)).all() and (s < np.float32(np.pi)).all()
        assert _copies_equal(s, a, p, r)
    assert not np.array_equal(got[0][0], got[0][7]) and not np.array_equal(got[2][0], got[2][1])   # a free row; an untied chain
    torch.manual_seed(3)
    again = sampling.sample_repeats(pm, ds, lengths, period, units, **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, got))
    rmsd = structures.repeat_rmsd(nerf.build_backbones(got, NAMES, center_coords=False), start, period, units)
    assert (rmsd[:2] <= 1e-6).all() and np.isnan(rmsd[2]), rmsd
    scalar = sampling.sample_repeats(pm, ds, [25, 26], 6, 4, start=1, num_steps=4, eta=0.0)   # scalars; eta = 0 draws nothing
    assert all(_copies_equal(s, 1, 6, 4) for s in scalar)


def test_script_writes_backbones_with_superposing_units(gpu, tmp_path):
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * 6, "gaussian_fourier", "mlp", seed=8)
    mdir, out = str(tmp_path / "model"), str(tmp_path / "out")
    _write_model_dir(mdir, o32, pad=64, T=20, offset=np.array([0.1, -0.2, 0.3, 1.9, 2.0, 2.1], dtype=np.float32))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample_repeats.py"), "-m", mdir, "-o", out, "-n", "3", "--period", "6",
                        "--units", "4", "--flank_n", "2", "--flank_c", "3", "--num_steps", "5", "--seed", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "repeat_rmsd.json", "sampled_angles", "sampled_pdb"]
    assert sorted(os.listdir(os.path.join(out, "sampled_pdb"))) == [f"generated_{i}.pdb" for i in range(3)]
    assert sorted(os.listdir(os.path.join(out, "sampled_angles"))) == [f"generated_{i}.csv.gz" for i in range(3)]
    with open(os.path.join(out, "repeat_rmsd.json")) as fh:
        report = json.load(fh)
    assert report["length"] == 29 and sorted(report["repeat_rmsd"]) == [f"generated_{i}.pdb" for i in range(3)]
    assert all(v is not None and 0 <= v <= 1e-6 for v in report["repeat_rmsd"].values()), report["repeat_rmsd"]
