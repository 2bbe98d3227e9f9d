"""Few-step motif scaffolding on the device (fd_sample_strided_inpaint, fd_sample_strided_inpaint_resample,
fd_p_sample_step_coef_inpaint, sampling.scaffold(..., num_steps=...)) against the float32 statement of
tests/strided_inpaint_reference.py and against the composition of the entries that existed before them.  The update and the
replacement are compared BIT FOR BIT; the network's prediction and the free-running loop with the tolerances of the plain
sampler's tests (tests/test_gpu_parity.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inpaint_reference as ipr
import resample_reference as rsr
import strided_inpaint_reference as sir
import strided_reference as sref
from conftest import GOLDEN
from foldingdiff_amd import _binding, beta_schedules, datasets, nerf, sampling, structures
from oracle import ref_philox, ref_sampling
from test_gpu_parity import FWD_TOL, PRECISIONS, STEP_TOL, _c1_models, _free_running_check, _inputs, _pair, _record, _share_time_table
from test_inpaint_gpu import _device_draws, _masks, _sample_inpaint, _sample_plain
from test_resample_gpu import _jump
from test_strided_gpu import ANG, C1_LENS, F, SENTINEL, _bits, _forward, _rows, _strided, _valid

pytestmark = pytest.mark.gpu
P = _binding.ptr


def _arr(a, dtype=np.float32):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _step_coef_inpaint(h, x, t, lens, a, b, s, z, level_out, known, fixed, kcoef, zk, wrap=1):
    """fd_p_sample_step_coef_inpaint -> (rc, eps_out, x_out); both outputs start at the sentinel."""
    xs = _arr(x)
    B, L, _ = xs.shape
    ls, zs, zks = _arr(lens, np.int32), _arr(z), _arr(zk)
    eps, out = np.full_like(xs, SENTINEL), np.full_like(xs, SENTINEL)
    rc = _binding.load().fd_p_sample_step_coef_inpaint(h, P(xs), int(t), P(ls), B, L, float(a), float(b), float(s), P(zs), wrap,
                                                       int(level_out), P(known), P(fixed), P(kcoef), P(zks), P(eps), P(out))
    return rc, eps, out


def _strided_inpaint(h, x0, lens, visits, coef, known, fixed, kcoef, seed, full_history, noise=None, known_noise=None, n_visits=None):
    """fd_sample_strided_inpaint -> (rc, out); `out` starts at the sentinel."""
    x0 = _arr(x0)
    B, L, _ = x0.shape
    ls, vs, cf, zs, kz = _arr(lens, np.int32), _arr(visits, np.int32), _arr(coef), _arr(noise), _arr(known_noise)
    K = n_visits if n_visits is not None else len(vs)
    out = np.full((_rows(max(K, 1), max(full_history, 0)), B, L, F), SENTINEL, dtype=np.float32)
    rc = _binding.load().fd_sample_strided_inpaint(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(zs), P(known), P(fixed), P(kcoef), P(kz),
                                                   C.c_uint64(seed), C.c_int64(0), P(out), full_history)
    return rc, out


def _strided_resample(h, x0, lens, grid, coef, run, jump_coef, known, fixed, kcoef, seed, n_grid=None, n_run=None):
    """fd_sample_strided_inpaint_resample -> (rc, out [B, L, F]); `out` starts at the sentinel."""
    x0 = _arr(x0)
    B, L, _ = x0.shape
    ls, gs, cf, rs = _arr(lens, np.int32), _arr(grid, np.int32), _arr(coef), _arr(run, np.int32)
    jc = None if jump_coef is None or len(jump_coef) == 0 else _arr(jump_coef)
    out = np.full((B, L, F), SENTINEL, dtype=np.float32)
    rc = _binding.load().fd_sample_strided_inpaint_resample(
        h, P(x0), P(ls), B, L, P(gs), (0 if gs is None else len(gs)) if n_grid is None else n_grid, P(cf), P(rs),
        (0 if rs is None else len(rs)) if n_run is None else n_run, P(jc), P(known), P(fixed), P(kcoef), C.c_uint64(seed), C.c_int64(0), P(out))
    return rc, out


def _err():
    return _binding.load().fd_last_error()


# ---------------------------------------------------------------------------------- 1. the hook, every update kernel
@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_conditioned_visit_bit_for_bit_in_every_update_kernel(gpu, precision, hidden, heads):
    """The row-image kernel (f16x3), the 16-lanes-per-token kernel (f32, d % 64 == 0) and the one-wave-per-token kernel (f32,
    d = 96).  One-layer models, L = 24, B = 3, T = 8, lens 24, 17, 9, visits 7, 4, 2, 0: every visit but the last lands on a level
    other than its own t (5, 3, 1; then 0), so a replacement at level t cannot pass.  The mask fixes scattered single elements (24), whole rows
    3-11 (17) and everything below the length of the shortest sequence, its last real row included.  x_out carries the bits of
    the restatement applied to the hook's own eps_out; eps_out carries fd_forward's bits and is within FWD_TOL of the oracle's
    forward.  No tolerance of its own."""
    o32, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, lens, visits = 8, [24, 17, 9], np.array([7, 4, 2, 0], dtype=np.int32)
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    known, fixed = _masks([17, 24, 24, 9], 24, rows=(3, 12))
    known, fixed = known[[2, 1, 3]].copy(), fixed[[2, 1, 3]].copy()
    assert fixed[0].any() and not fixed[0].all() and fixed[1, 3:12].all() and not fixed[1, 12:].any() and fixed[2, 8].all() and not fixed[2, 9:].any()
    fx = fixed.astype(bool)
    ok = _valid(lens, 24)
    levels = sir.landing_levels(visits)
    assert levels == [5, 3, 1, 0] and all(q != t for q, t in zip(levels[:-1], visits[:-1]))
    g = torch.Generator().manual_seed(29)
    worst = 0.0
    for eta in (0.0, 0.5):
        coef = sampling.ddim_coefficients(betas, visits, eta)
        for wrap in (0, 1):
            ang = ANG if wrap else [False] * F
            x = _inputs(3, 24, seed=5).numpy()
            for i, (t, q) in enumerate(zip(visits, levels)):
                a, b, s = coef[:, i]
                z = torch.randn(3, 24, F, generator=g).numpy()
                zk = torch.randn(3, 24, F, generator=g).numpy()
                rc, eps, out = _step_coef_inpaint(h, x, t, lens, a, b, s, None if s == 0 else z, q, known, fixed, kcoef,
                                                  zk if q > 0 else None, wrap)
                assert rc == 0, _err()
                want = sir.visit(x, eps, a, b, s, z, known, fixed, q, kcoef, zk, ang)
                assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), (eta, wrap, i)
                assert np.array_equal(_bits(eps)[ok], _bits(_forward(h, x, t, lens))[ok]), (eta, wrap, i)
                e = float(np.abs(eps - sref.forward(o32, x, t, lens).numpy())[ok].max())
                worst = max(worst, e)
                assert e <= FWD_TOL, (eta, wrap, i, e)
                if q == 0:
                    assert np.array_equal(_bits(out)[fx], _bits(known)[fx])
                else:   # the level-t mistake gives other bits: the comparison above can fail
                    assert not np.array_equal(ipr.known_at_level(known, int(t), kcoef, zk, ang)[fx], want[fx])
                # a free element is fd_p_sample_step_coef's: the conditioning touches the fixed ones only
                free = ok & ~fx
                assert np.array_equal(_bits(out)[free], _bits(sref.update(x, eps, a, b, s, z, ang))[free])
                x = np.where(ok, want, x).astype(np.float32)
    _record(f"strided_inpaint_hook_d{hidden}_{precision}", max_eps=worst)


# ---------------------------------------------------------------------------------- 2. the loop is the chain of hooks
SETTINGS = [([9, 6, 3, 0], 0.0), ([9, 6, 3, 0], 0.5), ([9, 7, 4, 2, 0], 0.0), ([9, 7, 4, 2, 0], 0.5)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_equals_the_chain_of_hooks_bit_for_bit(gpu, precision):
    """C1 (d = 192, 6 layers, L = 64, B = 4, T = 10).  Row i of the full history is the hook applied to row i - 1 with visit
    i's coefficients, draws and landing level, bit for bit; row -1 is x_init after the start replacement at level
    visits[0] + 1.  With explicit arrays z is row i of `noise` and the replacement's draws row i + 1 of `known_noise` (row 0:
    the start point).  With Philox the hook is fed the device generator's own draws of word t and of word 0x80000000 | q,
    each within 2e-5 of ref_philox (the bound tests/test_gpu_parity.py sets between the device's logf / sincosf and numpy's).
    The thinned history, the final-only run, eager launches and packed rows give the same bits below the lengths; with an
    all-zero mask the result is fd_sample_strided's."""
    g, _, _, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    B, L = 4, 64
    x0 = g["x0"]
    ok = _valid(C1_LENS, L)
    known, fixed = _masks(C1_LENS, L)
    fx = fixed.astype(bool)
    nothing = np.zeros_like(fixed)
    seed = 977
    for visits, eta in SETTINGS:
        K = len(visits)
        levels = sir.landing_levels(visits)
        coef = sampling.ddim_coefficients(betas, np.asarray(visits, dtype=np.int32), eta)
        gen = torch.Generator().manual_seed(31)
        explicit = torch.randn(K, B, L, F, generator=gen).numpy()
        explicit_known = torch.randn(K + 1, B, L, F, generator=gen).numpy()
        for noise, kz in ((explicit, explicit_known), (None, None)):
            kw = dict(noise=noise, known_noise=kz)
            rc, full = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, fixed, kcoef, seed, 1, **kw)
            assert rc == 0, _err()
            assert full.shape == (K, B, L, F) and np.isfinite(full[:, ok]).all()

            def tagged(level):
                zk = _device_draws(h, seed, ipr.TAG | level, B, L)
                assert np.abs(zk - ipr.tagged_draw(seed, level, 0, B, L, F)).max() < 2e-5, (visits, level)
                return zk

            prev = ipr.replace(x0, known, fixed, visits[0] + 1, kcoef, kz[0] if kz is not None else tagged(visits[0] + 1), ANG)
            for i, (t, q) in enumerate(zip(visits, levels)):
                a, b, s = coef[:, i]
                if s == 0:
                    z = None
                elif noise is not None:
                    z = noise[i]
                else:
                    z = _device_draws(h, seed, t, B, L)
                    assert np.abs(z - ref_philox.philox_normal(seed, int(t), 0, B, L, F)).max() < 2e-5, (visits, i)
                zk = None if q == 0 else kz[i + 1] if kz is not None else tagged(q)
                rc, _, want = _step_coef_inpaint(h, prev, t, C1_LENS, a, b, s, z, q, known, fixed, kcoef, zk)
                assert rc == 0, _err()
                assert np.array_equal(_bits(full[i])[ok], _bits(want)[ok]), (visits, eta, noise is None, i)
                prev = full[i]
            assert np.array_equal(_bits(full[-1])[fx], _bits(known)[fx])
            rc, final = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, fixed, kcoef, seed, 0, **kw)
            assert rc == 0 and np.array_equal(_bits(final[0])[ok], _bits(full[-1])[ok])
            rc, every2 = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, fixed, kcoef, seed, 2, **kw)
            states = [1, 3] if K == 4 else [1, 3, 4]
            assert rc == 0 and every2.shape[0] == len(states)
            assert np.array_equal(_bits(every2)[:, ok], _bits(full[states])[:, ok]), (visits, states)
            pm.set_option("use_graph", 0)
            rc, eager = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, fixed, kcoef, seed, 1, **kw)
            pm.set_option("use_graph", 1)
            assert rc == 0 and np.array_equal(_bits(eager)[:, ok], _bits(full)[:, ok]), (visits, "eager")
            pm.set_option("varlen", 1)
            rc, packed = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, fixed, kcoef, seed, 1, **kw)
            pm.set_option("varlen", 0)
            assert rc == 0 and np.array_equal(_bits(packed)[:, ok], _bits(full)[:, ok]), (visits, "varlen")
            rc, empty = _strided_inpaint(h, x0, C1_LENS, visits, coef, known, nothing, kcoef, seed, 1, **kw)
            rc2, plain = _strided(h, x0, C1_LENS, visits, coef, seed, 1, noise=noise)
            assert rc == 0 and rc2 == 0 and np.array_equal(_bits(empty)[:, ok], _bits(plain)[:, ok]), (visits, "all-zero mask")
            assert not np.array_equal(full[-1][ok & ~fx], plain[-1][ok & ~fx])       # the conditioning reaches the free elements


# ---------------------------------------------------------------------------------- 3. the full grid against fd_sample_inpaint
@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_grid_against_fd_sample_inpaint(gpu, precision):
    """K = T visits with eta = 1 land on the levels fd_sample_inpaint's steps leave, with the same seed and tag: the FIXED
    elements of every history row carry fd_sample_inpaint's bits.  The free elements follow another arithmetic (a x + b eps
    + s z against p_sample's statement, coefficients equal to 2.7e-13 before rounding): teacher-forced from
    fd_sample_inpaint's previous row, with the device's own draws, a visit stays within STEP_TOL of its next row."""
    g, _, _, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    B, L, seed = 4, 64, 4242
    known, fixed = _masks(C1_LENS, L)
    fx = fixed.astype(bool)
    ok = _valid(C1_LENS, L)
    visits = np.arange(T - 1, -1, -1, dtype=np.int32)
    coef = sampling.ddim_coefficients(betas, visits, 1.0)
    rc, want = _sample_inpaint(h, g["x0"], C1_LENS, T - 1, known, fixed, kcoef, seed, 1)
    assert rc == 0, _err()
    rc, got = _strided_inpaint(h, g["x0"], C1_LENS, visits, coef, known, fixed, kcoef, seed, 1)
    assert rc == 0, _err()
    assert got.shape == want.shape == (T, B, L, F)
    assert np.array_equal(_bits(got)[:, fx], _bits(want)[:, fx])
    prev = ipr.replace(g["x0"], known, fixed, T, kcoef, _device_draws(h, seed, ipr.TAG | T, B, L), ANG)
    worst = 0.0
    for i, t in enumerate(visits):
        a, b, s = coef[:, i]
        z = None if s == 0 else _device_draws(h, seed, int(t), B, L)
        zk = None if t == 0 else _device_draws(h, seed, ipr.TAG | int(t), B, L)
        rc, _, out = _step_coef_inpaint(h, prev, t, C1_LENS, a, b, s, z, int(t), known, fixed, kcoef, zk)
        assert rc == 0, _err()
        assert np.array_equal(_bits(out)[fx], _bits(want[i])[fx]), i
        e = float(ref_sampling.circ_dist(out, want[i])[ok & ~fx].max())
        worst = max(worst, e)
        assert e <= STEP_TOL, (i, e)
        prev = want[i]
    _record(f"strided_inpaint_full_grid_{precision}", max=worst, steps=T)


# ---------------------------------------------------------------------------------- 4. the resampled run is its composition
def _compose(h, x0, lens, grid, coef, run, jump_coef, known, fixed, kcoef, seed):
    """The resampled run from fd_sample_strided_inpaint and fd_inpaint_jump, [n_run, B, L, F]: per segment the strided
    conditioned run over the rest of the grid with the segment's seed and the whole history (the rows of the segment's
    visits are kept), then the jump into the next."""
    grid = [int(t) for t in grid]
    x = np.ascontiguousarray(x0, dtype=np.float32)
    rows = []
    for s, (i, j) in enumerate(sir.segments(grid, run)):
        key = rsr.seeds(seed, s)
        if s > 0:
            rc, x = _jump(h, x, lens, int(run[i]) + 1, jump_coef[s - 1][0], jump_coef[s - 1][1], known, fixed, kcoef, key)
            assert rc == 0, _err()
        at = grid.index(int(run[i]))
        rc, hist = _strided_inpaint(h, x, lens, grid[at:], coef[:, at:], known, fixed, kcoef, key, 1)
        assert rc == 0, _err()
        rows.extend(hist[: j - i])
        x = hist[j - i - 1]
    return np.stack(rows)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_resampled_run_equals_its_composition(gpu, precision):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision=precision)
    T, B, L, lens, seed = 25, 4, 64, [50, 33, 64, 12], 5
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    x0 = _inputs(B, L, seed=4).numpy()
    known, fixed = _masks(lens, L)
    fx = fixed.astype(bool)
    grid = sampling.ddim_visits(T, 8)
    coef = sampling.ddim_coefficients(betas, grid, 0.5)
    run = sampling.strided_resample_schedule(grid, 2, 2)
    jc = sampling.strided_jump_coef(betas, grid, run)
    assert len(run) == 8 + 3 * 2 and jc.shape == (3, 2)
    sir.check_run(grid, run)
    visits = np.array([T - 1, 11, 4, 0], dtype=np.int32)
    vcoef = sampling.ddim_coefficients(betas, visits, 0.5)
    before = (_sample_plain(h, x0, lens, T - 1, seed, 0), _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, seed, 0)[1],
              _strided(h, x0, lens, visits, vcoef, seed, 0)[1])
    composed = _compose(h, x0, lens, grid, coef, run, jc, known, fixed, kcoef, seed)[-1]
    runs = {}
    for graph, varlen in ((1, 0), (0, 0), (1, 1), (0, 1)):
        pm.set_option("use_graph", graph)
        pm.set_option("varlen", varlen)
        rc, runs[graph, varlen] = _strided_resample(h, x0, lens, grid, coef, run, jc, known, fixed, kcoef, seed)
        assert rc == 0, _err()
    pm.set_option("use_graph", 1)
    pm.set_option("varlen", 0)
    assert np.array_equal(_bits(runs[1, 0]), _bits(composed))
    assert np.array_equal(_bits(runs[0, 0]), _bits(composed))
    for b, n in enumerate(lens):
        for graph in (1, 0):
            assert np.array_equal(_bits(runs[graph, 1][b, :n]), _bits(composed[b, :n])), (graph, b)
    assert np.array_equal(_bits(runs[1, 0])[fx], _bits(known)[fx])
    # a run without a jump through the resample entry is fd_sample_strided_inpaint's (jump_coef null)
    rc, single = _strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, seed, 0)
    assert rc == 0, _err()
    rc, flat = _strided_resample(h, x0, lens, grid, coef, grid, None, known, fixed, kcoef, seed)
    assert rc == 0, _err()
    assert np.array_equal(_bits(flat), _bits(single[0]))
    free = _valid(lens, L) & ~fx
    assert not np.array_equal(runs[1, 0][free], flat[free])             # the jumps change the free elements: the check can fail
    # the plain, the conditioned and the strided sampler are what they were: every field is cleared
    after = (_sample_plain(h, x0, lens, T - 1, seed, 0), _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, seed, 0)[1],
             _strided(h, x0, lens, visits, vcoef, seed, 0)[1])
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------- 5. against the oracle, free-running
FREE_VISITS = np.array([8, 5, 2, 0], dtype=np.int32)   # every |b| <= 3.6, as in tests/test_strided_gpu.py, under which STEP_TOL holds
FREE_SEED = 20240917   # the draws' seed, chosen on the CPU: the oracle's own fp32 and fp64 loops satisfy the check (asserted below)
_FREE_REF = {}


def _free_reference(o32, o64, x0, betas, T, eta, known, fixed, kcoef):
    """The restatement's loop with the fp32 and the fp64 oracle on explicit draws; computed once, shared by the precisions."""
    if eta not in _FREE_REF:
        coef = sampling.ddim_coefficients(betas, FREE_VISITS, eta)
        assert np.abs(coef[1]).max() <= 3.6
        gen = torch.Generator().manual_seed(FREE_SEED)
        z = torch.randn(len(FREE_VISITS), 4, 64, F, generator=gen).numpy()
        kz = torch.randn(len(FREE_VISITS) + 1, 4, 64, F, generator=gen).numpy()
        _share_time_table(o64, o32, T)
        _FREE_REF[eta] = (coef, z, kz, sir.loop(o32, C1_LENS, x0, FREE_VISITS, coef, ANG, known, fixed, kcoef, z, kz),
                          sir.loop(o64, C1_LENS, x0, FREE_VISITS, coef, ANG, known, fixed, kcoef, z, kz))
    return _FREE_REF[eta]


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_free_running_c1_against_the_oracle(gpu, precision, eta):
    g, o32, o64, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    kcoef = sampling.inpaint_levels(betas)
    known, fixed = _masks(C1_LENS, 64)
    coef, z, kz, want32, want64 = _free_reference(o32, o64, g["x0"], betas, T, eta, known, fixed, kcoef)
    ok = _valid(C1_LENS, 64)
    sel = lambda a: np.where(ok, a, 0.0)   # noqa: E731  (positions beyond a length are nobody's result)
    # the condition on the start and the draws: the oracle's own two precisions stay together, 4 of 4 sequences clean
    _free_running_check(f"strided_inpaint_free_c1_oracle32_vs_64_eta{eta}", sel(want32), sel(want64), tol=STEP_TOL, min_clean=4)
    rc, got = _strided_inpaint(h, g["x0"], C1_LENS, FREE_VISITS, coef, known, fixed, kcoef, 0, 1, noise=z, known_noise=kz)
    assert rc == 0, _err()
    fx = fixed.astype(bool)
    assert np.array_equal(_bits(got)[:, fx], _bits(want32)[:, fx])       # explicit draws: the fixed elements are the statement's bits
    _free_running_check(f"strided_inpaint_free_c1_{precision}_eta{eta}", sel(got), sel(want32), tol=STEP_TOL, min_clean=4)


# ---------------------------------------------------------------------------------- 6. the contract
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision="f16x3")
    T = 12
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    lib = _binding.load()
    lens = [50, 33, 64, 12]
    x0 = _inputs(4, 64, seed=4).numpy()
    grid = np.array([11, 7, 3, 0], dtype=np.int32)
    coef = sampling.ddim_coefficients(betas, grid, 0.5)
    known, fixed = _masks(lens, 64)
    kcoef = sampling.inpaint_levels(betas)
    run = sampling.strided_resample_schedule(grid, 1, 2)
    jc = sampling.strided_jump_coef(betas, grid, run)
    assert run.tolist() == [11, 7, 7, 3, 3, 0, 0] and len(jc) == 3
    before = _sample_plain(h, x0, lens, T - 1, 5, 1)
    nan_coef, inf_coef = coef.copy(), coef.copy()
    nan_coef[1, 2] = np.nan
    inf_coef[2, 0] = np.inf
    beyond = fixed.copy()
    beyond[1, 33, 4] = 1                      # the first position past lens[1]
    shared = [(dict(grid=None, n_grid=4), b"visits is null"), (dict(coef=None), b"coef is null"), (dict(n_grid=0), b"n_visits = 0"),
              (dict(grid=[12, 7, 3, 0]), b"visits[0] = 12 outside"), (dict(grid=[11, 7, -1, 0]), b"visits[2] = -1 outside"),
              (dict(grid=[11, 7, 7, 0]), b"visits[2] = 7 follows 7"), (dict(grid=[11, 3, 7, 0]), b"visits[2] = 7 follows 3"),
              (dict(coef=nan_coef), b"coef[1][2]"), (dict(coef=inf_coef), b"coef[2][0]"),
              (dict(fixed=beyond), b"fixed element beyond"), (dict(known=None), b"known is null"), (dict(fixed=None), b"fixed is null"),
              (dict(kcoef=None), b"known_coef")]
    for kw, word in shared:
        a = dict(grid=grid, coef=coef, n_grid=None, known=known, fixed=fixed, kcoef=kcoef)
        a.update(kw)
        rc, out = _strided_inpaint(h, x0, lens, a["grid"], a["coef"], a["known"], a["fixed"], a["kcoef"], 5, 1, n_visits=a["n_grid"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all(), word
        rc, out = _strided_resample(h, x0, lens, a["grid"], a["coef"], run, jc, a["known"], a["fixed"], a["kcoef"], 5, n_grid=a["n_grid"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all(), word
    rc, out = _strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, 5, -1)
    assert rc == -1 and b"full_history" in lib.fd_last_error() and (out == SENTINEL).all()

    def edit(i, v):
        out = run.copy()
        out[i] = v
        return out

    def coefs(i, k, v):
        out = jc.copy()
        out[i, k] = v
        return out

    resample = [(dict(run=None), b"run is null"), (dict(n_run=0), b"n_run"),
                (dict(run=edit(0, 7)), b"run[0]"), (dict(run=edit(-1, 3)), b"run[%d]" % (len(run) - 1)),
                (dict(run=edit(2, 5)), b"run[2]"),                        # not on the grid
                (dict(run=edit(2, 12)), b"run[2]"), (dict(run=edit(2, -1)), b"run[2]"),
                (dict(run=edit(2, 0)), b"run[2]"),                        # two visits down at once: neither a descent nor a jump
                (dict(jc=None), b"jump_coef is null"),
                (dict(jc=coefs(1, 0, np.nan)), b"jump 1"), (dict(jc=coefs(0, 1, 1.5)), b"jump 0"), (dict(jc=coefs(2, 0, -0.25)), b"jump 2"),
                (dict(jc=coefs(1, 1, np.inf)), b"jump 1")]
    for kw, word in resample:
        a = dict(run=run, jc=jc, n_run=None)
        a.update(kw)
        rc, out = _strided_resample(h, x0, lens, grid, coef, a["run"], a["jc"], known, fixed, kcoef, 5, n_run=a["n_run"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all(), word
        after = _sample_plain(h, x0, lens, T - 1, 5, 1)        # a rejected call changes nothing
        assert np.array_equal(_bits(after), _bits(before)), word
    z = np.zeros((4, 64, F), dtype=np.float32)
    hook = [(dict(s=0.5, z=None), b"z is required"), (dict(a=np.nan), b"not finite"), (dict(b=np.inf), b"not finite"),
            (dict(s=-np.inf), b"not finite"), (dict(level=-1), b"level_out = -1"), (dict(level=T + 1), b"level_out = %d" % (T + 1)),
            (dict(level=1, zk=None), b"z_known is required"), (dict(level=T, zk=None), b"z_known is required"),
            (dict(fixed=beyond), b"fixed element beyond"), (dict(known=None), b"known is null"), (dict(kcoef=None), b"known_coef"),
            (dict(t=T), b""), (dict(t=-1), b"")]
    for kw, word in hook:
        a = dict(t=3, a=1.0, b=-1.0, s=0.0, z=z, level=2, known=known, fixed=fixed, kcoef=kcoef, zk=z)
        a.update(kw)
        rc, eps, out = _step_coef_inpaint(h, x0, a["t"], lens, a["a"], a["b"], a["s"], a["z"], a["level"], a["known"], a["fixed"], a["kcoef"],
                                          a["zk"])
        assert rc == -1 and word in lib.fd_last_error(), (kw, rc, lib.fd_last_error())
        assert (out == SENTINEL).all() and (eps == SENTINEL).all(), kw
    # level 0 needs no z_known, s == 0 no z
    rc, _, out = _step_coef_inpaint(h, x0, 3, lens, 1.0, -1.0, 0.0, None, 0, known, fixed, kcoef, None)
    assert rc == 0 and np.array_equal(_bits(out)[fixed.astype(bool)], _bits(known)[fixed.astype(bool)]), lib.fd_last_error()
    # the same calls with nothing wrong; then the plain sampler is what it was, and so are the new runs
    rc, one = _strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, 5, 1)
    assert rc == 0 and np.isfinite(one[:, _valid(lens, 64)]).all(), lib.fd_last_error()
    rc, two = _strided_resample(h, x0, lens, grid, coef, run, jc, known, fixed, kcoef, 5)
    assert rc == 0 and np.isfinite(two[_valid(lens, 64)]).all(), lib.fd_last_error()
    after = _sample_plain(h, x0, lens, T - 1, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))
    rc, again = _strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, 5, 1)
    assert rc == 0 and np.array_equal(_bits(again), _bits(one))


# ---------------------------------------------------------------------------------- 7. Python end to end
def test_scaffold_in_a_few_steps_reproduces_the_motif_backbone(gpu, monkeypatch):
    """sampling.scaffold(..., num_steps=5) and (..., num_steps=6, jump_length=2, n_resample=2) on rows 5-16 of 1CRN's angles,
    T = 20, total lengths 30 and 31, a tiny model: the fixed rows are the motif's bits and the motif's residues of the
    NeRF-built backbones superpose on the motif's own backbone within n_angles * 1e-6 * extent (1.3e-3 A), the first-order
    angular bound of the end-to-end test of tests/test_inpaint_gpu.py."""
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    _, _, pm = _pair(seed=11, precision="f16x3")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64, mean_offset=None), timesteps=20,
                                      beta_schedule="cosine")
    names = ds.feature_names["angles"]
    feats = structures.featurize([os.path.join(GOLDEN, "1CRN.pdb")], distances=[], angles=names)[0]
    motif = feats[names].values[5:17].astype(np.float32)
    assert motif.shape == (12, F) and np.isfinite(motif).all()
    calls = []
    real = sampling._run_fd_strided_inpaint

    def spy(*a):
        calls.append((len(a[3]), None if a[8] is None else len(a[8])))
        return real(*a)

    monkeypatch.setattr(sampling, "_run_fd_strided_inpaint", spy)
    monkeypatch.setattr(sampling, "_run_fd_strided_inpaint_default", spy)          # (the spy is the device call: rows_hint as usual)
    own = structures.motif_backbone(motif, names)
    extent = float(np.sqrt(((own[:, None, :] - own[None, :, :]) ** 2).sum(-1)).max())
    bound = (12 * F + 1) * 1e-6 * extent                       # the motif's rows and tau of the row before them
    outs = {}
    for name, kw in (("few", dict(num_steps=5)), ("few_resampled", dict(num_steps=6, jump_length=2, n_resample=2)), ("eta", dict(num_steps=5, eta=1.0))):
        torch.manual_seed(3)
        samples, offs = sampling.scaffold(pm, ds, motif, [30, 31], **kw)
        assert offs == [9, 9] and [s.shape for s in samples] == [(30, F), (31, F)]
        for s, o in zip(samples, offs):
            assert np.array_equal(_bits(s[o: o + 12]), _bits(motif))
            assert np.isfinite(s).all() and not np.array_equal(s[:o], np.zeros_like(s[:o]))
        rmsd = structures.motif_rmsd(nerf.build_backbones(samples, names), own, offs)
        print(f"{name} scaffold: motif rmsd {rmsd} (bound {bound:.3e}, extent {extent:.2f} A)")
        _record(f"scaffold_1crn_{name}", max=float(rmsd.max()), bound=bound)
        assert (rmsd <= bound).all(), (name, rmsd, bound)
        outs[name] = samples
    assert calls == [(5, None), (6, 10), (5, None)]
    assert not np.array_equal(outs["few"][0][:8], outs["few_resampled"][0][:8]) and not np.array_equal(outs["few"][0][:8], outs["eta"][0][:8])
    torch.manual_seed(3)
    hist, _ = sampling.scaffold(pm, ds, motif, [30, 31], num_steps=5, final_only=False)
    assert [s.shape for s in hist] == [(5, 30, F), (5, 31, F)]
    assert all(np.array_equal(_bits(a[-1]), _bits(b)) for a, b in zip(hist, outs["few"]))
