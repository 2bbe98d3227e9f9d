"""The entry points that hang off a model handle at 3, 4, 5, 9 and 16 features with mixed wrap flags (layouts, inputs and
their conditions: tests/feature_set_cases.py; the conditions are asserted on the CPU by tests/test_feature_sets.py and here
again on the device's own prediction).  Parts A and C compare bits; the only tolerances are FWD_TOL of tests/test_gpu_parity.py
and the 2e-5 draw bound of its test_philox_stream, both imported."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_set_cases as fs
import resample_reference as jref
import strided_reference as sref
from foldingdiff_amd import _binding, beta_schedules, sampling
from oracle import ref_philox
from test_gpu_parity import FWD_TOL, _pair, _record, _share_time_table, _step
from test_solver_gpu import _step_solver
from test_steer_gpu import _step_x0
from test_strided_gpu import SENTINEL, _forward, _step_coef

pytestmark = pytest.mark.gpu
P = _binding.ptr
DRAW_TOL = 2e-5   # test_gpu_parity.test_philox_stream: the device's logf / sincosf against numpy's
bits = fs.bits


def _model(flags, precision, hidden, heads, layers=1):
    """(o32, o64, pm): test_gpu_parity._pair with the layout's flags; the weights are feature_set_cases.oracle's."""
    return _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=layers, maxpos=32, ft=tuple(flags), seed=fs.MODEL_SEED,
                 precision=precision)


def _call(pm, h, step, x, lens, wrap):
    """The hook of ``step`` -> (eps_out or None, {"x": x_out, "x0": x0_out where the hook writes one})."""
    if step.kind == "plain":       # fd_p_sample_step has no eps_out: the caller takes fd_forward's bits
        return None, {"x": _step(pm, h, x, step.t, lens, step.z, wrap)}
    if step.kind == "coef":
        rc, eps, out = _step_coef(h, x, step.t, lens, *step.coef, step.z, wrap)
        outs = {"x": out}
    elif step.kind == "solver":
        rc, eps, x0, out = _step_solver(h, x, step.t, lens, *step.coef, step.prev, wrap)
        outs = {"x": out, "x0": x0}
    else:
        rc, eps, x0, out = _step_x0(h, x, step.t, lens, *step.coef, step.z, wrap)
        outs = {"x": out, "x0": x0}
    assert rc == 0, (step.name, _binding.load().fd_last_error())
    return eps, outs


# ---------------------------------------------------------------------------------- A. one-step statements, bit for bit
@pytest.mark.parametrize("precision,hidden,heads", fs.VARIANTS)
@pytest.mark.parametrize("layout", list(fs.LAYOUTS))
def test_one_step_statements_bit_for_bit(gpu, layout, precision, hidden, heads):
    """Every update hook -- fd_p_sample_step, fd_p_sample_step_coef, fd_p_sample_step_solver, fd_p_sample_step_coef_x0 -- of
    every update kernel at every layout, wrap 0 and 1: x_out (and x0_out) carry the bits of the float32 statement applied to
    the hook's own eps_out (fd_p_sample_step, which has none: to fd_forward's); eps_out carries fd_forward's bits and is within
    FWD_TOL of the fp32 oracle.  With wrap = 1 every angular output lies in [-pi, pi] and every non-angular column keeps a
    value beyond pi; with wrap = 0 the statement without any wrap holds.  The wrap witnesses of feature_set_cases.check_step are
    asserted on the device's eps, so a wrap selected by the wrong bit, or left out, changes a compared element."""
    flags = fs.LAYOUTS[layout]
    F = len(flags)
    o32, o64, pm = _model(flags, precision, hidden, heads)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    _share_time_table(o64, o32, fs.T)
    h = pm.prepare(betas, list(flags))
    lens, ok = fs.LENS, fs.valid(fs.LENS, fs.L, F)
    fwd = {}
    worst = dev64 = ora64 = 0.0
    for step in fs.hook_steps(flags, betas):
        x = fs.state_of(step, flags)
        key = (step.t, step.wide)
        if key not in fwd:
            fwd[key] = _forward(h, x, step.t, lens)
            want32 = sref.forward(o32, x, step.t, lens).numpy()
            want64 = sref.forward(o64, x, step.t, lens).numpy()
            e = float(np.abs(fwd[key] - want32)[ok].max())
            e_dev, e_ora = float(np.abs(fwd[key] - want64)[ok].max()), float(np.abs(want32 - want64)[ok].max())
            worst, dev64, ora64 = max(worst, e), max(dev64, e_dev), max(ora64, e_ora)
            print(f"{layout} d{hidden} {precision} t={step.t} wide={step.wide}: |eps - oracle32| {e:.3e}  |eps - oracle64| {e_dev:.3e}  "
                  f"|oracle32 - oracle64| {e_ora:.3e}")
            # FWD_TOL, or -- both being fp32-class computations of the same sums -- at most twice the fp32 oracle's own
            # distance from the fp64 oracle (the factor covers the summation order)
            assert e <= FWD_TOL or e_dev <= 2 * e_ora, (step.name, e, e_dev, e_ora)
        for wrap in (0, 1):
            use = flags if wrap else (False,) * F
            eps, outs = _call(pm, h, step, x, lens, wrap)
            if eps is None:
                eps = fwd[key]
            else:
                assert np.array_equal(bits(eps)[ok], bits(fwd[key])[ok]), (step.name, wrap)
            want = fs.expected(step, x, eps, use)
            assert sorted(want) == sorted(outs)
            for name in want:
                assert np.array_equal(bits(outs[name])[ok], bits(want[name])[ok]), (step.name, wrap, name)
                for f, a in enumerate(flags):
                    col = outs[name][..., f][ok[..., f]]
                    if a and wrap:
                        assert (np.abs(col) <= fs.PI).all(), (step.name, name, f)
                    else:            # not angular, or nothing is: the column is not confined to a period
                        assert (np.abs(col) > fs.PI).any(), (step.name, wrap, name, f)
            if wrap:
                fs.check_step(step, x, eps, flags, ok)
    _record(f"featset_{layout}_d{hidden}_{precision}", max_eps=worst, max_eps_vs_fp64=dev64, oracle32_vs_fp64=ora64)


# ---------------------------------------------------------------------------------- B (last item). the draws at other F
def _draws(h, seed, t, off, B, L, F):
    out = torch.full((B, L, F), SENTINEL, device="cuda:0")
    torch.cuda.synchronize()                            # the fill runs on torch's stream, the generator on the handle's
    word = t - (1 << 32) if t >= (1 << 31) else t       # a tagged step word as the C int
    _binding.check(_binding.load().fd_philox_normal_dev(h, C.c_uint64(seed), word, C.c_int64(off), B, L, C.c_void_p(out.data_ptr()), None))
    _binding.check(_binding.load().fd_synchronize(h))
    torch.cuda.synchronize()
    return out.cpu().numpy()


PHILOX_CALLS = [(1234, 5, 0), ((7 << 40) + 99, 3, 1 << 33), (977, 0x80000000 | 4, 2), (977, 0x40000000 | 6, 0)]
_PHILOX = {}


def _philox_at(layout):
    """The draws of every call of PHILOX_CALLS from a handle of ``layout``, B = 5, L = 24; computed once per layout."""
    if layout not in _PHILOX:
        flags = fs.LAYOUTS[layout]
        _, _, pm = _model(flags, "f32", 96, 3)
        h = pm.prepare(beta_schedules.cosine_beta_schedule(fs.T), list(flags))
        _PHILOX[layout] = {call: _draws(h, *call, 5, 24, len(flags)) for call in PHILOX_CALLS}
    return _PHILOX[layout]


@pytest.mark.parametrize("layout", list(fs.LAYOUTS))
def test_philox_stream_of_a_feature_does_not_depend_on_the_feature_count(gpu, layout):
    """fd_philox_normal_dev of a handle with F features: within the draw bound of ref_philox.philox_normal(..., F) -- plain,
    64-bit seed and sequence index, the fixed elements' and the jumps' tagged words -- and column f carries the bits column f
    has at F = 16: a counter word, a Box-Muller pair or an output stride that used F would not.  At F = 16 the four blocks
    are four streams."""
    F = len(fs.LAYOUTS[layout])
    for call in PHILOX_CALLS:
        seed, t, off = call
        got, full = _philox_at(layout)[call], _philox_at("full16")[call]
        assert got.shape == (5, 24, F) and np.isfinite(got).all() and (got != SENTINEL).all()
        assert np.abs(got - ref_philox.philox_normal(seed, t, off, 5, 24, F)).max() < DRAW_TOL, call
        assert np.array_equal(bits(got), bits(full[..., :F])), call
        if layout == "full16":
            for g in range(1, 4):
                assert not np.array_equal(got[..., :4], got[..., 4 * g: 4 * g + 4]), (call, g)


# ---------------------------------------------------------------------------------- E. limits
def test_prepare_rejects_a_flag_list_of_the_wrong_length(gpu):
    flags = fs.LAYOUTS["canonical"]
    _, _, pm = _model(flags, "f32", 96, 3)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    for bad in (flags[:-1], flags + (True,), ()):
        with pytest.raises(AssertionError):
            pm.prepare(betas, list(bad))
    h = pm.prepare(betas, list(flags))      # ... and the handle is as usable as before
    x = fs.state(flags, 3, fs.L, 5)
    assert np.isfinite(_forward(h, x, 3, fs.LENS)[fs.valid(fs.LENS, fs.L, len(flags))]).all()


# ---------------------------------------------------------------------------------- C. loops are chains of hooks
LOOP_SEED = 977


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _run(h, family, betas, inp, full_history, noise=True, dev=False, seed=LOOP_SEED):
    """The run entry of ``family`` -> (rc, out [rows, B, L, F], started at the sentinel).  noise = False: both noise streams
    from Philox.  dev: the _dev entry (plain, strided, solver) on device copies."""
    lib = _binding.load()
    x0 = np.ascontiguousarray(inp.x_init, dtype=np.float32)
    B, L, F = x0.shape
    ls = np.ascontiguousarray(np.asarray(fs.LOOP_LENS, dtype=np.int32))
    K = fs.n_rows(family)
    rows = -(-K // full_history) if full_history else 1
    out = np.full((rows, B, L, F), SENTINEL, dtype=np.float32)
    zs = np.ascontiguousarray(inp.noise, dtype=np.float32) if noise and inp.noise is not None else None
    zk = np.ascontiguousarray(inp.known_noise, dtype=np.float32) if noise and inp.known_noise is not None else None
    vs = np.ascontiguousarray(fs.LOOP_VISITS)
    table = fs.loop_tables(family, betas)
    cf = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
    sd, off = C.c_uint64(seed), C.c_int64(0)
    if dev:
        x_d, l_d, z_d, out_d = _dev(x0), _dev(ls), _dev(zs), _dev(out)
        torch.cuda.synchronize()
        if family == "plain":
            rc = lib.fd_sample_dev(h, _dp(x_d), _dp(l_d), B, L, fs.LOOP_T - 1, _dp(z_d), sd, off, _dp(out_d), full_history, None)
        elif family == "strided":
            rc = lib.fd_sample_strided_dev(h, _dp(x_d), _dp(l_d), B, L, P(vs), K, P(cf), _dp(z_d), sd, off, _dp(out_d), full_history, None)
        else:
            assert family == "solver"
            rc = lib.fd_sample_solver_dev(h, _dp(x_d), _dp(l_d), B, L, P(vs), K, P(cf), _dp(out_d), full_history, None)
        _binding.check(lib.fd_synchronize(h))
        torch.cuda.synchronize()
        return rc, out_d.cpu().numpy()
    if family == "plain":
        rc = lib.fd_sample_ex(h, P(x0), P(ls), B, L, fs.LOOP_T - 1, P(zs), sd, off, P(out), full_history)
    elif family == "strided":
        rc = lib.fd_sample_strided(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(zs), sd, off, P(out), full_history)
    elif family == "solver":
        rc = lib.fd_sample_solver(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(out), full_history)
    elif family == "inpaint":
        rc = lib.fd_sample_inpaint(h, P(x0), P(ls), B, L, fs.LOOP_T - 1, P(zs), P(inp.known), P(inp.fixed), P(inp.kcoef), P(zk), sd, off,
                                   P(out), full_history)
    else:
        rc = lib.fd_sample_strided_inpaint(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(zs), P(inp.known), P(inp.fixed), P(inp.kcoef), P(zk),
                                           sd, off, P(out), full_history)
    return rc, out


def _visit_hook(pm, h, v, x, inp, wrap=1, lens=fs.LOOP_LENS):
    """The hook of a visit of a run -> (eps_out or None, x_out, x0_out or None)."""
    s = v.step
    if v.level is None:
        eps, outs = _call(pm, h, s, x, lens, wrap)
        return eps, outs["x"], outs.get("x0")
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    z = None if s.z is None else np.ascontiguousarray(s.z, dtype=np.float32)
    zk = None if v.zk is None else np.ascontiguousarray(v.zk, dtype=np.float32)
    out = np.full_like(xs, SENTINEL)
    if s.kind == "plain":
        rc = _binding.load().fd_p_sample_step_inpaint(h, P(xs), s.t, P(ls), B, L, P(z), wrap, P(inp.known), P(inp.fixed), P(inp.kcoef), P(zk),
                                                      P(out))
        eps = None
    else:
        eps = np.full_like(xs, SENTINEL)
        a, b, c = (float(k) for k in s.coef)
        rc = _binding.load().fd_p_sample_step_coef_inpaint(h, P(xs), s.t, P(ls), B, L, a, b, c, P(z), wrap, v.level, P(inp.known),
                                                           P(inp.fixed), P(inp.kcoef), P(zk), P(eps), P(out))
    assert rc == 0, (s.name, _binding.load().fd_last_error())
    return eps, out, None


def _loop_setup(family, precision, hidden, heads, layers):
    flags = fs.LAYOUTS["canonical"]
    _, _, pm = _model(flags, precision, hidden, heads, layers)
    betas = beta_schedules.cosine_beta_schedule(fs.LOOP_T)
    h = pm.prepare(betas, list(flags))
    inp = fs.loop_inputs(family, flags, betas, fs.LOOP_SEEDS[hidden, family])
    return flags, pm, betas, h, inp, fs.valid(fs.LOOP_LENS, fs.LOOP_L, len(flags))


@pytest.mark.parametrize("family", fs.FAMILIES)
@pytest.mark.parametrize("precision,hidden,heads,layers", fs.LOOP_VARIANTS)
def test_loop_rows_are_the_chain_of_hooks_at_the_canonical_layout(gpu, family, precision, hidden, heads, layers):
    """fd_sample, fd_sample_strided, fd_sample_solver, fd_sample_inpaint and fd_sample_strided_inpaint at F = 9 (three
    unwrapped columns, six angles), B = 4, L = 32, T = 10.  Row i of the full history carries the bits of the family's hook
    applied to row i - 1 (row -1: x_init, its fixed elements replaced at the start level by the float32 statement -- the
    start-point kernel) and of the float32 statement applied to the device's own prediction: the noise row stride, the history
    row stride, the state's ordinal, the known_noise row, all with F = 9.  With an explicit noise array, and with Philox, where the
    hook is fed the device generator's own draws (which are within the draw bound of ref_philox).  The wrap witnesses hold on
    the device's rows.  The final-only run, the thinned history, eager launches, packed rows and the device entry give the same
    bits; on the packed f16x3 path the history's padding is zero."""
    flags, pm, betas, h, inp, ok = _loop_setup(family, precision, hidden, heads, layers)
    F, (B, L) = len(flags), inp.x_init.shape[:2]
    K = fs.n_rows(family)
    lib = _binding.load()
    for explicit in ((True, False) if inp.noise is not None else (True,)):
        rc, full = _run(h, family, betas, inp, 1, noise=explicit)
        assert rc == 0, lib.fd_last_error()
        assert full.shape == (K, B, L, F) and np.isfinite(full[:, ok]).all()
        if explicit:
            state = fs.start_of(family, inp, flags)
        else:    # the start point's fixed elements: the tagged stream of the start level
            level0 = {"inpaint": fs.LOOP_T, "strided_inpaint": int(fs.LOOP_VISITS[0]) + 1}.get(family)
            state = inp.x_init if level0 is None else fs.ipr.replace(inp.x_init, inp.known, inp.fixed, level0, inp.kcoef,
                                                                       _draws(h, LOOP_SEED, 0x80000000 | level0, 0, B, L, F), flags)
        prev = None
        for i in range(K):
            z = zk = None
            if not explicit:
                v0 = fs.visit_of(family, i, betas, inp)
                if v0.step.z is not None:
                    z = _draws(h, LOOP_SEED, v0.step.t, 0, B, L, F)
                    assert np.abs(z - ref_philox.philox_normal(LOOP_SEED, v0.step.t, 0, B, L, F)).max() < DRAW_TOL
                if v0.level:
                    zk = _draws(h, LOOP_SEED, 0x80000000 | v0.level, 0, B, L, F)
                    assert np.abs(zk - fs.ipr.tagged_draw(LOOP_SEED, v0.level, 0, B, L, F)).max() < DRAW_TOL
            v = fs.visit_of(family, i, betas, inp, prev_x0=prev, z=z, zk=zk)
            eps, want, prev = _visit_hook(pm, h, v, state, inp)
            assert np.array_equal(bits(full[i])[ok], bits(want)[ok]), (family, explicit, i)
            if eps is None:
                eps = _forward(h, state, v.step.t, fs.LOOP_LENS)
            stated = fs.visit_expected(v, state, eps, flags, inp)
            assert np.array_equal(bits(full[i])[ok], bits(stated["x"])[ok]), (family, explicit, i)
            if prev is not None:
                assert np.array_equal(bits(prev)[ok], bits(stated["x0"])[ok]), (family, i)
            if explicit:
                fs.check_visit(v, state, eps, flags, ok, inp)
            state = full[i]
        # the other ways to the same run
        rc, final = _run(h, family, betas, inp, 0, noise=explicit)
        assert rc == 0 and np.array_equal(bits(final[0])[ok], bits(full[-1])[ok]), (family, "final")
        rc, every2 = _run(h, family, betas, inp, 2, noise=explicit)
        states = list(range(1, K, 2))
        assert rc == 0 and every2.shape[0] == len(states) and np.array_equal(bits(every2)[:, ok], bits(full[states])[:, ok]), (family, "every 2")
        pm.set_option("use_graph", 0)
        rc, eager = _run(h, family, betas, inp, 1, noise=explicit)
        pm.set_option("use_graph", 1)
        assert rc == 0 and np.array_equal(bits(eager)[:, ok], bits(full)[:, ok]), (family, "eager")
        pm.set_option("varlen", 1)
        rc, packed = _run(h, family, betas, inp, 1, noise=explicit)
        pm.set_option("varlen", 0)
        assert rc == 0 and np.array_equal(bits(packed)[:, ok], bits(full)[:, ok]), (family, "varlen")
        if precision == "f16x3":
            assert (packed[:, ~ok] == 0).all(), family
        if family in ("plain", "strided", "solver"):
            rc, dev = _run(h, family, betas, inp, 1, noise=explicit, dev=True)
            assert rc == 0 and np.array_equal(bits(dev)[:, ok], bits(full)[:, ok]), (family, "dev")
        if not explicit:     # the seed matters where something is drawn
            rc, other = _run(h, family, betas, inp, 1, noise=False, seed=LOOP_SEED + 1)
            assert rc == 0 and not np.array_equal(other[:, ok], full[:, ok])


def test_shift_trim_on_the_device_with_the_canonical_flags(gpu):
    """sampling._shift_trim on a device tensor (fd_shift_trim_dev: the handle's mask and feature count) with a length-9 offset:
    the bits of the numpy float32 statement -- s + offset rounded once, then the wrap in the six angular columns only."""
    flags = fs.LAYOUTS["canonical"]
    F = len(flags)
    _, _, pm = _model(flags, "f16x3", 192, 6)
    pm.prepare(beta_schedules.cosine_beta_schedule(fs.LOOP_T), list(flags))
    lens = fs.LOOP_LENS
    traj = np.stack([fs.state(flags, len(lens), fs.LOOP_L, 60 + r) for r in range(3)])
    offset = np.array([1.33, 1.46, 1.52, -1.3, 1.1, 3.0, 1.95, 2.03, 2.12], dtype=np.float32)
    ang = np.asarray(flags, dtype=bool)
    got = sampling._shift_trim(pm, torch.from_numpy(traj).to("cuda:0"), lens, offset, ang)
    host = sampling._shift_trim(pm, torch.from_numpy(traj), lens, offset, ang)
    for i, n in enumerate(lens):
        want = (traj[:, i, :n] + offset[None, None, :]).astype(np.float32)
        assert (np.abs(want[..., ang]) > np.pi).any(axis=(0, 1)).all() and (np.abs(want[..., ~ang]) > np.pi).any(axis=(0, 1)).all()
        want[..., ang] = fs.ipr.wrap32(want[..., ang])
        assert got[i].shape == (3, n, F)
        assert np.array_equal(bits(np.asarray(got[i])), bits(want)), i
        assert np.array_equal(bits(np.asarray(host[i])), bits(want)), i


# ---------------------------------------------------------------------------------- B. fixed elements, jumps and ties
def _sample_inpaint_rows(h, x0, lens, t_start, inp, known_noise, seed):
    """fd_sample_inpaint, full history, the update's draws from Philox -> (rc, out)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, F = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    zk = None if known_noise is None else np.ascontiguousarray(known_noise, dtype=np.float32)
    out = np.full((t_start + 1, B, L, F), SENTINEL, dtype=np.float32)
    rc = _binding.load().fd_sample_inpaint(h, P(x0), P(ls), B, L, t_start, None, P(inp.known), P(inp.fixed), P(inp.kcoef), P(zk),
                                           C.c_uint64(seed), C.c_int64(0), P(out), 1)
    return rc, out


@pytest.mark.parametrize("precision,hidden,heads", fs.FIXED_VARIANTS)
@pytest.mark.parametrize("layout", fs.FIXED_LAYOUTS)
def test_fixed_elements_jumps_and_ties_at_mixed_flags(gpu, layout, precision, hidden, heads):
    """B = 3, L = 24, T = 8 at the canonical layout and at sixteen features, on the row-image kernels and the one-wave-per-token
    kernels; every comparison is of bits, over all valid elements.
    * fd_p_sample_step_inpaint and fd_p_sample_step_coef_inpaint with explicit draws, wrap 0 and 1: the float32 statement
      (inpaint_reference.replace behind the update) applied to the device's prediction; level 0 leaves known's bits.
    * fd_inpaint_jump: resample_reference.jump fed the device generator's own draws of the two tagged words, which are within
      the draw bound of resample_reference.jump_draw and inpaint_reference.tagged_draw; padding keeps its bits.
    * the start-point replacement, through fd_sample_inpaint with t_start = 0 and 1: row 0 is the conditioned hook applied
      to inpaint_reference.replace(x_init) at level t_start + 1, with an explicit known_noise and with Philox (the device's
      own tagged draws); the last row's fixed elements are known's bits, where nothing is drawn.
    * fd_sample_repeat, one visit with coefficients by value: the init tie, the strided update and the tie of
      repeat_reference.tie under the model's flags, with the seam of an angular column between the copies and a non-angular
      column beyond pi, whose tied mean is the plain mean (feature_set_cases.check_tie, on the device's own values)."""
    flags = fs.LAYOUTS[layout]
    F, B, L, lens = len(flags), len(fs.LENS), fs.L, fs.LENS
    o32, _, pm = _model(flags, precision, hidden, heads)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    h = pm.prepare(betas, list(flags))
    lib = _binding.load()
    inp = fs.fixed_inputs(flags, fs.FIXED_SEEDS[layout, hidden])
    assert np.array_equal(bits(inp.kcoef), bits(sampling.inpaint_levels(betas)))
    ok = fs.valid(lens, L, F)
    fx = inp.fixed.astype(bool)
    x = inp.x_init
    for v in fs.fixed_visits(flags, betas):
        fwd = _forward(h, x, v.step.t, lens)
        for wrap in (0, 1):
            use = flags if wrap else (False,) * F
            eps, got, _ = _visit_hook(pm, h, v, x, inp, wrap, lens=lens)
            if eps is not None:
                assert np.array_equal(bits(eps)[ok], bits(fwd)[ok]), (v.step.name, wrap)
            want = fs.visit_expected(v, x, fwd, use, inp)["x"]
            assert np.array_equal(bits(got)[ok], bits(want)[ok]), (v.step.name, v.level, wrap)
            if v.level == 0:
                assert np.array_equal(bits(got)[fx], bits(inp.known)[fx])
            if wrap:
                fs.check_visit(v, x, fwd, flags, ok, inp)
                assert (np.abs(got[..., np.asarray(flags)][(ok & ~fx)[..., np.asarray(flags)]]) <= fs.PI).all()
    # jumps
    xj = fs.jump_state(flags)
    xs, ls = np.ascontiguousarray(xj), np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    for a, b in fs.JUMPS:
        jk, js = sampling.resample_jump_coef(betas, [a, b - 1])[0]
        got = np.full_like(xs, SENTINEL)
        rc = lib.fd_inpaint_jump(h, P(xs), P(ls), B, L, b, C.c_float(jk), C.c_float(js), P(inp.known), P(inp.fixed), P(inp.kcoef),
                                 C.c_uint64(fs.JUMP_SEED), C.c_int64(fs.JUMP_OFFSET), P(got))
        assert rc == 0, lib.fd_last_error()
        zf, zk = (_draws(h, fs.JUMP_SEED, w | b, fs.JUMP_OFFSET, B, L, F) for w in (jref.JUMP_TAG, fs.ipr.TAG))
        assert np.abs(zf - jref.jump_draw(fs.JUMP_SEED, b, fs.JUMP_OFFSET, B, L, F)).max() < DRAW_TOL
        assert np.abs(zk - fs.ipr.tagged_draw(fs.JUMP_SEED, b, fs.JUMP_OFFSET, B, L, F)).max() < DRAW_TOL
        want = jref.jump(xj, inp.known, inp.fixed, b, jk, js, inp.kcoef, zf, zk, flags, lens)
        assert np.array_equal(bits(got)[ok], bits(want)[ok]), (a, b)
        assert np.array_equal(bits(got)[~ok], bits(xj)[~ok]), (a, b)
        assert fs.wrap_witnesses(fs.jump_stages(xj, jk, js, zf, flags), flags, ok & ~fx) == [], (a, b)
        assert fs.wrap_witnesses(fs.replacement_stages(inp.known, b, inp.kcoef, zk, flags), flags, ok & fx) == [], (a, b)
    # the start-point replacement
    table = beta_schedules.step_coefficients(betas).numpy()
    seed = 4242
    for t_start in (0, 1):
        level0 = t_start + 1
        explicit = np.stack([fs.draws(B, L, F, 400 + j) for j in range(t_start + 2)])
        for known_noise in (explicit, None):
            rc, rows = _sample_inpaint_rows(h, x, lens, t_start, inp, known_noise, seed)
            assert rc == 0, lib.fd_last_error()
            zk0 = known_noise[level0] if known_noise is not None else _draws(h, seed, 0x80000000 | level0, 0, B, L, F)
            state = fs.ipr.replace(x, inp.known, inp.fixed, level0, inp.kcoef, zk0, flags)
            assert fs.wrap_witnesses(fs.replacement_stages(inp.known, level0, inp.kcoef, zk0, flags), flags, ok & fx) == []
            for j, t in enumerate(range(t_start, -1, -1)):
                z = None if t == 0 else _draws(h, seed, t, 0, B, L, F)
                zk = None if t == 0 else (known_noise[t] if known_noise is not None else _draws(h, seed, 0x80000000 | t, 0, B, L, F))
                v = fs.Visit(fs.Step("plain", t, tuple(table[:, t]), z=z), t, zk)
                _, want, _ = _visit_hook(pm, h, v, state, inp, lens=lens)
                assert np.array_equal(bits(rows[j])[ok], bits(want)[ok]), (t_start, known_noise is None, t)
                state = rows[j]
            assert np.array_equal(bits(rows[-1])[fx], bits(inp.known)[fx])
    # the tie of a repeat run under the model's flags
    x_tie = fs.tie_inputs(flags, fs.TIE_SEEDS[layout, hidden], o32)
    z = fs.draws(B, L, F, 301, scale=1.0)
    a, b, s = fs.TIE_COEF
    cf = np.array([[a], [b], [s]], dtype=np.float32)
    vs, ts = np.array([fs.TIE_T], dtype=np.int32), np.ascontiguousarray(np.asarray(fs.TIES, dtype=np.int32))
    got = np.full_like(x_tie, SENTINEL)
    rc = lib.fd_sample_repeat(h, P(x_tie), P(ls), B, L, P(vs), 1, P(cf), P(np.ascontiguousarray(z[None])), C.c_uint64(0), C.c_int64(0), P(ts),
                              P(got))
    assert rc == 0, lib.fd_last_error()
    mid, want = fs.tie_expected(x_tie, lambda st: _forward(h, st, fs.TIE_T, lens), flags, z)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    fs.check_tie(mid, want, flags, z)


# ---------------------------------------------------------------------------------- D. per-sequence timesteps, the loss, the AR pair
def _mask_of(lens, L):
    m = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        m[i, :n] = 1.0
    return m


@pytest.mark.parametrize("precision,hidden,heads", fs.FIXED_VARIANTS)
@pytest.mark.parametrize("layout", ["canonical", "minimal"])
def test_forward_with_one_timestep_per_sequence(gpu, layout, precision, hidden, heads):
    """fd_forward_t (forward_mixed_t) at F = 9 and F = 4: with every sequence at the same t the bits of fd_forward, row by row;
    with distinct t within FWD_TOL of the fp32 oracle."""
    flags = fs.LAYOUTS[layout]
    o32, _, pm = _model(flags, precision, hidden, heads)
    h = pm.prepare(beta_schedules.cosine_beta_schedule(fs.T), list(flags))
    lens, ok = fs.LENS, fs.valid(fs.LENS, fs.L, len(flags))
    x, mask = torch.from_numpy(fs.state(flags, len(lens), fs.L, 5)), _mask_of(lens, fs.L)
    for tv in (0, 4, 7):
        t = torch.full((len(lens),), tv, dtype=torch.long)
        got = pm.forward_mixed_t(x, t, mask).numpy()
        assert np.array_equal(bits(got)[ok], bits(_forward(h, x.numpy(), tv, lens))[ok]), tv
        assert np.array_equal(bits(got)[ok], bits(pm(x, t, attention_mask=mask).numpy())[ok]), tv
    t = torch.tensor([7, 0, 4])
    got = pm.forward_mixed_t(x, t, mask).numpy()
    e = float(np.abs(got - o32(x, t, attention_mask=mask).detach().numpy())[ok].max())
    _record(f"featset_fwd_t_{layout}_d{hidden}_{precision}", max=e)
    assert e <= FWD_TOL, e
    for b, tv in enumerate(t.tolist()):     # ... and each sequence has the bits it has when the whole batch sits at its timestep
        same = pm.forward_mixed_t(x, torch.full((len(lens),), tv, dtype=torch.long), mask).numpy()
        assert np.array_equal(bits(got[b])[ok[b]], bits(same[b])[ok[b]]), b


def test_denoise_loss_noises_and_wraps_by_the_models_flags(gpu):
    """fd_denoise_loss at the canonical layout on the row-image path: the noised input it builds is keep x0 + spread noise,
    each product and the sum rounded once, wrapped in the six angular columns only (the bits of the float32 statement; both
    kinds of column pass pi); the forward inside is forward_mixed_t's; the sums are losses.loss_terms' of that prediction,
    and the terms are the host statement's within test_loss_gpu's TERM_TOL."""
    from foldingdiff_amd import losses
    from test_loss_gpu import TERM_TOL
    flags = fs.LAYOUTS["canonical"]
    F = len(flags)
    ang = np.asarray(flags, dtype=bool)
    _, _, pm = _model(flags, "f16x3", 192, 6)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    pm.prepare(betas, list(flags))
    lens = fs.LENS
    mask = _mask_of(lens, fs.L)
    x0 = fs.known_values(flags, len(lens), fs.L, 55)
    noise = fs.draws(len(lens), fs.L, F, 56, scale=1.0)
    t = torch.tensor([6, 1, 3])
    levels = fs.ipr.levels(betas)
    keep, spread = levels[0, t.numpy() + 1], levels[1, t.numpy() + 1]
    sums, extra = pm.denoise_loss_sums(torch.from_numpy(x0), torch.from_numpy(noise), t, mask, keep=torch.from_numpy(keep),
                                       spread=torch.from_numpy(spread), return_corrupted=True, return_eps=True)
    raw = ((keep[:, None, None] * x0).astype(np.float32) + (spread[:, None, None] * noise).astype(np.float32)).astype(np.float32)
    assert (np.abs(raw) > np.pi + fs.MARGIN).any(axis=(0, 1)).all()           # every column passes pi before the wrap
    want = raw.copy()
    want[..., ang] = fs.ipr.wrap32(raw[..., ang])
    assert np.array_equal(bits(extra["corrupted"]), bits(want))               # every position of the pad, masked ones included
    eps = pm.forward_mixed_t(torch.from_numpy(want), t, mask).numpy()
    assert np.array_equal(bits(eps), bits(extra["eps"]))
    want_sums, terms = losses.loss_terms(eps, noise, mask, list(flags))
    assert np.array_equal(sums, want_sums)
    host = losses.host_terms(torch.from_numpy(eps), torch.from_numpy(noise), list(flags)).numpy() * mask.numpy()[:, :, None]
    err = float(np.abs(terms.astype(np.float64) - host).max())
    _record("featset_loss_terms_canonical", max=err)
    assert err <= TERM_TOL
    other = losses.host_terms(torch.from_numpy(eps), torch.from_numpy(noise), list(fs.rotated(flags))).numpy() * mask.numpy()[:, :, None]
    assert np.abs(other - host)[..., [0, 3]].max() > 100 * TERM_TOL            # the two columns whose flag a rotation changes would show


@pytest.mark.parametrize("layout,seed", [("minimal", 104), ("canonical", 109)])
def test_autoregressive_pair_at_other_feature_counts(gpu, layout, seed):
    """fd_ar_forward and a six-step fd_ar_sample (embed_img_ar_kernel, ar_step_kernel) at F = 4 and F = 9, against
    tests/ar_reference.py at tests/test_autoregressive_gpu.py's tolerance: the forward, and row i of step i given the
    device's own prefix.  (A model seed of its own per layout: that module caches its models by a key without the flags.)"""
    import ar_reference
    import test_autoregressive_gpu as ar
    flags = fs.LAYOUTS[layout]
    F = len(flags)
    o32, _, pm = ar._pair(192, 6, seed=seed, ft=tuple(flags))
    assert pm.n_inputs == F
    L, key_lens, seq_lengths = 33, [33, 1, 32, 8, 9], [33, 0, 128, 17, 64]
    x, mask, n = ar._uniform(len(key_lens), L, seed=seed, F=F), ar_reference.prefix_mask(key_lens, L), torch.tensor(seq_lengths)
    err = float(np.abs(pm(x, mask, n).numpy() - ar_reference.ar_forward(o32, x, mask, n).numpy().astype(np.float64)).max())
    _record(f"featset_ar_fwd_{layout}", max=err)
    assert err <= ar.FWD_TOL, err
    Lr, lens, ns = 16, [8, 5, 8, 3], 2           # steps 2 .. 7: six; they cross the 8-row packing
    start = ar._uniform(len(lens), Lr, seed=seed + 1, F=F)
    dev = ar._device_rollout(pm, start, lens, ns)
    assert tuple(dev.shape) == (len(lens), Lr, F) and torch.isfinite(dev).all()
    gap, at = ar._teacher_forced_gap(o32, dev, start, lens, ns)
    _record(f"featset_ar_step_{layout}", max=gap, step=at)
    assert torch.equal(dev[:, :ns], start[:, :ns]) and torch.equal(dev[:, max(lens):], start[:, max(lens):])
    assert not torch.equal(dev[:, ns:max(lens)], start[:, ns:max(lens)])
    assert gap <= ar.FWD_TOL, (gap, at)
