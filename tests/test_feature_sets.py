"""The inputs of tests/test_feature_sets_gpu.py meet the conditions under which its comparisons can fail (CPU; the fp32
oracle's prediction and the restatements alone): every non-angular column of every expected result holds a value beyond
pi, every angular column's value before its wrap lies outside [-pi, pi) somewhere, a flag list moved on by one position
gives other bits in every column whose flag changed, every column has fixed and free elements, and the restatements are
self-consistent at these feature counts.  Plus the limits of fd_create, which need no device."""
import ctypes as C

import numpy as np
import pytest

import feature_set_cases as fs
import inpaint_reference as ipr
import resample_reference as jref
import solver_reference as vref
import strided_inpaint_reference as sipr
import strided_reference as sref
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling

CASES = [(name, p, d, h) for name in fs.LAYOUTS for p, d, h in fs.VARIANTS]


def test_layouts_cover_the_shipped_feature_sets():
    shipped = {tuple(bool(a) for a in v) for v in datasets.FEATURE_SET_NAMES_TO_ANGULARITY.values()}
    assert {fs.LAYOUTS["cart"], fs.LAYOUTS["minimal"], fs.LAYOUTS["canonical"]} <= shipped
    assert sorted(len(v) for v in fs.LAYOUTS.values()) == [3, 4, 5, 9, 16]
    for flags in fs.LAYOUTS.values():   # a rotation changes at least one flag of every mixed layout
        assert (fs.rotated(flags) != flags) == (len(set(flags)) > 1)


# ---------------------------------------------------------------------------------------------------- the fused add
def test_fma32_rounds_once():
    """feature_set_cases.fma32 against exact rational arithmetic rounded to the nearest float32 (ties to even), on products
    and addends of mixed magnitudes and on constructed half-way cases, where rounding the float64 sum again would go wrong."""
    from fractions import Fraction

    def nearest(fr):
        f = np.float32(float(fr))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        return min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))

    rng = np.random.default_rng(0)
    n = 1500
    a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    c = (rng.normal(size=n) * rng.choice([1e-6, 1.0, 1e4], n)).astype(np.float32)
    # half-way cases: c = 1, a b = 2^-24 +- 2^-60 (one ulp of 1 is 2^-23): the float64 sum is exactly 1 + 2^-24
    a = np.concatenate([a, np.float32([2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 2.0 ** -12])])
    b = np.concatenate([b, np.float32([2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 2.0 ** -12])])
    c = np.concatenate([c, np.float32([1.0, 1.0, 1.0])])
    got = fs.fma32(a, b, c)
    want = np.array([nearest(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(fs.bits(got), fs.bits(want))
    assert got[-3] == np.float32(1 + 2.0 ** -23) and got[-2] == np.float32(1.0) and got[-1] == np.float32(1.0)
    twice = (c + (a * b).astype(np.float32)).astype(np.float32)
    assert 0.05 < (twice != got).mean() < 0.5       # rounding twice is another function


# ---------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("layout,precision,hidden,heads", CASES)
def test_one_step_inputs_meet_the_conditions(layout, precision, hidden, heads):
    """Conditions 1, 2 and 4 for every hook call of part A, on the oracle's eps.  (The precision does not enter on the CPU:
    the two f16x3 and the two f32 variants are four different models.)"""
    flags = fs.LAYOUTS[layout]
    F = len(flags)
    o32 = fs.oracle(flags, hidden, heads)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    ok = fs.valid(fs.LENS, fs.L, F)
    eps = {}
    steps = fs.hook_steps(flags, betas)
    assert {s.kind for s in steps} == {"plain", "coef", "solver", "x0"} and len(steps) == 18
    for step in steps:
        x = fs.state_of(step, flags)
        if (step.t, step.wide) not in eps:
            eps[step.t, step.wide] = sref.forward(o32, x, step.t, fs.LENS).numpy()
        fs.check_step(step, x, eps[step.t, step.wide], flags, ok)
    # a statement that wraps nothing passes through check_step's witnesses only for a layout without angles
    x = fs.state_of(steps[0], flags)
    plain = fs.stages(steps[0], x, eps[5, False], [False] * F)
    assert (fs.wrap_witnesses(plain, [False] * F, ok) == [])
    if any(flags):   # ... and the witnesses notice a state that never leaves [-pi, pi): nothing here is vacuous
        tame = fs.stages(steps[1], np.clip(x, -1.0, 1.0), np.zeros_like(x), flags)
        assert fs.wrap_witnesses(tame, flags, ok) != []


# ---------------------------------------------------------------------------------------------------- part E
@pytest.mark.parametrize("n_features", [0, 17])
def test_create_rejects_feature_counts_outside_1_to_16(lib, n_features):
    cfg = _binding.FdConfig(n_features=n_features, d_model=64, n_heads=2, d_ff=128, n_layers=1, max_pos=32, pos_type=0, decoder=0,
                            ln_eps=1e-12)
    h = C.c_void_p(0x5A5A)
    rc = lib.fd_create(C.byref(cfg), 0, C.byref(h))
    assert rc == -1 and b"n_features" in lib.fd_last_error(), (rc, lib.fd_last_error())   # -1 = FD_E_INVALID (include/fdmi.h)
    assert not h.value                      # no handle is left behind


# ---------------------------------------------------------------------------------------------------- part C
def _module_loop(family, o32, flags, betas, inp):
    """The run by the restatement modules' own loops."""
    lens = fs.LOOP_LENS
    if family == "strided":
        return sref.loop(o32, lens, inp.x_init, fs.LOOP_VISITS, fs.loop_tables(family, betas), flags, inp.noise)
    if family == "solver":
        return vref.loop(o32, lens, inp.x_init, fs.LOOP_VISITS, fs.loop_tables(family, betas), flags)
    if family == "inpaint":
        return ipr.loop(o32, lens, inp.x_init, fs.LOOP_T - 1, betas, flags, inp.known, inp.fixed, inp.kcoef, inp.noise, inp.known_noise)
    if family == "strided_inpaint":
        return sipr.loop(o32, lens, inp.x_init, fs.LOOP_VISITS, fs.loop_tables(family, betas), flags, inp.known, inp.fixed, inp.kcoef,
                         inp.noise, inp.known_noise)
    nothing = np.zeros(inp.x_init.shape, dtype=np.uint8)    # the plain sampler: the conditioned loop with nothing fixed
    return ipr.loop(o32, lens, inp.x_init, fs.LOOP_T - 1, betas, flags, inp.x_init, nothing, ipr.levels(betas), inp.noise,
                    np.zeros((fs.LOOP_T + 1,) + inp.x_init.shape, dtype=np.float32))


@pytest.mark.parametrize("family", fs.FAMILIES)
@pytest.mark.parametrize("precision,hidden,heads,layers", fs.LOOP_VARIANTS)
def test_loop_inputs_meet_the_conditions(family, precision, hidden, heads, layers, monkeypatch):
    """Conditions 1, 2 and 3 for every visit of every run family of part C, and condition 4: row i is the update applied to
    row i - 1 (reference_loop is built that way) and equals the restatement modules' own loop; angular columns lie in
    [-pi, pi], the others are the unwrapped arithmetic (check_step)."""
    flags = fs.LAYOUTS["canonical"]
    F = len(flags)
    o32 = fs.oracle(flags, hidden, heads, layers=layers)
    betas = beta_schedules.cosine_beta_schedule(fs.LOOP_T)
    inp = fs.loop_inputs(family, flags, betas, fs.LOOP_SEEDS[hidden, family])
    ok = fs.valid(fs.LOOP_LENS, fs.LOOP_L, F)
    if inp.fixed is not None:
        fs.check_fixed(inp.fixed, fs.LOOP_LENS)
        assert not inp.fixed.astype(bool)[~ok].any()
    rows, trace = fs.reference_loop(family, o32, flags, betas, inp)
    assert rows.shape == (fs.n_rows(family), len(fs.LOOP_LENS), fs.LOOP_L, F)
    for v, x, eps in trace:
        fs.check_visit(v, x, eps, flags, ok, inp)
    want = _module_loop(family, o32, flags, betas, inp)
    if family in ("plain", "inpaint"):
        # ipr.step runs ref_sampling.p_sample in torch, which rounds the noise product and the sum separately: the same bits
        # as plain_update with its noise add not fused; the kernels' fused add moves last bits, which the run then carries
        assert not np.array_equal(fs.bits(rows)[:, ok], fs.bits(want)[:, ok])
        monkeypatch.setattr(fs, "FUSED_NOISE_ADD", False)
        rows = fs.reference_loop(family, o32, flags, betas, inp)[0]
    assert np.array_equal(fs.bits(rows)[:, ok], fs.bits(want)[:, ok])
    ang = np.asarray(flags, dtype=bool)
    free = ok if inp.fixed is None else ok & ~inp.fixed.astype(bool)    # (a fixed element at level 0 is known's bits, which need not be wrapped)
    assert (np.abs(rows[..., ang][:, free[..., ang]]) <= fs.PI).all()


# ---------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("precision,hidden,heads", fs.FIXED_VARIANTS)
@pytest.mark.parametrize("layout", fs.FIXED_LAYOUTS)
def test_fixed_element_inputs_meet_the_conditions(layout, precision, hidden, heads):
    """Conditions 1-3 for the conditioned hooks, the jumps and the tied visit of part B."""
    flags = fs.LAYOUTS[layout]
    F, B = len(flags), len(fs.LENS)
    o32 = fs.oracle(flags, hidden, heads)
    betas = beta_schedules.cosine_beta_schedule(fs.T)
    inp = fs.fixed_inputs(flags, fs.FIXED_SEEDS[layout, hidden])
    ok = fs.valid(fs.LENS, fs.L, F)
    fx = inp.fixed.astype(bool)
    fs.check_fixed(inp.fixed, fs.LENS)
    assert not fx[~ok].any()
    for v in fs.fixed_visits(flags, betas):
        eps = sref.forward(o32, inp.x_init, v.step.t, fs.LENS).numpy()
        fs.check_visit(v, inp.x_init, eps, flags, ok, inp)
        out = fs.visit_expected(v, inp.x_init, eps, flags, inp)["x"]
        if v.level == 0:
            assert np.array_equal(fs.bits(out)[fx], fs.bits(inp.known)[fx])
    xj = fs.jump_state(flags)
    for a, b in fs.JUMPS:      # the jump's draws are Philox's own: ref_philox restates them on the CPU
        jk, js = sampling.resample_jump_coef(betas, [a, b - 1])[0]
        zf = jref.jump_draw(fs.JUMP_SEED, b, fs.JUMP_OFFSET, B, fs.L, F)
        zk = ipr.tagged_draw(fs.JUMP_SEED, b, fs.JUMP_OFFSET, B, fs.L, F)
        assert fs.wrap_witnesses(fs.jump_stages(xj, jk, js, zf, flags), flags, ok & ~fx) == [], (a, b)
        assert fs.wrap_witnesses(fs.replacement_stages(inp.known, b, inp.kcoef, zk, flags), flags, ok & fx) == [], (a, b)
        want = jref.jump(xj, inp.known, inp.fixed, b, jk, js, inp.kcoef, zf, zk, flags, fs.LENS)
        other = jref.jump(xj, inp.known, inp.fixed, b, jk, js, inp.kcoef, zf, zk, fs.rotated(flags), fs.LENS)
        for f in range(F):
            if fs.rotated(flags)[f] != flags[f]:
                for sel in (ok & fx, ok & ~fx):
                    assert not np.array_equal(fs.bits(want[..., f][sel[..., f]]), fs.bits(other[..., f][sel[..., f]])), (a, b, f)
    x_tie = fs.tie_inputs(flags, fs.TIE_SEEDS[layout, hidden], o32)
    z = fs.draws(B, fs.L, F, 301, scale=1.0)
    mid, out = fs.tie_expected(x_tie, lambda x: sref.forward(o32, x, fs.TIE_T, fs.LENS).numpy(), flags, z)
    fs.check_tie(mid, out, flags, z)
