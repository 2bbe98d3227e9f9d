"""
Feature layouts other than six all-angular features, for the entry points that hang off a model handle (TEST INFRASTRUCTURE
ONLY): the layouts, the model variants, the fixed-seed inputs and the list of one-step hook calls that
tests/test_feature_sets_gpu.py makes, with the float32 statements they are compared with and the conditions the inputs must
meet for those comparisons to mean something.  tests/test_feature_sets.py asserts the conditions on the CPU with the fp32
oracle's prediction; the GPU file asserts them again on the device's own prediction.

The restatements are those of tests/strided_reference.py, solver_reference.py and inpaint_reference.py, which read F from
the array shape; the plain sampler's update, which no restatement module writes out against a given eps, is ``plain_update``
(with the kernels' fused noise add).
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

import inpaint_reference as ipr
import solver_reference as vref
import strided_reference as sref
from foldingdiff_amd import beta_schedules, sampling
from oracle import ref_model

PI = np.float32(np.pi)
MARGIN = 1e-3   # how far past the seam a witness must lie: 100 x the forward tolerance, so the device's eps has the same witnesses

# name -> wrap flags.  What each reaches is tabulated in DESIGN.md.
LAYOUTS = {
    "cart": (False,) * 3,                               # mask 0; 13 idle lanes of a 16-lane token group; no wrap anywhere
    "minimal": (True,) * 4,                             # exactly one Philox block
    "odd5": (True, False, True, False, True),           # F ends in the middle of a Box-Muller pair of block 1; interleaved bits
    "canonical": (False,) * 3 + (True,) * 6,            # the shipped mixed set; Philox block 2; lane 8
    "full16": (False, True) * 8,                        # kMaxFeat; lane 15 and mask bit 15; Philox block 3
}
# (precision, d_model, heads): the row-image kernels (f16x3, two widths), the 16-lanes-per-token kernels (f32, d % 64 == 0)
# and the one-wave-per-token kernels (f32, d = 96)
VARIANTS = [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)]
MODEL_SEED = 3
T, L, LENS = 8, 24, [24, 17, 9]                         # parts A and B
VISITS = np.array([7, 4, 2, 0], dtype=np.int32)
LOOP_T, LOOP_L, LOOP_LENS = 10, 32, [32, 25, 17, 9]     # part C
LOOP_VARIANTS = [("f16x3", 192, 6, 2), ("f32", 128, 4, 1)]   # (precision, d_model, heads, layers)


def rotated(flags) -> tuple:
    """The flag list moved on by one position: flag f becomes flag f - 1's."""
    return tuple(flags[-1:]) + tuple(flags[:-1])


def oracle(flags, hidden, heads, layers=1, maxpos=32, seed=MODEL_SEED, dtype=torch.float32):
    """The oracle model a variant's device model takes its weights from (test_gpu_parity._pair with the same arguments)."""
    cfg = ref_model.OracleConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden, layer_norm_eps=1e-12,
                                 num_hidden_layers=layers, max_position_embeddings=maxpos, position_embedding_type="relative_key")
    return ref_model.synthetic_model(cfg, tuple(flags), "gaussian_fourier", "mlp", seed=seed).to(dtype)


def valid(lens, L, F) -> np.ndarray:
    v = np.zeros((len(lens), L, F), dtype=bool)
    for b, n in enumerate(lens):
        v[b, :n] = True
    return v


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def state(flags, B, L, seed, widen=1.0) -> np.ndarray:
    """A state no column of which sits inside [-pi, pi): non-angular columns N(0, 3^2) (bond lengths and coordinates are not
    confined to a period), angular columns N(0, 2.2^2), NOT wrapped.  A hook takes any finite state, and with a state past the
    seam the pre-wrap value of every step crosses it whatever the step's coefficients are -- at t = 0, where the state is
    scaled by 1.0002 and nothing is drawn, a wrapped state would cross nowhere."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([2.2 if a else 3.0 for a in flags]) * widen
    return (torch.randn(B, L, len(flags), generator=g) * scale).numpy().astype(np.float32)


def draws(B, L, F, seed, scale=2.0) -> np.ndarray:
    """An explicit noise array.  Twice the unit scale: the arbitrary triple (1e-3, 2^-20, -1.5) keeps nothing but -1.5 z, which
    has to pass pi in every column."""
    return (torch.randn(B, L, F, generator=torch.Generator().manual_seed(seed)) * scale).numpy().astype(np.float32)


def previous_x0(flags, B, L, seed) -> np.ndarray:
    """A previous prediction as a solver visit leaves it: angular columns in [-pi, pi), the others N(0, 3^2)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, 3.0, (B, L, len(flags))).astype(np.float32)
    u = rng.uniform(-np.pi, np.pi, (B, L, len(flags))).astype(np.float32)
    u[u >= PI] = -PI
    return np.where(np.asarray(flags, dtype=bool), u, p).astype(np.float32)


def _wrap_cols(v, is_angle) -> np.ndarray:
    return vref._wrap_cols(v, np.nonzero(np.asarray(is_angle, dtype=bool))[0])


FUSED_NOISE_ADD = True   # what the update kernels compute (below); tests/test_feature_sets.py also runs the reference's two roundings


def fma32(a, b, c) -> np.ndarray:
    """float32(a * b + c) with ONE rounding, exactly.  The product of two float32 is exact in float64; the float64 sum s and
    its error e come from Knuth's two-sum.  Rounding s to float32 is then right unless s sits exactly half way between two
    float32 neighbours while e != 0 (rounding to float64 is monotone and the half-way points are float64 numbers, so it can
    land on one but not cross it): there the sign of e decides."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float32).astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        lo = np.where(r64 <= s, r, np.nextafter(r, np.float32(-np.inf))).astype(np.float32)
        hi = np.where(r64 >= s, r, np.nextafter(r, np.float32(np.inf))).astype(np.float32)
        tie = (lo != hi) & ((s - lo.astype(np.float64)) == (hi.astype(np.float64) - s)) & (e != 0) & np.isfinite(s)
    return np.where(tie, np.where(e > 0, hi, lo), r).astype(np.float32)


def plain_update(x, eps, c1, bt, c3, sg, z, is_angle, fused=None) -> np.ndarray:
    """fd_p_sample_step's statement on float32 arrays, with the four scalars of ``beta_schedules.step_coefficients`` at t:
    x' = c1 (x - bt eps / c3), every operation rounded once; where z is given (t > 0) x' = fma(sg, z, x'), the product and
    the sum rounded ONCE; angular features wrapped.  The reference rounds sg z and the sum separately (``fused`` False: the
    bits of ``ref_sampling.p_sample``); the kernels' __fadd_rn(xn, __fmul_rn(sg, z)) is contracted into one FMA once inlined
    (DESIGN.md 6k says the same of the noising statement), the last bit of about one element in six differs, and that
    is what every sampler run of this project has computed -- so it is what is pinned here."""
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    c1, bt, c3, sg = (np.float32(k) for k in (c1, bt, c3, sg))
    v = (c1 * (x - (bt * eps).astype(np.float32) / c3).astype(np.float32)).astype(np.float32)
    if z is not None:
        if FUSED_NOISE_ADD if fused is None else fused:
            v = fma32(sg, z, v)
        else:
            v = (v + (sg * np.asarray(z, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    return _wrap_cols(v, is_angle)


@dataclass
class Step:
    """One hook call: kind plain | coef | solver | x0, the timestep, the coefficients by value, the draws and the previous
    prediction (None where the statement reads none)."""
    kind: str
    t: int
    coef: Tuple[float, ...]
    z: Optional[np.ndarray] = None
    prev: Optional[np.ndarray] = None
    wide: bool = False   # the call starts from the four times wider state (``state_of``)

    @property
    def name(self):
        return f"{self.kind}@t{self.t}{tuple(float(c) for c in self.coef)}"


ARBITRARY = [(1.7, -0.9, 0.3), (-0.25, 3.5, 0.0), (1e-3, 2.0 ** -20, -1.5)]   # test_strided_gpu's three triples


def hook_steps(flags, betas) -> list:
    """Part A's hook calls at T = 8, each from ``state_of(step, flags)``."""
    F = len(flags)
    B = len(LENS)
    table = beta_schedules.step_coefficients(betas).numpy()
    steps = [Step("plain", 5, tuple(table[:, 5]), z=draws(B, L, F, 101)), Step("plain", 0, tuple(table[:, 0]))]
    for eta in (0.0, 0.5):
        coef = sampling.ddim_coefficients(betas, VISITS, eta)
        assert np.array_equal(bits(coef), bits(sref.coefficients(betas, VISITS, eta)))
        for i, t in enumerate(VISITS):
            s = coef[2, i]
            steps.append(Step("coef", int(t), tuple(coef[:, i]), z=None if s == 0 else draws(B, L, F, 110 + i)))
    for j, (a, b, s) in enumerate(ARBITRARY):
        steps.append(Step("coef", 5, (a, b, s), z=None if s == 0 else draws(B, L, F, 120 + j), wide=True))
    sol = sampling.solver_coefficients(betas, VISITS)
    assert sol[2, 0] == 0 and sol[2, 1] != 0 and sol[2, 2] != 0
    steps.append(Step("solver", int(VISITS[0]), tuple(sol[:, 0])))
    steps.append(Step("solver", int(VISITS[1]), tuple(sol[:, 1]), prev=previous_x0(flags, B, L, 41)))
    steps.append(Step("solver", int(VISITS[2]), tuple(sol[:, 2]), prev=previous_x0(flags, B, L, 42)))
    dd = sampling.ddim_coefficients(betas, VISITS, 0.5)
    steps.append(Step("x0", int(VISITS[1]), tuple(dd[:, 1]) + tuple(sol[3:, 1]), z=draws(B, L, F, 131)))
    steps.append(Step("x0", int(VISITS[3]), tuple(dd[:, 3]) + tuple(sol[3:, 3])))
    return steps


def state_of(step: Step, flags) -> np.ndarray:
    """The state a hook call of part A starts from.  The arbitrary triples start from a state four times as wide: (-0.25, 3.5, 0)
    quarters the state and draws nothing, and a quarter of N(0, 3^2) passes pi nowhere."""
    return state(flags, len(LENS), L, 6, widen=4.0) if step.wide else state(flags, len(LENS), L, 5)


def stages(step: Step, x, eps, is_angle) -> dict:
    """name -> (value before the wrap, value after it) for every wrap the statement of ``step`` applies under ``is_angle``,
    in float32: "x" (the new state) everywhere, "x0" (the written prediction) and "d" (the difference to the previous
    prediction, where c != 0) for the solver, "x0" for a steered visit.  The value after the wrap of "x" and "x0" is the
    hook's expected output."""
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    none = [False] * x.shape[-1]
    out = {}
    if step.kind == "plain":
        out["x"] = (plain_update(x, eps, *step.coef, step.z, none), plain_update(x, eps, *step.coef, step.z, is_angle))
    elif step.kind == "coef":
        out["x"] = (sref.update(x, eps, *step.coef, step.z, none), sref.update(x, eps, *step.coef, step.z, is_angle))
    elif step.kind == "x0":
        a, b, s, u, v = step.coef
        out["x"] = (sref.update(x, eps, a, b, s, step.z, none), sref.update(x, eps, a, b, s, step.z, is_angle))
        out["x0"] = (vref.update(x, eps, None, a, b, 0.0, u, v, none)[1], vref.update(x, eps, None, a, b, 0.0, u, v, is_angle)[1])
    else:
        a, b, c, u, v = (np.float32(k) for k in step.coef)
        want, want0 = vref.update(x, eps, step.prev, a, b, c, u, v, is_angle)
        out["x0"] = (((u * x).astype(np.float32) + (v * eps).astype(np.float32)).astype(np.float32), want0)
        m = ((a * x).astype(np.float32) + (b * eps).astype(np.float32)).astype(np.float32)
        if c != 0:
            d_raw = (want0 - step.prev).astype(np.float32)
            d = _wrap_cols(d_raw.copy(), is_angle)
            out["d"] = (d_raw, d)
            m = (m + (c * d).astype(np.float32)).astype(np.float32)
        out["x"] = (m, want)
    return out


def expected(step: Step, x, eps, is_angle) -> dict:
    """The hook's outputs by name: "x", and "x0" where the hook writes one."""
    return {k: v[1] for k, v in stages(step, x, eps, is_angle).items() if k != "d"}


def wrap_witnesses(st: dict, flags, ok, outputs_only=False) -> list:
    """Condition 1 on the stages of one statement: the (stage, column) pairs WITHOUT a witness (empty = the condition holds).
    A non-angular column needs a valid element of the result beyond pi in magnitude -- wrapping it by mistake changes it; an
    angular column needs a valid element whose value before the wrap lies outside [-pi, pi) -- leaving the wrap out changes
    it.  Both by MARGIN.  ``outputs_only``: "d", which is no output, is asked for the angular columns alone (within a run the
    difference of two successive predictions is small, and nothing can make a bond length's pass pi)."""
    missing = []
    for key, (before, after) in st.items():
        for f, a in enumerate(flags):
            if outputs_only and key == "d" and not a:
                continue
            col = before[..., f][ok[..., f]].astype(np.float64) if a else after[..., f][ok[..., f]].astype(np.float64)
            if not (np.abs(col) > np.pi + MARGIN).any():
                missing.append((key, f))
    return missing


def check_step(step: Step, x, eps, flags, ok, outputs_only=False):
    """Conditions 1, 2 and the self-consistency of the restatement (condition 4's last two items) for one hook call."""
    F = len(flags)
    st = stages(step, x, eps, flags)
    assert wrap_witnesses(st, flags, ok, outputs_only) == [], (step.name, wrap_witnesses(st, flags, ok, outputs_only))
    raw, want, other = expected(step, x, eps, [False] * F), expected(step, x, eps, flags), expected(step, x, eps, rotated(flags))
    for key in want:
        for f, a in enumerate(flags):
            w = want[key][..., f][ok[..., f]]
            assert (np.abs(raw[key][..., f][ok[..., f]]) > np.pi + MARGIN).any(), (step.name, key, f)   # wrap = 0: no column stays inside
            if a:
                assert (np.abs(w) <= PI).all(), (step.name, key, f)
            elif step.kind != "solver" or step.coef[2] == 0:   # (a solver visit's unwrapped arithmetic: below)
                assert np.array_equal(bits(w), bits(raw[key][..., f][ok[..., f]])), (step.name, key, f)
            if rotated(flags)[f] != a:   # condition 2: a flag read from the neighbouring bit gives other bits in this column
                assert not np.array_equal(bits(w), bits(other[key][..., f][ok[..., f]])), (step.name, key, f)
    if step.kind == "solver" and step.coef[2] != 0:   # non-angular columns: a x + b eps + c (x0 - prev), nothing wrapped
        a, b, c, u, v = (np.float32(k) for k in step.coef)
        x0 = ((u * x).astype(np.float32) + (v * eps).astype(np.float32)).astype(np.float32)
        m = ((a * x).astype(np.float32) + (b * eps).astype(np.float32)).astype(np.float32)
        m = (m + (c * (x0 - step.prev).astype(np.float32)).astype(np.float32)).astype(np.float32)
        for f, ang in enumerate(flags):
            if not ang:
                assert np.array_equal(bits(want["x"][..., f]), bits(m[..., f])) and np.array_equal(bits(want["x0"][..., f]), bits(x0[..., f]))


# ------------------------------------------------------------------------------------------------ part B: fixed elements
def fixed_masks(lens, L, F, seed=17):
    """uint8 [B, L, F]: every feature column has a fixed and a free valid element in every batch item of length >= 2
    (condition 3).  Item 0: scattered single features; item 1: whole rows 3 .. 11; item 2: every other position, the
    column's parity swapped."""
    B = len(lens)
    rng = np.random.default_rng(seed)
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    for b, n in enumerate(lens):
        kind = b % 3
        if kind == 0:
            pick = rng.random((n, F)) < 0.3
            pick[0, :] = np.arange(F) % 2 == 0
            pick[n - 1, :] = np.arange(F) % 2 == 1
            fixed[b, :n] = pick
        elif kind == 1:
            fixed[b, 3: min(12, n - 1)] = 1
        else:
            fixed[b, :n] = (np.arange(n)[:, None] + np.arange(F)[None, :]) % 2
    return fixed


def known_values(flags, B, L, seed=18) -> np.ndarray:
    """known: non-angular columns N(0, 6^2).  Angular columns: half of the elements (at random) within 0.005 pi .. 0.07 pi of
    the seam, so that a replacement at a low level, which adds little noise, crosses it somewhere in every column; the other
    half N(0, 6^2), NOT wrapped (any finite value is legal, and level 0 returns its bits), so that a replacement at a middle
    level, which keeps about half of the value and draws from N(0, 1), still does."""
    rng = np.random.default_rng(seed)
    shape = (B, L, len(flags))
    plain = rng.normal(0.0, 6.0, shape)
    near = rng.choice([-1.0, 1.0], shape) * rng.uniform(0.93 * np.pi, 0.995 * np.pi, shape)
    ang = np.where(rng.random(shape) < 0.5, near, rng.normal(0.0, 6.0, shape))
    return np.where(np.asarray(flags, dtype=bool), ang, plain).astype(np.float32)


def check_fixed(fixed, lens):
    """Condition 3."""
    for b, n in enumerate(lens):
        if n < 2:
            continue
        col = fixed[b, :n].astype(bool)
        assert col.any(axis=0).all() and (~col).any(axis=0).all(), b


def replacement_stages(known, level, coef, z, is_angle) -> dict:
    """The replacement statement's value before and after its wrap (level >= 1)."""
    F = known.shape[-1]
    return {"known": (ipr.known_at_level(known, level, coef, z, [False] * F), ipr.known_at_level(known, level, coef, z, is_angle))}


# ------------------------------------------------------------------------------------------------ part C: the run families
FAMILIES = ["plain", "strided", "solver", "inpaint", "strided_inpaint"]
LOOP_VISITS = np.array([9, 6, 3, 0], dtype=np.int32)
LOOP_ETA = 1.0
# the input seed of every (d_model, family), chosen on the CPU: the first for which every visit of the oracle's run meets
# the conditions (tests/test_feature_sets.py asserts that it does)
LOOP_SEEDS = {(192, "plain"): 0, (192, "strided"): 3, (192, "solver"): 3, (192, "inpaint"): 8, (192, "strided_inpaint"): 1,
              (128, "plain"): 0, (128, "strided"): 1, (128, "solver"): 0, (128, "inpaint"): 7, (128, "strided_inpaint"): 5}


@dataclass
class Visit:
    """One row of a run: the update (a Step) and, for the families with fixed elements, the level the fixed elements leave at
    with their draws (None at level 0)."""
    step: Step
    level: Optional[int] = None
    zk: Optional[np.ndarray] = None


@dataclass
class LoopInputs:
    x_init: np.ndarray
    noise: Optional[np.ndarray]          # plain, inpaint: [T, ...] (row t); strided, strided_inpaint: [K, ...] (row i); solver: None
    known: Optional[np.ndarray] = None
    fixed: Optional[np.ndarray] = None
    kcoef: Optional[np.ndarray] = None
    known_noise: Optional[np.ndarray] = None   # inpaint: [T + 1, ...] (row = level); strided_inpaint: [K + 1, ...] (row 0 = the start)


def loop_inputs(family, flags, betas, seed) -> LoopInputs:
    F, B, Lp, Tn = len(flags), len(LOOP_LENS), LOOP_L, LOOP_T
    x = state(flags, B, Lp, 1000 + seed)
    rows = {"plain": Tn, "inpaint": Tn, "strided": len(LOOP_VISITS), "strided_inpaint": len(LOOP_VISITS)}.get(family)
    noise = None if rows is None else np.stack([draws(B, Lp, F, 2000 + 31 * seed + r) for r in range(rows)])
    inp = LoopInputs(x, noise)
    if family.endswith("inpaint"):
        inp.known, inp.fixed, inp.kcoef = known_values(flags, B, Lp, 3000 + seed), fixed_masks(LOOP_LENS, Lp, F, 17 + seed), ipr.levels(betas)
        inp.known_noise = np.stack([draws(B, Lp, F, 4000 + 31 * seed + r) for r in range(rows + 1)])
    return inp


def start_of(family, inp: LoopInputs, flags) -> np.ndarray:
    """The state the first visit starts from: x_init, its fixed elements replaced at the start level where the family has any."""
    if family == "inpaint":
        return ipr.replace(inp.x_init, inp.known, inp.fixed, LOOP_T, inp.kcoef, inp.known_noise[LOOP_T], flags)
    if family == "strided_inpaint":
        return ipr.replace(inp.x_init, inp.known, inp.fixed, int(LOOP_VISITS[0]) + 1, inp.kcoef, inp.known_noise[0], flags)
    return inp.x_init


def loop_tables(family, betas):
    """The coefficient table the entry takes (None for the plain sampler's two families, which read the handle's own)."""
    if family in ("strided", "strided_inpaint"):
        return sampling.ddim_coefficients(betas, LOOP_VISITS, LOOP_ETA)
    if family == "solver":
        return sampling.solver_coefficients(betas, LOOP_VISITS)
    return None


def n_rows(family) -> int:
    return LOOP_T if family in ("plain", "inpaint") else len(LOOP_VISITS)


def visit_of(family, i, betas, inp: LoopInputs, prev_x0=None, z=None, zk=None) -> Visit:
    """Row i's visit.  z / zk given: the draws to use in place of the arrays of ``inp`` (a Philox run)."""
    table = loop_tables(family, betas)
    if family in ("plain", "inpaint"):
        t = LOOP_T - 1 - i
        c = tuple(beta_schedules.step_coefficients(betas).numpy()[:, t])
        step = Step("plain", t, c, z=None if t == 0 else (inp.noise[t] if z is None else z))
        if family == "plain":
            return Visit(step)
        return Visit(step, t, None if t == 0 else (inp.known_noise[t] if zk is None else zk))
    t = int(LOOP_VISITS[i])
    if family == "solver":
        return Visit(Step("solver", t, tuple(table[:, i]), prev=prev_x0 if table[2, i] != 0 else None))
    s = table[2, i]
    step = Step("coef", t, tuple(table[:, i]), z=None if s == 0 else (inp.noise[i] if z is None else z))
    if family == "strided":
        return Visit(step)
    level = int(LOOP_VISITS[i + 1]) + 1 if i + 1 < len(LOOP_VISITS) else 0
    return Visit(step, level, None if level == 0 else (inp.known_noise[i + 1] if zk is None else zk))


def visit_expected(v: Visit, x, eps, flags, inp: LoopInputs) -> dict:
    """The row a visit leaves ("x"), and the solver's written prediction ("x0")."""
    out = expected(v.step, x, eps, flags)
    if v.level is not None:
        out["x"] = ipr.replace(out["x"], inp.known, inp.fixed, v.level, inp.kcoef, v.zk, flags)
    return out


def check_visit(v: Visit, x, eps, flags, ok, inp: LoopInputs):
    """Conditions 1 and 2 for a visit of a run: the update's on the free valid elements, the replacement's on the fixed ones."""
    fx = np.zeros_like(ok) if v.level is None else inp.fixed.astype(bool)
    check_step(v.step, x, eps, flags, ok & ~fx, outputs_only=True)
    if v.level:
        st = replacement_stages(inp.known, v.level, inp.kcoef, v.zk, flags)
        assert wrap_witnesses(st, flags, ok & fx) == [], (v.step.name, v.level, wrap_witnesses(st, flags, ok & fx))


def reference_loop(family, model, flags, betas, inp: LoopInputs):
    """(rows [K, B, L, F], the visits with the states and predictions they started from) of a run with an oracle model."""
    x, prev, rows, trace = start_of(family, inp, flags), None, [], []
    for i in range(n_rows(family)):
        v = visit_of(family, i, betas, inp, prev_x0=prev)
        eps = sref.forward(model, x, v.step.t, LOOP_LENS).numpy()
        out = visit_expected(v, x, eps, flags, inp)
        trace.append((v, x, eps))
        x, prev = out["x"], out.get("x0")
        rows.append(x)
    return np.stack(rows), trace


# ------------------------------------------------------------------------------------------------ part B: fixed elements, jumps, ties
FIXED_LAYOUTS = ["canonical", "full16"]
FIXED_VARIANTS = [("f16x3", 192, 6), ("f32", 96, 3)]
JUMPS = [(0, 1), (1, 3), (3, 5)]   # (level from, level to) at T = 8; beyond level 5 the replacement keeps under two fifths of the
                                   # known value and Philox draws from N(0, 1): no angular column could be asked to cross the seam
JUMP_SEED, JUMP_OFFSET = 0xC0FFEE1234567, 5
TIES = [(0, 4, 4), (1, 3, 4), (0, 1, 1)]         # lens 24, 17, 9: the whole front | a lead-in row | untied
TIE_COEF = (1.0, -0.9, 0.4)                      # one visit at t = 4 with coefficients by value (any finite triple is legal)
TIE_T = 4
TIE_SEEDS = {("canonical", 192): 0, ("canonical", 96): 0, ("full16", 192): 0, ("full16", 96): 0}   # chosen on the CPU, like LOOP_SEEDS


FIXED_SEEDS = {("canonical", 192): 0, ("canonical", 96): 0, ("full16", 192): 1, ("full16", 96): 1}   # chosen on the CPU, like LOOP_SEEDS


def fixed_inputs(flags, seed) -> LoopInputs:
    """Part B's state, known values, mask and level table (T = 8, B = 3, L = 24)."""
    F, B = len(flags), len(LENS)
    betas = beta_schedules.cosine_beta_schedule(T)
    return LoopInputs(state(flags, B, L, 5), None, known_values(flags, B, L, 3000 + seed), fixed_masks(LENS, L, F, 17 + seed), ipr.levels(betas))


def fixed_visits(flags, betas) -> list:
    """The conditioned hook calls of part B, each from ``fixed_inputs(flags).x_init``: fd_p_sample_step_inpaint at t = 5 and
    t = 0, fd_p_sample_step_coef_inpaint at visit 1 of 7, 4, 2, 0 (lands on level 3) and at its last visit (level 0)."""
    F, B = len(flags), len(LENS)
    table = beta_schedules.step_coefficients(betas).numpy()
    dd = sampling.ddim_coefficients(betas, VISITS, 0.5)
    return [Visit(Step("plain", 5, tuple(table[:, 5]), z=draws(B, L, F, 201)), 5, draws(B, L, F, 211)),
            Visit(Step("plain", 0, tuple(table[:, 0])), 0, None),
            Visit(Step("coef", 4, tuple(dd[:, 1]), z=draws(B, L, F, 202)), 3, draws(B, L, F, 212)),
            Visit(Step("coef", 0, tuple(dd[:, 3])), 0, None)]


def jump_state(flags) -> np.ndarray:
    """The state the jumps start from: twice as wide as ``state`` -- a jump shrinks it (jk < 1) and only a score or so of
    elements per column are free."""
    return state(flags, len(LENS), L, 6, widen=2.0)


def jump_stages(x, jk, js, z_free, flags) -> dict:
    """The free elements of a jump before and after the wrap."""
    jk, js = np.float32(jk), np.float32(js)
    v = ((jk * np.asarray(x, dtype=np.float32)).astype(np.float32) + (js * np.asarray(z_free, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    return {"jump": (v, _wrap_cols(v.copy(), flags))}


def tie_inputs(flags, seed, model) -> np.ndarray:
    """The start of the one-visit tied run.  The init tie makes the copies of a unit row equal, and the network, which sees
    positions only relative to each other, then predicts nearly the same for each: the copies reach the final tie about 1e-3
    apart.  So the seam cannot be straddled by placing copies; it is placed between them: with the oracle ``model``, copy 0 of
    every unit row of a tied sequence is moved (three passes of a fixed-point step) until the mean over the copies of the
    value before the visit's wrap is +-pi in every angular column.  Non-angular columns of those rows start at +-3.6."""
    import repeat_reference as rref
    x = state(flags, len(LENS), L, 70 + seed)
    ang = np.asarray(flags, dtype=bool)
    rng = np.random.default_rng(71 + seed)
    a, b, _ = TIE_COEF
    sign = {}
    for i, (start, period, units) in enumerate(TIES):
        if units > 1:
            sign[i] = rng.choice([-1.0, 1.0], (period, len(flags)))
            x[i, start: start + period] = np.where(ang, 3.1 * sign[i], 3.6 * sign[i]).astype(np.float32)
    for _ in range(3):
        tied = rref.tie(x, LENS, TIES, flags, init=True)
        raw = sref.update(tied, sref.forward(model, tied, TIE_T, LENS).numpy(), a, b, 0.0, None, [False] * len(flags)).astype(np.float64)
        for i, (start, period, units) in enumerate(TIES):
            if units > 1:
                mean = np.mean([raw[i, start + k * period: start + (k + 1) * period] for k in range(units)], axis=0)
                move = (np.pi * sign[i] - mean) / a
                x[i, start: start + period] = np.where(ang, x[i, start: start + period] + move, x[i, start: start + period]).astype(np.float32)
    return x


def tie_expected(x_init, eps_of, flags, z):
    """fd_sample_repeat's one visit -> (the state the final tie starts from, the final state): the init tie, the strided
    update without a draw on the prediction ``eps_of(state)``, the tie with s z."""
    import repeat_reference as rref
    a, b, s = TIE_COEF
    x = rref.tie(x_init, LENS, TIES, flags, init=True)
    mid = sref.update(x, eps_of(x), a, b, 0.0, None, flags)
    return mid, rref.tie(mid, LENS, TIES, flags, s=s, z=z)


def check_tie(mid, out, flags, z):
    """The copies straddle the seam in an angular column and lie beyond pi in a non-angular one, in every tied sequence; the
    result is then not what all-angular (or no angular) flags give: a non-angular column's tied mean is the plain mean."""
    import repeat_reference as rref
    ang = np.asarray(flags, dtype=bool)
    a, b, s = TIE_COEF
    for i, (start, period, units) in enumerate(TIES):
        if units == 1:
            continue
        copies = np.stack([mid[i, start + k * period: start + (k + 1) * period] for k in range(units)])   # [units, period, F]
        spread = copies.max(axis=0) - copies.min(axis=0)
        assert (spread[:, ang] > 6.28).sum() >= 3, i     # angular elements of unit rows with copies next to either end of [-pi, pi)
        assert (np.abs(copies[..., ~ang]).min(axis=0) > np.pi + MARGIN).any(), i
        rows = slice(start, start + period * units)
        for other in ([True] * len(flags), [False] * len(flags)):
            alt = rref.tie(mid, LENS, TIES, other, s=s, z=z)
            cols = ang != np.asarray(other, dtype=bool)
            assert not np.array_equal(bits(alt[i, rows][:, cols]), bits(out[i, rows][:, cols])), (i, other[0])
        plain = copies[..., ~ang].astype(np.float64).mean(axis=0) + s * z[i, start: start + period][:, ~ang]
        assert np.abs(out[i, start: start + period][:, ~ang] - plain).max() < 1e-5, i     # the plain mean, unwrapped
