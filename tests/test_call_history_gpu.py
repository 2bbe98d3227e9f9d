"""A model handle's results must not depend on its earlier calls (needs an MI355X: pytest -m gpu).

One fd_model keeps, between calls: up to four (B, L) workspaces; row images and q / k / v^T buffers zeroed at allocation only;
the token-row table (fd_ar_sample rewrites it on the device); the step slots, per-sequence timesteps, key mask and position
ids; the inpaint staging buffer and the device UpdateDyn with its conditioning and strided tables; a captured step graph with
the plan it was captured under; the non-finite flag.  The kinds and schedules are in tests/call_history_cases.py.

THE GATE is bit equality with the same call made as the FIRST call on a fresh handle of the same weights and options (its
"solo" result): same kernels, same plan, same inputs, so no tolerance.  Before it is used, per model and plan
(test_solo_results_are_reproducible_and_not_vacuous): two fresh handles give every kind's solo result bit for bit; solo
results are finite and hold no element the entry left unwritten; any two kinds' results differ; the forward kinds are
within FWD_TOL of the fp32 oracle and the single-step kinds within STEP_TOL.

Every element of every output is compared -- every entry here defines all of them: the forwards and the single steps compute
every position, masked ones included; a padded run evolves every position; a packed run (varlen = 1) leaves x_init at and
behind a length in the final state and zeros in the history rows; fd_ar_sample returns the seed at and behind
max(seq_lengths).  The outputs start at a sentinel and the solo check finds none left.

The run families and step hooks that came after the first matrix -- the solver, the strided conditioned run without jumps,
the steered run, the repeat run, fd_p_sample_step_coef_inpaint, _solver and _coef_x0 -- are kinds of their own
(cases.LATER_KINDS), under three of the five plans (cases.LATER_PLANS).  They are the paths that share one close
(api_run.hip: close_run), and what the matrix checks for them is that nothing of a finished run of any family is left on
the handle or in the device's UpdateDyn for the next call of any other.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ar_reference
import call_history_cases as cases
import inpaint_reference as ipr
import solver_reference as vref
import strided_inpaint_reference as sir
import strided_reference as sref
from foldingdiff_amd import _binding, beta_schedules, losses, modelling, sampling
from oracle import ref_sampling
from test_gpu_parity import FWD_TOL, STEP_TOL, _inputs, _mask, _pair
from test_inpaint_gpu import ANG, F, _bits, _masks, _sample_inpaint
from test_resample_gpu import _resample
from test_solver_gpu import _solver, _step_solver
from test_steer_gpu import _params, _steered, _step_x0
from test_strided_gpu import SENTINEL, _step_coef, _strided
from test_strided_inpaint_gpu import _step_coef_inpaint, _strided_inpaint, _strided_resample

pytestmark = pytest.mark.gpu
P = _binding.ptr
B, L, T, T_START = cases.B, cases.L, cases.T, cases.T_START
UNSUPPORTED, NONFINITE, INVALID = -5, -6, -1

MODELS = {
    "main": dict(hidden=192, heads=6, ff=384, layers=2, maxpos=128, pos="relative_key", seed=7, precision="f16x3"),
    "wide": dict(hidden=384, heads=12, ff=768, layers=2, maxpos=128, pos="relative_key", seed=8, precision="f16x3"),
    "abs": dict(hidden=192, heads=6, ff=384, layers=2, maxpos=128, pos="absolute", seed=9, precision="f16x3"),
    "f32": dict(hidden=128, heads=4, ff=256, layers=2, maxpos=128, pos="relative_key", seed=10, precision="f32"),
}
_BASE, _CONST = {}, {}


def _lib():
    return _binding.load()


def _const():
    """The schedule and the tables every case shares."""
    if not _CONST:
        betas = beta_schedules.cosine_beta_schedule(T)
        grid = np.array([3, 1, 0], dtype=np.int32)
        rgrid = np.array([3, 2, 0], dtype=np.int32)
        run = np.array([3, 2, 3, 2, 0], dtype=np.int32)                 # one jump: from the level visit 2 left (1) back to 4
        visits = np.array([3, 2, 1, 2, 1, 0], dtype=np.int32)           # one jump: from level 1 back to level 3
        _CONST.update(betas=betas, kcoef=sampling.inpaint_levels(betas), grid=grid, coef=sampling.ddim_coefficients(betas, grid, 1.0),
                      rgrid=rgrid, rcoef=sampling.ddim_coefficients(betas, rgrid, 0.5), run=run,
                      rjc=sampling.strided_jump_coef(betas, rgrid, run), visits=visits, jc=sampling.resample_jump_coef(betas, visits),
                      scoef=sampling.solver_coefficients(betas, grid), stcoef=sampling.steer_coefficients(betas, grid, 1.0),
                      event=np.array([1, 0, 1], dtype=np.uint8), steer=_params())
        assert len(_CONST["jc"]) == 1 and len(_CONST["rjc"]) == 1 and (_CONST["coef"][2, :-1] != 0).all()
        assert _CONST["scoef"][2, 1] != 0 and np.array_equal(_CONST["stcoef"][:3], _CONST["coef"])     # the middle visit has a c
    return SimpleNamespace(**_CONST)


def _base(model):
    """(fp32 oracle, its state dict) of a model, built once: every handle of the model loads the same weights."""
    if model not in _BASE:
        o32, _, pm = _pair(**MODELS[model])
        _BASE[model] = (o32, pm.config, {k: v.clone() for k, v in o32.state_dict().items()})
    return _BASE[model]


class _Handle:
    """A fresh fd_model of `model` with `opts` set once, right after fd_finalize.  close() destroys it."""

    def __init__(self, model, opts=None):
        _, cfg, sd = _base(model)
        self.model = model
        self.pm = modelling.BertForDiffusionBase(cfg, [True] * F)
        self.pm.load_state_dict(sd)
        self.pm.to("cuda:0")
        self.pm.set_precision(MODELS[model]["precision"])
        self.h = self.pm.prepare(_const().betas)
        self.keep = []          # device buffers a call left in use (an unfinished run's)
        for k, v in (opts or {}).items():
            self.opt(k, v)

    def opt(self, name, value):
        _binding.check(_lib().fd_set_option(self.h, name.encode(), int(value)))

    def close(self):
        _binding.check(_lib().fd_synchronize(self.h))
        self.pm._invalidate()
        self.keep.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------------------------- the cases
def _case(kind, lens, nb=B, nl=L, salt=0, absolute=False):
    """Every input of one call of `kind` at (nb, nl) with `lens`: its own x, masks, draws and seeds (salt: the kind's index)."""
    g = torch.Generator().manual_seed(5000 + salt)
    rn = lambda *s: torch.randn(*s, generator=g).numpy()   # noqa: E731
    lens = [int(n) for n in lens]
    c = SimpleNamespace(kind=kind, uid=(kind, tuple(lens), nb, nl, salt), B=nb, L=nl, lens_list=lens,
                        lens=np.ascontiguousarray(np.asarray(lens, dtype=np.int32)),
                        x=np.ascontiguousarray(_inputs(nb, nl, seed=100 + salt).numpy()), seed=7000 + salt, t=1 + salt % 3)
    c.z, c.zk = rn(nb, nl, F), rn(nb, nl, F)
    c.noise = rn(T_START + 1, nb, nl, F)
    c.known = np.random.default_rng(300 + salt).uniform(-3.1, 3.1, (nb, nl, F)).astype(np.float32)
    c.fixed = _masks(lens, nl, rows=(3 + salt % 5, 20 + salt))[1]
    c.tv = np.ascontiguousarray(np.roll(np.resize(np.array([0, T - 1, 64, 3, 3], dtype=np.int32), nb), salt))
    # fd_forward_ex: the prefix mask with holes, a masked first key, one sequence attending to nothing
    m = _mask(lens, nl).numpy().astype(np.uint8)
    m[0, 0] = 0
    m[1 % nb, nl // 3: nl // 2] = 0
    m[:, 5 + salt % 3] = 0
    m[nb - 1, :] = 0
    c.mask = np.ascontiguousarray(m)
    c.pids = None
    if absolute:
        c.pids = np.ascontiguousarray(np.stack([torch.randperm(128, generator=g)[:nl].numpy() for _ in range(nb)]).astype(np.int32))
    # fd_ar_*: the target lengths index the table, the keys' prefix is another arrangement of the same lengths
    c.seq_lengths = c.lens
    c.key_lens = np.ascontiguousarray(c.lens[::-1])
    c.ar_seed = np.ascontiguousarray(((torch.rand(nb, nl, F, generator=g) * 2 - 1) * 3.0).numpy())
    # fd_denoise_loss_ex: the device noises x with the levels of tv
    k = _const().kcoef
    c.keep, c.spread = np.ascontiguousarray(k[0, c.tv + 1]), np.ascontiguousarray(k[1, c.tv + 1])
    c.pair_coef = np.ascontiguousarray(np.linspace(0.5, 1.5, nb).astype(np.float32))
    # the later kinds (drawn last: the inputs above are what they were): the replacement's draws of a three-visit grid's four
    # levels, the three visits' draws, the uniforms of two events for one group, the ties
    n_grid = len(_const().grid)
    c.knoise, c.gnoise = rn(n_grid + 1, nb, nl, F), rn(n_grid, nb, nl, F)
    c.u = np.ascontiguousarray(torch.rand(2, 1, generator=g, dtype=torch.float64).numpy())
    c.ties = np.ascontiguousarray(np.asarray(cases.repeat_ties(lens), dtype=np.int32))
    return c


_CASES = {}


def _kind_case(model, kind):
    key = (model, kind)
    if key not in _CASES:
        _CASES[key] = _case(kind, cases.lens_of(kind), salt=cases.A_KINDS.index(kind), absolute=MODELS[model]["pos"] == "absolute")
    return _CASES[key]


def _new(c, rows=None):
    shape = (c.B, c.L, F) if rows is None else (rows, c.B, c.L, F)
    return np.full(shape, SENTINEL, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- the kinds: (H, case) -> (rc, {name: array})
def _k_forward(H, c):
    out = _new(c)
    return _lib().fd_forward(H.h, P(c.x), c.t, P(c.lens), c.B, c.L, P(out)), {"eps": out}


def _k_forward_t(H, c):
    out = _new(c)
    return _lib().fd_forward_t(H.h, P(c.x), P(c.tv), P(c.lens), c.B, c.L, P(out)), {"eps": out}


def _k_forward_ex(H, c):
    out = _new(c)
    return _lib().fd_forward_ex(H.h, P(c.x), c.t, P(c.mask), P(c.pids), c.B, c.L, P(out)), {"eps": out}


def _k_step(H, c):
    out = _new(c)
    return _lib().fd_p_sample_step(H.h, P(c.x), c.t, P(c.lens), c.B, c.L, P(c.z), 1, P(out)), {"x": out}


def _k_step_inpaint(H, c):
    out = _new(c)
    rc = _lib().fd_p_sample_step_inpaint(H.h, P(c.x), c.t, P(c.lens), c.B, c.L, P(c.z), 1, P(c.known), P(c.fixed), P(_const().kcoef),
                                         P(c.zk), P(out))
    return rc, {"x": out}


def _k_step_coef(H, c):
    a, b, s = _const().coef[:, 0]
    rc, eps, out = _step_coef(H.h, c.x, T_START, c.lens_list, a, b, s, c.z)
    return rc, {"eps": eps, "x": out}


def _fd_sample(H, c, noise, full_history):
    rows = -(-(T_START + 1) // full_history) if full_history else 1
    out = _new(c, rows)
    rc = _lib().fd_sample(H.h, P(c.x), P(c.lens), c.B, c.L, T_START, P(noise), C.c_uint64(c.seed), P(out), full_history)
    return rc, {"x": out}


def _k_run_history(H, c):
    return _fd_sample(H, c, None, 1)


def _k_run_packed(H, c):
    H.opt("varlen", 1)
    try:
        return _fd_sample(H, c, None, 0)
    finally:
        H.opt("varlen", 0)


def _k_run_host_noise(H, c):
    H.opt("use_graph", 0)
    try:
        return _fd_sample(H, c, c.noise, 2)
    finally:
        H.opt("use_graph", 1)


def _k_inpaint(H, c):
    rc, out = _sample_inpaint(H.h, c.x, c.lens_list, T_START, c.known, c.fixed, _const().kcoef, c.seed, 1)
    return rc, {"x": out}


def _k_inpaint_resample(H, c):
    k = _const()
    rc, out = _resample(H.h, c.x, c.lens_list, T_START, c.known, c.fixed, k.kcoef, k.visits, k.jc, c.seed)
    return rc, {"x": out}


def _k_strided(H, c):
    k = _const()
    rc, out = _strided(H.h, c.x, c.lens_list, k.grid, k.coef, c.seed, 1)
    return rc, {"x": out}


def _k_strided_inpaint_resample(H, c):
    k = _const()
    rc, out = _strided_resample(H.h, c.x, c.lens_list, k.rgrid, k.rcoef, k.run, k.rjc, c.known, c.fixed, k.kcoef, c.seed)
    return rc, {"x": out}


def _k_ar_forward(H, c):
    out = _new(c)
    return _lib().fd_ar_forward(H.h, P(c.x), P(c.seq_lengths), P(c.key_lens), c.B, c.L, P(out)), {"out": out}


def _k_ar_sample(H, c):
    out = _new(c)
    return _lib().fd_ar_sample(H.h, P(c.ar_seed), P(c.seq_lengths), c.B, c.L, 2, P(out)), {"x": out}


def _k_loss_ex(H, c):
    o = dict(sums=np.full((c.B, F), SENTINEL, np.float64), turns=np.full((c.B, F), -7, np.int64), pair_sums=np.full(c.B, SENTINEL, np.float64),
             pairs=np.full(c.B, -7, np.int64), corrupted=_new(c), eps=_new(c))
    idx = np.arange(6, dtype=np.int32)
    rc = _lib().fd_denoise_loss_ex(H.h, P(c.x), None, P(c.z), P(c.tv), P(c.keep), P(c.spread), P(c.lens), c.B, c.L, 0,
                                   float(losses.ANGULAR_BETA), float(losses.NONANGULAR_BETA), P(c.pair_coef), P(idx), P(o["sums"]),
                                   P(o["turns"]), P(o["pair_sums"]), P(o["pairs"]), P(o["corrupted"]), P(o["eps"]))
    return rc, o


def _k_run_left_open(H, c):
    """fd_sample_begin_dev, two of the four steps, no fd_sample_end_dev: the next call on the handle ends the run."""
    dev = "cuda:0"
    x, lens = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.lens).to(dev)
    out = torch.full((c.B, c.L, F), SENTINEL, dtype=torch.float32, device=dev)
    H.keep.append((x, lens, out))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = _lib().fd_sample_begin_dev(H.h, vp(x), vp(lens), c.B, c.L, T_START, C.c_uint64(c.seed), C.c_int64(0), vp(out), 0, None)
    if rc == 0:
        rc = _lib().fd_sample_steps_dev(H.h, 2, None, 0, None)
    return rc, {}


def _k_refused(H, c):
    """Two argument errors, each FD_E_INVALID with the output untouched: a zero length, a grid that does not descend."""
    k = _const()
    out = _new(c)
    bad = c.lens.copy()
    bad[1] = 0
    rc1 = _lib().fd_forward(H.h, P(c.x), c.t, P(bad), c.B, c.L, P(out))
    rc2, out2 = _strided(H.h, c.x, c.lens_list, [3, 3, 0], k.coef, c.seed, 1)
    assert rc1 == INVALID and rc2 == INVALID and (out == SENTINEL).all() and (out2 == SENTINEL).all(), (rc1, rc2)
    return 0, {}


def _k_solver(H, c):
    k = _const()
    rc, out = _solver(H.h, c.x, c.lens_list, k.grid, k.scoef, 1)
    return rc, {"x": out}


def _k_strided_inpaint(H, c):
    k = _const()
    rc, out = _strided_inpaint(H.h, c.x, c.lens_list, k.grid, k.coef, c.known, c.fixed, k.kcoef, c.seed, 1, known_noise=c.knoise)
    return rc, {"x": out}


def _k_steered(H, c):
    """One group of five particles, events behind the first and the last visit."""
    k = _const()
    rc, out, terms, reward, logw, anc = _steered(H.h, c.x, c.lens_list, k.grid, k.stcoef, None, c.seed, k.event, c.B, k.steer, c.u)
    return rc, {"x": out, "terms": terms, "reward": reward, "logw": logw, "ancestors": anc}


def _k_repeat(H, c):
    k = _const()
    out = _new(c)
    rc = _lib().fd_sample_repeat(H.h, P(c.x), P(c.lens), c.B, c.L, P(k.grid), len(k.grid), P(k.coef), P(c.gnoise), C.c_uint64(c.seed),
                                 C.c_int64(0), P(c.ties), P(out))
    return rc, {"x": out}


def _k_step_coef_inpaint(H, c):
    k = _const()
    a, b, s = k.coef[:, 0]
    rc, eps, out = _step_coef_inpaint(H.h, c.x, T_START, c.lens_list, a, b, s, c.z, int(k.grid[1]) + 1, c.known, c.fixed, k.kcoef, c.zk)
    return rc, {"eps": eps, "x": out}


def _k_step_solver(H, c):
    """The middle visit of the grid: the one whose c is not 0, so the previous prediction (c.known stands in) is read."""
    k = _const()
    rc, eps, x0, out = _step_solver(H.h, c.x, int(k.grid[1]), c.lens_list, *k.scoef[:, 1], c.known)
    return rc, {"eps": eps, "x0": x0, "x": out}


def _k_step_coef_x0(H, c):
    rc, eps, x0, out = _step_x0(H.h, c.x, T_START, c.lens_list, *_const().stcoef[:, 0], c.z)
    return rc, {"eps": eps, "x0": x0, "x": out}


RUN = {k: globals()["_k_" + k] for k in cases.A_KINDS}
FORWARD_KINDS = ("forward", "forward_t", "forward_ex", "ar_forward", "loss_ex")
STEP_KINDS = ("step", "step_inpaint", "step_coef", "step_coef_inpaint", "step_solver", "step_coef_x0")


def _same(got, want):
    """'' when every array of `got` carries the bits of `want`'s, else what differs."""
    assert set(got) == set(want)
    bad = []
    for name in sorted(got):
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if a.tobytes() != b.tobytes():
            ne = a.view(np.uint8).reshape(a.shape + (a.itemsize,)) != b.view(np.uint8).reshape(b.shape + (b.itemsize,))
            at = np.argwhere(ne.any(axis=-1))
            bad.append(f"{name}: {len(at)} of {a.size} elements differ, first at {at[0].tolist()} ({a[tuple(at[0])]!r} != {b[tuple(at[0])]!r})")
    return "; ".join(bad)


_SOLO = {}


def _solo(model, opts_name, kind, opts=None, case=None):
    """The result of `kind` as the first call on a fresh handle of `model` under the options, computed once per module.
    (rc, outputs); every B-kind's rc is 0 except the three an FD_PREC_F32 model refuses."""
    key = (model, opts_name, kind if case is None else case.uid)
    if key not in _SOLO:
        with _Handle(model, cases.PLANS[opts_name] if opts is None else opts) as H:
            _SOLO[key] = RUN[kind](H, case or _kind_case(model, kind))
    return _SOLO[key]


def _refused_by(model, kind):
    return MODELS[model]["precision"] == "f32" and kind in cases.F32_REFUSED


# ---------------------------------------------------------------------------------------------- the gate's own conditions
def _oracle_gap(model, kind, c, out):
    """The largest gap of a forward or single-step kind's result against the fp32 oracle: (gap, tolerance)."""
    o32 = _base(model)[0]
    k = _const()
    tt = lambda t: torch.full((c.B,), int(t), dtype=torch.long)   # noqa: E731
    x, mask = torch.from_numpy(c.x), _mask(c.lens_list, c.L)
    with torch.no_grad():
        if kind == "forward":
            want = o32(x, tt(c.t), attention_mask=mask).numpy()
        elif kind == "forward_t":
            want = o32(x, torch.from_numpy(c.tv).long(), attention_mask=mask).numpy()
        elif kind == "forward_ex":
            kw = {} if c.pids is None else {"position_ids": torch.from_numpy(c.pids).long()}
            want = o32(x, tt(c.t), attention_mask=torch.from_numpy(c.mask).float(), **kw).numpy()
        elif kind == "ar_forward":
            want = ar_reference.ar_forward(o32, x, ar_reference.prefix_mask(c.key_lens.tolist(), c.L), torch.from_numpy(c.seq_lengths).long()).numpy()
            return float(np.abs(out["out"].astype(np.float64) - want).max()), FWD_TOL
        elif kind == "loss_ex":
            want = o32(torch.from_numpy(out["corrupted"]), torch.from_numpy(c.tv).long(), attention_mask=mask).numpy()
        elif kind == "step":
            want = ipr.step(o32, c.x, c.t, c.lens_list, k.betas, c.z, c.known, np.zeros_like(c.fixed), k.kcoef, c.zk, ANG)
        elif kind == "step_inpaint":
            want = ipr.step(o32, c.x, c.t, c.lens_list, k.betas, c.z, c.known, c.fixed, k.kcoef, c.zk, ANG)
        elif kind == "step_coef":
            a, b, s = k.coef[:, 0]
            want = sref.update(c.x, sref.forward(o32, c.x, T_START, c.lens_list).numpy(), a, b, s, c.z, ANG)
        elif kind == "step_coef_inpaint":
            a, b, s = k.coef[:, 0]
            want = sir.visit(c.x, sref.forward(o32, c.x, T_START, c.lens_list).numpy(), a, b, s, c.z, c.known, c.fixed, int(k.grid[1]) + 1,
                             k.kcoef, c.zk, ANG)
        elif kind == "step_solver":
            want = vref.update(c.x, sref.forward(o32, c.x, int(k.grid[1]), c.lens_list).numpy(), c.known, *k.scoef[:, 1], ANG)[0]
        elif kind == "step_coef_x0":    # the state is fd_p_sample_step_coef's: the prediction of the clean state is a further output
            a, b, s = k.stcoef[:3, 0]
            want = sref.update(c.x, sref.forward(o32, c.x, T_START, c.lens_list).numpy(), a, b, s, c.z, ANG)
    if kind in STEP_KINDS:
        return float(ref_sampling.circ_dist(out["x"], want).max()), STEP_TOL
    return float(np.abs(out["eps"].astype(np.float64) - want).max()), FWD_TOL


def _kinds_of(model, plan="auto"):
    """The second kinds of a model's matrix under a plan, in KINDS' order (the later kinds: under cases.LATER_PLANS only)."""
    kinds = {"main": cases.B_KINDS, "wide": cases.WIDE_KINDS, "abs": cases.ABS_KINDS, "f32": cases.B_KINDS}[model]
    return cases.kinds_under(plan, kinds)


def _first_kinds_of(model, plan="auto"):
    if model not in ("main", "f32"):
        return _kinds_of(model, plan)
    return cases.kinds_under(plan, cases.A_KINDS)


@pytest.mark.parametrize("model,plan", [("main", p) for p in cases.PLANS] + [("wide", "auto"), ("abs", "auto"), ("f32", "auto")])
def test_solo_results_are_reproducible_and_not_vacuous(gpu, model, plan):
    results = {}
    for kind in _kinds_of(model, plan):
        rc, out = _solo(model, plan, kind)
        if _refused_by(model, kind):
            assert rc == UNSUPPORTED, (kind, rc, _lib().fd_last_error())
            assert all((a == SENTINEL).all() for a in out.values()), kind
            continue
        assert rc == 0, (kind, rc, _lib().fd_last_error())
        with _Handle(model, cases.PLANS[plan]) as H:           # a second fresh handle: the same bits
            rc2, again = RUN[kind](H, _kind_case(model, kind))
        assert rc2 == 0 and _same(again, out) == "", (kind, _same(again, out))
        for name, a in out.items():
            assert np.isfinite(a).all(), (kind, name)
            assert not (a == (SENTINEL if a.dtype.kind == "f" else -7)).any(), (kind, name, "an element the entry did not write")
        results[kind] = out
        if kind in FORWARD_KINDS + STEP_KINDS:
            gap, tol = _oracle_gap(model, kind, _kind_case(model, kind), out)
            print(f"{model} {plan} {kind}: {gap:.3e} against the fp32 oracle (bound {tol:g})")
            assert gap <= tol, (kind, gap)
    if model == "f32":
        assert set(_kinds_of(model, plan)) - set(results) == set(cases.F32_REFUSED)
    main = lambda o: o["x"] if "x" in o else o["eps"] if "eps" in o else o["out"]   # noqa: E731
    for a in results:
        for b in results:
            if a < b and main(results[a]).shape == main(results[b]).shape:
                assert not np.array_equal(main(results[a]), main(results[b])), (a, b)
    c = _kind_case(model, "run_packed") if "run_packed" in results and MODELS[model]["precision"] == "f16x3" else None
    if c is not None:           # the packed run's contract behind the lengths: x_init (FD_PREC_F32 has no packed rows)
        beyond = ~(np.arange(L)[None, :] < c.lens[:, None])
        assert np.array_equal(_bits(results["run_packed"]["x"][0])[beyond], _bits(c.x)[beyond])


# ---------------------------------------------------------------------------------------------- A. the transition matrix
def _row(model, plan, a):
    """One handle; for every second kind b: a, then b, and b carries its solo bits.  The history accumulates on purpose.
    Where a itself has a solo result it is compared too (it follows the previous b)."""
    seconds = _kinds_of(model, plan)
    for b in seconds:      # the solo results first: at most one other handle alive while the row's own is
        _solo(model, plan, b)
    if a in seconds:
        _solo(model, plan, a)
    with _Handle(model, cases.PLANS[plan]) as H:
        for b in seconds:
            rc, got = RUN[a](H, _kind_case(model, a))
            if _refused_by(model, a):
                assert rc == UNSUPPORTED, (a, rc)
            else:
                assert rc == 0, (f"{a} (before {b}) under {plan}", rc, _lib().fd_last_error())
                if a in seconds:
                    diff = _same(got, _solo(model, plan, a)[1])
                    assert diff == "", f"{model} / {plan}: {a} (first of the pair, before {b}) is not its solo result: {diff}"
            rc, got = RUN[b](H, _kind_case(model, b))
            want_rc, want = _solo(model, plan, b)
            assert rc == want_rc, (f"{b} after {a} under {plan}", rc, _lib().fd_last_error())
            diff = _same(got, want)
            assert diff == "", f"{model} / {plan}: {b} after {a} is not its solo result: {diff}"


@pytest.mark.parametrize("a,plan", [(a, plan) for plan in cases.PLANS for a in _first_kinds_of("main", plan)])
def test_transition_matrix_row(gpu, a, plan):
    """25 first kinds x 23 second kinds under the plans of cases.LATER_PLANS, the 18 x 16 that came first under the other two."""
    _row("main", plan, a)


@pytest.mark.parametrize("model,a", [(m, a) for m in ("wide", "abs", "f32") for a in _first_kinds_of(m)])
def test_transition_matrix_row_of_the_other_models(gpu, model, a):
    """Hidden 384 (the released instantiations): the forward and sampler kinds.  Absolute positions: fd_forward, fd_forward_ex
    with position_ids, a graph run, fd_ar_forward.  FD_PREC_F32: every kind; the three it refuses (FD_E_UNSUPPORTED, output
    untouched) stay in the row as first and as second calls and leave the next call's bits alone."""
    _row(model, "auto", a)


# ---------------------------------------------------------------------------------------------- B. the shape cache
_CACHE_CALL = {"run": "run_history", "packed": "run_packed", "forward": "forward", "step": "step"}


def test_shape_cache_parked_evicted_and_recreated_workspaces(gpu):
    """cases.CACHE_SCHEDULE on one handle (six shapes, four workspaces): a return to a parked shape that holds a captured
    graph, evictions with and without a graph, returns to evicted shapes; every shape at least twice with other lengths
    (tests/test_call_history.py checks those claims against the restated policy).  Every call equals its solo bits."""
    seen, calls = {}, []
    for i, (shape, call) in enumerate(cases.CACHE_SCHEDULE):
        nb, nl = cases.SHAPES[shape]
        visit = seen.get(shape, 0)
        seen[shape] = visit + 1
        c = _case(_CACHE_CALL[call], cases.shape_lens(shape, visit), nb, nl, salt=40 + i)
        calls.append((c, _solo("main", "auto", c.kind, case=c)))
    with _Handle("main") as H:
        for i, (c, (want_rc, want)) in enumerate(calls):
            rc, got = RUN[c.kind](H, c)
            assert rc == want_rc == 0, (i, rc, _lib().fd_last_error())
            diff = _same(got, want)
            assert diff == "", f"call {i} of the schedule, {c.kind} at {(c.B, c.L)} with {c.lens_list}: {diff}"
            assert np.isfinite(got["x" if "x" in got else "eps"]).all(), i


# ---------------------------------------------------------------------------------------------- C. options changed under a workspace
def _launch_counts(H, c):
    """{kernel class: launches per step} of one more padded-or-packed run of case c under the options in force (every step
    eager and bracketed: fd_profile_every 1, as test_launch_sequence_per_option counts them)."""
    lib = _lib()
    _binding.check(lib.fd_profile_reset(H.h))
    _binding.check(lib.fd_profile_every(H.h, 1))
    try:
        rc, _ = _fd_sample(H, c, None, 0)
        assert rc == 0, lib.fd_last_error()
    finally:
        _binding.check(lib.fd_profile_every(H.h, 0))
    name, ms, n, fl, by = C.c_char_p(), C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    out = {}
    for i in range(lib.fd_profile_count(H.h)):
        _binding.check(lib.fd_profile_get(H.h, i, C.byref(name), C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        if n.value:
            assert n.value % (T_START + 1) == 0, (name.value, n.value)
            out[name.value.decode()] = n.value // (T_START + 1)
    return out


def _apply(H, state):
    for k, default in cases.OPTION_DEFAULTS.items():
        H.opt(k, state.get(k, default))


@pytest.mark.parametrize("leave", [True, False], ids=["parked", "current"])
def test_options_changed_while_a_workspace_is_parked_or_current(gpu, leave):
    """A graph is captured on (5, 101) under fuse_ffn 2; then the options of cases.OPTION_STATES come into force one after the
    other -- with `leave` a run on (3, 64) parks the workspace before each change -- and the run is made again.  Every run
    carries the bits of a fresh handle under the options then in force; a state that flips back carries the first run's;
    states with another plan carry other bits; and a profiled run launches the kernel classes the options name."""
    c = _kind_case("main", "run_history")
    other = _case("run_history", (64, 9, 33), 3, 64, salt=90)      # the call that parks (5, 101): a graph run of its own
    layers = MODELS["main"]["layers"]
    solos, solos_other = [], []
    for i, state in enumerate(cases.OPTION_STATES):
        key = "options:" + repr(sorted(state.items()))
        with_opts = dict(cases.OPTION_DEFAULTS, **state)
        solos.append(_solo("main", key, "run_history", opts=with_opts))
        solos_other.append(_solo("main", key, "run_history", opts=with_opts, case=other))
        assert solos[-1][0] == 0 and solos_other[-1][0] == 0
    x = [s[1]["x"] for s in solos]
    assert not np.array_equal(x[0], x[1])        # fuse_ffn 2 against 0: another summation order (include/fdmi.h)
    assert not np.array_equal(x[5], x[6])        # fuse_attn 0 against 1
    assert not np.array_equal(x[0], x[3])        # packed: zeros behind the lengths ...
    valid = np.arange(L)[None, :] < c.lens[:, None]
    assert np.array_equal(_bits(x[0])[:, valid], _bits(x[3])[:, valid])   # ... the same bits below them
    with _Handle("main") as H:
        fused_attn_takes = bool(_lib().fd_fused_attn_supported(H.h, L))
        for i, state in enumerate(cases.OPTION_STATES):
            if leave and i > 0:      # under the options of the state before: (3, 64)'s own graph goes stale at every change too
                rc, got = _k_run_history(H, other)
                assert rc == 0 and _same(got, solos_other[i - 1][1]) == "", (i, _same(got, solos_other[i - 1][1]))
            _apply(H, state)
            rc, got = _k_run_history(H, c)
            assert rc == 0, (i, state, _lib().fd_last_error())
            diff = _same(got, solos[i][1])
            assert diff == "", f"state {i} {state}: not the fresh handle's bits under the same options: {diff}"
            if i in cases.OPTION_FLIPS_BACK:
                assert _same(got, solos[0][1]) == "", i
            counts = _launch_counts(H, c)
            ffn2, attn = state.get("fuse_ffn") == 2, state.get("fuse_attn", -1)
            want = dict(attn_out_ffn_fused=layers * ffn2, gemm_ffn_up=layers * (not ffn2), gemm_ffn_down=layers * (not ffn2))
            if attn >= 0:
                fused = attn == 1 and fused_attn_takes
                want.update(qkv_attention_fused=layers * fused, attention=layers * (not fused))
            assert {k: counts.get(k, 0) for k in want} == want, (i, state, counts)
            # the profiled eager run is history too: the graph run behind it is still the fresh handle's
            rc, got = _k_run_history(H, c)
            assert rc == 0 and _same(got, solos[i][1]) == "", (i, state, _same(got, solos[i][1]))


# ---------------------------------------------------------------------------------------------- D. two handles interleaved
_INTERLEAVED = ("forward", "run_history", "step", "run_packed", "inpaint", "loss_ex", "strided", "forward_t", "run_host_noise")


@pytest.mark.parametrize("first,second", [("main", "wide"), ("main", "f32")])
def test_two_handles_interleaved(gpu, first, second):
    """Two models alive in one process on one device, their calls alternating (the second handle goes through the kinds in
    the opposite order): the process-wide statics -- LDS opt-ins, the CU count, the environment overrides -- and the
    per-handle state do not mix.  Every call equals its solo bits."""
    for k in _INTERLEAVED:
        _solo(first, "auto", k)
        _solo(second, "auto", k)
    with _Handle(first) as H1, _Handle(second) as H2:
        for k1, k2 in zip(_INTERLEAVED + _INTERLEAVED[::-1], _INTERLEAVED[::-1] + _INTERLEAVED):
            for H, k in ((H1, k1), (H2, k2)):
                rc, got = RUN[k](H, _kind_case(H.model, k))
                want_rc, want = _solo(H.model, "auto", k)
                assert rc == want_rc == 0, (H.model, k, rc, _lib().fd_last_error())
                diff = _same(got, want)
                assert diff == "", f"{H.model}: {k} (interleaved with {first if H is H2 else second}) is not its solo result: {diff}"


# ---------------------------------------------------------------------------------------------- E. after a non-finite call
@pytest.mark.parametrize("plan", ["unfused", "auto"])
def test_calls_after_a_nonfinite_call_are_healthy(gpu, plan):
    """A padded fd_forward at (5, 101) with long sequences whose input holds one NaN (later: one Inf) at a valid position 57
    answers FD_E_NONFINITE.  The NaN reaches every row of that sequence, and with them q / k / v^T slots that a later call
    with a shorter sequence does not rewrite but still reads: keys 33 .. 63 of a 33-long sequence get p = 0 and their v^T slot
    still enters the P V product (0 * NaN).  The library must poison the call that got the NaN only, as the reference does:
    behind it, on the same handle and with healthy inputs, a packed run that puts the sequence at 33, a padded forward and a
    single step succeed with their solo bits.  (Before check_flag zeroed the workspace's images and q / k / v^T buffers again
    behind such a call, the packed run returned FD_E_NONFINITE under both plans, after the NaN and after the Inf.)"""
    packed = _case("run_packed", cases.HEALTHY_PACKED_LENS, salt=70)
    fwd = _case("forward", cases.lens_of("forward"), salt=71)
    step = _case("step", cases.lens_of("step"), salt=72)
    healthy = [("the packed run", packed), ("the padded forward", fwd), ("the step", step)]
    want = [_solo("main", plan, c.kind, case=c) for _, c in healthy]
    assert all(rc == 0 and np.isfinite(o["x" if "x" in o else "eps"]).all() for rc, o in want)
    failures = []
    with _Handle("main", cases.PLANS[plan]) as H:
        for value in (np.nan, np.inf):
            bad = _case("forward", cases.POISON_LENS, salt=73)
            bad.x[cases.POISON_AT] = value
            rc, _ = _k_forward(H, bad)
            assert rc == NONFINITE, (value, rc, _lib().fd_last_error())
            for (name, c), (_, solo) in zip(healthy, want):
                rc, got = RUN[c.kind](H, c)
                if rc != 0:
                    failures.append(f"after {value}: {name} returned {rc} ({_lib().fd_last_error().decode()})")
                elif _same(got, solo):
                    failures.append(f"after {value}: {name}: {_same(got, solo)}")
    assert not failures, failures
