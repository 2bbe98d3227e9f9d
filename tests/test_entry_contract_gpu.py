"""The argument-error and call-order contract of the older model entries: fd_forward, fd_forward_t, fd_forward_ex,
fd_p_sample_step, fd_sample_ex, fd_sample_begin_dev and the FD_E_STATE paths of fd_sample_steps_dev / fd_sample_end_dev.
Every refusal is pinned by its return code, a distinguishing word of its message, and an output buffer (prefilled with -7)
that stays untouched; where two things are wrong at once, the error of the earlier check is the one reported.  The newer
entries' errors are tests/test_inpaint_gpu.py's and tests/test_resample_gpu.py's.

Plain runs around conditioned runs: tests/test_inpaint_gpu.py asserts that a plain run is bit-identical before and after
fd_sample_inpaint, and tests/test_resample_gpu.py:136-153 (`before` ... `after`, "the dyn fields are cleared") the same around
fd_sample_inpaint_resample with a four-jump schedule on a larger model.  Here: the one-jump schedule 5 4 3 4 3 2 1 0, and a
resample call refused for a bad schedule.

The smallest models of the suite (2 layers, B = 2, L = 16, lens = [16, 9], T = 6): hidden 96 / 3 heads in f32, hidden 192 /
6 heads in f16x3."""
import ctypes as C

import numpy as np
import pytest
import torch

from foldingdiff_amd import _binding, beta_schedules, sampling
from test_gpu_parity import _inputs, _pair
from test_inpaint_gpu import F, _bits, _masks
from test_resample_gpu import _resample

pytestmark = pytest.mark.gpu
P = _binding.ptr
T, B, L, LENS, MAXPOS = 6, 2, 16, [16, 9], 32
MODELS = {"f32": dict(hidden=96, heads=3, ff=192), "f16x3": dict(hidden=192, heads=6, ff=384)}
INVALID, STATE, UNSUPPORTED = -1, -2, -5
_CACHE = {}


def _model(precision):
    """(product model, finalized handle), built once per precision."""
    if precision not in _CACHE:
        _, _, pm = _pair(layers=2, maxpos=MAXPOS, seed=1, precision=precision, **MODELS[precision])
        _CACHE[precision] = (pm, pm.prepare(beta_schedules.cosine_beta_schedule(T)))
    return _CACHE[precision]


def _i32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _args(Lc=L, Bc=B):
    """The valid arguments of every entry at padded length Lc (host arrays; lens = [Lc, Lc / 2 + 1]; `out` prefilled with -7)."""
    n = max(Bc, 1)
    return dict(x=np.ascontiguousarray(_inputs(n, Lc, seed=2).numpy()), lens=_i32(([Lc, (Lc + 2) // 2] * n)[:n]), t=3, tv=_i32(([3, 0] * n)[:n]),
                z=np.zeros((n, Lc, F), dtype=np.float32), out=np.full((n, Lc, F), -7.0, dtype=np.float32), B=Bc, L=Lc, wrap=1,
                mask=np.ones((n, Lc), dtype=np.uint8), ids=None, fh=0)


def _refused(rc, code, word, out=None):
    msg = _binding.load().fd_last_error()
    assert rc == code and word in msg, (rc, code, word, msg)
    if out is not None:
        assert (out == -7).all(), word


# every entry as a function of the argument dictionary (a None is a null pointer)
def _forward(h, a):
    return _binding.load().fd_forward(h, P(a["x"]), a["t"], P(a["lens"]), a["B"], a["L"], P(a["out"]))


def _forward_t(h, a):
    return _binding.load().fd_forward_t(h, P(a["x"]), P(a["tv"]), P(a["lens"]), a["B"], a["L"], P(a["out"]))


def _forward_ex(h, a):
    return _binding.load().fd_forward_ex(h, P(a["x"]), a["t"], P(a["mask"]), P(a["ids"]), a["B"], a["L"], P(a["out"]))


def _p_sample_step(h, a):
    return _binding.load().fd_p_sample_step(h, P(a["x"]), a["t"], P(a["lens"]), a["B"], a["L"], P(a["z"]), a["wrap"], P(a["out"]))


def _sample_ex(h, a, seed=11):
    return _binding.load().fd_sample_ex(h, P(a["x"]), P(a["lens"]), a["B"], a["L"], a["t"], None, C.c_uint64(seed), C.c_int64(0),
                                        P(a["out"]), a["fh"])


def _edit(key, i, v):
    def apply(a):
        a[key] = a[key].copy()
        a[key][i] = v
    return apply


def _set(**kw):
    return lambda a: a.update(kw)


SHAPE = [(_set(B=0), INVALID, b"must be positive"), (_set(t=T), INVALID, b"timestep %d outside" % T)]
TOO_LONG = (INVALID, b"exceeds max_position_embeddings")
NULLS = lambda *keys: [(_set(**{k: None}), INVALID, b"null argument") for k in keys]   # noqa: E731
LENS_BAD = [(_edit("lens", 1, 0), INVALID, b"lens[1]=0"), (_edit("lens", 1, L + 1), INVALID, b"lens[1]=%d" % (L + 1))]
HOST_ENTRIES = {
    "fd_forward": (_forward, SHAPE + NULLS("x", "lens", "out") + LENS_BAD),
    "fd_forward_t": (_forward_t, [SHAPE[0]] + NULLS("x", "tv", "lens", "out") + LENS_BAD
                     + [(_edit("tv", 1, -1), INVALID, b"t[1]=-1"), (_edit("tv", 0, T), INVALID, b"t[0]=%d" % T)]),
    "fd_p_sample_step": (_p_sample_step, SHAPE + NULLS("x", "lens", "out") + LENS_BAD + [(_set(z=None), INVALID, b"z is required")]),
    "fd_sample_ex": (_sample_ex, SHAPE + NULLS("x", "lens", "out") + LENS_BAD + [(_set(fh=-1), INVALID, b"full_history = -1")]),
}


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("entry", sorted(HOST_ENTRIES))
def test_argument_errors_one_at_a_time(gpu, entry, precision):
    _, h = _model(precision)
    call, cases = HOST_ENTRIES[entry]
    for change, code, word in cases:
        a = _args()
        change(a)
        _refused(call(h, a), code, word, a["out"])
    a = _args(Lc=MAXPOS + 1)                      # L > max_pos
    _refused(call(h, a), *TOO_LONG, a["out"])
    a = _args()                                    # check order: the null output is seen before the bad length
    a["lens"][1] = 0
    a["out"] = None
    _refused(call(h, a), INVALID, b"null argument")
    a = _args()                                    # the same call with nothing wrong
    assert call(h, a) == 0, _binding.load().fd_last_error()
    assert np.isfinite(a["out"][1, :9]).all() and (a["out"][0] != -7).all()


def test_forward_ex_argument_errors(gpu):
    _, h = _model("f16x3")
    cases = SHAPE + NULLS("x", "out") + [(_set(mask=None), INVALID, b"without a mask and without position ids")]
    for change, code, word in cases:
        a = _args()
        change(a)
        _refused(_forward_ex(h, a), code, word, a["out"])
    a = _args(Lc=MAXPOS + 1)
    _refused(_forward_ex(h, a), *TOO_LONG, a["out"])
    a = _args()                                    # check order (the entry takes no lengths): null output before the missing mask
    a.update(out=None, mask=None)
    _refused(_forward_ex(h, a), INVALID, b"null argument")
    _, h32 = _model("f32")                         # an f32 model: unsupported, behind the argument checks
    a = _args()
    _refused(_forward_ex(h32, a), UNSUPPORTED, b"needs FD_PREC_F16X3", a["out"])
    a = _args()
    a["mask"] = None
    _refused(_forward_ex(h32, a), INVALID, b"use fd_forward", a["out"])
    a = _args()
    assert _forward_ex(h, a) == 0, _binding.load().fd_last_error()
    assert (a["out"] != -7).all()


def _dev(a):
    return torch.from_numpy(a).to("cuda:0")


def _begin(h, x, lens, out, Bc=B, Lc=L, t_start=T - 1, fh=0, seed=11):
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    return _binding.load().fd_sample_begin_dev(h, vp(x), vp(lens), Bc, Lc, t_start, C.c_uint64(seed), C.c_int64(0), vp(out), fh, None)


def _steps(h, n, noise=None, t0=0):
    return _binding.load().fd_sample_steps_dev(h, n, None if noise is None else C.c_void_p(noise.data_ptr()), t0, None)


def _end(h, out):
    return _binding.load().fd_sample_end_dev(h, C.c_void_p(out.data_ptr()), None)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_begin_dev_argument_errors(gpu, precision):
    _, h = _model(precision)
    a = _args()
    x, lens = _dev(a["x"]), _dev(a["lens"])
    out = _dev(a["out"])
    untouched = lambda: bool((out == -7).all().item())   # noqa: E731
    for kw, word in [(dict(x=None), b"null argument"), (dict(lens=None), b"null argument"), (dict(out=None), b"null argument"),
                     (dict(Bc=0), b"must be positive"), (dict(t_start=T), b"timestep %d outside" % T),
                     (dict(Lc=MAXPOS + 1), TOO_LONG[1]), (dict(fh=-1), b"full_history = -1")]:
        k = dict(x=x, lens=lens, out=out)
        k.update(kw)
        _refused(_begin(h, **k), INVALID, word)
        assert untouched(), word
    _refused(_begin(h, x, lens, None, fh=-1), INVALID, b"null argument")      # check order: null output before full_history
    assert untouched()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_run_state_machine(gpu, precision):
    _, h = _model(precision)
    lib = _binding.load()
    a = _args()
    x, lens = _dev(a["x"]), _dev(a["lens"])
    out = _dev(a["out"])
    noise = torch.zeros(T, B, L, F, device="cuda:0")

    def plain(hd=None):
        p = _args()
        p["t"] = T - 1
        assert _sample_ex(hd or h, p, seed=5) == 0, lib.fd_last_error()
        return _bits(p["out"])

    def begun(steps=0, then_forward=None):
        """A run begun on the shared model, `steps` of its steps run, then (then_forward = L') an fd_forward at length L'."""
        assert _begin(h, x, lens, out) == 0, lib.fd_last_error()
        assert _steps(h, steps) == 0, lib.fd_last_error()
        if then_forward:
            assert _forward(h, _args(Lc=then_forward)) == 0, lib.fd_last_error()

    want = plain()

    def refused(call, code, word, hd=None):
        """The refusal, then a plain run with the bits it gave before."""
        _refused(call(), code, word)
        assert np.array_equal(plain(hd), want), word

    # no run begun on a finalized model: a new handle (the same weights) before its first call ...
    _, _, fresh = _pair(layers=2, maxpos=MAXPOS, seed=1, precision=precision, **MODELS[precision])
    hf = fresh.prepare(beta_schedules.cosine_beta_schedule(T))
    refused(lambda: _steps(hf, 1), STATE, b"without fd_sample_begin_dev", hf)
    # ... and the shared one, whose last call was a whole run
    refused(lambda: _end(h, out), STATE, b"no sampling run in progress")
    refused(lambda: _steps(h, 1), STATE, b"no sampling run in progress")
    for Lc in (L, 8):                             # another call takes the workspace: at the run's shape, at another shape
        begun(then_forward=Lc)
        refused(lambda: _steps(h, 1), STATE, b"no sampling run in progress")
        begun(then_forward=Lc)
        refused(lambda: _end(h, out), STATE, b"no sampling run in progress")
    begun(steps=2)
    refused(lambda: _end(h, out), STATE, b"have not been run")
    begun(steps=2)
    refused(lambda: _steps(h, T - 1), INVALID, b"n_steps = %d with %d steps left" % (T - 1, T - 2))
    begun(steps=2)
    refused(lambda: _steps(h, -1), INVALID, b"n_steps = -1")
    begun(steps=2)
    refused(lambda: _steps(h, 2, noise, -1), INVALID, b"noise rows start at t = -1")
    begun(steps=2)
    refused(lambda: _steps(h, 2, noise, T - 3), INVALID, b"noise rows start at t = %d" % (T - 3))
    assert lib.fd_synchronize(h) == 0 and bool((out == -7).all().item())      # final state only: `out` is fd_sample_end_dev's
    # a refusal leaves the run itself usable: the same run in pieces, refusals between them, is the one call's bits
    assert _begin(h, x, lens, out, seed=5) == 0, lib.fd_last_error()
    _refused(_end(hf, out), STATE, b"no sampling run in progress")            # (the other handle's last call was a whole run)
    assert _steps(h, 2) == 0
    _refused(_end(h, out), STATE, b"have not been run")
    _refused(_steps(h, T - 1), INVALID, b"n_steps")
    _refused(_steps(h, 2, noise, T - 3), INVALID, b"noise rows")
    assert _steps(h, T - 2) == 0 and _end(h, out) == 0, lib.fd_last_error()
    assert lib.fd_synchronize(h) == 0
    assert np.array_equal(_bits(out.cpu().numpy()), want)
    _refused(_steps(h, 1), STATE, b"no sampling run in progress")             # the run is over


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_plain_runs_around_resampled_runs(gpu, precision):
    _, h = _model(precision)
    lib = _binding.load()
    betas = beta_schedules.cosine_beta_schedule(T)
    coef = sampling.inpaint_levels(betas)
    known, fixed = _masks(LENS, L, rows=(2, 6))
    fx = fixed.astype(bool)
    assert fx[1].any()
    x0 = _args()["x"]
    visits = np.array([5, 4, 3, 4, 3, 2, 1, 0], dtype=np.int32)
    jc = sampling.resample_jump_coef(betas, visits)
    assert jc.shape == (1, 2)

    def plain():
        p = _args()
        p["t"] = T - 1
        assert _sample_ex(h, p, seed=5) == 0, lib.fd_last_error()
        return p["out"]

    before = plain()
    rc, got = _resample(h, x0, LENS, T - 1, known, fixed, coef, visits, jc, 5)
    assert rc == 0, lib.fd_last_error()
    assert np.array_equal(_bits(got)[fx], _bits(known)[fx])
    assert not np.array_equal(got[~fx], before[~fx])                      # the run was conditioned ...
    assert np.array_equal(_bits(plain()), _bits(before))                  # ... and a plain run after it is what it was before
    bad = visits.copy()
    bad[3] = 1                                                            # 3 -> 1: neither the next step down nor a jump up
    rc, out = _resample(h, x0, LENS, T - 1, known, fixed, coef, bad, jc, 5)
    _refused(rc, INVALID, b"visits[3]", out)
    assert np.array_equal(_bits(plain()), _bits(before))
    rc, again = _resample(h, x0, LENS, T - 1, known, fixed, coef, visits, jc, 5)
    assert rc == 0 and np.array_equal(_bits(again), _bits(got))
