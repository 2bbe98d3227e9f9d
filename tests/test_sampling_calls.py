"""The host side of every driver in ``foldingdiff_amd/sampling.py``, pinned call by call: which runner is called with which
arguments, what is drawn from torch's generator in which order, where the drawn arrays end up, which options the model is
given and what comes back.  Every runner is replaced by a stand-in that copies ``x0`` into ``out``; the model is a stub on
the CPU.  ``golden/sampling_calls.json`` was written from this module (``golden/make_golden_sampling_calls.py``) before
the drivers' shared decisions were collected into single functions, and holds no drawn value: drawn arrays are compared
in-process with the logged draws and recorded as "draw j, rows lo..hi"."""
import contextlib
import ctypes
import inspect
import json
import os
import zlib
from unittest import mock

import numpy as np
import pytest
import torch

from foldingdiff_amd import datasets, sampling
from foldingdiff_amd import distributed as fdist

F, T, PAD = 6, 12, 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_calls.json")
RUNNERS = ("_run_fd_sample", "_run_fd_sample_strided", "_run_fd_sample_solver", "_run_fd_inpaint", "_run_fd_inpaint_resample",
           "_run_fd_strided_inpaint", "_run_fd_sample_steered", "_run_fd_sample_repeat")
INT_INPUTS = ("lens", "visits", "event", "tie", "fixed", "grid", "run")   # integer arrays a driver fills in: recorded in full
OFFSET = np.array([0.3, -0.2, 3.0, 1.9, 2.0, 2.1], dtype=np.float32)


class _Model:
    n_inputs = F
    device = torch.device("cpu")

    def __init__(self):
        self.log, self.opts = [], {}

    def prepare(self, betas, is_angle=None):
        self.log.append(["prepare"])
        return 0

    def set_option(self, name, value):
        self.log.append(["set_option", name, int(value)])
        prev, self.opts[name] = self.opts.get(name, 0), int(value)
        return prev


class _Draws:
    """The calls of ``torch.randn``, ``torch.randint`` and ``dset.sample_noise`` in order, with a copy of what each returned."""

    def __init__(self):
        self.made = []

    def logged(self, kind, fn):
        def call(*args, **kwargs):
            got = fn(*args, **kwargs)
            self.made.append((kind, got.detach().clone()))
            return got
        return call

    def origin(self, a: np.ndarray):
        """``[j, lo, hi]``: ``a`` [b, L, F] is the rows lo..hi, cut to L positions, of draw j; "zero"; or None."""
        if not a.any():
            return "zero"
        b, L, _ = a.shape
        for j, (_, d) in enumerate(self.made):
            if d.ndim == 3 and d.dtype == torch.float32 and d.shape[0] >= b and d.shape[1] >= L and d.shape[2] == a.shape[2]:
                for lo in range(d.shape[0] - b + 1):
                    if d[lo: lo + b, :L].contiguous().numpy().tobytes() == a.tobytes():
                        return [j, lo, lo + b]
        return None

    def seed(self, value: int):
        """``{"randint": j}`` for a seed that is the j-th draw, the number itself otherwise."""
        for j, (kind, d) in enumerate(self.made):
            if kind == "randint" and int(d.reshape(-1)[0]) == value:
                return {"randint": j}
        return value


def _describe(name, v, draws):
    if v is None or isinstance(v, (bool, float, str)):
        return v
    if isinstance(v, (int, np.integer)):
        return draws.seed(int(v)) if name == "seed" else int(v)
    if isinstance(v, ctypes.Structure):
        return bytes(v).hex()
    assert isinstance(v, np.ndarray), (name, type(v))
    d = {"shape": list(v.shape), "dtype": str(v.dtype)}
    if name in INT_INPUTS:   # (never an output such as ``ancestors``: those arrive uninitialised)
        assert v.dtype.kind in "iub", (name, v.dtype)
        d["values"] = v.tolist()
    elif name == "x0":
        d["from"] = draws.origin(v)
    elif name == "zs":
        d["from"] = [draws.origin(row) for row in v]
    elif name == "known":   # (float32 subtraction and remainder of the test's own values: the same bits on every CPU)
        d["crc"] = zlib.crc32(np.ascontiguousarray(v).tobytes())
    return d


def _stand_in(name, calls, draws):
    sig = inspect.signature(getattr(sampling, name))

    def run(*args, **kwargs):
        a = sig.bind(*args, **kwargs).arguments
        calls.append({"runner": name, **{k: _describe(k, v, draws) for k, v in a.items() if k != "h"}})
        a["out"][...] = a["x0"]
        for k in ("terms", "logw", "ancestors"):
            if a.get(k) is not None:
                a[k][...] = 0
        if "reward" in a:
            a["reward"][:] = np.arange(len(a["reward"]))     # the last particle of every group is the best
    return run


def _shapes(r):
    if isinstance(r, (torch.Tensor, np.ndarray)):
        return [list(r.shape), str(r.dtype)]
    if isinstance(r, dict):
        return {k: _shapes(v) for k, v in r.items()}
    if isinstance(r, (list, tuple)):
        return [_shapes(v) for v in r]
    return r


def _dset(offset=None):
    return datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=PAD, mean_offset=offset),
                                        timesteps=T, beta_schedule="cosine")


def _record(fn, mode="torch", stream=True, world=None, offset=None, shards=None):
    model, ds, draws, calls = _Model(), _dset(offset), _Draws(), []
    ds.sample_noise = draws.logged("sample_noise", ds.sample_noise)
    with contextlib.ExitStack() as st:
        for name in RUNNERS:
            st.enter_context(mock.patch.object(sampling, name, _stand_in(name, calls, draws)))
        st.enter_context(mock.patch.object(sampling, "NOISE_MODE", mode))
        st.enter_context(mock.patch.object(sampling, "STREAM_NOISE", stream))
        st.enter_context(mock.patch.object(torch, "randn", draws.logged("randn", torch.randn)))
        st.enter_context(mock.patch.object(torch, "randint", draws.logged("randint", torch.randint)))
        if world is not None:
            st.enter_context(mock.patch.object(sampling, "_dist_world", lambda: world))
            st.enter_context(mock.patch.object(fdist, "any_rank_failed", lambda failed, device=None, group=None: failed))
        if shards is not None:
            st.enter_context(mock.patch.object(fdist, "shard_by_tokens", shards))
        torch.manual_seed(7)
        np.random.seed(7)
        returned = fn(model, ds)
    rec = {"calls": calls, "draws": [[kind, list(d.shape)] for kind, d in draws.made], "model": model.log, "returned": _shapes(returned)}
    return json.loads(json.dumps(rec))


def _ramp(*shape):
    """The tests' own float inputs: distinct, never zero, never a draw."""
    return (torch.arange(1, int(np.prod(shape)) + 1, dtype=torch.float32).reshape(shape) % 97 - 48.5) / 20.0


class _Items:
    """Five noised items of lengths 5 .. 9, as ``reconstruct`` reads them."""
    filenames = [f"item{i}" for i in range(5)]

    def __init__(self, ds):
        self.alpha_beta_terms = ds.alpha_beta_terms

    def __len__(self):
        return 5

    def __getitem__(self, idx, use_t_val=None):
        return {"corrupted": _ramp(PAD, F) + idx, "lengths": 5 + idx, "angles": _ramp(PAD, F) - idx}


def _known_fixed():
    known = [np.asarray(_ramp(l, F)) + np.float32(0.25 * i) for i, l in enumerate((5, 6, 7, 8, 9, 7))]
    fixed = [np.arange(len(k)) % 3 == 1 for k in known]
    fixed[2] = np.asarray(_ramp(7, F)) > 0          # an element mask
    return known, fixed


def _scenarios():
    S = {}
    lengths = [5, 9, 6, 8, 7, 7]
    few = dict(num_steps=5, solver="dpm2m", spacing="logsnr", history_every=2)
    sample_kw = {"full": dict(), "k5_eta0_final": dict(num_steps=5, eta=0.0, final_only=True), "k5_eta1": dict(num_steps=5, eta=1.0),
                 "dpm2m": dict(few, final_only=False), "dpm2m_final": dict(few, final_only=True)}
    for mode in ("torch", "philox"):
        for name, kw in sample_kw.items():
            S[f"sample/{name}/{mode}"] = (lambda m, ds, kw=kw: sampling.sample(m, ds, n=2, sweep_lengths=(5, 8), batch_size=4, **kw), dict(mode=mode))
        for rank in (0, 1):   # the second batch is one item: its first shard is empty
            for name in ("full", "k5_eta1", "dpm2m"):
                S[f"sample2/{name}/{mode}/rank{rank}"] = (
                    lambda m, ds, kw=sample_kw[name]: sampling.sample(m, ds, n=1, sweep_lengths=(5, 10), batch_size=4, gather="none", **kw),
                    dict(mode=mode, world=(2, rank)))
        whole = fdist.shard_by_tokens
        for name in ("full", "k5_eta1"):   # ... and here its second shard
            S[f"sample2/{name}/{mode}/rank1_empty_second"] = (
                lambda m, ds, kw=sample_kw[name]: sampling.sample(m, ds, n=1, sweep_lengths=(5, 10), batch_size=4, gather="none", **kw),
                dict(mode=mode, world=(2, 1), shards=lambda lens, w: [(0, 1), (1, 1)] if len(lens) == 1 else whole(lens, w)))
    betas = lambda ds: ds.alpha_beta_terms["betas"]   # noqa: E731
    loop = lambda m, ds, **kw: sampling.p_sample_loop(m, [6, 9], _ramp(2, 9, F), T, betas(ds), is_angle=[True] * F, **kw)   # noqa: E731
    for stream in (True, False):
        s = f"stream{int(stream)}"
        S[f"loop/step_noise/{s}"] = (lambda m, ds: loop(m, ds, step_noise=np.asarray(_ramp(T, 2, 9, F)), history_every=5), dict(stream=stream))
        S[f"loop/seed/{s}"] = (lambda m, ds: loop(m, ds, seed=1234, seq_offset=3, final_only=True), dict(stream=stream))
        S[f"loop/draw_batch/{s}"] = (lambda m, ds: loop(m, ds, draw_batch=(4, 1, 3), seq_offset=1), dict(stream=stream))
        S[f"loop/draw_batch_k4/{s}"] = (lambda m, ds: loop(m, ds, draw_batch=(4, 1, 3), num_steps=4, eta=1.0), dict(stream=stream))
    few_step = {"plain": dict(), "strided": dict(num_steps=3, eta=0.5), "dpm2m": dict(num_steps=3, solver="dpm2m", spacing="logsnr", lambda_min=-2.0)}
    for mode in ("torch", "philox"):
        for name, kw in few_step.items():
            S[f"reverse_from/{name}/{mode}"] = (lambda m, ds, kw=kw: sampling.reverse_from(m, _ramp(2, 9, F), [9, 5], 6, betas(ds), **kw), dict(mode=mode))
            S[f"reconstruct/{name}/{mode}"] = (lambda m, ds, kw=kw: sampling.reconstruct(m, _Items(ds), noise_timesteps=7, bs=3, **kw), dict(mode=mode))
    known, fixed = _known_fixed()
    inpaint_kw = {"plain": dict(final_only=False, t_start=8), "resampled": dict(jump_length=3, n_resample=2),
                  "strided": dict(num_steps=4, eta=0.5, final_only=False), "strided_resampled": dict(num_steps=5, jump_length=2, n_resample=2)}
    for name, kw in inpaint_kw.items():
        for off in (None, OFFSET):
            S[f"inpaint/{name}/{'offset' if off is not None else 'no_offset'}"] = (
                lambda m, ds, kw=kw: sampling.inpaint(m, ds, known, fixed, batch_size=4, **kw), dict(offset=off))
    motif = np.asarray(_ramp(3, F))
    S["scaffold/centred"] = (lambda m, ds: sampling.scaffold(m, ds, motif, [5, 7, 9], batch_size=2), dict(offset=OFFSET))
    S["scaffold/random_strided"] = (lambda m, ds: sampling.scaffold(m, ds, motif, [5, 7, 9], offsets="random", pin_lead_angle=False, batch_size=2,
                                                                    num_steps=4, jump_length=1, n_resample=3), {})
    for select in ("best", "all"):
        S[f"steer/{select}"] = (lambda m, ds, select=select: sampling.steer(m, ds, lengths[:3], n_particles=4, select=select, num_steps=6,
                                                                            batch_size=8, reward={"clashes": -1.0, "rg": 0.5}), dict(offset=OFFSET))
    S["steer/seed_all_steps"] = (lambda m, ds: sampling.steer(m, ds, lengths[:2], n_particles=4, seed=11, batch_size=4, every=2), {})
    S["repeats/k5"] = (lambda m, ds: sampling.sample_repeats(m, ds, lengths, [2, 3, 2, 2, 3, 1], 2, [0, 1, 1, 2, 0, 3], num_steps=5, batch_size=4),
                       dict(offset=OFFSET))
    S["repeats/all_steps_logsnr"] = (lambda m, ds: sampling.sample_repeats(m, ds, lengths[:3], 2, 2, eta=0.5, spacing="logsnr", num_steps=4), {})
    return S


SCENARIOS = _scenarios()


def record_all():
    return {name: _record(fn, **kw) for name, (fn, kw) in SCENARIOS.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_has_exactly_these_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_driver_makes_the_calls_it_made(golden, name):
    fn, kw = SCENARIOS[name]
    got, want = _record(fn, **kw), golden[name]
    assert got["draws"] == want["draws"]
    assert got["model"] == want["model"]
    assert len(got["calls"]) == len(want["calls"])
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got["returned"] == want["returned"]


def test_stream_noise_does_not_change_a_cpu_run(golden):
    for name in golden:
        if name.startswith("loop/") and name.endswith("/stream1"):
            assert golden[name] == golden[name[:-1] + "0"], name


def test_every_drawn_array_was_traced(golden):
    """No x0 or zs of a driver that draws its own is of unknown origin; the arrays the tests hand in are."""
    for name, rec in golden.items():
        own_input = name.startswith(("loop/", "reverse_from/", "reconstruct/"))
        for c in rec["calls"]:
            assert (c["x0"]["from"] is None) == own_input, name
            if isinstance(c.get("zs"), dict):
                assert (None in c["zs"]["from"]) == name.startswith("loop/step_noise"), name
