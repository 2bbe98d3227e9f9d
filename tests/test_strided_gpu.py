"""Few-step sampling on a strided schedule on the device (fd_sample_strided, fd_sample_strided_dev, fd_p_sample_step_coef,
sampling.sample(num_steps=...)) against the float32 statement of tests/strided_reference.py: the update BIT FOR BIT, the
network's prediction and the free-running loop with the tolerances of the plain sampler's tests (tests/test_gpu_parity.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import strided_reference as sref
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling
from oracle import ref_philox
from test_gpu_parity import FWD_TOL, PRECISIONS, STEP_TOL, _c1_models, _free_running_check, _inputs, _pair, _record, _share_time_table
from test_inpaint_gpu import _masks, _sample_inpaint, _sample_plain

pytestmark = pytest.mark.gpu
F = 6
ANG = [True] * F
P = _binding.ptr
SENTINEL = -7.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _valid(lens, L):
    v = np.zeros((len(lens), L, F), dtype=bool)
    for b, n in enumerate(lens):
        v[b, :n] = True
    return v


def _step_coef(h, x, t, lens, a, b, s, z, wrap=1):
    """fd_p_sample_step_coef -> (rc, eps_out, x_out); both outputs start at the sentinel."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    zs = None if z is None else np.ascontiguousarray(z, dtype=np.float32)
    eps, out = np.full_like(xs, SENTINEL), np.full_like(xs, SENTINEL)
    rc = _binding.load().fd_p_sample_step_coef(h, P(xs), int(t), P(ls), B, L, float(a), float(b), float(s), P(zs), wrap, P(eps), P(out))
    return rc, eps, out


def _forward(h, x, t, lens):
    xs = np.ascontiguousarray(x, dtype=np.float32)
    B, L, _ = xs.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    eps = np.empty_like(xs)
    _binding.check(_binding.load().fd_forward(h, P(xs), int(t), P(ls), B, L, P(eps)))
    return eps


def _rows(K, full_history):
    return -(-K // full_history) if full_history else 1


def _strided(h, x0, lens, visits, coef, seed, full_history, noise=None, seq_offset=0, n_visits=None):
    """fd_sample_strided -> (rc, out); `out` starts at the sentinel."""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, L, _ = x0.shape
    ls = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    vs = None if visits is None else np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    K = n_visits if n_visits is not None else len(vs)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float32)
    zs = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    out = np.full((_rows(max(K, 1), full_history), B, L, F), SENTINEL, dtype=np.float32)
    rc = _binding.load().fd_sample_strided(h, P(x0), P(ls), B, L, P(vs), K, P(cf), P(zs), C.c_uint64(seed), C.c_int64(seq_offset),
                                           P(out), full_history)
    return rc, out


def _strided_dev(h, x0, lens, visits, coef, seed, full_history, noise=None):
    """fd_sample_strided_dev on device copies -> (rc, out on the host)."""
    dev = "cuda:0"
    x_d = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).to(dev)
    B, L, _ = x_d.shape
    l_d = torch.tensor([int(n) for n in lens], dtype=torch.int32, device=dev)
    z_d = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(dev)
    vs = np.ascontiguousarray(np.asarray(visits, dtype=np.int32))
    cf = np.ascontiguousarray(coef, dtype=np.float32)
    out_d = torch.full((_rows(len(vs), full_history), B, L, F), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = _binding.load().fd_sample_strided_dev(h, C.c_void_p(x_d.data_ptr()), C.c_void_p(l_d.data_ptr()), B, L, P(vs), len(vs), P(cf),
                                               C.c_void_p(z_d.data_ptr()) if z_d is not None else None, C.c_uint64(seed), C.c_int64(0),
                                               C.c_void_p(out_d.data_ptr()), full_history, None)
    return rc, out_d.cpu().numpy()


def _device_draws(h, seed, t, B, L):
    """The device's own Philox draws of step word t (what the update kernels draw inside a run)."""
    out = torch.empty(B, L, F, device="cuda:0")
    _binding.check(_binding.load().fd_philox_normal_dev(h, C.c_uint64(seed), int(t), C.c_int64(0), B, L, C.c_void_p(out.data_ptr()), None))
    _binding.check(_binding.load().fd_synchronize(h))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------- 1. the three update kernels
@pytest.mark.parametrize("precision,hidden,heads", [("f16x3", 192, 6), ("f16x3", 384, 12), ("f32", 128, 4), ("f32", 96, 3)])
def test_update_statement_bit_for_bit_in_every_update_kernel(gpu, precision, hidden, heads):
    """The row-image kernel (f16x3), the 16-lanes-per-token kernel (f32, d % 64 == 0) and the one-wave-per-token kernel
    (f32, d = 96).  One-layer models, L = 24, B = 3, T = 8, ragged lengths, visits 7, 4, 2, 0.  x_out carries the bits of
    the float32 statement applied to the hook's own eps_out; eps_out carries fd_forward's bits and is within FWD_TOL of
    the oracle's forward.  No tolerance of its own."""
    o32, _, pm = _pair(hidden=hidden, heads=heads, ff=2 * hidden, layers=1, maxpos=32, seed=3, precision=precision)
    T, lens, visits = 8, [24, 17, 9], np.array([7, 4, 2, 0], dtype=np.int32)
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    ok = _valid(lens, 24)
    g = torch.Generator().manual_seed(29)
    worst = 0.0
    for eta in (0.0, 0.5):
        coef = sampling.ddim_coefficients(betas, visits, eta)
        assert np.array_equal(_bits(coef), _bits(sref.coefficients(betas, visits, eta)))
        for wrap in (0, 1):
            x = _inputs(3, 24, seed=5).numpy()
            for i, t in enumerate(visits):
                a, b, s = coef[:, i]
                z = torch.randn(3, 24, F, generator=g).numpy()
                rc, eps, out = _step_coef(h, x, t, lens, a, b, s, None if s == 0 else z, wrap)
                assert rc == 0, _binding.load().fd_last_error()
                want = sref.update(x, eps, a, b, s, z, ANG if wrap else [False] * F)
                assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), (eta, wrap, i)
                assert np.array_equal(_bits(eps)[ok], _bits(_forward(h, x, t, lens))[ok]), (eta, wrap, i)
                e = float(np.abs(eps - sref.forward(o32, x, t, lens).numpy())[ok].max())
                worst = max(worst, e)
                assert e <= FWD_TOL, (eta, wrap, i, e)
                if wrap:
                    assert (np.abs(out[ok]) <= np.float32(np.pi)).all()
                x = np.where(ok, want, x).astype(np.float32)
    # coefficients from no table at all: three arbitrary finite floats, with and without a draw
    x = _inputs(3, 24, seed=6).numpy()
    z = torch.randn(3, 24, F, generator=g).numpy()
    for a, b, s in [(1.7, -0.9, 0.3), (-0.25, 3.5, 0.0), (1e-3, 2.0 ** -20, -1.5)]:
        for wrap in (0, 1):
            rc, eps, out = _step_coef(h, x, 5, lens, a, b, s, None if s == 0 else z, wrap)
            assert rc == 0, _binding.load().fd_last_error()
            want = sref.update(x, eps, a, b, s, z, ANG if wrap else [False] * F)
            assert np.array_equal(_bits(out)[ok], _bits(want)[ok]), (a, b, s, wrap)
    _record(f"strided_hook_d{hidden}_{precision}", max_eps=worst)


# ---------------------------------------------------------------------------------- 2. the loop is the chain of hooks
C1_LENS = [64, 50, 33, 20]
SETTINGS = [([9, 6, 3, 0], 0.5), ([8, 5, 2, 0], 0.5), ([9, 7, 4, 2, 0], 0.5), ([9, 6, 3, 0], 0.0)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_equals_the_chain_of_hooks_bit_for_bit(gpu, precision):
    """C1 (d = 192, 6 layers, L = 64, B = 4, T = 10).  Row i of the full history is the hook applied to row i - 1 (row -1 =
    x_init) with visit i's coefficients and draws, bit for bit: the table lookup by timestep, the advance through next_t,
    the noise row and the history ordinal.  With an explicit noise array z is its row i.  With Philox the kernel draws with
    the plain sampler's key (seed, t): the hook is fed the device generator's own draws of step word t -- the bits the kernel
    drew -- and those draws are within 2e-5 of ref_philox.philox_normal(seed, t, ...), the bound tests/test_gpu_parity.py
    sets between the device's logf / sincosf and numpy's (ref_philox's values themselves cannot give the kernel's bits).
    The thinned history, the final-only run, eager launches, packed rows and the device entry give the same bits below
    the lengths."""
    g, _, _, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    B, L = 4, 64
    x0 = g["x0"]
    ok = _valid(C1_LENS, L)
    seed = 977
    for visits, eta in SETTINGS:
        K = len(visits)
        coef = sampling.ddim_coefficients(betas, np.asarray(visits, dtype=np.int32), eta)
        explicit = torch.randn(K, B, L, F, generator=torch.Generator().manual_seed(31)).numpy()
        for noise in (explicit, None):
            rc, full = _strided(h, x0, C1_LENS, visits, coef, seed, 1, noise=noise)
            assert rc == 0, _binding.load().fd_last_error()
            assert full.shape == (K, B, L, F) and np.isfinite(full[:, ok]).all()
            prev = x0
            for i, t in enumerate(visits):
                a, b, s = coef[:, i]
                if s == 0:
                    z = None
                elif noise is not None:
                    z = noise[i]
                else:
                    z = _device_draws(h, seed, t, B, L)
                    assert np.abs(z - ref_philox.philox_normal(seed, int(t), 0, B, L, F)).max() < 2e-5, (visits, i)
                rc, _, want = _step_coef(h, prev, t, C1_LENS, a, b, s, z)
                assert rc == 0, _binding.load().fd_last_error()
                assert np.array_equal(_bits(full[i])[ok], _bits(want)[ok]), (visits, eta, noise is None, i)
                prev = full[i]
            rc, final = _strided(h, x0, C1_LENS, visits, coef, seed, 0, noise=noise)
            assert rc == 0 and np.array_equal(_bits(final[0])[ok], _bits(full[-1])[ok])
            rc, every2 = _strided(h, x0, C1_LENS, visits, coef, seed, 2, noise=noise)
            states = [1, 3] if K == 4 else [1, 3, 4]
            assert rc == 0 and every2.shape[0] == len(states)
            assert np.array_equal(_bits(every2)[:, ok], _bits(full[states])[:, ok]), (visits, states)
            pm.set_option("use_graph", 0)
            rc, eager = _strided(h, x0, C1_LENS, visits, coef, seed, 1, noise=noise)
            pm.set_option("use_graph", 1)
            assert rc == 0 and np.array_equal(_bits(eager)[:, ok], _bits(full)[:, ok]), (visits, "eager")
            pm.set_option("varlen", 1)
            rc, packed = _strided(h, x0, C1_LENS, visits, coef, seed, 1, noise=noise)
            pm.set_option("varlen", 0)
            assert rc == 0 and np.array_equal(_bits(packed)[:, ok], _bits(full)[:, ok]), (visits, "varlen")
            if precision == "f16x3":                 # packed rows (the row-image path): the history's padding is zeroed, as in fd_sample
                assert (packed[:, ~ok] == 0).all()
            rc, dev = _strided_dev(h, x0, C1_LENS, visits, coef, seed, 1, noise=noise)
            assert rc == 0 and np.array_equal(_bits(dev)[:, ok], _bits(full)[:, ok]), (visits, "dev")
            if noise is None and eta > 0:
                rc, other = _strided(h, x0, C1_LENS, visits, coef, seed + 1, 1)
                assert rc == 0 and not np.array_equal(other[:, ok], full[:, ok])       # the seed matters where something is drawn
        if eta == 0.0:   # no draw anywhere: the seed cannot matter, and no noise array is needed
            rc, a_ = _strided(h, x0, C1_LENS, visits, coef, 1, 1)
            rc2, b_ = _strided(h, x0, C1_LENS, visits, coef, 2, 1)
            assert rc == 0 and rc2 == 0 and np.array_equal(_bits(a_), _bits(b_))


# ---------------------------------------------------------------------------------- 3. against the oracle, free-running
FREE_VISITS = np.array([8, 5, 2, 0], dtype=np.int32)   # every |b| <= 3.6: below the plain sampler's worst coefficient (1.0e2), under which STEP_TOL was set
FREE_SEED = 20240917   # the draws' seed, chosen on the CPU: the oracle's own fp32 and fp64 loops satisfy the check (asserted below)
_FREE_REF = {}


def _free_reference(o32, o64, x0, betas, T, eta):
    """The restatement's loop with the fp32 and the fp64 oracle on explicit draws; computed once, shared by the precisions."""
    if eta not in _FREE_REF:
        coef = sampling.ddim_coefficients(betas, FREE_VISITS, eta)
        assert np.abs(coef[1]).max() <= 3.6
        z = torch.randn(len(FREE_VISITS), 4, 64, F, generator=torch.Generator().manual_seed(FREE_SEED)).numpy()
        _share_time_table(o64, o32, T)
        _FREE_REF[eta] = (coef, z, sref.loop(o32, C1_LENS, x0, FREE_VISITS, coef, ANG, z), sref.loop(o64, C1_LENS, x0, FREE_VISITS, coef, ANG, z))
    return _FREE_REF[eta]


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_free_running_c1_against_the_oracle(gpu, precision, eta):
    g, o32, o64, pm = _c1_models(precision)
    T = int(g["T"])
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    coef, z, want32, want64 = _free_reference(o32, o64, g["x0"], betas, T, eta)
    ok = _valid(C1_LENS, 64)
    sel = lambda a: np.where(ok, a, 0.0)   # noqa: E731  (positions beyond a length are nobody's result)
    # the condition on the start and the draws: the oracle's own two precisions stay together
    _free_running_check(f"strided_free_c1_oracle32_vs_64_eta{eta}", sel(want32), sel(want64))
    rc, got = _strided(h, g["x0"], C1_LENS, FREE_VISITS, coef, 0, 1, noise=z)
    assert rc == 0, _binding.load().fd_last_error()
    _free_running_check(f"strided_free_c1_{precision}_eta{eta}", sel(got), sel(want32), tol=STEP_TOL)


# ---------------------------------------------------------------------------------- 4. the contract
def test_argument_errors_leave_the_output_alone_and_later_runs_are_unaffected(gpu):
    _, _, pm = _pair(hidden=192, heads=6, ff=384, layers=2, maxpos=128, seed=7, precision="f16x3")
    T = 12
    betas = beta_schedules.cosine_beta_schedule(T)
    h = pm.prepare(betas)
    lib = _binding.load()
    lens = [50, 33, 64, 12]
    x0 = _inputs(4, 64, seed=4).numpy()
    visits = np.array([11, 7, 3, 0], dtype=np.int32)
    coef = sampling.ddim_coefficients(betas, visits, 0.5)
    known, fixed = _masks(lens, 64)
    kcoef = sampling.inpaint_levels(betas)
    before = _sample_plain(h, x0, lens, T - 1, 5, 1)
    rc, before_inpaint = _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, 5, 1)
    assert rc == 0
    nan_coef, inf_coef = coef.copy(), coef.copy()
    nan_coef[1, 2] = np.nan
    inf_coef[2, 0] = np.inf
    bad = [(dict(visits=None, n_visits=4), b"visits is null"),
           (dict(coef=None), b"coef is null"),
           (dict(n_visits=0), b"n_visits = 0"),
           (dict(visits=[12, 7, 3, 0]), b"visits[0] = 12 outside"),
           (dict(visits=[11, 7, -1, 0]), b"visits[2] = -1 outside"),
           (dict(visits=[11, 7, 7, 0]), b"visits[2] = 7 follows 7"),
           (dict(visits=[11, 3, 7, 0]), b"visits[2] = 7 follows 3"),
           (dict(coef=nan_coef), b"coef[1][2]"),
           (dict(coef=inf_coef), b"coef[2][0]")]
    for kw, word in bad:
        a = dict(visits=visits, coef=coef, n_visits=None)
        a.update(kw)
        rc, out = _strided(h, x0, lens, a["visits"], a["coef"], 5, 1, n_visits=a["n_visits"])
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all(), word
        after = _sample_plain(h, x0, lens, T - 1, 5, 1)        # a rejected call changes nothing
        assert np.array_equal(_bits(after), _bits(before)), word
    z = np.zeros((4, 64, F), dtype=np.float32)
    for (a, b, s, zz), word in [((1.0, -1.0, 0.5, None), b"z is required"), ((np.nan, -1.0, 0.0, z), b"not finite"),
                                ((1.0, np.inf, 0.0, z), b"not finite"), ((1.0, -1.0, -np.inf, z), b"not finite")]:
        rc, eps, out = _step_coef(h, x0, 3, lens, a, b, s, zz)
        assert rc == -1 and word in lib.fd_last_error(), (word, rc, lib.fd_last_error())
        assert (out == SENTINEL).all() and (eps == SENTINEL).all()
    rc, eps, out = _step_coef(h, x0, T, lens, 1.0, -1.0, 0.0, None)           # the timestep is checked like fd_p_sample_step's
    assert rc == -1 and (out == SENTINEL).all()
    # a valid strided run, both noise sources and the device entry; then the plain and the conditioned sampler are what they were
    rc, run = _strided(h, x0, lens, visits, coef, 5, 1)
    assert rc == 0 and np.isfinite(run[:, _valid(lens, 64)]).all(), lib.fd_last_error()
    assert not np.array_equal(run[-1], before[-1])
    rc, _ = _strided_dev(h, x0, lens, visits, coef, 5, 0)
    assert rc == 0
    after = _sample_plain(h, x0, lens, T - 1, 5, 1)
    assert np.array_equal(_bits(after), _bits(before))
    rc, after_inpaint = _sample_inpaint(h, x0, lens, T - 1, known, fixed, kcoef, 5, 1)
    assert rc == 0 and np.array_equal(_bits(after_inpaint), _bits(before_inpaint))
    rc, again = _strided(h, x0, lens, visits, coef, 5, 1)                     # ... and the strided run after them too
    assert rc == 0 and np.array_equal(_bits(again), _bits(run))


# ---------------------------------------------------------------------------------- 5. Python end to end
def test_sample_end_to_end_on_a_tiny_model(gpu, monkeypatch):
    _, _, pm = _pair(seed=11, precision="f16x3")
    T = 20
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64), timesteps=T, beta_schedule="cosine")
    results = {}
    for mode in ("philox", "torch"):
        monkeypatch.setattr(sampling, "NOISE_MODE", mode)
        for eta in (0.0, 1.0):
            runs = []
            for _ in range(2):
                torch.manual_seed(3)
                runs.append(sampling.sample(pm, ds, n=2, sweep_lengths=(30, 33), final_only=False, num_steps=5, eta=eta))
            assert [s.shape for s in runs[0]] == [(5, l, F) for l in (30, 30, 31, 31, 32, 32)]
            for s0, s1 in zip(*runs):
                assert np.array_equal(_bits(s0), _bits(s1))                          # reproducible under the same seed
                assert np.isfinite(s0).all() and (s0 >= -np.float32(np.pi)).all() and (s0 < np.float32(np.pi)).all()
            results[mode, eta] = runs[0]
        assert not np.array_equal(results[mode, 0.0][0], results[mode, 1.0][0])      # eta matters
    # eta = 0 draws nothing: a deterministic map of the start noise, whatever the noise mode (the Philox seed is drawn behind
    # the batch's start noise and nothing reads it)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(results["philox", 0.0], results["torch", 0.0]))
    assert not np.array_equal(results["philox", 1.0][0], results["torch", 1.0][0])
    torch.manual_seed(3)
    fin = sampling.sample(pm, ds, n=2, sweep_lengths=(30, 33), final_only=True, num_steps=5, eta=0.0)
    assert [s.shape for s in fin] == [(1, l, F) for l in (30, 30, 31, 31, 32, 32)]
    assert all(np.array_equal(_bits(a[0]), _bits(b[-1])) for a, b in zip(fin, results["torch", 0.0]))
    # reverse_from starts its schedule at t_start: the same states as the C entry on visits 6, 3, 0
    monkeypatch.setattr(sampling, "NOISE_MODE", "philox")
    betas = ds.alpha_beta_terms["betas"]
    x = _inputs(2, 40, seed=8)
    got = sampling.reverse_from(pm, x, [40, 25], 6, betas, is_angle=True, num_steps=3, eta=0.0).numpy()
    visits = sampling.ddim_visits(T, 3, 6)
    assert visits.tolist() == [6, 3, 0]
    h = pm.prepare(betas, True)
    rc, want = _strided(h, x.numpy(), [40, 25], visits, sampling.ddim_coefficients(betas, visits, 0.0), 0, 0)
    assert rc == 0 and np.array_equal(_bits(got)[_valid([40, 25], 40)], _bits(want[0])[_valid([40, 25], 40)])
    # the device-resident entry of the package
    x_d = x.to("cuda:0")
    l_d = torch.tensor([40, 25], dtype=torch.int32, device="cuda:0")
    out_d = sampling.sample_on_device(pm, x_d, l_d, betas, is_angle=True, t_start=6, num_steps=3, eta=0.0, full_history=True)
    assert tuple(out_d.shape) == (3, 2, 40, F) and np.array_equal(_bits(out_d[-1].cpu().numpy())[_valid([40, 25], 40)], _bits(got)[_valid([40, 25], 40)])
