"""Steering by particle resampling, the parts that need no device: the numpy restatement's own properties
(tests/steer_reference.py), the schedule helpers of ``sampling``, the Python argument errors, the header and the binding,
and the argument checks of the two model-free entries (every one made before the first HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import steer_reference as st
from conftest import REPO
from foldingdiff_amd import _binding, beta_schedules, datasets, sampling, structures

P = _binding.ptr
ENTRIES = ("fd_sample_steered", "fd_p_sample_step_coef_x0", "fd_steer_rewards", "fd_steer_resample")


# ---------------------------------------------------------------------------------- the resampling statement
@pytest.mark.parametrize("P_", [1, 2, 5, 64])
def test_equal_weights_resample_to_the_identity(P_):
    for u in (0.0, 0.25, 0.5, 0.999):
        for G in (1, 3):
            n = G * P_
            logw, r_prev, anc, flags, margin = st.resample(np.full(n, 2.5), np.zeros(n), np.full(n, 2.5), P_, 1.7, 1.0, [u] * G)
            assert np.array_equal(anc, np.arange(n)) and flags.all()
            assert margin > 1e-9 or u == 0.0   # (u = 0 puts every target on a cumulative sum: the strict > decides)
            assert (logw == 0).all() and (r_prev == 2.5).all()
            # ess_frac below 1: ESS = P, nothing is resampled, the weights stay
            logw, _, anc, flags, _ = st.resample(np.full(n, 2.5), np.full(n, 0.125), np.full(n, 2.5), P_, 1.7, 0.5, [u] * G)
            assert np.array_equal(anc, np.arange(n)) and not flags.any() and (logw == 0.125).all()


def test_one_dominant_particle_becomes_every_ancestor():
    for P_, who in ((2, 1), (5, 2), (64, 63), (65, 0)):
        reward = np.zeros(2 * P_)
        reward[who] = 80.0            # group 0: exp(-80) of the others is far below any target's distance
        reward[P_:] = np.linspace(0, 1e-3, P_)
        logw, r_prev, anc, flags, _ = st.resample(reward, np.zeros(2 * P_), np.zeros(2 * P_), P_, 1.0, 0.9, [0.37, 0.37])
        assert (anc[:P_] == who).all() and flags[0] == 1 and (r_prev[:P_] == 80.0).all() and (logw[:P_] == 0).all()
        assert np.array_equal(anc[P_:], P_ + np.arange(P_)) and flags[1] == 0   # the flat group keeps its particles


def test_without_resampling_the_log_weights_telescope():
    """ess_frac = 0 never resamples; after any number of events logw = lambda * (the latest reward), up to the rounding of
    the differences it was summed from."""
    rng = np.random.default_rng(3)
    P_, G, lam = 5, 3, 0.75
    logw, r_prev = np.zeros(G * P_), np.zeros(G * P_)
    for _ in range(7):
        reward = rng.normal(0, 3, G * P_)
        logw, r_prev, anc, flags, _ = st.resample(reward, logw, r_prev, P_, lam, 0.0, rng.random(G))
        assert np.array_equal(anc, np.arange(G * P_)) and not flags.any() and np.array_equal(r_prev, reward)
    assert np.allclose(logw, lam * reward, rtol=0, atol=1e-13)


def test_a_single_particle_is_its_own_ancestor():
    logw, r_prev, anc, flags, _ = st.resample(np.array([3.0, -1.0]), np.zeros(2), np.zeros(2), 1, 2.0, 1.0, [0.0, 0.99])
    assert np.array_equal(anc, [0, 1]) and flags.all() and (logw == 0).all() and np.array_equal(r_prev, [3.0, -1.0])


def test_weights_that_are_not_usable_never_resample():
    logw, _, anc, flags, _ = st.resample(np.array([np.nan, 1.0, 2.0]), np.zeros(3), np.zeros(3), 3, 1.0, 1.0, [0.5])
    assert np.array_equal(anc, [0, 1, 2]) and not flags.any() and np.isnan(logw[0])


def test_systematic_resampling_follows_the_weights():
    """Weights 0.5, 1, 0.5 (W = 2, cumsums 0.5, 1.5, 2) and u = 0.5: targets 0.33, 1, 1.67; u = 0.9: 0.6, 1.27, 1.93."""
    reward = np.log(np.array([1.0, 2.0, 1.0]))
    _, r_prev, anc, flags, margin = st.resample(reward, np.zeros(3), np.zeros(3), 3, 1.0, 1.0, [0.5])
    assert np.array_equal(anc, [0, 1, 2]) and flags[0] == 1
    _, r_prev, anc, _, _ = st.resample(reward, np.zeros(3), np.zeros(3), 3, 1.0, 1.0, [0.9])
    assert np.array_equal(anc, [1, 1, 2]) and np.array_equal(r_prev, reward[[1, 1, 2]])


def test_reward_terms_of_the_reference_on_known_chains():
    rng = np.random.default_rng(1)
    idx = [0, 1, 2, 3, 4, 5, -1, -1, -1]
    helix = st.chain_terms(st.backbone(st.angles_of("helix", 40, rng), idx), 0.63)
    strand = st.chain_terms(st.backbone(st.angles_of("extended", 40, rng), idx), 0.63)
    coil = st.chain_terms(st.backbone(st.angles_of("random", 100, rng), idx), 0.63)
    assert helix[2] > 0.8 and helix[3] == 0 and helix[0] == 0
    assert strand[3] > 0.8 and strand[2] == 0 and strand[1] > 2 * helix[1]   # an extended chain is far less compact
    assert coil[0] > 0
    assert st.weighted([1.0, 0.5, -2.0, 3.0], [4.0, 2.0, 0.25, 1.0]) == 4.0 + 1.0 - 0.5 + 3.0
    # the shift: float32 sum, wrapped where angular; no offset: the values themselves
    x = np.array([[[3.0, 1.0]]], dtype=np.float32)
    got = st.shift(x, np.array([0.5, 0.5], np.float32), [True, False])
    assert got[0, 0, 1] == np.float32(1.5) and abs(got[0, 0, 0] - (3.5 - 2 * np.pi)) < 1e-6
    assert np.array_equal(st.shift(x, None, [True, False]), x)


# ---------------------------------------------------------------------------------- the schedule helpers
def test_steer_events_and_coefficients():
    T = 20
    betas = beta_schedules.cosine_beta_schedule(T)
    visits = sampling.ddim_visits(T, 8)          # 19, 16, 14, 11, 8, 5, 3, 0
    assert visits.tolist() == [19, 16, 14, 11, 8, 5, 3, 0]
    ev = sampling.steer_events(visits, 10, 1)
    assert ev.dtype == np.uint8 and ev.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert sampling.steer_events(visits, 10, 2).tolist() == [0, 0, 0, 0, 0, 1, 0, 1]
    assert sampling.steer_events(visits, 10, 3).tolist() == [0, 0, 0, 0, 0, 0, 1, 1]   # the last visit is always one
    assert sampling.steer_events(visits, 10, 9).tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert sampling.steer_events(visits, 0, 1).tolist() == [0] * 8                     # nothing below t = 0: no event at all
    assert sampling.steer_events(visits, T, 1).tolist() == [1] * 8
    with pytest.raises(ValueError):
        sampling.steer_events(visits, 10, 0)
    for eta in (1.0, 0.3):
        coef = sampling.steer_coefficients(betas, visits, eta)
        assert coef.dtype == np.float32 and coef.shape == (5, 8) and coef.flags["C_CONTIGUOUS"]
        assert np.array_equal(coef[:3].view(np.uint32), sampling.ddim_coefficients(betas, visits, eta).view(np.uint32))
        assert np.array_equal(coef[3:].view(np.uint32), sampling.solver_coefficients(betas, visits)[3:].view(np.uint32))
        assert (coef[2, :-1] != 0).all()
    assert sampling.reward_weights(None).tolist() == [-1.0, 0.0, 0.0, 0.0]
    assert sampling.reward_weights({"strand": 2, "rg": -0.5}).tolist() == [0.0, -0.5, 0.0, 2.0]


def test_python_argument_errors():
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=64), timesteps=20, beta_schedule="cosine")
    bad = [dict(select="first"), dict(spacing="cosine"), dict(n_particles=0), dict(n_particles=1025), dict(eta=0.0), dict(lam=np.inf),
           dict(ess_frac=-0.1), dict(clash_alpha=0.0), dict(reward={"sheet": 1.0}), dict(reward={"rg": np.nan}), dict(lengths=[]),
           dict(lengths=[0]), dict(lengths=[65]), dict(batch_size=4), dict(every=0), dict(num_steps=21), dict(eta=1.5)]
    for kw in bad:
        a = dict(lengths=[30, 31], n_particles=8)
        a.update(kw)
        with pytest.raises(ValueError):
            sampling.steer(None, ds, **a)
    with pytest.raises(ValueError):
        structures.steer_terms([np.zeros((4, 6), np.float32)], ds.feature_names["angles"], reward={"sheet": 1.0})
    with pytest.raises(ValueError):
        structures.steer_terms([np.zeros((4, 5), np.float32)], ds.feature_names["angles"])
    with pytest.raises(ValueError):
        structures.steer_terms([np.zeros((4, 6), np.float32)], ds.feature_names["angles"], offset=np.zeros(6, np.float32))


def test_script_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sample_steered", os.path.join(REPO, "bin", "sample_steered.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["-m", "dir", "--particles", "4", "--w_strand", "5", "--num_steps", "20", "--every", "2"])
    assert (a.particles, a.w_strand, a.num_steps, a.every) == (4, 5.0, 20, 2)
    assert (a.lam, a.ess_frac, a.steer_from, a.w_clashes, a.w_rg, a.w_helix, a.eta) == (1.0, 0.5, None, -1.0, 0.0, 0.0, 1.0)
    from foldingdiff_amd import build
    assert "steer.hip" in build.SOURCES


def test_kernels_hold_no_scratch():
    """steer.hip compiles for the device alone and none of its five kernels has a private segment or a spill (the resampling
    kernel's three arrays of 1024 doubles are LDS)."""
    import subprocess

    from foldingdiff_amd import build as fbuild
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    r = subprocess.run([hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
                        "--cuda-device-only", "-o", "-", os.path.join(fbuild.CSRC, "steer.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ("steer_shift_kernel", "steer_atoms_kernel", "steer_terms_kernel", "steer_resample_kernel", "steer_gather_kernel"):
        m = re.search(r"\.name:\s+_Z\S*" + kernel + r"\S*\n(.*?)\.wavefront_size", r.stdout, re.S)
        assert m, f"{kernel}'s metadata not found"
        md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(1))}
        print(kernel, md)
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md


def test_entries_are_declared_and_bound(lib):
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _binding.exported_symbols() and hasattr(lib, name)
    assert "typedef struct fd_steer_params" in src
    assert C.sizeof(_binding.FdSteerParams) == 4 * 8 + 3 * 8 + 9 * 4 + 4 + 16 * 4
    assert lib.fd_abi_version() == 7


# ---------------------------------------------------------------------------------- the model-free entries' checks
def test_model_free_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Each bad call returns -1 with its word in fd_last_error() and leaves the outputs alone, on a machine without a GPU
    too.  No valid call is made."""
    i32 = lambda *v: np.array(v, np.int32)   # noqa: E731
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    x = np.zeros((2, 6, 6), np.float32)
    nan_live, nan_dead = x.copy(), x.copy()
    nan_live[1, 3, 2] = np.nan
    nan_dead[0, 5, 0] = np.nan            # beyond lens[0] = 4: not looked at, so this call is rejected for another reason
    idx, w = i32(0, 1, 2, 3, 4, 5, -1, -1, -1), np.array([-1.0, 0.0, 0.5, 0.5])
    off, ang = np.zeros(6, np.float32), np.ones(6, np.uint8)

    def rewards(x=x, lens=i32(4, 6), B=2, L=6, F=6, idx=idx, off=off, ang=ang, w=w, alpha=0.63, terms="default", rew="default"):
        terms = np.full((2, 4), -7.0) if isinstance(terms, str) else terms
        rew = np.full(2, -7.0) if isinstance(rew, str) else rew
        return [terms, rew], lib.fd_steer_rewards(0, P(x), P(lens), B, L, F, P(idx), P(off), P(ang), P(w), alpha, P(terms), P(rew))

    inf_off = off.copy()
    inf_off[2] = np.inf
    for kw, word in [(dict(x=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(w=None), b"null"),
                     (dict(terms=None), b"null"), (dict(rew=None), b"null"), (dict(ang=None), b"is_angle"),
                     (dict(B=0), b"B=0"), (dict(L=0), b"L=0"), (dict(F=2), b"F=2"), (dict(F=17), b"F=17"),
                     (dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"),
                     (dict(L=4096, lens=i32(4, 2049)), b"outside [1, 2048]"),
                     (dict(idx=i32(0, 1, 6, 3, 4, 5, -1, -1, -1)), b"feat_idx[2]"), (dict(idx=i32(-1, 1, 2, 3, 4, 5, -1, -1, -1)), b"feat_idx[0]"),
                     (dict(w=np.array([1.0, np.nan, 0.0, 0.0])), b"weights[1]"), (dict(w=np.array([1.0, 0.0, 0.0, np.inf])), b"weights[3]"),
                     (dict(alpha=0.0), b"clash_alpha"), (dict(alpha=float("nan")), b"clash_alpha"), (dict(off=inf_off), b"offset[2]"),
                     (dict(x=nan_live), b"not finite at sequence 1, position 3"), (dict(x=nan_dead, alpha=-1.0), b"clash_alpha")]:
        expect(word, *rewards(**kw))
    assert checked == 23

    def resample(reward="default", logw="default", r_prev="default", G=2, P_=3, lam=1.0, ess=0.5, u="default", anc="default", flags="default"):
        d = lambda v, make: make() if isinstance(v, str) else v   # noqa: E731
        reward = d(reward, lambda: np.zeros(6))
        logw, r_prev = d(logw, lambda: np.full(6, -7.0)), d(r_prev, lambda: np.full(6, -7.0))
        u = d(u, lambda: np.array([0.1, 0.9]))
        anc, flags = d(anc, lambda: np.full(6, -7, np.int32)), d(flags, lambda: np.full(2, 249, np.uint8))
        rc = lib.fd_steer_resample(0, P(reward), P(logw), P(r_prev), G, P_, lam, ess, P(u), P(anc), P(flags))
        return [logw, r_prev, anc, None if flags is None else flags.astype(np.int64) - 256], rc

    for kw, word in [(dict(reward=None), b"null"), (dict(logw=None), b"null"), (dict(r_prev=None), b"null"), (dict(u=None), b"null"),
                     (dict(anc=None), b"null"), (dict(flags=None), b"null"), (dict(G=0), b"G=0"), (dict(P_=0), b"P=0"),
                     (dict(P_=1025), b"P=1025"), (dict(lam=float("inf")), b"lambda"), (dict(lam=float("nan")), b"lambda"),
                     (dict(ess=-0.5), b"ess_frac"), (dict(ess=float("nan")), b"ess_frac"), (dict(u=np.array([0.1, 1.0])), b"u[1]"),
                     (dict(u=np.array([-1e-9, 0.5])), b"u[0]"), (dict(u=np.array([np.nan, 0.5])), b"u[0]")]:
        expect(word, *resample(**kw))
    assert checked == 23 + 16
