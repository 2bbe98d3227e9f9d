"""Resampling schedules of motif-conditioned sampling, the parts that need no GPU: the schedule generator, the jump
coefficients, the host preparation of ``sampling.inpaint(..., jump_length, n_resample)`` (the device call replaced by a
stand-in), the CPU restatement (tests/resample_reference.py) and the code generation of the jump kernel."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import inpaint_reference as ipr
import resample_reference as rsr
from foldingdiff_amd import _binding, beta_schedules, build as fbuild, sampling
from oracle import ref_model, ref_philox, ref_sampling
from test_inpaint import F, _StubModel, _dset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24   # the unit roundoff of float32


def _legal(visits, t_start):
    v = [int(a) for a in visits]
    assert v[0] == t_start and v[-1] == 0 and all(0 <= a <= t_start for a in v)
    for i in range(1, len(v)):
        assert v[i] == v[i - 1] - 1 or v[i] >= v[i - 1], (i, v)


def test_the_hand_checked_schedule():
    got = sampling.resample_schedule(5, 2, 2)
    assert got.dtype == np.int32 and got.tolist() == [5, 4, 3, 2, 3, 2, 1, 0, 1, 0]


@pytest.mark.parametrize("t_start", [0, 1, 5, 24])
@pytest.mark.parametrize("jump_length", [1, 2, 5, 30])
@pytest.mark.parametrize("n_resample", [1, 2, 3])
def test_schedule_length_and_legality(t_start, jump_length, n_resample):
    v = sampling.resample_schedule(t_start, jump_length, n_resample)
    n_levels = len(range(0, t_start + 1 - jump_length, jump_length))
    assert len(v) == t_start + 1 + n_levels * (n_resample - 1) * jump_length
    _legal(v, t_start)
    if n_resample == 1:
        assert v.tolist() == list(range(t_start, -1, -1))
    # every jump goes up jump_length levels: from level a to level a + jump_length
    jumps = [(int(v[i - 1]), int(v[i]) + 1) for i in range(1, len(v)) if v[i] != v[i - 1] - 1]
    assert len(jumps) == n_levels * (n_resample - 1) and all(b - a == jump_length for a, b in jumps)


def test_schedule_rejects_what_is_not_a_schedule():
    for bad in ((5, 0, 2), (5, 2, 0), (5, -1, 1)):
        with pytest.raises(ValueError):
            sampling.resample_schedule(*bad)


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_jump_coef_against_the_float64_formula(schedule):
    T = 25
    betas = beta_schedules.get_variance_schedule(schedule, T)
    visits = sampling.resample_schedule(T - 1, 5, 3).tolist() + [3, 2, 1, 0, T - 1]   # ... and a jump from level 0 to level T
    visits = np.asarray(visits + list(range(T - 2, -1, -1)), dtype=np.int32)
    got = sampling.resample_jump_coef(betas, visits)
    acp = np.concatenate([[1.0], ref_sampling.alpha_terms(ref_sampling.beta_schedule(schedule, T))["alphas_cumprod"].numpy().astype(np.float64)])
    jumps = [(int(visits[i - 1]), int(visits[i]) + 1) for i in range(1, len(visits)) if visits[i] != visits[i - 1] - 1]
    assert got.dtype == np.float32 and got.shape == (len(jumps), 2) and (0, T) in jumps and (0, 5) in jumps
    keep = sampling.inpaint_levels(betas)[0].astype(np.float64)
    for (a, b), (jk, js) in zip(jumps, got):
        r = acp[b] / acp[a]
        assert jk == np.float32(np.sqrt(r)) and js == np.float32(np.sqrt(1.0 - r))
        assert 0.0 <= jk <= 1.0 and 0.0 <= js <= 1.0
        assert abs(float(jk) ** 2 + float(js) ** 2 - 1.0) <= 2e-7
        # telescoping: keep[j] = fl32(sqrt(acp(j))) and jk = fl32(sqrt(acp(b) / acp(a))) each carry one relative rounding
        # |e| <= U, so jk * keep[a] / keep[b] = (1 + e1)(1 + e2) / (1 + e3) lies within 3 U + 4 U^2 of 1 (the float64
        # arithmetic of this check adds 2^-50 at most)
        assert abs(float(jk) * keep[a] - keep[b]) <= (3 * U + 4 * U * U + 2.0 ** -50) * keep[b], (a, b)
    assert sampling.resample_jump_coef(betas, np.arange(T - 1, -1, -1)).shape == (0, 2)


def _oracle(T=4):
    cfg = ref_model.OracleConfig(hidden_size=32, num_attention_heads=2, intermediate_size=64, layer_norm_eps=1e-12,
                                 num_hidden_layers=1, max_position_embeddings=16, position_embedding_type="relative_key")
    return ref_model.synthetic_model(cfg, (True,) * F, "gaussian_fourier", "mlp", seed=2), ref_sampling.beta_schedule("cosine", T)


def _case(T=4, B=2, L=8):
    rng = np.random.default_rng(12)
    x0 = ref_sampling.wrap(torch.from_numpy(rng.standard_normal((B, L, F)).astype(np.float32) * 1.5)).numpy()
    fixed = np.zeros((B, L, F), dtype=bool)
    fixed[0, 2:5] = True
    fixed[1, 1, 3] = True
    known = np.where(fixed, rng.uniform(-3, 3, (B, L, F)), np.nan).astype(np.float32)
    return x0, known, fixed, [8, 5]


def test_restatement_without_a_jump_is_the_replacement_loop():
    T, seed = 4, 1234567
    model, betas = _oracle(T)
    x0, known, fixed, lens = _case(T)
    coef = ipr.levels(betas)
    B, L = 2, 8
    zero = np.zeros((B, L, F), dtype=np.float32)
    step_noise = np.stack([zero if t == 0 else ref_philox.philox_normal(seed, t, 0, B, L, F) for t in range(T)])
    known_noise = np.stack([zero if j == 0 else ipr.tagged_draw(seed, j, 0, B, L, F) for j in range(T + 1)])
    want = ipr.loop(model, lens, x0, T - 1, betas, [True] * F, known, fixed, coef, step_noise, known_noise)
    got = rsr.loop(model, lens, x0, T - 1, betas, [True] * F, known, fixed, coef, list(range(T - 1, -1, -1)), np.zeros((0, 2), np.float32), seed)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # with jumps: one row per visit, the last row holds known's bits, a repeated step index draws fresh noise
    visits = sampling.resample_schedule(T - 1, 2, 2)
    jc = sampling.resample_jump_coef(betas, visits)
    res = rsr.loop(model, lens, x0, T - 1, betas, [True] * F, known, fixed, coef, visits, jc, seed)
    assert res.shape == (len(visits), B, L, F) and np.isfinite(res).all()
    assert np.array_equal(res[-1][fixed].view(np.uint32), known[fixed].view(np.uint32))
    assert not np.array_equal(res[-1][~fixed], want[-1][~fixed])
    assert rsr.seeds(seed, 0) == seed and rsr.seeds(2 ** 64 - 1, 1) == rsr.GOLDEN - 1 and len({rsr.seeds(seed, s) for s in range(5)}) == 5


def test_restatement_jump_statement():
    T = 4
    _, betas = _oracle(T)
    x0, known, fixed, lens = _case(T)
    coef = ipr.levels(betas)
    rng = np.random.default_rng(5)
    zf, zk = rng.standard_normal((2, 2, 8, F)).astype(np.float32)
    jk, js = np.float32(0.8), np.float32(0.6)
    got = rsr.jump(x0, known, fixed, 3, jk, js, coef, zf, zk, [True] * F, lens)
    valid = np.zeros_like(fixed)
    valid[0, :8] = valid[1, :5] = True
    lv = ipr.known_at_level(np.nan_to_num(known), 3, coef, zk, [True] * F)
    assert np.array_equal(got[fixed].view(np.uint32), lv[fixed].view(np.uint32))
    free = valid & ~fixed
    want = ipr.wrap32((jk * x0).astype(np.float32) + (js * zf).astype(np.float32))
    assert np.array_equal(got[free].view(np.uint32), want[free].view(np.uint32)) and (np.abs(got[free]) <= np.float32(np.pi)).all()
    assert np.array_equal(got[~valid].view(np.uint32), x0[~valid].view(np.uint32))
    unwrapped = rsr.jump(x0, known, fixed, 3, jk, js, coef, zf, zk, [False] * F, lens)
    assert not np.array_equal(unwrapped[free], got[free])            # the wrap is per feature
    # the three streams of one level and key differ
    a, b, c = ref_philox.philox_normal(9, 3, 0, 2, 8, F), ipr.tagged_draw(9, 3, 0, 2, 8, F), rsr.jump_draw(9, 3, 0, 2, 8, F)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@pytest.fixture
def device_calls(monkeypatch):
    """Replaces both device calls of ``inpaint``; each records its arguments and returns the known value where an element is
    fixed and the start point elsewhere."""
    calls = {"plain": [], "resample": []}

    def plain(h, x0, lens, t_start, known, fixed, coef, seed, out, full_history):
        calls["plain"].append(dict(t_start=t_start, seed=seed, full_history=full_history))
        out[:] = np.where(fixed.astype(bool), known, x0)[None]

    def resample(h, x0, lens, t_start, known, fixed, coef, visits, jump_coef, seed, out):
        calls["resample"].append(dict(x0=x0.copy(), lens=lens.copy(), t_start=t_start, known=known.copy(), fixed=fixed.copy(),
                                      coef=coef.copy(), visits=visits.copy(), jump_coef=jump_coef.copy(), seed=seed, rows=out.shape[0]))
        out[:] = np.where(fixed.astype(bool), known, x0)[None]

    monkeypatch.setattr(sampling, "_run_fd_inpaint", plain)
    monkeypatch.setattr(sampling, "_run_fd_inpaint_resample", resample)
    return calls


def test_inpaint_with_a_resampling_schedule_prepares_the_new_call(device_calls):
    rng = np.random.default_rng(3)
    offset = np.array([0.3, -0.2, 3.0, 1.9, 2.0, 2.1], dtype=np.float32)
    k0 = rng.uniform(-np.pi, np.pi, (7, F)).astype(np.float32)
    k1 = rng.uniform(-np.pi, np.pi, (5, F)).astype(np.float32)
    f0 = np.zeros(7, dtype=bool)
    f0[2:5] = True
    f1 = np.zeros((5, F), dtype=bool)
    f1[0, 3] = f1[4, 0] = True
    model, ds = _StubModel(), _dset(offset)          # T = 5
    out = sampling.inpaint(model, ds, [k0, k1, k1], [f0, f1, f1], jump_length=2, n_resample=2, batch_size=2)
    assert not device_calls["plain"] and len(device_calls["resample"]) == 2
    c, c2 = device_calls["resample"]
    betas = ds.alpha_beta_terms["betas"]
    want_visits = sampling.resample_schedule(4, 2, 2)
    assert c["visits"].dtype == np.int32 and np.array_equal(c["visits"], want_visits) and c["t_start"] == 4 and c["rows"] == 1
    assert c["jump_coef"].dtype == np.float32 and np.array_equal(c["jump_coef"], sampling.resample_jump_coef(betas, want_visits))
    assert c["jump_coef"].shape == (2, 2)
    assert np.array_equal(c["coef"], sampling.inpaint_levels(betas)) and c["lens"].tolist() == [7, 5] and c2["lens"].tolist() == [5]
    assert c["seed"] != c2["seed"]                                         # one Philox seed per batch, as without resampling
    want_fixed = np.zeros((2, 7, F), dtype=bool)
    want_fixed[0, 2:5] = True
    want_fixed[1, :5] = f1
    assert c["fixed"].dtype == np.uint8 and np.array_equal(c["fixed"].astype(bool), want_fixed)
    data = np.zeros((2, 7, F), dtype=np.float32)
    data[0, :7], data[1, :5] = k0, k1
    want_known = ipr.wrap32(data - offset)                                  # model space: minus the mean offset, wrapped
    assert c["known"].dtype == np.float32 and np.array_equal(c["known"][want_fixed], want_known[want_fixed])
    assert (c["known"][~want_fixed] == 0).all()
    assert [o.shape for o in out] == [(7, F), (5, F), (5, F)]
    assert ("varlen", 1) in model.options and model.options[-1] == ("varlen", 0)
    # scaffold hands the two through
    motif = rng.uniform(-3, 3, (3, F)).astype(np.float32)
    sampling.scaffold(model, _dset(None), motif, [9], jump_length=1, n_resample=3)
    assert np.array_equal(device_calls["resample"][-1]["visits"], sampling.resample_schedule(4, 1, 3)) and not device_calls["plain"]


def test_inpaint_defaults_make_the_call_they_made(device_calls):
    k = np.zeros((6, F), dtype=np.float32)
    f = np.zeros(6, dtype=bool)
    f[1:3] = True
    model, ds = _StubModel(), _dset(None)
    sampling.inpaint(model, ds, [k], [f])
    sampling.inpaint(model, ds, [k], [f], jump_length=2)                   # n_resample = 1: the plain descent
    sampling.inpaint(model, ds, [k], [f], n_resample=3)                    # no jump_length: the plain descent
    sampling.inpaint(model, ds, [k], [f], jump_length=2, n_resample=1, final_only=False)
    assert len(device_calls["plain"]) == 4 and not device_calls["resample"]
    assert [c["full_history"] for c in device_calls["plain"]] == [0, 0, 0, 1]
    with pytest.raises(ValueError, match="final"):
        sampling.inpaint(model, ds, [k], [f], jump_length=2, n_resample=2, final_only=False)
    with pytest.raises(ValueError):
        sampling.inpaint(model, ds, [k], [f], jump_length=0, n_resample=2)
    assert len(device_calls["plain"]) == 4 and not device_calls["resample"]


def test_header_binding_and_library_export_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ("fd_sample_inpaint_resample", "fd_inpaint_jump"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _binding._SIGNATURES and hasattr(lib, name), name
    assert "#define FDMI_ABI_VERSION 7" in header
    assert hasattr(sampling, "resample_schedule") and hasattr(sampling, "resample_jump_coef") and hasattr(sampling, "_run_fd_inpaint_resample")


def test_scaffold_script_has_the_two_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sample_scaffold", os.path.join(REPO, "bin", "sample_scaffold.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["-m", "x", "--motif", "y", "--motif_residues", "1", "2"]
    args = cli.build_parser().parse_args(base)
    assert args.jump_length is None and args.n_resample == 1
    args = cli.build_parser().parse_args(base + ["--jump_length", "5", "--n_resample", "2"])
    assert args.jump_length == 5 and args.n_resample == 2


def test_the_jump_kernel_uses_no_scratch(tmp_path):
    """inpaint_jump_kernel compiled as the product build compiles it: no private segment, no spill."""
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    out = tmp_path / "inpaint_jump.s"
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include")] \
        + fbuild.PER_SOURCE_FLAGS.get("inpaint_jump", []) + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(fbuild.CSRC, "inpaint_jump.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    metas = re.findall(r"\.name:\s+(_ZN4fdmi19inpaint_jump_kernel\w+)\n(.*?)\.wavefront_size", asm, re.S)
    assert len(metas) == 1, [m[0] for m in metas]
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", metas[0][1])}
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert "inpaint_jump.hip" in fbuild.SOURCES
