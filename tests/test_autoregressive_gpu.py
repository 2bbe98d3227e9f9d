"""
The autoregressive baseline on the device (needs an MI355X: pytest -m gpu): ``fd_ar_forward`` against the CPU restatement
(tests/ar_reference.py), the rollout of ``fd_ar_sample`` step by step and free-running, and the reference class's own
rollout (tests/golden/ref_autoregressive.npz).  Models are tiny: 2 layers, intermediate size 2 x hidden.

Tolerances:
  * a forward, and row i of step i given the device's own prefix (teacher forcing):  max|d| <= 1e-5 against the fp32
    restatement, the project's forward gate (test_gpu_parity.py).  Every rollout mistake that is easy to make moves row i
    by far more: key i attended too 5e-4, row i's input zeroed 8e-2, the length row added behind the LayerNorm 0.9, the
    step index or one common length in place of the sequence's own > 1, a changed prefix position 1.8e-4.
  * the free-running rollout against the fp64 restatement: not fixed in advance.  With e32 = the largest gap of ONE fp32
    against fp64 restated forward at that shape and E_ref = the largest gap of the fp32 against the fp64 rollout, the
    device may be off by E_dev <= (1e-5 / e32) * E_ref: the multiple of fp32 noise the forward gate allows one forward.
  * seeds, and positions at and behind max(seq_lengths): bit-equal to the input; the same call twice: bit-equal.
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ar_reference
from conftest import GOLDEN, REPO, golden
from foldingdiff_amd import _binding, modelling, structures
from oracle import ref_model

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
REPORT = {}
MODES = ["auto", "fuse_attn1", "fuse_ffn2"]
_OPTS = {"auto": {}, "fuse_attn1": {"fuse_attn": 1}, "fuse_ffn2": {"fuse_ffn": 2}}


def _record(name, **kw):
    """Every measured figure is printed before its assertion (pytest -s shows them)."""
    REPORT[name] = {k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kw.items()}
    print(name, json.dumps(REPORT[name], sort_keys=True))


_PAIRS = {}


def _pair(hidden, heads, pos="relative_key", time_encoding="gaussian_fourier", maxpos=128, seed=0, ft=(True,) * 6):
    """(fp32 oracle, fp64 oracle on the fp32 length table, product model on cuda:0) with identical synthetic weights,
    built once per configuration."""
    key = (hidden, heads, pos, time_encoding, maxpos, seed)
    if key not in _PAIRS:
        ocfg = ref_model.OracleConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                      num_hidden_layers=2, max_position_embeddings=maxpos, position_embedding_type=pos)
        o32 = ref_model.synthetic_model(ocfg, ft, time_encoding, "mlp", seed=seed)
        pcfg = modelling.BertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=2 * hidden,
                                    num_hidden_layers=2, max_position_embeddings=maxpos, position_embedding_type=pos)
        pm = modelling.BertForAutoregressiveBase(pcfg, list(ft), time_encoding=time_encoding, decoder="mlp")
        pm.load_state_dict(o32.state_dict())
        pm.to("cuda:0")
        pm.set_precision("f16x3")
        pm.prepare()
        _PAIRS[key] = (o32, ar_reference.as_double(o32, maxpos + 1), pm)
    return _PAIRS[key]


class _mode:
    """Run the device calls of a block under one of MODES; None when the fused attention does not take the shape."""

    def __init__(self, pm, mode, L):
        self.pm, self.opts = pm, _OPTS[mode]
        self.ok = "fuse_attn" not in self.opts or bool(_binding.load().fd_fused_attn_supported(pm._ensure_handle(), L))

    def __enter__(self):
        for k, v in self.opts.items():
            self.pm.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.opts:
            self.pm.set_option(k, -1)


def _uniform(B, L, seed, F=6):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, L, F, generator=g) * 2 - 1) * 3.0


def _device_rollout(pm, seed, lens, ns):
    """The full [B, L, F] state of fd_ar_sample (the Python method trims it)."""
    x = np.ascontiguousarray(seed.numpy())
    out = np.full_like(x, np.nan)
    n = np.ascontiguousarray(np.asarray(lens, np.int32))
    _binding.check(_binding.load().fd_ar_sample(pm.prepare(), _binding.ptr(x), _binding.ptr(n), x.shape[0], x.shape[1], ns,
                                                _binding.ptr(out)))
    return torch.from_numpy(out)


# ------------------------------------------------------------ 1. the forward
SHAPES = [(33, [33, 1, 32, 8, 9], [33, 0, 128, 17, 64]), (128, [128, 1, 100, 64, 65], [128, 0, 97, 17, 64])]


@pytest.mark.parametrize("L,key_lens,seq_lengths", SHAPES)
@pytest.mark.parametrize("hidden,heads", [(192, 6), (384, 12)])
def test_forward_against_the_restatement(gpu, hidden, heads, L, key_lens, seq_lengths):
    o32, _, pm = _pair(hidden, heads)
    x, mask, n = _uniform(len(key_lens), L, seed=hidden + L), ar_reference.prefix_mask(key_lens, L), torch.tensor(seq_lengths)
    want = ar_reference.ar_forward(o32, x, mask, n).numpy().astype(np.float64)
    ran = 0
    for mode in MODES:
        with _mode(pm, mode, L) as md:
            if not md.ok:
                continue
            err = np.abs(pm(x, mask, n).numpy() - want).max()
        ran += 1
        _record(f"ar_fwd_d{hidden}_L{L}_{mode}", max=err)
        assert err <= FWD_TOL, (mode, err)
    assert ran >= 2


@pytest.mark.parametrize("pos,time_encoding", [("absolute", "gaussian_fourier"), ("relative_key", "sinusoidal")])
def test_forward_absolute_positions_and_sinusoidal_lengths(gpu, pos, time_encoding):
    L, key_lens, seq_lengths = SHAPES[0]
    o32, _, pm = _pair(192, 6, pos=pos, time_encoding=time_encoding, seed=7)
    x, mask, n = _uniform(len(key_lens), L, seed=3), ar_reference.prefix_mask(key_lens, L), torch.tensor(seq_lengths)
    err = np.abs(pm(x, mask, n).numpy() - ar_reference.ar_forward(o32, x, mask, n).numpy().astype(np.float64)).max()
    _record(f"ar_fwd_{pos}_{time_encoding}", max=err)
    assert err <= FWD_TOL


# ------------------------------------------------------------ 2 / 3. the rollout, teacher-forced per step
def _teacher_forced_gap(o32, dev, seed, lens, ns):
    """For every step i: the restated forward on the device's own positions < i, positions >= i as the seed holds them
    (row i enters the step with the caller's values), keys 0 .. i-1; its row i against the device's position i.
    Returns (largest gap, the step it is at)."""
    B, L, _ = seed.shape
    n = torch.as_tensor(lens)
    steps = list(range(ns, int(n.max())))
    worst, at = 0.0, -1
    for c0 in range(0, len(steps), 32):   # 32 steps per restated forward
        chunk = steps[c0:c0 + 32]
        xs, ms = [], []
        for i in chunk:
            x = dev.clone()
            x[:, i:] = seed[:, i:]
            m = torch.zeros(B, L)
            m[:, :i] = 1.0
            xs.append(x)
            ms.append(m)
        out = ar_reference.ar_forward(o32, torch.cat(xs), torch.cat(ms), n.repeat(len(chunk))).view(len(chunk), B, L, -1)
        for j, i in enumerate(chunk):
            gap = (out[j, :, i].double() - dev[:, i].double()).abs().max().item()
            if gap > worst:
                worst, at = gap, i
    return worst, at


def _check_rollout_teacher_forced(hidden, heads, pos, mode, L, lens, ns, seed_no):
    o32, _, pm = _pair(hidden, heads, pos=pos)
    seed = _uniform(len(lens), L, seed=seed_no)
    with _mode(pm, mode, L) as md:
        if not md.ok:
            pytest.fail(f"the fused attention kernel does not take L={L} at d={hidden}")   # (every shape here is in its range)
        dev = _device_rollout(pm, seed, lens, ns)
    assert torch.isfinite(dev).all()
    gap, at = _teacher_forced_gap(o32, dev, seed, lens, ns)
    _record(f"ar_step_d{hidden}_{pos}_L{L}_{mode}", max=gap, step=at)
    assert torch.equal(dev[:, :ns], seed[:, :ns]), "the seeds must come back bit for bit"
    assert torch.equal(dev[:, max(lens):], seed[:, max(lens):]), "positions at and behind max(seq_lengths) keep the seed"
    assert not torch.equal(dev[:, ns:max(lens)], seed[:, ns:max(lens)])
    assert gap <= FWD_TOL, (gap, at)


ROLL = dict(L=40, lens=[40, 33, 9, 17, 3], ns=2)   # steps cross the 8-row packing, the 16-row waves, the 32-key tile, 128 rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hidden,heads", [(192, 6), (384, 12)])
def test_rollout_teacher_forced(gpu, hidden, heads, mode):
    _check_rollout_teacher_forced(hidden, heads, "relative_key", mode, seed_no=11, **ROLL)


def test_rollout_teacher_forced_absolute_positions(gpu):
    _check_rollout_teacher_forced(192, 6, "absolute", "auto", seed_no=12, **ROLL)


@pytest.mark.parametrize("mode", MODES)
def test_rollout_teacher_forced_128(gpu, mode):
    """Four key tiles and full 128-row sequences, every step."""
    _check_rollout_teacher_forced(384, 12, "relative_key", mode, L=128, lens=[128, 97, 64], ns=4, seed_no=13)


# ------------------------------------------------------------ 4. free-running against fp64
def _noise_figures(o32, o64, seed, lens, ns):
    """(e32, E_ref, the fp64 rollout): e32 on the forward of the last step -- the fp64 rollout's state, keys 0 .. max-2,
    every row compared."""
    n = torch.as_tensor(lens)
    r64 = ar_reference.ar_sample(o64, seed.double(), n, ns, return_full=True)
    r32 = ar_reference.ar_sample(o32, seed, n, ns, return_full=True)
    mask = torch.zeros(seed.shape[:2])
    mask[:, : int(n.max()) - 1] = 1.0
    f32 = ar_reference.ar_forward(o32, r64.float(), mask, n)
    f64 = ar_reference.ar_forward(o64, r64.float().double(), mask.double(), n)
    return (f32.double() - f64).abs().max().item(), (r32.double() - r64).abs().max().item(), r64


@pytest.mark.parametrize("hidden,heads,pos", [(192, 6, "relative_key"), (384, 12, "relative_key"), (192, 6, "absolute")])
def test_rollout_free_running_against_fp64(gpu, hidden, heads, pos):
    o32, o64, pm = _pair(hidden, heads, pos=pos)
    L, lens, ns = ROLL["L"], ROLL["lens"], ROLL["ns"]
    seed = _uniform(len(lens), L, seed=11)
    e32, e_ref, r64 = _noise_figures(o32, o64, seed, lens, ns)
    gate = FWD_TOL / e32 * e_ref
    for mode in MODES:
        with _mode(pm, mode, L) as md:
            if not md.ok:   # (the fused attention kernel is built for the relative position types)
                continue
            dev = _device_rollout(pm, seed, lens, ns)
        e_dev = (dev.double() - r64).abs().max().item()
        _record(f"ar_free_d{hidden}_{pos}_{mode}", e32=e32, E_ref=e_ref, gate=gate, E_dev=e_dev)
        assert e_dev <= gate, (mode, e_dev, gate)


# ------------------------------------------------------------ 5. the reference class's own rollout
@pytest.fixture(scope="module")
def abs_models():
    gm = golden("ref_abs_model.npz")
    sd = {k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")}
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="absolute")
    o32 = ref_model.OracleBertForDiffusion(ocfg, [True] * 6)
    o32.load_state_dict(sd, strict=True)
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                               max_position_embeddings=64, position_embedding_type="absolute")
    pm = modelling.BertForAutoregressiveBase(cfg, [True] * 6)
    pm.load_state_dict(sd)
    pm.to("cuda:0")
    return o32, ar_reference.as_double(o32, 65), pm


def test_sample_against_the_reference_class(gpu, abs_models):
    o32, o64, pm = abs_models
    ga = golden("ref_autoregressive.npz")
    seed, lens, ns, valid = torch.from_numpy(ga["seed"]), ga["seq_lengths"].tolist(), int(ga["num_seed"]), ga["valid"]
    e32, _, _ = _noise_figures(o32, o64, seed, lens, ns)
    restated = ar_reference.ar_sample(o32, seed, torch.tensor(lens), ns, return_full=True).numpy().astype(np.float64)
    e_ref = np.abs(restated - ga["rollout"])[valid].max()
    gate = FWD_TOL / e32 * e_ref
    items = pm.sample(seed, torch.tensor(lens), num_seed=ns, pbar=False)
    assert [tuple(i.shape) for i in items] == [(n, 6) for n in lens]
    e_dev = max(np.abs(it.numpy().astype(np.float64) - ga["rollout"][b, :n]).max() for b, (it, n) in enumerate(zip(items, lens)))
    x = torch.from_numpy(ga["fwd_x"])
    fwd = pm(x, ar_reference.prefix_mask(ga["fwd_key_lens"].tolist(), x.shape[1]), torch.from_numpy(ga["fwd_seq_lengths"]))
    e_fwd = np.abs(fwd.numpy().astype(np.float64) - ga["fwd_out"]).max()
    _record("ar_golden", e32=e32, E_ref=e_ref, gate=gate, E_dev=e_dev, fwd=e_fwd)
    assert e_fwd <= FWD_TOL
    assert e_dev <= gate


# ------------------------------------------------------------ 6. repeatability, arguments, the seeds' featuriser
def test_same_call_same_bits(gpu):
    _, _, pm = _pair(192, 6)
    seed = _uniform(5, ROLL["L"], seed=21)
    a = _device_rollout(pm, seed, ROLL["lens"], ROLL["ns"])
    b = _device_rollout(pm, seed, ROLL["lens"], ROLL["ns"])
    assert torch.equal(a, b)
    items = pm.sample(seed, torch.tensor(ROLL["lens"]), num_seed=ROLL["ns"], pbar=False)
    assert all(torch.equal(it, a[i, :n]) for i, (it, n) in enumerate(zip(items, ROLL["lens"])))
    x, mask, n = _uniform(5, 33, seed=22), ar_reference.prefix_mask(SHAPES[0][1], 33), torch.tensor(SHAPES[0][2])
    assert torch.equal(pm(x, mask, n), pm(x, mask, n))


def test_entries_check_their_arguments(gpu):
    lib = _binding.load()
    _, _, pm = _pair(192, 6)
    h = pm.prepare()
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    x = np.zeros((2, 8, 6), np.float32)

    def fwd(x=x, n=i32(8, 5), k=i32(8, 5), B=2, L=8, out="default", h=h):
        out = np.full((2, 8, 6), -7, np.float32) if isinstance(out, str) else out
        return out, lib.fd_ar_forward(h, P(x), P(n), P(k), B, L, P(out))

    def smp(x=x, n=i32(8, 5), B=2, L=8, ns=2, out="default", h=h):
        out = np.full((2, 8, 6), -7, np.float32) if isinstance(out, str) else out
        return out, lib.fd_ar_sample(h, P(x), P(n), B, L, ns, P(out))

    cases = [(fwd, dict(x=None), -1, b"null"), (fwd, dict(n=None), -1, b"null"), (fwd, dict(k=None), -1, b"null"),
             (fwd, dict(out=None), -1, b"null"), (fwd, dict(B=0), -1, b"positive"), (fwd, dict(L=129), -1, b"exceeds"),
             (fwd, dict(n=i32(8, 129)), -1, b"seq_lengths"), (fwd, dict(n=i32(-1, 5)), -1, b"seq_lengths"),
             (fwd, dict(k=i32(8, 0)), -1, b"lens"), (fwd, dict(k=i32(9, 5)), -1, b"lens"),
             (smp, dict(x=None), -1, b"null"), (smp, dict(n=None), -1, b"null"), (smp, dict(out=None), -1, b"null"),
             (smp, dict(ns=0), -1, b"num_seed"), (smp, dict(n=i32(9, 5)), -1, b"exceeds"), (smp, dict(n=i32(8, 129)), -1, b"seq_lengths")]
    for fn, kw, code, word in cases:
        out, rc = fn(**kw)
        msg = lib.fd_last_error()
        assert rc == code and word in msg, (kw, rc, msg)
        assert out is None or (out == -7).all()
    # lengths at or below the seeds: nothing to generate, the seed comes back
    seed = _uniform(2, 8, seed=5).numpy()
    out, rc = smp(x=seed, n=i32(2, 0), ns=2)
    assert rc == 0 and np.array_equal(out, seed)
    # the exact-fp32 mode has no autoregressive path
    pcfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                                max_position_embeddings=32, position_embedding_type="relative_key")
    p32 = modelling.BertForAutoregressiveBase(pcfg, [True] * 6).to("cuda:0").set_precision("f32")
    h32 = p32.prepare()
    for fn in (fwd, smp):
        out, rc = fn(h=h32)
        assert rc == -5 and b"FD_PREC_F16X3" in lib.fd_last_error() and (out == -7).all()
    with pytest.raises(_binding.FdmiError, match="FD_PREC_F16X3"):
        p32.sample(torch.zeros(2, 8, 6), torch.tensor([8, 5]))


def test_sample_initial_angles_on_a_real_structure(gpu, tmp_path):
    """The default featuriser (the device's internal coordinates) on 1CRN: the first residues' six angles, NaN where the
    chain's start has none."""
    spec = importlib.util.spec_from_file_location("sample_autoregressive", os.path.join(REPO, "bin", "sample_autoregressive.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    src = os.path.join(GOLDEN, "1CRN.pdb")
    os.symlink(src, tmp_path / "1CRN.pdb")
    got = cli.sample_initial_angles(3, 4, eps=0.0, pdb_dir=str(tmp_path))
    want = structures.canonical_distances_and_dihedrals(src, angles=structures.EXHAUSTIVE_ANGLES,
                                                        distances=structures.MINIMAL_DISTS).values[:4].astype(np.float32)
    assert got.shape == (3, 4, 6)
    for i in range(3):
        assert np.array_equal(np.isnan(got[i].numpy()), np.isnan(want))
        assert np.allclose(got[i].numpy(), want, atol=1e-6, equal_nan=True)
    assert np.isfinite(got[0, 1:3].numpy()).all() and np.abs(np.nan_to_num(got.numpy())).max() <= np.pi
