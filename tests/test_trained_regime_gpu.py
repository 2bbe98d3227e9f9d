"""
The kernels in a trained model's regime (tests/trained_regime_cases.py): peaked softmax, saturated GELU.  Needs an MI355X:  pytest -m gpu

synthetic_model's weights keep |score| <= 1.1, so every p is about 1 / L, every online-softmax alpha about 1 and GELU close to
linear -- and a score computed as plain fp16 x fp16 stays under every gate of tests/test_gpu_parity.py.  Here the same kernels run
on weights whose scores span tens (moderate) to hundreds (sharp) of logits; tests/test_trained_regime.py asserts on the CPU that the
weights are in that regime and that a lost lo plane of q or k then misses the gate of every case below more than fivefold.

No new tolerance.  The criterion is _rel_gate: the device error relative to max|want64| must be <= max(4 e_ref, 2e-6), e_ref being
the fp32 oracle's own error on the same case, computed in the test.  Every test first asserts, through _assert_plan_launches, that
each forced plan launches the kernels it names.
"""
import numpy as np
import pytest
import torch

import trained_regime_cases as cases
from foldingdiff_amd import beta_schedules
from oracle import ref_sampling
from test_gpu_parity import (FWD_TOL, STEP_TOL, _RECIPE_SHAPES, _assert_plan_launches, _capture_stages, _debug_read,
                             _fused_kernel_takes, _inputs, _mask, _pair, _record, _rel_gate, _reset_plan, _scales, _step)
from test_persistent_passes_gpu import _assert_grids, _assert_items_differ, _assert_shape_loops, _set_grid, _want_grids
from test_trained_regime import FWD_TOL as _CPU_FWD_TOL

pytestmark = pytest.mark.gpu

_EVERY_PLAN = [(fa, ffu, packed) for packed in (0, 1) for fa in (0, 1, 2) for ffu in (0, 1, 2)]


def _regime_models(name, regime, T=1000, precision="f16x3", edit=None):
    """(architecture, fp32 oracle, fp64 oracle, product model) of cases.MODELS[name] in `regime`; edit(sd) changes the state dict
    before all three load it."""
    arch, _ = cases.MODELS[name]
    o32, o64, pm = _pair(seed=cases.SEED, precision=precision, **arch)
    sd = cases.state_dict_for(name, regime)
    if edit is not None:
        edit(sd)
    cases.load_both(o32, o64, sd)
    pm.load_state_dict(sd)
    pm.to("cuda:0")
    o64.time_table = o32.time_embed(torch.arange(T)).double()
    return arch, o32, o64, pm


def test_the_cases_module_agrees_with_the_parity_module(gpu):
    assert cases.SHAPES_A == _RECIPE_SHAPES and _CPU_FWD_TOL == FWD_TOL
    got, w32, w64 = np.array([1.0, 2.5]), np.array([1.0, 2.0 + 1e-6]), np.array([1.0, 2.0])
    assert cases.rel_gate(got, w32, w64) == _rel_gate(got, w32, w64)
    assert torch.equal(cases.inputs(3, 7, seed=2), _inputs(3, 7, seed=2)) and torch.equal(cases.mask_of([7, 1], 7), _mask([7, 1], 7))


# ---------------------------------------------------------------------------------------------- A. every launch plan
@pytest.mark.parametrize("regime", cases.REGIMES)
@pytest.mark.parametrize("name", ["d384", "d192"])
def test_forward_every_plan(gpu, name, regime):
    """fuse_attn (0, 1, 2) x fuse_ffn (0, 1, 2) x padded / packed rows, the three shapes, two inputs each, t at both ends of the
    schedule.  fuse_attn 2 stays bit-identical to 0; the other plan-to-plan differences are recorded, not gated (the 2e-6 / 4e-6
    alarms of tests/test_gpu_parity.py were measured at the other regime, and two plans inside the gate are within two gates of
    each other anyway)."""
    arch, o32, o64, pm = _regime_models(name, regime)
    hidden, layers = arch["hidden"], arch["layers"]
    for B, L, lens in cases.SHAPES_A:
        _assert_plan_launches(pm, layers, B, L, lens, _EVERY_PLAN)
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    try:
        for B, L, lens in cases.SHAPES_A:
            mask = _mask(lens, L)
            valid = mask.bool().numpy()
            worst = dict(rel_err=0.0, e_ref=0.0, err_over_gate=0.0, attn16_vs_two_kernel=0.0, ffn16_vs_gemms=0.0, tail_vs_gemms=0.0)
            fam = {}
            for rep in (1, 2):
                x = _inputs(B, L, seed=rep)
                for tval in (0, 999):
                    t = torch.full((B,), tval, dtype=torch.long)
                    want32 = o32(x, t, attention_mask=mask).numpy()[valid]
                    want64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
                    outs = {}
                    for fa, ffu, packed in _EVERY_PLAN:
                        if fa == 2 and not 96 < L <= 128:   # (the 32-row kernel takes 97..128 positions)
                            continue
                        pm.set_option("varlen", packed)
                        pm.set_option("fuse_attn", fa)
                        pm.set_option("fuse_ffn", ffu)
                        assert fa == 0 or _fused_kernel_takes(pm, L), (fa, L)
                        got = pm(x, t, attention_mask=mask).numpy()[valid]
                        outs[packed, fa, ffu] = got
                        e_dev, e_ref, tol = _rel_gate(got, want32, want64)
                        print(f"trained {name} {regime} {B}x{L} rep{rep} t{tval} packed{packed} fuse_attn{fa} fuse_ffn{ffu}: "
                              f"rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
                        worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref),
                                     err_over_gate=max(worst["err_over_gate"], e_dev / tol))
                        fam[f"attn{fa}_ffn{ffu}"] = max(fam.get(f"attn{fa}_ffn{ffu}", 0.0), e_dev)
                        assert np.isfinite(got).all() and e_dev <= tol, \
                            f"{B} x {L}, inputs {rep}, t {tval}, varlen {packed}, fuse_attn {fa}, fuse_ffn {ffu}: rel_err {e_dev:.3e} > {tol:.3e}"
                    for (packed, fa, ffu), got in outs.items():
                        if fa == 2:
                            assert np.array_equal(got, outs[packed, 0, ffu]), \
                                f"{B} x {L}, inputs {rep}, t {tval}, varlen {packed}, fuse_ffn {ffu}: fuse_attn 2 is not fuse_attn 0 bit for bit"
                        if fa == 1:
                            worst["attn16_vs_two_kernel"] = max(worst["attn16_vs_two_kernel"], float(np.abs(got - outs[packed, 0, ffu]).max()))
                        if ffu:
                            key = "ffn16_vs_gemms" if ffu == 1 else "tail_vs_gemms"
                            worst[key] = max(worst[key], float(np.abs(got - outs[packed, fa, 0]).max()))
            _record(f"trained_fwd_{name}_{regime}_{B}x{L}", **worst, **fam)
    finally:
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- B. no fused attention
@pytest.mark.parametrize("regime", cases.REGIMES)
@pytest.mark.parametrize("name", ["rkq384", "long384", "abs192", "head64"])
def test_forward_without_a_fused_attention(gpu, name, regime):
    """relative_key_query at L = 128 (the key term's r_scale_k), relative_key at L = 200 (attention_img.hip with two key tiles:
    the CPU test asserts that alpha really rescales), absolute positions, head size 64 (attention_gen.hip): the q|k|v GEMM and
    the attention kernel under every feed-forward plan the model has, padded and packed rows."""
    arch, o32, o64, pm = _regime_models(name, regime)
    layers = arch["layers"]
    ffn_plans = (0, 1, 2) if arch["hidden"] in (192, 384) and arch["ff"] == 2 * arch["hidden"] else (0,)   # (ffn16_supported)
    (B, L, lens), = cases.SHAPES[name]
    _assert_plan_launches(pm, layers, B, L, lens, [(0, ffu, packed) for packed in (0, 1) for ffu in ffn_plans])
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    x, mask = _inputs(B, L, seed=1), _mask(lens, L)
    valid = mask.bool().numpy()
    worst = dict(rel_err=0.0, e_ref=0.0, err_over_gate=0.0)
    try:
        for fa in (1, 2):
            pm.set_option("fuse_attn", fa)
            assert not _fused_kernel_takes(pm, L), fa
        pm.set_option("fuse_attn", -1)
        for tval in (42, 999):
            t = torch.full((B,), tval, dtype=torch.long)
            want32 = o32(x, t, attention_mask=mask).numpy()[valid]
            want64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
            for packed in (0, 1):
                pm.set_option("varlen", packed)
                for ffu in ffn_plans:
                    pm.set_option("fuse_ffn", ffu)
                    got = pm(x, t, attention_mask=mask).numpy()[valid]
                    e_dev, e_ref, tol = _rel_gate(got, want32, want64)
                    print(f"trained {name} {regime} L={L} t{tval} packed{packed} fuse_ffn{ffu}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
                    worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref),
                                 err_over_gate=max(worst["err_over_gate"], e_dev / tol))
                    assert np.isfinite(got).all() and e_dev <= tol, f"t {tval}, varlen {packed}, fuse_ffn {ffu}: rel_err {e_dev:.3e} > {tol:.3e}"
        _record(f"trained_fwd_{name}_{regime}_L{L}", **worst)
    finally:
        _reset_plan(pm)


@pytest.mark.parametrize("fuse_ln", [0, 1])
@pytest.mark.parametrize("regime", cases.REGIMES)
def test_forward_f32_precision(gpu, regime, fuse_ln):
    """precision "f32": attention_f32.hip with its split log2e and the clamp of exponents at -200 (sharp: the CPU test asserts
    that valid scores lie more than 200 below their row maximum), at L = 128 and 33, fuse_ln 0 and 1."""
    arch, o32, o64, pm = _regime_models("f32_192", regime, precision="f32")
    pm.set_option("fuse_ln", fuse_ln)
    for B, L, lens in cases.SHAPES["f32_192"]:
        _assert_plan_launches(pm, arch["layers"], B, L, lens, [(0, 0, 0)])
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    assert pm.precision == "f32"
    for B, L, lens in cases.SHAPES["f32_192"]:
        x, mask = _inputs(B, L, seed=1), _mask(lens, L)
        valid = mask.bool().numpy()
        worst = dict(rel_err=0.0, e_ref=0.0, err_over_gate=0.0)
        for tval in (42, 999):
            t = torch.full((B,), tval, dtype=torch.long)
            want32 = o32(x, t, attention_mask=mask).numpy()[valid]
            want64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
            got = pm(x, t, attention_mask=mask).numpy()[valid]
            e_dev, e_ref, tol = _rel_gate(got, want32, want64)
            print(f"trained f32 {regime} fuse_ln{fuse_ln} {B}x{L} t{tval}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
            worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref), err_over_gate=max(worst["err_over_gate"], e_dev / tol))
            assert np.isfinite(got).all() and e_dev <= tol, f"{B} x {L}, t {tval}: rel_err {e_dev:.3e} > {tol:.3e}"
        _record(f"trained_fwd_f32_{regime}_fuse{fuse_ln}_{B}x{L}", **worst)


# ---------------------------------------------------------------------------------------------- C. stage by stage
class _Stages:
    """The debug_stop / debug_layer / fd_debug_read walk of test_every_stage_of_every_layer_with_distinct_image_scales: stop slots
    embed 1, then per layer q|k|v 1, attention 1 (a fused attention launch takes both), attention.output 1, up 1, down 1 (ffn16
    takes the last two, the layer tail all three)."""

    def __init__(self, pm, arch, B, L, x, t, mask):
        self.pm, self.x, self.t, self.mask = pm, x, t, mask
        self.B, self.L, self.hidden = B, L, arch["hidden"]
        self.valid = mask.bool().numpy()
        self.cap_rows = (B * ((L + 7) // 8 * 8) + 127) // 128 * 128
        self.H, self.LTOT = arch["hidden"] // 32, 32 * ((L + 31) // 32)
        self.width = dict(h=arch["hidden"], h_out=arch["hidden"], a=arch["hidden"], ctx=arch["hidden"], g=arch["ff"], g_head=arch["hidden"])

    def run(self, stop):
        self.pm.set_option("debug_stop", stop)
        self.pm(self.x, self.t, attention_mask=self.mask)

    def read(self, name):
        B, L = self.B, self.L
        if name in "qkv":   # [B][H][padded L][32], the same under both row layouts
            a = _debug_read(self.pm, name, B * self.H * self.LTOT * 32).reshape(B, self.H, self.LTOT, 32)[:, :, :L]
            return a.transpose(0, 2, 1, 3).reshape(B, L, self.hidden)[self.valid]
        rows = _debug_read(self.pm, name, self.cap_rows * self.width[name]).reshape(self.cap_rows, self.width[name])
        ri = _debug_read(self.pm, "rowinfo", 2 * self.cap_rows).reshape(self.cap_rows, 2).astype(np.int64)
        out = np.full((B, L, self.width[name]), np.nan, np.float32)
        real = (ri[:, 0] >= 0) & (ri[:, 1] < L)   # (padded rows: the positions L .. ceil8(L) - 1 are rows of the image, not of the model)
        out[ri[real, 0], ri[real, 1]] = rows[real]
        return out[self.valid]


_STAGE_PLANS = ((0, 0), (1, 0), (1, 1), (1, 2))


@pytest.mark.parametrize("regime", cases.REGIMES)
def test_every_stage_of_every_layer(gpu, regime):
    """d 384, 5 x 128, t = 42: h, q, k, v, ctx, a, g, h_out of every layer and the head's GELU output against the fp64 oracle's
    activations, per tensor with the forward's criterion, under plans (fuse_attn, fuse_ffn) = (0, 0), (1, 0), (1, 1), (1, 2),
    padded and packed rows.  A miss is named by layer, stage and plan."""
    arch, o32, o64, pm = _regime_models("d384", regime, T=100)
    layers = arch["layers"]
    B, L, lens = cases.SHAPES_A[0]
    _assert_plan_launches(pm, layers, B, L, lens, [(fa, ffu, packed) for packed in (0, 1) for fa, ffu in _STAGE_PLANS])
    pm.prepare(beta_schedules.cosine_beta_schedule(100))
    x, mask = _inputs(B, L, seed=1), _mask(lens, L)
    t = torch.full((B,), 42, dtype=torch.long)
    cap32, _ = _capture_stages(o32, x, t, mask)
    cap64, _ = _capture_stages(o64, x.double(), t, mask.double())
    st = _Stages(pm, arch, B, L, x, t, mask)
    valid = st.valid
    worst = {}

    def check(name, li, plan):
        got, key = st.read(name), (name, li if name != "g_head" else 0)
        e_dev, e_ref, tol = _rel_gate(got, cap32[key][valid], cap64[key][valid])
        print(f"trained {regime} stage {name:6s} layer {li} plan {plan}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
        if e_dev / tol >= worst.get(name, (-1.0,))[0]:
            worst[name] = (e_dev / tol, e_dev, e_ref, li, str(plan))
        assert np.isfinite(got).all() and e_dev <= tol, f"layer {li}, stage {name}, plan {plan}: rel_err {e_dev:.3e} > {tol:.3e} (e_ref {e_ref:.3e})"

    try:
        for packed in (0, 1):
            pm.set_option("varlen", packed)
            for fa, ffu in _STAGE_PLANS:
                pm.set_option("fuse_attn", fa)
                pm.set_option("fuse_ffn", ffu)
                plan = dict(fuse_attn=fa, fuse_ffn=ffu, varlen=packed)
                for li in range(layers):
                    pm.set_option("debug_layer", li)
                    s0 = 1 + 5 * li
                    st.run(s0)
                    check("h", li, plan)
                    if fa == 0:
                        st.run(s0 + 1)
                        for name in "qkv":
                            check(name, li, plan)
                    st.run(s0 + 2)
                    check("ctx", li, plan)
                    if ffu < 2:
                        st.run(s0 + 3)
                        check("a", li, plan)
                    if ffu == 0:
                        st.run(s0 + 4)
                        check("g", li, plan)
                    st.run(s0 + 5)
                    check("h_out", li, plan)
                if (packed, fa, ffu) == (0, 0, 0):
                    st.run(1 + 5 * layers + 1)
                    check("g_head", layers - 1, plan)
        for name, (over, e_dev, e_ref, li, plan) in worst.items():
            _record(f"trained_stage_{regime}_{name}", err_over_gate=over, rel_err=e_dev, e_ref=e_ref, layer=li, plan=plan)
    finally:
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- D. one reverse step
@pytest.mark.parametrize("regime", cases.REGIMES)
@pytest.mark.parametrize("name,shape,packed", [("d192", 1, 1), ("d384", 2, 0)])
def test_one_reverse_step_teacher_forced(gpu, name, shape, packed, regime):
    """fd_p_sample_step teacher-forced on the fp64 oracle's state at t = 999, 400, 1, 0 (d 192 at 7 x 101 with packed rows, d 384
    at 3 x 7), plans (fused attention, layer tail), (two kernels, fused feed-forward) and the GEMMs.  The step adds
    c(t) x (error of the forward) to the posterior mean, c(t) = beta_t / (sqrt(1 - alphabar_t) sqrt(alpha_t)) from the schedule:
    the circular error must be <= c(t) x the case's forward bound in absolute units + 1e-6, and <= STEP_TOL wherever that is
    the smaller of the two.
    The reference is the fp64 oracle's prediction put through p_sample and the wrap in fp32, the device's own arithmetic for
    that closed form (test_wrap_on_the_device_is_bit_identical_to_the_reference): the update and the wrap of angles near pi
    round by 1e-6 in fp32 whatever the prediction (the fp32 oracle's step is 1.0e-6 from the all-fp64 step at t = 1 and 0, where
    c(t) is below 0.01), which is not what c(t) x the forward bound measures.  The distance from the all-fp64 step is printed."""
    arch, o32, o64, pm = _regime_models(name, regime)
    B, L, lens = cases.SHAPES_A[shape]
    plans = [(1, 2), (0, 1), (0, 0)]
    _assert_plan_launches(pm, arch["layers"], B, L, lens, [(fa, ffu, packed) for fa, ffu in plans])
    betas = beta_schedules.cosine_beta_schedule(1000)
    h = pm.prepare(betas)
    mask = _mask(lens, L)
    valid = mask.bool().numpy()
    x = _inputs(B, L, seed=8)
    g = torch.Generator().manual_seed(5)
    worst = {}
    try:
        pm.set_option("varlen", packed)
        for tval in (999, 400, 1, 0):
            t = torch.full((B,), tval, dtype=torch.long)
            z = torch.randn(B, L, 6, generator=g)
            eps32 = o32(x, t, attention_mask=mask).numpy()[valid]
            eps64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
            _, e_ref, gate = _rel_gate(eps32, eps32, eps64)
            c = cases.eps_coefficient(betas.numpy(), tval)
            bound = c * gate * float(np.abs(eps64).max()) + 1e-6
            full64 = o64(x.double(), t, attention_mask=mask.double())
            want = ref_sampling.wrap(ref_sampling.p_sample(lambda *a, **k: full64.float(), x, t, lens, betas, z), -torch.pi, torch.pi)
            all64 = ref_sampling.wrap(ref_sampling.p_sample(lambda *a, **k: full64, x.double(), t, lens, betas.double(), z.double()),
                                      -torch.pi, torch.pi)
            for fa, ffu in plans:
                pm.set_option("fuse_attn", fa)
                pm.set_option("fuse_ffn", ffu)
                out = _step(pm, h, x.numpy(), tval, lens, z.numpy())
                e = float(ref_sampling.circ_dist(out[valid], want.numpy()[valid]).max())
                e_all64 = float(ref_sampling.circ_dist(out[valid], all64.numpy()[valid]).max())
                print(f"trained step {name} {regime} t{tval} fuse_attn{fa} fuse_ffn{ffu}: {e:.3e}  bound {bound:.3e}  c(t) {c:.4g}  e_ref {e_ref:.3e}"
                      f"  (against the update in fp64 too: {e_all64:.3e})")
                if e / bound >= worst.get(tval, (-1.0,))[0]:
                    worst[tval] = (e / bound, e, bound, c)
                assert np.isfinite(out[valid]).all() and e <= bound, (tval, fa, ffu, e, bound)
                assert e <= STEP_TOL or bound > STEP_TOL, (tval, fa, ffu, e)
            x = want.float()
        for tval, (over, e, bound, c) in worst.items():
            _record(f"trained_step_{name}_{regime}_t{tval}", err_over_bound=over, max=e, bound=bound, eps_coefficient=c)
    finally:
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- E. later items
@pytest.mark.parametrize("packed", [0, 1])
def test_later_items_of_the_persistent_kernels(gpu, packed):
    """d 192, sharp, lengths long -> one row -> long and across the 64-key boundary, on 1 and 2 workgroups (option debug_grid):
    every sequence after a workgroup's first is computed by the item-to-item code, and a next sequence masked with the previous
    one's length matters far more when the mass sits on few keys.  Plans (fused 16-row attention, layer tail) and (fused 32-row
    attention, fused feed-forward); _rel_gate against the oracles and the same bits as the same plan on the full grid."""
    arch, o32, o64, pm = _regime_models("d192", "sharp")
    B, L, lens = cases.SHAPES["d192"][3]
    assert lens == [128, 1, 100, 33, 128, 64, 65]
    plans = [(1, 2), (2, 1)]
    _assert_shape_loops(B, L, lens, (1, 2))
    _assert_plan_launches(pm, arch["layers"], B, L, lens, [(fa, ffu, packed) for fa, ffu in plans])
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    mask = _mask(lens, L)
    valid = mask.bool().numpy()
    worst = dict(rel_err=0.0, e_ref=0.0, err_over_gate=0.0)
    try:
        pm.set_option("varlen", packed)
        for rep, tval in ((1, 999), (2, 0)):
            x = _inputs(B, L, seed=rep)
            _assert_items_differ(x, lens, 1)
            _assert_items_differ(x, lens, 2)
            t = torch.full((B,), tval, dtype=torch.long)
            want32 = o32(x, t, attention_mask=mask).numpy()[valid]
            want64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
            base = {}
            for cap in (0, 1, 2):
                _set_grid(pm, cap)
                for fa, ffu in plans:
                    pm.set_option("fuse_attn", fa)
                    pm.set_option("fuse_ffn", ffu)
                    assert _fused_kernel_takes(pm, L), fa
                    where = f"inputs {rep}, t {tval}, varlen {packed}, fuse_attn {fa}, fuse_ffn {ffu}, debug_grid {cap}"
                    got = pm(x, t, attention_mask=mask).numpy()[valid]
                    _assert_grids(pm, _want_grids(cap, B, L, fa, ffu), where)
                    e_dev, e_ref, tol = _rel_gate(got, want32, want64)
                    print(f"trained capped {where}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
                    worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref), err_over_gate=max(worst["err_over_gate"], e_dev / tol))
                    assert np.isfinite(got).all() and e_dev <= tol, f"{where}: rel_err {e_dev:.3e} > {tol:.3e}"
                    if cap == 0:
                        base[fa, ffu] = got
                    else:
                        same = got == base[fa, ffu]
                        assert same.all(), f"{where}: {int((~same).sum())} values differ from the full grid's, max {float(np.abs(got - base[fa, ffu]).max()):.3e}"
        _record(f"trained_capped_grid_192_sharp_packed{packed}", **worst)
    finally:
        _set_grid(pm, 0)
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- F. row sums
_IDENTITY_LAYER = 1


def _identity_value(sd):
    w = sd[f"encoder.layer.{_IDENTITY_LAYER}.attention.self.value.weight"]
    w.copy_(torch.eye(w.shape[0]))
    sd[f"encoder.layer.{_IDENTITY_LAYER}.attention.self.value.bias"].zero_()


@pytest.mark.parametrize("regime", cases.REGIMES)
def test_context_with_an_identity_value_projection(gpu, regime):
    """One layer's `value` is the identity with zero bias (in the state dict: the oracles get the same weights), so that layer's
    ctx is sum_keys p . h, a weighted mean of O(1) rows: a wrong normaliser l_run shows in it directly instead of being washed
    through a random projection.  ctx of that layer against the fp64 oracle with the per-tensor criterion, two-kernel and fused
    attention, padded and packed rows, 5 x 128 and 3 x 7; every element finite -- sharp at 3 x 7 has rows where one key holds all
    the mass to the last bit (asserted on the fp64 probabilities)."""
    arch, o32, o64, pm = _regime_models("d384", regime, T=100, edit=_identity_value)
    li, layers = _IDENTITY_LAYER, arch["layers"]
    assert torch.equal(o64.encoder.layer[li].attention.self.value.weight, torch.eye(arch["hidden"], dtype=torch.float64))
    plans = [(0, 0), (1, 0)]
    shapes = (cases.SHAPES_A[0], cases.SHAPES_A[2])
    for B, L, lens in shapes:
        _assert_plan_launches(pm, layers, B, L, lens, [(fa, ffu, packed) for packed in (0, 1) for fa, ffu in plans])
    pm.prepare(beta_schedules.cosine_beta_schedule(100))
    try:
        for B, L, lens in shapes:
            x, mask = _inputs(B, L, seed=1), _mask(lens, L)
            t = torch.full((B,), 42, dtype=torch.long)
            cap32, _ = _capture_stages(o32, x, t, mask)
            cap64, _ = _capture_stages(o64, x.double(), t, mask.double())
            st = _Stages(pm, arch, B, L, x, t, mask)
            valid = st.valid
            seen = []
            cases.forward_restated(o64, x.double(), t, mask.double(), seen=seen)
            pmax = seen[li][1].max(-1).values[mask.bool()[:, None, :].expand(-1, seen[li][1].shape[1], -1)]
            all_on_one_key = float((pmax == 1.0).double().mean())
            if regime == "sharp" and L == 7:
                assert all_on_one_key > 0
            # with the identity, ctx is the weighted mean of h: the oracle's own row sums are 1 to fp64
            hv = cap64[("h", li)]
            assert np.abs(cap64[("ctx", li)][valid]).max() <= np.abs(hv[valid]).max() * (1 + 1e-12)
            worst = dict(rel_err=0.0, e_ref=0.0, err_over_gate=0.0, rows_with_all_mass_on_one_key=all_on_one_key)
            pm.set_option("debug_layer", li)
            for packed in (0, 1):
                pm.set_option("varlen", packed)
                for fa, ffu in plans:
                    pm.set_option("fuse_attn", fa)
                    pm.set_option("fuse_ffn", ffu)
                    st.run(1 + 5 * li + 2)
                    got = st.read("ctx")
                    e_dev, e_ref, tol = _rel_gate(got, cap32[("ctx", li)][valid], cap64[("ctx", li)][valid])
                    print(f"trained {regime} identity-value ctx {B}x{L} packed{packed} fuse_attn{fa}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
                    worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref), err_over_gate=max(worst["err_over_gate"], e_dev / tol))
                    assert np.isfinite(got).all(), f"{B} x {L}, varlen {packed}, fuse_attn {fa}: {int((~np.isfinite(got)).sum())} non-finite ctx elements"
                    assert e_dev <= tol, f"{B} x {L}, varlen {packed}, fuse_attn {fa}: ctx rel_err {e_dev:.3e} > {tol:.3e} (e_ref {e_ref:.3e})"
            _record(f"trained_ctx_identity_value_{regime}_{B}x{L}", **worst)
    finally:
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- G. image scales
@pytest.mark.parametrize("name", ["d384", "d192", "rkq384", "long384"])
def test_image_scales_follow_the_gains(gpu, name):
    """fd_debug_read("scales") in both regimes: s_q, s_k and the distance table's scale are positive powers of two that moved from
    their plain-weights values in the direction of the gains (an image holds value x scale, so a larger gain is a smaller scale),
    and the largest |q|, |k| and distance-table entry of the fp64 oracle times the scale stays below the fp16 maximum.  (That the
    lo planes behind these scales are not flushed is test_every_stage_of_every_layer's q and k.)"""
    arch, gains = cases.MODELS[name]
    layers = arch["layers"]
    sc = {}
    for regime in ("plain",) + cases.REGIMES:
        _, o32, o64, pm = _regime_models(name, regime, T=100)
        pm.prepare(beta_schedules.cosine_beta_schedule(100))
        sc[regime] = [_scales(pm, li) for li in range(layers)]
        if regime == "plain":
            continue
        gq, gk, gd, _ = gains[regime]
        top = {"q": 0.0, "k": 0.0}
        for B, L, lens in cases.SHAPES[name]:
            x, mask = _inputs(B, L, seed=1), _mask(lens, L)
            cap64, _ = _capture_stages(o64, x.double(), torch.full((B,), 42, dtype=torch.long), mask.double())
            for li in range(layers):
                for key, sname in (("q", "s_q"), ("k", "s_k")):
                    stored = float(np.abs(cap64[(key, li)][mask.bool().numpy()]).max()) * sc[regime][li][sname]
                    top[key] = max(top[key], stored)
                    assert stored < 65504, (regime, li, key, stored)
        for li in range(layers):
            s, s0 = sc[regime][li], sc["plain"][li]
            for sname, gain in (("s_q", gq), ("s_k", gk), ("demb_s", gd)):
                assert s[sname] > 0 and np.log2(s[sname]) == round(np.log2(s[sname])), (regime, li, sname, s[sname])
                assert s[sname] < s0[sname], f"{regime}, layer {li}: {sname} = {s[sname]} did not move down from {s0[sname]} (gain {gain})"
            table = float(o64.encoder.layer[li].attention.self.distance_embedding.weight.detach().abs().max()) * s["demb_s"]
            assert table < 65504, (regime, li, table)
            for other in ("s_h", "s_v", "s_a"):   # what the gains do not name keeps its scale
                assert s[other] == s0[other], (regime, li, other, s[other], s0[other])
        _record(f"trained_scales_{name}_{regime}", s_q=sc[regime][0]["s_q"], s_k=sc[regime][0]["s_k"], demb_s=sc[regime][0]["demb_s"],
                plain_s_q=sc["plain"][0]["s_q"], plain_s_k=sc["plain"][0]["s_k"], plain_demb_s=sc["plain"][0]["demb_s"],
                largest_stored_q=top["q"], largest_stored_k=top["k"])
    for li in range(layers):   # sharp at or below moderate wherever its gain is at or above
        for sname, i in (("s_q", 0), ("s_k", 1), ("demb_s", 2)):
            lo, hi = gains["moderate"][i], gains["sharp"][i]
            a, b = sc["moderate"][li][sname], sc["sharp"][li][sname]
            assert (b < a) if hi > lo else (b == a) if hi == lo else (b > a), (li, sname, a, b)
