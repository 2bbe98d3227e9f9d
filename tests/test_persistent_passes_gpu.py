"""
The persistent fused kernels' SECOND AND LATER items against the oracle.  Needs an MI355X:  pytest -m gpu

seq_attn16.hip / seq_attn.hip (one workgroup walks the sequences blockIdx.x, + gridDim.x, ...) and ffn16.hip (one workgroup walks
128-row passes the same way) load the next item under the end of the current one: the next hidden state / hi plane into registers
the current rows just left, the lo plane block by block behind the stores, the layer tail's residual straight into the
accumulators, the weight stream wrapping with two stages in flight.  With one workgroup per compute unit a batch needs more items
than the device has CUs before any of that code runs, so every oracle gate of tests/test_gpu_parity.py stays within a workgroup's
first item.  Here option "debug_grid" caps the workgroup count (host side only: the kernels are the production ones), so 5 to 7
items already give a workgroup three of them, and two tests run more than two rounds of items on the real grid.

No test here is allowed to be empty: each asserts first which kernels launched, on which grid (fd_debug_read "grids"), how many
items the fullest workgroup got, and that items which follow each other differ.  No new tolerance: every gate is one of
tests/test_gpu_parity.py's (_rel_gate, FWD_TOL, STEP_TOL, the 2e-6 / 4e-6 plan-to-plan alarms) or bit equality -- a row's
arithmetic does not depend on the workgroup that computes it nor on what that workgroup computed before.
"""
import numpy as np
import pytest
import torch

from foldingdiff_amd import _binding, beta_schedules, sampling
from oracle import ref_sampling
from test_gpu_parity import (FWD_TOL, STEP_TOL, _LN_EPS, _RECIPE_MODELS, _assert_plan_launches, _assert_scales_differ, _c3_chunks,
                             _debug_read, _fused_kernel_takes, _inputs, _launches_per_step, _mask, _pair, _recipe_pair, _record,
                             _rel_gate, _reset_plan, _share_time_table, _step)

pytestmark = pytest.mark.gpu

# chosen for the transitions: long -> one row -> long and both directions across the 64-key boundary (waves gain and lose rows);
# padded passes that are not sequence-aligned (6 x 104 rows); several sequences per pass (only the attention kernels loop)
_SHAPES = ((7, 128, [128, 1, 100, 33, 128, 64, 65]), (6, 101, [101, 50, 99, 3, 100, 77]), (5, 7, [7, 1, 3, 7, 2]))


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ceil(n, m):
    return (n + m - 1) // m * m


def _passes(B, L, lens, packed):
    """128-row passes the feed-forward kernel walks: the token rows (padded: B sequences of ceil8(L) rows; packed: each length rounded
    up to 8) rounded up to whole passes, as the workspace's row table counts them."""
    rows = sum(_ceil(n, 8) for n in lens) if packed else B * _ceil(L, 8)
    return _ceil(rows, 128) // 128


def _launch_passes(B, L):
    """FfnArgs::panels, what the launcher sizes the grid by: the workspace's capacity (packed rows: a bound)."""
    return _ceil(B * _ceil(L, 8), 128) // 128


def _most_items(items, grid):
    """Items of the fullest workgroup when `grid` workgroups walk `items` (workgroup 0 takes 0, grid, 2 grid, ...)."""
    return (items + grid - 1) // grid


def _want_grids(cap, B, L, fa, ffu):
    """(seq_attn16, seq_attn, ffn16) x-grids of a forward under plan (fa, ffu) at option debug_grid = cap, as persistent_grid() of
    csrc/launch_common.h computes them; None: the plan does not launch that kernel."""
    lim = min(cap, _ncu()) if cap > 0 else _ncu()
    return (min(lim, B) if fa == 1 else None, min(lim, B) if fa == 2 and 96 < L <= 128 else None,
            min(lim, _launch_passes(B, L)) if ffu else None)


def _assert_grids(pm, want, where):
    got = [int(v) for v in _debug_read(pm, "grids", 3)]
    for name, g, w in zip(("seq_attn16", "seq_attn", "ffn16"), got, want):
        assert w is None or g == w, f"{where}: {name} ran on {g} workgroups, not {w} (all three: {got})"


def _set_grid(pm, cap):
    pm.set_option("debug_grid", cap)


def _assert_items_differ(x, lens, step):
    """Sequences `step` apart (consecutive items of a workgroup) have different inputs on their common positions."""
    for i in range(len(lens) - step):
        n = min(lens[i], lens[i + step])
        assert not torch.equal(x[i, :n], x[i + step, :n]), (i, step)


def _plans(L):
    return [(fa, ffu, packed) for packed in (0, 1) for fa in (0, 1, 2) for ffu in (0, 1, 2) if fa != 2 or 96 < L <= 128]


def _assert_shape_loops(B, L, lens, caps):
    """Cap 1 gives some workgroup >= 3 items, cap 2 >= 2: sequences for the attention kernels; passes, padded and packed, for the
    feed-forward kernel (not at L = 7, where the whole batch is one pass and only the attention kernels loop)."""
    need = {1: 3, 2: 2, 3: 2}
    for cap in caps:
        assert _most_items(B, min(cap, B)) >= need[cap], (B, cap)
        if L > 96:
            for packed in (0, 1):
                n = _passes(B, L, lens, packed)
                assert n <= _launch_passes(B, L) and _most_items(n, min(cap, _launch_passes(B, L))) >= need[cap], (B, L, packed, cap, n)
    if 3 in caps and B == 7:
        assert B % 3 == 1   # an uneven last round: one workgroup with three sequences, two with two


# ---------------------------------------------------------------------------------------------- (a) forward, every plan
@pytest.mark.parametrize("hidden,heads,ff,layers", _RECIPE_MODELS)
def test_forward_every_plan_on_a_capped_grid(gpu, hidden, heads, ff, layers):
    """Every launch plan -- fuse_attn (0, 1, 2) x fuse_ffn (0, 1, 2) x padded / packed rows -- of the recipe models on 1, 2 and 3
    workgroups: every sequence after a workgroup's first is computed by the item-to-item code.  Gates per forward: _rel_gate against
    the fp32 and fp64 oracles on every valid position, and the same bits as the same plan on the full grid.  Every shape twice with
    different inputs, t at both ends of the schedule.
    On the fp64 oracle alone, first: for shape one, any two sequences' outputs differ by more than 100 x the gate on their common
    valid positions, so a workgroup that stored an earlier item's result for a later one cannot pass."""
    o32, o64, pm = _recipe_pair(hidden, heads, ff, layers)
    T = 1000
    _share_time_table(o64, o32, T)
    caps = (1, 2, 3)
    for B, L, lens in _SHAPES:
        _assert_shape_loops(B, L, lens, caps)
        _assert_plan_launches(pm, layers, B, L, lens, _plans(L))
    pm.prepare(beta_schedules.cosine_beta_schedule(T))
    _assert_scales_differ(pm, layers)
    try:
        for si, (B, L, lens) in enumerate(_SHAPES):
            mask = _mask(lens, L)
            valid = mask.bool().numpy()
            worst = dict(rel_err=0.0, e_ref=0.0, least_pair_distance_over_gate=np.inf)
            for rep in (1, 2):
                x = _inputs(B, L, seed=rep)
                for step in (1, 2, 3):
                    _assert_items_differ(x, lens, step)
                for tval in (0, 999):
                    t = torch.full((B,), tval, dtype=torch.long)
                    full32 = o32(x, t, attention_mask=mask).numpy()
                    full64 = o64(x.double(), t, attention_mask=mask.double()).numpy()
                    want32, want64 = full32[valid], full64[valid]
                    if si == 0:   # (cap 1: every pair of sequences shares the workgroup)
                        _, _, tol = _rel_gate(want32, want32, want64)
                        gate = tol * np.abs(want64).max()
                        for i in range(B):
                            for j in range(i + 1, B):
                                n = min(lens[i], lens[j])
                                apart = float(np.abs(full64[i, :n] - full64[j, :n]).max())
                                worst["least_pair_distance_over_gate"] = min(worst["least_pair_distance_over_gate"], apart / gate)
                                assert apart >= 100 * gate, (rep, tval, i, j, apart, gate)
                    base = {}
                    for cap in (0,) + caps:
                        _set_grid(pm, cap)
                        for fa, ffu, packed in _plans(L):
                            pm.set_option("varlen", packed)
                            pm.set_option("fuse_attn", fa)
                            pm.set_option("fuse_ffn", ffu)
                            assert fa == 0 or _fused_kernel_takes(pm, L), (fa, L)
                            where = f"{B} x {L}, inputs {rep}, t {tval}, varlen {packed}, fuse_attn {fa}, fuse_ffn {ffu}, debug_grid {cap}"
                            got = pm(x, t, attention_mask=mask).numpy()[valid]
                            _assert_grids(pm, _want_grids(cap, B, L, fa, ffu), where)
                            if cap == 0:
                                base[fa, ffu, packed] = got
                                continue
                            e_dev, e_ref, tol = _rel_gate(got, want32, want64)
                            print(f"capped fwd d={hidden} {where}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}")
                            worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref))
                            assert np.isfinite(got).all() and e_dev <= tol, f"{where}: rel_err {e_dev:.3e} > {tol:.3e}"
                            same = got == base[fa, ffu, packed]
                            assert same.all(), f"{where}: {int((~same).sum())} values differ from the full grid's, " \
                                               f"max {float(np.abs(got - base[fa, ffu, packed]).max()):.3e}"
            if si:
                del worst["least_pair_distance_over_gate"]
            _record(f"fwd_capped_grid_{hidden}_{B}x{L}", **worst)
    finally:
        _set_grid(pm, 0)
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- (b) a real LayerNorm eps
@pytest.mark.parametrize("hidden,heads,ff,layers", [(384, 12, 768, 3), (192, 6, 384, 2)])
def test_forward_layer_norm_eps_on_a_capped_grid(gpu, hidden, heads, ff, layers):
    """layer_norm_eps = 1e-2 (the models of test_forward_layer_norm_eps) on 1 and 2 workgroups: the fused feed-forward kernel reads
    eps, and the layer tail eps1, inside its pass loop.  Fused attention with the fused feed-forward and with the layer tail, padded
    and packed rows; the two gates of test_forward_every_plan_on_a_capped_grid plus that test's FWD_TOL against both oracles."""
    o32, o64, pm = _pair(hidden=hidden, heads=heads, ff=ff, layers=layers, maxpos=128, seed=3, precision="f16x3", ln_eps=_LN_EPS)
    T = 100
    _share_time_table(o64, o32, T)
    B, L, lens = _SHAPES[0]
    plans = [(1, ffu, packed) for packed in (0, 1) for ffu in (1, 2)]
    _assert_shape_loops(B, L, lens, (1, 2))
    _assert_plan_launches(pm, layers, B, L, lens, plans)
    pm.prepare(beta_schedules.cosine_beta_schedule(T))
    x, mask = _inputs(B, L, seed=1), _mask(lens, L)
    _assert_items_differ(x, lens, 1)
    _assert_items_differ(x, lens, 2)
    valid = mask.bool().numpy()
    t = torch.full((B,), 42, dtype=torch.long)
    want32 = o32(x, t, attention_mask=mask).numpy()[valid]
    want64 = o64(x.double(), t, attention_mask=mask.double()).numpy()[valid]
    worst = dict(rel_err=0.0, e_ref=0.0, max_abs=0.0)
    try:
        base = {}
        for cap in (0, 1, 2):
            _set_grid(pm, cap)
            for fa, ffu, packed in plans:
                pm.set_option("varlen", packed)
                pm.set_option("fuse_attn", fa)
                pm.set_option("fuse_ffn", ffu)
                where = f"ln_eps d={hidden}, varlen {packed}, fuse_attn {fa}, fuse_ffn {ffu}, debug_grid {cap}"
                got = pm(x, t, attention_mask=mask).numpy()[valid]
                _assert_grids(pm, _want_grids(cap, B, L, fa, ffu), where)
                if cap == 0:
                    base[ffu, packed] = got
                    continue
                e_dev, e_ref, tol = _rel_gate(got, want32, want64)
                e32, e64 = float(np.abs(got - want32).max()), float(np.abs(got - want64).max())
                print(f"capped {where}: rel_err {e_dev:.3e}  e_ref {e_ref:.3e}  abs {e32:.3e} {e64:.3e}")
                worst.update(rel_err=max(worst["rel_err"], e_dev), e_ref=max(worst["e_ref"], e_ref), max_abs=max(worst["max_abs"], e32, e64))
                assert np.isfinite(got).all() and e_dev <= tol, f"{where}: rel_err {e_dev:.3e} > {tol:.3e}"
                assert e32 <= FWD_TOL and e64 <= FWD_TOL, (where, e32, e64)
                assert np.array_equal(got, base[ffu, packed]), f"{where}: max {float(np.abs(got - base[ffu, packed]).max()):.3e} from the full grid"
        _record(f"fwd_capped_grid_ln_eps_{hidden}", **worst)
    finally:
        _set_grid(pm, 0)
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- (c) reverse steps
def test_steps_on_a_capped_grid(gpu):
    """fd_p_sample_step of the d_model 192 recipe model on 1 and 2 workgroups, teacher-forced down the schedule under the plans
    (fused attention, layer tail) and (two-kernel attention, fused feed-forward), against the oracle's p_sample + wrap on every
    sequence.  Then sample_on_device (graph replay) at debug_grid 0, 1, 2: the three histories are the same bits on valid positions
    -- the capped grid through graph capture, and the re-capture after the option changed."""
    hidden, heads, ff, layers = _RECIPE_MODELS[1]
    o32, _, pm = _recipe_pair(hidden, heads, ff, layers)
    T = 1000
    betas = beta_schedules.cosine_beta_schedule(T)
    B, L, lens = _SHAPES[0]
    _assert_shape_loops(B, L, lens, (1, 2))
    _assert_plan_launches(pm, layers, B, L, lens, [(1, 2, 0), (0, 1, 0)])
    h = pm.prepare(betas)
    _assert_scales_differ(pm, layers)
    x = _inputs(B, L, seed=8)
    _assert_items_differ(x, lens, 1)
    _assert_items_differ(x, lens, 2)
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    try:
        for tval in (999, 400, 1, 0):
            z = torch.randn(B, L, 6, generator=g)
            want = ref_sampling.wrap(ref_sampling.p_sample(o32, x, torch.full((B,), tval, dtype=torch.long), lens, betas, z), -torch.pi, torch.pi)
            for cap in (1, 2):
                _set_grid(pm, cap)
                for fa, ffu in ((1, 2), (0, 1)):
                    pm.set_option("fuse_attn", fa)
                    pm.set_option("fuse_ffn", ffu)
                    out = _step(pm, h, x.numpy(), tval, lens, z.numpy())
                    _assert_grids(pm, _want_grids(cap, B, L, fa, ffu), (tval, cap, fa, ffu))
                    for i, n in enumerate(lens):
                        e = float(ref_sampling.circ_dist(out[i, :n], want[i, :n].numpy()).max())
                        worst = max(worst, e)
                        assert e <= STEP_TOL, (tval, cap, fa, ffu, i, e)
            x = want
        _record("step_capped_grid_recipe_192", max=worst)
        betas5 = beta_schedules.cosine_beta_schedule(5)
        xd = _inputs(B, L, seed=2).cuda()
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
        pm.set_option("fuse_attn", 1)
        pm.set_option("fuse_ffn", 2)
        hist = {}
        for cap in (0, 1, 2):
            _set_grid(pm, cap)
            hist[cap] = sampling.sample_on_device(pm, xd, ld, betas5, seed=4, full_history=True).cpu()
            _assert_grids(pm, _want_grids(cap, B, L, 1, 2), f"sample_on_device, debug_grid {cap}")
        assert tuple(hist[0].shape) == (5, B, L, 6)
        for i, n in enumerate(lens):
            assert torch.isfinite(hist[0][:, i, :n]).all()
            for cap in (1, 2):
                assert torch.equal(hist[cap][:, i, :n], hist[0][:, i, :n]), (cap, i)
    finally:
        _set_grid(pm, 0)
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- (d) the real grid
def _ragged_lens(B):
    return [40 + (13 * i) % 89 if i % 16 == 0 else 128 for i in range(B)]


def _full_grid_forwards(pm, o32, tag, B, L, lens, rounds):
    """Plans (fused attention, layer tail) and (two-kernel attention, fused feed-forward) on the full grid, padded and packed, two
    inputs: every valid position of every sequence against the fp32 oracle, and the plan-to-plan alarms of
    test_fused_projection_attention_kernels (2e-6) and test_fused_feed_forward_kernel (4e-6) down to the unfused plan."""
    ncu = _ncu()
    mask = _mask(lens, L)
    valid = mask.bool().numpy()
    t = torch.full((B,), 321, dtype=torch.long)
    worst = dict(max=0.0, attn16_vs_two_kernel=0.0, ffn16_vs_gemms=0.0)
    for rep in (1, 2):
        x = _inputs(B, L, seed=10 + rep)
        _assert_items_differ(x, lens, ncu)
        want = o32(x, t, attention_mask=mask).numpy()[valid]
        for packed in (0, 1):
            pm.set_option("varlen", packed)
            outs = {}
            for fa, ffu in ((0, 0), (1, 0), (1, 2), (0, 1)):
                pm.set_option("fuse_attn", fa)
                pm.set_option("fuse_ffn", ffu)
                where = f"{tag}: inputs {rep}, varlen {packed}, fuse_attn {fa}, fuse_ffn {ffu}"
                outs[fa, ffu] = pm(x, t, attention_mask=mask).numpy()[valid]
                _assert_grids(pm, _want_grids(0, B, L, fa, ffu), where)
                if (fa, ffu) in ((1, 2), (0, 1)):
                    e = float(np.abs(outs[fa, ffu] - want).max())
                    print(f"full grid {where}: {e:.3e}")
                    worst["max"] = max(worst["max"], e)
                    assert np.isfinite(outs[fa, ffu]).all() and e <= FWD_TOL, (where, e)
            d_attn = float(np.abs(outs[1, 0] - outs[0, 0]).max())
            d_ffn = max(float(np.abs(outs[1, 2] - outs[1, 0]).max()), float(np.abs(outs[0, 1] - outs[0, 0]).max()))
            worst.update(attn16_vs_two_kernel=max(worst["attn16_vs_two_kernel"], d_attn), ffn16_vs_gemms=max(worst["ffn16_vs_gemms"], d_ffn))
            assert d_attn <= 2e-6, (tag, rep, packed, d_attn)
            assert d_ffn <= 4e-6, (tag, rep, packed, d_ffn)
    _record(f"fwd_full_grid_{tag}", rounds=rounds, **worst)


def test_three_items_per_workgroup_on_the_full_grid(gpu):
    """debug_grid 0, more than two rounds of items: 2 CUs + 40 sequences of 128 positions (every 16th shorter) at d_model 192, so that
    workgroups of the fused attention take three sequences and, padded and packed alike, workgroups of the fused feed-forward
    three passes, with a ragged last round.  EVERY sequence against the oracle (the full-size tests sample six or seven), forward
    and one reverse step."""
    ncu = _ncu()
    B, L = 2 * ncu + 40, 128
    lens = _ragged_lens(B)
    assert sum(n < 128 for n in lens) == (B + 15) // 16 and min(lens) >= 40
    packed_rows = sum(_ceil(n, 8) for n in lens)
    assert packed_rows > 2 * ncu * 128, packed_rows
    for packed in (0, 1):
        n = _passes(B, L, lens, packed)
        assert _most_items(n, ncu) == 3 and n % ncu, (packed, n)   # three passes on some workgroups, two on the others
    assert _most_items(B, ncu) == 3 and B % ncu
    layers = 2
    o32, _, pm = _pair(hidden=192, heads=6, ff=384, layers=layers, maxpos=128, seed=3, precision="f16x3")
    _assert_plan_launches(pm, layers, B, L, lens, [(1, 2, 0), (0, 1, 0), (1, 2, 1), (0, 1, 1)])
    betas = beta_schedules.cosine_beta_schedule(1000)
    h = pm.prepare(betas)
    try:
        _set_grid(pm, 0)
        _full_grid_forwards(pm, o32, "192_three_rounds", B, L, lens, rounds=3)
        pm.set_option("varlen", 0)
        pm.set_option("fuse_attn", 1)
        pm.set_option("fuse_ffn", 2)
        x = _inputs(B, L, seed=11)
        z = torch.randn(B, L, 6, generator=torch.Generator().manual_seed(6))
        out = _step(pm, h, x.numpy(), 640, lens, z.numpy())
        _assert_grids(pm, _want_grids(0, B, L, 1, 2), "step")
        want = ref_sampling.wrap(ref_sampling.p_sample(o32, x, torch.full((B,), 640, dtype=torch.long), lens, betas, z), -torch.pi, torch.pi).numpy()
        worst = max(float(ref_sampling.circ_dist(out[i, :n], want[i, :n]).max()) for i, n in enumerate(lens))
        _record("step_full_grid_192_three_rounds", max=worst)
        assert np.isfinite(out).all() and worst <= STEP_TOL, worst
    finally:
        _reset_plan(pm)


def test_two_items_on_some_workgroups_of_the_full_grid(gpu):
    """The released width, CUs + 24 sequences: 24 workgroups take a second item, the others end after their first."""
    ncu = _ncu()
    B, L = ncu + 24, 128
    lens = _ragged_lens(B)
    for packed in (0, 1):
        n = _passes(B, L, lens, packed)
        assert _most_items(n, ncu) == 2 and 0 < n - ncu <= 24, (packed, n)
    layers = 2
    o32, _, pm = _pair(hidden=384, heads=12, ff=768, layers=layers, maxpos=128, seed=3, precision="f16x3")
    _assert_plan_launches(pm, layers, B, L, lens, [(1, 2, 0), (0, 1, 0), (1, 2, 1), (0, 1, 1)])
    pm.prepare(beta_schedules.cosine_beta_schedule(1000))
    try:
        _set_grid(pm, 0)
        _full_grid_forwards(pm, o32, "384_two_rounds", B, L, lens, rounds=2)
    finally:
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- (e) C3's second batch as sampled
def test_c3_second_batch_as_sample_runs_it(gpu):
    """The second batch sampling.sample() makes of BASELINE C3 (268 sequences of 101 .. 127 positions) with the options it sets:
    packed rows and the exact row count as "rows_hint", the fused kernels on auto.  The hint puts the 246 passes on the layer tail
    (asserted through the launch counters on a 256-CU device); test_steps_c3_chunk_shapes_teacher_forced pads the rows and so runs
    the GEMMs.  Released width, two layers: forward and one reverse step against the oracle on EVERY sequence."""
    lens = _c3_chunks()[1]
    B, L = len(lens), max(lens)
    assert (B, L) == (268, 127)
    layers = 2
    o32, _, pm = _pair(hidden=384, heads=12, ff=768, layers=layers, maxpos=128, seed=0, precision="f16x3")
    betas = beta_schedules.cosine_beta_schedule(1000)
    rows_hint = sum((int(n) + 7) // 8 * 8 for n in lens)   # (sampling.sample)
    x = _inputs(B, L, seed=21)
    _assert_items_differ(x, lens, 1)
    try:
        pm.set_option("varlen", 1)
        pm.set_option("rows_hint", rows_hint)
        if _ncu() == 256:
            assert (rows_hint + 127) // 128 == 246
            got = _launches_per_step(pm, x.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda:0"), beta_schedules.cosine_beta_schedule(2))
            assert got.get("attn_out_ffn_fused", 0) == layers and got.get("gemm_qkv", 0) == layers and got.get("attention", 0) == layers, got
            assert not any(got.get(k, 0) for k in ("gemm_attn_out", "gemm_ffn_up", "gemm_ffn_down", "ffn_fused", "qkv_attention_fused")), got
        h = pm.prepare(betas)
        mask = _mask(lens, L)
        valid = mask.bool().numpy()
        t = torch.full((B,), 400, dtype=torch.long)
        got = pm(x, t, attention_mask=mask).numpy()[valid]
        if _ncu() == 256:
            _assert_grids(pm, (None, None, 256), "forward")   # (the launcher goes by the bound of 268 x 128 rows, the kernel by the count)
        e = float(np.abs(got - o32(x, t, attention_mask=mask).numpy()[valid]).max())
        assert np.isfinite(got).all() and e <= FWD_TOL, e
        z = torch.randn(B, L, 6, generator=torch.Generator().manual_seed(6))
        out = _step(pm, h, x.numpy(), 400, lens, z.numpy())
        want = ref_sampling.wrap(ref_sampling.p_sample(o32, x, t, lens, betas, z), -torch.pi, torch.pi).numpy()
        worst = max(float(ref_sampling.circ_dist(out[i, :n], want[i, :n]).max()) for i, n in enumerate(lens))
        _record("c3_second_batch_as_sampled", fwd_max=e, step_max=worst)
        assert np.isfinite(out).all() and worst <= STEP_TOL, worst
    finally:
        pm.set_option("rows_hint", 0)
        _reset_plan(pm)


# ---------------------------------------------------------------------------------------------- (f) many inputs through one handle
@pytest.mark.parametrize("ffu", [1, 2])
@pytest.mark.parametrize("hidden,heads,ff,layers", [(192, 6, 384, 6), (384, 12, 768, 3)])
def test_a_sequence_of_different_inputs_through_one_handle(gpu, hidden, heads, ff, layers, ffu):
    """scripts/ffn16_stress.py, bounded and with a DIFFERENT input per run (a stale plane of the same input would survive the
    script): 40 forwards of 4 x 128 through one handle with the fused feed-forward (1) / the layer tail (2), each against the GEMM
    launches on the same input (4e-6) and the fp32 oracle (FWD_TOL); runs 10 .. 19 and 30 .. 39 on ONE workgroup, which then walks
    all four passes.  The first mismatch fails the test and names the run and the wrong 16-row blocks; nothing is retried, and a
    HIP error ends the test (it raises)."""
    o32, _, pm = _pair(hidden=hidden, heads=heads, ff=ff, layers=layers, maxpos=128, seed=3, precision="f16x3")
    B, L = 4, 128
    lens = [L] * B
    _assert_plan_launches(pm, layers, B, L, lens, [(0, 0, 0), (0, ffu, 0)])
    pm.prepare(beta_schedules.cosine_beta_schedule(100))
    mask = torch.ones(B, L)
    t = torch.full((B,), 42, dtype=torch.long)
    assert _passes(B, L, lens, 0) == 4
    pm.set_option("fuse_attn", 0)
    worst = dict(vs_gemms=0.0, vs_oracle=0.0)
    previous = None

    def blocks(d, tol):
        rows = d.max(axis=2)
        return {b: sorted({int(i) // 16 for i in np.nonzero(rows[b] > tol)[0]}) for b in range(B) if (rows[b] > tol).any()}

    try:
        for run in range(40):
            cap = (run // 10) % 2
            _set_grid(pm, cap)
            x = _inputs(B, L, seed=100 + run)
            assert previous is None or not torch.equal(x, previous)
            previous = x
            pm.set_option("fuse_ffn", 0)
            two = pm(x, t, attention_mask=mask).numpy()
            pm.set_option("fuse_ffn", ffu)
            one = pm(x, t, attention_mask=mask).numpy()   # (_binding.check raises on a HIP error or a non-finite result)
            _assert_grids(pm, _want_grids(cap, B, L, 0, ffu), f"run {run}")
            want = o32(x, t, attention_mask=mask).numpy()
            d2, do = np.abs(one - two), np.abs(one - want)
            worst.update(vs_gemms=max(worst["vs_gemms"], float(d2.max())), vs_oracle=max(worst["vs_oracle"], float(do.max())))
            assert np.isfinite(one).all() and d2.max() <= 4e-6, \
                f"run {run} (debug_grid {cap}): {d2.max():.3e} from the GEMM launches; wrong 16-row blocks per sequence: {blocks(d2, 4e-6)}"
            assert do.max() <= FWD_TOL, \
                f"run {run} (debug_grid {cap}): {do.max():.3e} from the oracle; wrong 16-row blocks per sequence: {blocks(do, FWD_TOL)}"
        _record(f"fwd_input_sequence_{hidden}_ffn{ffu}", runs=40, **worst)
    finally:
        _set_grid(pm, 0)
        _reset_plan(pm)
