"""
The trained-model regime of tests/trained_regime_cases.py, on the CPU: the weights are what they claim to be (conditions on the fp64
oracle, not tolerances), the problem stays well posed in fp32, and an attention operand that lost its lo plane -- invisible at
synthetic_model's plain weights -- misses the GPU tests' gate several times over.  No GPU needed.
"""
import math

import numpy as np
import pytest
import torch

import trained_regime_cases as cases

FWD_TOL = 1e-5   # tests/test_gpu_parity.py's (that module loads the GPU library; tests/test_trained_regime_gpu.py asserts the two agree)
_CASES = [(name, regime) for name in cases.MODELS for regime in cases.REGIMES]


def test_pinned_gains_are_powers_of_two():
    for name, (arch, gains) in cases.MODELS.items():
        assert set(gains) == set(cases.REGIMES), name
        for regime, g in gains.items():
            assert len(g) == 4 and all(v >= 1 and math.log2(v) == round(math.log2(v)) for v in g), (name, regime, g)
        (mq, mk, md, mi), (sq, sk, sd, si) = gains["moderate"], gains["sharp"]
        # sharp is moderate pushed further: the content term q . k and the pre-activations
        assert sq * sk > mq * mk and si > mi, (name, gains)
        if arch["pos"] == "absolute":
            assert all(g[2] == 1 for g in gains.values()), name   # (no distance table: nothing to multiply)


@pytest.mark.parametrize("name", list(cases.MODELS))
def test_gains_touch_the_named_parameters_only(name):
    arch, gains = cases.MODELS[name]
    plain = cases.state_dict_for(name, "plain")
    for regime in cases.REGIMES:
        gq, gk, gd, gi = gains[regime]
        sd = cases.trained_gains(plain, arch["layers"], gq, gk, gd, gi)
        assert list(sd) == list(plain)
        named = 0
        for key, v in sd.items():
            if not cases.named_by_gains(key, arch["layers"]):
                assert torch.equal(v, plain[key]) and v.dtype == plain[key].dtype, key
                continue
            named += 1
            g = gi if ("intermediate" in key or "token_decoder" in key) else gq if "query" in key else gk if "key" in key else gd
            assert torch.equal(v, plain[key] * g), key
            assert torch.equal(v / g, plain[key]), key   # a power of two: exact, nothing rounded away
        per_layer = 6 + (arch["pos"] != "absolute")
        assert named == arch["layers"] * per_layer + 2, (name, named)
        assert all(torch.equal(a, b) for a, b in zip(plain.values(), cases.state_dict_for(name, "plain").values()))   # input not modified


@pytest.mark.parametrize("name,regime", _CASES)
def test_regime_conditions_and_sensitivity(name, regime):
    """Per model, regime and shape of the GPU tests, on the fp64 oracle at t = 42, inputs of seed 1:
    the regime's conditions in every layer (asserted from 64 keys up, recorded below), the fp32 oracle within 3e-6 of the fp64 one,
    and q or k rounded to fp16 in every layer moving the output by more than 5 x the case's gate max(4 e_ref, 2e-6); the distance
    table rounded to fp16 by more than 2 x the gate in the sharp regime on the large shapes of the every-plan models.
    Conditions of single GPU cases: relative_key at L = 200 -- of the rows that have a second key tile, at least 25 % find their
    largest score there (alpha really rescales); f32, sharp -- some valid score lies more than 200 below its row maximum (the
    kernel's clamp is reached); d 384, sharp, 3 x 7 -- some rows hold all the mass on one key to the last bit."""
    arch, _ = cases.MODELS[name]
    o32, o64 = cases.oracle_pair(name, regime)
    for B, L, lens in cases.SHAPES[name]:
        x, mask = cases.inputs(B, L), cases.mask_of(lens, L)
        t = torch.full((B,), cases.T_STATS, dtype=torch.long)
        valid = mask.bool().numpy()
        want64, stats = cases.regime_stats(o64, x, t, mask)
        want64 = want64.numpy()[valid]
        want32 = o32(x, t, attention_mask=mask).numpy()[valid]
        _, e_ref, gate = cases.rel_gate(want32, want32, want64)
        where = f"{name} {regime} {B} x {L}"
        for key in stats[0]:
            print(f"{where}: {key:16s}", " ".join(f"{s[key]:.3g}" for s in stats))
        missed = cases.check_conditions(regime, stats)
        if L >= cases.ASSERT_FROM_L:
            assert not missed, (where, missed)
        else:
            print(f"{where}: recorded only, conditions missed: {missed}")
        assert e_ref <= cases.E_REF_MAX, (where, e_ref)
        moved = {}
        for op in ("q", "k") + (("e",) if arch["pos"] != "absolute" else ()):
            got = cases.forward_restated(o64, x.double(), t, mask.double(), rounded=op).numpy()[valid]
            moved[op] = cases.rel_gate(got, want32, want64)[0] / gate
        print(f"{where}: e_ref {e_ref:.2e} gate {gate:.2e}, moved (in gates) by an fp16 " + " ".join(f"{k} {v:.1f}" for k, v in moved.items()))
        assert moved["q"] > 5 and moved["k"] > 5, (where, moved)
        if regime == "sharp" and name in ("d384", "d192") and L >= cases.ASSERT_FROM_L:
            assert moved["e"] > 2, (where, moved)
        if L > 128:
            assert all(s["argmax_past_128"] >= 0.25 for s in stats), (where, [s["argmax_past_128"] for s in stats])
        if name == "f32_192" and regime == "sharp":
            assert max(s["range_max"] for s in stats) > 200, (where, [s["range_max"] for s in stats])
        if name == "d384" and regime == "sharp" and L == 7:
            assert max(s["pmax_is_1"] for s in stats) > 0, (where, [s["pmax_is_1"] for s in stats])


@pytest.mark.parametrize("name", ["d384", "d192"])
def test_plain_weights_hide_a_lost_lo_plane(name):
    """The gap being closed: on synthetic_model's weights as they are, q, k or the distance table rounded to fp16 in every layer
    stays under FWD_TOL, the gate of every forward test at those weights -- and none of the regimes' conditions holds."""
    o32, o64 = cases.oracle_pair(name, "plain")
    for B, L, lens in cases.SHAPES_A:
        x, mask = cases.inputs(B, L), cases.mask_of(lens, L)
        t = torch.full((B,), cases.T_STATS, dtype=torch.long)
        valid = mask.bool().numpy()
        want64, stats = cases.regime_stats(o64, x, t, mask)
        want64 = want64.numpy()[valid]
        for op in "qke":
            got = cases.forward_restated(o64, x.double(), t, mask.double(), rounded=op).numpy()[valid]
            moved = float(np.abs(got - want64).max())
            print(f"{name} plain {B} x {L}: fp16 {op} moves the output by {moved:.2e}")
            assert moved < FWD_TOL, (name, B, L, op, moved)
        assert max(s["score_max"] for s in stats) <= 1.5 and max(s["ff_max"] for s in stats) < 4, (name, B, L)
        assert cases.check_conditions("moderate", stats) and cases.check_conditions("sharp", stats)


def test_restated_attention_is_the_oracles():
    """forward_restated without a rounded operand is the oracle's forward to the last bit, in both dtypes."""
    for name in ("d384", "rkq384", "abs192"):
        o32, o64 = cases.oracle_pair(name, "sharp")
        B, L, lens = 3, 7, [7, 1, 3]
        x, mask = cases.inputs(B, L), cases.mask_of(lens, L)
        t = torch.full((B,), cases.T_STATS, dtype=torch.long)
        assert torch.equal(cases.forward_restated(o32, x, t, mask), o32(x, t, attention_mask=mask)), name
        assert torch.equal(cases.forward_restated(o64, x.double(), t, mask.double()), o64(x.double(), t, attention_mask=mask.double())), name


def test_eps_coefficient_is_the_posterior_means():
    """c(t) against p_sample itself: with z = 0, moving eps by d moves the step's output by c(t) d."""
    from foldingdiff_amd import beta_schedules
    from oracle import ref_sampling
    betas = beta_schedules.cosine_beta_schedule(1000)

    class Const:
        def __init__(self, v):
            self.v = v

        def __call__(self, x, t, attention_mask):
            return torch.full_like(x, self.v)

    x = torch.zeros(1, 4, 6, dtype=torch.float64)
    for tv in (999, 400, 1, 0):
        t = torch.full((1,), tv, dtype=torch.long)
        z = torch.zeros_like(x)
        a = ref_sampling.p_sample(Const(0.0), x, t, [4], betas.double(), z)
        b = ref_sampling.p_sample(Const(1.0), x, t, [4], betas.double(), z)
        assert abs(float((a - b).abs().max()) - cases.eps_coefficient(betas.numpy(), tv)) <= 1e-9 * max(1.0, cases.eps_coefficient(betas.numpy(), tv)), tv
