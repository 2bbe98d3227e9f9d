"""
CPU restatement of the resampling schedules of motif-conditioned sampling (TEST INFRASTRUCTURE ONLY), built on
tests/inpaint_reference.py: the jump statement of include/fdmi.h in float32 numpy and the walk over a ``visits`` schedule
with one Philox key per segment, every draw from ``oracle.ref_philox``.

A jump takes the state from level a up to level b > a: fixed elements are the replacement at level b, free elements are
``wrap?(jk * x + js * z)`` with each product and the sum rounded once, positions at or beyond a length keep their bits.
"""
import numpy as np

import inpaint_reference as ipr
from oracle import ref_philox

JUMP_TAG = 0x40000000            # bit 30 of the Philox step word: the jump's stream for the free elements
GOLDEN = 0x9E3779B97F4A7C15      # the stride of the segments' seeds


def seeds(seed: int, s: int) -> int:
    """The Philox key of segment s (s = 0: the seed itself)."""
    return (int(seed) + int(s) * GOLDEN) & 0xFFFFFFFFFFFFFFFF


def jump_draw(seed: int, level: int, seq_offset: int, B: int, L: int, F: int) -> np.ndarray:
    """The jump's Philox draw for the free elements: ``ref_philox.philox_normal`` with bit 30 of the step word set."""
    return ref_philox.philox_normal(seed, JUMP_TAG | level, seq_offset, B, L, F)


def jump(x, known, fixed, level_to: int, jk, js, coef, z_free, z_known, is_angle, lens) -> np.ndarray:
    """``x`` [B, L, F] taken to ``level_to`` >= 1: the fixed elements at that level (draws ``z_known``), the free ones
    ``jk * x + js * z_free`` (float32 products, float32 sum), angular features wrapped; l >= lens[i] untouched."""
    x = np.asarray(x, dtype=np.float32)
    fixed = np.asarray(fixed).astype(bool)
    jk, js = np.float32(jk), np.float32(js)
    with np.errstate(invalid="ignore"):
        v = ((jk * x).astype(np.float32) + (js * np.asarray(z_free, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    v[..., cols] = ipr.wrap32(v[..., cols])
    out = ipr.replace(v, known, fixed, level_to, coef, z_known, is_angle)
    for i, n in enumerate(lens):
        out[i, n:] = x[i, n:]
    return out


def loop(model, lens, x_init, t_start: int, betas, is_angle, known, fixed, coef, visits, jump_coef, seed: int,
         seq_offset: int = 0) -> np.ndarray:
    """The whole resampled run, [n_visits, B, L, F] (row i = the state after the i-th visit; the last row is what
    fd_sample_inpaint_resample returns).  Every draw comes from ``ref_philox`` with the segment's key."""
    x = np.asarray(x_init, dtype=np.float32)
    B, L, F = x.shape
    visits = [int(v) for v in visits]
    assert visits[0] == t_start and visits[-1] == 0
    key, seg = seeds(seed, 0), 0
    x = ipr.replace(x, known, fixed, t_start + 1, coef, ipr.tagged_draw(key, t_start + 1, seq_offset, B, L, F), is_angle)
    out = []
    for i, t in enumerate(visits):
        if i > 0 and t != visits[i - 1] - 1:
            assert t >= visits[i - 1], (i, t)
            seg += 1
            key = seeds(seed, seg)
            jk, js = jump_coef[seg - 1]
            x = jump(x, known, fixed, t + 1, jk, js, coef, jump_draw(key, t + 1, seq_offset, B, L, F),
                     ipr.tagged_draw(key, t + 1, seq_offset, B, L, F), is_angle, lens)
        x = ipr.step(model, x, t, lens, betas, ref_philox.philox_normal(key, t, seq_offset, B, L, F) if t > 0 else None, known, fixed,
                     coef, ipr.tagged_draw(key, t, seq_offset, B, L, F) if t > 0 else None, is_angle)
        out.append(x)
    return np.stack(out)
