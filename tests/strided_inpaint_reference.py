"""
CPU restatement of few-step motif scaffolding (TEST INFRASTRUCTURE ONLY): a strided visit with replacement is
``strided_reference.update`` followed by ``inpaint_reference.replace`` at the level the visit LANDS on, and a resampled run
over a grid is that visit plus ``resample_reference.jump`` with one Philox key per segment (``resample_reference.seeds``).

Levels as in tests/strided_reference.py: visit i of a grid g_0 > ... > g_{K-1} runs the network at t = g_i on a state at
level g_i + 1 and leaves it at level q_i = g_{i+1} + 1, q_{K-1} = 0.  ``known_noise`` of a strided run has one row per
visit: row 0 = the start point (level g_0 + 1), row i + 1 = the state visit i leaves; the last row is never read.
"""
import numpy as np
import torch

import inpaint_reference as ipr
import resample_reference as rsr
import strided_reference as sref
from oracle import ref_philox


def landing_levels(visits) -> list:
    """q_i for every visit of a strictly descending grid."""
    v = [int(t) for t in visits]
    return [t + 1 for t in v[1:]] + [0]


def visit(x, eps, a, b, s, z, known, fixed, level: int, kcoef, z_known, is_angle) -> np.ndarray:
    """One visit on float32 arrays from a given prediction: the strided update of every element, then the fixed ones at
    ``level`` (z_known is not looked at for level 0, z not where s == 0)."""
    return ipr.replace(sref.update(x, eps, a, b, s, z, is_angle), known, fixed, level, kcoef, z_known, is_angle)


def _visit_model(model, x, t, lens, a, b, s, z, known, fixed, level, kcoef, z_known, is_angle):
    """``visit`` with the prediction of an oracle model, in the model's dtype: a float32 model follows ``visit`` exactly; a
    float64 model runs the update in float64 from the same float32 coefficients, its fixed elements are the float32
    statement's values."""
    dtype = next(model.parameters()).dtype
    eps = sref.forward(model, x, int(t), lens)
    if dtype == torch.float32:
        return visit(np.asarray(x, dtype=np.float32), eps.numpy(), a, b, s, z, known, fixed, level, kcoef, z_known, is_angle)
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    v = float(a) * xt + float(b) * eps
    if s != 0:
        v = v + float(s) * torch.as_tensor(np.asarray(z), dtype=dtype)
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (xt.shape[-1],)))[0]
    v[..., cols] = sref._wrap(v[..., cols])
    fx = np.asarray(fixed).astype(bool)
    lv = ipr.known_at_level(np.where(fx, known, np.float32(0)), level, kcoef, z_known, is_angle)
    return np.where(fx, lv.astype(np.float64), v.numpy())


@torch.no_grad()
def loop(model, lens, x_init, visits, coef, is_angle, known, fixed, kcoef, noise, known_noise) -> np.ndarray:
    """One strictly descending run with replacement, [K, B, L, F] (row i = the state after visit i): the start point's
    fixed elements at level visits[0] + 1 (known_noise[0]), then every visit.  noise [K, ...], known_noise [K + 1, ...]."""
    x = ipr.replace(np.asarray(x_init, dtype=np.float32), known, fixed, int(visits[0]) + 1, kcoef, known_noise[0], is_angle)
    q = landing_levels(visits)
    out = []
    for i, t in enumerate(visits):
        a, b, s = (float(c) for c in coef[:, i])
        x = _visit_model(model, x, t, lens, a, b, s, None if s == 0 else noise[i], known, fixed, q[i], kcoef,
                         known_noise[i + 1] if q[i] > 0 else None, is_angle)
        out.append(np.asarray(x))
    return np.stack(out)


def segments(grid, run) -> list:
    """[(first index, one past the last)] of the descents of a run over a grid."""
    pos = {int(t): i for i, t in enumerate(grid)}
    r = [int(t) for t in run]
    cuts = [0] + [i for i in range(1, len(r)) if pos[r[i]] != pos[r[i - 1]] + 1] + [len(r)]
    return list(zip(cuts[:-1], cuts[1:]))


def check_run(grid, run) -> None:
    """The legality rules of include/fdmi.h."""
    g, r = [int(t) for t in grid], [int(t) for t in run]
    pos = {t: i for i, t in enumerate(g)}
    assert all(g[i] < g[i - 1] for i in range(1, len(g))) and g[-1] >= 0, g
    assert r[0] == g[0] and r[-1] == g[-1] and all(t in pos for t in r), (g, r)
    for i in range(1, len(r)):
        assert pos[r[i]] == pos[r[i - 1]] + 1 or r[i] >= r[i - 1], (i, r)


def jump_levels(grid, run) -> list:
    """(a, b) of every jump in the order met: a = the level the visit before it landed on, b = run[i] + 1."""
    g = [int(t) for t in grid]
    q = dict(zip(g, landing_levels(g)))
    return [(q[int(run[i - 1])], int(run[i]) + 1) for i, _ in segments(grid, run)[1:]]


@torch.no_grad()
def resampled_loop(model, lens, x_init, grid, coef, run, jump_coef, is_angle, known, fixed, kcoef, seed: int,
                   seq_offset: int = 0) -> np.ndarray:
    """The whole resampled run over a grid, [n_run, B, L, F] (row i = the state after the i-th visit; the last row is what
    fd_sample_strided_inpaint_resample returns).  Every draw comes from ``ref_philox`` with the segment's key."""
    x = np.asarray(x_init, dtype=np.float32)
    B, L, F = x.shape
    g = [int(t) for t in grid]
    check_run(g, run)
    pos = {t: i for i, t in enumerate(g)}
    q = landing_levels(g)
    key = rsr.seeds(seed, 0)
    x = ipr.replace(x, known, fixed, g[0] + 1, kcoef, ipr.tagged_draw(key, g[0] + 1, seq_offset, B, L, F), is_angle)
    out = []
    for seg, (i0, i1) in enumerate(segments(g, run)):
        if seg > 0:
            key = rsr.seeds(seed, seg)
            level = int(run[i0]) + 1
            jk, js = jump_coef[seg - 1]
            x = rsr.jump(x, known, fixed, level, jk, js, kcoef, rsr.jump_draw(key, level, seq_offset, B, L, F),
                         ipr.tagged_draw(key, level, seq_offset, B, L, F), is_angle, lens)
        for i in range(i0, i1):
            t = int(run[i])
            k = pos[t]
            a, b, s = (float(c) for c in coef[:, k])
            z = None if s == 0 else ref_philox.philox_normal(key, t, seq_offset, B, L, F)
            zk = ipr.tagged_draw(key, q[k], seq_offset, B, L, F) if q[k] > 0 else None
            x = np.asarray(_visit_model(model, x, t, lens, a, b, s, z, known, fixed, q[k], kcoef, zk, is_angle), dtype=np.float32)
            out.append(x)
    return np.stack(out)
