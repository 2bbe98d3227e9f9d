"""
CPU restatement of motif-conditioned sampling by replacement (TEST INFRASTRUCTURE ONLY): ``oracle.ref_sampling.p_sample``
plus the loop's wrap, then the replacement statement of include/fdmi.h in float32 numpy, with the replacement's draws
taken from arrays or from ``oracle.ref_philox`` with the tagged step word.

Levels: a state at level j has seen j forward-noising steps; the state that enters reverse step t is at level t + 1, the
state step t leaves is at level t.  ``coef`` = ``sampling.inpaint_levels(betas)``: keep[0..T] then spread[0..T].
"""
import numpy as np
import torch

from oracle import ref_philox, ref_sampling

TAG = 0x80000000   # the top bit of the Philox step word: the replacement's stream


def levels(betas) -> np.ndarray:
    """float32 [2, T + 1] from ``ref_sampling.alpha_terms``: level 0 = (1, 0), level j = the terms of timestep j - 1."""
    terms = ref_sampling.alpha_terms(torch.as_tensor(betas, dtype=torch.float32))
    keep = np.concatenate([[1.0], terms["sqrt_alphas_cumprod"].numpy()]).astype(np.float32)
    spread = np.concatenate([[0.0], terms["sqrt_one_minus_alphas_cumprod"].numpy()]).astype(np.float32)
    return np.stack([keep, spread])


def wrap32(v: np.ndarray) -> np.ndarray:
    """The reference's wrap on a float32 array, in torch's float32 arithmetic (what the device reproduces bit for bit)."""
    return ref_sampling.wrap(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)), -torch.pi, torch.pi).numpy()


def known_at_level(known: np.ndarray, level: int, coef: np.ndarray, z, is_angle) -> np.ndarray:
    """The value every element WOULD take at ``level`` if it were fixed, float32 [B, L, F]: level 0 = ``known``'s bits;
    level j >= 1 = keep[j] * known + spread[j] * z with each product and the sum rounded once, angular features wrapped."""
    known = np.asarray(known, dtype=np.float32)
    if level == 0:
        return known.copy()
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = (coef[0, level] * known).astype(np.float32) + (coef[1, level] * z).astype(np.float32)
    v = v.astype(np.float32)
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    v[..., cols] = wrap32(v[..., cols])
    return v


def tagged_draw(seed: int, level: int, seq_offset: int, B: int, L: int, F: int) -> np.ndarray:
    """The replacement's Philox draw of ``level``: ``ref_philox.philox_normal`` with the top bit of the step word set."""
    return ref_philox.philox_normal(seed, TAG | level, seq_offset, B, L, F)


def replace(x: np.ndarray, known, fixed, level: int, coef, z, is_angle) -> np.ndarray:
    """``x`` with its fixed elements set to their value at ``level``."""
    fixed = np.asarray(fixed).astype(bool)
    return np.where(fixed, known_at_level(np.where(fixed, known, np.float32(0)), level, coef, z, is_angle),
                    np.asarray(x, dtype=np.float32)).astype(np.float32)


@torch.no_grad()
def step(model, x, t: int, lens, betas, z, known, fixed, coef, z_known, is_angle) -> np.ndarray:
    """One reverse step with replacement: p_sample + the loop's wrap (the oracle model), then level t for the fixed ones."""
    xt = torch.as_tensor(np.asarray(x), dtype=next(model.parameters()).dtype)
    B = xt.shape[0]
    zt = None if z is None else torch.as_tensor(np.asarray(z), dtype=xt.dtype)
    out = ref_sampling.p_sample(model, xt, torch.full((B,), t, dtype=torch.long), lens, betas.to(xt.dtype), zt)
    for j, a in enumerate(is_angle):
        if a:
            out[:, :, j] = ref_sampling.wrap(out[:, :, j], -torch.pi, torch.pi)
    return replace(out.to(torch.float32).numpy(), known, fixed, t, coef, z_known, is_angle)


@torch.no_grad()
def loop(model, lens, x_init, t_start: int, betas, is_angle, known, fixed, coef, step_noise, known_noise) -> np.ndarray:
    """The whole run, [t_start + 1, B, L, F] (row j = the state after step t = t_start - j): the start point's fixed
    elements at level t_start + 1, then ``step`` for t = t_start .. 0.  step_noise[t] / known_noise[level] are arrays
    ([t_start + 1, ...] / [t_start + 2, ...]; row 0 of either is not read)."""
    x = replace(np.asarray(x_init, dtype=np.float32), known, fixed, t_start + 1, coef, known_noise[t_start + 1], is_angle)
    out = []
    for t in range(t_start, -1, -1):
        x = step(model, x, t, lens, betas, step_noise[t] if t > 0 else None, known, fixed, coef,
                 known_noise[t] if t > 0 else None, is_angle)
        out.append(x)
    return np.stack(out)
