"""
CPU restatement of few-step sampling on a strided schedule (TEST INFRASTRUCTURE ONLY): the update statement of
include/fdmi.h in numpy float32, the coefficient table of ``sampling.ddim_coefficients`` written out visit by visit in
Python floats, and the loop over an oracle model.

Levels as in tests/inpaint_reference.py: the state that enters step t is at level t + 1.  Visit i runs the network at
t = visits[i] (level p = visits[i] + 1) and leaves the state at level q = visits[i + 1] + 1, q = 0 behind the last visit.
"""
import math

import numpy as np
import torch

from oracle import ref_sampling


def acp_levels(betas) -> list:
    """acp[j] for the levels j = 0 .. T in float64: acp[0] = 1, acp[j] = the running product of 1 - float64(betas[u]), u < j."""
    out = [1.0]
    for b in torch.as_tensor(betas).detach().cpu().tolist():   # (tolist of a float32 tensor: the exact values as Python floats)
        out.append(out[-1] * (1.0 - b))
    return out


def coefficients64(betas, visits, eta: float) -> np.ndarray:
    """float64 [3, K], rows a | b | s, one visit at a time."""
    acp = acp_levels(betas)
    visits = [int(v) for v in visits]
    rows = []
    for i, t in enumerate(visits):
        p = t + 1
        q = visits[i + 1] + 1 if i + 1 < len(visits) else 0
        r = acp[p] / acp[q]
        s = eta * math.sqrt((1.0 - acp[q]) / (1.0 - acp[p])) * math.sqrt(1.0 - r)
        a = math.sqrt(1.0 / r)
        b = math.sqrt(max(1.0 - acp[q] - s * s, 0.0)) - a * math.sqrt(1.0 - acp[p])
        rows.append((a, b, s))
    return np.array(rows, dtype=np.float64).T


def coefficients(betas, visits, eta: float) -> np.ndarray:
    """The float32 table: the float64 values rounded once."""
    return np.ascontiguousarray(coefficients64(betas, visits, eta).astype(np.float32))


def _wrap(v: torch.Tensor) -> torch.Tensor:
    return ref_sampling.wrap(v, -torch.pi, torch.pi)


def update(x, eps, a, b, s, z, is_angle) -> np.ndarray:
    """The statement on float32 arrays: x' = a x + b eps, every product and the sum rounded once; + s z (product and sum
    rounded once) only where s != 0 -- z is then not looked at; angular features wrapped by the reference's wrap in torch
    float32 (what the device reproduces bit for bit)."""
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    a, b, s = np.float32(a), np.float32(b), np.float32(s)
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((a * x).astype(np.float32) + (b * eps).astype(np.float32)).astype(np.float32)
        if s != 0:
            v = (v + (s * np.asarray(z, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (x.shape[-1],)))[0]
    if len(cols):
        v[..., cols] = _wrap(torch.from_numpy(np.ascontiguousarray(v[..., cols]))).numpy()
    return v


@torch.no_grad()
def forward(model, x, t: int, lens) -> torch.Tensor:
    """The oracle's prediction at timestep t, in the model's dtype."""
    xt = torch.as_tensor(np.asarray(x), dtype=next(model.parameters()).dtype)
    mask = torch.zeros(xt.shape[:2])
    for i, n in enumerate(lens):
        mask[i, :n] = 1.0
    return model(xt, torch.full((xt.shape[0],), int(t), dtype=torch.long), attention_mask=mask)


@torch.no_grad()
def loop(model, lens, x_init, visits, coef, is_angle, noise) -> np.ndarray:
    """The whole run with an oracle model, [K, B, L, F] (row i = the state after visit i), in the model's dtype: a float32
    model follows ``update`` exactly; a float64 model runs the same statement in float64 from the same float32 table.
    ``noise`` [K, B, L, F]; rows of visits with s == 0 are not read."""
    dtype = next(model.parameters()).dtype
    x = np.asarray(x_init, dtype=np.float32)
    x = x if dtype == torch.float32 else torch.as_tensor(x, dtype=dtype)
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (np.asarray(x_init).shape[-1],)))[0]
    out = []
    for i, t in enumerate(visits):
        a, b, s = (float(c) for c in coef[:, i])
        eps = forward(model, x, int(t), lens)
        if dtype == torch.float32:
            x = update(x, eps.numpy(), a, b, s, None if s == 0 else noise[i], is_angle)
            out.append(x)
            continue
        v = a * x + b * eps
        if s != 0:
            v = v + s * torch.as_tensor(noise[i], dtype=dtype)
        v[..., cols] = _wrap(v[..., cols])
        x = v
        out.append(v.numpy().copy())
    return np.stack(out)
