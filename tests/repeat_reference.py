"""
CPU restatement of the repeat tie (TEST INFRASTRUCTURE ONLY): the statement of include/fdmi.h (fd_tie_repeats,
fd_sample_repeat) in numpy float32, every product, sum and quotient rounded once, and the chain of a run over any step
function.

Sequence b has a tie (start, period, units): row start + k * period + j is copy k of unit row j; units == 1 ties nothing.
For a tied element, x_k its value in copy k:
    d_k = x_k - x_0 (wrapped where angular), k = 1 .. units - 1;  m = x_0 + (d_1 + .. + d_{units-1}) / float32(units)
    m = m + s z where s != 0 (z at the copy-0 position);  m = wrap(m) where angular;  every copy <- m
A free element of a row below the length: m = x, then the same + s z and wrap.  Rows at or beyond a length keep their bits.
``init``: every copy <- x_0 and nothing else.
"""
import numpy as np
import torch

from oracle import ref_sampling


def _wrap(v: np.ndarray) -> np.ndarray:
    """The reference's wrap in torch float32 (what the device reproduces bit for bit)."""
    return ref_sampling.wrap(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)), -torch.pi, torch.pi).numpy()


def _wrap_cols(v: np.ndarray, cols: np.ndarray) -> np.ndarray:
    """[rows, F] float32 with the angular columns wrapped."""
    v = np.array(v, dtype=np.float32)
    if len(cols) and v.size:
        v[:, cols] = _wrap(v[:, cols])
    return v


def tie(x, lens, ties, is_angle, init=False, s=0.0, z=None) -> np.ndarray:
    """The statement on a float32 [B, L, F] array; returns a new array.  ``z`` [B, L, F] is looked at only where s != 0."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    B, L, F = x.shape
    s = np.float32(s)
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (F,)))[0]
    z = None if z is None else np.asarray(z, dtype=np.float32)
    assert init or s == 0 or z is not None, "s != 0 needs the draws"
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = int(lens[b])
            start, period, units = (int(v) for v in ties[b])
            assert start >= 0 and period >= 1 and units >= 1 and start + period * units <= n <= L
            tied = np.zeros(n, dtype=bool)
            if units > 1:
                tied[start: start + period * units] = True
                x0 = x[b, start: start + period]                                         # [period, F]
                if init:
                    m = x0.copy()
                else:
                    total = None
                    for k in range(1, units):
                        xk = x[b, start + k * period: start + (k + 1) * period]
                        d = _wrap_cols((xk - x0).astype(np.float32), cols)
                        total = d if total is None else (total + d).astype(np.float32)
                    m = (x0 + (total / np.float32(units)).astype(np.float32)).astype(np.float32)
                    if s != 0:
                        m = (m + (s * z[b, start: start + period]).astype(np.float32)).astype(np.float32)
                    m = _wrap_cols(m, cols)
                for k in range(units):
                    out[b, start + k * period: start + (k + 1) * period] = m
            if init:
                continue
            free = np.nonzero(~tied)[0]
            m = x[b, free]
            if s != 0:
                m = (m + (s * z[b, free]).astype(np.float32)).astype(np.float32)
            out[b, free] = _wrap_cols(m, cols)
    return out


def chain(step_fn, x_init, lens, ties, is_angle, visits, coef, noise) -> np.ndarray:
    """fd_sample_repeat's statement over a step function: the init tie, then per visit i ``step_fn(x, t, a, b)`` -- the strided
    update without its draw, wrap(a x + b eps) below the lengths -- followed by the tie with s = coef[2][i] and noise[i].
    Returns the final state."""
    x = tie(x_init, lens, ties, is_angle, init=True)
    for i, t in enumerate(visits):
        a, b, s = coef[:, i]
        x = np.asarray(step_fn(x, int(t), a, b), dtype=np.float32)
        x = tie(x, lens, ties, is_angle, s=s, z=None if s == 0 or noise is None else noise[i])
    return x
