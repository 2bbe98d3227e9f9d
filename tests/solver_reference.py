"""
CPU restatement of few-step sampling with the second-order multistep solver (TEST INFRASTRUCTURE ONLY): the update
statement of include/fdmi.h in numpy float32, the coefficient table of ``sampling.solver_coefficients`` written out visit
by visit from the lambda / h form of DPM-Solver++(2M) (Lu et al. 2022, algorithm 2) in Python floats with ``expm1``, and the
loop over an oracle model.

Levels as in tests/strided_reference.py: visit i runs the network at t = visits[i] (level p = visits[i] + 1) and leaves
the state at level q = visits[i + 1] + 1, q = 0 behind the last visit.
"""
import math

import numpy as np
import torch

from strided_reference import _wrap, acp_levels, forward


def coefficients64(betas, visits, order: int = 2) -> np.ndarray:
    """float64 [5, K], rows a | b | c | u | v, one visit at a time.  With lam = log(alpha / sigma), h = lam_q - lam_p and
    phi = -expm1(-h) = 1 - exp(-h), the published step is
        x_q = (sigma_q / sigma_p) x_p + alpha_q phi D,     D = x0 + (x0 - x0_prev) / (2 r),   r = (lam_p - lam_p') / h
    with x0 = (x_p - sigma_p eps) / alpha_p.  Collecting x_p and eps:  a = sigma_q / sigma_p + alpha_q phi / alpha_p,
    b = -alpha_q phi sigma_p / alpha_p,  c = alpha_q phi / (2 r),  u = 1 / alpha_p,  v = -sigma_p / alpha_p.  Level 0 has
    sigma = 0, lam = +inf, so the last visit has h = inf, phi = 1 and takes the first-order step (c = 0), as the first does."""
    acp = acp_levels(betas)
    visits = [int(t) for t in visits]
    K = len(visits)

    def level(j):
        alpha, sigma = math.sqrt(acp[j]), math.sqrt(1.0 - acp[j])
        lam = math.inf if j == 0 else 0.5 * (math.log(acp[j]) - math.log1p(-acp[j]))
        return alpha, sigma, lam

    rows = []
    for i, t in enumerate(visits):
        alpha_p, sigma_p, lam_p = level(t + 1)
        alpha_q, sigma_q, lam_q = level(visits[i + 1] + 1 if i + 1 < K else 0)
        h = lam_q - lam_p
        phi = -math.expm1(-h)
        a = sigma_q / sigma_p + alpha_q * phi / alpha_p
        b = -alpha_q * phi * sigma_p / alpha_p
        c = 0.0
        if order == 2 and 0 < i < K - 1:
            r = (lam_p - level(visits[i - 1] + 1)[2]) / h
            c = alpha_q * phi / (2.0 * r)
        rows.append((a, b, c, 1.0 / alpha_p, -sigma_p / alpha_p))
    return np.array(rows, dtype=np.float64).T


def _wrap_cols(v: np.ndarray, cols) -> np.ndarray:
    if len(cols):
        v[..., cols] = _wrap(torch.from_numpy(np.ascontiguousarray(v[..., cols]))).numpy()
    return v


def update(x, eps, prev, a, b, c, u, v, is_angle):
    """The statement on float32 arrays -> (x', x0): every product and every sum rounded once; angular features wrapped by the
    reference's wrap in torch float32 (what the device reproduces bit for bit); the difference x0 - prev is wrapped too;
    where c == 0 ``prev`` is not looked at (it may be None, or hold NaN)."""
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    a, b, c, u, v = (np.float32(k) for k in (a, b, c, u, v))
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (x.shape[-1],)))[0]
    with np.errstate(invalid="ignore", over="ignore"):
        m = ((a * x).astype(np.float32) + (b * eps).astype(np.float32)).astype(np.float32)
        x0 = _wrap_cols(((u * x).astype(np.float32) + (v * eps).astype(np.float32)).astype(np.float32), cols)
        if c != 0:
            d = _wrap_cols((x0 - np.asarray(prev, dtype=np.float32)).astype(np.float32), cols)
            m = (m + (c * d).astype(np.float32)).astype(np.float32)
    return _wrap_cols(m, cols), x0


@torch.no_grad()
def loop(model, lens, x_init, visits, coef, is_angle) -> np.ndarray:
    """The whole run with an oracle model, [K, B, L, F] (row i = the state after visit i), in the model's dtype: a float32
    model follows ``update`` exactly; a float64 model runs the same statement in float64 from the same float32 table."""
    dtype = next(model.parameters()).dtype
    x = np.asarray(x_init, dtype=np.float32)
    x = x if dtype == torch.float32 else torch.as_tensor(x, dtype=dtype)
    cols = np.nonzero(np.broadcast_to(np.asarray(is_angle, dtype=bool), (np.asarray(x_init).shape[-1],)))[0]
    out, prev = [], None
    for i, t in enumerate(visits):
        a, b, c, u, v = (float(k) for k in coef[:, i])
        eps = forward(model, x, int(t), lens)
        if dtype == torch.float32:
            x, prev = update(x, eps.numpy(), prev, a, b, c, u, v, is_angle)
            out.append(x)
            continue
        m = a * x + b * eps
        x0 = u * x + v * eps
        x0[..., cols] = _wrap(x0[..., cols])
        if c != 0:
            d = x0 - prev
            d[..., cols] = _wrap(d[..., cols])
            m = m + c * d
        m[..., cols] = _wrap(m[..., cols])
        x, prev = m, x0
        out.append(m.numpy().copy())
    return np.stack(out)


# ---- the analytic case of the order test: data that is Gaussian per element, N(m, s0^2).  The optimal eps and the exact end
# point of the probability-flow ODE are closed forms (float64, no wrapping).
def gaussian_eps(x, acp_p, m=0.3, s0=0.5):
    """E[eps | x_p = x] for x_p = alpha x_0 + sigma eps, x_0 ~ N(m, s0^2)."""
    alpha, var = math.sqrt(acp_p), acp_p * s0 * s0 + (1.0 - acp_p)
    return math.sqrt(1.0 - acp_p) * (x - alpha * m) / var


def gaussian_ode_end(x_start, acp_start, m=0.3, s0=0.5):
    """The probability-flow ODE keeps (x - alpha m) / sqrt(alpha^2 s0^2 + sigma^2) constant; at level 0: alpha = 1, sigma = 0."""
    std = math.sqrt(acp_start * s0 * s0 + (1.0 - acp_start))
    return m + s0 * (x_start - math.sqrt(acp_start) * m) / std


def gaussian_run(betas, visits, coef64, x_start, m=0.3, s0=0.5) -> np.ndarray:
    """The solver's statement in float64, without wrapping, on the analytic eps; coef64 [5, K] float64."""
    acp = acp_levels(betas)
    x = np.asarray(x_start, dtype=np.float64).copy()
    prev = None
    for i, t in enumerate(visits):
        a, b, c, u, v = coef64[:, i]
        eps = gaussian_eps(x, acp[int(t) + 1], m, s0)
        x0 = u * x + v * eps
        x = a * x + b * eps + (c * (x0 - prev) if c != 0 else 0.0)
        prev = x0
    return x
