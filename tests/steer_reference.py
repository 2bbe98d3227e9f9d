"""
CPU restatement of steering by particle resampling (TEST INFRASTRUCTURE ONLY): the statements of include/fdmi.h's
fd_sample_steered block in numpy -- the shift, the reward terms (through the oracle's NeRF, tests/clash_lddt_reference.py
and tests/psea_reference.py), the reweighting and systematic resampling with its decision margin, and the chain over an
oracle model.
"""
import numpy as np
import torch

import clash_lddt_reference as cref
import psea_reference as pref
import solver_reference as vref
import strided_reference as sref
from oracle import ref_nerf

TERMS = ("clashes", "rg", "helix", "strand")


def shift(x0, offset, is_angle) -> np.ndarray:
    """ang = x0 + offset in float32, rounded once, wrapped where angular; offset None: x0 as it is."""
    x0 = np.asarray(x0, dtype=np.float32)
    if offset is None:
        return x0.copy()
    v = (x0 + np.asarray(offset, dtype=np.float32)).astype(np.float32)
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    if len(cols):
        v[..., cols] = sref._wrap(torch.from_numpy(np.ascontiguousarray(v[..., cols]))).numpy()
    return v


def backbone(ang, feat_idx) -> np.ndarray:
    """float64 [3 len, 3]: the oracle's NeRF of one chain's float32 features [len, F], not centred."""
    ang = np.asarray(ang, dtype=np.float32)
    col = lambda k: None if feat_idx[k] < 0 else ang[:, feat_idx[k]]   # noqa: E731
    return ref_nerf.build(col(0), col(1), col(2), tau=col(3), ca_c_n=col(4), c_n_ca=col(5), center=False, len_c_n=col(6),
                          len_n_ca=col(7), len_ca_c=col(8))


def weighted(weights, terms) -> float:
    """w0 t0 + w1 t1 + w2 t2 + w3 t3, left to right, every product and sum rounded once (Python floats)."""
    r = float(weights[0]) * float(terms[0])
    for k in range(1, 4):
        r = r + float(weights[k]) * float(terms[k])
    return r


def chain_terms(coords, alpha):
    """(clashes, rg, helix fraction, strand fraction, clash margin, P-SEA margin) of one backbone [3 len, 3] float64."""
    n = len(coords) // 3
    count, _, m_clash = cref.clashes(coords.astype(np.float32), alpha)
    ca = coords[1::3]
    rg = float(np.sqrt(((ca - ca.mean(axis=0)) ** 2).sum() / n))
    sse = pref.psea(ca)
    return float(count), rg, sse.count("a") / n, sse.count("b") / n, m_clash, pref.threshold_margin(ca)


def rewards(ang, lens, feat_idx, weights, alpha=0.63):
    """terms float64 [B, 4], reward float64 [B] and the smallest decision margin of the integer terms, for ang [B, L, F]
    (already shifted)."""
    B = len(lens)
    terms, rew, margin = np.zeros((B, 4)), np.zeros(B), np.inf
    for b in range(B):
        t = chain_terms(backbone(ang[b, : lens[b]], feat_idx), alpha)
        terms[b] = t[:4]
        rew[b] = weighted(weights, t[:4])
        margin = min(margin, t[4], t[5])
    return terms, rew, margin


def resample(reward, logw, r_prev, P, lam, ess_frac, u):
    """The resample statement -> (logw, r_prev, ancestors int32 [G P] global, resampled uint8 [G], margin).  Every sum in
    index order (np.cumsum; np.sum would add pairwise).  margin = the smallest |target_k - cumsum_j| / W over the groups that
    resample, and for ess_frac < 1 also every group's |ESS - ess_frac P| / P: what the ulps between two exp() could flip."""
    reward = np.asarray(reward, dtype=np.float64)
    logw = np.asarray(logw, dtype=np.float64) + np.float64(lam) * (reward - np.asarray(r_prev, dtype=np.float64))
    r_prev = reward.copy()
    G = len(reward) // P
    anc = np.arange(G * P, dtype=np.int32)
    flags = np.zeros(G, dtype=np.uint8)
    margin = np.inf
    for g in range(G):
        sl = slice(g * P, (g + 1) * P)
        lw = logw[sl]
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.exp(lw - lw.max())
            cum = np.cumsum(w)
            W, S2 = cum[-1], np.cumsum(w * w)[-1]
            ess = W * W / S2
        if not (np.isfinite(W) and W > 0):
            continue
        if ess_frac < 1:
            margin = min(margin, abs(ess - ess_frac * P) / P)
        if not (ess_frac >= 1 or ess < ess_frac * P):
            continue
        target = (np.float64(u[g]) + np.arange(P, dtype=np.float64)) / np.float64(P) * W
        a = np.minimum(np.searchsorted(cum, target, side="right"), P - 1)   # the smallest j with cum[j] > target
        margin = min(margin, float(np.abs(target[:, None] - cum[None, :]).min() / W))
        anc[sl] = g * P + a
        r_prev[sl] = r_prev[sl][a]
        logw[sl] = 0.0
        flags[g] = 1
    return logw, r_prev, anc, flags, margin


@torch.no_grad()
def chain(model, lens, x_init, visits, coef, noise, event, P, u, feat_idx, weights, lam, ess_frac, offset, is_angle, alpha=0.63):
    """The steered run over a float32 oracle model.  coef [5, K] a | b | s | u | v; noise [K, B, L, F]; u [n_events, G].
    -> dict(out, terms, reward, logw, ancestors [n_events, B], margins [n_events] of the resampling decisions)."""
    x = np.asarray(x_init, dtype=np.float32)
    B = len(lens)
    logw, r_prev = np.zeros(B), np.zeros(B)
    ancestors, margins, e = [], [], 0
    for i, t in enumerate(visits):
        a, b, s, cu, cv = (float(c) for c in coef[:, i])
        eps = sref.forward(model, x, int(t), lens).numpy()
        x0 = vref.update(x, eps, None, a, b, 0.0, cu, cv, is_angle)[1]
        x = sref.update(x, eps, a, b, s, None if s == 0 else noise[i], is_angle)
        if event[i]:
            _, rew, _ = rewards(shift(x0, offset, is_angle), lens, feat_idx, weights, alpha)
            logw, r_prev, anc, _, m = resample(rew, logw, r_prev, P, lam, ess_frac, u[e])
            x = x[anc]
            ancestors.append(anc)
            margins.append(m)
            e += 1
    terms, rew, _ = rewards(shift(x, offset, is_angle), lens, feat_idx, weights, alpha)
    return dict(out=x, terms=terms, reward=rew, logw=logw, ancestors=np.array(ancestors, dtype=np.int32).reshape(e, B),
                margins=np.array(margins))


# ---------------------------------------------------------------------------------------------------- test chains
def angles_of(kind, n, rng, F=6):
    """float32 [n, 6] canonical-full-angles (phi, psi, omega, tau, CA:C:1N, C:1N:1CA) of a helical, an extended or a
    compact random stretch, each with a little noise so that no decision sits on a threshold."""
    deg = np.pi / 180.0
    a = np.zeros((n, F))
    a[:, 2] = np.pi - 0.02
    a[:, 3], a[:, 4], a[:, 5] = 111 * deg, 116 * deg, 121.5 * deg
    if kind == "helix":
        a[:, 0], a[:, 1] = -57 * deg, -47 * deg
    elif kind == "extended":
        a[:, 0], a[:, 1] = -120 * deg, 130 * deg
    else:
        a[:, 0], a[:, 1] = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n)
    a[:, :2] += rng.normal(0.0, 0.03, (n, 2))
    return a.astype(np.float32)
