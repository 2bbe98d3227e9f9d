"""
CPU restatement of the torsion-space relaxer (TEST INFRASTRUCTURE ONLY): the three statements of include/fdmi.h (fd_nerf_scan,
fd_relax_energy, fd_relax) in numpy float64 -- float32 where the statement says so -- written from the header.

The scan: the displacement (d0, d1, d2) of atom k >= 3 is oracle/ref_nerf.place's, from the same operands (so numpy's promotion
gives the same float32 products); the frame is carried, not recomputed: u = unit(d), m = unit(e_x x u), M = [u | m x u | m],
p_k = R d + p, R <- R M, seeded with ref_nerf.place's frame of the three seed atoms.  Composed left to right here; the device
composes the same transforms in a tree.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np

import guide_reference as gr
import repeat_reference as rr
from oracle import ref_nerf

RADII = np.array([1.55, 1.7, 1.7])
# (angle name, default length, torsion slot, angle slot, length slot, torsion row offset) of atom k = 3 i + 3 + j
_ATOM = (("CA:C:1N", ref_nerf.C_N_LENGTH, 1, 4, 6, 0), ("C:1N:1CA", ref_nerf.N_CA_LENGTH, 2, 5, 7, 0), ("tau", ref_nerf.CA_C_LENGTH, 0, 3, 8, 1))


def _unit(v):
    return v / np.sqrt((v * v).sum())


def local_displacement(bond_angle, bond_length, torsion) -> np.ndarray:
    """The vector ref_nerf.place multiplies its frame with: the same expressions on the same operands."""
    return np.array([-bond_length * np.cos(bond_angle), bond_length * np.cos(torsion) * np.sin(bond_angle),
                     bond_length * np.sin(torsion) * np.sin(bond_angle)], dtype=np.float64)


def seed_frame() -> np.ndarray:
    bc = _unit(ref_nerf.C_INIT - ref_nerf.CA_INIT)
    n = _unit(np.cross(ref_nerf.CA_INIT - ref_nerf.N_INIT, bc))
    return np.stack([bc, np.cross(n, bc), n], axis=-1)


def nerf_scan(ang, feat_idx, center: bool = False) -> np.ndarray:
    """float32 [len, F] rows with fd_nerf's columns -> float64 [3 len, 3], the frame composed along the chain."""
    ang = np.asarray(ang, dtype=np.float32)
    n = 3 * len(ang)
    out = np.zeros((n, 3))
    out[:3] = ref_nerf.N_INIT, ref_nerf.CA_INIT, ref_nerf.C_INIT
    R, p = seed_frame(), ref_nerf.C_INIT.copy()
    ex = np.array([1.0, 0.0, 0.0])
    for k in range(3, n):
        i, j = divmod(k - 3, 3)
        name, dflt_len, st, sa, sl, up = _ATOM[j]
        angle = ref_nerf.DEFAULT_ANGLE[name] if feat_idx[sa] < 0 else ang[i, feat_idx[sa]]
        length = dflt_len if feat_idx[sl] < 0 else ang[i, feat_idx[sl]]
        d = local_displacement(angle, length, ang[i + up, feat_idx[st]])
        u = _unit(d)
        m = _unit(np.cross(ex, u))
        p = R @ d + p
        R = R @ np.stack([u, np.cross(m, u), m], axis=-1)
        out[k] = p
    return out - out.mean(axis=0) if center else out


def scan_gate(coords) -> float:
    """1e-9 x the chain's largest |p_k - p_0|."""
    c = np.asarray(coords)
    return 1e-9 * np.sqrt(((c - c[0]) ** 2).sum(axis=1)).max()


class Params(NamedTuple):
    feat_idx: Sequence[int]
    is_angle: Sequence[bool]
    move: Sequence[bool]
    alpha: float = 0.63
    margin: float = 0.15
    w_clash: float = 1.0
    w_tether: float = 0.0
    step0: float = 0.01
    grow: float = 1.2
    shrink: float = 0.5
    max_step: float = 0.5


def clash_energy(coords, alpha, margin, w):
    """The soft clash term on float64 [3 len, 3] -> (E, gradient [3 len, 3])."""
    p = np.asarray(coords, dtype=np.float64)
    n = len(p)
    idx = np.arange(n)
    r = RADII[idx % 3]
    diff = p[:, None, :] - p[None, :, :]
    d = np.sqrt((diff * diff).sum(axis=2))
    t = alpha * (r[:, None] + r[None, :]) + margin
    apart = np.abs(idx[:, None] - idx[None, :]) >= 2
    v = np.where(apart, np.maximum(0.0, t - d), 0.0)
    E = w * (v * v)[idx[:, None] < idx[None, :]].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where((v > 0) & (d > 0), -2.0 * w * v / d, 0.0)
    return E, (k[:, :, None] * diff).sum(axis=1)


def wrap64(v):
    return v - 2.0 * np.pi * np.floor((v + np.pi) / (2.0 * np.pi))


def relax_energy(x, anchor, prm: Params, fixed=None, rst=None, coords=None, build=nerf_scan, signs=True):
    """One chain, float32 [len, F] -> (energies [3], G [len, F], gnorm, coords).  ``coords``: evaluate on these (the device's
    own) instead of building them; ``rst``: an (i, j, d0, tol, w) tuple or None; ``anchor`` None: the input itself; ``signs``
    False: the derivative without the rows (every sign +1: right for sin(angle) > 0 and lengths > 0 only)."""
    x = np.asarray(x, dtype=np.float32)
    n, F = x.shape
    idx = np.asarray(prm.feat_idx)
    if coords is None:
        coords = build(x, idx)
    e_clash, gc = clash_energy(coords, prm.alpha, prm.margin, prm.w_clash)
    e_rst, _, g_rst = gr.restraint_energy(coords, rst if rst is not None else ([], [], [], [], []))
    gc = gc + g_rst
    G = gr.nerf_vjp(coords, gc, idx, F, False, x if signs else None)
    move = np.asarray(prm.move, dtype=bool)[:F]
    ang = np.asarray(prm.is_angle, dtype=bool)[:F]
    delta = x.astype(np.float64) - np.asarray(x if anchor is None else anchor, dtype=np.float32).astype(np.float64)
    delta[:, ang] = wrap64(delta[:, ang])
    e_tether = prm.w_tether * (delta[:, move] ** 2).sum()
    G = G + 2.0 * prm.w_tether * delta
    G[:, ~move] = 0.0
    if fixed is not None:
        G[np.asarray(fixed, dtype=bool)[:n]] = 0.0
    return np.array([e_clash, e_rst, e_tether]), G, float(np.sqrt((G * G).sum())), coords


def trial(x, G, gnorm, h, prm: Params) -> np.ndarray:
    """x' of the descent statement from the state's gradient and norm."""
    x = np.asarray(x, dtype=np.float32)
    s = prm.max_step / gnorm if h * gnorm > prm.max_step else h
    moved = (x - (s * G).astype(np.float32)).astype(np.float32)
    ang = np.nonzero(np.asarray(prm.is_angle, dtype=bool)[: x.shape[1]])[0]
    moved = rr._wrap_cols(moved, ang)
    return np.where(G != 0, moved, x)


def relax(x, anchor, prm: Params, n_iter: int, fixed=None, rst=None, h: Optional[float] = None, signs=True):
    """One chain: the descent statement -> (x, energies [3], trace [n_iter + 1], accepted, h).  ``anchor`` None: the input."""
    x = np.asarray(x, dtype=np.float32).copy()
    anchor = x.copy() if anchor is None else np.asarray(anchor, dtype=np.float32)
    h = prm.step0 if h is None else float(h)
    E3, G, gn, _ = relax_energy(x, anchor, prm, fixed, rst, signs=signs)
    E = (E3[0] + E3[1]) + E3[2]
    trace, accepted = [E], 0
    for _ in range(n_iter):
        xt = trial(x, G, gn, h, prm)
        E3t, Gt, gnt, _ = relax_energy(xt, anchor, prm, fixed, rst, signs=signs)
        Et = (E3t[0] + E3t[1]) + E3t[2]
        if Et <= E:
            x, E3, E, G, gn = xt, E3t, Et, Gt, gnt
            h *= prm.grow
            accepted += 1
        else:
            h *= prm.shrink
        trace.append(E)
    return x, E3, np.array(trace), accepted, h


def count_clashes(coords, alpha=0.63) -> int:
    """The integer rule of DESIGN 6h on float32-rounded coordinates: atoms that clash with at least one other."""
    p = np.asarray(coords, dtype=np.float32).astype(np.float64)
    n = len(p)
    idx = np.arange(n)
    r = RADII[idx % 3]
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    hit = (np.abs(idx[:, None] - idx[None, :]) >= 2) & (d <= alpha * (r[:, None] + r[None, :]))
    return int(hit.any(axis=1).sum())


# ------------------------------------------------------------------ the chains of the device tests: torsions only
def helix_chain(seed: int, n: int = 40) -> np.ndarray:
    """An ideal helix (phi -1.0, psi -0.8, omega pi) with a fifth of the residues' phi / psi perturbed by N(0, 0.8)."""
    rng = np.random.default_rng(seed)
    x = np.tile(np.array([-1.0, -0.8, np.pi]), (n, 1))
    hit = rng.choice(n, size=max(1, n // 5), replace=False)
    x[hit, :2] += rng.normal(0.0, 0.8, size=(len(hit), 2))
    return rr._wrap_cols(x.astype(np.float32), np.array([0, 1]))


def random_chain(seed: int, n: int = 40) -> np.ndarray:
    """Uniformly random phi / psi with omega = pi."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-np.pi, np.pi, size=(n, 2)), np.full((n, 1), np.pi)], axis=1)
    return x.astype(np.float32)


# the batch of tests/test_relax_gpu.py's descent: (kind, residues, seed); tests/test_relax.py asserts that the statement above
# brings every one of them to E_clash == 0 and zero clashing atoms within the device test's 60 iterations
DEVICE_CHAINS = (("helix", 12, 6), ("random", 40, 4), ("helix", 40, 7), ("random", 64, 2), ("helix", 86, 2), ("random", 128, 1))
IDX3 = np.array([0, 1, 2, -1, -1, -1, -1, -1, -1], dtype=np.int32)


def device_chains():
    return [(helix_chain if kind == "helix" else random_chain)(seed, n) for kind, n, seed in DEVICE_CHAINS]
