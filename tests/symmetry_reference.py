"""
CPU restatement of the cyclic-oligomer statements (TEST INFRASTRUCTURE ONLY): the symmetry statement, the docking descent and
the scaffold-guide statement with its symmetry lines (include/fdmi.h: fd_symmetry_energy, fd_symmetry_dock,
fd_scaffold_guide_step_sym) in numpy float64, written from the header on top of tests/relax_reference.py,
tests/template_reference.py and tests/scaffold_guide_reference.py, whose restatements are imported and not copied.
"""
from typing import NamedTuple, Optional

import numpy as np

import guide_reference as gr
import relax_reference as xr
import repeat_reference as rr
import scaffold_guide_reference as sg
import template_reference as tr


class Params(NamedTuple):
    alpha: float = 0.63
    margin: float = 0.15
    w_clash: float = 1.0
    w_contact: float = 0.1
    d_on: float = 8.0
    d_off: float = 12.0
    w_radial: float = 0.01
    r_max: float = 0.0
    lever: float = 10.0
    max_shift: float = 1.0
    step0: float = 0.01
    grow: float = 1.2
    shrink: float = 0.5
    pose_iters: int = 1


class Energy(NamedTuple):
    e: np.ndarray          # [3] clash | contact | radial
    contacts: int
    wrench: np.ndarray     # [6] F | tau
    dcoords: np.ndarray    # [3 len, 3] = g Q
    g: np.ndarray          # [3 len, 3] in the assembly frame
    y: np.ndarray          # [3 len, 3] the placed chain
    min_gap: float         # the smallest | d - d_on | over the CA pairs between copies (inf without one)


def rot_z(k: int, n: int) -> np.ndarray:
    c, s = np.cos(2.0 * np.pi * k / n), np.sin(2.0 * np.pi * k / n)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def place(coords, pose) -> np.ndarray:
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    return np.asarray(coords, dtype=np.float64).reshape(-1, 3) @ pose[:9].reshape(3, 3).T + pose[9:]


def energy(coords, order: int, pose, prm: Params = Params()) -> Energy:
    """One chain's [3 len, 3] coordinates, its order and pose -> the symmetry statement's values."""
    p = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    Q = pose[:9].reshape(3, 3)
    n_at = len(p)
    y = place(p, pose)
    g = np.zeros_like(y)
    if order < 2:
        return Energy(np.zeros(3), 0, np.zeros(6), np.zeros_like(y), g, y, np.inf)
    idx = np.arange(n_at)
    r = xr.RADII[idx % 3]
    lim = prm.alpha * (r[:, None] + r[None, :]) + prm.margin
    ca = (idx % 3 == 1)
    ca_pair = ca[:, None] & ca[None, :]
    span = prm.d_off - prm.d_on
    e_clash = e_con = 0.0
    contacts = 0
    min_gap = np.inf
    for k in range(1, order):
        partner = y @ rot_z(k, order).T
        diff = y[:, None, :] - partner[None, :, :]
        d = np.sqrt((diff * diff).sum(axis=2))
        v = np.maximum(0.0, lim - d)
        e_clash += 0.5 * prm.w_clash * (v * v).sum()
        u = np.clip((prm.d_off - d) / span, 0.0, 1.0)
        s = np.where(ca_pair, u * u * (3.0 - 2.0 * u), 0.0)
        e_con += -0.5 * prm.w_contact * s.sum()
        contacts += int((ca_pair & (d < prm.d_on)).sum())
        if ca_pair.any():
            min_gap = min(min_gap, float(np.abs(d[ca_pair] - prm.d_on).min()))
        slope = -2.0 * prm.w_clash * v + np.where(ca_pair, 6.0 * prm.w_contact * u * (1.0 - u) / span, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            kf = np.where(d > 0, slope / d, 0.0)
        g += (kf[:, :, None] * diff).sum(axis=1)
    c = y[ca].mean(axis=0)
    rho = np.sqrt(c[0] * c[0] + c[1] * c[1])
    ex = max(0.0, rho - prm.r_max)
    e_rad = prm.w_radial * ex * ex
    if rho > 0:
        g[ca] += 2.0 * prm.w_radial * ex * np.array([c[0], c[1], 0.0]) / (rho * ca.sum())
    wrench = np.concatenate([g.sum(axis=0), np.cross(y, g).sum(axis=0)])
    return Energy(np.array([e_clash, e_con, e_rad]), contacts, wrench, g @ Q, g, y, min_gap)


def rodrigues(w) -> np.ndarray:
    theta = float(np.sqrt((w * w).sum()))
    if not theta > 0:
        return np.eye(3)
    u = w / theta
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.cos(theta) * np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * np.outer(u, u)


def trial(pose, wrench, h: float, prm: Params) -> np.ndarray:
    """The next trial pose of the docking descent from the pose's wrench."""
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    dt = -h * wrench[:3]
    w = -h * wrench[3:] / (prm.lever * prm.lever)
    m = max(np.sqrt((dt * dt).sum()), prm.lever * np.sqrt((w * w).sum()))
    k = prm.max_shift / m if m > prm.max_shift else 1.0
    R = rodrigues(k * w)
    return np.concatenate([(R @ pose[:9].reshape(3, 3)).reshape(9), R @ pose[9:] + k * dt])


def dock(coords, order: int, pose, prm: Params, n_iter: int, h: Optional[float] = None):
    """One chain: the docking descent -> (pose, Energy at it, trace [n_iter + 1], accepted, h)."""
    pose = np.asarray(pose, dtype=np.float64).reshape(12).copy()
    h = prm.step0 if h is None else float(h)
    cur = energy(coords, order, pose, prm)
    E = (cur.e[0] + cur.e[1]) + cur.e[2]
    trace, accepted = [E], 0
    for _ in range(n_iter):
        pt = trial(pose, cur.wrench, h, prm)
        nxt = energy(coords, order, pt, prm)
        Et = (nxt.e[0] + nxt.e[1]) + nxt.e[2]
        if Et <= E:
            pose, cur, E = pt, nxt, Et
            h *= prm.grow
            accepted += 1
        else:
            h *= prm.shrink
        trace.append(E)
    return pose, cur, np.array(trace), accepted, h


def fit_pose(coords, placed):
    """The pose of the proper rigid fit of coords onto placed (all atoms, unit weights) through the template statement:
    (pose [12], rmsd)."""
    p = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    fit = tr.template_energy(p, (np.arange(len(p)), np.asarray(placed, dtype=np.float64).reshape(-1, 3), np.ones(len(p))))
    return np.concatenate([fit.R.T.reshape(9), -fit.R.T @ fit.t]), fit.rmsd


def assembly(coords, pose, order: int) -> np.ndarray:
    y = place(coords, pose)
    return np.stack([y @ rot_z(k, order).T for k in range(order)])


def explicit_interchain(chains, prm: Params):
    """The inter-chain energy clash + contact of an explicit assembly [n, 3 len, 3], every unordered pair of chains once, and the
    unordered CA pairs below d_on between different chains."""
    n, n_at = len(chains), chains.shape[1]
    idx = np.arange(n_at)
    r = xr.RADII[idx % 3]
    lim = prm.alpha * (r[:, None] + r[None, :]) + prm.margin
    ca_pair = (idx % 3 == 1)[:, None] & (idx % 3 == 1)[None, :]
    E, contacts = 0.0, 0
    for i in range(n):
        for j in range(i + 1, n):
            d = np.sqrt(((chains[i][:, None, :] - chains[j][None, :, :]) ** 2).sum(axis=2))
            v = np.maximum(0.0, lim - d)
            u = np.clip((prm.d_off - d) / (prm.d_off - prm.d_on), 0.0, 1.0)
            E += prm.w_clash * (v * v).sum() - prm.w_contact * np.where(ca_pair, u * u * (3.0 - 2.0 * u), 0.0).sum()
            contacts += int((ca_pair & (d < prm.d_on)).sum())
    return E, contacts


def hard_clashes_between(chains, alpha: float = 0.63) -> int:
    """fd_backbone_clashes' rule between the copies of an assembly, on float32-rounded coordinates: the atoms of copy 0 that lie
    within alpha (r_a + r_b) of an atom of another copy."""
    c = np.asarray(chains, dtype=np.float32).astype(np.float64)
    idx = np.arange(c.shape[1])
    r = xr.RADII[idx % 3]
    hit = np.zeros(c.shape[1], dtype=bool)
    for j in range(1, len(c)):
        d = np.sqrt(((c[0][:, None, :] - c[j][None, :, :]) ** 2).sum(axis=2))
        hit |= (d <= alpha * (r[:, None] + r[None, :])).any(axis=1)
    return int(hit.sum())


def step(x, x0, known, fixed, lens, feat_idx, offset, is_angle, restraints, templates, orders, pose_in, placed_in, prm: Params, h_in, c,
         max_norm, s=0.0, z=None, clash: sg.Clash = sg.Clash(), build=xr.nerf_scan):
    """tr.step with the symmetry lines behind the template line.  ``placed_in``: a list of [3 len, 3] arrays or None.  Returns
    (x_out, energies [B, 3], largest violation [B], gnorm [B], template rmsd [B], symmetry energies [B, 3], contacts [B],
    poses [B, 12], placed (list), h [B])."""
    x = np.asarray(x, dtype=np.float32)
    B, L, F = x.shape
    out = x.copy()
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    c, s = np.float32(c), np.float32(s)
    energies, worst, gnorm, rmsd = np.zeros((B, 3)), np.zeros(B), np.zeros(B), np.zeros(B)
    sym_e, contacts, poses, placed, hs = np.zeros((B, 3)), np.zeros(B, dtype=np.int64), np.zeros((B, 12)), [], np.zeros(B)
    for b in range(B):
        n = int(lens[b])
        fx = np.asarray(fixed[b][:n], dtype=bool)
        ang = gr.shift(sg.assemble(x0[b][:n], known[b][:n], fx), offset, is_angle)
        coords = build(ang, np.asarray(feat_idx))
        e_rst, worst[b], gc = gr.restraint_energy(coords, restraints[b] if restraints[b] is not None else ([], [], [], [], []))
        e_clash = 0.0
        if clash.w > 0:
            e_clash, g_clash = xr.clash_energy(coords, clash.alpha, clash.margin, clash.w)
            gc = gc + g_clash
        fit = tr.template_energy(coords, templates[b] if templates[b] is not None else tr.NO_TEMPLATE)
        gc = gc + fit.grad
        energies[b], rmsd[b] = (e_rst, e_clash, fit.energy), fit.rmsd
        pose, h = np.asarray(pose_in[b], dtype=np.float64), float(h_in[b])
        if orders[b] >= 2:
            if placed_in is not None:
                pose, _ = fit_pose(coords, placed_in[b])
            pose, _, _, _, h = dock(coords, int(orders[b]), pose, prm, prm.pose_iters, h)
            ev = energy(coords, int(orders[b]), pose, prm)
            gc = gc + ev.dcoords
            sym_e[b], contacts[b] = ev.e, ev.contacts
        poses[b], hs[b] = pose, h
        placed.append(place(coords, pose))
        G = gr.nerf_vjp(coords, gc, feat_idx, F, False, ang)
        G = np.where(fx, 0.0, G)
        gnorm[b] = np.sqrt((G * G).sum())
        clip = max_norm / gnorm[b] if gnorm[b] > max_norm else 1.0
        m = x[b, :n]
        if c != 0:
            m = (m - ((np.float64(c) * clip) * G).astype(np.float32)).astype(np.float32)
        if s != 0:
            m = (m + (s * np.asarray(z, dtype=np.float32)[b, :n]).astype(np.float32)).astype(np.float32)
        out[b, :n] = np.where(fx, x[b, :n], rr._wrap_cols(m, cols))
    return out, energies, worst, gnorm, rmsd, sym_e, contacts, poses, placed, hs


def random_pose(rng, radius: float) -> np.ndarray:
    """A random proper rotation and a translation of length up to `radius`."""
    return np.concatenate([tr.random_rotation(rng).reshape(9), rng.uniform(-1.0, 1.0, 3) * radius / np.sqrt(3.0)])
