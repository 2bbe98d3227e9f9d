"""
CPU restatement of the superposition restraints (TEST INFRASTRUCTURE ONLY): the template statement of include/fdmi.h
(fd_template_energy) in numpy float64 with np.linalg.eigh in place of the device's Jacobi sweeps, and the scaffold-guide
statement with its template line (fd_scaffold_guide_step_tpl), written from the header on top of tests/guide_reference.py,
tests/relax_reference.py and tests/scaffold_guide_reference.py, whose restatements are imported and not copied.
"""
from typing import NamedTuple

import numpy as np

import guide_reference as gr
import relax_reference as xr
import repeat_reference as rr
import scaffold_guide_reference as sg


class Fit(NamedTuple):
    energy: float
    rmsd: float
    grad: np.ndarray       # [3 len, 3], zero on the atoms that are not named
    R: np.ndarray          # [3, 3]
    t: np.ndarray          # [3]
    gap: float             # (largest - second eigenvalue) / (largest - smallest) of Horn's matrix; 0 where R is not unique
    extent: float          # the largest distance of a named atom from the centroid cp
    residuals: np.ndarray  # [n, 3]


def horn_matrix(M) -> np.ndarray:
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def rotation_of(q) -> np.ndarray:
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def template_energy(coords, tpl) -> Fit:
    """One chain's [3 len, 3] coordinates and its template (atoms, xyz [n, 3], w) -> the statement's values."""
    p_all = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    atoms, m, w = np.asarray(tpl[0], dtype=np.int64), np.asarray(tpl[1], dtype=np.float64).reshape(-1, 3), np.asarray(tpl[2], dtype=np.float64)
    grad = np.zeros_like(p_all)
    if not len(atoms):
        return Fit(0.0, 0.0, grad, np.eye(3), np.zeros(3), 0.0, 0.0, np.zeros((0, 3)))
    p = p_all[atoms]
    W = w.sum()
    cp, cm = (w[:, None] * p).sum(0) / W, (w[:, None] * m).sum(0) / W
    u, v = m - cm, p - cp
    M = np.einsum("k,ki,kj->ij", w, u, v)
    lam, vec = np.linalg.eigh(horn_matrix(M))
    R = rotation_of(vec[:, -1])
    r = v - u @ R.T
    E = float((w * (r * r).sum(1)).sum())
    grad[atoms] = 2.0 * w[:, None] * r
    spread = lam[-1] - lam[0]
    return Fit(E, float(np.sqrt(E / W)), grad, R, cp - R @ cm, float((lam[-1] - lam[-2]) / spread) if spread > 0 else 0.0,
               float(np.sqrt((v * v).sum(1)).max()), r)


def mirrored(tpl):
    """The template reflected in z."""
    return tpl[0], np.asarray(tpl[1], dtype=np.float64).reshape(-1, 3) * np.array([1.0, 1.0, -1.0]), tpl[2]


NO_TEMPLATE = ([], np.zeros((0, 3)), [])


def energy(ang, feat_idx, rst, tpl, clash: sg.Clash = sg.Clash(), coords=None):
    """sg.energy with the template line behind the clash line: (E_rst, largest violation, E_clash, E_tpl, rmsd, unmasked G,
    coords)."""
    ang = np.asarray(ang, dtype=np.float32)
    if coords is None:
        coords = xr.nerf_scan(ang, np.asarray(feat_idx))
    e_rst, worst, gc = gr.restraint_energy(coords, rst if rst is not None else ([], [], [], [], []))
    e_clash = 0.0
    if clash.w > 0:
        e_clash, g_clash = xr.clash_energy(coords, clash.alpha, clash.margin, clash.w)
        gc = gc + g_clash
    fit = template_energy(coords, tpl if tpl is not None else NO_TEMPLATE)
    gc = gc + fit.grad
    return e_rst, worst, e_clash, fit.energy, fit.rmsd, gr.nerf_vjp(coords, gc, feat_idx, ang.shape[1], False, ang), coords


def step(x, x0, known, fixed, lens, feat_idx, offset, is_angle, restraints, templates, c, max_norm, s=0.0, z=None,
         clash: sg.Clash = sg.Clash(), build=xr.nerf_scan):
    """sg.step with one template per chain: (x_out, energies [B, 3] restraint | clash | template, largest violation [B],
    gnorm [B], template rmsd [B], the chains' masked G)."""
    x = np.asarray(x, dtype=np.float32)
    B, L, F = x.shape
    out = x.copy()
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    c, s = np.float32(c), np.float32(s)
    energies, worst, gnorm, rmsd = np.zeros((B, 3)), np.zeros(B), np.zeros(B), np.zeros(B)
    Gs = []
    for b in range(B):
        n = int(lens[b])
        fx = np.asarray(fixed[b][:n], dtype=bool)
        ang = gr.shift(sg.assemble(x0[b][:n], known[b][:n], fx), offset, is_angle)
        energies[b, 0], worst[b], energies[b, 1], energies[b, 2], rmsd[b], G, _ = energy(
            ang, feat_idx, restraints[b], templates[b], clash, coords=build(ang, np.asarray(feat_idx)))
        G = np.where(fx, 0.0, G)
        Gs.append(G)
        gnorm[b] = np.sqrt((G * G).sum())
        clip = max_norm / gnorm[b] if gnorm[b] > max_norm else 1.0
        m = x[b, :n]
        if c != 0:
            m = (m - ((np.float64(c) * clip) * G).astype(np.float32)).astype(np.float32)
        if s != 0:
            m = (m + (s * np.asarray(z, dtype=np.float32)[b, :n]).astype(np.float32)).astype(np.float32)
        out[b, :n] = np.where(fx, x[b, :n], rr._wrap_cols(m, cols))
    return out, energies, worst, gnorm, rmsd, Gs


def energy64(ang64, feat_idx, tpl):
    """(E_tpl, unmasked G) of float64 rows, everything in float64 (finite differences)."""
    coords = sg.nerf_scan64(ang64, feat_idx)
    fit = template_energy(coords, tpl)
    ang = np.asarray(ang64, dtype=np.float64)
    return fit.energy, gr.nerf_vjp(coords, fit.grad, feat_idx, ang.shape[1], False, ang.astype(np.float32))


def random_rotation(rng) -> np.ndarray:
    q = rng.standard_normal(4)
    return rotation_of(q / np.linalg.norm(q))
