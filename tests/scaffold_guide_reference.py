"""
CPU restatement of restraint guidance combined with replacement (TEST INFRASTRUCTURE ONLY): the scaffold-guide statement of
include/fdmi.h (fd_scaffold_guide_step) in numpy float64 -- float32 where the statement says so -- written from the header on
top of tests/guide_reference.py (shift, restraints, derivative) and tests/relax_reference.py (the NeRF scan, the soft clash
term), whose restatements are imported and not copied.
"""
from typing import NamedTuple

import numpy as np

import guide_reference as gr
import relax_reference as xr
import repeat_reference as rr


class Clash(NamedTuple):
    alpha: float = 0.63
    margin: float = 0.15
    w: float = 0.0


def assemble(x0, known, fixed) -> np.ndarray:
    """p = fixed ? known : x0 on float32 [rows, F]; x0 is not looked at where fixed."""
    fixed = np.asarray(fixed, dtype=bool)
    return np.where(fixed, np.asarray(known, dtype=np.float32), np.where(fixed, np.float32(0), np.asarray(x0, dtype=np.float32))).astype(np.float32)


def energy(ang, feat_idx, rst, clash: Clash = Clash(), coords=None):
    """One chain's shifted float32 [len, F] rows -> (E_rst, largest violation, E_clash, G [len, F] unmasked, coords): the scan,
    the restraints, then the clashes where clash.w > 0, and the derivative with the rows' signs."""
    ang = np.asarray(ang, dtype=np.float32)
    if coords is None:
        coords = xr.nerf_scan(ang, np.asarray(feat_idx))
    e_rst, worst, gc = gr.restraint_energy(coords, rst if rst is not None else ([], [], [], [], []))
    e_clash = 0.0
    if clash.w > 0:
        e_clash, g_clash = xr.clash_energy(coords, clash.alpha, clash.margin, clash.w)
        gc = gc + g_clash
    G = gr.nerf_vjp(coords, gc, feat_idx, ang.shape[1], False, ang)
    return e_rst, worst, e_clash, G, coords


def step(x, x0, known, fixed, lens, feat_idx, offset, is_angle, restraints, c, max_norm, s=0.0, z=None, clash: Clash = Clash(),
         build=xr.nerf_scan):
    """The scaffold-guide statement on float32 [B, L, F] arrays; ``fixed`` [B, L, F] per element, ``restraints``: one
    (i, j, d0, tol, w) tuple per chain; ``build(ang, feat_idx)``: the statement's coordinates (the device tests hand in
    fd_nerf_scan's own, as tests/test_guide_gpu.py does with fd_nerf's: numpy's float32 cos / sin are not the device's to the
    last bit).  Returns (x_out, energies [B, 2] restraint | clash, largest violation [B], gnorm [B],
    clip factor [B], the chains' masked G); rows at or beyond a length and fixed elements keep their bits."""
    x = np.asarray(x, dtype=np.float32)
    B, L, F = x.shape
    out = x.copy()
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    c, s = np.float32(c), np.float32(s)
    energies, worst, gnorm, clip = np.zeros((B, 2)), np.zeros(B), np.zeros(B), np.ones(B)
    Gs = []
    for b in range(B):
        n = int(lens[b])
        fx = np.asarray(fixed[b][:n], dtype=bool)
        ang = gr.shift(assemble(x0[b][:n], known[b][:n], fx), offset, is_angle)
        energies[b, 0], worst[b], energies[b, 1], G, _ = energy(ang, feat_idx, restraints[b], clash, coords=build(ang, np.asarray(feat_idx)))
        G = np.where(fx, 0.0, G)
        Gs.append(G)
        gnorm[b] = np.sqrt((G * G).sum())
        clip[b] = max_norm / gnorm[b] if gnorm[b] > max_norm else 1.0
        m = x[b, :n]
        if c != 0:
            m = (m - ((np.float64(c) * clip[b]) * G).astype(np.float32)).astype(np.float32)
        if s != 0:
            m = (m + (s * np.asarray(z, dtype=np.float32)[b, :n]).astype(np.float32)).astype(np.float32)
        out[b, :n] = np.where(fx, x[b, :n], rr._wrap_cols(m, cols))
    return out, energies, worst, gnorm, clip, Gs


# ------------------------------------------------------------------ float64 scan, for finite differences only
# xr.nerf_scan reads float32 rows (the device's statement), and a float32 row cannot carry a step of 1e-6.  The same scan on
# float64 rows: xr.local_displacement on float64 operands, the frame carried as there.
def nerf_scan64(ang64, feat_idx) -> np.ndarray:
    from oracle import ref_nerf
    ang = np.asarray(ang64, dtype=np.float64)
    n = 3 * len(ang)
    out = np.zeros((n, 3))
    out[:3] = ref_nerf.N_INIT, ref_nerf.CA_INIT, ref_nerf.C_INIT
    R, p = xr.seed_frame(), ref_nerf.C_INIT.copy()
    ex = np.array([1.0, 0.0, 0.0])
    for k in range(3, n):
        i, j = divmod(k - 3, 3)
        name, dflt_len, st, sa, sl, up = xr._ATOM[j]
        angle = ref_nerf.DEFAULT_ANGLE[name] if feat_idx[sa] < 0 else ang[i, feat_idx[sa]]
        length = dflt_len if feat_idx[sl] < 0 else ang[i, feat_idx[sl]]
        d = xr.local_displacement(np.float64(angle), np.float64(length), np.float64(ang[i + up, feat_idx[st]]))
        u = xr._unit(d)
        m = xr._unit(np.cross(ex, u))
        p = R @ d + p
        R = R @ np.stack([u, np.cross(m, u), m], axis=-1)
        out[k] = p
    return out


def energy64(ang64, feat_idx, rst, clash: Clash = Clash()):
    """(E_rst + E_clash, unmasked G) of float64 rows, everything in float64."""
    coords = nerf_scan64(ang64, feat_idx)
    e_rst, _, gc = gr.restraint_energy(coords, rst)
    e_clash = 0.0
    if clash.w > 0:
        e_clash, g_clash = xr.clash_energy(coords, clash.alpha, clash.margin, clash.w)
        gc = gc + g_clash
    ang = np.asarray(ang64, dtype=np.float64)
    # (gr.nerf_vjp takes the signs from float32 rows; the rows of these tests keep their signs under the rounding)
    return e_rst + e_clash, gr.nerf_vjp(coords, gc, feat_idx, ang.shape[1], False, ang.astype(np.float32))
