"""
CPU restatement of restraint guidance (TEST INFRASTRUCTURE ONLY): the statements of include/fdmi.h (fd_nerf_vjp,
fd_restraint_energy, fd_guide_step) in numpy float64 -- float32 where the statement says so -- written from the header, and a
torch float64 restatement of oracle/ref_nerf.place / build (with the frame carried along the chain) that exists for autograd only.

The derivative: atom k >= 3 of a chain was placed from atoms k-3, k-2, k-1; with i = (k - 3) / 3, j = (k - 3) % 3 its torsion,
bond angle and bond length are (slots of fd_nerf's feat_idx, row)
    j = 0: psi 1 (i),     CA:C:1N 4 (i),   0C:1N 6 (i)
    j = 1: omega 2 (i),   C:1N:1CA 5 (i),  N:CA 7 (i)
    j = 2: phi 0 (i + 1), N:CA:C 3 (i),    CA:C 8 (i)
and with g the upstream gradient (minus its mean where centered), q = p - p_0, Fs_k = sum_{m >= k} g_m,
Tq_k = sum_{m >= k} q_m x g_m, b = q_{k-2}, c = q_{k-1}, d = q_k, u = unit(c - b), r = d - c, M = Tq_k - c x Fs_k:
    d / d torsion = u . M,   d / d angle = sa unit(r x u) . M,   d / d length = sl unit(r) . Fs_k
The coordinates alone do not decide the signs sa, sl: r = bl (-cos(angle) u + sin(angle) w) with w the unit vector across u that
the torsion picks, so unit(r x u) is the angle's rotation axis times sign(bl sin(angle)) and unit(r) the bond's direction times
sign(bl) -- (angle, torsion) and (-angle, torsion + pi) build the same chain.  With the float32 rows the forward read (`feats`)
sa = sign(sin(float64(angle))) sign(bl), sl = sign(bl), the sign of zero and of a default counting as +1; without them
sa = sl = 1, which is right where every angle feature has sin > 0 and every length is > 0.
"""
import numpy as np
import torch

import repeat_reference as rr
from oracle import ref_nerf

# (torsion, angle, length) slots of feat_idx for j = 0, 1, 2, and whether the torsion belongs to row i + 1
SLOTS = ((1, 4, 6, 0), (2, 5, 7, 0), (0, 3, 8, 1))


def _unit(v):
    return v / np.sqrt((v * v).sum())


def _sign(v) -> float:
    return -1.0 if v < 0 else 1.0


def nerf_vjp(coords, dcoords, feat_idx, F, centered, feats=None) -> np.ndarray:
    """One chain: float64 [3 len, 3] twice -> float64 [len, F]; ``feats``: the float32 [len, F] rows the forward read, or None
    (every sign +1)."""
    p = np.asarray(coords, dtype=np.float64)
    g = np.asarray(dcoords, dtype=np.float64)
    n = len(p)
    assert p.shape == g.shape == (n, 3) and n % 3 == 0
    if centered:
        g = g - g.mean(axis=0)
    q = p - p[0]
    Fs = np.cumsum(g[::-1], axis=0)[::-1]
    Tq = np.cumsum(np.cross(q, g)[::-1], axis=0)[::-1]
    out = np.zeros((n // 3, F), dtype=np.float64)
    if feats is not None:
        feats = np.asarray(feats, dtype=np.float32)
        assert feats.shape == (n // 3, F)
    for k in range(3, n):
        i, j = divmod(k - 3, 3)
        st, sa, sl, up = SLOTS[j]
        sign_l = _sign(feats[i, feat_idx[sl]]) if feats is not None and feat_idx[sl] >= 0 else 1.0
        sign_a = sign_l * (_sign(np.sin(np.float64(feats[i, feat_idx[sa]]))) if feats is not None and feat_idx[sa] >= 0 else 1.0)
        b, c, d = q[k - 2], q[k - 1], q[k]
        u, r = _unit(c - b), d - c
        M = Tq[k] - np.cross(c, Fs[k])
        out[i + up, feat_idx[st]] += u @ M
        if feat_idx[sa] >= 0:
            out[i, feat_idx[sa]] += sign_a * (_unit(np.cross(r, u)) @ M)
        if feat_idx[sl] >= 0:
            out[i, feat_idx[sl]] += sign_l * (_unit(r) @ Fs[k])
    return out


def restraint_energy(coords, rst):
    """One chain: float64 [3 len, 3] and (i, j, d0, tol, w) lists -> (E, largest v, gradient [3 len, 3]); the gradient of an
    atom is summed in list order."""
    p = np.asarray(coords, dtype=np.float64)
    grad = np.zeros_like(p)
    E, worst = 0.0, 0.0
    for i, j, d0, tol, w in zip(*rst):
        diff = p[i] - p[j]
        d = np.sqrt((diff * diff).sum())
        v = max(0.0, abs(d - d0) - tol)
        E += w * v * v
        worst = max(worst, v)
        if v > 0 and d > 0:
            term = 2.0 * w * v * np.sign(d - d0) * diff / d
            grad[i] += term
            grad[j] -= term
    return E, worst, grad


def shift(x0, offset, is_angle) -> np.ndarray:
    """The shift statement of fd_sample_steered on float32 [rows, F]: x0 + offset rounded once, wrapped where angular; no
    offset: x0 as it is."""
    x0 = np.asarray(x0, dtype=np.float32)
    if offset is None:
        return x0.copy()
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    return rr._wrap_cols((x0 + np.asarray(offset, dtype=np.float32)).astype(np.float32), cols)


def build_ref(ang, feat_idx) -> np.ndarray:
    """oracle/ref_nerf.build (center = False) of float32 [len, F] rows with fd_nerf's columns."""
    ang = np.asarray(ang, dtype=np.float32)
    col = lambda s: None if feat_idx[s] < 0 else ang[:, feat_idx[s]]   # noqa: E731
    return ref_nerf.build(col(0), col(1), col(2), tau=col(3), ca_c_n=col(4), c_n_ca=col(5), center=False, len_c_n=col(6),
                          len_n_ca=col(7), len_ca_c=col(8))


def guide_step(x, x0, lens, feat_idx, offset, is_angle, restraints, c, max_norm, s=0.0, z=None, build=build_ref, signs=True, return_G=False):
    """The guide statement on float32 [B, L, F] arrays; ``restraints``: one (i, j, d0, tol, w) tuple per chain.  Returns
    (x_out, energy [B], gnorm [B], clip factor [B]) and, with ``return_G``, the list of the chains' G; rows at or beyond a length
    keep their bits.  ``signs`` False: the derivative without the shifted rows (every sign +1)."""
    x = np.asarray(x, dtype=np.float32)
    x0 = np.asarray(x0, dtype=np.float32)
    B, L, F = x.shape
    out = x.copy()
    cols = np.nonzero(np.asarray(is_angle, dtype=bool))[0]
    c, s = np.float32(c), np.float32(s)
    energy, gnorm, clip = np.zeros(B), np.zeros(B), np.ones(B)
    Gs = []
    for b in range(B):
        n = int(lens[b])
        ang = shift(x0[b, :n], offset, is_angle)
        coords = build(ang, feat_idx)
        energy[b], _, gc = restraint_energy(coords, restraints[b])
        G = nerf_vjp(coords, gc, feat_idx, F, False, ang if signs else None)
        Gs.append(G)
        gnorm[b] = np.sqrt((G * G).sum())
        clip[b] = max_norm / gnorm[b] if gnorm[b] > max_norm else 1.0
        m = x[b, :n]
        if c != 0:
            m = (m - ((np.float64(c) * clip[b]) * G).astype(np.float32)).astype(np.float32)
        if s != 0:
            m = (m + (s * np.asarray(z, dtype=np.float32)[b, :n]).astype(np.float32)).astype(np.float32)
        out[b, :n] = rr._wrap_cols(m, cols)
    return (out, energy, gnorm, clip, Gs) if return_G else (out, energy, gnorm, clip)


# ------------------------------------------------------------------ torch float64 NeRF, for autograd only
# ref_nerf.place recomputes the frame [bc | nbc | n] of an atom from the three positions before it.  In float64 that costs the
# reference itself more than the gate it is used at: the differences of positions tens of A from the origin, crossed where
# |sin(angle)| goes down to 0.02, leave autograd 1.6e-12 of the largest entry from a long-double evaluation at 600 residues (the
# statement on the same coordinates: 1.1e-13).  The same function with the frame carried -- u = unit(d), m = unit(e_x x u),
# p_k = R d + p, R <- R [u | m x u | m], seeded with ref_nerf.place's frame of the seed atoms, as tests/relax_reference.py's
# nerf_scan does in numpy -- has no such cancellation: autograd within 1.0e-14 of the long-double evaluation at 600 residues, the
# coordinates within 2.3e-13 A (3e-12 to 8.5e-12 A with the frames recomputed).
def _step_t(R, p, bond_angle, bond_length, torsion):
    unit = lambda v: v / torch.linalg.norm(v)   # noqa: E731
    d = torch.stack([-bond_length * torch.cos(bond_angle), bond_length * torch.cos(torsion) * torch.sin(bond_angle),
                     bond_length * torch.sin(torsion) * torch.sin(bond_angle)])
    u = unit(d)
    m = unit(torch.linalg.cross(torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64), u))
    return R @ torch.stack([u, torch.linalg.cross(m, u), m], dim=-1), R @ d + p


def build_torch(feats: torch.Tensor, feat_idx, center: bool) -> torch.Tensor:
    """ref_nerf.build on a float64 [len, F] tensor, differentiable: [3 len, 3]; the frame is carried (above)."""
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    col = lambda s, i, dflt: feats[i, feat_idx[s]] if feat_idx[s] >= 0 else f64(dflt)   # noqa: E731
    unit = lambda v: v / torch.linalg.norm(v)   # noqa: E731
    out = [f64(ref_nerf.N_INIT), f64(ref_nerf.CA_INIT), f64(ref_nerf.C_INIT)]
    bc = unit(out[2] - out[1])
    n = unit(torch.linalg.cross(out[1] - out[0], bc))
    R, p = torch.stack([bc, torch.linalg.cross(n, bc), n], dim=-1), out[2]
    for i in range(feats.shape[0] - 1):
        R, p = _step_t(R, p, col(4, i, ref_nerf.DEFAULT_ANGLE["CA:C:1N"]), col(6, i, ref_nerf.C_N_LENGTH), col(1, i, 0.0))
        out.append(p)
        R, p = _step_t(R, p, col(5, i, ref_nerf.DEFAULT_ANGLE["C:1N:1CA"]), col(7, i, ref_nerf.N_CA_LENGTH), col(2, i, 0.0))
        out.append(p)
        R, p = _step_t(R, p, col(3, i, ref_nerf.DEFAULT_ANGLE["tau"]), col(8, i, ref_nerf.CA_C_LENGTH), col(0, i + 1, 0.0))
        out.append(p)
    xyz = torch.stack(out)
    return xyz - xyz.mean(dim=0) if center else xyz


def autograd_vjp(ang32, feat_idx, dcoords, center):
    """(coordinates of the float64 restatement on these float32 angles, d (coords . dcoords) / d angles by autograd)."""
    feats = torch.tensor(np.asarray(ang32, dtype=np.float32).astype(np.float64), requires_grad=True)
    xyz = build_torch(feats, feat_idx, center)
    if not xyz.requires_grad:   # one residue: the three seed atoms, which no feature moves
        return xyz.numpy(), np.zeros(feats.shape)
    (xyz * torch.from_numpy(np.asarray(dcoords, dtype=np.float64))).sum().backward()
    return xyz.detach().numpy(), feats.grad.numpy()
