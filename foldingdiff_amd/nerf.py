"""
NeRF: sampled angles -> Cartesian backbone coordinates on the GPU (one C-ABI call, ``fd_nerf``).

Mirrors the part of foldingdiff/nerf.py that the sampler's post-processing uses
(``NERFBuilder`` :27-142 as driven by ``create_new_chain_nerf``,
foldingdiff/angles_and_coords.py:112-184): N, CA, C positions built from phi / psi / omega, the
bond angles and (if the feature set has them) bond lengths; constants otherwise.  Writing PDB
files (biotite) stays outside this path.
"""
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _binding

N_CA_LENGTH = 1.46
CA_C_LENGTH = 1.54
C_N_LENGTH = 1.34
N_INIT = np.array([17.047, 14.099, 3.625])
CA_INIT = np.array([16.967, 12.784, 4.338])
C_INIT = np.array([15.685, 12.755, 5.133])

# feature name -> slot of fd_nerf's feat_idx (create_new_chain_nerf's name mapping, angles_and_coords.py:150-173)
_SLOT = {"phi": 0, "psi": 1, "omega": 2, "tau": 3, "N:CA:C": 3, "CA:C:1N": 4, "C:1N:1CA": 5,
         "0C:1N": 6, "N:CA": 7, "CA:C": 8}


def feature_columns(feature_names: Sequence[str]) -> np.ndarray:
    """int32 [9]: ``fd_nerf``'s ``feat_idx`` for these column names, -1 for a bond angle or length that is not a feature."""
    for req in ("phi", "psi", "omega"):
        assert req in feature_names, f"NeRF needs the dihedral {req!r}"
    idx = np.full(9, -1, dtype=np.int32)
    for col, name in enumerate(feature_names):
        if name not in _SLOT:
            raise ValueError(f"Unrecognized feature: {name}")
        idx[_SLOT[name]] = col
    return idx


def build_backbones(
    angles: Union[np.ndarray, Sequence[np.ndarray]],
    feature_names: Sequence[str],
    center_coords: bool = True,
    device: int = 0,
    method: str = "serial",
) -> List[np.ndarray]:
    """Coordinates for a batch of sampled backbones.

    ``angles``: ``[B, L, F]`` array or a list of ``[len_i, F]`` arrays (e.g. ``[s[-1] for s in sample(...)]``);
    ``feature_names``: the F column names (``dset.feature_names["angles"]``).  Returns one
    ``float64 [3 * len_i, 3]`` array per chain (N, CA, C per residue), centred like
    ``NERFBuilder.centered_cartesian_coords`` unless ``center_coords=False``.

    ``method``: ``"serial"`` is ``fd_nerf``, one lane per chain, bit for bit the reference's arithmetic; ``"scan"`` is
    ``fd_nerf_scan``, one workgroup per chain (chains of at most 2048 residues), which composes the frames along the chain
    instead of recomputing each from three positions and so differs from ``"serial"`` in the last bits (within 1e-9 of the
    chain's extent)."""
    if method not in ("serial", "scan"):
        raise ValueError(f"method={method!r}: 'serial' or 'scan'")
    chains = [np.asarray(a, dtype=np.float32) for a in (angles if not isinstance(angles, np.ndarray) or angles.ndim != 3 else list(angles))]
    F = len(feature_names)
    assert all(c.ndim == 2 and c.shape[1] == F for c in chains), "each chain must be [len, F]"
    idx = feature_columns(feature_names)
    B, L = len(chains), max(len(c) for c in chains)
    feats = np.zeros((B, L, F), dtype=np.float32)
    lens = np.zeros(B, dtype=np.int32)
    for i, c in enumerate(chains):
        feats[i, : len(c)] = c
        lens[i] = len(c)
    out = np.empty((B, 3 * L, 3), dtype=np.float64)
    ptr = _binding.ptr
    entry = _binding.load().fd_nerf if method == "serial" else _binding.load().fd_nerf_scan
    _binding.check(entry(device, ptr(feats), ptr(lens), B, L, F, ptr(idx), 1 if center_coords else 0, ptr(out)))
    return [out[i, : 3 * lens[i]].copy() for i in range(B)]


def _vjp_padded(coords: np.ndarray, lens: np.ndarray, dcoords: np.ndarray, F: int, idx: np.ndarray, centered: bool, device: int,
                feats: Optional[np.ndarray] = None) -> np.ndarray:
    """``fd_nerf_vjp`` -- with ``feats`` (float32 ``[B, L, F]``) ``fd_nerf_vjp_feats`` -- on padded arrays: float64
    ``[B, 3L, 3]`` twice -> float64 ``[B, L, F]`` (rows at or beyond a length 0)."""
    B, L = coords.shape[0], coords.shape[1] // 3
    out = np.zeros((B, L, F), dtype=np.float64)
    ptr = _binding.ptr
    lib = _binding.load()
    if feats is None:
        _binding.check(lib.fd_nerf_vjp(device, ptr(coords), ptr(lens), B, L, F, ptr(idx), 1 if centered else 0, ptr(dcoords), ptr(out)))
    else:
        assert feats.dtype == np.float32 and feats.shape == (B, L, F) and feats.flags.c_contiguous
        _binding.check(lib.fd_nerf_vjp_feats(device, ptr(coords), ptr(lens), B, L, F, ptr(idx), 1 if centered else 0, ptr(dcoords), ptr(feats), ptr(out)))
    return out


def coords_vjp(
    coords: Sequence[np.ndarray],
    dcoords: Sequence[np.ndarray],
    feature_names: Sequence[str],
    centered: bool = True,
    device: int = 0,
    angles: Optional[Sequence[np.ndarray]] = None,
) -> List[np.ndarray]:
    """The gradient of any function of backbone coordinates with respect to the angles (and bond lengths) NeRF built them
    from, on the GPU.

    ``angles``: the ``[len_i, F]`` rows ``build_backbones`` was given (``fd_nerf_vjp_feats``): exact wherever the forward is
    finite.  Without them (``fd_nerf_vjp``, from the coordinates alone) the result is exact only where every bond-angle feature
    has ``sin > 0`` and every bond-length feature is ``> 0``, as a backbone's are; elsewhere the bond-angle and bond-length
    entries come out with the wrong sign, because ``(angle, torsion)`` and ``(-angle, torsion + pi)`` build the same chain.

    ``coords``: one ``[3 len_i, 3]`` array per chain, as ``build_backbones`` returns them; ``dcoords``: the function's
    gradient with respect to them, the same shapes; ``centered``: the coordinates came from ``center_coords=True``.  Returns
    one ``float64 [len_i, F]`` array per chain in the column order of ``feature_names`` (a torsion, an angle or a bond
    length moves everything behind it as a rigid body), fp64, the same bits on every call.  Columns and rows NeRF does not
    read (phi of the first residue, the last residue's other angles) are 0."""
    xs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in coords]
    gs = [np.asarray(g, dtype=np.float64).reshape(-1, 3) for g in dcoords]
    assert len(xs) == len(gs) and len(xs) > 0 and all(x.shape == g.shape and len(x) % 3 == 0 and len(x) > 0 for x, g in zip(xs, gs)), \
        "coords and dcoords are lists of equally shaped [3 len, 3] arrays"
    F = len(feature_names)
    idx = feature_columns(feature_names)
    B, L = len(xs), max(len(x) for x in xs) // 3
    lens = np.array([len(x) // 3 for x in xs], dtype=np.int32)
    xyz, grad = np.zeros((B, 3 * L, 3), dtype=np.float64), np.zeros((B, 3 * L, 3), dtype=np.float64)
    for i, (x, g) in enumerate(zip(xs, gs)):
        xyz[i, : len(x)] = x
        grad[i, : len(g)] = g
    feats = None
    if angles is not None:
        rows = [np.asarray(a, dtype=np.float32) for a in angles]
        assert len(rows) == B and all(r.shape == (n, F) for r, n in zip(rows, lens)), "angles: one [len, F] array per chain"
        feats = np.zeros((B, L, F), dtype=np.float32)
        for i, r in enumerate(rows):
            feats[i, : len(r)] = r
    out = _vjp_padded(xyz, lens, grad, F, idx, centered, device, feats)
    return [out[i, : lens[i]].copy() for i in range(B)]


def build_backbones_torch(angles, lengths: Sequence[int], feature_names: Sequence[str], center_coords: bool = True, device: int = 0):
    """``build_backbones`` as a differentiable torch function: a float32 ``[B, L, F]`` tensor of angles and the chains'
    ``lengths`` -> a float64 ``[B, 3L, 3]`` tensor of coordinates (atoms at or beyond ``3 * lengths[b]``: 0).  The forward is
    ``fd_nerf``, the backward ``fd_nerf_vjp_feats`` on the float32 rows the forward was given, so any torch loss on the
    coordinates back-propagates to the angles, bond angles and lengths of either sign included; the gradient is
    ``coords_vjp``'s with ``angles``, cast to the dtype of ``angles``, and 0 on the rows at or beyond a length.  Both passes go
    through host arrays, whatever device ``angles`` lives on."""
    import torch

    idx = feature_columns(feature_names)
    F = len(feature_names)
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))

    class _Nerf(torch.autograd.Function):
        @staticmethod
        def forward(ctx, ang):
            feats = np.ascontiguousarray(ang.detach().cpu().numpy(), dtype=np.float32)
            assert feats.ndim == 3 and feats.shape[2] == F and feats.shape[0] == len(lens), "angles are [B, L, F], one length per chain"
            B, L, _ = feats.shape
            out = np.empty((B, 3 * L, 3), dtype=np.float64)
            ptr = _binding.ptr
            _binding.check(_binding.load().fd_nerf(device, ptr(feats), ptr(lens), B, L, F, ptr(idx), 1 if center_coords else 0, ptr(out)))
            ctx.coords, ctx.feats, ctx.dtype = out, feats.copy(), ang.dtype
            return torch.from_numpy(out.copy()).to(ang.device)

        @staticmethod
        def backward(ctx, grad):
            g = np.ascontiguousarray(grad.detach().cpu().numpy(), dtype=np.float64)
            return torch.from_numpy(_vjp_padded(ctx.coords, lens, g, F, idx, center_coords, device, ctx.feats)).to(device=grad.device, dtype=ctx.dtype)

    return _Nerf.apply(angles)


class NERFBuilder:
    """Single-chain builder with the reference's constructor arguments (bond angles / lengths as floats
    or per-residue arrays); ``cartesian_coords`` / ``centered_cartesian_coords`` run on the GPU."""

    def __init__(self, phi_dihedrals, psi_dihedrals, omega_dihedrals,
                 bond_len_n_ca=N_CA_LENGTH, bond_len_ca_c=CA_C_LENGTH, bond_len_c_n=C_N_LENGTH,
                 bond_angle_n_ca=121 / 180 * np.pi, bond_angle_ca_c=109 / 180 * np.pi, bond_angle_c_n=115 / 180 * np.pi,
                 init_coords=None, device: int = 0) -> None:
        if init_coords is not None:
            raise NotImplementedError("custom init_coords: the device builder starts from the reference's 1CRN seed")
        cols, names = [], []
        def add(name, v, default):
            if isinstance(v, (float, int)):
                if abs(float(v) - default) > 1e-12:
                    raise NotImplementedError(f"scalar override of {name} (only the reference default or an array)")
                return
            cols.append(np.asarray(v, dtype=np.float32).squeeze()); names.append(name)
        for n, v in (("phi", phi_dihedrals), ("psi", psi_dihedrals), ("omega", omega_dihedrals)):
            cols.append(np.asarray(v, dtype=np.float32).squeeze()); names.append(n)
        add("tau", bond_angle_ca_c, 109 / 180 * np.pi)
        add("CA:C:1N", bond_angle_c_n, 115 / 180 * np.pi)
        add("C:1N:1CA", bond_angle_n_ca, 121 / 180 * np.pi)
        add("0C:1N", bond_len_c_n, C_N_LENGTH)
        add("N:CA", bond_len_n_ca, N_CA_LENGTH)
        add("CA:C", bond_len_ca_c, CA_C_LENGTH)
        self._feats, self._names, self._device = np.stack(cols, axis=1), names, device

    @property
    def cartesian_coords(self) -> np.ndarray:
        return build_backbones([self._feats], self._names, center_coords=False, device=self._device)[0]

    @property
    def centered_cartesian_coords(self) -> np.ndarray:
        return build_backbones([self._feats], self._names, center_coords=True, device=self._device)[0]
