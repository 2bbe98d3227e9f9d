"""
Input side of the package: PDB backbones -> internal coordinates -> datasets, TM-score / superposed-RMSD scoring, and
secondary-structure annotation.

The inverse of ``angles_and_coords`` / ``nerf``.  Restates, without biotite:

* ``canonical_distances_and_dihedrals`` / ``extract_backbone_coords`` (foldingdiff/angles_and_coords.py:30-109,
  :271-284): the geometry of EVERY parsed file comes from one ``fd_internal_coords`` launch (one lane per residue,
  fp64), the PDB parsing stays on the host (``read_backbone``);
* ``CathCanonicalAnglesDataset`` and its angle-only subclasses (foldingdiff/datasets.py:75-566) over a list of files
  or a directory (``PdbAnglesDataset``), without the pickle cache;
* the scorers of ``sampling.get_reconstruction_error`` (the reference's ``_score_angles``, foldingdiff/sampling.py:266-284,
  which runs the external TM-align binary): ``tm_scorer`` scores with the TM-score of the CA traces (``fd_tm_score``,
  the published TM-score search restated on the device; see ``tm_score``), ``rmsd_scorer`` with the backbone RMSD
  after optimal superposition (``fd_superpose_rmsd``).  Each scores a whole call with one launch;
* ``count_structures_in_pdb`` / ``make_ss_cooccurrence_plot`` (bin/annot_secondary_structures.py:64-166), which take
  the labels from biotite's ``annotate_sse``: ``annotate_sse`` here restates that algorithm (P-SEA) on the device
  (``fd_annotate_sse``, every chain of a call in one launch), ``ss_cooccurrence`` is the plot function.

* ``tmalign.run_tmalign`` / ``max_tm_across_refs`` (foldingdiff/tmalign.py:22-83) and ``get_pairwise_tmscores``
  (bin/hclust_structures.py:38-69), which run one TM-align subprocess per pair of chains whose residues do not
  correspond: ``tm_align``, ``pairwise_tm``, ``max_tm_across_refs`` and ``pairwise_tmscores`` search the residue
  alignment and the superposition on the device (``fd_tm_align``, one workgroup per pair; ``starts=`` chooses among
  TM-align's five starts through ``fd_tm_align_ex``).

* ``count_clashes`` / ``count_clashes_parallel`` (foldingdiff/vdw_clashes.py:34-78), a Python double loop over atom pairs
  in one process per file, and ``lddt`` / ``lddt_sampled_folded`` (foldingdiff/lddt.py:32-100), one OpenStructure
  container per pair: ``count_clashes``, ``count_clashes_parallel``, ``lddt`` and ``lddt_scorer`` count the atom pairs on
  the device (``fd_backbone_clashes``, ``fd_lddt``: one workgroup per structure, integer results).

* ``add_oxygen_to_backbone`` (bin/add_oxygen_to_backbone.py:42-83), one biotite atom at a time: ``add_oxygens`` places the
  carbonyl oxygens of every backbone of a call in one launch (``fd_backbone_oxygens``), and ``dssp`` / ``dssp_counts`` /
  ``dssp_from_backbones`` / ``dssp_of_pdb`` label N / CA / C / O backbones with the DSSP states from their backbone hydrogen
  bonds (``fd_dssp``, one workgroup per chain).  The reference has no DSSP of its own (it shells out to mkdssp).

PDB parser rules (``read_backbone``; the reference relies on biotite 0.34's ``PDBFile`` for them):

1. a file with more than one MODEL record is rejected (``None``), as the reference does;
2. ATOM records are read, plus HETATM records of selenomethionine (MSE); other HETATM records are skipped;
3. of an atom with alternate locations, the first record in the file is kept;
4. a residue is identified by (chain, resSeq, iCode); residues are taken in the order they first appear;
5. each residue contributes its N, CA and C atoms, in that order;
6. all chains are concatenated in file order (the reference runs ``dihedral_backbone`` over the whole structure, so
   the geometry across a chain break is computed like any other);
7. a residue without one of N / CA / C rejects the file (``None``, with a debug log line).  This project's choice:
   it stands in for biotite's ``BadStructureError``, whose exact trigger is not pinned here.
"""
import ctypes as C
import glob
import gzip
import json
import logging
import os
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd
import torch

from . import _binding, datasets, nerf, utils
from ._binding import ptr

EXHAUSTIVE_ANGLES = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
EXHAUSTIVE_DISTS = ["0C:1N", "N:CA", "CA:C"]
MINIMAL_ANGLES = ["phi", "psi", "omega"]
MINIMAL_DISTS: List[str] = []

# fd_internal_coords' output columns
CANONICAL = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical"]
# accepted names -> output column (the reference also accepts "N:CA:C" for tau and "C:1N" for 0C:1N)
_ALIASES = {**{c: c for c in CANONICAL}, "N:CA:C": "tau", "C:1N": "0C:1N"}
_DIHEDRALS = ("phi", "psi", "omega")
_BACKBONE = ("N", "CA", "C")


# ---------------------------------------------------------------------------------------------------- parsing
def _open(fname: str):
    return gzip.open(fname, "rt") if str(fname).endswith(".gz") else open(fname, "rt")


def read_backbone(fname: str) -> Optional[Tuple[np.ndarray, List[Tuple[str, str, str]]]]:
    """N, CA, C coordinates of every residue of a ``.pdb`` / ``.pdb.gz`` file: (float32 [3n, 3], the n residue ids
    (chain, resSeq, iCode)), or ``None`` for a rejected file.  Rules 1-7 of the module docstring."""
    n_models = 0
    atoms = {}       # residue id -> {atom name: xyz}; the first record of an atom wins (alternate locations)
    order = []       # residue ids in order of first appearance
    with _open(fname) as fh:
        for line in fh:
            rec = line[:6]
            if rec == "MODEL ":
                n_models += 1
                continue
            if rec != "ATOM  " and not (rec == "HETATM" and line[17:20] == "MSE"):
                continue
            name = line[12:16].strip()
            if name not in _BACKBONE:
                continue
            rid = (line[21], line[22:26].strip(), line[26].strip())
            res = atoms.get(rid)
            if res is None:
                res = atoms[rid] = {}
                order.append(rid)
            if name not in res:
                res[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    if n_models > 1:
        logging.debug(f"{fname}: {n_models} models - skipping")
        return None
    if not order:
        logging.debug(f"{fname}: no backbone atoms - skipping")
        return None
    for rid in order:
        missing = [a for a in _BACKBONE if a not in atoms[rid]]
        if missing:
            logging.debug(f"{fname}: residue {rid} lacks {missing} - skipping")
            return None
    xyz = np.array([atoms[rid][a] for rid in order for a in _BACKBONE], dtype=np.float32)
    return xyz, order


def extract_backbone_coords(fname: str, atoms: Sequence[str] = ("CA",)) -> Optional[np.ndarray]:
    """float32 coordinates of the chosen backbone atoms of every residue, in file order (N, CA, C within a residue):
    ``extract_backbone_coords`` (foldingdiff/angles_and_coords.py:271-284), the ``"coords"`` the datasets carry.
    ``None`` for a file ``read_backbone`` rejects."""
    bb = read_backbone(fname)
    if bb is None:
        return None
    keep = [k for k, a in enumerate(_BACKBONE) if a in atoms]
    return bb[0].reshape(-1, 3, 3)[:, keep].reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- call plumbing
def _pack(arrays: Sequence[np.ndarray], dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """[n_i, 3] arrays laid back to back for one device call: (one contiguous [sum n_i, 3] array, int32 offsets, int32 lens)."""
    lens = np.array([len(x) for x in arrays], dtype=np.int32)
    offsets = (np.cumsum(lens) - lens).astype(np.int32)
    flat = np.concatenate(arrays) if len(arrays) else np.zeros((0, 3))
    return np.ascontiguousarray(flat, dtype=dtype), offsets, lens


def _ca_traces(chains: Sequence[np.ndarray], cap: int, what: str = "chain") -> List[np.ndarray]:
    """The chains as float64 arrays, each checked to be an [n, 3] trace of 1 <= n <= ``cap`` residues."""
    out = [np.asarray(x, dtype=np.float64) for x in chains]
    for i, x in enumerate(out):
        if x.ndim != 2 or x.shape[1] != 3 or not 1 <= len(x) <= cap:
            raise ValueError(f"{what} {i}: {x.shape}; expected an [n, 3] CA trace with 1 <= n <= {cap}")
    return out


def _norm_lens(norm_lens, floor: np.ndarray, what: str) -> np.ndarray:
    """``norm_lens`` as int32, checked to hold one length per pair and none below ``floor`` (``what`` names it)."""
    nl = np.asarray(norm_lens, dtype=np.int64).reshape(-1)
    if nl.shape != floor.shape or (nl < floor).any() or (nl > np.iinfo(np.int32).max).any():
        raise ValueError(f"norm_lens {nl.tolist()} must hold one length >= {what} per pair (floors {floor.tolist()})")
    return nl.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- featurising
def internal_coords(chains: Sequence[np.ndarray], device: int = 0) -> List[np.ndarray]:
    """The nine canonical features (float32 [n_i, 9], columns ``CANONICAL``) of every backbone in ``chains``
    (each [3 n_i, 3]: N, CA, C per residue), all in one ``fd_internal_coords`` launch."""
    if not chains:
        return []
    for c in chains:
        assert c.ndim == 2 and c.shape[1] == 3 and len(c) % 3 == 0 and len(c) > 0, f"expected [3n, 3], got {c.shape}"
    xyz, offsets, lens = _pack(chains, np.float32)
    offsets, lens = offsets // 3, lens // 3   # in residues
    out = np.empty((int(lens.sum()), 9), dtype=np.float32)
    _binding.check(_binding.load().fd_internal_coords(device, ptr(xyz), ptr(offsets), ptr(lens), len(chains), ptr(out)))
    return [out[o: o + n] for o, n in zip(offsets, lens)]


def _columns(distances: Sequence[str], angles: Sequence[str]) -> List[str]:
    for d in distances:
        if d not in _ALIASES or _ALIASES[d].count(":") != 1:
            raise ValueError(f"Unrecognized distance: {d}")
    for a in angles:
        if a not in _ALIASES or _ALIASES[a].count(":") == 1:
            raise ValueError(f"Unrecognized angle: {a}")
    return list(distances) + list(angles)


def _in_range(feats: np.ndarray, angles: Sequence[str], fname: str) -> bool:
    """The reference's range check (angles_and_coords.py:78-82): the three dihedrals and every requested angle, float32
    values against float64 pi; NaN padding is ignored."""
    for a in list(_DIHEDRALS) + [a for a in angles if _ALIASES[a] not in _DIHEDRALS]:
        v = feats[:, CANONICAL.index(_ALIASES[a])]
        v = v[~np.isnan(v)]
        if v.size and not (v.min() >= -np.pi and v.max() <= np.pi):
            logging.warning(f"Illegal values for {a} in {fname} -- skipping")
            return False
    return True


def featurize_backbones(fnames: Sequence[str], device: int = 0) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
    """(float32 [n, 9] canonical features, float32 [3n, 3] backbone) per file, ``None`` for a rejected one; the files
    are parsed on the host, the geometry of all of them is one device launch."""
    parsed = [read_backbone(f) for f in fnames]
    ok = [i for i, p in enumerate(parsed) if p is not None]
    feats = internal_coords([parsed[i][0] for i in ok], device=device)
    out: List[Optional[Tuple[np.ndarray, np.ndarray]]] = [None] * len(fnames)
    for i, f in zip(ok, feats):
        out[i] = (f, parsed[i][0])
    return out


def featurize(fnames: Sequence[str], distances: Sequence[str] = tuple(EXHAUSTIVE_DISTS),
              angles: Sequence[str] = tuple(EXHAUSTIVE_ANGLES), device: int = 0) -> List[Optional[pd.DataFrame]]:
    """``canonical_distances_and_dihedrals`` for many files with one ``fd_internal_coords`` call: per file a DataFrame
    with the columns ``distances + angles`` (float32), or ``None`` if the file is rejected (parser rules 1 and 7) or
    one of its angles leaves [-pi, pi]."""
    cols = _columns(distances, angles)
    out: List[Optional[pd.DataFrame]] = []
    for fname, r in zip(fnames, featurize_backbones(fnames, device=device)):
        if r is None or not _in_range(r[0], angles, fname):
            out.append(None)
            continue
        out.append(pd.DataFrame({c: r[0][:, CANONICAL.index(_ALIASES[c])] for c in cols}))
    return out


def canonical_distances_and_dihedrals(fname: str, distances: List[str] = MINIMAL_DISTS,
                                      angles: List[str] = MINIMAL_ANGLES) -> Optional[pd.DataFrame]:
    """The reference's single-file form (foldingdiff/angles_and_coords.py:30-109), same signature and defaults."""
    assert os.path.isfile(fname), fname
    return featurize([fname], distances=distances, angles=angles)[0]


# ---------------------------------------------------------------------------------------------------- datasets
def _pdb_fnames(pdbs: Union[str, Sequence[str]]) -> List[str]:
    """A list of files, or the ``*.pdb`` / ``*.pdb.gz`` files of a directory (sorted: the reference takes the
    filesystem's order, which the seeded shuffle then depends on)."""
    if isinstance(pdbs, (list, tuple)):
        for f in pdbs:
            assert os.path.isfile(f), f"Given file does not exist: {f}"
        return list(pdbs)
    assert os.path.isdir(pdbs), f"{pdbs} is neither a list of files nor a directory"
    fnames = []
    for ext in (".pdb", ".pdb.gz"):
        fnames.extend(sorted(glob.glob(os.path.join(pdbs, f"*{ext}"))))
    assert fnames, f"No PDB files found in {pdbs}"
    return fnames


def _featurize_for_dataset(fnames: Sequence[str]) -> List[Optional[Tuple[pd.DataFrame, np.ndarray]]]:
    """Default ``featurizer`` of ``PdbAnglesDataset``: (9-column DataFrame, CA coordinates) per file or ``None``
    (what the reference's ``__compute_featurization`` gets from its two pool maps)."""
    out = []
    for fname, r in zip(fnames, featurize_backbones(fnames)):
        if r is None or not _in_range(r[0], EXHAUSTIVE_ANGLES, fname):
            out.append(None)
            continue
        out.append((pd.DataFrame(r[0], columns=CANONICAL), r[1][1::3].copy()))
    return out


class PdbAnglesDataset:
    """``CathCanonicalAnglesDataset`` (foldingdiff/datasets.py:75-465) over PDB files: items of the nine canonical
    features, with the reference's filtering, seeded shuffle and split, zero-centring, padding and item keys.

    ``pdbs``: a list of files or a directory.  ``featurizer(fnames)`` returns per file ``(DataFrame with the columns
    CANONICAL, float32 [n, 3] CA coordinates)`` or ``None``; the default reads the files and featurises them on the
    device.  ``trim_strategy``: "leftalign" or "discard" ("randomcrop" is not supported)."""

    feature_names = {"angles": list(CANONICAL)}
    feature_is_angular = {"angles": list(datasets.FEATURE_SET_NAMES_TO_ANGULARITY["canonical"])}

    def __init__(self, pdbs: Union[str, Sequence[str]], split: Optional[str] = None, pad: int = 512, min_length: int = 40,
                 trim_strategy: str = "leftalign", zero_center: bool = True,
                 featurizer: Optional[Callable[[Sequence[str]], list]] = None) -> None:
        assert pad > min_length
        if trim_strategy not in ("leftalign", "discard"):
            raise NotImplementedError(f"trim_strategy={trim_strategy!r}")
        self.trim_strategy, self.pad, self.min_length = trim_strategy, pad, min_length
        self.feature_idx = [CANONICAL.index(f) for f in self.feature_names["angles"]]
        fnames = _pdb_fnames(pdbs)
        feats = (featurizer or _featurize_for_dataset)(fnames)
        assert len(feats) == len(fnames)
        self.structures = [{"angles": r[0], "coords": r[1], "fname": f} for f, r in zip(fnames, feats) if r is not None]
        for s in self.structures:
            assert list(s["angles"].columns) == CANONICAL and len(s["coords"]) == len(s["angles"]), s["fname"]
        if self.min_length:
            self.structures = [s for s in self.structures if s["angles"].shape[0] >= self.min_length]
        if self.trim_strategy == "discard":
            self.structures = [s for s in self.structures if s["angles"].shape[0] <= self.pad]
        # shuffled even without a split, so that contiguous splits act like random ones (datasets.py:190-208)
        self.rng = np.random.default_rng(seed=6489)
        self.rng.shuffle(self.structures)
        if split is not None:
            n = len(self.structures)
            cut = int(n * 0.8)
            if split == "train":
                self.structures = self.structures[:cut]
            elif split == "validation":
                self.structures = self.structures[cut: cut + int(n * 0.1)]
            elif split == "test":
                self.structures = self.structures[cut + int(n * 0.1):]
            else:
                raise ValueError(f"Unknown split: {split}")
        # circular mean of ALL nine columns, the distances included (the reference's quirk); NaN padding ignored
        self.means = None
        if zero_center:
            concat = np.concatenate([s["angles"] for s in self.structures])
            self.means = np.arctan2(np.nanmean(np.sin(concat), axis=0), np.nanmean(np.cos(concat), axis=0))
        self.all_lengths = [s["angles"].shape[0] for s in self.structures]
        self._length_rng = np.random.default_rng(seed=6489)

    @property
    def filenames(self) -> List[str]:
        return [s["fname"] for s in self.structures]

    def __len__(self) -> int:
        return len(self.structures)

    def sample_length(self, n: int = 1) -> Union[int, List[int]]:
        assert n > 0
        if n == 1:
            return self._length_rng.choice(self.all_lengths)
        return self._length_rng.choice(self.all_lengths, size=n, replace=True).tolist()

    def get_masked_means(self) -> Optional[np.ndarray]:
        """The means of the features this dataset returns (``None`` without zero-centring)."""
        return None if self.means is None else np.copy(self.means)[self.feature_idx]

    def set_masked_means(self, mean_values: np.ndarray) -> None:
        """Overwrite the means of the features this dataset returns, e.g. with a model's training_mean_offset.npy."""
        if self.means is None:
            raise NotImplementedError
        self.means[self.feature_idx] = np.asarray(mean_values).copy()

    def __getitem__(self, index: int, ignore_zero_center: bool = False):
        if not 0 <= index < len(self):
            raise IndexError("Index out of range")
        s = self.structures[index]
        angles = np.asarray(s["angles"].values)
        coords = np.asarray(s["coords"])
        if self.means is not None and not ignore_zero_center:
            angles = angles - self.means
            # "angular" = every column whose name does not hold exactly one ':' (datasets.py:405-411)
            ang = [j for j, c in enumerate(CANONICAL) if c.count(":") != 1]
            angles[:, ang] = utils.modulo_with_wrapped_range(angles[:, ang], -np.pi, np.pi)
        angles = np.nan_to_num(angles[:, self.feature_idx], nan=0.0)
        l = min(self.pad, angles.shape[0])
        attn_mask = torch.zeros(size=(self.pad,))
        attn_mask[:l] = 1.0
        if angles.shape[0] < self.pad:
            angles = np.pad(angles, ((0, self.pad - angles.shape[0]), (0, 0)), mode="constant", constant_values=0)
            coords = np.pad(coords, ((0, self.pad - coords.shape[0]), (0, 0)), mode="constant", constant_values=0)
        else:   # left-align ("discard" has removed the longer ones)
            angles, coords = angles[: self.pad], coords[: self.pad]
        return {
            "angles": torch.from_numpy(np.ascontiguousarray(angles)).float(),
            "coords": torch.from_numpy(np.ascontiguousarray(coords)).float(),
            "attn_mask": attn_mask,
            "position_ids": torch.arange(start=0, end=self.pad, step=1, dtype=torch.long),
            "lengths": torch.tensor(l, dtype=torch.int64),
        }


class PdbAnglesOnlyDataset(PdbAnglesDataset):
    """``CathCanonicalAnglesOnlyDataset`` (datasets.py:487-548): the three dihedrals and the three bond angles."""
    feature_names = {"angles": list(datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-full-angles"])}
    feature_is_angular = {"angles": list(datasets.FEATURE_SET_NAMES_TO_ANGULARITY["canonical-full-angles"])}


class PdbMinimalAnglesDataset(PdbAnglesDataset):
    """``CathCanonicalMinimalAnglesDataset`` (datasets.py:551-561): phi, psi, omega, tau."""
    feature_names = {"angles": list(datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-minimal-angles"])}
    feature_is_angular = {"angles": list(datasets.FEATURE_SET_NAMES_TO_ANGULARITY["canonical-minimal-angles"])}


# training_args["angles_definitions"] -> dataset class ("cart-coords" is not supported)
DATASETS = {"canonical": PdbAnglesDataset, "canonical-full-angles": PdbAnglesOnlyDataset,
            "canonical-minimal-angles": PdbMinimalAnglesDataset}


# ---------------------------------------------------------------------------------------------------- scoring
def superposed_rmsd(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], device: int = 0) -> np.ndarray:
    """RMSD of a[i] to b[i] after optimal rotation and translation, for every pair (each [m_i, 3], m_i >= 1), in one
    ``fd_superpose_rmsd`` call; float64 [len(a_list)]."""
    assert len(a_list) == len(b_list)
    if not a_list:
        return np.zeros((0,), dtype=np.float64)
    a = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in a_list]
    b = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in b_list]
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and len(x) > 0, f"pair {i}: {x.shape} vs {y.shape}"
    (A, offsets, lens), B = _pack(a), _pack(b)[0]
    out = np.empty((len(a),), dtype=np.float64)
    _binding.check(_binding.load().fd_superpose_rmsd(device, ptr(A), ptr(B), ptr(offsets), ptr(lens), len(a), ptr(out)))
    return out


def motif_backbone(motif: np.ndarray, feature_names: Sequence[str], at_chain_start: bool = False, device: int = 0) -> np.ndarray:
    """The motif's own NeRF-built backbone, float64 ``[3 m, 3]`` (N, CA, C per residue), from its ``[m, F]`` angle rows
    alone.  NeRF's first residue is a constant seed (with the seed's bond lengths), and the N-CA-C angle of residue i + 1
    is read from row i; so the rows are built behind one lead-in row -- a copy of the first row, of which only ``tau``
    shapes the motif -- and the seed residue is dropped.  This is the geometry ``sampling.scaffold`` (``pin_lead_angle``)
    reproduces at any offset >= 1.  ``at_chain_start``: the motif as the start of a chain (offset 0), where its first
    residue is the seed residue itself: the rows built as they are."""
    motif = np.asarray(motif, dtype=np.float32)
    if at_chain_start:
        return nerf.build_backbones([motif], feature_names, center_coords=False, device=device)[0]
    xyz = nerf.build_backbones([np.concatenate([motif[:1], motif])], feature_names, center_coords=False, device=device)[0]
    return xyz[3:].copy()


def motif_rmsd(backbones: Sequence[np.ndarray], motif_backbone: np.ndarray, offsets: Sequence[int], device: int = 0) -> np.ndarray:
    """N / CA / C RMSD (Angstrom, after optimal superposition) of residues ``offsets[i] .. offsets[i] + m - 1`` of every
    generated backbone (``[3 len_i, 3]``, ``nerf.build_backbones``) against the motif's backbone (``[3 m, 3]``,
    ``motif_backbone``); float64 ``[len(backbones)]``."""
    ref = np.asarray(motif_backbone, dtype=np.float64).reshape(-1, 3)
    assert len(backbones) == len(offsets) and len(ref) % 3 == 0
    m3 = len(ref)
    parts = []
    for i, (bb, o) in enumerate(zip(backbones, offsets)):
        bb = np.asarray(bb, dtype=np.float64).reshape(-1, 3)
        assert 0 <= 3 * int(o) and 3 * int(o) + m3 <= len(bb), f"backbone {i}: {len(bb) // 3} residues, motif at {o} .. {int(o) + m3 // 3 - 1}"
        parts.append(bb[3 * int(o): 3 * int(o) + m3])
    return superposed_rmsd(parts, [ref] * len(parts), device=device)


def repeat_rmsd(backbones: Sequence[np.ndarray], start, period, units, device: int = 0) -> np.ndarray:
    """How exactly the repeat units of a backbone superpose (``sampling.sample_repeats``): for every backbone
    (``[3 len_i, 3]``, N / CA / C per residue, ``nerf.build_backbones``) the RMSD in Angstrom, after optimal superposition,
    of the atoms of the tied residues ``[start + 1, start + (units - 1) * period)`` onto the same range shifted by
    ``period`` -- all units but the last onto all units but the first; float64 ``[len(backbones)]`` from one
    ``superposed_rmsd`` call.  The first tied residue is left out: NeRF reads the N-CA-C angle of residue ``i`` from row
    ``i - 1``, which for residue ``start`` is a free row (for residue 0: the fixed seed), while its images in the later units
    read a tied row.  Every other residue of the range is built from tied rows alone.  ``start``, ``period`` and ``units``
    are scalars or one value per backbone.  NaN where ``units == 1`` (nothing is tied) or the range is empty."""
    n = len(backbones)
    per = [np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)) for v in (start, period, units)]
    out = np.full((n,), np.nan, dtype=np.float64)
    a_parts, b_parts, where = [], [], []
    for i, (bb, s, p, r) in enumerate(zip(backbones, *per)):
        bb = np.asarray(bb, dtype=np.float64).reshape(-1, 3)
        if s < 0 or p < 1 or r < 1 or 3 * (s + p * r) > len(bb):
            raise ValueError(f"backbone {i}: {len(bb) // 3} residues, tie (start={s}, period={p}, units={r})")
        lo, hi = int(s) + 1, int(s + (r - 1) * p)
        if r > 1 and hi > lo:
            a_parts.append(bb[3 * lo: 3 * hi])
            b_parts.append(bb[3 * (lo + int(p)): 3 * (hi + int(p))])
            where.append(i)
    if where:
        out[where] = superposed_rmsd(a_parts, b_parts, device=device)
    return out


# ---------------------------------------------------------------------------------------------------- distance restraints
BACKBONE_ATOMS = {"N": 0, "CA": 1, "C": 2}


class Restraints:
    """One chain's distance restraints between backbone atoms (``fd_restraint_energy``): arrays ``i``, ``j``
    (int32 atom indices ``3 * residue + {0 N, 1 CA, 2 C}``, ``i != j``) and ``d0``, ``tol``, ``w`` (float64, finite, ``>= 0``).
    A restraint costs ``w * max(0, |d - d0| - tol)^2`` with ``d`` the distance of its two atoms: ``tol = 0`` is harmonic,
    ``d0 = 0, tol = 8`` is "within 8 Angstrom".  ``a + b`` joins two sets.

    Distances alone do not fix handedness: a structure and its mirror image cost the same.  Restraints among L-amino-acid
    backbone segments mostly do tell the two apart, because each segment's own internal angles enter the sampler's state and
    are not mirrored; that is a tendency, not a guarantee.  ``Template`` is the term that does fix it."""

    def __init__(self, i, j, d0, tol, w):
        self.i = np.ascontiguousarray(np.asarray(i, dtype=np.int64).reshape(-1).astype(np.int32))
        self.j = np.ascontiguousarray(np.asarray(j, dtype=np.int64).reshape(-1).astype(np.int32))
        n = len(self.i)
        self.d0, self.tol, self.w = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (d0, tol, w))
        if len(self.j) != n:
            raise ValueError(f"{n} first atoms, {len(self.j)} second atoms")
        if n and ((self.i < 0).any() or (self.j < 0).any() or (self.i == self.j).any()):
            raise ValueError("a restraint names two different atoms, each >= 0")
        for name, v in (("d0", self.d0), ("tol", self.tol), ("w", self.w)):
            if not (np.isfinite(v).all() and (v >= 0).all()):
                raise ValueError(f"{name} must be finite and >= 0")

    def __len__(self) -> int:
        return len(self.i)

    def __add__(self, other: "Restraints") -> "Restraints":
        return Restraints(*(np.concatenate([getattr(self, k), getattr(other, k)]) for k in ("i", "j", "d0", "tol", "w")))

    def min_length(self) -> int:
        """The residues a chain needs for every atom named here to exist."""
        return 0 if not len(self) else int(max(self.i.max(), self.j.max())) // 3 + 1


def contact_restraints(pairs, max_dist: float = 8.0, weight: float = 1.0, atom: str = "CA") -> Restraints:
    """"These residues are in contact": for every entry ``(i, j)`` or ``(i, j, max_dist)`` of ``pairs`` (residue indices from
    0) a restraint that costs nothing while the two residues' ``atom`` (``"N"``, ``"CA"`` or ``"C"``) lie within ``max_dist``
    Angstrom and ``weight * (d - max_dist)^2`` beyond."""
    if atom not in BACKBONE_ATOMS:
        raise ValueError(f"atom={atom!r}: expected one of {sorted(BACKBONE_ATOMS)}")
    rows = [tuple(p) for p in pairs]
    if any(len(p) not in (2, 3) for p in rows):
        raise ValueError("every pair is (i, j) or (i, j, max_dist)")
    if any(int(p[0]) < 0 or int(p[1]) < 0 or int(p[0]) == int(p[1]) for p in rows):
        raise ValueError("a contact names two different residues, each >= 0")
    a = BACKBONE_ATOMS[atom]
    return Restraints([3 * int(p[0]) + a for p in rows], [3 * int(p[1]) + a for p in rows], np.zeros(len(rows)),
                      np.array([float(p[2]) if len(p) == 3 else float(max_dist) for p in rows], dtype=np.float64), float(weight))


def motif_restraints(motif_backbone: np.ndarray, placed_at: Sequence[int], weight: float = 1.0, tol: float = 0.0,
                     atoms: Sequence[str] = ("CA",)) -> Restraints:
    """"These residues sit relative to each other as in the motif": every pair among the chosen ``atoms`` of the motif's
    residues, at the distance it has in ``motif_backbone`` (``[3 m, 3]``, N / CA / C per residue, e.g. the residues picked
    from ``read_backbone``).  ``placed_at[r]`` is the residue index motif residue ``r`` takes in the new chain; the residues
    need not be contiguous, so two separate segments are placed relative to each other.  ``m (m - 1) / 2`` restraints per
    atom pair type; see ``Restraints`` on the mirror image."""
    xyz = np.asarray(motif_backbone, dtype=np.float64).reshape(-1, 3)
    placed = [int(p) for p in placed_at]
    if len(xyz) % 3 or len(xyz) != 3 * len(placed):
        raise ValueError(f"motif_backbone has {len(xyz)} atoms for {len(placed)} placed residues (3 per residue)")
    if len(set(placed)) != len(placed) or (placed and min(placed) < 0):
        raise ValueError("placed_at names distinct residues, each >= 0")
    unknown = [a for a in atoms if a not in BACKBONE_ATOMS]
    if unknown or not len(atoms) or len(set(atoms)) != len(atoms):
        raise ValueError(f"atoms={tuple(atoms)!r}: distinct entries of {sorted(BACKBONE_ATOMS)}")
    if not np.isfinite(xyz).all():
        raise ValueError("motif_backbone is not finite")
    sites = [(r, BACKBONE_ATOMS[a]) for r in range(len(placed)) for a in atoms]
    i, j, d0 = [], [], []
    for p, (ra, aa) in enumerate(sites):
        for rb, ab in sites[p + 1:]:
            i.append(3 * placed[ra] + aa)
            j.append(3 * placed[rb] + ab)
            d0.append(float(np.linalg.norm(xyz[3 * ra + aa] - xyz[3 * rb + ab])))
    return Restraints(i, j, d0, float(tol), float(weight))


def segment_restraints(motif_backbone: np.ndarray, segments: Sequence[Tuple[int, int, int]], weight: float = 1.0, tol: float = 0.0,
                       atoms: Sequence[str] = ("CA",)) -> Restraints:
    """"These segments sit relative to each other as in the motif" (``sampling.scaffold_segments``): a
    discontiguous motif is a list of ``segments`` ``(motif_start, motif_stop, placed_at)`` -- residues ``motif_start ..
    motif_stop - 1`` of ``motif_backbone`` (``[3 m, 3]``, N / CA / C per residue) take the residues ``placed_at ..`` of the new
    chain.  Returns ``motif_restraints``' restraints, in its order and with its distances bit for bit, for the atom pairs whose
    two residues lie in DIFFERENT segments only: a segment's own geometry is held exactly by replacement, and pairs inside it
    would only add stiffness.  ``ValueError`` for a segment that is empty or outside the motif, segments that share a motif
    residue or a placed residue, and everything ``motif_restraints`` rejects; see ``Restraints`` on the mirror image."""
    xyz = np.asarray(motif_backbone, dtype=np.float64).reshape(-1, 3)
    if len(xyz) % 3:
        raise ValueError(f"motif_backbone has {len(xyz)} atoms (3 per residue)")
    m = len(xyz) // 3
    rows, placed, owner = [], [], []
    for k, seg in enumerate(segments):
        if len(seg) != 3:
            raise ValueError("every segment is (motif_start, motif_stop, placed_at)")
        lo, hi, at = (int(v) for v in seg)
        if not 0 <= lo < hi <= m:
            raise ValueError(f"segment {k} = motif residues [{lo}, {hi}) is empty or outside the motif's {m} residues")
        if at < 0:
            raise ValueError(f"segment {k} is placed at residue {at}")
        rows.extend(range(lo, hi))
        placed.extend(range(at, at + hi - lo))
        owner.extend([k] * (hi - lo))
    if len(set(rows)) != len(rows):
        raise ValueError("two segments share a motif residue")
    sub = xyz.reshape(m, 3, 3)[rows].reshape(-1, 3) if rows else xyz[:0]
    every = motif_restraints(sub, placed, weight=weight, tol=tol, atoms=atoms)   # (its checks: distinct placed residues, the atoms)
    seg_of = {p: k for p, k in zip(placed, owner)}
    keep = np.array([seg_of[int(i) // 3] != seg_of[int(j) // 3] for i, j in zip(every.i, every.j)], dtype=bool)
    return Restraints(every.i[keep], every.j[keep], every.d0[keep], every.tol[keep], every.w[keep])


def pack_restraints(restraints, lengths: Sequence[int]):
    """``fd_restraint_energy``'s packed layout for a batch: ``(rst_offsets int32 [B + 1], rst_i, rst_j int32 [R], rst_d0,
    rst_tol, rst_w float64 [R])`` from one ``Restraints`` per chain (``None``: none), or a single one for every chain.
    ``ValueError`` for a restraint on an atom beyond its chain."""
    lengths = [int(l) for l in lengths]
    per = [restraints] * len(lengths) if restraints is None or isinstance(restraints, Restraints) else list(restraints)
    if len(per) != len(lengths):
        raise ValueError(f"{len(per)} restraint sets for {len(lengths)} chains")
    per = [Restraints([], [], [], [], []) if r is None else r for r in per]
    for b, (r, n) in enumerate(zip(per, lengths)):
        if r.min_length() > n:
            raise ValueError(f"chain {b} has {n} residues, its restraints need {r.min_length()}")
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int32)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([getattr(r, k) for r in per]).astype(dt))   # noqa: E731
    return (np.ascontiguousarray(offsets), cat("i", np.int32), cat("j", np.int32), cat("d0", np.float64), cat("tol", np.float64),
            cat("w", np.float64))


def restraint_energy(coords: Sequence[np.ndarray], restraints, device: int = 0, return_gradient: bool = False):
    """Energy and largest violation of distance restraints on a batch of backbones, in one ``fd_restraint_energy`` call.
    ``coords``: one ``[3 len_i, 3]`` array per chain (``nerf.build_backbones``); ``restraints``: as for ``pack_restraints``.
    Returns ``(energy, max_violation)``, float64 ``[B]`` each -- and with ``return_gradient`` a third entry, the list of the
    energy's gradients with respect to the coordinates (``[3 len_i, 3]``), which ``nerf.coords_vjp`` carries on to the
    angles.  Each atom's gradient is summed in the order of the list, so the bits do not depend on scheduling."""
    xs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in coords]
    assert xs and all(len(x) % 3 == 0 and len(x) > 0 for x in xs), "coords is a list of [3 len, 3] arrays"
    lens = np.array([len(x) // 3 for x in xs], dtype=np.int32)
    packed = pack_restraints(restraints, lens.tolist())
    B, L = len(xs), int(lens.max())
    xyz = np.zeros((B, 3 * L, 3), dtype=np.float64)
    for b, x in enumerate(xs):
        xyz[b, : len(x)] = x
    energy, worst = np.empty(B, dtype=np.float64), np.empty(B, dtype=np.float64)
    grad = np.empty((B, 3 * L, 3), dtype=np.float64) if return_gradient else None
    _binding.check(_binding.load().fd_restraint_energy(device, ptr(xyz), ptr(lens), B, L, *(ptr(a) for a in packed), ptr(energy), ptr(worst),
                                                       ptr(grad)))
    if not return_gradient:
        return energy, worst
    return energy, worst, [grad[b, : 3 * lens[b]].copy() for b in range(B)]


# ---------------------------------------------------------------------------------------------------- superposition restraints
class Template:
    """One chain's superposition restraint (``fd_template_energy``): ``atoms`` (int32 atom indices ``3 * residue
    + {0 N, 1 CA, 2 C}``, strictly increasing), ``xyz`` (float64 ``[n, 3]``, the position each should take in the template's
    own frame) and ``w`` (float64, finite, ``> 0``).  The chain costs ``sum w |r|^2`` with ``r`` the residuals after the optimal
    superposition of the template on the named atoms by a PROPER rotation and a translation: unlike distances
    (``Restraints``), this tells a structure from its mirror image.  Entries are kept sorted by atom."""

    def __init__(self, atoms, xyz, w=1.0):
        atoms = np.asarray(atoms, dtype=np.int64).reshape(-1)
        xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
        n = len(atoms)
        if len(xyz) != n:
            raise ValueError(f"{n} atoms, {len(xyz)} target positions")
        w = np.broadcast_to(np.asarray(w, dtype=np.float64), (n,))
        order = np.argsort(atoms, kind="stable")
        self.atoms = np.ascontiguousarray(atoms[order].astype(np.int32))
        self.xyz = np.ascontiguousarray(xyz[order])
        self.w = np.ascontiguousarray(w[order])
        if n and (self.atoms[0] < 0 or (np.diff(self.atoms) <= 0).any()):
            raise ValueError("a template names distinct atoms, each >= 0")
        if not np.isfinite(self.xyz).all():
            raise ValueError("xyz must be finite")
        if not (np.isfinite(self.w).all() and (self.w > 0).all()):
            raise ValueError("w must be finite and > 0")

    def __len__(self) -> int:
        return len(self.atoms)

    def min_length(self) -> int:
        """The residues a chain needs for every atom named here to exist."""
        return 0 if not len(self) else int(self.atoms[-1]) // 3 + 1

    def mirrored(self) -> "Template":
        """The same template reflected in z: what the mirror image of a fitting structure fits."""
        return Template(self.atoms, self.xyz * np.array([1.0, 1.0, -1.0]), self.w)


def motif_template(motif_backbone: np.ndarray, segments: Sequence[Tuple[int, int, int]], atoms: Sequence[str] = ("N", "CA", "C"),
                   weight: float = 1.0) -> Template:
    """"These segments sit in space as in the motif, in the motif's hand": ``segment_restraints``' ``segments``
    ``(motif_start, motif_stop, placed_at)`` -- residues ``motif_start .. motif_stop - 1`` of ``motif_backbone`` (``[3 m, 3]``,
    N / CA / C per residue) take the residues ``placed_at ..`` of the new chain -- as one ``Template`` over the chosen ``atoms``
    of every segment residue, with the motif's own coordinates as targets.  ``ValueError`` for what ``segment_restraints``
    rejects."""
    xyz = np.asarray(motif_backbone, dtype=np.float64).reshape(-1, 3)
    if len(xyz) % 3:
        raise ValueError(f"motif_backbone has {len(xyz)} atoms (3 per residue)")
    m = len(xyz) // 3
    unknown = [a for a in atoms if a not in BACKBONE_ATOMS]
    if unknown or not len(atoms) or len(set(atoms)) != len(atoms):
        raise ValueError(f"atoms={tuple(atoms)!r}: distinct entries of {sorted(BACKBONE_ATOMS)}")
    if not np.isfinite(xyz).all():
        raise ValueError("motif_backbone is not finite")
    rows, placed = [], []
    for k, seg in enumerate(segments):
        if len(seg) != 3:
            raise ValueError("every segment is (motif_start, motif_stop, placed_at)")
        lo, hi, at = (int(v) for v in seg)
        if not 0 <= lo < hi <= m:
            raise ValueError(f"segment {k} = motif residues [{lo}, {hi}) is empty or outside the motif's {m} residues")
        if at < 0:
            raise ValueError(f"segment {k} is placed at residue {at}")
        rows.extend(range(lo, hi))
        placed.extend(range(at, at + hi - lo))
    if len(set(rows)) != len(rows):
        raise ValueError("two segments share a motif residue")
    if len(set(placed)) != len(placed):
        raise ValueError("two segments share a placed residue")
    which = sorted(BACKBONE_ATOMS[a] for a in atoms)
    return Template([3 * p + a for p in placed for a in which], [xyz[3 * r + a] for r in rows for a in which] or np.zeros((0, 3)),
                    float(weight))


def pack_templates(templates, lengths: Sequence[int]):
    """``fd_template_energy``'s packed layout for a batch: ``(tpl_offsets int32 [B + 1], tpl_atom int32 [n], tpl_xyz float64
    [n, 3], tpl_w float64 [n])`` from one ``Template`` per chain (``None``: none), or a single one for every chain.
    ``ValueError`` for a template on an atom beyond its chain."""
    lengths = [int(l) for l in lengths]
    per = [templates] * len(lengths) if templates is None or isinstance(templates, Template) else list(templates)
    if len(per) != len(lengths):
        raise ValueError(f"{len(per)} templates for {len(lengths)} chains")
    per = [Template([], np.zeros((0, 3))) if t is None else t for t in per]
    for b, (t, n) in enumerate(zip(per, lengths)):
        if t.min_length() > n:
            raise ValueError(f"chain {b} has {n} residues, its template needs {t.min_length()}")
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in per])]).astype(np.int32)
    return (np.ascontiguousarray(offsets), np.ascontiguousarray(np.concatenate([t.atoms for t in per]).astype(np.int32)),
            np.ascontiguousarray(np.concatenate([t.xyz for t in per]).astype(np.float64).reshape(-1, 3)),
            np.ascontiguousarray(np.concatenate([t.w for t in per]).astype(np.float64)))


def template_energy(coords: Sequence[np.ndarray], templates, device: int = 0, return_gradient: bool = False,
                    return_transform: bool = False, mirror: bool = False):
    """Energy and RMSD of superposition restraints on a batch of backbones, in one ``fd_template_energy`` call.  ``coords``:
    one ``[3 len_i, 3]`` array per chain; ``templates``: as for ``pack_templates``.  Returns ``(energy, rmsd)``, float64 ``[B]``
    each (``rmsd``: the weighted RMSD of the named atoms after the optimal proper fit, 0 without entries); with
    ``return_gradient`` the list of the energy's gradients with respect to the coordinates (``[3 len_i, 3]``, zero on atoms
    not named) follows, and with ``return_transform`` the fits ``(R [B, 3, 3], t [B, 3])`` with ``R m + t`` the template laid
    on the chain.  ``mirror=True`` fits the template reflected in z instead: comparing ``rmsd`` with the ``rmsd`` of
    ``mirror=True`` says which hand a placement has, which no distance can."""
    xs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in coords]
    assert xs and all(len(x) % 3 == 0 and len(x) > 0 for x in xs), "coords is a list of [3 len, 3] arrays"
    lens = np.array([len(x) // 3 for x in xs], dtype=np.int32)
    if mirror:
        one = templates is None or isinstance(templates, Template)
        flip = lambda t: None if t is None else t.mirrored()   # noqa: E731
        templates = flip(templates) if one else [flip(t) for t in templates]
    packed = pack_templates(templates, lens.tolist())
    B, L = len(xs), int(lens.max())
    xyz = np.zeros((B, 3 * L, 3), dtype=np.float64)
    for b, x in enumerate(xs):
        xyz[b, : len(x)] = x
    energy, rmsd = np.empty(B, dtype=np.float64), np.empty(B, dtype=np.float64)
    grad = np.empty((B, 3 * L, 3), dtype=np.float64) if return_gradient else None
    fit = np.empty((B, 12), dtype=np.float64) if return_transform else None
    _binding.check(_binding.load().fd_template_energy(device, ptr(xyz), ptr(lens), B, L, *(ptr(a) for a in packed), ptr(energy), ptr(rmsd),
                                                      ptr(fit), ptr(grad)))
    result = [energy, rmsd]
    if return_gradient:
        result.append([grad[b, : 3 * lens[b]].copy() for b in range(B)])
    if return_transform:
        result.append((fit[:, :9].reshape(B, 3, 3).copy(), fit[:, 9:].copy()))
    return tuple(result)


# ---------------------------------------------------------------------------------------------------- relaxation in torsion space
class RelaxResult(NamedTuple):
    """What ``relax`` returns: per chain the relaxed angles (float32 ``[len_i, F]``), and arrays over the chains: the energy
    terms clash | restraint | tether before and after (float64 ``[B, 3]``), the accepted steps, the clashing atoms before and
    after (``count_clashes`` on ``build_backbones(method="scan")``), the largest change of a moved angle in radians, the step
    sizes to continue from, and with ``return_trace`` the total energy after every iteration (``[n_iter + 1, B]``)."""
    angles: List[np.ndarray]
    energy_before: np.ndarray
    energy_after: np.ndarray
    accepted: np.ndarray
    clashes_before: np.ndarray
    clashes_after: np.ndarray
    max_change: np.ndarray
    step: np.ndarray
    trace: Optional[np.ndarray]


def _relax_inputs(angles, lengths, feature_names, restraints, fixed, anchor, move, alpha, margin, clash_weight, tether, step0, grow,
                  shrink, max_step):
    """The padded arrays and the ``fd_relax_params`` both relax entries take; argument errors the library would also refuse
    are left to it (its message names the argument)."""
    F = len(feature_names)
    if isinstance(angles, np.ndarray) and angles.ndim == 3:
        if lengths is None:
            raise ValueError("a padded [B, L, F] array needs lengths")
        chains = [np.asarray(a[: int(n)], dtype=np.float32) for a, n in zip(angles, lengths)]
    else:
        chains = [np.asarray(a, dtype=np.float32) for a in angles]
        if lengths is not None:
            chains = [c[: int(n)] for c, n in zip(chains, lengths)]
    if not chains or any(c.ndim != 2 or c.shape[1] != F or len(c) == 0 for c in chains):
        raise ValueError(f"each chain must be [len >= 1, {F}]")
    idx = nerf.feature_columns(feature_names)
    unknown = [m for m in move if m not in feature_names]
    if unknown:
        raise ValueError(f"move={tuple(move)!r}: {unknown} are not among the features {list(feature_names)}")
    B, L = len(chains), max(len(c) for c in chains)
    lens = np.array([len(c) for c in chains], dtype=np.int32)
    feats = np.zeros((B, L, F), dtype=np.float32)
    for b, c in enumerate(chains):
        feats[b, : len(c)] = c
    anc = None
    if anchor is not None:
        anc = np.zeros((B, L, F), dtype=np.float32)
        rows = list(anchor) if not (isinstance(anchor, np.ndarray) and anchor.ndim == 3) else [a[: n] for a, n in zip(anchor, lens)]
        if len(rows) != B or any(np.shape(a) != c.shape for a, c in zip(rows, chains)):
            raise ValueError("anchor: one array per chain, shaped like its angles")
        for b, a in enumerate(rows):
            anc[b, : lens[b]] = a
    fix = None
    if fixed is not None:
        if len(fixed) != B:
            raise ValueError(f"fixed: {len(fixed)} entries for {B} chains")
        fix = np.zeros((B, L), dtype=np.uint8)
        for b, f in enumerate(fixed):
            if f is None:
                continue
            f = np.asarray(f)
            if f.dtype == bool:
                if len(f) != lens[b]:
                    raise ValueError(f"fixed[{b}]: a boolean array has one entry per residue ({lens[b]})")
                fix[b, : lens[b]] = f
            elif f.size:
                if f.min() < 0 or f.max() >= lens[b]:
                    raise ValueError(f"fixed[{b}]: residues outside [0, {lens[b]})")
                fix[b, f.astype(np.int64)] = 1
    prm = _binding.FdRelaxParams()
    for k in range(9):
        prm.feat_idx[k] = int(idx[k])
    for f, name in enumerate(feature_names[:16]):
        prm.is_angle[f] = 0 if ":" in name and name.count(":") == 1 else 1   # one ':' names a bond length, as in the PDB writers
        prm.move[f] = 1 if name in move else 0
    prm.clash_alpha, prm.clash_margin, prm.w_clash, prm.w_tether = float(alpha), float(margin), float(clash_weight), float(tether)
    prm.step0, prm.grow, prm.shrink, prm.max_step = float(step0), float(grow), float(shrink), float(max_step)
    return chains, feats, anc, lens, fix, prm, pack_restraints(restraints, lens.tolist())


def relax_energy(angles, lengths, feature_names: Sequence[str], restraints=None, fixed=None, anchor=None,
                 move: Sequence[str] = ("phi", "psi", "omega"), alpha: float = 0.63, margin: float = 0.15, clash_weight: float = 1.0,
                 tether: float = 0.0, device: int = 0):
    """The energy ``relax`` descends and its gradient with respect to the angles, in one ``fd_relax_energy`` call: float64
    ``[B, 3]`` (clash | restraint | tether), the gradient norms ``[B]`` and one float64 ``[len_i, F]`` gradient per chain, zero
    where a column is not in ``move`` or a row is ``fixed``.  Arguments as for ``relax``; ``anchor``: the angles the tether
    pulls towards (default: the input, so the tether costs nothing)."""
    chains, feats, anc, lens, fix, prm, packed = _relax_inputs(angles, lengths, feature_names, restraints, fixed, anchor, move, alpha, margin,
                                                               clash_weight, tether, 0.01, 1.2, 0.5, 0.5)
    B, L, F = feats.shape
    energy, gnorm, grad = np.empty((B, 3)), np.empty(B), np.zeros((B, L, F))
    _binding.check(_binding.load().fd_relax_energy(device, ptr(feats), ptr(anc), ptr(lens), B, L, F, C.byref(prm), ptr(fix),
                                                   *(ptr(a) for a in packed), ptr(energy), ptr(gnorm), ptr(grad)))
    return energy, gnorm, [grad[b, : lens[b]].copy() for b in range(B)]


def relax(angles, lengths, feature_names: Sequence[str], restraints=None, fixed=None, n_iter: int = 200,
          move: Sequence[str] = ("phi", "psi", "omega"), alpha: float = 0.63, margin: float = 0.15, clash_weight: float = 1.0,
          tether: float = 0.0, step0: float = 0.01, grow: float = 1.2, shrink: float = 0.5, max_step: float = 0.5, device: int = 0,
          return_trace: bool = False) -> RelaxResult:
    """Relax finished backbones in torsion space on the device (``fd_relax``): ``n_iter`` steps of a descent
    with an adaptive step on  clash + restraints + tether, whose energy never rises.  The clash term is ``count_clashes``'
    rule made soft -- a pair closer than ``alpha (r_a + r_b) + margin`` costs ``clash_weight`` times the squared shortfall --
    so a chain whose clash energy reaches 0 has no clashing atom at ``alpha``.

    ``angles``: a list of ``[len_i, F]`` arrays, or a padded ``[B, L, F]`` array with ``lengths``; ``feature_names`` as for
    ``nerf.build_backbones``.  ``restraints``: as for ``pack_restraints`` (a ``Restraints`` per chain, one for all, or None).
    ``fixed``: per chain a boolean array over its residues or a list of residue indices whose angles keep their bits.
    ``move``: the columns that may change; ``tether``: the weight of the squared distance to the input angles.  ``step0``,
    ``grow``, ``shrink``, ``max_step``: a step starts at ``step0``, grows by ``grow`` when it lowered the energy, shrinks by
    ``shrink`` when it did not (the state then stays), and never moves the angles by more than ``max_step`` radians in norm.

    This is not a force field: backbone-only repulsion in torsion space removes clashes and keeps restraints, nothing more;
    whether relaxed backbones are more designable is unmeasured."""
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"n_iter={n_iter} must be >= 0")
    chains, feats, anc, lens, fix, prm, packed = _relax_inputs(angles, lengths, feature_names, restraints, fixed, None, move, alpha, margin,
                                                               clash_weight, tether, step0, grow, shrink, max_step)
    B, L, F = feats.shape
    lib = _binding.load()
    rst = [ptr(a) for a in packed]
    before, gnorm = np.empty((B, 3)), np.empty(B)
    _binding.check(lib.fd_relax_energy(device, ptr(feats), None, ptr(lens), B, L, F, C.byref(prm), ptr(fix), *rst, ptr(before), ptr(gnorm), None))
    out, after, accepted = feats.copy(), np.empty((B, 3)), np.zeros(B, dtype=np.int32)
    step = np.full(B, float(step0))
    trace = np.empty((max(n_iter, 0) + 1, B)) if return_trace else None
    _binding.check(lib.fd_relax(device, ptr(feats), None, ptr(lens), B, L, F, C.byref(prm), ptr(fix), *rst, n_iter, ptr(step), ptr(out),
                                ptr(after), ptr(trace), ptr(accepted)))
    relaxed = [out[b, : lens[b]].copy() for b in range(B)]
    clashes = count_clashes(nerf.build_backbones(chains + relaxed, feature_names, center_coords=False, device=device, method="scan"),
                            alpha=alpha, device=device)
    change = np.zeros(B)
    for b, (c, r) in enumerate(zip(chains, relaxed)):
        d = r.astype(np.float64) - c.astype(np.float64)
        ang = np.array([bool(prm.is_angle[f]) for f in range(F)])
        d[:, ang] = d[:, ang] - 2.0 * np.pi * np.floor((d[:, ang] + np.pi) / (2.0 * np.pi))
        change[b] = np.abs(d).max()
    return RelaxResult(relaxed, before, after, accepted.astype(np.int64), clashes[:B], clashes[B:], change, step, trace)


def relax_to_folder(angle_frames: Sequence[pd.DataFrame], names: Sequence[str], outdir: str, device: int = 0, **relax_args) -> dict:
    """``relax`` on the chains of ``angle_frames`` (DataFrames whose columns are the feature names; chains that share their
    columns go through one call) and its outputs in ``outdir``: ``relaxed_angles/{name}.csv.gz``, ``relaxed_pdb/{name}.pdb``
    and ``relax_report.json`` -- per chain the clashing atoms and the energy terms (clash | restraint | tether) before and
    after, the accepted steps and the largest angle change in radians.  Returns the report."""
    from .angles_and_coords import _write_chains
    names = [str(n) for n in names]
    if len(names) != len(angle_frames) or len(set(names)) != len(names):
        raise ValueError("one distinct name per chain")
    os.makedirs(os.path.join(outdir, "relaxed_angles"), exist_ok=True)
    groups = {}
    for i, df in enumerate(angle_frames):
        groups.setdefault(tuple(str(c) for c in df.columns), []).append(i)
    relaxed: List[Optional[pd.DataFrame]] = [None] * len(names)
    rows = {}
    for cols, members in groups.items():
        res = relax([np.nan_to_num(np.asarray(angle_frames[i].values, dtype=np.float32), nan=0.0) for i in members], None, list(cols),
                    device=device, **relax_args)
        for k, i in enumerate(members):
            relaxed[i] = pd.DataFrame(res.angles[k], columns=list(cols))
            rows[names[i]] = {"clashes_before": int(res.clashes_before[k]), "clashes_after": int(res.clashes_after[k]),
                              "energy_before": [float(v) for v in res.energy_before[k]], "energy_after": [float(v) for v in res.energy_after[k]],
                              "accepted": int(res.accepted[k]), "max_angle_change": float(res.max_change[k])}
    for name, df in zip(names, relaxed):
        df.to_csv(os.path.join(outdir, "relaxed_angles", f"{name}.csv.gz"))
    pdb_dir = os.path.join(outdir, "relaxed_pdb")
    os.makedirs(pdb_dir, exist_ok=True)
    _write_chains([os.path.join(pdb_dir, f"{name}.pdb") for name in names], relaxed, None, None, True, device)
    report = {"args": {k: (list(v) if isinstance(v, tuple) else v) for k, v in relax_args.items()},
              "energy_terms": ["clash", "restraint", "tether"], "chains": {n: rows[n] for n in names}}
    with open(os.path.join(outdir, "relax_report.json"), "w") as sink:
        json.dump(report, sink, indent=4)
    return report


# ---------------------------------------------------------------------------------------------------- cyclic oligomers
def symmetry_params(alpha: float = 0.63, margin: float = 0.15, clash_weight: float = 1.0, contact_weight: float = 0.1,
                    d_on: float = 8.0, d_off: float = 12.0, radial_weight: float = 0.01, r_max: float = 0.0, lever: float = 10.0,
                    max_shift: float = 1.0, step0: float = 0.01, grow: float = 1.2, shrink: float = 0.5,
                    pose_iters: int = 1) -> "_binding.FdSymmetryParams":
    """``fd_symmetry_params`` (include/fdmi.h).  The defaults are choices, not fits: the clash term is
    ``relax``' (``alpha``, ``margin``, ``clash_weight``); a CA-CA pair between copies earns up to ``contact_weight``, fully
    below ``d_on`` and nothing beyond ``d_off`` (Angstrom); ``radial_weight`` with ``r_max = 0`` is a weak pull of the CA
    centroid towards the axis, so that copies that start apart still meet.  ``lever`` (Angstrom) converts a torque into a turn,
    ``max_shift`` bounds what one step moves the chain, ``step0`` / ``grow`` / ``shrink`` are ``relax``' step rule, and
    ``pose_iters`` is how many rigid-body steps a guided visit takes.  Argument errors are left to the library."""
    p = _binding.FdSymmetryParams()
    p.clash_alpha, p.clash_margin, p.w_clash, p.w_contact = float(alpha), float(margin), float(clash_weight), float(contact_weight)
    p.d_on, p.d_off, p.w_radial, p.r_max = float(d_on), float(d_off), float(radial_weight), float(r_max)
    p.lever, p.max_shift, p.step0, p.grow, p.shrink = float(lever), float(max_shift), float(step0), float(grow), float(shrink)
    p.pose_iters, p.reserved = int(pose_iters), 0
    return p


def _orders(order, B: int) -> np.ndarray:
    """One int32 order per chain from a single order or one per chain."""
    out = np.ascontiguousarray(np.broadcast_to(np.asarray(order, dtype=np.int32), (B,)))
    if (out < 1).any() or (out > 12).any():
        raise ValueError(f"order={order!r}: symmetry orders lie in [1, 12]")
    return out


def start_pose(coords, order, radius=None, lengths: Optional[Sequence[int]] = None) -> np.ndarray:
    """Starting poses float64 ``[B, 12]`` (``Q`` row-major, then ``t``) for ``dock_cyclic`` and ``sample_symmetric``:
    ``Q = I`` and the chain's CA centroid at ``(radius, 0, 0)``.  ``coords``: one ``[3 len_i, 3]`` array per chain, or None
    with ``lengths`` when there is no structure yet.  ``radius`` defaults to ``Rg / sin(pi / n)`` with the chain's own CA
    radius of gyration -- neighbouring copies' centroids are then ``2 Rg`` apart --, or with ``Rg = 2.2 len^0.38`` without
    coordinates: NeRF's seed CA (``nerf.CA_INIT``, where every uncentred backbone has its first residue) then stands in for
    the centroid, so the chain's first residue starts at the radius; an order of 1 gets radius 0."""
    if coords is None:
        if lengths is None:
            raise ValueError("start_pose needs coords or lengths")
        B = len(lengths)
    else:
        xs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in coords]
        B = len(xs)
    orders = _orders(order, B)
    radii = None if radius is None else np.broadcast_to(np.asarray(radius, dtype=np.float64), (B,))
    pose = np.zeros((B, 12), dtype=np.float64)
    pose[:, [0, 4, 8]] = 1.0
    for b in range(B):
        if coords is None:
            centre, rg = nerf.CA_INIT, 2.2 * float(lengths[b]) ** 0.38
        else:
            ca = xs[b][1::3]
            centre = ca.mean(axis=0)
            rg = float(np.sqrt(((ca - centre) ** 2).sum(axis=1).mean()))
        if radii is not None:
            r = float(radii[b])
        else:
            r = rg / np.sin(np.pi / orders[b]) if orders[b] >= 2 else 0.0
        pose[b, 9:] = np.array([r, 0.0, 0.0]) - centre
    return pose


def cyclic_assembly(coords, pose, order) -> np.ndarray:
    """The explicit oligomer of one chain: float64 ``[n, 3 len, 3]``, copy ``k`` being ``R_k (Q p + t)`` with ``R_k`` the
    rotation by ``2 pi k / n`` about z (copy 0 is the placed chain itself)."""
    p = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    n = int(order)
    if not 1 <= n <= 12:
        raise ValueError(f"order={order!r}: symmetry orders lie in [1, 12]")
    y = p @ pose[:9].reshape(3, 3).T + pose[9:]
    out = np.empty((n,) + y.shape)
    for k in range(n):
        c, s = np.cos(2.0 * np.pi * k / n), np.sin(2.0 * np.pi * k / n)
        out[k] = y @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).T
    return out


def _symmetry_inputs(coords, order, pose):
    xs = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in coords]
    if not xs or any(len(x) % 3 or not len(x) for x in xs):
        raise ValueError("coords is a list of [3 len, 3] arrays")
    lens = np.array([len(x) // 3 for x in xs], dtype=np.int32)
    B, L = len(xs), int(lens.max())
    xyz = np.zeros((B, 3 * L, 3), dtype=np.float64)
    for b, x in enumerate(xs):
        xyz[b, : len(x)] = x
    poses = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(-1, 12))
    if len(poses) != B:
        raise ValueError(f"{len(poses)} poses for {B} chains")
    return xyz, lens, B, L, _orders(order, B), poses


def symmetry_energy(coords, order, pose, params=None, device: int = 0, return_wrench: bool = False, return_gradient: bool = False):
    """A batch of chains scored against their own C_n copies about z, in one ``fd_symmetry_energy`` call.  ``coords``: one
    ``[3 len_i, 3]`` array per chain; ``order``: one order for all or one per chain (1: not symmetric, zeros); ``pose``:
    ``[B, 12]`` as from ``start_pose``; ``params``: ``symmetry_params()``.  Returns ``(energy [B, 3] clash | contact | radial,
    contacts int32 [B])`` -- per subunit: ``n`` times clash + contact is the inter-chain energy of the explicit oligomer, and
    ``contacts`` counts ordered (CA, copy, CA) triples closer than ``d_on`` --, then with ``return_wrench`` ``[B, 6]`` (the
    force ``dE/dt`` and the torque about the origin) and with ``return_gradient`` the list of ``dE/dcoords`` ``[3 len_i, 3]``."""
    xyz, lens, B, L, orders, poses = _symmetry_inputs(coords, order, pose)
    prm = symmetry_params() if params is None else params
    energy, contacts = np.empty((B, 3)), np.empty(B, dtype=np.int32)
    wrench = np.empty((B, 6)) if return_wrench else None
    grad = np.empty((B, 3 * L, 3)) if return_gradient else None
    _binding.check(_binding.load().fd_symmetry_energy(device, ptr(xyz), ptr(lens), B, L, ptr(orders), ptr(poses), C.byref(prm), ptr(energy),
                                                      ptr(contacts), ptr(wrench), ptr(grad)))
    result = [energy, contacts]
    if return_wrench:
        result.append(wrench)
    if return_gradient:
        result.append([grad[b, : 3 * lens[b]].copy() for b in range(B)])
    return tuple(result)


class DockResult(NamedTuple):
    """What ``dock_cyclic`` returns, arrays over the chains: the poses ``[B, 12]``, the energy terms clash | contact | radial
    ``[B, 3]`` and the contacts there, the accepted steps, the step sizes to continue from, and with ``return_trace`` the total
    energy after every iteration (``[n_iter + 1, B]``)."""
    pose: np.ndarray
    energy: np.ndarray
    contacts: np.ndarray
    accepted: np.ndarray
    step: np.ndarray
    trace: Optional[np.ndarray]


def dock_cyclic(coords, order, pose=None, n_iter: int = 100, params=None, step=None, device: int = 0,
                return_trace: bool = False) -> DockResult:
    """Dock rigid chains into C_n assemblies on the device (``fd_symmetry_dock``): ``n_iter`` steps of a
    descent with an adaptive step on the pose alone, whose energy never rises; the chains' internal coordinates do not
    change.  ``pose`` defaults to ``start_pose(coords, order)``; ``step``: the step sizes of an earlier result to continue
    from.  This is no docking program: backbone-only repulsion, a CA contact reward and a pull to the axis; what the
    interfaces are worth is unmeasured."""
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"n_iter={n_iter} must be >= 0")
    if pose is None:
        pose = start_pose(coords, order)
    xyz, lens, B, L, orders, poses = _symmetry_inputs(coords, order, pose)
    prm = symmetry_params() if params is None else params
    h = np.full(B, float(prm.step0)) if step is None else np.ascontiguousarray(np.asarray(step, dtype=np.float64).reshape(B)).copy()
    out, energy, contacts = np.empty((B, 12)), np.empty((B, 3)), np.empty(B, dtype=np.int32)
    accepted = np.zeros(B, dtype=np.int32)
    trace = np.empty((n_iter + 1, B)) if return_trace else None
    _binding.check(_binding.load().fd_symmetry_dock(device, ptr(xyz), ptr(lens), B, L, ptr(orders), ptr(poses), C.byref(prm), n_iter, ptr(h),
                                                    ptr(out), ptr(energy), ptr(contacts), ptr(trace), ptr(accepted)))
    return DockResult(out, energy, contacts, accepted.astype(np.int64), h, trace)


class RmsdScorer:
    """A ``scorer=`` for ``sampling.get_reconstruction_error``: per item (RMSD of NeRF(reconstruction) to NeRF(truth),
    RMSD of NeRF(reconstruction) to the backbone of the item's PDB file), in Angstrom after optimal superposition --
    the reference's ``_score_angles`` (foldingdiff/sampling.py:266-284) with RMSD in place of the TM-score.

    Like the reference, it builds the backbones from the angles exactly as ``reconstruct`` returns them: the training
    mean offset is NOT added back first.  The feature names follow from the number of columns (9, 6 or 4: the
    ``canonical*`` sets).  The file's backbone is compared over the residues the item holds (the first ``len`` of
    them: left-aligned items); an unreadable file scores NaN.  ``score_batch`` scores all items of a call with one NeRF
    launch and one RMSD launch; ``get_reconstruction_error`` uses it."""

    def __init__(self, device: int = 0):
        self.device = device

    def __call__(self, reconst_angles, truth_angles, truth_pdb_file: str) -> Tuple[float, float]:
        s, c = self.score_batch([reconst_angles], [truth_angles], [truth_pdb_file])
        return float(s[0]), float(c[0])

    def score_batch(self, recon: Sequence, truth: Sequence, files: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        n = len(recon)
        assert len(truth) == n == len(files)
        if n == 0:
            return np.zeros((0,)), np.zeros((0,))
        recon = [np.asarray(r, dtype=np.float32) for r in recon]
        truth = [np.asarray(t, dtype=np.float32) for t in truth]
        F = recon[0].shape[1]
        names = [v for k, v in datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES.items() if k in DATASETS and len(v) == F]
        assert names, f"no canonical feature set has {F} features"
        xyz = nerf.build_backbones(recon + truth, names[0], device=self.device)
        a, b, which = [], [], []
        for i, f in enumerate(files):
            a.append(xyz[i]); b.append(xyz[n + i]); which.append(("angles", i))
            bb = read_backbone(f) if os.path.isfile(f) else None
            if bb is not None and len(bb[0]) >= len(xyz[i]):
                a.append(xyz[i]); b.append(bb[0][: len(xyz[i])]); which.append(("coords", i))
        r = superposed_rmsd(a, b, device=self.device)
        scores, coord_scores = np.full(n, np.nan), np.full(n, np.nan)
        for (kind, i), v in zip(which, r):
            (scores if kind == "angles" else coord_scores)[i] = v
        return scores, coord_scores


rmsd_scorer = RmsdScorer()


TM_MAX_LEN = 2048     # FDMI_TM_MAX_LEN and FDMI_SSE_MAX_LEN


def tm_d0(Ln: int) -> float:
    """The TM-score's distance scale for normalisation length ``Ln``: 1.24 cbrt(Ln - 15) - 1.8 for Ln > 21, else 0.5."""
    return 1.24 * float(np.cbrt(Ln - 15)) - 1.8 if Ln > 21 else 0.5


def tm_score(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], norm_lens: Optional[Sequence[int]] = None,
             stride: int = 1, device: int = 0, return_transform: bool = False):
    """TM-score of each residue-paired CA trace pair (a[i], b[i], each [n_i, 3] with 1 <= n_i <= 2048), normalised by
    ``norm_lens[i]`` (>= n_i; default n_i), in one ``fd_tm_score`` call: float64 [len(a_list)], plus R [n, 3, 3] and
    t [n, 3] with b ~ a @ R.T + t when ``return_transform`` is set.

    The score is the maximum over superpositions found by the seed-and-extend search of Zhang & Skolnick (2004):
    seed fragments of lengths n, n/2, n/4, ... and min(n, 4) starting every ``stride`` residues, each extended by
    repeatedly refitting on the residues within d_cut (DESIGN.md "TM-score" states the rules).  It is not pinned to the
    TMscore / TMalign binaries; TM-align also searches the residue alignment, so its number is usually the same or
    higher."""
    if len(a_list) != len(b_list):
        raise ValueError(f"{len(a_list)} traces against {len(b_list)}")
    a, b = _ca_traces(a_list, TM_MAX_LEN, "a"), _ca_traces(b_list, TM_MAX_LEN, "b")
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape:
            raise ValueError(f"pair {i}: {x.shape} vs {y.shape}; expected two traces of one length")
    (A, offsets, lens), B = _pack(a), _pack(b)[0]
    nl = lens if norm_lens is None else _norm_lens(norm_lens, lens, "n_i")
    if int(stride) < 1:
        raise ValueError(f"stride={stride} must be >= 1")
    n = len(a)
    out = np.empty((n,), dtype=np.float64)
    T = np.empty((n, 12), dtype=np.float64)
    if n == 0:
        return (out, T[:, :9].reshape(0, 3, 3), T[:, 9:]) if return_transform else out
    _binding.check(_binding.load().fd_tm_score(device, ptr(A), ptr(B), ptr(offsets), ptr(lens), ptr(nl), n, int(stride),
                                               ptr(out), ptr(T)))
    if return_transform:
        return out, T[:, :9].reshape(n, 3, 3).copy(), T[:, 9:].copy()
    return out


class TmScorer:
    """A ``scorer=`` for ``sampling.get_reconstruction_error``: per item (TM-score of NeRF(reconstruction) to
    NeRF(truth), TM-score of NeRF(reconstruction) to the item's PDB file), over CA atoms -- the two TM-scores of the
    reference's ``_score_angles`` (foldingdiff/sampling.py:266-284), with ``tm_score``'s search in place of TM-align.

    The first is normalised by the item's length.  The second compares with the first ``len`` CA atoms of the file
    (left-aligned items) and is normalised by the file's residue count, as TM-align normalises by its second chain;
    an unreadable file, or one shorter than the item, scores NaN.  Like the reference (and ``RmsdScorer``), the
    backbones are built from the angles exactly as ``reconstruct`` returns them: the training mean offset is NOT added
    back first.  ``score_batch`` scores all items of a call with one NeRF launch and one TM-score launch."""

    def __init__(self, device: int = 0, stride: int = 1):
        self.device, self.stride = device, stride

    def __call__(self, reconst_angles, truth_angles, truth_pdb_file: str) -> Tuple[float, float]:
        s, c = self.score_batch([reconst_angles], [truth_angles], [truth_pdb_file])
        return float(s[0]), float(c[0])

    def score_batch(self, recon: Sequence, truth: Sequence, files: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        n = len(recon)
        assert len(truth) == n == len(files)
        if n == 0:
            return np.zeros((0,)), np.zeros((0,))
        recon = [np.asarray(r, dtype=np.float32) for r in recon]
        truth = [np.asarray(t, dtype=np.float32) for t in truth]
        F = recon[0].shape[1]
        names = [v for k, v in datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES.items() if k in DATASETS and len(v) == F]
        assert names, f"no canonical feature set has {F} features"
        xyz = nerf.build_backbones(recon + truth, names[0], device=self.device)
        a, b, norm, which = [], [], [], []
        for i, f in enumerate(files):
            ca = xyz[i][1::3]
            a.append(ca); b.append(xyz[n + i][1::3]); norm.append(len(ca)); which.append(("angles", i))
            bb = read_backbone(f) if os.path.isfile(f) else None
            if bb is not None and len(bb[0]) >= len(xyz[i]):
                file_ca = bb[0][1::3]
                a.append(ca); b.append(file_ca[: len(ca)]); norm.append(len(file_ca)); which.append(("coords", i))
        r = tm_score(a, b, norm_lens=norm, stride=self.stride, device=self.device)
        scores, coord_scores = np.full(n, np.nan), np.full(n, np.nan)
        for (kind, i), v in zip(which, r):
            (scores if kind == "angles" else coord_scores)[i] = v
        return scores, coord_scores


tm_scorer = TmScorer()


# ---------------------------------------------------------------------------------------------------- secondary structure
_SSE_LABELS = np.array(["c", "a", "b"])


def _annotate(ca_list: Sequence[np.ndarray], device: int) -> Tuple[List[np.ndarray], np.ndarray]:
    """(int8 labels per chain, int32 [len, 2] counts) of one ``fd_annotate_sse`` call."""
    ca = _ca_traces(ca_list, TM_MAX_LEN)
    n = len(ca)
    counts = np.zeros((n, 2), dtype=np.int32)
    if n == 0:
        return [], counts
    X, offsets, lens = _pack(ca)
    sse = np.empty((len(X),), dtype=np.int8)
    _binding.check(_binding.load().fd_annotate_sse(device, ptr(X), ptr(offsets), ptr(lens), n, ptr(sse), ptr(counts)))
    return [sse[o: o + m] for o, m in zip(offsets, lens)], counts


def annotate_sse(ca_list: Sequence[np.ndarray], device: int = 0) -> List[np.ndarray]:
    """Secondary structure of each CA trace ([n_i, 3], any float dtype, 1 <= n_i <= 2048): a ``'U1'`` array of 'a'
    (helix), 'b' (strand) and 'c' (coil) per chain, all chains in one ``fd_annotate_sse`` launch.

    The labels are those of the P-SEA algorithm (Labesse et al. 1997) as biotite's ``annotate_sse`` restates it, from
    CA-CA distances, angles and dihedrals alone (DESIGN.md "Secondary structure (P-SEA)" states the rules).  They are
    not pinned to biotite."""
    return [_SSE_LABELS[s] for s in _annotate(ca_list, device)[0]]


def count_secondary_structures(ca_list: Sequence[np.ndarray], device: int = 0) -> np.ndarray:
    """int [len(ca_list), 2]: the number of helices and of strands (maximal runs of 'a' and of 'b' in
    ``annotate_sse``'s labels) of each CA trace, in one launch."""
    return _annotate(ca_list, device)[1].astype(np.int64)


def _single_chain_ca(fname: str) -> Optional[np.ndarray]:
    """CA trace of a file for ``count_structures_in_pdb``: ``None`` for a file ``read_backbone`` rejects (more than one
    model, like the reference; also a residue without N / CA / C, parser rule 7); one chain only, as the reference
    asserts."""
    assert os.path.exists(fname), fname
    bb = read_backbone(fname)
    if bb is None:
        return None
    chains = sorted({rid[0] for rid in bb[1]})
    assert len(chains) == 1, f"{fname}: chains {chains}, expected one"
    return bb[0][1::3]


def _count_files(fnames: Sequence[str], device: int) -> List[Tuple[int, int]]:
    traces = [_single_chain_ca(f) for f in fnames]
    ok = [i for i, t in enumerate(traces) if t is not None]
    counts = count_secondary_structures([traces[i] for i in ok], device=device)
    out = [(-1, -1)] * len(fnames)
    for i, c in zip(ok, counts):
        out[i] = (int(c[0]), int(c[1]))
    return out


def count_structures_in_pdb(fname: str, backend: str = "psea", device: int = 0) -> Tuple[int, int]:
    """(# alpha helices, # beta strands) of the single chain in a PDB file, (-1, -1) for a file with several models:
    ``count_structures_in_pdb`` (bin/annot_secondary_structures.py:64-105) with ``annotate_sse`` above."""
    if backend != "psea":
        raise ValueError(f"Unrecognized backend for calculating secondary structures: {backend} (only psea exists here)")
    return _count_files([fname], device)[0]


def write_ss_cooccurrence(names: Sequence[str], counts: Sequence[Sequence[int]], json_file: str = "", outpdf: str = "",
                          title: str = "Secondary structure co-occurrence", **kwargs) -> None:
    """The output half of ``make_ss_cooccurrence_plot`` (bin/annot_secondary_structures.py:137-166) for counts already
    at hand: the JSON ``{name: [n_alpha, n_beta]}`` and the 2-D histogram (``**kwargs`` go to ``hist2d``).  Without
    matplotlib the plot is skipped with a log line."""
    counts = [(int(a), int(b)) for a, b in counts]
    assert len(names) == len(counts)
    if json_file:
        logging.info(f"Writing json of ss counts to {json_file}")
        with open(json_file, "w") as sink:
            json.dump({k: list(ab) for k, ab in zip(names, counts)}, sink, indent=4)
    if not outpdf:
        return
    if not counts:
        logging.warning(f"No structures to plot, not writing {outpdf}")
        return
    try:
        from matplotlib.figure import Figure
    except ImportError as e:
        logging.warning(f"matplotlib is not available ({e}), not writing {outpdf}")
        return
    fig = Figure(dpi=300)
    ax = fig.subplots()
    h = ax.hist2d([c[0] for c in counts], [c[1] for c in counts], bins=np.arange(10), density=True, vmin=0.0, **kwargs)
    ax.set_xlabel(r"Number of $\alpha$ helices", fontsize=12)
    ax.set_ylabel(r"Number of $\beta$ sheets", fontsize=12)
    if title:
        ax.set_title(title.strip(), fontsize=14)
    cbar = fig.colorbar(h[-1], ax=ax)
    cbar.ax.set_ylabel("Frequency", fontsize=12)
    fig.savefig(outpdf, bbox_inches="tight")


def ss_cooccurrence(pdb_files: Sequence[str], json_file: str = "", outpdf: str = "", max_seq_len: int = 0,
                    title: str = "Secondary structure co-occurrence", device: int = 0, **kwargs) -> Tuple[np.ndarray, np.ndarray]:
    """``make_ss_cooccurrence_plot`` (bin/annot_secondary_structures.py:108-166): helix and strand counts of every
    file from one ``fd_annotate_sse`` call, files that give (-1, -1) dropped, files of more than ``max_seq_len``
    residues (when > 0) left out; writes ``json_file`` and ``outpdf`` when named (``write_ss_cooccurrence``) and
    returns (alpha counts, beta counts).  The JSON pairs each kept file with its own counts (the reference zips the
    unfiltered file list with the filtered counts)."""
    pdb_files = list(pdb_files)
    if max_seq_len > 0:
        orig_len = len(pdb_files)
        parsed = [read_backbone(p) for p in pdb_files]
        pdb_files = [p for p, bb in zip(pdb_files, parsed) if bb is None or len(bb[1]) <= max_seq_len]
        logging.info(f"Filtering out sequences with more than {max_seq_len} residues: {orig_len} --> {len(pdb_files)}")
    logging.info(f"Calculating {len(pdb_files)} structures using psea")
    kept = [(p, c) for p, c in zip(pdb_files, _count_files(pdb_files, device)) if c != (-1, -1)]
    write_ss_cooccurrence([os.path.basename(p) for p, _ in kept], [c for _, c in kept], json_file=json_file,
                          outpdf=outpdf, title=title, **kwargs)
    counts = np.array([c for _, c in kept], dtype=np.int64).reshape(-1, 2)
    return counts[:, 0], counts[:, 1]


# ---------------------------------------------------------------------------------------------------- oxygens, DSSP
DSSP_MAX_LEN = 1024   # FDMI_DSSP_MAX_LEN
DSSP_STATES = np.array(list("-HBEGITS"))   # fd_dssp's state codes 0 .. 7
DSSP_NO_DONOR, DSSP_NO_ACCEPTOR = 1, 2     # fd_dssp's flag bits
_BACKBONE_O = _BACKBONE + ("O",)


def read_backbone_atoms(fname: str) -> Optional[Tuple[np.ndarray, List[str]]]:
    """N, CA, C and O of every residue of a ``.pdb`` / ``.pdb.gz`` file: (float64 [n, 4, 3], the n residue names), or
    ``None`` for a file ``read_backbone`` rejects.  The same rules 1-7 (the module docstring); O is optional: the O row of
    a residue without an O record (a generated backbone, or the last residue of ``write_backbone_with_o_pdb``'s files)
    is NaN."""
    n_models = 0
    atoms, names, order = {}, {}, []
    with _open(fname) as fh:
        for line in fh:
            rec = line[:6]
            if rec == "MODEL ":
                n_models += 1
                continue
            if rec != "ATOM  " and not (rec == "HETATM" and line[17:20] == "MSE"):
                continue
            name = line[12:16].strip()
            if name not in _BACKBONE_O:
                continue
            rid = (line[21], line[22:26].strip(), line[26].strip())
            res = atoms.get(rid)
            if res is None:
                res = atoms[rid] = {}
                names[rid] = line[17:20].strip()
                order.append(rid)
            if name not in res:
                res[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    if n_models > 1 or not order or any(a not in atoms[rid] for rid in order for a in _BACKBONE):
        logging.debug(f"{fname}: several models, no backbone atoms or a residue without N / CA / C - skipping")
        return None
    nan = (np.nan, np.nan, np.nan)
    xyz = np.array([[atoms[rid].get(a, nan) for a in _BACKBONE_O] for rid in order], dtype=np.float64)
    return xyz, [names[rid] for rid in order]


def _residue_arrays(chains: Sequence[np.ndarray], atoms: int, what: str) -> List[np.ndarray]:
    """The chains as float64 [n, atoms, 3] arrays (an [atoms n, 3] array is reshaped), 1 <= n <= DSSP_MAX_LEN."""
    out = []
    for i, x in enumerate(chains):
        x = np.asarray(x, dtype=np.float64)
        ok = (x.ndim == 2 and x.shape[1] == 3 and len(x) % atoms == 0) or (x.ndim == 3 and x.shape[1:] == (atoms, 3))
        if not ok or not 1 <= x.size // (3 * atoms) <= DSSP_MAX_LEN:
            raise ValueError(f"{what} {i}: {x.shape}; expected [n, {atoms}, 3] or [{atoms} n, 3] with 1 <= n <= {DSSP_MAX_LEN}")
        out.append(x.reshape(-1, atoms, 3))
    return out


def add_oxygens(backbones: Sequence[np.ndarray], reference_torsion: bool = False, device: int = 0) -> List[np.ndarray]:
    """The carbonyl oxygens of N / CA / C backbones (each [3n, 3] or [n, 3, 3], 1 <= n <= 1024), all of them in one
    ``fd_backbone_oxygens`` launch: float64 [n, 4, 3] per backbone, N, CA, C copied and O placed at the CA-C-O angle
    2.0992622 rad and C=O length 1.2359372 A of the reference's bin/add_oxygen_to_backbone.py, trans to the next residue's
    N (torsion psi + pi).  ``reference_torsion``: the torsion psi that script passes, which puts the O where the next N
    is.  The last residue has no psi; its O row is NaN, as the reference gives it no oxygen."""
    xs = _residue_arrays(backbones, 3, "backbone")
    if not xs:
        return []
    X, offsets, lens = _pack(xs)
    out = np.empty((len(X), 4, 3), dtype=np.float64)
    _binding.check(_binding.load().fd_backbone_oxygens(device, ptr(X), ptr(offsets), ptr(lens), len(xs), int(bool(reference_torsion)),
                                                       ptr(out)))
    return [out[o: o + n] for o, n in zip(offsets, lens)]


def _dssp(chains, flags, device: int, want_bonds: bool):
    """One ``fd_dssp`` call: (int8 states per chain, int32 [n_chains, 3] counts, (acc, energy) per chain or None)."""
    xs = _residue_arrays(chains, 4, "chain")
    n = len(xs)
    counts = np.zeros((n, 3), dtype=np.int32)
    if n == 0:
        return [], counts, ([] if want_bonds else None)
    X, offsets, lens = _pack(xs)
    fl = None
    if flags is not None:
        if len(flags) != n or any(len(np.reshape(f, -1)) != m for f, m in zip(flags, lens)):
            raise ValueError("flags: expected one uint8 array of the chain's length per chain")
        fl = np.ascontiguousarray(np.concatenate([np.reshape(f, -1) for f in flags]), dtype=np.uint8)
    state = np.empty((len(X),), dtype=np.int8)
    acc = np.empty((len(X), 2), dtype=np.int32) if want_bonds else None
    energy = np.empty((len(X), 2), dtype=np.float64) if want_bonds else None
    _binding.check(_binding.load().fd_dssp(device, ptr(X), ptr(fl), ptr(offsets), ptr(lens), n, ptr(state), ptr(acc), ptr(energy),
                                           ptr(counts)))
    cut = lambda a: [a[o: o + m] for o, m in zip(offsets, lens)]   # noqa: E731
    return cut(state), counts, (list(zip(cut(acc), cut(energy))) if want_bonds else None)


def dssp(chains: Sequence[np.ndarray], flags: Optional[Sequence[np.ndarray]] = None, device: int = 0, return_hbonds: bool = False):
    """DSSP states of N / CA / C / O backbones (each [n, 4, 3] or [4n, 3], 1 <= n <= 1024; an O row of NaN is a residue
    without oxygen), all chains in one ``fd_dssp`` launch: a ``'U1'`` array of ``-HBEGITS`` per chain.  With
    ``return_hbonds`` also a list of ``(acc int32 [n, 2], energy float64 [n, 2])``: per donor residue its two kept
    acceptors (chain-local, -1 where none) and their energies in kcal/mol.

    ``flags``: per chain a uint8 [n] array, bit 0 (``DSSP_NO_DONOR``) for a residue without an amide hydrogen (proline),
    bit 1 (``DSSP_NO_ACCEPTOR``) for one that accepts nothing.

    The rules are Kabsch & Sander's (1983), restated in DESIGN.md 6t; beta-bulges and sheet labels are not built, and
    the labels are not pinned to the mkdssp binary."""
    states, _, bonds = _dssp(chains, flags, device, return_hbonds)
    out = [DSSP_STATES[s] for s in states]
    return (out, bonds) if return_hbonds else out


def dssp_counts(chains: Sequence[np.ndarray], flags: Optional[Sequence[np.ndarray]] = None, device: int = 0) -> np.ndarray:
    """int [len(chains), 3]: kept hydrogen bonds, maximal runs of 'H' and maximal runs of 'E' of each chain (``dssp``'s
    labels), in one launch."""
    return _dssp(chains, flags, device, False)[1].astype(np.int64)


def dssp_from_backbones(backbones: Sequence[np.ndarray], device: int = 0, return_hbonds: bool = False):
    """``dssp(add_oxygens(backbones))``: for NeRF output, where every residue is a glycine and none a proline."""
    return dssp(add_oxygens(backbones, device=device), device=device, return_hbonds=return_hbonds)


def dssp_of_pdb(fname: str, device: int = 0) -> Optional[np.ndarray]:
    """``dssp`` labels of a PDB file (``None`` for one ``read_backbone`` rejects, or of more than 1024 residues): the file's
    own O atoms where every residue but the last has one, ``add_oxygens`` otherwise; PRO is flagged as no donor."""
    bb = read_backbone_atoms(fname)
    if bb is None or len(bb[0]) > DSSP_MAX_LEN:
        return None
    xyz, names = bb
    if np.isnan(xyz[:-1, 3]).any():
        xyz = add_oxygens([xyz[:, :3]], device=device)[0]
    flags = np.array([DSSP_NO_DONOR if n == "PRO" else 0 for n in names], dtype=np.uint8)
    return dssp([xyz], flags=[flags], device=device)[0]


# ---------------------------------------------------------------------------------------------------- alignment
ALIGN_MAX_LEN = 512   # FDMI_ALIGN_MAX_LEN
_ALIGN_MAX_SEEDS = 256


def _tm_seed_count(n: int, stride: int) -> int:
    lmin = min(n, 4)
    lengths, l = [], n
    while l > lmin:
        lengths.append(l)
        l //= 2
    lengths.append(lmin)
    return sum((n - l) // stride + 1 + ((n - l) % stride != 0) for l in lengths)


def tm_align_stride(n_ali: int) -> int:
    """The stride at which ``fd_tm_align`` searches an alignment of ``n_ali`` pairs: the smallest s >= 1 that leaves
    at most 256 seeds (one lane each)."""
    s = 1
    while _tm_seed_count(int(n_ali), s) > _ALIGN_MAX_SEEDS:
        s += 1
    return s


def _align_traces(chains: Sequence[np.ndarray], what: str = "chain") -> List[np.ndarray]:
    return _ca_traces(chains, ALIGN_MAX_LEN, what)


ALIGN_STARTS = ("threading", "ss", "ss_dist", "local", "fragment")   # bit k of FDMI_ALIGN_START_*: 1 << k
_DEFAULT_STARTS = ("threading", "ss")


def align_start_bits(starts=_DEFAULT_STARTS) -> int:
    """The ``starts`` bit set of ``fd_tm_align_ex`` for a selection of ``ALIGN_STARTS`` names; ``"all"`` is all five.
    An unknown name, an empty selection and a repeated name raise ValueError."""
    if isinstance(starts, str):
        starts = ALIGN_STARTS if starts == "all" else (starts,)
    names = list(starts)
    if not names:
        raise ValueError("starts: empty selection")
    bits = 0
    for name in names:
        if name not in ALIGN_STARTS:
            raise ValueError(f"starts: unknown start {name!r}; expected \"all\" or names from {ALIGN_STARTS}")
        if bits & (1 << ALIGN_STARTS.index(name)):
            raise ValueError(f"starts: {name!r} is named twice")
        bits |= 1 << ALIGN_STARTS.index(name)
    return bits


def _align_indexed(chains: List[np.ndarray], pair_a: np.ndarray, pair_b: np.ndarray, norm_lens, max_iter: int, device: int,
                   want_map: bool, starts=_DEFAULT_STARTS, want_start_tms: bool = False):
    """One ``fd_tm_align`` call (``fd_tm_align_ex`` for any but the default starts, or when the per-start scores are
    wanted) over already-checked float64 traces: (tm [P], T [P, 12], n_ali [P], maps or None), and the [P, 5] per-start
    scores with ``want_start_tms``."""
    bits = align_start_bits(starts)
    X, offsets, lens = _pack(chains)
    P = len(pair_a)
    pa, pb = np.ascontiguousarray(pair_a, dtype=np.int32), np.ascontiguousarray(pair_b, dtype=np.int32)
    if P and (min(pa.min(), pb.min()) < 0 or max(pa.max(), pb.max()) >= len(chains)):
        raise ValueError(f"pair indices must lie in [0, {len(chains)})")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter={max_iter} must be >= 1")
    nl = lens[pb] if norm_lens is None else _norm_lens(norm_lens, np.minimum(lens[pa], lens[pb]), "min(n1, n2)")
    tm = np.empty((P,), dtype=np.float64)
    T = np.empty((P, 12), dtype=np.float64)
    n_ali = np.empty((P,), dtype=np.int32)
    start_tms = np.empty((P, len(ALIGN_STARTS)), dtype=np.float64) if want_start_tms else None
    if P == 0:
        return (tm, T, n_ali, ([] if want_map else None)) + ((start_tms,) if want_start_tms else ())
    map_off = flat = None
    if want_map:
        map_off = np.concatenate([[0], np.cumsum(lens[pa], dtype=np.int64)[:-1]]).astype(np.int64)
        flat = np.empty((int(lens[pa].sum()),), dtype=np.int32)
    args = (device, ptr(X), ptr(offsets), ptr(lens), len(chains), ptr(pa), ptr(pb), ptr(nl), P, int(max_iter), ptr(tm), ptr(T),
            ptr(n_ali), ptr(map_off), ptr(flat))
    if bits == align_start_bits(_DEFAULT_STARTS) and not want_start_tms:
        _binding.check(_binding.load().fd_tm_align(*args))
    else:
        _binding.check(_binding.load().fd_tm_align_ex(*args, bits, ptr(start_tms)))
    maps = [flat[o: o + lens[i]].copy() for o, i in zip(map_off, pa)] if want_map else None
    return (tm, T, n_ali, maps) + ((start_tms,) if want_start_tms else ())


def _polish(chains, pa, pb, nl, maps, device):
    """``tm_score`` at stride 1 over the aligned pairs of each map, normalised as the alignment was."""
    xa = [chains[i][m >= 0] for i, m in zip(pa, maps)]
    ya = [chains[j][m[m >= 0]] for j, m in zip(pb, maps)]
    return tm_score(xa, ya, norm_lens=nl, stride=1, device=device, return_transform=True)


def tm_align(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], norm_lens: Optional[Sequence[int]] = None,
             max_iter: int = 10, return_transform: bool = False, return_map: bool = False, polish: bool = False,
             device: int = 0, starts=_DEFAULT_STARTS, return_start_tms: bool = False):
    """TM-score of each pair of CA traces (a[i] [n1, 3], b[i] [n2, 3], 1 <= n <= 512) whose residues need not
    correspond, in one ``fd_tm_align`` call: float64 [len(a_list)], normalised by ``norm_lens[i]`` (>= min(n1, n2);
    default n2, the "Chain_2" number ``tmalign.run_tmalign`` returns).  With ``return_transform`` also R [n, 3, 3] and
    t [n, 3] with b ~ a @ R.T + t; with ``return_map`` also a list of int32 [n1] maps, ``map[i]`` = the residue of b
    aligned with residue i of a, or -1.

    The residue alignment and the superposition are searched together in the manner of TM-align (Zhang & Skolnick
    2005): two starts (the best gapless threading; a dynamic programme over P-SEA labels), each refined by up to
    ``max_iter`` rounds of dynamic programming on the superposition's score matrix with gap-open penalties -0.6 and 0,
    every alignment scored by ``tm_score``'s search at the coarse stride ``tm_align_stride(n_ali)`` (DESIGN.md
    "TM-align-style alignment" states the rules).  It is not pinned to the TMalign binary; with fewer starts than
    TM-align's five it is a lower bound on the optimum TM-align looks for.

    ``starts``: the starts to search from, names from ``ALIGN_STARTS`` ("threading", "ss", "ss_dist": labels plus
    distances under the threading's superposition, "local": the best of up to 128 fragment-pair superpositions,
    "fragment": threading of the longest stretch without a chain break) or ``"all"``; any but the default goes through
    ``fd_tm_align_ex``.  More starts never score lower.  With ``return_start_tms`` also (last) a float64 [n, 5] array:
    the best score reached from each start (at the coarse stride, with ``polish`` too), -1 where it was not requested
    or does not apply to the pair.

    ``polish``: the aligned pairs are scored again by ``tm_score`` at stride 1.  Stride 1's seeds contain the coarse
    stride's, so the polished score (and its transform) is never lower."""
    if len(a_list) != len(b_list):
        raise ValueError(f"{len(a_list)} traces against {len(b_list)}")
    a, b = _align_traces(a_list, "a"), _align_traces(b_list, "b")
    n = len(a)
    pa, pb = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
    got = _align_indexed(a + b, pa, pb, norm_lens, max_iter, device, return_map or polish, starts, return_start_tms)
    tm, T, _, maps = got[:4]
    start_tms = got[4] if return_start_tms else None
    R, t = T[:, :9].reshape(n, 3, 3).copy(), T[:, 9:].copy()
    if polish and n:
        nl = [len(y) for y in b] if norm_lens is None else list(norm_lens)
        tm, R, t = _polish(a + b, pa, pb, nl, maps, device)
    out = (tm,) + ((R, t) if return_transform else ()) + ((maps,) if return_map else ()) + ((start_tms,) if return_start_tms else ())
    return out if len(out) > 1 else tm


def pairwise_tm(chains: Sequence[np.ndarray], pairs=None, norm_lens: Optional[Sequence[int]] = None, max_iter: int = 10,
                polish: bool = False, chunk: int = 1 << 16, device: int = 0, starts=_DEFAULT_STARTS) -> np.ndarray:
    """``tm_align`` scores of ``pairs`` (an [P, 2] list of (i, j) indices into ``chains``: chain i aligned to chain j,
    normalised by chain j's length unless ``norm_lens`` says otherwise; default every i < j in row order): float64 [P].
    The pair list is cut into chunks of ``chunk`` pairs and every call uploads only the chains its chunk names, so the
    host and device buffers stay bounded however long the list is.  ``starts`` as in ``tm_align``."""
    align_start_bits(starts)
    ca = _align_traces(chains)
    if pairs is None:
        iu = np.triu_indices(len(ca), k=1)
        pairs = np.stack(iu, axis=1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(ca)):
        raise ValueError(f"pair indices must lie in [0, {len(ca)})")
    if int(chunk) < 1:
        raise ValueError(f"chunk={chunk} must be >= 1")
    nl = None
    if norm_lens is not None:
        nl = np.asarray(norm_lens, dtype=np.int64).reshape(-1)
        if nl.shape != (len(pairs),):
            raise ValueError(f"norm_lens must hold one length per pair ({len(pairs)}), got {nl.shape}")
    out = np.empty((len(pairs),), dtype=np.float64)
    for lo in range(0, len(pairs), int(chunk)):
        sub = pairs[lo: lo + int(chunk)]
        used, inv = np.unique(sub, return_inverse=True)
        inv = inv.reshape(sub.shape)
        local = [ca[i] for i in used]
        sub_nl = None if nl is None else nl[lo: lo + len(sub)]
        tm, _, _, maps = _align_indexed(local, inv[:, 0], inv[:, 1], sub_nl, max_iter, device, polish, starts)
        if polish:
            pnl = [len(local[j]) for j in inv[:, 1]] if sub_nl is None else list(sub_nl)
            tm = _polish(local, inv[:, 0], inv[:, 1], pnl, maps, device)[0]
        out[lo: lo + len(sub)] = tm
    return out


def max_tm_across_refs(query_ca: Sequence[np.ndarray], refs_ca: Sequence[np.ndarray], max_iter: int = 10,
                       polish: bool = False, chunk: int = 1 << 16, device: int = 0,
                       starts=_DEFAULT_STARTS) -> Tuple[np.ndarray, np.ndarray]:
    """(max, argmax) over the references of the ``tm_align`` score of every query against every reference, normalised
    by the reference's length: ``tmalign.max_tm_across_refs`` (foldingdiff/tmalign.py:57-83) for many queries at once.
    float64 [n_queries] and int64 [n_queries] (the first reference on a tie).  ``starts`` as in ``tm_align``."""
    align_start_bits(starts)
    q, r = _align_traces(query_ca, "query"), _align_traces(refs_ca, "reference")
    if not r:
        raise ValueError("no references")
    nq, nr = len(q), len(r)
    qi, ri = np.meshgrid(np.arange(nq), np.arange(nr), indexing="ij")
    pairs = np.stack([qi.ravel(), nq + ri.ravel()], axis=1)
    tm = pairwise_tm(q + r, pairs, max_iter=max_iter, polish=polish, chunk=chunk, device=device, starts=starts).reshape(nq, nr)
    best = tm.argmax(axis=1) if nq else np.zeros((0,), np.int64)
    return tm[np.arange(nq), best], best.astype(np.int64)


def _alignable_files(fnames: Sequence[str]) -> Tuple[List[str], List[np.ndarray]]:
    """The files ``tm_align`` can take and their CA traces: files ``read_backbone`` rejects and chains of more than
    512 residues are logged and left out (the reference's ``run_tmalign`` gives NaN for a file TM-align fails on)."""
    kept, traces = [], []
    for f in fnames:
        ca = _single_chain_ca(f)
        if ca is None:
            logging.warning(f"{f}: not readable as one model - left out")
        elif len(ca) > ALIGN_MAX_LEN:
            logging.warning(f"{f}: {len(ca)} residues, more than {ALIGN_MAX_LEN} - left out")
        else:
            kept.append(f)
            traces.append(np.asarray(ca, dtype=np.float64))
    return kept, traces


def pairwise_tmscores(fnames: Sequence[str], max_iter: int = 10, device: int = 0, starts=_DEFAULT_STARTS) -> pd.DataFrame:
    """The symmetric table of ``get_pairwise_tmscores`` (bin/hclust_structures.py:38-69): index and columns are the
    files' base names without extension, the diagonal is 1.0, and for k before v in ``fnames`` the score of k aligned
    to v (normalised by v's length) goes on both sides.  ``starts`` as in ``tm_align``."""
    align_start_bits(starts)
    kept, traces = _alignable_files(list(fnames))
    logging.info(f"Computing pairwise distances between {len(kept)} pdb files")
    bnames = [os.path.splitext(os.path.basename(f))[0] for f in kept]
    vals = np.ones((len(kept), len(kept)), dtype=np.float64)
    if len(kept) > 1:
        iu = np.triu_indices(len(kept), k=1)
        tm = pairwise_tm(traces, np.stack(iu, axis=1), max_iter=max_iter, device=device, starts=starts)
        vals[iu] = tm
        vals[(iu[1], iu[0])] = tm
    return pd.DataFrame(vals, index=bnames, columns=bnames)


def training_tm_scores(pdb_files: Sequence[str], train_files: Sequence[str], max_iter: int = 10,
                       device: int = 0, starts=_DEFAULT_STARTS) -> Tuple[dict, dict]:
    """``compute_training_tm_scores`` (bin/tmscore_training.py:22-42) without the files it writes: ({sample name: the
    largest score against the training chains}, {sample name: that training file}).  ``starts`` as in ``tm_align``."""
    align_start_bits(starts)
    samples, q = _alignable_files(list(pdb_files))
    refs, r = _alignable_files(list(train_files))
    if not refs:
        raise ValueError("no usable training structure")
    best, which = max_tm_across_refs(q, r, max_iter=max_iter, device=device, starts=starts) if q else ([], [])
    names = [os.path.splitext(os.path.basename(f))[0] for f in samples]
    return ({k: float(v) for k, v in zip(names, best)}, {k: refs[int(j)] for k, j in zip(names, which)})


# ---------------------------------------------------------------------------------------------------- clashes and lDDT
PAIRCOUNT_MAX_ATOMS = 65536   # FDMI_PAIRCOUNT_MAX_ATOMS
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def _atom_arrays(arrays: Sequence[np.ndarray], per: int, what: str) -> List[np.ndarray]:
    """The structures as float32 arrays, each checked to be [per * n, 3] with n >= 1 and at most 65536 atoms."""
    out = [np.asarray(x, dtype=np.float32) for x in arrays]
    for i, x in enumerate(out):
        if x.ndim != 2 or x.shape[1] != 3 or len(x) == 0 or len(x) % per or len(x) > PAIRCOUNT_MAX_ATOMS:
            raise ValueError(f"{what} {i}: {x.shape}; expected [{per} n, 3] coordinates with n >= 1 and at most "
                             f"{PAIRCOUNT_MAX_ATOMS} atoms")
    return out


def count_clashes(chains: Sequence[np.ndarray], alpha: float = 0.63, device: int = 0, return_flags: bool = False):
    """Van der Waals clashes of every backbone in ``chains`` (each [3 n_i, 3]: N, CA, C per residue), all in one
    ``fd_backbone_clashes`` launch: an int64 array of the number of atoms that clash with at least one other atom --
    ``count_clashes`` (foldingdiff/vdw_clashes.py:34-68) -- and with ``return_flags`` also a list of boolean [3 n_i] arrays,
    True for an atom that clashes.

    Atoms a and b (indices in file order) clash iff |a - b| >= 2 and d(a, b) <= alpha * (r_a + r_b), r = 1.55 for N and
    1.7 for CA and C (DESIGN.md "Clash counts and lDDT").  Unlike the reference, two neighbouring atoms at distance
    exactly 0 do not clash."""
    alpha = float(alpha)
    if not (alpha > 0 and np.isfinite(alpha)):
        raise ValueError(f"alpha={alpha} must be > 0 and finite")
    xs = _atom_arrays(chains, 3, "chain")
    n = len(xs)
    counts = np.zeros((n,), dtype=np.int32)
    if n == 0:
        return (counts.astype(np.int64), []) if return_flags else counts.astype(np.int64)
    xyz, offsets, lens = _pack(xs, np.float32)
    flags = np.empty((len(xyz),), dtype=np.uint8) if return_flags else None
    _binding.check(_binding.load().fd_backbone_clashes(device, ptr(xyz), ptr(offsets // 3), ptr(lens // 3), n, alpha,
                                                       ptr(counts), ptr(flags)))
    if return_flags:
        return counts.astype(np.int64), [flags[o: o + m].astype(bool) for o, m in zip(offsets, lens)]
    return counts.astype(np.int64)


def steer_terms(angles: Union[np.ndarray, Sequence[np.ndarray]], feature_names: Sequence[str], reward=None,
                offset: Optional[np.ndarray] = None, is_angle: Optional[Sequence[bool]] = None, alpha: float = 0.63,
                device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The reward terms of steered sampling (``sampling.steer``) for a batch of backbones given as angles, in one
    ``fd_steer_rewards`` call: float64 ``[B, 4]`` -- the clashing atoms at ``alpha`` (``count_clashes``), the radius of
    gyration of the CA atoms in Angstrom, the helix and the strand fraction (``annotate_sse``) -- and float64 ``[B]``, their
    sum weighted by ``reward`` (a dict over ``sampling.REWARD_TERMS``; default ``{"clashes": -1}``), left to right.

    ``angles``: ``[B, L, F]`` or a list of ``[len_i, F]`` arrays, columns named by ``feature_names`` as for
    ``nerf.build_backbones``.  With ``offset`` (float32 ``[F]``) the values are first shifted by it and the columns of
    ``is_angle`` wrapped to [-pi, pi), as ``sampling.sample`` does with the training mean offset; without, they are taken as
    they are."""
    from . import nerf, sampling
    chains = [np.asarray(a, dtype=np.float32) for a in (angles if not isinstance(angles, np.ndarray) or angles.ndim != 3 else list(angles))]
    F = len(feature_names)
    if not chains or any(c.ndim != 2 or c.shape[1] != F or len(c) == 0 for c in chains):
        raise ValueError(f"each backbone must be [len >= 1, {F}]")
    if offset is not None and is_angle is None:
        raise ValueError("an offset needs is_angle: the columns to wrap after the shift")
    weights = sampling.reward_weights(reward)
    idx = nerf.feature_columns(feature_names)
    B, L = len(chains), max(len(c) for c in chains)
    feats = np.zeros((B, L, F), dtype=np.float32)
    lens = np.array([len(c) for c in chains], dtype=np.int32)
    for i, c in enumerate(chains):
        feats[i, : len(c)] = c
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float32).reshape(-1)
    ang = None if is_angle is None else np.ascontiguousarray(np.asarray(is_angle, dtype=bool).reshape(-1).astype(np.uint8))
    if (off is not None and len(off) != F) or (ang is not None and len(ang) != F):
        raise ValueError(f"offset and is_angle must have {F} entries")
    terms, rew = np.empty((B, 4), dtype=np.float64), np.empty((B,), dtype=np.float64)
    _binding.check(_binding.load().fd_steer_rewards(device, ptr(feats), ptr(lens), B, L, F, ptr(idx), ptr(off), ptr(ang), ptr(weights),
                                                    float(alpha), ptr(terms), ptr(rew)))
    return terms, rew


def count_clashes_parallel(filenames: Sequence[str], nthreads: Optional[int] = None, device: int = 0) -> dict:
    """``count_clashes_parallel`` (foldingdiff/vdw_clashes.py:71-78): {file name: clash count} with the reference's
    default ``alpha``, the files parsed on the host by ``read_backbone`` and counted in one launch.  ``nthreads`` is
    accepted for the reference's signature and ignored.  A file ``read_backbone`` rejects raises ``ValueError``."""
    filenames = list(filenames)
    chains = []
    for f in filenames:
        bb = read_backbone(f)
        if bb is None:
            raise ValueError(f"{f}: not readable as one model with N, CA and C in every residue")
        chains.append(bb[0])
    return {f: int(c) for f, c in zip(filenames, count_clashes(chains, device=device))}


def lddt(models: Sequence[np.ndarray], refs: Sequence[np.ndarray], atoms_per_res: int = 3, radius: float = 15.0,
         thresholds: Sequence[float] = LDDT_THRESHOLDS, per_residue: bool = False, device: int = 0,
         return_counts: bool = False):
    """lDDT (Mariani et al. 2013) of ``models[i]`` against ``refs[i]``, every pair in one ``fd_lddt`` launch: float64
    [len(models)], NaN where no atom pair of the reference is within ``radius`` (a single residue).  Both of a pair are
    [atoms_per_res * n_i, 3] with the same residues and the same atoms per residue in the same order (1 for CA traces, 3
    for N, CA, C backbones; at most 8).

    A pair of atoms of different residues is included iff its distance in the reference is below ``radius``, and
    conserved at a threshold iff its distance in the model differs by less than it; the score is the mean over the
    thresholds of conserved / included (DESIGN.md "Clash counts and lDDT").  These are the defaults of OpenStructure's
    ``compare-structures --lddt``, which the reference runs in a container per pair (foldingdiff/lddt.py:32-56), without
    its stereochemistry checks; the score is not pinned to that binary.

    ``per_residue``: also a list of float64 [n_i] arrays, the same ratio over the included pairs with an atom in the
    residue (NaN where there is none).  ``return_counts``: the integers instead of the ratios -- int64 [len, 2]
    (conserved summed over the thresholds, included) and, with ``per_residue``, a list of int64 [n_i, 2]."""
    A = int(atoms_per_res)
    if not 1 <= A <= 8:
        raise ValueError(f"atoms_per_res={atoms_per_res} outside [1, 8]")
    radius = float(radius)
    if not (radius > 0 and np.isfinite(radius)):
        raise ValueError(f"radius={radius} must be > 0 and finite")
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= 8 or not (np.isfinite(thr) & (thr > 0)).all():
        raise ValueError(f"thresholds={list(thresholds)}: expected 1 to 8 positive finite values")
    if len(models) != len(refs):
        raise ValueError(f"{len(models)} models against {len(refs)} references")
    ms, rs = _atom_arrays(models, A, "model"), _atom_arrays(refs, A, "reference")
    for i, (x, y) in enumerate(zip(ms, rs)):
        if x.shape != y.shape:
            raise ValueError(f"pair {i}: model {x.shape} vs reference {y.shape}; expected the same residues in both")
    n = len(ms)
    counts = np.zeros((n, 2), dtype=np.int64)
    res_counts = []
    if n:
        (M, offsets, lens), R = _pack(ms, np.float32), _pack(rs, np.float32)[0]
        res = np.empty((len(M) // A, 2), dtype=np.int32) if per_residue else None
        _binding.check(_binding.load().fd_lddt(device, ptr(M), ptr(R), ptr(offsets // A), ptr(lens // A), n, A, radius,
                                               ptr(thr), len(thr), ptr(counts), ptr(res)))
        if per_residue:
            res_counts = [res[o: o + m].astype(np.int64) for o, m in zip(offsets // A, lens // A)]
    if return_counts:
        return (counts, res_counts) if per_residue else counts

    def ratio(c):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(c[..., 1] > 0, c[..., 0] / (len(thr) * c[..., 1].astype(np.float64)), np.nan)

    return (ratio(counts), [ratio(c) for c in res_counts]) if per_residue else ratio(counts)


class LddtScorer:
    """A ``scorer=`` for ``sampling.get_reconstruction_error``, shaped like ``TmScorer``: per item (lDDT of
    NeRF(reconstruction) against NeRF(truth), lDDT of NeRF(reconstruction) against the backbone of the item's PDB
    file), over the N, CA and C atoms with the reconstruction as the model.  The file's backbone is compared over the
    residues the item holds (the first ``len`` of them: left-aligned items); an unreadable file, or one shorter than
    the item, scores NaN.  Like the other scorers, the backbones are built from the angles exactly as ``reconstruct``
    returns them.  ``score_batch`` scores all items of a call with one NeRF launch and one lDDT launch."""

    def __init__(self, device: int = 0, radius: float = 15.0, thresholds: Sequence[float] = LDDT_THRESHOLDS):
        self.device, self.radius, self.thresholds = device, radius, tuple(thresholds)

    def __call__(self, reconst_angles, truth_angles, truth_pdb_file: str) -> Tuple[float, float]:
        s, c = self.score_batch([reconst_angles], [truth_angles], [truth_pdb_file])
        return float(s[0]), float(c[0])

    def score_batch(self, recon: Sequence, truth: Sequence, files: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        n = len(recon)
        assert len(truth) == n == len(files)
        if n == 0:
            return np.zeros((0,)), np.zeros((0,))
        recon = [np.asarray(r, dtype=np.float32) for r in recon]
        truth = [np.asarray(t, dtype=np.float32) for t in truth]
        F = recon[0].shape[1]
        names = [v for k, v in datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES.items() if k in DATASETS and len(v) == F]
        assert names, f"no canonical feature set has {F} features"
        xyz = nerf.build_backbones(recon + truth, names[0], device=self.device)
        a, b, which = [], [], []
        for i, f in enumerate(files):
            a.append(xyz[i]); b.append(xyz[n + i]); which.append(("angles", i))
            bb = read_backbone(f) if os.path.isfile(f) else None
            if bb is not None and len(bb[0]) >= len(xyz[i]):
                a.append(xyz[i]); b.append(bb[0][: len(xyz[i])]); which.append(("coords", i))
        r = lddt(a, b, atoms_per_res=3, radius=self.radius, thresholds=self.thresholds, device=self.device)
        scores, coord_scores = np.full(n, np.nan), np.full(n, np.nan)
        for (kind, i), v in zip(which, r):
            (scores if kind == "angles" else coord_scores)[i] = v
        return scores, coord_scores


lddt_scorer = LddtScorer()


def lddt_sampled_folded(sampled_dir: str, folded_dir: str, out_path: str = "lddt.json", device: int = 0) -> dict:
    """``lddt_sampled_folded`` (foldingdiff/lddt.py:59-100): {sampled stem: {folded stem: lDDT}} for every
    ``<sampled_dir>/<stem>.pdb`` and each of its ``<folded_dir>/<stem>_*.pdb``, the folded structure as the model and
    the sampled one as the reference, over N, CA and C; written to ``out_path`` when that is not empty.  All pairs are
    scored in one launch.  A pair that cannot be scored (a file ``read_backbone`` rejects, different residue counts, or
    no atom pair within the radius) gets -1.0, the reference's failure value."""
    sampled = sorted(glob.glob(os.path.join(sampled_dir, "*.pdb")))
    logging.info(f"Found {len(sampled)} sampled structures in {sampled_dir}")
    pairs = []   # (sampled file, folded file)
    for s in sampled:
        stem = os.path.splitext(os.path.basename(s))[0]
        pairs.extend((s, f) for f in sorted(glob.glob(os.path.join(folded_dir, f"{glob.escape(stem)}_*.pdb"))))
    backbones = {}
    for f in {f for pair in pairs for f in pair}:
        try:
            bb = read_backbone(f)
        except (OSError, ValueError) as e:
            logging.error(f"Cannot read {f}: {e}")
            bb = None
        backbones[f] = None if bb is None else bb[0]
    ok = [k for k, (s, f) in enumerate(pairs)
          if backbones[s] is not None and backbones[f] is not None and backbones[s].shape == backbones[f].shape]
    values = [-1.0] * len(pairs)
    scores = lddt([backbones[pairs[k][1]] for k in ok], [backbones[pairs[k][0]] for k in ok], atoms_per_res=3, device=device)
    for k, v in zip(ok, scores):
        if np.isfinite(v):
            values[k] = float(v)
    out: dict = {}
    for (s, f), v in zip(pairs, values):
        if v < 0:
            logging.error(f"Failed to compute lDDT for {f} and {s}")
        out.setdefault(os.path.splitext(os.path.basename(s))[0], {})[os.path.splitext(os.path.basename(f))[0]] = v
    if out_path:
        logging.info(f"Writing lDDT scores to {out_path}")
        with open(out_path, "w") as sink:
            json.dump(out, sink, indent=4)
    return out
