#!/usr/bin/env python3
"""Golden fixture for the clash count: the reference's own ``count_clashes`` (foldingdiff/vdw_clashes.py:34-68) run on
six backbones.  It needs a checkout of the reference, named by FD_REFERENCE as for make_golden.py (the GPU machines have
none, which is why the output is committed):

    FD_REFERENCE=<reference checkout> python tests/golden/make_golden_clashes.py

biotite is not installable here, so stub modules stand in for it the way make_golden.py stubs it: ``PDBFile.read(name)``
hands the reference an atom array (float32 ``coord``, ``element`` N / C / C per residue) of a backbone held in memory,
and ``filter_backbone`` keeps every atom.  Everything after the read is the reference's code, unchanged.  The per-atom
flags are the reference's too: its module sees numpy through a proxy that records what its ``np.any(is_clash, axis=1)``
returned.

The backbones: 1CRN (tests/golden/1CRN.pdb), 1CRN scaled by 0.8 and by 0.6, 1CRN plus N(0, 1 A) jitter, and two
random-walk chains of 22 and 342 residues (tests/clash_lddt_reference.walk_backbone).

Written: ref_clashes.npz -- names; per backbone float32 xyz_<k> [3n, 3], bool flags_<k> [3n]; int64 counts [6]; alpha.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FD_REFERENCE", "")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

BACKBONES = {}   # name -> float32 [3n, 3]


class _Atoms:
    def __init__(self, coord):
        self.coord = coord
        self.element = np.array(["N", "C", "C"] * (len(coord) // 3))

    def __len__(self):
        return len(self.coord)

    def __getitem__(self, mask):
        assert np.asarray(mask).all()
        return self


class _PDBFile:
    def __init__(self, name):
        self.name = name

    @classmethod
    def read(cls, name):
        return cls(name)

    def get_structure(self):
        return [_Atoms(BACKBONES[self.name])]


class _RecordingNumpy:
    """numpy, except that ``any`` keeps its last result."""

    def __init__(self):
        self.last_any = None

    def __getattr__(self, name):
        return getattr(np, name)

    def any(self, *args, **kwargs):
        self.last_any = np.any(*args, **kwargs)
        return self.last_any


def import_reference():
    for n in ("biotite", "biotite.structure", "biotite.structure.io", "biotite.structure.io.pdb"):
        sys.modules[n] = types.ModuleType(n)
    sys.modules["biotite.structure.io.pdb"].PDBFile = _PDBFile
    sys.modules["biotite.structure"].filter_backbone = lambda atoms: np.ones(len(atoms), dtype=bool)
    sys.modules["biotite"].structure = sys.modules["biotite.structure"]
    assert os.path.isfile(os.path.join(REF, "foldingdiff", "vdw_clashes.py")), "set FD_REFERENCE to the reference checkout"
    sys.path.insert(0, REF)
    from foldingdiff import vdw_clashes
    return vdw_clashes


def main():
    import clash_lddt_reference as cr
    from foldingdiff_amd import structures

    crn = structures.read_backbone(os.path.join(HERE, "1CRN.pdb"))[0]
    rng = np.random.default_rng(20240607)
    BACKBONES["1CRN"] = crn
    BACKBONES["1CRN_x0.8"] = (crn * np.float32(0.8)).astype(np.float32)
    BACKBONES["1CRN_x0.6"] = (crn * np.float32(0.6)).astype(np.float32)
    BACKBONES["1CRN_jitter"] = (crn.astype(np.float64) + rng.standard_normal(crn.shape)).astype(np.float32)
    BACKBONES["walk_22"] = cr.walk_backbone(rng, 22)
    BACKBONES["walk_342"] = cr.walk_backbone(rng, 342)

    vdw = import_reference()
    rec = vdw.np = _RecordingNumpy()
    out = {"names": np.array(list(BACKBONES)), "alpha": np.float64(0.63)}
    counts = []
    for k, (name, xyz) in enumerate(BACKBONES.items()):
        n = int(vdw.count_clashes(name))
        flags = np.asarray(rec.last_any, dtype=bool)
        assert flags.shape == (len(xyz),) and int(flags.sum()) == n
        mine, my_flags, margin = cr.clashes(xyz)
        print(f"{name}: {len(xyz) // 3} residues, reference count {n}, restatement {mine}, margin {margin:.3g}")
        assert margin >= cr.MIN_MARGIN
        counts.append(n)
        out[f"xyz_{k}"] = xyz
        out[f"flags_{k}"] = flags
    out["counts"] = np.array(counts, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "ref_clashes.npz"), **out)


if __name__ == "__main__":
    main()
