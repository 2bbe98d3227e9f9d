"""structures.py on the host: the PDB parser rules and the dataset semantics of CathCanonicalAnglesDataset
(foldingdiff/datasets.py:75-566) with the device featurisation replaced by fixed arrays.  No GPU needed."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from foldingdiff_amd import angles_and_coords, datasets, structures

CANON = ["0C:1N", "N:CA", "CA:C", "phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]


def _atom(serial, name, resn, chain, resseq, xyz, rec="ATOM", alt=" ", icode=" "):
    x, y, z = xyz
    line = f"{rec:<6}{serial:>5} {name:<4}{alt}{resn:>3} {chain}{resseq:>4}{icode}   {x:>8.3f}{y:>8.3f}{z:>8.3f}  1.00  0.00"
    return line + f"           {name[0]:>1}  "


def _residue(serial, resn, chain, resseq, base, rec="ATOM", icode=" ", names=("N", "CA", "C", "O")):
    return [_atom(serial + k, n, resn, chain, resseq, (base + k, base + 0.5 * k, -base), rec=rec, icode=icode)
            for k, n in enumerate(names)]


def _write(tmp_path, name, lines):
    p = tmp_path / name
    p.write_text("\n".join(lines + ["END"]) + "\n")
    return str(p)


def test_reads_n_ca_c_in_file_order(tmp_path):
    f = _write(tmp_path, "two.pdb", ["HEADER    TEST"] + _residue(1, "GLY", "A", 1, 1.0) + _residue(5, "ALA", "A", 2, 10.0))
    xyz, ids = structures.read_backbone(f)
    assert xyz.dtype == np.float32 and xyz.shape == (6, 3)
    assert ids == [("A", "1", ""), ("A", "2", "")]
    # N, CA, C of residue 1, then of residue 2; O is not part of the backbone
    want = np.array([[1, 1, -1], [2, 1.5, -1], [3, 2, -1], [10, 10, -10], [11, 10.5, -10], [12, 11, -10]], np.float32)
    assert np.array_equal(xyz, want)
    ca = structures.extract_backbone_coords(f)
    assert np.array_equal(ca, want[1::3]) and ca.dtype == np.float32
    assert np.array_equal(structures.extract_backbone_coords(f, atoms=["N", "C"]), want[[0, 2, 3, 5]])


def test_multi_model_is_rejected(tmp_path):
    res = _residue(1, "GLY", "A", 1, 1.0) + _residue(5, "ALA", "A", 2, 10.0)
    f = _write(tmp_path, "nmr.pdb", ["MODEL        1"] + res + ["ENDMDL", "MODEL        2"] + res + ["ENDMDL"])
    assert structures.read_backbone(f) is None
    assert structures.extract_backbone_coords(f) is None
    # one MODEL record is a single structure
    g = _write(tmp_path, "one.pdb", ["MODEL        1"] + res + ["ENDMDL"])
    assert structures.read_backbone(g)[0].shape == (6, 3)
    # a rejected file never reaches the device: no launch for an empty batch
    assert structures.featurize([f]) == [None]


def test_first_alternate_location_wins(tmp_path):
    lines = _residue(1, "GLY", "A", 1, 1.0)
    lines += [_atom(5, "N", "SER", "A", 2, (20, 0, 0), alt="B"),
              _atom(6, "N", "SER", "A", 2, (30, 0, 0), alt="A"),
              _atom(7, "CA", "SER", "A", 2, (21, 0, 0), alt="A"),
              _atom(8, "CA", "SER", "A", 2, (31, 0, 0), alt="B"),
              _atom(9, "C", "SER", "A", 2, (22, 0, 0))]
    xyz, ids = structures.read_backbone(_write(tmp_path, "alt.pdb", lines))
    assert len(ids) == 2
    assert np.array_equal(xyz[3:, 0], [20, 21, 22])   # the first record of each atom, whatever its altloc letter


def test_hetatm_mse_kept_other_hetatm_skipped(tmp_path):
    lines = (_residue(1, "GLY", "A", 1, 1.0) + _residue(5, "MSE", "A", 2, 10.0, rec="HETATM")
             + _residue(9, "LIG", "A", 3, 20.0, rec="HETATM") + _residue(13, "HOH", "A", 4, 30.0, rec="HETATM", names=("O",)))
    xyz, ids = structures.read_backbone(_write(tmp_path, "het.pdb", lines))
    assert ids == [("A", "1", ""), ("A", "2", "")]
    assert np.array_equal(xyz[3:, 0], [10, 11, 12])


def test_insertion_codes_are_separate_residues(tmp_path):
    lines = (_residue(1, "GLY", "A", 52, 1.0) + _residue(5, "ALA", "A", 52, 10.0, icode="A")
             + _residue(9, "SER", "A", 53, 20.0))
    xyz, ids = structures.read_backbone(_write(tmp_path, "ins.pdb", lines))
    assert ids == [("A", "52", ""), ("A", "52", "A"), ("A", "53", "")]
    assert np.array_equal(xyz[:, 0], [1, 2, 3, 10, 11, 12, 20, 21, 22])


def test_chains_concatenated_in_file_order(tmp_path):
    lines = _residue(1, "GLY", "B", 1, 1.0) + ["TER"] + _residue(5, "ALA", "A", 1, 10.0)
    xyz, ids = structures.read_backbone(_write(tmp_path, "ch.pdb", lines))
    assert ids == [("B", "1", ""), ("A", "1", "")]
    assert np.array_equal(xyz[:, 0], [1, 2, 3, 10, 11, 12])


def test_missing_backbone_atom_rejects_the_file(tmp_path, caplog):
    lines = _residue(1, "GLY", "A", 1, 1.0) + _residue(5, "ALA", "A", 2, 10.0, names=("N", "CA", "O"))
    f = _write(tmp_path, "gap.pdb", lines)
    with caplog.at_level("DEBUG"):
        assert structures.read_backbone(f) is None
    assert "lacks ['C']" in caplog.text
    assert structures.featurize([f]) == [None]
    assert structures.read_backbone(_write(tmp_path, "empty.pdb", ["HEADER    NOTHING"])) is None


def test_gzip_reads_like_plain(tmp_path):
    lines = _residue(1, "GLY", "A", 1, 1.0) + _residue(5, "ALA", "A", 2, 10.0)
    f = _write(tmp_path, "p.pdb", lines)
    g = str(tmp_path / "p.pdb.gz")
    with gzip.open(g, "wt") as fh:
        fh.write(open(f).read())
    a, b = structures.read_backbone(f), structures.read_backbone(g)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_fixture_files_parse():
    xyz, ids = structures.read_backbone(os.path.join(GOLDEN, "1CRN.pdb"))
    assert xyz.shape == (46 * 3, 3) and ids[0] == ("A", "1", "") and ids[-1] == ("A", "46", "")
    assert np.array_equal(xyz[0], np.array([17.047, 14.099, 3.625], np.float32))   # N of THR 1 (nerf.py's seed)
    xyz, ids = structures.read_backbone(os.path.join(GOLDEN, "all_residues.pdb"))
    assert xyz.shape == (20 * 3, 3) and ids[0] == ("A", "0", "") and ids[-1] == ("A", "19", "")


def test_feature_names_and_reexport():
    assert angles_and_coords.canonical_distances_and_dihedrals is structures.canonical_distances_and_dihedrals
    assert structures.CANONICAL == CANON
    with pytest.raises(ValueError):
        structures.featurize([], distances=["CA:CB"], angles=["phi"])
    with pytest.raises(ValueError):
        structures.featurize([], distances=[], angles=["chi1"])


# ---------------------------------------------------------------------------------------------------- datasets
def _fake_frame(n, seed):
    """Nine-column features of an n-residue chain with the reference's NaN / 0 padding."""
    rng = np.random.default_rng(seed)
    v = np.empty((n, 9), np.float32)
    v[:, :3] = rng.uniform(1.2, 1.6, (n, 3))
    v[:, 3:] = rng.uniform(-np.pi, np.pi, (n, 6))
    v[0, 0] = 6.0   # a long C-N distance (a chain break): minus its mean it lies beyond pi
    v[0, 3] = np.nan
    v[-1, :3] = 0.0
    v[-1, 4:] = np.nan
    return pd.DataFrame(v, columns=CANON)


def _make(tmp_path, lengths, **kw):
    files = []
    for i, n in enumerate(lengths):
        p = tmp_path / f"s{i:02d}.pdb"
        p.write_text("")
        files.append(str(p))
    table = {f: (_fake_frame(n, i), np.full((n, 3), float(i), np.float32)) for i, (f, n) in enumerate(zip(files, lengths))}
    calls = []

    def featurizer(fnames):
        calls.append(list(fnames))
        return [table[f] for f in fnames]

    cls = kw.pop("cls", structures.PdbAnglesDataset)
    kw.setdefault("min_length", 0)
    ds = cls(kw.pop("pdbs", files), featurizer=featurizer, **kw)
    assert len(calls) == 1   # every file in one featurizer call
    return ds, files, table


def test_seeded_shuffle_even_without_split(tmp_path):
    ds, files, _ = _make(tmp_path, [5 + i for i in range(10)], pad=32)
    # np.random.default_rng(6489).shuffle of ten items
    order = [2, 0, 6, 3, 9, 5, 4, 7, 8, 1]
    assert ds.filenames == [files[i] for i in order]
    assert ds.all_lengths == [5 + i for i in order]
    # a directory gives the same files (sorted) and so the same order
    ds2, _, _ = _make(tmp_path, [5 + i for i in range(10)], pad=32, pdbs=str(tmp_path))
    assert ds2.filenames == ds.filenames


def test_split_sizes(tmp_path):
    order = [2, 0, 6, 3, 9, 5, 4, 7, 8, 1]
    parts = {}
    for split in ("train", "validation", "test"):
        ds, files, _ = _make(tmp_path, [5 + i for i in range(10)], pad=32, split=split)
        parts[split] = ds.filenames
    assert parts["train"] == [files[i] for i in order[:8]]
    assert parts["validation"] == [files[order[8]]] and parts["test"] == [files[order[9]]]
    with pytest.raises(ValueError):
        _make(tmp_path, [5] * 3, pad=32, split="holdout")
    # 25 items: int(20), int(2.5) = 2, the remaining 3
    sizes = [len(_make(tmp_path, [5] * 25, pad=32, split=s)[0]) for s in ("train", "validation", "test")]
    assert sizes == [20, 2, 3]


def test_min_length_then_discard_or_leftalign(tmp_path):
    lengths = [3, 10, 20, 40, 41]
    ds, files, _ = _make(tmp_path, lengths, pad=40, min_length=10, trim_strategy="discard")
    assert sorted(ds.all_lengths) == [10, 20, 40]   # 3 below min_length, 41 above pad
    ds, files, _ = _make(tmp_path, lengths, pad=40, min_length=10, trim_strategy="leftalign")
    assert sorted(ds.all_lengths) == [10, 20, 40, 41]
    i = ds.filenames.index(files[4])
    it = ds[i]
    assert int(it["lengths"]) == 40 and it["angles"].shape == (40, 9) and it["attn_mask"].sum() == 40
    with pytest.raises(AssertionError):
        _make(tmp_path, lengths, pad=10, min_length=10)
    with pytest.raises(NotImplementedError):
        _make(tmp_path, lengths, pad=40, trim_strategy="randomcrop")


def test_circular_means_over_all_nine_columns(tmp_path):
    ds, files, table = _make(tmp_path, [7, 12, 9], pad=16)
    concat = np.concatenate([table[f][0].values for f in files]).astype(np.float64)
    want = np.array([np.arctan2(np.nanmean(np.sin(c)), np.nanmean(np.cos(c))) for c in concat.T])
    got = ds.get_masked_means()
    assert got.shape == (9,) and np.abs(got - want).max() <= 1e-6
    # the distance columns get the circular mean too, not the arithmetic one
    d = concat[:, 0][~np.isnan(concat[:, 0])]
    assert abs(got[0] - np.arctan2(np.sin(d).mean(), np.cos(d).mean())) <= 1e-6
    assert abs(got[0] - d.mean()) > 1e-3
    assert structures.PdbAnglesDataset(files, min_length=0, pad=16, zero_center=False,
                                       featurizer=lambda fn: [table[f] for f in fn]).get_masked_means() is None


def test_item_centring_wrap_nan_padding_keys(tmp_path):
    ds, files, table = _make(tmp_path, [7, 12, 9], pad=16)
    m = ds.get_masked_means().astype(np.float64)
    for idx, f in enumerate(ds.filenames):
        raw = table[f][0].values.astype(np.float64)
        n = len(raw)
        it = ds[idx]
        assert set(it) == {"angles", "coords", "attn_mask", "position_ids", "lengths"}
        assert it["angles"].dtype == torch.float32 and it["angles"].shape == (16, 9)
        assert it["coords"].dtype == torch.float32 and it["coords"].shape == (16, 3)
        assert it["attn_mask"].dtype == torch.float32 and it["attn_mask"].tolist() == [1.0] * n + [0.0] * (16 - n)
        assert it["position_ids"].dtype == torch.int64 and it["position_ids"].tolist() == list(range(16))
        assert it["lengths"].dtype == torch.int64 and it["lengths"].ndim == 0 and int(it["lengths"]) == n
        a = it["angles"].numpy().astype(np.float64)
        want = raw - m
        want[:, 3:] = (want[:, 3:] + np.pi) % (2 * np.pi) - np.pi   # only the angular columns are wrapped
        want = np.nan_to_num(want, nan=0.0)
        assert np.abs(a[:n] - want).max() <= 1e-5
        assert np.all(a[n:] == 0.0)
        assert a[0, 3] == 0.0 and np.all(a[n - 1, 4:] == 0.0)   # the NaN padding of phi / the last row -> 0
        assert np.abs(a[:, 3:]).max() <= np.pi + 1e-6
        # a distance minus its (circular) mean is not wrapped
        assert a[0, 0] > np.pi and abs(a[0, 0] - (6.0 - m[0])) <= 1e-6
        assert np.array_equal(it["coords"].numpy()[:n], table[f][1]) and np.all(it["coords"].numpy()[n:] == 0)
    raw_item = ds.__getitem__(0, ignore_zero_center=True)["angles"].numpy()
    n0 = ds.all_lengths[0]
    assert np.array_equal(raw_item[:n0], np.nan_to_num(table[ds.filenames[0]][0].values, nan=0.0))
    with pytest.raises(IndexError):
        ds[3]


def test_angle_subsets_and_masked_means(tmp_path):
    full, files, table = _make(tmp_path, [7, 12, 9], pad=16)
    for cls, key in ((structures.PdbAnglesOnlyDataset, "canonical-full-angles"),
                     (structures.PdbMinimalAnglesDataset, "canonical-minimal-angles")):
        names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES[key]
        ds, _, _ = _make(tmp_path, [7, 12, 9], pad=16, cls=cls)
        assert ds.feature_names["angles"] == names and ds.feature_is_angular["angles"] == [True] * len(names)
        idx = [CANON.index(n) for n in names]
        assert np.array_equal(ds.get_masked_means(), full.get_masked_means()[idx])
        assert torch.equal(ds[1]["angles"], full[1]["angles"][:, idx])
        offset = np.linspace(-1.0, 1.0, len(names)).astype(np.float32)
        ds.set_masked_means(offset)
        assert np.allclose(ds.get_masked_means(), offset)
        assert np.allclose(ds.means[:3], full.means[:3])   # the other columns keep theirs
        raw = table[ds.filenames[1]][0].values[:, idx].astype(np.float64)
        want = np.nan_to_num((raw - offset + np.pi) % (2 * np.pi) - np.pi, nan=0.0)
        n = len(raw)
        assert np.abs(ds[1]["angles"].numpy()[:n] - want).max() <= 1e-5
    assert structures.DATASETS["canonical-full-angles"] is structures.PdbAnglesOnlyDataset


def test_works_inside_noised_dataset(tmp_path):
    ds, files, _ = _make(tmp_path, [7, 12, 9], pad=16, cls=structures.PdbAnglesOnlyDataset)
    noised = datasets.NoisedAnglesDataset(ds, dset_key="angles", timesteps=10, beta_schedule="cosine")
    assert noised.filenames == ds.filenames and noised.pad == 16 and len(noised) == 3
    torch.manual_seed(0)
    it = noised.__getitem__(2, use_t_val=5)
    assert it["corrupted"].shape == (16, 6) and int(it["t"]) == 5
    assert torch.equal(it["angles"], ds[2]["angles"])
    assert noised.sample_length() in ds.all_lengths


def test_internal_coords_kernels_use_no_scratch(tmp_path):
    """Both kernels of internal_coords.hip compile for gfx950 without scratch (the 4x4 Jacobi stays in registers)."""
    import re
    import subprocess
    from foldingdiff_amd import build as fbuild
    out = tmp_path / "internal_coords.s"
    cmd = [fbuild.find_hipcc(), "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-S", "--cuda-device-only",
           "-o", str(out), os.path.join(fbuild.CSRC, "internal_coords.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    found = set()
    for kernel in ("internal_coords_kernel", "superpose_rmsd_kernel"):
        m = re.search(r"\.name:\s+(\S*" + kernel + r"\S*)\n(.*?)\.wavefront_size", asm, re.S)
        assert m, kernel
        md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(2))}
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (kernel, md)
        found.add(kernel)
    assert "scratch_" not in asm and len(found) == 2
