#!/usr/bin/env python3
"""
Sample protein backbones from a trained autoregressive baseline model on MI355X -- stand-in for the reference's
``bin/sample_autoregressive.py`` (same arguments, same files):

    <outdir>/model_snapshot/                      copy of the model directory (from_dir(copy_to=...))
    <outdir>/sampled_angles/generated_{i}.csv.gz  angles of every sampled backbone
    <outdir>/sampled_pdb/generated_{i}.pdb        N-CA-C backbones built by NeRF on the device

For every length in ``--lengths`` (half-open, as the reference's ``range``) one ``sample`` call generates ``--num``
backbones from the same ``--num`` seeds: the first ``--num_angles`` residues of structures drawn from ``--seed_pdbs``
(the reference hard-wires ``../data/cath/dompdb``; here the directory is an argument, and its files are taken in sorted
order).  The model must be a local directory: training_args.json, config.json, models/best_by_valid/*.ckpt and
training_mean_offset.npy.
"""
import argparse
import logging
import os
import sys
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import modelling, structures, utils  # noqa: E402
from foldingdiff_amd.angles_and_coords import write_preds_pdb_folder  # noqa: E402


def sample_initial_angles(n_samples: int, n_angles: int = 4, eps: float = 1e-4, seed=1234, pdb_dir="",
                          featurizer=None) -> torch.Tensor:
    """Initial angles of naturally occurring proteins (bin/sample_autoregressive.py:20-52): [n_samples, n_angles, 6], the
    first ``n_angles`` residues (phi, psi, omega, tau, CA:C:1N, C:1N:1CA) of ``n_samples`` files of ``pdb_dir`` drawn with
    ``default_rng(seed).integers``; with ``eps`` Gaussian noise of that scale is added under ``torch.manual_seed(seed)``.
    ``featurizer(fname) -> DataFrame`` defaults to ``structures.canonical_distances_and_dihedrals`` (on the device)."""
    pdb_files = sorted(p for p in Path(pdb_dir).glob("*") if p.is_file())
    assert pdb_files, f"no files in {pdb_dir}"
    logging.info(f"Sampling from {len(pdb_files)} PDB files")
    if featurizer is None:
        def featurizer(fname):
            return structures.canonical_distances_and_dihedrals(
                str(fname), angles=structures.EXHAUSTIVE_ANGLES, distances=structures.MINIMAL_DISTS)
    retval = torch.zeros((n_samples, n_angles, 6))
    rng = np.random.default_rng(seed)
    for i, idx in enumerate(rng.integers(0, len(pdb_files), n_samples)):
        angles = featurizer(pdb_files[idx])
        assert angles is not None, f"Error when parsing {pdb_files[idx]}"
        retval[i, :, :] = torch.from_numpy(np.asarray(angles.values[:n_angles, :], dtype=np.float32))
    if eps:
        logging.info(f"Adding noise zero means and variance {eps} to angles")
        torch.manual_seed(seed)
        retval += torch.randn((n_samples, n_angles, 6)) * eps
    return utils.modulo_with_wrapped_range(retval, -np.pi, np.pi)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("model", help="Model name or path", type=str)
    parser.add_argument("-o", "--outdir", help="Output directory", default=".")
    parser.add_argument("--num", default=10, type=int, help="Number of samples at each length from 50-128")
    parser.add_argument("--num_angles", help="Number of angles to sample as seed angles", type=int, default=4)
    parser.add_argument("-l", "--lengths", type=int, nargs=2, default=[50, 128], help="Range of lengths to sample from")
    parser.add_argument("-d", "--device", type=str, default="cuda:0", help="Device to run generations on")
    parser.add_argument("--seed_pdbs", type=str, required=True,
                        help="Directory of PDB files the seed angles are drawn from (the reference reads data/cath/dompdb)")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    outdir = Path(args.outdir).absolute()
    assert os.path.isdir(args.model), f"{args.model} is not a local model directory (there is no network access here)"
    logging.info(f"Creating {outdir}")
    os.makedirs(outdir, exist_ok=True)
    assert not os.listdir(outdir), f"Expected {outdir} to be empty"

    device = torch.device(args.device)
    m = modelling.BertForAutoregressiveBase.from_dir(args.model, copy_to=str(outdir / "model_snapshot")).to(device)
    angle_offsets = np.load(Path(args.model) / "training_mean_offset.npy")

    # the seeds, shifted by the same amount the training data was shifted
    initial_angles = sample_initial_angles(args.num, args.num_angles, eps=0.0, pdb_dir=args.seed_pdbs)
    initial_angles = utils.modulo_with_wrapped_range(initial_angles - torch.from_numpy(angle_offsets))
    initial_angles = torch.nan_to_num(initial_angles, nan=0.0)

    sampled_angles_dir = outdir / "sampled_angles"
    os.makedirs(sampled_angles_dir, exist_ok=False)
    pad = 128  # (the reference's seed tensor: torch.zeros((num, 128, 6)))
    sampled_angles = []
    for n in range(args.lengths[0], args.lengths[1]):
        seed_values = torch.zeros((args.num, pad, 6))
        seed_values[:, : args.num_angles, :] = initial_angles
        s = m.sample(seed_angles=seed_values, seq_lengths=torch.tensor([n for _ in range(args.num)]),
                     num_seed=args.num_angles, pbar=False)
        sampled_angles.extend(
            pd.DataFrame(utils.modulo_with_wrapped_range(vals.cpu().numpy() + angle_offsets, -np.pi, np.pi),
                         columns=structures.EXHAUSTIVE_ANGLES)
            for vals in s)

    for i, s in enumerate(sampled_angles):
        s.to_csv(sampled_angles_dir / f"generated_{i}.csv.gz")
    written = write_preds_pdb_folder(sampled_angles, str(outdir / "sampled_pdb"), device=device.index or 0)
    assert all(written), "a sampled backbone held NaN coordinates"


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
