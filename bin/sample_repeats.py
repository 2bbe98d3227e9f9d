#!/usr/bin/env python3
"""
Sample repeat proteins: backbones whose angle rows are tied across the ``--units`` copies of a ``--period``-residue unit,
between free flanks of ``--flank_n`` and ``--flank_c`` residues (sampling.sample_repeats).  The tied rows come
out periodic bit for bit, so the repeat region has exact screw symmetry.  Every backbone has ``flank_n + period * units +
flank_c`` residues.  The model and output arguments are bin/sample.py's:

    <outdir>/model_snapshot/                      copy of the model directory
    <outdir>/sampled_angles/generated_{i}.csv.gz  final angles of every backbone
    <outdir>/sampled_pdb/generated_{i}.pdb        N-CA-C backbones built by NeRF on the device
    <outdir>/repeat_rmsd.json                     the settings and, per backbone, the RMSD (Angstrom, after superposition) of
                                                  all units but the last onto all units but the first (structures.repeat_rmsd)

A tie that cannot exist (a period, a unit count or a flank out of range) is a usage error before the model directory is
looked at; one that does not fit the model's padded length (``max_seq_len`` of its training_args.json) is a usage error
before the model is loaded or anything is written.  The model must be a local directory, as for bin/sample.py.  Single device.
"""
import argparse
import json
import logging
import os
import sys
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEED = 7344   # bin/sample.py's default


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-m", "--model", type=str, required=True,
                        help="Path to model directory: training_args.json, config.json and a models folder at a minimum")
    parser.add_argument("--outdir", "-o", type=str, default=os.getcwd(), help="Path to output directory")
    parser.add_argument("--num", "-n", type=int, default=10, help="Number of backbones to generate")
    parser.add_argument("--period", type=int, required=True, help="residues in one repeat unit")
    parser.add_argument("--units", type=int, required=True, help="copies of the unit (1: nothing is tied)")
    parser.add_argument("--flank_n", type=int, default=0, help="free residues in front of the repeat region")
    parser.add_argument("--flank_c", type=int, default=0, help="free residues behind the repeat region")
    parser.add_argument("--num_steps", type=int, default=None, help="network evaluations per backbone (default: every timestep)")
    parser.add_argument("--eta", type=float, default=1.0, help="noise of the strided update, [0, 1]; 1 = the ancestral update of the respaced chain")
    parser.add_argument("--spacing", type=str, default="uniform", choices=("uniform", "logsnr"), help="how the visits are spaced")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Batch size to use when sampling")
    parser.add_argument("--seed", type=int, default=SEED, help="Random seed")
    parser.add_argument("--device", type=str, default="cuda:0", help="Device to use")
    return parser


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.period < 1 or args.units < 1 or args.flank_n < 0 or args.flank_c < 0 or args.num < 1:
        parser.error(f"--period {args.period} --units {args.units} --flank_n {args.flank_n} --flank_c {args.flank_c} -n {args.num}: "
                     "period, units and n are at least 1, the flanks at least 0")
    length = args.flank_n + args.period * args.units + args.flank_c
    outdir = Path(args.outdir)
    if not os.path.isdir(args.model):
        raise AssertionError(f"{args.model} is not a local model directory")
    with open(Path(args.model) / "training_args.json") as source:
        training_args = json.load(source)
    if length > int(training_args["max_seq_len"]):
        parser.error(f"{args.flank_n} + {args.period} x {args.units} + {args.flank_c} = {length} residues do not fit the model's "
                     f"padded length {training_args['max_seq_len']}")
    if os.path.isdir(outdir) and os.listdir(outdir):
        raise AssertionError(f"Expected {outdir} to be empty!")

    import pandas as pd
    import torch

    from foldingdiff_amd import modelling, sampling, structures
    from foldingdiff_amd.angles_and_coords import write_preds_pdb_folder
    from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset

    train_dset = NoisedAnglesDataset(   # the data-free dataset shell of bin/sample.py
        dset=AnglesEmptyDataset.from_dir(args.model), dset_key="angles", timesteps=training_args["timesteps"], exhaustive_t=False,
        beta_schedule=training_args["variance_schedule"], nonangular_variance=1.0, angular_variance=training_args["variance_scale"])
    os.makedirs(outdir, exist_ok=True)
    device = torch.device(args.device)
    model = modelling.BertForDiffusionBase.from_dir(args.model, copy_to=str(outdir / "model_snapshot")).to(device)
    torch.manual_seed(args.seed)
    lengths = [length] * args.num
    sampled = sampling.sample_repeats(model, train_dset, lengths, args.period, args.units, start=args.flank_n, num_steps=args.num_steps,
                                      eta=args.eta, spacing=args.spacing, batch_size=args.batchsize)
    names = train_dset.feature_names["angles"]
    sampled_dfs = [pd.DataFrame(s, columns=names) for s in sampled]
    sampled_angles_folder = outdir / "sampled_angles"
    os.makedirs(sampled_angles_folder, exist_ok=True)
    logging.info(f"Writing sampled angles to {sampled_angles_folder}")
    for i, s in enumerate(sampled_dfs):
        s.to_csv(sampled_angles_folder / f"generated_{i}.csv.gz")
    coords = []
    pdb_files = write_preds_pdb_folder(sampled_dfs, str(outdir / "sampled_pdb"), device=device.index or 0, coords_out=coords)
    kept = [i for i, (f, xyz) in enumerate(zip(pdb_files, coords)) if f and xyz is not None]
    rmsd = structures.repeat_rmsd([coords[i] for i in kept], args.flank_n, args.period, args.units, device=device.index or 0)
    with open(outdir / "repeat_rmsd.json", "w") as sink:
        json.dump({"settings": vars(args), "length": length,
                   "repeat_rmsd": {os.path.basename(pdb_files[i]): (None if r != r else float(r)) for i, r in zip(kept, rmsd)}}, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
