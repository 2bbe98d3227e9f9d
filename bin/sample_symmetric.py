#!/usr/bin/env python3
"""
Sample subunits of cyclic homo-oligomers: every backbone is scored, behind every visit, against its own ``--order`` copies about
an axis -- soft clashes between copies, a CA contact reward, a weak pull to the axis -- while a rigid pose relative to the axis
is carried through the run, and is docked rigidly (``--dock_iters`` steps) at the end (sampling.sample_symmetric).
The model and output arguments are bin/sample.py's:

    <outdir>/model_snapshot/                       copy of the model directory
    <outdir>/sampled_angles/generated_{i}.csv.gz   final angles of every monomer
    <outdir>/assembly_pdb/generated_{i}.pdb        the oligomer: one chain per copy (A, B, ...), N-CA-C backbones
    <outdir>/symmetry.json                         the settings and, per sample, the pose (Q row-major, then t), the energies
                                                   clash | contact | radial per subunit and the inter-copy CA contacts

A length that does not fit the model's padded length (``max_seq_len`` of its training_args.json) or an order outside [2, 12] is
a usage error before the model is loaded or anything is written.  The model must be a local directory, as for bin/sample.py.
Single device.  Backbone-only repulsion and a contact reward are no force field: nothing is claimed about the interfaces.
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
    parser.add_argument("--num", "-n", type=int, default=10, help="Number of subunits to generate")
    parser.add_argument("-l", "--length", type=int, required=True, help="residues in one subunit")
    parser.add_argument("--order", type=int, default=3, help="copies about the axis, 2 to 12")
    parser.add_argument("--num_steps", type=int, default=None, help="network evaluations per backbone (default: every timestep)")
    parser.add_argument("--eta", type=float, default=1.0, help="noise of the strided update, [0, 1]; 1 = the ancestral update of the respaced chain")
    parser.add_argument("--scale", type=float, default=1.0, help="strength of the guidance")
    parser.add_argument("--pose_iters", type=int, default=1, help="rigid-body steps of the pose behind every visit")
    parser.add_argument("--dock_iters", type=int, default=100, help="rigid-body steps of the final docking")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Batch size to use when sampling")
    parser.add_argument("--seed", type=int, default=SEED, help="Random seed")
    parser.add_argument("--device", type=str, default="cuda:0", help="Device to use")
    return parser


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.length < 1 or args.num < 1 or not 2 <= args.order <= 12 or args.dock_iters < 0 or args.pose_iters < 0:
        parser.error(f"-l {args.length} -n {args.num} --order {args.order} --dock_iters {args.dock_iters} --pose_iters {args.pose_iters}: "
                     "length and n are at least 1, the order lies in [2, 12], the iteration counts are at least 0")
    outdir = Path(args.outdir)
    if not os.path.isdir(args.model):
        raise AssertionError(f"{args.model} is not a local model directory")
    with open(Path(args.model) / "training_args.json") as source:
        training_args = json.load(source)
    if args.length > int(training_args["max_seq_len"]):
        parser.error(f"{args.length} residues do not fit the model's padded length {training_args['max_seq_len']}")
    if os.path.isdir(outdir) and os.listdir(outdir):
        raise AssertionError(f"Expected {outdir} to be empty!")

    import pandas as pd
    import torch

    from foldingdiff_amd import modelling, nerf, sampling, structures
    from foldingdiff_amd.angles_and_coords import write_assembly_pdb
    from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset

    train_dset = NoisedAnglesDataset(   # the data-free dataset shell of bin/sample.py
        dset=AnglesEmptyDataset.from_dir(args.model), dset_key="angles", timesteps=training_args["timesteps"], exhaustive_t=False,
        beta_schedule=training_args["variance_schedule"], nonangular_variance=1.0, angular_variance=training_args["variance_scale"])
    os.makedirs(outdir, exist_ok=True)
    device = torch.device(args.device)
    model = modelling.BertForDiffusionBase.from_dir(args.model, copy_to=str(outdir / "model_snapshot")).to(device)
    torch.manual_seed(args.seed)
    res = sampling.sample_symmetric(model, train_dset, [args.length] * args.num, order=args.order, num_steps=args.num_steps, scale=args.scale,
                                    symmetry_params=structures.symmetry_params(pose_iters=args.pose_iters), dock_iters=args.dock_iters,
                                    eta=args.eta, batch_size=args.batchsize, device=device.index or 0)
    names = list(train_dset.feature_names["angles"])
    sampled_angles_folder = outdir / "sampled_angles"
    os.makedirs(sampled_angles_folder, exist_ok=True)
    logging.info(f"Writing sampled angles to {sampled_angles_folder}")
    for i, s in enumerate(res.angles):
        pd.DataFrame(s, columns=names).to_csv(sampled_angles_folder / f"generated_{i}.csv.gz")
    pdb_folder = outdir / "assembly_pdb"
    os.makedirs(pdb_folder, exist_ok=True)
    backbones = nerf.build_backbones(res.angles, names, center_coords=False, device=device.index or 0, method="scan")
    report = {}
    for i, xyz in enumerate(backbones):
        write_assembly_pdb(structures.cyclic_assembly(xyz, res.pose[i], args.order), str(pdb_folder / f"generated_{i}.pdb"))
        report[f"generated_{i}.pdb"] = {"pose": [float(v) for v in res.pose[i]], "energy": [float(v) for v in res.energy[i]],
                                        "contacts": int(res.contacts[i])}
    with open(outdir / "symmetry.json", "w") as sink:
        json.dump({"settings": vars(args), "energy_terms": ["clash", "contact", "radial"], "samples": report}, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
