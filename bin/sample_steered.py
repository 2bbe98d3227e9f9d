#!/usr/bin/env python3
"""
Sample protein backbones steered toward a reward, without gradients: ``--particles`` particles per backbone run the noisy
few-step sampler together and are resampled on the device in proportion to ``exp(lam * (reward now - reward before))`` of
their predicted clean structure (sampling.steer).  The model and output arguments are bin/sample.py's:

    <outdir>/model_snapshot/                      copy of the model directory
    <outdir>/sampled_angles/generated_{i}.csv.gz  final angles of every returned backbone
    <outdir>/sampled_pdb/generated_{i}.pdb        N-CA-C backbones built by NeRF on the device
    <outdir>/steering.json                        the settings, the events, and per sample its reward terms (clashing atoms,
                                                  radius of gyration, helix and strand fraction), reward and particle index

The reward is ``w_clashes * clashes + w_rg * rg + w_helix * helix + w_strand * strand``; the default asks for backbones
without clashing atoms.  The model must be a local directory, as for bin/sample.py.  Single device.
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

import pandas as pd  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import modelling, sampling  # noqa: E402
from foldingdiff_amd.angles_and_coords import write_preds_pdb_folder  # noqa: E402
from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset  # noqa: E402

SEED = 7344   # bin/sample.py's default


def build_datasets(model_dir: Path) -> NoisedAnglesDataset:
    """The data-free dataset shell of bin/sample.py."""
    with open(model_dir / "training_args.json") as source:
        training_args = json.load(source)
    dset = AnglesEmptyDataset.from_dir(str(model_dir))
    return NoisedAnglesDataset(
        dset=dset,
        dset_key="coords" if training_args["angles_definitions"] == "cart-coords" else "angles",
        timesteps=training_args["timesteps"],
        exhaustive_t=False,
        beta_schedule=training_args["variance_schedule"],
        nonangular_variance=1.0,
        angular_variance=training_args["variance_scale"],
    )


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-m", "--model", type=str, required=True,
                        help="Path to model directory: training_args.json, config.json and a models folder at a minimum")
    parser.add_argument("--outdir", "-o", type=str, default=os.getcwd(), help="Path to output directory")
    parser.add_argument("--num", "-n", type=int, default=10, help="Number of backbones to generate *per length*")
    parser.add_argument("-l", "--lengths", type=int, nargs=2, default=[50, 128], help="Range of lengths to sample from")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Particles per call")
    parser.add_argument("--particles", type=int, default=8, help="particles per backbone")
    parser.add_argument("--lam", type=float, default=1.0, help="the tilt: the run samples from p(x) exp(lam * reward(x))")
    parser.add_argument("--ess_frac", type=float, default=0.5,
                        help="an event resamples when the effective sample size falls below this share of the particles (1: always, 0: never)")
    parser.add_argument("--steer_from", type=int, default=None, help="events follow the visits with t below this (default: T // 2)")
    parser.add_argument("--every", type=int, default=1, help="... every this many of them")
    parser.add_argument("--w_clashes", type=float, default=-1.0, help="weight of the number of clashing backbone atoms")
    parser.add_argument("--w_rg", type=float, default=0.0, help="weight of the radius of gyration of the CA atoms (Angstrom)")
    parser.add_argument("--w_helix", type=float, default=0.0, help="weight of the helix fraction (P-SEA)")
    parser.add_argument("--w_strand", type=float, default=0.0, help="weight of the strand fraction (P-SEA)")
    parser.add_argument("--num_steps", type=int, default=None, help="network evaluations per particle (default: every timestep)")
    parser.add_argument("--eta", type=float, default=1.0, help="noise of the strided update, (0, 1]; 1 = the ancestral update of the respaced chain")
    parser.add_argument("--all", action="store_true", help="write every particle, not the best of each backbone")
    parser.add_argument("--seed", type=int, default=SEED, help="Random seed")
    parser.add_argument("--device", type=str, default="cuda:0", help="Device to use")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    outdir = Path(args.outdir)
    if not os.path.isdir(args.model):
        raise AssertionError(f"{args.model} is not a local model directory (there is no network access here)")
    if os.path.isdir(outdir) and os.listdir(outdir):
        raise AssertionError(f"Expected {outdir} to be empty!")
    os.makedirs(outdir, exist_ok=True)
    train_dset = build_datasets(Path(args.model))
    model = modelling.BertForDiffusionBase.from_dir(args.model, copy_to=str(outdir / "model_snapshot")).to(torch.device(args.device))
    lo, hi = args.lengths
    assert lo < hi <= train_dset.dset.pad
    lengths = [l for l in range(lo, hi) for _ in range(args.num)]
    reward = {"clashes": args.w_clashes, "rg": args.w_rg, "helix": args.w_helix, "strand": args.w_strand}
    torch.manual_seed(args.seed)
    sampled, info = sampling.steer(model, train_dset, lengths, n_particles=args.particles, reward=reward, lam=args.lam, ess_frac=args.ess_frac,
                                   steer_from=args.steer_from, every=args.every, num_steps=args.num_steps, eta=args.eta,
                                   select="all" if args.all else "best", seed=args.seed, batch_size=args.batchsize)
    names = train_dset.feature_names["angles"]
    sampled_dfs = [pd.DataFrame(s, columns=names) for s in sampled]
    sampled_angles_folder = outdir / "sampled_angles"
    os.makedirs(sampled_angles_folder, exist_ok=True)
    logging.info(f"Writing sampled angles to {sampled_angles_folder}")
    for i, s in enumerate(sampled_dfs):
        s.to_csv(sampled_angles_folder / f"generated_{i}.csv.gz")
    write_preds_pdb_folder(sampled_dfs, str(outdir / "sampled_pdb"))
    with open(outdir / "steering.json", "w") as sink:
        json.dump({"settings": vars(args), "reward_terms": list(sampling.REWARD_TERMS), "visits": info["visits"].tolist(),
                   "events": info["events"].tolist(),
                   "samples": {f"generated_{i}": {"length": int(len(s)), "terms": info["terms"][i].tolist(), "reward": float(info["reward"][i]),
                                                  "particle": int(info["index"][i])} for i, s in enumerate(sampled)}}, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
