#!/usr/bin/env python3
"""
The denoising loss of a trained model over PDB structures on MI355X: the numbers the reference's validation_step and
validation_epoch_end log while training (val_loss, val_loss_<feature>), for a fixed checkpoint.

    bin/validation_loss.py MODEL_DIR PDBS... [--timesteps-curve N] [--loss l1] [--circle-reg X] [--pdist-loss ...] [-o out.json]

The structures are read and featurised as bin/partial_noise_reconstruct.py does (the model directory's training
arguments: feature set, padding, minimum length, schedule, training means) and wrapped in the model's noise schedule.
Each item is noised once at a random timestep (the reference's random stream under --seed); forward and loss run as one
device call per batch.  With --timesteps-curve N the loss is also evaluated with every item at each of N evenly spaced
timesteps ("curve": {"timesteps": [...], "loss": [[F floats] per timestep]}), the standard diagnostic of a diffusion
model.  The loss is the one the model was trained with, as its training_args.json says: "loss" (smooth_l1, wrapped
for angular features, or l1), "circle_reg" (the circle penalty) and "use_pdist_loss" (the pairwise-distance loss, a
weight or MIN MAX TIMESTEPS; it adds val_loss_pairwise_dist_loss and one more value to val_loss).  --loss, --circle-reg
and --pdist-loss override what the directory says.

The model must be a local directory (no hub download): training_args.json, config.json, models/ and
training_mean_offset.npy.
"""
import argparse
import json
import logging
import os
import sys
from pathlib import Path

BIN = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(BIN)
for p in (REPO, BIN):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import modelling, validation  # noqa: E402
from partial_noise_reconstruct import load_dataset  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("model", type=str, help="Local model directory")
    parser.add_argument("pdb_files", nargs="+", help="PDB files to evaluate on (.pdb or .pdb.gz)")
    parser.add_argument("--timesteps-curve", type=int, default=0, metavar="N",
                        help="also evaluate the loss at N evenly spaced timesteps (default: 0 = no curve)")
    parser.add_argument("--loss", type=str, default=None, choices=["smooth_l1", "l1", "radian_l1_smooth"],
                        help="Loss to report (default: the model directory's)")
    parser.add_argument("--circle-reg", type=float, default=None, help="Circle penalty (default: the model directory's)")
    parser.add_argument("--pdist-loss", type=float, nargs="+", default=None, metavar="X",
                        help="Pairwise-distance loss: one weight, or MIN MAX TIMESTEPS; 0 turns it off (default: the model directory's)")
    parser.add_argument("-b", "--batch-size", type=int, default=512, help="Structures per device call (default: 512)")
    parser.add_argument("--seed", type=int, default=6489, help="Seed of the noising (default: 6489)")
    parser.add_argument("-d", "--device", type=int, default=0, help="GPU to use (default: 0)")
    parser.add_argument("-o", "--output-json", type=str, default=None, help="Output JSON file (default: print)")
    return parser


def loss_settings(net, dset, loss=None, circle_reg=None, pdist_loss=None) -> dict:
    """Apply the command line's overrides to what from_dir found, and name the features for the pairwise term."""
    if pdist_loss is not None:
        if len(pdist_loss) not in (1, 3):
            raise ValueError("--pdist-loss takes one weight, or MIN MAX TIMESTEPS")
        pdist_loss = float(pdist_loss[0]) if len(pdist_loss) == 1 else (float(pdist_loss[0]), float(pdist_loss[1]), int(pdist_loss[2]))
    net.set_loss(net.loss_key if loss is None else loss, net.circle_lambda if circle_reg is None else circle_reg,
                 net.use_pairwise_dist_loss if pdist_loss is None else pdist_loss)
    net.ft_names = list(dset.feature_names[dset.dset_key])
    return {"loss": net.loss_key, "circle_reg": net.circle_lambda, "use_pdist_loss": net.use_pairwise_dist_loss}


def evaluate(model_dir: str, pdb_files, timesteps_curve: int = 0, batch_size: int = 512, seed: int = 6489, device: int = 0,
             loss=None, circle_reg=None, pdist_loss=None):
    assert os.path.isdir(model_dir), f"Model path {model_dir} is not a local directory"
    dset = load_dataset(pdb_files, Path(model_dir))
    net = modelling.BertForDiffusionBase.from_dir(model_dir).to(torch.device(f"cuda:{device}"))
    settings = loss_settings(net, dset, loss, circle_reg, pdist_loss)
    torch.manual_seed(seed)
    out = {"model": model_dir, "n_structures": len(dset), "seed": seed, **settings}
    out.update(validation.validation_loss(net, dset, batch_size=batch_size))
    logging.info(f"val_loss over {len(dset)} structures: {out['val_loss']:.4f}")
    if timesteps_curve > 0:
        ts = np.unique(np.linspace(0, dset.timesteps - 1, timesteps_curve).round().astype(int))
        curve = validation.loss_by_timestep(net, dset, ts.tolist(), batch_size=batch_size, seed=seed)
        features = list(dset.feature_names[dset.dset_key])
        if curve.shape[1] > len(features):
            features.append(validation.PAIRWISE_NAME)
        out["curve"] = {"timesteps": ts.tolist(), "features": features, "loss": curve.tolist()}
    return out


def main():
    args = build_parser().parse_args()
    out = evaluate(args.model, args.pdb_files, timesteps_curve=args.timesteps_curve, batch_size=args.batch_size,
                   seed=args.seed, device=args.device, loss=args.loss, circle_reg=args.circle_reg, pdist_loss=args.pdist_loss)
    if args.output_json:
        with open(args.output_json, "w") as sink:
            json.dump(out, sink, indent=4)
    else:
        print(json.dumps(out, indent=4))


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
