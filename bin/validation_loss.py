#!/usr/bin/env python3
"""
The denoising loss of a trained model over PDB structures on MI355X: the numbers the reference's validation_step and
validation_epoch_end log while training (val_loss, val_loss_<feature>), for a fixed checkpoint.

    bin/validation_loss.py MODEL_DIR PDBS... [--timesteps-curve N] [-o out.json]

The structures are read and featurised as bin/partial_noise_reconstruct.py does (the model directory's training
arguments: feature set, padding, minimum length, schedule, training means) and wrapped in the model's noise schedule.
Each item is noised once at a random timestep (the reference's random stream under --seed); forward and loss run as one
device call per batch.  With --timesteps-curve N the loss is also evaluated with every item at each of N evenly spaced
timesteps ("curve": {"timesteps": [...], "loss": [[F floats] per timestep]}), the standard diagnostic of a diffusion
model.  Loss: smooth L1 (wrapped for angular features), as bin/train.py's default; the pairwise-distance loss and the
circle penalty are not built.

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
    parser.add_argument("-b", "--batch-size", type=int, default=512, help="Structures per device call (default: 512)")
    parser.add_argument("--seed", type=int, default=6489, help="Seed of the noising (default: 6489)")
    parser.add_argument("-d", "--device", type=int, default=0, help="GPU to use (default: 0)")
    parser.add_argument("-o", "--output-json", type=str, default=None, help="Output JSON file (default: print)")
    return parser


def evaluate(model_dir: str, pdb_files, timesteps_curve: int = 0, batch_size: int = 512, seed: int = 6489, device: int = 0):
    assert os.path.isdir(model_dir), f"Model path {model_dir} is not a local directory"
    dset = load_dataset(pdb_files, Path(model_dir))
    net = modelling.BertForDiffusionBase.from_dir(model_dir).to(torch.device(f"cuda:{device}"))
    torch.manual_seed(seed)
    out = {"model": model_dir, "n_structures": len(dset), "seed": seed}
    out.update(validation.validation_loss(net, dset, batch_size=batch_size))
    logging.info(f"val_loss over {len(dset)} structures: {out['val_loss']:.4f}")
    if timesteps_curve > 0:
        ts = np.unique(np.linspace(0, dset.timesteps - 1, timesteps_curve).round().astype(int))
        curve = validation.loss_by_timestep(net, dset, ts.tolist(), batch_size=batch_size, seed=seed)
        out["curve"] = {"timesteps": ts.tolist(), "features": list(dset.feature_names[dset.dset_key]), "loss": curve.tolist()}
    return out


def main():
    args = build_parser().parse_args()
    out = evaluate(args.model, args.pdb_files, timesteps_curve=args.timesteps_curve, batch_size=args.batch_size,
                   seed=args.seed, device=args.device)
    if args.output_json:
        with open(args.output_json, "w") as sink:
            json.dump(out, sink, indent=4)
    else:
        print(json.dumps(out, indent=4))


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
