#!/usr/bin/env python3
"""
Motif-conditioned sampling on MI355X: keep a segment of an existing structure and generate the rest of the chain around
it (sampling.scaffold: the motif's angle rows are held fixed by replacement inside the update kernel).  The reference has
no such script; the flags and the output tree follow bin/sample.py:

    <outdir>/sampled_angles/scaffold_{i}.csv.gz   final angles of every generated backbone
    <outdir>/sampled_pdb/scaffold_{i}.pdb         N-CA-C backbones built by NeRF on the device
    <outdir>/motif_rmsd.json                      {scaffold_{i}.pdb: {"offset", "motif_rmsd", "pdb_rmsd"}}:
                                                  where the motif sits, the N/CA/C RMSD of those residues against the
                                                  motif's own NeRF-built backbone (structures.motif_rmsd; zero up to
                                                  float32 rounding) and against the coordinates of the PDB file itself
                                                  (nonzero for real structures: NeRF's bond lengths are constants)

--motif_residues LO HI are 0-based residue indices into the file's parsed backbone, HI exclusive.  One backbone is
generated per length in range(*--lengths), --num times.  Single device; the model must be a local directory, as for
bin/sample.py.  --jump_length J --n_resample R (both off by default) run a resampling schedule: the run goes
back up J noise levels and comes down again, R descents per stretch.  --num_steps K [--eta E] runs the conditioned chain in K
network evaluations on a strided schedule with the DDIM update; --jump_length then counts visits.  Whether the scaffolds are designable is not measured here: nothing in this repository folds a sequence.
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

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import modelling, sampling, structures  # noqa: E402
from foldingdiff_amd.angles_and_coords import write_preds_pdb_folder  # noqa: E402
from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset  # noqa: E402

SEED = 7344   # bin/sample.py's default


def build_datasets(model_dir: Path) -> NoisedAnglesDataset:
    """bin/sample.py's data-free dataset shell."""
    with open(model_dir / "training_args.json") as source:
        training_args = json.load(source)
    if training_args["angles_definitions"] == "cart-coords":
        raise NotImplementedError("a motif is a set of internal-angle rows: cart-coords models have none")
    return NoisedAnglesDataset(
        dset=AnglesEmptyDataset.from_dir(str(model_dir)), dset_key="angles", timesteps=training_args["timesteps"],
        exhaustive_t=False, beta_schedule=training_args["variance_schedule"], nonangular_variance=1.0,
        angular_variance=training_args["variance_scale"])


def placement(value: str):
    """--placement: center | random | a residue index."""
    if value in ("center", "random"):
        return value
    try:
        return int(value)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{value!r}: expected center, random or an integer")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-m", "--model", type=str, required=True,
                        help="Path to model directory: training_args.json, config.json and a models folder at a minimum")
    parser.add_argument("--motif", type=str, required=True, help="PDB file that holds the motif")
    parser.add_argument("--motif_residues", type=int, nargs=2, required=True, metavar=("LO", "HI"),
                        help="0-based residues LO .. HI-1 of the file's backbone are the motif")
    parser.add_argument("-l", "--lengths", type=int, nargs=2, default=[50, 128], help="Range of total lengths (upper bound exclusive)")
    parser.add_argument("--num", "-n", type=int, default=1, help="Number of scaffolds to generate *per length*")
    parser.add_argument("--placement", type=placement, default="center",
                        help="where the motif's first residue goes: center, random (numpy's generator, seeded by --seed) or an index")
    parser.add_argument("--jump_length", type=int, default=None,
                        help="resampling: noise levels to go back up at every jump (default: off, the plain descent)")
    parser.add_argument("--n_resample", type=int, default=1, help="resampling: descents per stretch of --jump_length levels (1: off)")
    parser.add_argument("--num_steps", type=int, default=None,
                        help="few-step sampling: network evaluations per descent on a strided schedule (default: every timestep)")
    parser.add_argument("--eta", type=float, default=0.0, help="few-step sampling: 0 = DDIM (deterministic), 1 = ancestral; needs --num_steps")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Batch size to use when sampling")
    parser.add_argument("--outdir", "-o", type=str, default=os.getcwd(), help="Path to output directory")
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
    device = torch.device(args.device)
    device_index = device.index or 0
    train_dset = build_datasets(Path(args.model))
    names = train_dset.feature_names["angles"]
    feats = structures.featurize([args.motif], distances=[n for n in names if n.count(":") == 1],
                                 angles=[n for n in names if n.count(":") != 1], device=device_index)[0]
    if feats is None:
        raise AssertionError(f"{args.motif}: no usable backbone")
    lo, hi = args.motif_residues
    if not 0 <= lo < hi <= len(feats):
        raise AssertionError(f"--motif_residues {lo} {hi}: the file has {len(feats)} residues")
    motif = feats[names].values[lo:hi].astype(np.float32)
    if not np.isfinite(motif).all():
        raise AssertionError(f"residues {lo} .. {hi - 1} of {args.motif} hold an undefined angle (a chain end?)")
    len_lo, len_hi = args.lengths
    assert hi - lo <= len_lo < len_hi <= train_dset.pad, f"lengths {len_lo} .. {len_hi} with a motif of {hi - lo} and a pad of {train_dset.pad}"
    lengths = [l for l in range(len_lo, len_hi) for _ in range(args.num)]
    os.makedirs(outdir, exist_ok=True)
    model = modelling.BertForDiffusionBase.from_dir(args.model).to(device)

    torch.manual_seed(args.seed)
    np.random.seed(args.seed % (2 ** 32))
    offsets = {"center": None, "random": "random"}.get(args.placement, args.placement)
    resample = {}
    n_visits = train_dset.timesteps
    if args.num_steps is not None:
        resample = dict(num_steps=args.num_steps, eta=args.eta)
        n_visits = args.num_steps
    elif args.eta != 0.0:
        raise AssertionError("--eta applies to a strided run: give --num_steps")
    if args.jump_length is not None and args.n_resample > 1:
        resample.update(jump_length=args.jump_length, n_resample=args.n_resample)
        n_visits = len(sampling.resample_schedule(n_visits - 1, args.jump_length, args.n_resample))   # (as many as over a grid of K)
    logging.info(f"{len(lengths)} chains, {n_visits} reverse steps (visits) per chain over {train_dset.timesteps} timesteps")
    sampled, offsets = sampling.scaffold(model, train_dset, motif, lengths, offsets=offsets, batch_size=args.batchsize, **resample)

    sampled_dfs = [pd.DataFrame(s, columns=names) for s in sampled]
    angles_dir = outdir / "sampled_angles"
    os.makedirs(angles_dir, exist_ok=True)
    for i, df in enumerate(sampled_dfs):
        df.to_csv(angles_dir / f"scaffold_{i}.csv.gz")
    coords = []
    pdb_files = write_preds_pdb_folder(sampled_dfs, str(outdir / "sampled_pdb"), basename_prefix="scaffold_", device=device_index,
                                       coords_out=coords)
    kept = [i for i, (f, xyz) in enumerate(zip(pdb_files, coords)) if f and xyz is not None]
    file_backbone = structures.read_backbone(args.motif)[0].reshape(-1, 3)[3 * lo: 3 * hi]
    # the motif's own backbone: behind a lead-in row, or, where it starts the chain, from NeRF's seed residue
    r_own = np.zeros(len(kept))
    for start in (False, True):
        sel = [j for j, i in enumerate(kept) if (offsets[i] == 0) == start]
        if sel:
            own = structures.motif_backbone(motif, names, at_chain_start=start, device=device_index)
            r_own[sel] = structures.motif_rmsd([coords[kept[j]] for j in sel], own, [offsets[kept[j]] for j in sel], device=device_index)
    r_pdb = structures.motif_rmsd([coords[i] for i in kept], file_backbone, [offsets[i] for i in kept], device=device_index)
    report = {os.path.basename(pdb_files[i]): {"offset": int(offsets[i]), "motif_rmsd": float(a), "pdb_rmsd": float(b)}
              for i, a, b in zip(kept, r_own, r_pdb)}
    with open(outdir / "motif_rmsd.json", "w") as sink:
        json.dump(report, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
