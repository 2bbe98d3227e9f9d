#!/usr/bin/env python3
"""
Partially noise PDB structures and reconstruct them with a trained model on MI355X -- stand-in for the reference's
bin/partial_noise_reconstruct.py (same positional arguments and flags).

The structures are read and featurised by foldingdiff_amd.structures (one device launch for all files), forward-noised
to t = --timesteps and denoised again on the device, and every reconstruction is scored with the backbone RMSD after
optimal superposition (Angstrom, lower is better).  The output JSON holds

    {"timesteps": T, "model": DIR, "rmsd": {file: RMSD of NeRF(reconstruction) to NeRF(original angles)},
     "rmsd_coord": {file: RMSD of NeRF(reconstruction) to the file's own backbone}}

With --tmscore the same reconstructions are also scored by TM-score (structures.tm_scorer: CA traces, the published
TM-score search on the device in place of the external TM-align binary; higher is better, 1 = identical), under the
reference's key and one for the file's own backbone:

     "tmscores": {file: TM-score of NeRF(reconstruction) to NeRF(original angles)},
     "tmscores_coord": {file: TM-score of NeRF(reconstruction) to the file's CA atoms, normalised by its length}

With --lddt they are also scored by lDDT (structures.lddt_scorer: N, CA and C atoms, the reconstruction as the model;
higher is better, 1 = every local distance kept):

     "lddt": {file: lDDT of NeRF(reconstruction) against NeRF(original angles)},
     "lddt_coord": {file: lDDT of NeRF(reconstruction) against the file's own backbone}

The model must be a local directory (no hub download): training_args.json, config.json, models/ and
training_mean_offset.npy.  Files the parser rejects (several models, a residue without N / CA / C, angles out of
range) or that are shorter than the model's min_seq_len are left out of the output.
"""
import argparse
import json
import logging
import os
import sys
from pathlib import Path
from typing import Collection, Dict, Optional, Tuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import datasets, modelling, sampling, structures  # noqa: E402


def load_dataset(pdb_files: Collection[str], model_dir: Path) -> datasets.NoisedAnglesDataset:
    """The reference's load_dataset: the clean dataset class of the model's feature set, padded and filtered like its
    training data, centred with the training means, wrapped in the model's noise schedule."""
    logging.info(f"Loading dataset from {len(pdb_files)} pdb files")
    with open(model_dir / "training_args.json") as source:
        training_args = json.load(source)
    key = training_args["angles_definitions"]
    if key not in structures.DATASETS:
        raise NotImplementedError(f"angles_definitions={key!r}: only the canonical angle feature sets are supported")
    dset = structures.DATASETS[key](
        pdbs=list(pdb_files),
        split=None,
        pad=training_args["max_seq_len"],
        min_length=training_args.get("min_seq_len", 0),   # bin/train.py's default
        trim_strategy="leftalign",
        zero_center=True,  # the offset is replaced by the training one just below
    )
    dset.set_masked_means(np.load(model_dir / "training_mean_offset.npy"))
    return datasets.NoisedAnglesDataset(
        dset,
        dset_key="angles",
        timesteps=training_args["timesteps"],
        beta_schedule=training_args["variance_schedule"],
        nonangular_variance=1.0,
        angular_variance=training_args["variance_scale"],
    )


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("pdb_files", nargs="+", help="PDB files to reconstruct (.pdb or .pdb.gz)")
    parser.add_argument("output_json", type=str, help="Output JSON file")
    parser.add_argument("-t", "--timesteps", type=int, default=800, help="Timesteps of noise to add (default: 800)")
    parser.add_argument("-m", "--model", type=str, required=True, help="Local model directory")
    parser.add_argument("-d", "--device", type=int, default=0, help="GPU to use (default: 0)")
    parser.add_argument("--tmscore", action="store_true",
                        help='also write TM-scores ("tmscores", "tmscores_coord") of the same reconstructions')
    parser.add_argument("--lddt", action="store_true", help='also write lDDT scores ("lddt", "lddt_coord") of the same reconstructions')
    parser.add_argument("--num_steps", type=int, default=None,
                        help="denoise in this many network evaluations on a strided schedule with the DDIM update (default: every timestep)")
    parser.add_argument("--eta", type=float, default=0.0, help="with --num_steps: 0 = DDIM .. 1 = the ancestral update of the respaced chain")
    parser.add_argument("--solver", type=str, default=None, choices=["ddim", "dpm2m"],
                        help="with --num_steps: the update of a visit, ddim (default) or dpm2m, a second-order multistep solver (needs --eta 0)")
    parser.add_argument("--spacing", type=str, default=None, choices=["uniform", "logsnr"],
                        help="with --num_steps: visits spaced evenly in t (default) or in log-SNR")
    parser.add_argument("--lambda_min", type=float, default=None,
                        help="with --spacing logsnr: the log-SNR below which the visits are not spread (default: the library's, -3)")
    return parser


FEW_STEP_FLAGS = ("solver", "spacing", "lambda_min")   # passed on, and recorded, only when given


def get_reconstruction_error(pdb_files: Collection[str], timesteps: int, model: str, device: int = 0,
                             num_steps: Optional[int] = None, eta: float = 0.0, **few_step) -> Tuple[Dict[str, float], Dict[str, float]]:
    """(RMSD to the original angles' backbone, RMSD to the file's backbone) per file that entered the dataset."""
    assert os.path.isdir(model), f"Model path {model} is not a local directory"
    dset = load_dataset(pdb_files, Path(model))
    net = modelling.BertForDiffusionBase.from_dir(model).to(torch.device(f"cuda:{device}"))
    scores, coord_scores = sampling.get_reconstruction_error(net, dset=dset, noise_timesteps=timesteps,
                                                             scorer=structures.RmsdScorer(device=device), num_steps=num_steps, eta=eta,
                                                             **few_step)
    files = dset.filenames   # the dataset's (shuffled) order, which the scores follow
    logging.info(f"Reconstruction RMSD from t={timesteps}: {np.min(scores):.3f}-{np.max(scores):.3f} A")
    return ({f: float(s) for f, s in zip(files, scores)}, {f: float(s) for f, s in zip(files, coord_scores)})


def get_reconstruction_scores(pdb_files: Collection[str], timesteps: int, model: str, device: int = 0,
                              tmscore: bool = True, lddt: bool = False, num_steps: Optional[int] = None,
                              eta: float = 0.0, **few_step) -> Dict[str, Dict[str, float]]:
    """One reconstruction per file, scored by the RMSD scorer and the chosen others: {"rmsd", "rmsd_coord" [, "tmscores",
    "tmscores_coord"] [, "lddt", "lddt_coord"]}, each {file: score} over the files that entered the dataset."""
    assert os.path.isdir(model), f"Model path {model} is not a local directory"
    dset = load_dataset(pdb_files, Path(model))
    net = modelling.BertForDiffusionBase.from_dir(model).to(torch.device(f"cuda:{device}"))
    recon, truth, files = sampling.reconstruct(net, dset, noise_timesteps=timesteps, num_steps=num_steps, eta=eta, **few_step)
    out = {}
    scorers = [("rmsd", structures.RmsdScorer(device=device))]
    if tmscore:
        scorers.append(("tmscores", structures.TmScorer(device=device)))
    if lddt:
        scorers.append(("lddt", structures.LddtScorer(device=device)))
    for key, scorer in scorers:
        scores, coord_scores = scorer.score_batch(recon, truth, files)
        out[key] = {f: float(s) for f, s in zip(files, scores)}
        out[f"{key}_coord"] = {f: float(s) for f, s in zip(files, coord_scores)}
    for key in ("tmscores", "lddt"):
        if key in out:
            logging.info(f"Reconstruction {key} from t={timesteps}: {min(out[key].values()):.3f}-{max(out[key].values()):.3f}")
    return out


def main():
    args = build_parser().parse_args()
    few_step = {k: getattr(args, k) for k in FEW_STEP_FLAGS if getattr(args, k) is not None}
    strided = {} if args.num_steps is None else {"num_steps": args.num_steps, "eta": args.eta, **few_step}
    if args.tmscore or args.lddt:
        scores = get_reconstruction_scores(args.pdb_files, timesteps=args.timesteps, model=args.model, device=args.device,
                                           tmscore=args.tmscore, lddt=args.lddt, num_steps=args.num_steps, eta=args.eta, **few_step)
        with open(args.output_json, "w") as sink:
            json.dump({"timesteps": args.timesteps, "model": args.model, **strided, **scores}, sink, indent=4)
        return
    rmsd, rmsd_coord = get_reconstruction_error(args.pdb_files, timesteps=args.timesteps, model=args.model, device=args.device,
                                                num_steps=args.num_steps, eta=args.eta, **few_step)
    with open(args.output_json, "w") as sink:
        json.dump({"timesteps": args.timesteps, "model": args.model, **strided, "rmsd": rmsd, "rmsd_coord": rmsd_coord}, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
