#!/usr/bin/env python3
"""
Compute the maximum TM score of generated structures against a training set on MI355X -- stand-in for the reference's
bin/tmscore_training.py (same -d / -n arguments).

Every generated backbone is aligned to every training chain by foldingdiff_amd.structures.max_tm_across_refs (the
TM-align-style search restated on the device in place of one TMalign subprocess per pair), normalised by the training
chain's length.  Writes tm_scores.json ({sample name: best score}) and tm_scores_ref.json ({sample name: the best
matching training file}) into the directory of generated structures, like compute_training_tm_scores, and
tm_scores_settings.json ({"starts": ...}; the keys of the other two are the sample names).

--starts all searches every pair from all five of TM-align's starts instead of two (fd_tm_align_ex): slower, never a
lower score, so never a higher novelty.

What differs: the training set is named with --train (a directory of .pdb / .pdb.gz files, or a text file listing one
path per line); the reference builds the CATH training split, whose data pipeline is not here.  Files that cannot be
read as one model, and chains of more than 512 residues, are logged and left out.
"""
import argparse
import json
import logging
import os
import re
import sys
from glob import glob
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from foldingdiff_amd import structures  # noqa: E402


STARTS = {"two": ("threading", "ss"), "all": "all"}


def training_files(train: str):
    if os.path.isdir(train):
        return sorted(glob(os.path.join(train, "*.pdb")) + glob(os.path.join(train, "*.pdb.gz")))
    with open(train) as source:
        return [line.strip() for line in source if line.strip()]


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-d", "--dirname", type=str, default=os.path.join(os.getcwd(), "sampled_pdb"),
                        help="Directory of generated PDB structures")
    parser.add_argument("-n", "--nsubset", type=int, default=0, help="Take only first n hits, 0 ignore")
    parser.add_argument("--train", type=str, required=True,
                        help="Training structures: a directory of PDB files, or a file listing one PDB path per line")
    parser.add_argument("--device", type=int, default=0, help="GPU index")
    parser.add_argument("--starts", choices=sorted(STARTS), default="two",
                        help="Starts of the alignment search: two (threading, secondary structure) or all five")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    assert os.path.isdir(args.dirname), args.dirname
    generated = glob(os.path.join(args.dirname, "*.pdb"))
    generated = sorted(generated, key=lambda x: tuple(int(i) for i in re.findall(r"[0-9]+", os.path.basename(x))))
    assert generated, f"{args.dirname} does not contain any pdb files"
    logging.info(f"Found {len(generated)} generated structures")
    if args.nsubset > 0:
        logging.info(f"Subsetting to the first {args.nsubset} pdb files")
        generated = generated[: args.nsubset]
    train = training_files(args.train)
    assert train, f"{args.train} names no training structures"
    logging.info(f"Calculating tm scores against {len(train)} training structures...")
    scores, refs = structures.training_tm_scores(generated, train, device=args.device, starts=STARTS[args.starts])
    outdir = Path(args.dirname)
    with open(outdir / "tm_scores_settings.json", "w") as sink:
        json.dump({"starts": args.starts}, sink, indent=4)
    with open(outdir / "tm_scores.json", "w") as sink:
        json.dump(scores, sink, indent=4)
    with open(outdir / "tm_scores_ref.json", "w") as sink:
        json.dump(refs, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
