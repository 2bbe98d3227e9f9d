#!/usr/bin/env python3
"""
lDDT between each sampled structure and its folded structures on MI355X -- stand-in for running the reference's
foldingdiff/lddt.py as a script (same positional arguments):

    python bin/lddt.py <sampled_dir> <folded_dir> [-o lddt.json]

Every <sampled_dir>/<stem>.pdb is paired with every <folded_dir>/<stem>_*.pdb, the folded structure as the model and the
sampled one as the reference, and the JSON {sampled stem: {folded stem: lDDT}} is written (default: lddt.json in the
working directory, like the reference).  The score is structures.lddt over the N, CA and C atoms (inclusion radius 15 A,
thresholds 0.5, 1, 2 and 4 A, no stereochemistry checks) in place of an OpenStructure container per pair; all pairs are
scored in one device launch.  A pair that cannot be scored -- an unreadable file, different residue counts, a single
residue -- gets -1.0, the reference's failure value.
"""
import argparse
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from foldingdiff_amd import structures  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("sampled_dir", type=str, help="directory of sampled structures (*.pdb)")
    parser.add_argument("folded_dir", type=str, help="directory of their folded structures (<stem>_*.pdb)")
    parser.add_argument("-o", "--output", type=str, default="lddt.json", help="output JSON file (default: lddt.json)")
    parser.add_argument("-d", "--device", type=int, default=0, help="GPU to use (default: 0)")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    structures.lddt_sampled_folded(args.sampled_dir, args.folded_dir, out_path=args.output, device=args.device)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
