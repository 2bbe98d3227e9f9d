#!/usr/bin/env python3
"""
Add the carbonyl oxygens to N-CA-C backbones on MI355X -- stand-in for the reference's bin/add_oxygen_to_backbone.py
(same positional arguments): some downstream tools (PyMOL, ProteinMPNN's featuriser, DSSP) want O.

    python bin/add_oxygen_to_backbone.py sampled_pdb sampled_pdb_with_o

Every ``*.pdb`` of the input directory (or the one input file) is read, side chains and any oxygens it holds are
discarded, the oxygens of all files are placed in one launch (foldingdiff_amd.structures.add_oxygens) and each backbone is
written under its own name into ``outdir`` with four atoms per residue, every residue renamed GLY as the reference does.
The last residue has no psi and gets no oxygen, as in the reference.

The oxygen sits trans to the next residue's N (torsion psi + pi).  The reference's script passes psi itself, which puts
the oxygen where the next N is; --reference_torsion reproduces that for whoever must match its files.  Files with
several models, without backbone atoms or of more than 1024 residues are skipped with a log line.
"""
import argparse
import glob
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from foldingdiff_amd import structures  # noqa: E402
from foldingdiff_amd.angles_and_coords import write_backbone_with_o_pdb  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("input", type=str, help="Input file, or directory with .pdb files")
    parser.add_argument("outdir", type=str, help="Output directory to write .pdb files")
    parser.add_argument("--reference_torsion", action="store_true",
                        help="place O at the torsion psi, as the reference's script does, instead of psi + pi")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if os.path.isdir(args.input):
        pdb_files = sorted(glob.glob(os.path.join(args.input, "*.pdb")))
        logging.info(f"Found {len(pdb_files)} pdb files in {args.input}")
    elif os.path.isfile(args.input):
        pdb_files = [args.input]
    else:
        raise ValueError(f"Invalid input: {args.input}")
    os.makedirs(args.outdir, exist_ok=True)
    kept = []
    for fname in pdb_files:
        bb = structures.read_backbone(fname)
        if bb is None or len(bb[1]) > structures.DSSP_MAX_LEN:
            logging.warning(f"{fname}: rejected by the parser or longer than {structures.DSSP_MAX_LEN} residues - skipping")
            continue
        kept.append((fname, bb[0]))
    with_o = structures.add_oxygens([xyz for _, xyz in kept], reference_torsion=args.reference_torsion)
    for (fname, _), coords4 in zip(kept, with_o):
        write_backbone_with_o_pdb(coords4, os.path.join(args.outdir, os.path.basename(fname)))


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
