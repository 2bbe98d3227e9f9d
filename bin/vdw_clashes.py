#!/usr/bin/env python3
"""
Count the van der Waals clashes of PDB backbones on MI355X -- stand-in for running the reference's
foldingdiff/vdw_clashes.py as a script (same arguments):

    python bin/vdw_clashes.py <pdb file1> <pdb file2> ... [--json FILE]

Prints the mean clash count of the files, as the reference does.  A clash count is the number of N / CA / C atoms within
0.63 (r_a + r_b) of an atom at least two positions away in the file (structures.count_clashes); all files are counted in
one device launch.  With --json the counts are also written as {file: count}.  A file that cannot be read as one model
with N, CA and C in every residue ends the run with an error that names it.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from foldingdiff_amd import structures  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("pdb_files", nargs="+", help="PDB files (.pdb or .pdb.gz)")
    parser.add_argument("--json", type=str, default="", help="also write {file: count} to this JSON file")
    parser.add_argument("-d", "--device", type=int, default=0, help="GPU to use (default: 0)")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    clashes_counts = structures.count_clashes_parallel(args.pdb_files, device=args.device)
    if args.json:
        with open(args.json, "w") as sink:
            json.dump(clashes_counts, sink, indent=4)
    print(np.mean(list(clashes_counts.values())))


if __name__ == "__main__":
    main()
