#!/usr/bin/env python3
"""
Count the secondary structures of PDB files as determined by P-SEA on MI355X -- stand-in for the reference's
bin/annot_secondary_structures.py (same positional arguments and flags).

The CA trace of every file is annotated by foldingdiff_amd.structures.annotate_sse (the P-SEA algorithm restated on the
device in place of biotite's annotate_sse, all files in one launch), the helices and strands of each are counted, and
the 2-D histogram of the counts is written to the PDF (skipped with a log line when matplotlib is missing).  With
--json the counts are also written as {file name: [n_alpha, n_beta]}.  Files with several models are left out.

What is NOT here: --backend dssp (there is no DSSP binary here), and a single training_args.json as input, which
stands for the CATH test split of that model (it needs the CATH data pipeline).  Both raise.  --threads is accepted
for compatibility; the device annotates every file at once.
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
    parser.add_argument("infiles", type=str, nargs="+", help="PDB files to compute secondary structures for")
    parser.add_argument("outpdf", type=str, help="PDF file to write plot of secondary structure co-occurrence frequencies")
    parser.add_argument("--backend", type=str, choices=["dssp", "psea"], default="psea",
                        help="Backend for calculating secondary structure (only psea exists here)")
    parser.add_argument("-t", "--threads", type=int, default=1, help="accepted for compatibility; one device launch does all files")
    parser.add_argument("--title", type=str, default="", help="Title for plot")
    parser.add_argument("--freqlim", type=float, default=0.09,
                        help="Upper limit for frequency in 2D histogram. Set to 0 to disable.")
    parser.add_argument("--json", type=str, default="", help="JSON file to write co-occurences in (alpha, beta)")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.backend != "psea":
        raise NotImplementedError(f"--backend {args.backend}: there is no DSSP here, only psea")
    if len(args.infiles) == 1 and args.infiles[0].endswith(".json"):
        raise NotImplementedError("a training_args.json input stands for the CATH test split, which needs the CATH data pipeline; "
                                  "pass the PDB files themselves")
    structures.ss_cooccurrence(args.infiles, json_file=args.json, outpdf=args.outpdf, title=args.title,
                               vmax=args.freqlim if args.freqlim > 0 else None)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
