#!/usr/bin/env python3
"""
DSSP states of PDB files on MI355X: the arguments of bin/annot_secondary_structures.py without --backend.

Every file is labelled from its backbone hydrogen bonds (foldingdiff_amd.structures.dssp, Kabsch & Sander's rules restated
on the device, all files in one launch): the file's own O atoms where it has them, oxygens placed by
structures.add_oxygens otherwise (generated backbones), PRO as no donor.  The 2-D histogram of the numbers of H runs and
E runs goes to the PDF (skipped with a log line when matplotlib is missing).  With --json the per-file results are
written as {file name: {"dssp": the label string, "n_helix": runs of H, "n_strand": runs of E, "n_hbonds": kept bonds}}.
Files with several models or of more than 1024 residues are left out.

The labels are not pinned to the mkdssp binary: beta-bulges and sheet labels are not built.  --threads is
accepted for compatibility; the device labels every file at once.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from foldingdiff_amd import structures  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("infiles", type=str, nargs="+", help="PDB files to compute DSSP states for")
    parser.add_argument("outpdf", type=str, help="PDF file to write plot of secondary structure co-occurrence frequencies")
    parser.add_argument("-t", "--threads", type=int, default=1, help="accepted for compatibility; one device launch does all files")
    parser.add_argument("--title", type=str, default="", help="Title for plot")
    parser.add_argument("--freqlim", type=float, default=0.09,
                        help="Upper limit for frequency in 2D histogram. Set to 0 to disable.")
    parser.add_argument("--json", type=str, default="", help="JSON file to write the per-file strings and run counts in")
    return parser


def dssp_files(fnames, device: int = 0):
    """[(file, label string, (bonds, H runs, E runs))] of the files that can be labelled."""
    kept, chains, flags = [], [], []
    for f in fnames:
        bb = structures.read_backbone_atoms(f)
        if bb is None or len(bb[0]) > structures.DSSP_MAX_LEN:
            logging.warning(f"{f}: rejected by the parser or longer than {structures.DSSP_MAX_LEN} residues - skipping")
            continue
        kept.append(f)
        chains.append(bb[0])
        flags.append(np.array([structures.DSSP_NO_DONOR if n == "PRO" else 0 for n in bb[1]], dtype=np.uint8))
    need = [k for k, x in enumerate(chains) if np.isnan(x[:-1, 3]).any()]
    for k, x in zip(need, structures.add_oxygens([chains[k][:, :3] for k in need], device=device)):
        chains[k] = x
    labels = structures.dssp(chains, flags=flags, device=device)
    counts = structures.dssp_counts(chains, flags=flags, device=device)
    return [(f, "".join(s), tuple(int(v) for v in c)) for f, s, c in zip(kept, labels, counts)]


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    res = dssp_files(args.infiles)
    if args.json:
        with open(args.json, "w") as sink:
            json.dump({os.path.basename(f): {"dssp": s, "n_helix": c[1], "n_strand": c[2], "n_hbonds": c[0]} for f, s, c in res},
                      sink, indent=4)
    structures.write_ss_cooccurrence([os.path.basename(f) for f, _, _ in res], [(c[1], c[2]) for _, _, c in res], outpdf=args.outpdf,
                                     title=args.title, vmax=args.freqlim if args.freqlim > 0 else None)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
