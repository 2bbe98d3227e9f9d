#!/usr/bin/env python3
"""
Relax finished backbones in torsion space on the device (structures.relax): a descent on phi / psi / omega
that pushes clashing backbone atoms apart -- the rule of bin/vdw_clashes.py made soft -- and may be tethered to the input
angles.  It is no force field: nothing here knows side chains, hydrogen bonds or solvent, and whether relaxed backbones are
more designable is unmeasured.

    bin/relax_backbones.py <folder of angle CSVs> -o <outdir>      the *.csv / *.csv.gz files bin/sample.py writes
    bin/relax_backbones.py --pdb a.pdb b.pdb.gz -o <outdir>        backbones read from PDB files

A PDB file goes through structures.featurize with six features (the three dihedrals and the three bond angles), so its
backbone is REBUILT ON IDEAL BOND LENGTHS (1.34, 1.46, 1.54 Angstrom) from the first residue's frame before it is relaxed:
the relaxed file superposes on the input, it does not coincide with it.

Writes <outdir>/relaxed_angles/{name}.csv.gz, <outdir>/relaxed_pdb/{name}.pdb and <outdir>/relax_report.json: per chain the
clashing atoms before and after, the energy terms (clash | restraint | tether) before and after, the accepted steps and the
largest angle change in radians.
"""
import argparse
import glob
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import pandas as pd  # noqa: E402

from foldingdiff_amd import structures  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("angles", type=str, nargs="?", default=None, help="folder of angle CSVs as bin/sample.py writes them (sampled_angles/)")
    parser.add_argument("--pdb", type=str, nargs="+", default=None,
                        help="PDB files instead of angle CSVs; each is featurised with six features and rebuilt on ideal bond lengths")
    parser.add_argument("--outdir", "-o", type=str, required=True, help="output directory (created; must be empty)")
    parser.add_argument("--n_iter", type=int, default=200, help="iterations of the descent")
    parser.add_argument("--alpha", type=float, default=0.63, help="the clash rule's factor on the sum of the van der Waals radii")
    parser.add_argument("--margin", type=float, default=0.15, help="Angstrom added to the clash distance (>= 1e-3 keeps a relaxed chain clash-free)")
    parser.add_argument("--clash_weight", type=float, default=1.0, help="weight of the clash term")
    parser.add_argument("--tether", type=float, default=0.0, help="weight of the squared angle distance to the input")
    parser.add_argument("--move", type=str, nargs="+", default=["phi", "psi", "omega"], help="the columns that may change")
    parser.add_argument("--max_step", type=float, default=0.5, help="the most one iteration moves the angles, in radians (norm)")
    parser.add_argument("--device", "-d", type=int, default=0, help="GPU index")
    return parser


def stem(fname: str) -> str:
    base = os.path.basename(fname)
    for ext in (".csv.gz", ".csv", ".pdb.gz", ".pdb"):
        if base.endswith(ext):
            return base[: -len(ext)]
    return base


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if (args.angles is None) == (args.pdb is None):
        raise SystemExit("give either a folder of angle CSVs or --pdb files")
    if os.path.isdir(args.outdir) and os.listdir(args.outdir):
        raise SystemExit(f"Expected {args.outdir} to be empty!")
    if args.pdb is not None:
        files = list(args.pdb)
        frames = structures.featurize(files, distances=(), angles=structures.EXHAUSTIVE_ANGLES, device=args.device)
        rejected = [f for f, df in zip(files, frames) if df is None]
        if rejected:
            raise SystemExit(f"not a usable single-chain backbone: {rejected}")
    else:
        files = sorted(glob.glob(os.path.join(args.angles, "*.csv")) + glob.glob(os.path.join(args.angles, "*.csv.gz")))
        if not files:
            raise SystemExit(f"no *.csv or *.csv.gz files in {args.angles}")
        frames = [pd.read_csv(f, index_col=0) for f in files]
    os.makedirs(args.outdir, exist_ok=True)
    report = structures.relax_to_folder(frames, [stem(f) for f in files], args.outdir, device=args.device, n_iter=args.n_iter, alpha=args.alpha,
                                        margin=args.margin, clash_weight=args.clash_weight, tether=args.tether, move=tuple(args.move),
                                        max_step=args.max_step)
    before = sum(r["clashes_before"] for r in report["chains"].values())
    after = sum(r["clashes_after"] for r in report["chains"].values())
    logging.info(f"{len(files)} chains relaxed into {args.outdir}: {before} clashing atoms before, {after} after")


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
