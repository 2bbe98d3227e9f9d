#!/usr/bin/env python3
"""
Run hierarchical clustering on the pairwise TM-score distances between all PDB files of a directory on MI355X --
stand-in for the reference's bin/hclust_structures.py (--dirname and -o).

All n (n - 1) / 2 pairs are aligned by foldingdiff_amd.structures.pairwise_tmscores (the TM-align-style search restated
on the device in place of one TMalign subprocess per pair); d(x, y) = 1 - TMscore(x, y) is clustered by average
linkage.  Next to the PDF named by -o this writes <stem>_dist.csv (the distance matrix), <stem>_linkage.csv (scipy's
linkage matrix) and <stem>_settings.json ({"starts": ...}).  --starts all searches every pair from all five of TM-align's
starts instead of two (fd_tm_align_ex): slower, never a lower score, so never a larger distance.  The clustermap PDF itself is drawn by seaborn and is skipped with a log line when seaborn is missing.

What is NOT here: --testsubset (it samples the CATH test split, whose data pipeline is not here) and --sctm.  Files that
cannot be read as one model, and chains of more than 512 residues, are logged and left out.
"""
import argparse
import json
import logging
import os
import re
import sys
from glob import glob

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from foldingdiff_amd import structures  # noqa: E402


STARTS = {"two": ("threading", "ss"), "all": "all"}


def int_key(path: str):
    """Files in the order of the integers in their names (the reference asserts exactly one), then by name."""
    return tuple(int(i) for i in re.findall(r"[0-9]+", os.path.basename(path))), os.path.basename(path)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--dirname", type=str, required=True, help="Directory of PDB files to analyze")
    parser.add_argument("-o", "--output", type=str, default="tmscore_hclust.pdf", help="PDF file to write output clustering plot")
    parser.add_argument("--device", type=int, default=0, help="GPU index")
    parser.add_argument("--starts", choices=sorted(STARTS), default="two",
                        help="Starts of the alignment search: two (threading, secondary structure) or all five")
    return parser


def main(argv=None) -> None:
    import scipy.cluster.hierarchy as hc
    import scipy.spatial as sp

    args = build_parser().parse_args(argv)
    fnames = sorted(glob(os.path.join(args.dirname, "*.pdb")), key=int_key)
    assert fnames, f"{args.dirname} does not contain any pdb files"
    # TMscore of 1 = perfect match --> 0 distance, so need 1.0 - tmscore
    pdist_df = 1.0 - structures.pairwise_tmscores(fnames, device=args.device, starts=STARTS[args.starts])
    assert len(pdist_df) >= 2, "clustering needs at least two structures"
    stem = os.path.splitext(args.output)[0]
    pdist_df.to_csv(stem + "_dist.csv")
    with open(stem + "_settings.json", "w") as sink:
        json.dump({"starts": args.starts}, sink, indent=4)
    linkage = hc.linkage(sp.distance.squareform(pdist_df.values, checks=False), method="average", optimal_ordering=False)
    np.savetxt(stem + "_linkage.csv", linkage, delimiter=",")
    try:
        import seaborn as sns
    except ImportError as e:
        logging.warning(f"seaborn is not available ({e}), not writing {args.output}")
        return
    c = sns.clustermap(pdist_df, row_linkage=linkage, col_linkage=linkage, method=None, row_cluster=True, col_cluster=True,
                       vmin=0.0, vmax=1.0, xticklabels=False, yticklabels=False,
                       cbar_kws={"label": r"$d(x, y) = 1 - \mathrm{TMscore}(x, y)$"})
    c.savefig(args.output)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
