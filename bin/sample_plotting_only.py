#!/usr/bin/env python3
"""
The angle-distribution report of a finished sampling run: per angle, the histogram divergence KL(generated || test)
between the sampled angles and the angles of a set of test structures -- the first quantitative result of the reference's
bin/sample_plotting_only.py (:105-110; nbins = 200 with a pseudocount).

    bin/sample_plotting_only.py [DIR] --test-pdbs DIR_OR_LIST

DIR (default: the working directory) is the output directory of bin/sample.py: DIR/sampled_angles/generated_*.csv.gz are
read in the order of their numbers, and the feature set and the padded length come from
DIR/model_snapshot/training_args.json.  --test-pdbs names a directory of .pdb / .pdb.gz files, a text file with one path
per line, or the files themselves; those of at most max_seq_len residues are featurised on device 0 without
zero-centring (the reference's ignore_zero_center=True).  Logs "Angle <name> KL(generated || test) = ..." and writes
DIR/plots/angle_kl.json, and with matplotlib installed DIR/plots/dist_combined.pdf (the overlaid histograms).  The
Ramachandran and CDF plots of the reference are not drawn.
"""
import argparse
import json
import logging
import os
import re
import sys
from glob import glob
from pathlib import Path
from typing import Dict, List, Sequence

BIN = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(BIN)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from foldingdiff_amd import custom_metrics as cm  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("dir_name", nargs="?", default=os.getcwd(), help="Output directory of bin/sample.py (default: .)")
    parser.add_argument("--test-pdbs", nargs="+", required=True, metavar="DIR_OR_LIST",
                        help="Test structures: a directory, a text file of paths, or .pdb / .pdb.gz files")
    return parser


def int_getter(x: str) -> int:
    """The one integer in a file name."""
    matches = re.findall(r"[0-9]+", x)
    assert len(matches) == 1, x
    return int(matches.pop())


def list_test_pdbs(spec: Sequence[str]) -> List[str]:
    """--test-pdbs as a list of files (a directory is listed sorted; a text file holds one path per line)."""
    if len(spec) == 1 and os.path.isdir(spec[0]):
        files = sorted(f for ext in ("*.pdb", "*.pdb.gz") for f in glob(os.path.join(spec[0], ext)))
    elif len(spec) == 1 and not spec[0].endswith((".pdb", ".pdb.gz")):
        with open(spec[0]) as source:
            files = [line.strip() for line in source if line.strip()]
    else:
        files = list(spec)
    if not files:
        raise ValueError(f"no test structures in {spec}")
    return files


def read_sampled(dir_name: Path) -> pd.DataFrame:
    """Every DIR/sampled_angles/generated_*.csv.gz, in the order of their numbers, stacked."""
    fnames = sorted(glob(os.path.join(dir_name, "sampled_angles", "*.csv.gz")), key=lambda x: int_getter(os.path.basename(x)))
    if not fnames:
        raise FileNotFoundError(f"no sampled_angles/*.csv.gz under {dir_name}")
    logging.info(f"Found {len(fnames)} sets of generated angles")
    return pd.concat([pd.read_csv(f, index_col=0) for f in fnames], ignore_index=True)


def featurise_test(pdb_files: Sequence[str], training_args: dict) -> np.ndarray:
    """The unmasked, un-centred features of the test files of at most max_seq_len residues, stacked: float32 [N, F]."""
    from foldingdiff_amd import structures

    key = training_args["angles_definitions"]
    if key not in structures.DATASETS:
        raise NotImplementedError(f"angles_definitions={key!r}: only the canonical angle feature sets are supported")
    dset = structures.DATASETS[key](pdbs=list(pdb_files), split=None, pad=training_args["max_seq_len"],
                                    min_length=training_args.get("min_seq_len", 0), trim_strategy="discard", zero_center=False)
    logging.info(f"{len(dset)}/{len(pdb_files)} test structures of at most {dset.pad} residues")
    rows = []
    for i in range(len(dset)):
        item = dset.__getitem__(i, ignore_zero_center=True)
        rows.append(item["angles"][item["attn_mask"] != 0].numpy())
    return np.concatenate(rows, axis=0)


def plot_overlap(sampled: np.ndarray, test: np.ndarray, names: Sequence[str], kl: Dict[str, float], fname: Path) -> bool:
    """Test against sampled histograms, one panel per feature.  False (and a log line) without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except ImportError:
        logging.info(f"matplotlib is not installed: {fname} not written")
        return False
    ncols = 3 if len(names) > 4 else 2
    nrows = -(-len(names) // ncols)
    fig, axes = plt.subplots(dpi=300, nrows=nrows, ncols=ncols, figsize=(4.4 * ncols, 3.25 * nrows), squeeze=False)
    for i, (name, ax) in enumerate(zip(names, axes.flatten())):
        lo, hi = min(test[:, i].min(), sampled[:, i].min()), max(test[:, i].max(), sampled[:, i].max())
        for label, vals in (("Test", test[:, i]), ("Sampled", sampled[:, i])):
            ax.hist(vals, bins=60, range=(lo, hi), density=True, alpha=0.45, edgecolor="black", label=label)
        ax.set(title=f"{name} distribution, KL={kl[name]:.4f}")
        if i == 0:
            ax.legend()
    for ax in axes.flatten()[len(names):]:
        ax.axis("off")
    fig.tight_layout()
    fig.savefig(fname, bbox_inches="tight")
    plt.close(fig)
    return True


def report(dir_name: Path, test: np.ndarray, feature_names: Sequence[str]) -> Dict[str, float]:
    """KL(generated || test) per feature of DIR's sampled angles against ``test`` [N, F]; logs them, writes
    DIR/plots/angle_kl.json and, with matplotlib, DIR/plots/dist_combined.pdf.  The sampled angles come out of their
    files as float64, as in the reference, so the histograms are numpy's (custom_metrics.kl_from_empirical's host path)."""
    dir_name = Path(dir_name)
    sampled_df = read_sampled(dir_name)
    missing = [n for n in feature_names if n not in sampled_df.columns]
    if missing:
        raise ValueError(f"sampled angles lack the columns {missing}")
    sampled = sampled_df[list(feature_names)].values
    kl = cm.angle_kl_report(sampled, test, feature_names, nbins=200, pseudocount=True)
    for name in feature_names:
        logging.info(f"Angle {name} KL(generated || test) = {kl[name]}")
    plotdir = dir_name / "plots"
    os.makedirs(plotdir, exist_ok=True)
    with open(plotdir / "angle_kl.json", "w") as sink:
        json.dump({"nbins": 200, "pseudocount": True, "n_generated": int(sampled.shape[0]), "n_test": int(test.shape[0]),
                   "kl_generated_test": kl}, sink, indent=4)
    plot_overlap(sampled, test, feature_names, kl, plotdir / "dist_combined.pdf")
    return kl


def main(argv=None):
    args = build_parser().parse_args(argv)
    dir_name = Path(args.dir_name)
    with open(dir_name / "model_snapshot" / "training_args.json") as source:
        training_args = json.load(source)
    from foldingdiff_amd import datasets

    names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES[training_args["angles_definitions"]]
    report(dir_name, featurise_test(list_test_pdbs(args.test_pdbs), training_args), names)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
