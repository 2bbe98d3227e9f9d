#!/usr/bin/env python3
"""Time fd_annotate_sse on a sampling run's worth of backbones: 780 chains (lengths 50-127, 10 each) annotated in one
call.  The chains are generated from a seed by the tests' generator (helix, strand and random-walk segments, 0.25 A
noise), so that all three labels occur.

    python scripts/psea_time.py [--reps 5] [--numpy-chains 8] [--json out.json]

Prints one JSON line: seconds per call (host clock around the synchronous call, after a warm-up call), chains/s, and
the tests' numpy restatement (tests/psea_reference.py) timed on the first few chains, with its chains/s beside.  The
kernel time itself comes from a run of its own under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from foldingdiff_amd import structures  # noqa: E402
import psea_reference as pr  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--numpy-chains", type=int, default=8)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    rng = np.random.default_rng(0)
    chains = [pr.segment_chain(rng, n, 0.25) for n in range(50, 128) for _ in range(10)]
    got = structures.annotate_sse(chains)   # warm-up: code object, allocations
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        counts = structures.count_secondary_structures(chains)
        times.append(time.perf_counter() - t0)
    k = args.numpy_chains
    t0 = time.perf_counter()
    want = [pr.psea(c) for c in chains[:k]]
    t_np = (time.perf_counter() - t0) / k
    labels = "".join("".join(g) for g in got)
    res = {
        "chains": len(chains), "residues": len(labels), "reps": args.reps,
        "call_s_median": float(np.median(times)), "call_s_min": float(np.min(times)),
        "chains_per_s": len(chains) / float(np.median(times)),
        "numpy_s_per_chain": t_np, "numpy_chains_per_s": 1.0 / t_np, "numpy_chains_timed": k,
        "numpy_chains_equal": sum("".join(g) == w for g, w in zip(got, want)),
        "labels": {c: labels.count(c) for c in "cab"},
        "mean_helices": float(counts[:, 0].mean()), "mean_strands": float(counts[:, 1].mean()),
    }
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
