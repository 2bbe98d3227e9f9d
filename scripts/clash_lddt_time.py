#!/usr/bin/env python3
"""Time fd_backbone_clashes and fd_lddt on a sampling run's worth of backbones: one count_clashes call on 780 chains of
128 residues, and one lddt call on 6240 pairs of that size (every chain against eight jittered models of itself, N, CA
and C).  The chains come from a seed through the tests' generator (tests/clash_lddt_reference.walk_backbone).

    python scripts/clash_lddt_time.py [--reps 5] [--json out.json]

Prints one JSON line: seconds per call (host clock around the synchronous call -- upload, launch, download -- after a
warm-up call) and structures/s, with the tests' numpy restatement timed on one chain and one pair beside.  The kernel
times themselves come from a run of its own under `rocprofv3 --kernel-trace --stats`."""
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
import clash_lddt_reference as cr  # noqa: E402


def timed(fn, reps):
    fn()   # warm-up: code object, allocations
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), float(np.min(times))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    rng = np.random.default_rng(0)
    chains = [cr.walk_backbone(rng, 128) for _ in range(780)]
    refs = [c for c in chains for _ in range(8)]
    models = [cr.jittered_model(rng, r) for r in refs]
    counts, t_clash, t_clash_min = timed(lambda: structures.count_clashes(chains), args.reps)
    scores, t_lddt, t_lddt_min = timed(lambda: structures.lddt(models, refs), args.reps)
    t0 = time.perf_counter()
    want_clash = cr.clashes(chains[0])[0]
    t_np_clash = time.perf_counter() - t0
    t0 = time.perf_counter()
    (cons, total), _, _ = cr.lddt_counts(models[0], refs[0])
    t_np_lddt = time.perf_counter() - t0
    res = {
        "chains": len(chains), "pairs": len(models), "residues_per_chain": 128, "reps": args.reps,
        "clash_call_s_median": t_clash, "clash_call_s_min": t_clash_min, "clash_chains_per_s": len(chains) / t_clash,
        "lddt_call_s_median": t_lddt, "lddt_call_s_min": t_lddt_min, "lddt_pairs_per_s": len(models) / t_lddt,
        "numpy_clash_s_per_chain": t_np_clash, "numpy_lddt_s_per_pair": t_np_lddt,
        "numpy_equal": bool(int(counts[0]) == want_clash and scores[0] == cons / (4 * total)),
        "mean_clashes": float(counts.mean()), "mean_lddt": float(scores.mean()),
    }
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
