#!/usr/bin/env python3
"""Time fd_tm_score on the job the C3 reconstruction sweep scores: 780 items (lengths 50-127, 10 each), each scored
twice as get_reconstruction_error's TM-scores are (against NeRF of the true angles, Ln = n, and against the file's CA
atoms, Ln = the file's length), so 1,560 residue-paired pairs in one call.  The pairs are generated from a seed: CA
traces built by NeRF from random backbone angles, and noised, rotated copies of them.

    python scripts/tm_time.py [--reps 5] [--stride 1] [--numpy-pairs 4] [--json out.json]

Prints one JSON line: seconds per call (host clock around the synchronous call, after a warm-up call), pairs/s, and
the tests' numpy restatement (tests/tm_reference.py) timed on the first few pairs, with its pairs/s beside.  The
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

from foldingdiff_amd import datasets, nerf, structures  # noqa: E402
import tm_reference as tr  # noqa: E402


def c3_pairs(seed=0):
    """(a_list, b_list, norm_lens) of the 1,560 pairs."""
    rng = np.random.default_rng(seed)
    names = datasets.FEATURE_SET_NAMES_TO_FEATURE_NAMES["canonical-full-angles"]
    lens = [n for n in range(50, 128) for _ in range(10)]
    # phi, psi, omega near a helix / strand mixture, bond angles near their means: chain-like traces
    angles = []
    for n in lens:
        f = np.zeros((n, 6), np.float32)
        f[:, 0] = rng.choice([-1.1, -2.4], n) + rng.normal(0, 0.3, n)
        f[:, 1] = rng.choice([-0.8, 2.3], n) + rng.normal(0, 0.3, n)
        f[:, 2] = np.pi + rng.normal(0, 0.05, n)
        f[:, 3:] = np.array([1.94, 2.03, 2.13]) + rng.normal(0, 0.03, (n, 3))
        angles.append(f)
    ca = [x[1::3] for x in nerf.build_backbones(angles, names)]
    a_list, b_list, norm = [], [], []
    for c in ca:
        n = len(c)
        for extra in (0, int(rng.integers(0, 20))):   # Ln = n (NeRF of the angles), Ln >= n (the file's length)
            a_list.append(c)
            b_list.append(c @ tr.rotation(rng).T + rng.uniform(-30, 30, 3) + rng.standard_normal(c.shape) * rng.uniform(0.5, 6.0))
            norm.append(n + extra)
    return a_list, b_list, norm


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--stride", type=int, default=1)
    p.add_argument("--numpy-pairs", type=int, default=4)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    a_list, b_list, norm = c3_pairs()
    n_pairs = len(a_list)
    seeds = sum(len(tr.seeds(len(a), args.stride)) for a in a_list)
    got = structures.tm_score(a_list, b_list, norm_lens=norm, stride=args.stride)   # warm-up: code object, allocations
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        again = structures.tm_score(a_list, b_list, norm_lens=norm, stride=args.stride)
        times.append(time.perf_counter() - t0)
        assert np.array_equal(again, got)
    k = args.numpy_pairs
    t0 = time.perf_counter()
    want = [tr.tm_search(a, b, Ln=L, stride=args.stride)[0] for a, b, L in zip(a_list[:k], b_list[:k], norm[:k])]
    t_np = (time.perf_counter() - t0) / k
    res = {
        "pairs": n_pairs, "seeds": seeds, "stride": args.stride, "reps": args.reps,
        "call_s_median": float(np.median(times)), "call_s_min": float(np.min(times)),
        "pairs_per_s": n_pairs / float(np.median(times)),
        "numpy_s_per_pair": t_np, "numpy_pairs_per_s": 1.0 / t_np, "numpy_pairs_timed": k,
        "max_abs_diff_vs_numpy": float(np.abs(np.array(want) - got[:k]).max()),
        "tm_mean": float(got.mean()), "tm_min": float(got.min()), "tm_max": float(got.max()),
    }
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
