#!/usr/bin/env python3
"""Time fd_tm_align on the novelty job of the manuscript sweep in miniature: 780 seeded chains (lengths 50-127, 10
each: helix, strand and random-walk segments under random rotations) against 64 references of the same kind, 49,920
pairs, through structures.max_tm_across_refs.

    python scripts/tmalign_time.py [--reps 3] [--refs 64] [--numpy-pairs 3] [--starts two|all|both] [--json out.json]

Prints one JSON line: seconds per call (host clock around the whole synchronous call with its copies and host checks,
after a warm-up call), pairs/s, and the tests' numpy restatement (tests/tmalign_reference.py) timed on a few pairs on
one host thread -- the only baseline there is.  --starts all times fd_tm_align_ex with all five starts; --starts both
times the two in one process, one after the other on the same device, and adds what the three further starts change:
the share of pairs each raises above starts 1 and 2 and the distribution of TM(all) - TM(two) over the pairs ("gain").
The kernel time itself comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/tmalign_time.py --reps 1 --numpy-pairs 0 --starts both"""
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
import tmalign_reference as ta  # noqa: E402


def chains(n_refs, seed=0):
    rng = np.random.default_rng(seed)
    queries = [pr.segment_chain(rng, n, 0.3) for n in range(50, 128) for _ in range(10)]
    refs = [pr.segment_chain(rng, int(n), 0.3) for n in rng.integers(50, 128, n_refs)]
    return queries, refs


STARTS = {"two": ("threading", "ss"), "all": "all"}


def timed(queries, refs, starts, reps):
    """Seconds per max_tm_across_refs call after a warm-up call (code object, allocations), and its result."""
    best, which = structures.max_tm_across_refs(queries, refs, starts=starts)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        again, again_which = structures.max_tm_across_refs(queries, refs, starts=starts)
        times.append(time.perf_counter() - t0)
        assert np.array_equal(again, best) and np.array_equal(again_which, which)
    return times, best


def gains(queries, refs):
    """What the further starts change over all pairs: one fd_tm_align_ex call with the per-start scores."""
    nq = len(queries)
    A = [queries[q] for q in range(nq) for _ in refs]
    B = [r for _ in range(nq) for r in refs]
    tm, st = structures.tm_align(A, B, starts="all", return_start_tms=True)
    two = st[:, :2].max(1)
    gain = tm - two
    out = {"pairs_raised": float((gain > 0).mean()), "gain_mean": float(gain.mean()), "gain_max": float(gain.max()),
           "gain_quantiles": {str(q): float(np.quantile(gain, q)) for q in (0.5, 0.9, 0.99, 0.999)},
           "gain_mean_where_raised": float(gain[gain > 0].mean()) if (gain > 0).any() else 0.0}
    for k, name in enumerate(structures.ALIGN_STARTS[2:], start=2):
        out[f"raised_by_{name}"] = float((st[:, k] > two).mean())
        out[f"skipped_{name}"] = float((st[:, k] == -1).mean())
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--refs", type=int, default=64)
    p.add_argument("--numpy-pairs", type=int, default=3)
    p.add_argument("--starts", choices=["two", "all", "both"], default="two")
    p.add_argument("--json", default=None)
    args = p.parse_args()
    queries, refs = chains(args.refs)
    n_pairs = len(queries) * len(refs)
    first = "all" if args.starts == "all" else "two"
    times, best = timed(queries, refs, STARTS[first], args.reps)
    res = {
        "queries": len(queries), "refs": len(refs), "pairs": n_pairs, "reps": args.reps, "starts": args.starts,
        "call_s_median": float(np.median(times)), "call_s_min": float(np.min(times)),
        "pairs_per_s": n_pairs / float(np.median(times)),
        "max_tm_mean": float(best.mean()), "max_tm_min": float(best.min()), "max_tm_max": float(best.max()),
    }
    if args.starts == "both":
        times, best_all = timed(queries, refs, STARTS["all"], args.reps)
        assert (best_all >= best).all()
        res["all"] = {"call_s_median": float(np.median(times)), "call_s_min": float(np.min(times)),
                      "pairs_per_s": n_pairs / float(np.median(times)), "max_tm_mean": float(best_all.mean()),
                      "max_tm_min": float(best_all.min()), "max_tm_max": float(best_all.max()),
                      "max_tm_raised": float((best_all > best).mean()), "max_tm_gain_mean": float((best_all - best).mean()),
                      "max_tm_gain_max": float((best_all - best).max())}
        res["all"].update(gains(queries, refs))
    k = args.numpy_pairs
    if k > 0:
        t0 = time.perf_counter()
        want = [ta.tm_align(queries[q * 97 % len(queries)], refs[q])["tm"] for q in range(k)]
        t_np = (time.perf_counter() - t0) / k
        got = structures.tm_align([queries[q * 97 % len(queries)] for q in range(k)], refs[:k])
        res.update({"numpy_s_per_pair": t_np, "numpy_pairs_per_s": 1.0 / t_np, "numpy_pairs_timed": k,
                    "max_abs_diff_vs_numpy": float(np.abs(np.array(want) - got).max())})
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
