#!/usr/bin/env python3
"""
What the tie launches of repeat sampling cost beside the visits.

``fd_sample_repeat`` against ``fd_sample_strided`` on the SAME host batch, visits, coefficients and Philox seed, in the same
process: the uploads, the network evaluations and the download are common to both; the repeat run adds one tie launch per
visit (plus the one on the start point) and replays the step graph one visit per call.  Released shape by default (12 layers,
384 / 12, relative_key), random weights, B = 512, L = 128, T = 1000, K = 50, period 16 x 8 units.  After one warm-up of each
the two are run alternately ``--reps`` times, the host clock around the call (which ends in its download); medians are
reported.  Also prints the units' superposed RMSD of the repeat run's backbones (structures.repeat_rmsd).

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import datasets, modelling, nerf, sampling, structures  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--period", type=int, default=16)
    ap.add_argument("--units", type=int, default=8)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    B, L, T, K, F = args.batch, args.length, args.timesteps, args.num_steps, 6
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    model = modelling.BertForDiffusionBase(cfg, [True] * F)
    model.to("cuda:0")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=L), timesteps=T, beta_schedule="cosine")
    betas = ds.alpha_beta_terms["betas"]
    h = model.prepare(betas, [True] * F)
    visits = sampling.ddim_visits(T, K)
    coef = sampling.ddim_coefficients(betas, visits, 1.0)
    x0 = np.ascontiguousarray(((torch.rand(B, L, F) * 2 - 1) * 3.0).numpy())
    lens = np.full(B, L, dtype=np.int32)
    ties = sampling.repeat_ties([L] * B, args.period, args.units)
    out = np.empty((1, B, L, F), np.float32)

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, visits, coef, None, 1234, 0, out, 0),
            "repeat": lambda: sampling._run_fd_sample_repeat(h, x0, lens, visits, coef, None, 1234, 0, ties, out[0])}
    for run in runs.values():
        run()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, run in runs.items():
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    strided_s, repeat_s = med(times["strided"]), med(times["repeat"])
    runs["repeat"]()
    rmsd = structures.repeat_rmsd(nerf.build_backbones(list(out[0][:16]), ds.feature_names["angles"], center_coords=False), 0, args.period, args.units)
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "period": args.period, "units": args.units,
                      "reps": args.reps, "strided_s": strided_s, "repeat_s": repeat_s, "ratio": repeat_s / strided_s,
                      "ms_per_visit_strided": 1e3 * strided_s / K, "ms_per_visit_added": 1e3 * (repeat_s - strided_s) / K,
                      "strided_spread_percent": 100.0 * (max(times["strided"]) - min(times["strided"])) / strided_s,
                      "repeat_rmsd_max_of_16": float(np.nanmax(rmsd)), "all_s": times}))


if __name__ == "__main__":
    main()
