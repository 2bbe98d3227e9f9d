#!/usr/bin/env python3
"""
Wall time of a conditioned strided visit: ``fd_sample_strided_inpaint`` beside ``fd_sample_strided`` on the
same grid in the same process, and a resampled run over that grid (``fd_sample_strided_inpaint_resample``,
``--jump_length`` visits back up, ``--n_resample`` descents per stretch) per visit.  All three through the host entries
(the new ones have no device-array variants): each call uploads x_init / lens / the tables and downloads the final state,
1.5 MB each way at the default shape.

Released shape by default (12 layers, 384 / 12, relative_key), random weights, B = 512, L = 128, T = 1000, K = 50, a motif
of 20 residues in the middle of every chain, ``eta = 0``, Philox for the replacement.  After one warm-up of each (code
objects, workspace, graph capture), the three are run alternately ``--reps`` times; the host clock is around the call (which
returns with the stream drained), medians are reported.  Prints one JSON line.
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

from foldingdiff_amd import beta_schedules, modelling, sampling  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--motif", type=int, default=20)
    ap.add_argument("--jump_length", type=int, default=5)
    ap.add_argument("--n_resample", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    B, L, T, K, F = args.batch, args.length, args.timesteps, args.num_steps, 6
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    model = modelling.BertForDiffusionBase(cfg, [True] * F)
    model.to("cuda:0")
    betas = beta_schedules.cosine_beta_schedule(T)
    h = model.prepare(betas, [True] * F)
    rng = np.random.default_rng(0)
    x0 = rng.uniform(-3.0, 3.0, (B, L, F)).astype(np.float32)
    lens = np.full(B, L, dtype=np.int32)
    known = rng.uniform(-3.0, 3.0, (B, L, F)).astype(np.float32)
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    lo = (L - args.motif) // 2
    fixed[:, lo: lo + args.motif] = 1
    grid = sampling.ddim_visits(T, K)
    coef = sampling.ddim_coefficients(betas, grid, args.eta)
    kcoef = sampling.inpaint_levels(betas)
    run = sampling.strided_resample_schedule(grid, args.jump_length, args.n_resample)
    jump_coef = sampling.strided_jump_coef(betas, grid, run)
    out = np.empty((1, B, L, F), dtype=np.float32)

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, grid, coef, None, 1, 0, out, 0),
            "conditioned": lambda: sampling._run_fd_strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, None, None, 1, out, 0),
            "resampled": lambda: sampling._run_fd_strided_inpaint(h, x0, lens, grid, coef, known, fixed, kcoef, run, jump_coef, 1, out, 0)}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "eta": args.eta, "motif": args.motif,
                      "jump_length": args.jump_length, "n_resample": args.n_resample, "run_visits": int(len(run)),
                      "jumps": int(len(jump_coef)), "reps": args.reps,
                      "strided_s": med(times["strided"]), "conditioned_s": med(times["conditioned"]), "resampled_s": med(times["resampled"]),
                      "strided_ms_per_visit": 1e3 * med(times["strided"]) / K, "conditioned_ms_per_visit": 1e3 * med(times["conditioned"]) / K,
                      "resampled_ms_per_visit": 1e3 * med(times["resampled"]) / len(run), "all_s": times}))


if __name__ == "__main__":
    main()
