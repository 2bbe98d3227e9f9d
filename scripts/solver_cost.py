#!/usr/bin/env python3
"""
What a visit of the second-order multistep solver costs beside a DDIM visit: ``sampling.sample_on_device(num_steps=K,
solver="dpm2m")`` -- ``fd_sample_solver_dev`` -- against ``solver=None`` with ``eta = 0`` -- ``fd_sample_strided_dev`` -- on the
SAME visits, every array already on the device, in the same process.  The solver's update reads and writes one [B, L, F]
float32 array more per visit (the previous prediction of the clean state: 2 x 1.57 MB at the default shape) and draws nothing.

Released shape by default (12 layers, 384 / 12, relative_key), random weights, B = 512, L = 128, T = 1000, K = 20.  After one
warm-up of each (code objects, workspace, graph capture), the two are run alternately ``--reps`` times; every call ends in a
device synchronise, the host clock is around the call, medians are reported.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from foldingdiff_amd import beta_schedules, modelling, sampling  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=20)
    ap.add_argument("--spacing", default="logsnr", choices=["uniform", "logsnr"])
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args(argv)
    B, L, T, K = args.batch, args.length, args.timesteps, args.num_steps
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    model = modelling.BertForDiffusionBase(cfg, [True] * 6)
    model.to("cuda:0")
    betas = beta_schedules.cosine_beta_schedule(T)
    model.prepare(betas, [True] * 6)
    x = ((torch.rand(B, L, 6) * 2 - 1) * 3.0).to("cuda:0")
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda:0")

    def run(solver):
        return sampling.sample_on_device(model, x, lens, betas, [True] * 6, num_steps=K, eta=0.0, solver=solver, spacing=args.spacing)

    runs = {"ddim": lambda: run("ddim"), "dpm2m": lambda: run("dpm2m")}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    d, s = med(times["ddim"]), med(times["dpm2m"])
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "spacing": args.spacing, "reps": args.reps,
                      "ddim_s": d, "dpm2m_s": s, "ddim_ms_per_visit": 1e3 * d / K, "dpm2m_ms_per_visit": 1e3 * s / K,
                      "extra_us_per_visit": 1e6 * (s - d) / K, "extra_percent": 100.0 * (s - d) / d,
                      "ddim_spread_percent": 100.0 * (max(times["ddim"]) - min(times["ddim"])) / d, "all_s": times}))


if __name__ == "__main__":
    main()
