#!/usr/bin/env python3
"""
Wall time of few-step sampling on a strided schedule: ``sampling.sample_on_device(num_steps=K)`` --
``fd_sample_strided_dev``, every array already on the device -- with ``eta = 0`` (DDIM, nothing drawn) and ``eta = 1`` (a
Philox draw per element and visit but the last), beside the plain sampler's per-step time from the same process:
``fd_sample_dev`` over ``--plain_steps`` steps from ``t_start = plain_steps - 1``, Philox.

Released shape by default (12 layers, 384 / 12, relative_key), random weights, B = 512, L = 128, T = 1000, K = 50.  After one
warm-up of each (code objects, workspace, graph capture), the three are run alternately ``--reps`` times; every call ends in
a device synchronise, the host clock is around the call, medians are reported.  Prints one JSON line.
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
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--plain_steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
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

    def strided(eta):
        return sampling.sample_on_device(model, x, lens, betas, [True] * 6, seed=1, num_steps=K, eta=eta)

    def plain():
        return sampling.sample_on_device(model, x, lens, betas, [True] * 6, seed=1, t_start=args.plain_steps - 1)

    runs = {"eta0": lambda: strided(0.0), "eta1": lambda: strided(1.0), "plain": plain}
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
    per_step = med(times["plain"]) / args.plain_steps
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "plain_steps": args.plain_steps, "reps": args.reps,
                      "strided_eta0_s": med(times["eta0"]), "strided_eta1_s": med(times["eta1"]), "plain_s": med(times["plain"]),
                      "plain_ms_per_step": 1e3 * per_step, "K_plain_steps_s": K * per_step,
                      "eta0_ms_per_visit": 1e3 * med(times["eta0"]) / K, "eta1_ms_per_visit": 1e3 * med(times["eta1"]) / K,
                      "all_s": times}))


if __name__ == "__main__":
    main()
