#!/usr/bin/env python3
"""
Wall time of the autoregressive sampler on the device: ``BertForAutoregressiveBase.sample`` (one
``fd_ar_sample`` call: the triangle of forwards, no host round trips) against the reference-shaped loop the library could
already run before it -- one full-length ``fd_forward_t`` per generated position, driven from Python, each with its own
upload and download.  The second loop adds the length embedding behind the LayerNorm, so its numbers are not the
baseline's; its launches and copies are those a square loop would make, which is what is timed.

Released shape by default (12 layers, 384 / 12, relative_key), random weights, B = 10, L = 128, num_seed = 4.  The two
are run alternately ``--reps`` times after one warm-up each; every call ends in a device synchronise (the download).
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

import torch  # noqa: E402

from foldingdiff_amd import beta_schedules, modelling  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--num_seed", type=int, default=4)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused", action="store_true",
                    help="options fuse_attn 1 and fuse_ffn 2 on both models: two launches per layer instead of plan_step's choice")
    args = ap.parse_args(argv)
    B, L, ns = args.batch, args.length, args.num_seed
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    ar = modelling.BertForAutoregressiveBase(cfg, [True] * 6)
    df = modelling.BertForDiffusionBase(cfg, [True] * 6)
    df.load_state_dict(ar.state_dict())
    ar.to("cuda:0")
    df.to("cuda:0")
    if args.fused:
        ar.prepare()
        df.prepare(beta_schedules.cosine_beta_schedule(1000))
        for m in (ar, df):
            m.set_option("fuse_attn", 1)
            m.set_option("fuse_ffn", 2)
    seed = (torch.rand(B, L, 6) * 2 - 1) * 3.0
    lens = torch.full((B,), L, dtype=torch.long)

    def triangle():
        return ar.sample(seed, lens, num_seed=ns, pbar=False)

    def square():
        ret = seed.clone()
        mask = torch.zeros(B, L)
        for i in range(ns, L):
            mask[:, :i] = 1.0
            ret[:, i] = df.forward_mixed_t(ret, lens, mask)[:, i]
        return ret

    triangle(), square()   # warm-up: code objects, workspaces, tables
    t_tri, t_sq = [], []
    for _ in range(args.reps):
        for fn, acc in ((triangle, t_tri), (square, t_sq)):
            t0 = time.perf_counter()
            fn()
            acc.append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    print(json.dumps({"B": B, "L": L, "num_seed": ns, "layers": args.layers, "steps": L - ns, "reps": args.reps, "fused": args.fused,
                      "fd_ar_sample_s": med(t_tri), "fd_ar_sample_all_s": t_tri,
                      "forward_loop_s": med(t_sq), "forward_loop_all_s": t_sq, "ratio": med(t_sq) / med(t_tri)}))


if __name__ == "__main__":
    main()
