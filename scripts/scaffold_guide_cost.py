#!/usr/bin/env python3
"""
What a guided visit costs with replacement, the scan and the clash term, beside DESIGN 6w's figure.

``fd_sample_strided``, ``fd_sample_guided`` and ``fd_sample_guided_inpaint`` on the SAME host batch, visits, coefficients,
restraints and Philox seed, in the same process: the uploads, the network evaluations and the download are common to all
three.  The guided run puts five launches behind a visit (shift, one-lane-per-chain NeRF, restraints, derivative, update), the
new run six (assemble and shift, NeRF scan, restraints, soft clashes, derivative, masked update; five with
``--clash_weight 0``).  The workload is scripts/guide_cost.py's: released shape (12 layers, 384 / 12, relative_key), random
weights, B = 512, L = 128, T = 1000, K = 50, per chain the 36 CA-CA distances among 9 residues of a random chain plus up to 4
contacts -- and, for the new run, two held 8-residue segments (rows 20-27 and 80-87 with their lead elements).  After one
warm-up of each the three are run alternately ``--reps`` times, the host clock around the call (which ends in its download);
medians are reported.

``--trace``: one run of each and nothing else, for a run of its own under
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/scaffold_guide_cost.py --trace``.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import datasets, modelling, sampling, structures  # noqa: E402
from guide_cost import OFFSET, restraint_sets  # noqa: E402

SEGMENTS = ((20, 28), (80, 88))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--clash_weight", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args(argv)
    B, L, T, K, F = args.batch, args.length, args.timesteps, args.num_steps, 6
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    model = modelling.BertForDiffusionBase(cfg, [True] * F)
    model.to("cuda:0")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=L), timesteps=T, beta_schedule="cosine")
    names = list(ds.feature_names["angles"])
    betas = ds.alpha_beta_terms["betas"]
    h = model.prepare(betas, [True] * F)
    visits = sampling.ddim_visits(T, K)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    coef3 = np.ascontiguousarray(coef[:3])
    guide = sampling.guidance_coefficients(betas, visits, coef, args.scale)
    x0 = np.ascontiguousarray(((torch.rand(B, L, F) * 2 - 1) * 3.0).numpy())
    lens = np.full(B, L, dtype=np.int32)
    rng = np.random.default_rng(1)
    packed = structures.pack_restraints(restraint_sets(rng, B, L, names), [L] * B)
    per_chain = np.diff(packed[0])
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    for lo, hi in SEGMENTS:
        if hi <= L:
            fixed[:, lo:hi] = 1
            fixed[:, lo - 1, names.index("tau")] = 1
    known = np.where(fixed == 1, rng.uniform(-3.0, 3.0, fixed.shape), 0.0).astype(np.float32)
    known_coef = sampling.inpaint_levels(betas)
    params = sampling.guide_params(names, OFFSET, 1.0)
    sparams = sampling.scaffold_guide_params(names, OFFSET, 1.0, clash_weight=args.clash_weight)
    out = np.empty((1, B, L, F), np.float32)
    energy, energy2, worst = np.empty(B), np.empty((B, 2)), np.empty(B)

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, visits, coef3, None, 1234, 0, out, 0),
            "guided": lambda: sampling._run_fd_sample_guided(h, x0, lens, visits, coef, None, 1234, 0, guide, params, packed, out[0], energy, worst),
            "guided_inpaint": lambda: sampling._run_fd_sample_guided_inpaint(h, x0, lens, visits, coef, known, fixed, known_coef, 1234, guide, sparams,
                                                                             packed, out[0], energy2, worst)}
    if args.trace:
        for run in runs.values():
            run()
        return
    for run in runs.values():
        run()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, run in runs.items():
            t0 = time.perf_counter()
            run()
            times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    strided_s, guided_s, new_s = (med(times[k]) for k in ("strided", "guided", "guided_inpaint"))
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "scale": args.scale, "clash_weight": args.clash_weight,
                      "reps": args.reps, "restraints_per_chain": [int(per_chain.min()), int(per_chain.max())],
                      "held_elements_per_chain": int(fixed[0].sum()),
                      "strided_s": strided_s, "guided_s": guided_s, "guided_inpaint_s": new_s,
                      "ratio_guided": guided_s / strided_s, "ratio_guided_inpaint": new_s / strided_s,
                      "ms_per_visit_strided": 1e3 * strided_s / K, "ms_per_visit_added_guided": 1e3 * (guided_s - strided_s) / K,
                      "ms_per_visit_added_guided_inpaint": 1e3 * (new_s - strided_s) / K,
                      "strided_spread_percent": 100.0 * (max(times["strided"]) - min(times["strided"])) / strided_s,
                      "final_restraint_energy_mean": float(energy2[:, 0].mean()), "final_clash_energy_mean": float(energy2[:, 1].mean()),
                      "all_s": times}))


if __name__ == "__main__":
    main()
