#!/usr/bin/env python3
"""
What the guide launches of restraint-guided sampling cost beside the visits.

``fd_sample_guided`` against ``fd_sample_strided`` and ``fd_sample_repeat`` with nothing tied, on the SAME host batch, visits,
coefficients and Philox seed, in the same process: the uploads, the network evaluations and the download are common to all
three; the repeat run replays the step graph one visit per call with one small launch in between, the guided run puts its
five launches there (shift, NeRF, restraints, derivative, update).  Released shape by default (12 layers, 384 / 12,
relative_key), random weights, B = 512, L = 128, T = 1000, K = 50; every chain gets the 36 CA-CA distances among 9 residues
of a random chain plus up to 4 contacts.  After one warm-up of each the three are run alternately ``--reps`` times, the host
clock around the call (which ends in its download); medians are reported, and the mean final restraint energy of the batch
with the guide table and with a table of zeros (random weights: as what it is).

``--trace``: one strided and one guided run and nothing else, for a run of its own under
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/guide_cost.py --trace``.

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

OFFSET = np.array([-1.3, 1.1, 3.0, 1.95, 2.03, 2.12], dtype=np.float32)   # about the training means of the full-angle set


def restraint_sets(rng, B, L, names):
    """Per chain: all CA-CA distances among 9 residues as they are in a random chain, and up to 4 contacts."""
    ang = np.concatenate([rng.uniform(-np.pi, np.pi, (B, L, 3)), np.array([1.94, 2.03, 2.12]) + 0.1 * rng.standard_normal((B, L, 3))],
                         axis=2).astype(np.float32)
    targets = nerf.build_backbones(ang, names, center_coords=False)
    sets = []
    for b in range(B):
        res = sorted(rng.choice(L, 9, replace=False).tolist())
        motif = targets[b].reshape(-1, 3, 3)[res].reshape(-1, 3)
        pairs = [(int(i), int(j)) for i, j in rng.choice(L, (4, 2)) if i != j]
        sets.append(structures.motif_restraints(motif, res) + structures.contact_restraints(pairs))
    return sets


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0)
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
    packed = structures.pack_restraints(restraint_sets(np.random.default_rng(1), B, L, names), [L] * B)
    per_chain = np.diff(packed[0])
    params = sampling.guide_params(names, OFFSET, 1.0)
    ties = sampling.repeat_ties([L] * B, 1, 1)
    out = np.empty((1, B, L, F), np.float32)
    energy, worst = np.empty(B), np.empty(B)

    def guided(table=guide):
        sampling._run_fd_sample_guided(h, x0, lens, visits, coef, None, 1234, 0, table, params, packed, out[0], energy, worst)

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, visits, coef3, None, 1234, 0, out, 0),
            "repeat_untied": lambda: sampling._run_fd_sample_repeat(h, x0, lens, visits, coef3, None, 1234, 0, ties, out[0]),
            "guided": guided}
    if args.trace:
        runs["strided"]()
        guided()
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
    strided_s, repeat_s, guided_s = (med(times[k]) for k in ("strided", "repeat_untied", "guided"))
    guided()
    e_guided, v_guided = float(energy.mean()), float(worst.mean())
    guided(np.zeros_like(guide))
    e_plain, v_plain = float(energy.mean()), float(worst.mean())
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "scale": args.scale, "reps": args.reps,
                      "restraints_per_chain": [int(per_chain.min()), int(per_chain.max())],
                      "strided_s": strided_s, "repeat_untied_s": repeat_s, "guided_s": guided_s, "ratio": guided_s / strided_s,
                      "ms_per_visit_strided": 1e3 * strided_s / K, "ms_per_visit_added": 1e3 * (guided_s - strided_s) / K,
                      "strided_spread_percent": 100.0 * (max(times["strided"]) - min(times["strided"])) / strided_s,
                      "final_energy_mean_guided": e_guided, "final_energy_mean_zero_table": e_plain,
                      "final_max_violation_mean_guided": v_guided, "final_max_violation_mean_zero_table": v_plain, "all_s": times}))


if __name__ == "__main__":
    main()
