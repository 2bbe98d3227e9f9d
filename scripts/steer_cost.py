#!/usr/bin/env python3
"""
What an event of steered sampling costs beside a visit, and what steering does on random weights.

Cost: ``fd_sample_steered`` on the SAME host batch, visits and Philox seed with an event after every visit and with no event
at all, in the same process; the uploads, the visits and the final rewards pass are common to both, so the difference over
the number of visits is one event (shift + NeRF + clashes + P-SEA + terms + resample + gather + the copy back).  Released
shape by default (12 layers, 384 / 12, relative_key), random weights, B = 512 = 64 groups x 8 particles, L = 128, T = 1000,
K = 20.  After one warm-up of each the two are run alternately ``--reps`` times, the host clock around the call (which ends
in its download); medians are reported.

Effect: ``sampling.steer`` with 64 groups x 8 particles (``select="best"``) against 512 unsteered samples (one particle per
group: the plain noisy strided run) with the same schedule -- the mean final clash count and strand fraction of each.  The
weights are random: the figures say that the resampling does what it states, not what it buys on a trained model.

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

from foldingdiff_amd import datasets, modelling, sampling  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--particles", type=int, default=8)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--effect_steps", type=int, default=50, help="visits of the effect runs (0: skip them)")
    ap.add_argument("--w_clashes", type=float, default=-1.0)
    ap.add_argument("--w_strand", type=float, default=10.0)
    ap.add_argument("--lam", type=float, default=1.0)
    args = ap.parse_args(argv)
    G, P, L, T, K = args.groups, args.particles, args.length, args.timesteps, args.num_steps
    B, F = G * P, 6
    cfg = modelling.BertConfig(hidden_size=384, num_attention_heads=12, intermediate_size=768, num_hidden_layers=args.layers,
                               max_position_embeddings=128, position_embedding_type="relative_key")
    torch.manual_seed(0)
    model = modelling.BertForDiffusionBase(cfg, [True] * F)
    model.to("cuda:0")
    ds = datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=L), timesteps=T, beta_schedule="cosine")
    betas = ds.alpha_beta_terms["betas"]
    h = model.prepare(betas, [True] * F)
    names = ds.feature_names["angles"]
    reward = {"clashes": args.w_clashes, "strand": args.w_strand}

    visits = sampling.ddim_visits(T, K)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    params = sampling.steer_params(sampling.reward_weights(reward), args.lam, 0.5, 0.63, names, None)
    x0 = np.ascontiguousarray(((torch.rand(B, L, F) * 2 - 1) * 3.0).numpy())
    lens = np.full(B, L, dtype=np.int32)
    u = np.random.default_rng(0).random((K, G))
    out, terms, rew, logw = np.empty((B, L, F), np.float32), np.empty((B, 4)), np.empty(B), np.empty(B)

    def run(event):
        sampling._run_fd_sample_steered(h, x0, lens, visits, coef, None, 1234, 0, event, P, params, u, out, terms, rew, logw, None)

    runs = {"none": np.zeros(K, np.uint8), "all": np.ones(K, np.uint8)}
    for ev in runs.values():
        run(ev)
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, ev in runs.items():
            t0 = time.perf_counter()
            run(ev)
            times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    none_s, all_s = med(times["none"]), med(times["all"])
    result = {"B": B, "groups": G, "particles": P, "L": L, "T": T, "layers": args.layers, "num_steps": K, "reps": args.reps,
              "no_event_s": none_s, "all_events_s": all_s, "ms_per_visit_with_its_share_of_the_call": 1e3 * none_s / K,
              "ms_per_event": 1e3 * (all_s - none_s) / K, "event_percent_of_visit": 100.0 * (all_s - none_s) / none_s,
              "no_event_spread_percent": 100.0 * (max(times["none"]) - min(times["none"])) / none_s, "all_s": times}

    if args.effect_steps > 0:
        kw = dict(reward=reward, lam=args.lam, ess_frac=0.5, num_steps=args.effect_steps, eta=1.0, seed=11, batch_size=B)
        torch.manual_seed(5)
        _, steered = sampling.steer(model, ds, [L] * G, n_particles=P, select="best", **kw)
        torch.manual_seed(5)
        _, pool = sampling.steer(model, ds, [L] * G, n_particles=P, select="all", **kw)
        torch.manual_seed(5)
        _, plain = sampling.steer(model, ds, [L] * B, n_particles=1, select="all", **kw)
        mean = lambda info, k: float(info["terms"][:, k].mean())   # noqa: E731
        # selection alone, without resampling: the best of every P consecutive unsteered samples
        pick = np.array([g * P + int(np.argmax(plain["reward"][g * P: (g + 1) * P])) for g in range(B // P)])
        picked = plain["terms"][pick]
        result["effect"] = {"num_steps": args.effect_steps, "reward": reward, "lam": args.lam, "ess_frac": 0.5, "events": int(steered["events"].sum()),
                            "unsteered_n": int(len(plain["reward"])), "unsteered_mean_clashes": mean(plain, 0), "unsteered_mean_strand": mean(plain, 3),
                            "unsteered_mean_rg": mean(plain, 1), "unsteered_mean_helix": mean(plain, 2),
                            "unsteered_best_of_p_mean_clashes": float(picked[:, 0].mean()), "unsteered_best_of_p_mean_strand": float(picked[:, 3].mean()),
                            "steered_all_particles_mean_clashes": mean(pool, 0), "steered_all_particles_mean_strand": mean(pool, 3),
                            "steered_best_n": int(len(steered["reward"])), "steered_best_mean_clashes": mean(steered, 0),
                            "steered_best_mean_strand": mean(steered, 3), "steered_best_mean_rg": mean(steered, 1),
                            "steered_best_mean_helix": mean(steered, 2),
                            "distinct_final_ancestors_per_group": float(np.mean([len(set(a[-1, g * P: (g + 1) * P].tolist())) for a in steered["ancestors"]
                                                                                 for g in range(a.shape[1] // P)]))}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
