#!/usr/bin/env python3
"""
What a guided visit costs with the cyclic-symmetry lines behind it, beside DESIGN 6y's figure.

``fd_sample_strided``, ``fd_sample_guided_inpaint`` (nothing held, no restraints, the intra-chain clash term on) and
``fd_sample_guided_inpaint_sym`` with the same settings plus order ``--order`` and ``--pose_iters`` rigid-body steps per visit,
on the SAME host batch, visits, coefficients and Philox seed, in the same process: the uploads, the network evaluations and the
download are common to all three.  The workload is scripts/scaffold_guide_cost.py's shape: released architecture (12 layers,
384 / 12, relative_key), random weights, B = 512, L = 128, T = 1000, K = 50.  After one warm-up of each the three are run
alternately ``--reps`` times, the host clock around the call (which ends in its download); medians are reported.

``--trace``: one run of each and nothing else, for a run of its own under
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/symmetry_cost.py --trace``.

``--pair``: no guided run.  The final states of ONE ``fd_sample_strided`` run become fixed structures (``nerf.build_backbones``,
the scan), placed by ``structures.start_pose`` at ``--radius_scale`` times its default radius (0.5: the copies interpenetrate, as
they do in the guided run on random weights), and ``fd_symmetry_energy`` is called ``--reps`` times on them at ``--order``,
``--d_on`` and ``--d_off``: under ``rocprofv3 --kernel-trace --stats``, one process per setting, ``symmetry_pair_kernel``'s time
at the default limits, at limits below the clash limit (``--d_on 1 --d_off 2``) and at another order says what the CA limit and
what the copy count cost.  It does not depend on what a guided run does to the structures.

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
from guide_cost import OFFSET  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--num_steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--clash_weight", type=float, default=1.0)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--pose_iters", type=int, default=1)
    ap.add_argument("--d_on", type=float, default=8.0, help="the contact term's inner limit")
    ap.add_argument("--d_off", type=float, default=12.0, help="its outer limit (below the clash limit of about 2.3 A the pair test is the clash test alone)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pair", action="store_true", help="fd_symmetry_energy on fixed structures only (see above)")
    ap.add_argument("--radius_scale", type=float, default=0.5)
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
    no_restraints = structures.pack_restraints(None, [L] * B)
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    known = np.zeros((B, L, F), dtype=np.float32)
    known_coef = sampling.inpaint_levels(betas)
    sparams = sampling.scaffold_guide_params(names, OFFSET, 1.0, clash_weight=args.clash_weight)
    sym_params = structures.symmetry_params(pose_iters=args.pose_iters, d_on=args.d_on, d_off=args.d_off)
    orders = np.full(B, args.order, dtype=np.int32)
    pose0 = structures.start_pose(None, orders, lengths=[L] * B)
    out = np.empty((1, B, L, F), np.float32)
    energy2, energy3, worst, rmsd = np.empty((B, 2)), np.empty((B, 3)), np.empty(B), np.empty(B)
    sym_e, sym_c, sym_pose = np.empty((B, 3)), np.empty(B, dtype=np.int32), np.empty((B, 12))

    if args.pair:
        from foldingdiff_amd import nerf
        sampling._run_fd_sample_strided(h, x0, lens, visits, coef3, None, 1234, 0, out, 0)
        rows = out[0] + np.asarray(OFFSET, dtype=np.float32)   # (data space; NeRF takes any angle, wrapped or not)
        chains = nerf.build_backbones(list(rows), names, center_coords=False, method="scan")
        if not all(np.isfinite(c).all() for c in chains):
            raise SystemExit("a structure is not finite")
        default = structures.start_pose(chains, orders)
        poses = structures.start_pose(chains, orders, radius=args.radius_scale * (default[:, 9:] + np.array([c[1::3].mean(axis=0) for c in chains]))[:, 0])
        for _ in range(args.reps):
            energy, contacts = structures.symmetry_energy(chains, orders, poses, params=sym_params)
        print(json.dumps({"B": B, "L": L, "order": args.order, "d_on": args.d_on, "d_off": args.d_off, "radius_scale": args.radius_scale, "reps": args.reps,
                          "energy_mean": [float(v) for v in energy.mean(axis=0)], "contacts_mean": float(contacts.mean())}))
        return

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, visits, coef3, None, 1234, 0, out, 0),
            "guided_inpaint": lambda: sampling._run_fd_sample_guided_inpaint(h, x0, lens, visits, coef, known, fixed, known_coef, 1234, guide, sparams,
                                                                             no_restraints, out[0], energy2, worst),
            "guided_inpaint_sym": lambda: sampling._run_fd_sample_guided_inpaint_sym(h, x0, lens, visits, coef, known, fixed, known_coef, 1234, guide,
                                                                                     sparams, no_restraints, (None,) * 4, orders, pose0, sym_params,
                                                                                     out[0], energy3, worst, rmsd, sym_e, sym_c, sym_pose)}
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
    strided_s, plain_s, sym_s = (med(times[k]) for k in ("strided", "guided_inpaint", "guided_inpaint_sym"))
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "scale": args.scale, "clash_weight": args.clash_weight,
                      "order": args.order, "pose_iters": args.pose_iters, "d_on": args.d_on, "d_off": args.d_off, "reps": args.reps,
                      "strided_s": strided_s, "guided_inpaint_s": plain_s, "guided_inpaint_sym_s": sym_s,
                      "ratio_guided_inpaint": plain_s / strided_s, "ratio_guided_inpaint_sym": sym_s / strided_s,
                      "ratio_sym_over_guided_inpaint": sym_s / plain_s,
                      "ms_per_visit_strided": 1e3 * strided_s / K, "ms_per_visit_added_guided_inpaint": 1e3 * (plain_s - strided_s) / K,
                      "ms_per_visit_added_guided_inpaint_sym": 1e3 * (sym_s - strided_s) / K,
                      "strided_spread_percent": 100.0 * (max(times["strided"]) - min(times["strided"])) / strided_s,
                      "final_symmetry_energy_mean": [float(v) for v in sym_e.mean(axis=0)], "final_contacts_mean": float(sym_c.mean()),
                      "all_s": times}))


if __name__ == "__main__":
    main()
