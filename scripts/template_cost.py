#!/usr/bin/env python3
"""
What a guided visit costs with a superposition restraint in place of the distance restraints, beside DESIGN 6y's
figure.

``fd_sample_strided``, ``fd_sample_guided_inpaint`` with scripts/scaffold_guide_cost.py's 36 to 40 distance restraints per chain,
and ``fd_sample_guided_inpaint_tpl`` with a 48-atom template (N, CA and C of the 16 held residues) and no distance restraint, on
the SAME host batch, visits, coefficients, held segments and Philox seed, in the same process: the uploads, the network
evaluations and the download are common to all three.  Both guided runs put six launches behind a visit (shift, scan,
restraints, clashes, derivative, update); the new one a seventh, ``template_kernel``, while its restraint launch walks empty
lists.  The workload is scripts/scaffold_guide_cost.py's: released shape (12 layers, 384 / 12, relative_key), random weights,
B = 512, L = 128, T = 1000, K = 50, two held 8-residue segments (rows 20-27 and 80-87 with their lead elements).  After one
warm-up of each the three are run alternately ``--reps`` times, the host clock around the call (which ends in its download);
medians are reported.

``--trace``: one run of each and nothing else, for a run of its own under
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/template_cost.py --trace``.

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
from scaffold_guide_cost import SEGMENTS  # noqa: E402


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
    no_restraints = structures.pack_restraints(None, [L] * B)
    per_chain = np.diff(packed[0])
    fixed = np.zeros((B, L, F), dtype=np.uint8)
    for lo, hi in SEGMENTS:
        fixed[:, lo:hi] = 1
        fixed[:, lo - 1, names.index("tau")] = 1
    known = np.where(fixed == 1, rng.uniform(-3.0, 3.0, fixed.shape), 0.0).astype(np.float32)
    known_coef = sampling.inpaint_levels(betas)
    held = [r for lo, hi in SEGMENTS for r in range(lo, hi)]
    atoms = [3 * r + a for r in held for a in range(3)]
    templates = [structures.Template(atoms, np.cumsum(rng.standard_normal((len(atoms), 3)) * 1.5, axis=0)) for _ in range(B)]
    tpl_packed = structures.pack_templates(templates, [L] * B)
    sparams = sampling.scaffold_guide_params(names, OFFSET, 1.0, clash_weight=args.clash_weight)
    out = np.empty((1, B, L, F), np.float32)
    energy2, energy3, worst, rmsd = np.empty((B, 2)), np.empty((B, 3)), np.empty(B), np.empty(B)

    runs = {"strided": lambda: sampling._run_fd_sample_strided(h, x0, lens, visits, coef3, None, 1234, 0, out, 0),
            "guided_inpaint": lambda: sampling._run_fd_sample_guided_inpaint(h, x0, lens, visits, coef, known, fixed, known_coef, 1234, guide, sparams,
                                                                             packed, out[0], energy2, worst),
            "guided_inpaint_tpl": lambda: sampling._run_fd_sample_guided_inpaint_tpl(h, x0, lens, visits, coef, known, fixed, known_coef, 1234, guide,
                                                                                     sparams, no_restraints, tpl_packed, out[0], energy3, worst, rmsd)}
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
    strided_s, dist_s, tpl_s = (med(times[k]) for k in ("strided", "guided_inpaint", "guided_inpaint_tpl"))
    print(json.dumps({"B": B, "L": L, "T": T, "layers": args.layers, "num_steps": K, "scale": args.scale, "clash_weight": args.clash_weight,
                      "reps": args.reps, "restraints_per_chain": [int(per_chain.min()), int(per_chain.max())], "template_atoms_per_chain": len(atoms),
                      "held_elements_per_chain": int(fixed[0].sum()),
                      "strided_s": strided_s, "guided_inpaint_s": dist_s, "guided_inpaint_tpl_s": tpl_s,
                      "ratio_guided_inpaint": dist_s / strided_s, "ratio_guided_inpaint_tpl": tpl_s / strided_s,
                      "ms_per_visit_strided": 1e3 * strided_s / K, "ms_per_visit_added_guided_inpaint": 1e3 * (dist_s - strided_s) / K,
                      "ms_per_visit_added_guided_inpaint_tpl": 1e3 * (tpl_s - strided_s) / K,
                      "strided_spread_percent": 100.0 * (max(times["strided"]) - min(times["strided"])) / strided_s,
                      "final_template_energy_mean": float(energy3[:, 2].mean()), "final_template_rmsd_mean": float(rmsd.mean()),
                      "all_s": times}))


if __name__ == "__main__":
    main()
