#!/usr/bin/env python3
"""
Sample backbones toward distance restraints (sampling.guide; with ``--hold_motif`` sampling.scaffold_segments, 6y): residue pairs that should be in contact
(``--contacts``), and / or the residues of a motif, which need not be contiguous, that should sit relative to each other as
they do in a PDB file (``--motif_pdb --motif_residues --placed_at``).  After every visit of the few-step sampler the predicted
backbone is built on the device and the state takes a clipped step down the gradient of the restraint energy.  The model and
output arguments are bin/sample.py's:

    <outdir>/model_snapshot/                      copy of the model directory
    <outdir>/sampled_angles/generated_{i}.csv.gz  final angles of every backbone
    <outdir>/sampled_pdb/generated_{i}.pdb        N-CA-C backbones built by NeRF on the device
    <outdir>/restraints.json                      the settings, the number of restraints and, per backbone, the restraint
                                                  energy and the largest violation (Angstrom); with a motif also the CA RMSD
                                                  of the placed residues to the motif after superposition

``--contacts FILE``: one ``i j [max_dist]`` per line, residue indices from 0, CA atoms, ``max_dist`` 8 Angstrom unless given;
``#`` starts a comment.  ``--motif_residues 3-9,20-27`` picks residues of the file by position (from 0, ranges inclusive) and
``--placed_at 10,40`` gives, per range, the index its first residue takes in the new backbone.  Distances do not tell a
structure from its mirror image, so a low energy with a high RMSD is possible.  A restraint that does not fit ``--length``, or
a length beyond the model's padded length, is a usage error before the model is loaded or anything is written.  The model
must be a local directory, as for bin/sample.py.  Single device.

``--hold_motif`` (needs ``--motif_pdb``): every range of ``--motif_residues`` is HELD by replacement -- its angle rows are fixed
to the file's, so its backbone is reproduced exactly -- and the restraints are kept between residues of different ranges only,
which places the ranges relative to each other.  ``--clash_weight W`` adds the relaxer's soft clash term, weighted by W, to the
energy whose gradient is followed; the report then also holds ``clash_energy``.  Without these two flags the script does what
it did before them.

``--placement {distances,template,both}`` (needs a motif) chooses what places the motif's residues: ``distances``
is the behaviour above; ``template`` replaces the motif's distance restraints by a superposition restraint -- the N, CA and C
atoms of the placed residues are fitted to the file's by a proper rotation, weighted by ``--template_weight W``, which a mirror
image cannot satisfy --; ``both`` uses the two together.  Without ``--hold_motif`` nothing is held and the run is
``sampling.guide_inpaint`` with nothing fixed.  The report then also holds ``template_energy``, ``template_rmsd`` and
``template_mirror_rmsd`` (the fit of the template reflected in z: below ``template_rmsd`` means the wrong hand came out).
Without the flag the script does what it did before it.
"""
import argparse
import json
import logging
import os
import sys
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEED = 7344   # bin/sample.py's default


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-m", "--model", type=str, required=True,
                        help="Path to model directory: training_args.json, config.json and a models folder at a minimum")
    parser.add_argument("--outdir", "-o", type=str, default=os.getcwd(), help="Path to output directory")
    parser.add_argument("--num", "-n", type=int, default=10, help="Number of backbones to generate")
    parser.add_argument("--length", "-l", type=int, required=True, help="residues in every backbone")
    parser.add_argument("--contacts", type=str, default=None, help="file of residue pairs to bring into contact: i j [max_dist]")
    parser.add_argument("--motif_pdb", type=str, default=None, help="PDB file the motif's residues are taken from")
    parser.add_argument("--motif_residues", type=str, default=None, help="residues of the file by position, e.g. 3-9,20-27")
    parser.add_argument("--placed_at", type=str, default=None, help="per range, the index its first residue takes, e.g. 10,40")
    parser.add_argument("--hold_motif", action="store_true",
                        help="hold every range of --motif_residues by replacement and restrain across ranges only")
    parser.add_argument("--clash_weight", type=float, default=None, help="weight of the soft clash term inside the guided run")
    parser.add_argument("--placement", type=str, default=None, choices=("distances", "template", "both"),
                        help="what places the motif: its pair distances (default), a superposition restraint, or both")
    parser.add_argument("--template_weight", type=float, default=1.0, help="weight of every atom of the superposition restraint")
    parser.add_argument("--scale", type=float, default=1.0, help="guidance scale; 0 is the unguided sampler")
    parser.add_argument("--max_norm", type=float, default=1.0, help="clip of a backbone's gradient norm")
    parser.add_argument("--guide_from", type=int, default=None, help="guide only the visits at or below this timestep (default: all)")
    parser.add_argument("--weight", type=float, default=1.0, help="weight of every restraint")
    parser.add_argument("--num_steps", type=int, default=None, help="network evaluations per backbone (default: every timestep)")
    parser.add_argument("--eta", type=float, default=1.0, help="noise of the strided update, [0, 1]; 1 = the ancestral update of the respaced chain")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Batch size to use when sampling")
    parser.add_argument("--seed", type=int, default=SEED, help="Random seed")
    parser.add_argument("--device", type=str, default="cuda:0", help="Device to use")
    return parser


def read_contacts(fname: str):
    pairs = []
    with open(fname) as source:
        for n, line in enumerate(source, 1):
            words = line.split("#", 1)[0].split()
            if not words:
                continue
            if len(words) not in (2, 3):
                raise ValueError(f"{fname}:{n}: expected 'i j [max_dist]', got {line.strip()!r}")
            pairs.append((int(words[0]), int(words[1])) + ((float(words[2]),) if len(words) == 3 else ()))
    return pairs


def parse_ranges(text: str):
    """'3-9,20-27' -> [[3 .. 9], [20 .. 27]]; a single number is a range of one."""
    out = []
    for part in text.split(","):
        lo, _, hi = part.strip().partition("-")
        lo, hi = int(lo), int(hi) if hi else int(lo)
        if lo < 0 or hi < lo:
            raise ValueError(f"range {part!r}: first <= last, both >= 0")
        out.append(list(range(lo, hi + 1)))
    return out


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.num < 1 or args.length < 1:
        parser.error(f"-n {args.num} -l {args.length}: both at least 1")
    motif_args = (args.motif_pdb, args.motif_residues, args.placed_at)
    if any(a is not None for a in motif_args) and any(a is None for a in motif_args):
        parser.error("--motif_pdb, --motif_residues and --placed_at go together")
    if args.hold_motif and args.motif_pdb is None:
        parser.error("--hold_motif holds the ranges of a motif: give --motif_pdb, --motif_residues and --placed_at")
    if args.clash_weight is not None and not args.clash_weight >= 0:
        parser.error(f"--clash_weight {args.clash_weight} must be >= 0")
    with_template = args.placement in ("template", "both")
    if with_template and args.motif_pdb is None:
        parser.error(f"--placement {args.placement} places a motif: give --motif_pdb, --motif_residues and --placed_at")
    if not (args.template_weight > 0 and args.template_weight < float("inf")):
        parser.error(f"--template_weight {args.template_weight} must be > 0 and finite")
    if args.contacts is None and args.motif_pdb is None:
        parser.error("nothing to aim at: give --contacts and / or a motif")
    outdir = Path(args.outdir)
    if not os.path.isdir(args.model):
        raise AssertionError(f"{args.model} is not a local model directory")
    with open(Path(args.model) / "training_args.json") as source:
        training_args = json.load(source)
    if args.length > min(int(training_args["max_seq_len"]), 2048):
        parser.error(f"--length {args.length} does not fit the model's padded length {training_args['max_seq_len']} (at most 2048)")

    import numpy as np

    from foldingdiff_amd import structures

    restraints, motif_ca, placed, segments, file_xyz, template = None, None, None, None, None, None
    try:
        if args.contacts is not None:
            restraints = structures.contact_restraints(read_contacts(args.contacts), weight=args.weight)
        if args.motif_pdb is not None:
            ranges = parse_ranges(args.motif_residues)
            starts = [int(v) for v in args.placed_at.split(",")]
            if len(starts) != len(ranges):
                raise ValueError(f"--placed_at has {len(starts)} entries for {len(ranges)} ranges")
            picked = [r for rng in ranges for r in rng]
            placed = [s + k for rng, s in zip(ranges, starts) for k in range(len(rng))]
            bb = structures.read_backbone(args.motif_pdb)
            if bb is None:
                raise ValueError(f"{args.motif_pdb}: no usable backbone")
            xyz = bb[0].astype(np.float64).reshape(-1, 3, 3)
            if max(picked) >= len(xyz):
                raise ValueError(f"{args.motif_pdb} has {len(xyz)} residues, --motif_residues asks for residue {max(picked)}")
            motif = xyz[picked].reshape(-1, 3)
            motif_ca = xyz[picked, 1]
            if args.hold_motif:   # (the ranges of the file are the segments; sampling.scaffold_segments repeats these checks)
                segments = [(rng[0], rng[-1] + 1, s) for rng, s in zip(ranges, starts)]
                file_xyz = xyz.reshape(-1, 3)
                m = structures.segment_restraints(file_xyz, segments, weight=args.weight)
            else:
                m = structures.motif_restraints(motif, placed, weight=args.weight)
            contacts = restraints
            if args.placement != "template":
                restraints = m if restraints is None else restraints + m
            if with_template:
                template = structures.motif_template(xyz.reshape(-1, 3), [(rng[0], rng[-1] + 1, s) for rng, s in zip(ranges, starts)],
                                                     weight=args.template_weight)
            if max(placed) >= args.length:
                raise ValueError(f"the motif is placed up to residue {max(placed)}, --length is {args.length}")
        if restraints is not None and restraints.min_length() > args.length:
            raise ValueError(f"the restraints need {restraints.min_length()} residues, --length is {args.length}")
    except ValueError as e:
        parser.error(str(e))
    if os.path.isdir(outdir) and os.listdir(outdir):
        raise AssertionError(f"Expected {outdir} to be empty!")

    import pandas as pd
    import torch

    from foldingdiff_amd import modelling, sampling
    from foldingdiff_amd.angles_and_coords import write_preds_pdb_folder
    from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset

    train_dset = NoisedAnglesDataset(   # the data-free dataset shell of bin/sample.py
        dset=AnglesEmptyDataset.from_dir(args.model), dset_key="angles", timesteps=training_args["timesteps"], exhaustive_t=False,
        beta_schedule=training_args["variance_schedule"], nonangular_variance=1.0, angular_variance=training_args["variance_scale"])
    os.makedirs(outdir, exist_ok=True)
    device = torch.device(args.device)
    model = modelling.BertForDiffusionBase.from_dir(args.model, copy_to=str(outdir / "model_snapshot")).to(device)
    torch.manual_seed(args.seed)
    names = train_dset.feature_names["angles"]
    guide_args = dict(num_steps=args.num_steps, eta=args.eta, scale=args.scale, max_norm=args.max_norm, guide_from=args.guide_from,
                      batch_size=args.batchsize)
    lengths = [args.length] * args.num
    if args.hold_motif:
        feats = structures.featurize([args.motif_pdb], distances=[n for n in names if n.count(":") == 1],
                                     angles=[n for n in names if n.count(":") != 1], device=device.index or 0)[0]
        if feats is None:
            raise AssertionError(f"{args.motif_pdb}: no usable backbone")
        motif_angles = feats[list(names)].values.astype(np.float32)
        if not np.isfinite(motif_angles[picked]).all():
            raise AssertionError(f"--motif_residues of {args.motif_pdb} hold an undefined angle (a chain end?)")
        sampled, info = sampling.scaffold_segments(model, train_dset, motif_angles, file_xyz, segments, lengths, restraints=contacts,
                                                   restraint_weight=args.weight, clash_weight=args.clash_weight or 0.0,
                                                   **(dict(placement=args.placement, template_weight=args.template_weight) if with_template else {}),
                                                   **guide_args)
    elif args.clash_weight is not None or with_template:   # guidance with the clash term or a template and nothing held
        free = [np.full((args.length, len(names)), np.nan, dtype=np.float32)] * args.num
        sampled, info = sampling.guide_inpaint(model, train_dset, free, [np.zeros(args.length, dtype=bool)] * args.num, restraints,
                                               clash_weight=args.clash_weight or 0.0, **(dict(templates=template) if with_template else {}),
                                               **guide_args)
    else:
        sampled, info = sampling.guide(model, train_dset, lengths, restraints, **guide_args)
    sampled_dfs = [pd.DataFrame(s, columns=names) for s in sampled]
    sampled_angles_folder = outdir / "sampled_angles"
    os.makedirs(sampled_angles_folder, exist_ok=True)
    logging.info(f"Writing sampled angles to {sampled_angles_folder}")
    for i, s in enumerate(sampled_dfs):
        s.to_csv(sampled_angles_folder / f"generated_{i}.csv.gz")
    coords = []
    pdb_files = write_preds_pdb_folder(sampled_dfs, str(outdir / "sampled_pdb"), device=device.index or 0, coords_out=coords)
    kept = [i for i, (f, xyz) in enumerate(zip(pdb_files, coords)) if f and xyz is not None]
    report = {"settings": vars(args), "length": args.length, "n_restraints": 0 if restraints is None else len(restraints),
              "energy": {os.path.basename(pdb_files[i]): float(info["energy"][i]) for i in kept},
              "max_violation": {os.path.basename(pdb_files[i]): float(info["max_violation"][i]) for i in kept}}
    if "clash_energy" in info:
        report["clash_energy"] = {os.path.basename(pdb_files[i]): float(info["clash_energy"][i]) for i in kept}
    if with_template:
        for key in ("template_energy", "template_rmsd"):
            report[key] = {os.path.basename(pdb_files[i]): float(info[key][i]) for i in kept}
        _, mirrored = structures.template_energy([coords[i] for i in kept], template, device=device.index or 0, mirror=True)
        report["template_mirror_rmsd"] = {os.path.basename(pdb_files[i]): float(r) for i, r in zip(kept, mirrored)}
    if motif_ca is not None:
        ca_rows = [3 * p + 1 for p in placed]
        rmsd = structures.superposed_rmsd([coords[i][ca_rows] for i in kept], [motif_ca] * len(kept), device=device.index or 0)
        report["motif_ca_rmsd"] = {os.path.basename(pdb_files[i]): float(r) for i, r in zip(kept, rmsd)}
    with open(outdir / "restraints.json", "w") as sink:
        json.dump(report, sink, indent=4)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
