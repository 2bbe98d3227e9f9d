#!/usr/bin/env python3
"""
Sample protein backbones from a trained foldingdiff model on MI355X -- stand-in for the output stage of the
reference's ``bin/sample.py`` (same flags, same files):

    <outdir>/model_snapshot/                      copy of the model directory (from_dir(copy_to=...), :341-343)
    <outdir>/sampled_angles/generated_{i}.csv.gz  final angles of every sampled backbone (:360-368)
    <outdir>/sampled_pdb/generated_{i}.pdb        N-CA-C backbones built by NeRF on the device (:369, :105-128)
    with --fullhistory: sampled_angles/sample_history/generated_{i}/generated_{i}_timestep_{t}.csv.gz and
                        sampled_pdb/sample_history/generated_{i}/generated_{i}_timestep_{t}.pdb (:371-398)
    with --psea: plots/ss_cooccurrence_sampled.json  {generated_{i}.pdb: [n_alpha, n_beta]} of the final backbones and
                 plots/ss_cooccurrence_sampled.pdf   their 2-D histogram, when matplotlib is installed (:456-469)

    with --dssp: dssp.json  {generated_{i}.pdb: {"dssp": the DSSP label string, "n_hbonds": kept backbone hydrogen bonds,
                 "n_helix": runs of H, "n_strand": runs of E, "hbonds_per_residue": n_hbonds / residues}} of the final backbones,
                 oxygens placed on the device (structures.add_oxygens, structures.dssp: DESIGN.md 6t); without --dssp the
                 output tree is unchanged

    with --clashes: clash_counts.json               {generated_{i}.pdb: van der Waals clash count} of the final backbones
                    (structures.count_clashes on the coordinates as written: what bin/vdw_clashes.py gives on the files;
                    without --clashes the output tree is unchanged)

    with --relax N: relaxed_angles/generated_{i}.csv.gz, relaxed_pdb/generated_{i}.pdb and relax_report.json: the sampled
                    backbones after N iterations of the torsion-space relaxer (structures.relax: backbone clashes removed by a
                    descent on the angles; no force field); without --relax the output tree is unchanged

The secondary structures are annotated on the device (structures.count_secondary_structures: P-SEA, in place of
biotite's annotate_sse) from the coordinates of the backbones just written, without reading the files back.  The step
is opt-in: the reference runs it unless --nopsea is given, here it runs only with --psea, and without --psea the
output tree is what it was before the step existed; --nopsea is accepted and changes nothing.

What is NOT here (outside the sampler path): the angle-distribution plots (matplotlib / astropy) and the
--testcomparison statistics against the CATH test set (they need the dataset pipeline); --testcomparison therefore
raises.  The model must be a local directory
(no network): training_args.json, config.json, models/best_by_valid/*.ckpt [, training_mean_offset.npy].

One process per GPU under ``torchrun`` shards every batch over the GPUs (sampling.sample); rank 0 writes the files.
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

import pandas as pd  # noqa: E402
import torch  # noqa: E402

from foldingdiff_amd import modelling, sampling, structures  # noqa: E402
from foldingdiff_amd.angles_and_coords import coords_as_written, write_preds_pdb_folder  # noqa: E402
from foldingdiff_amd.datasets import AnglesEmptyDataset, NoisedAnglesDataset  # noqa: E402

# the value the reference's default seed expression (bin/sample.py:34-37) evaluates to
SEED = 7344


def build_datasets(model_dir: Path) -> NoisedAnglesDataset:
    """The data-free dataset shell of the reference's ``build_datasets(load_actual=False)`` (bin/sample.py:49-93)."""
    with open(model_dir / "training_args.json") as source:
        training_args = json.load(source)
    dset = AnglesEmptyDataset.from_dir(str(model_dir))
    return NoisedAnglesDataset(
        dset=dset,
        dset_key="coords" if training_args["angles_definitions"] == "cart-coords" else "angles",
        timesteps=training_args["timesteps"],
        exhaustive_t=False,
        beta_schedule=training_args["variance_schedule"],
        nonangular_variance=1.0,
        angular_variance=training_args["variance_scale"],
    )


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-m", "--model", type=str, required=True,
                        help="Path to model directory: training_args.json, config.json and a models folder at a minimum")
    parser.add_argument("--outdir", "-o", type=str, default=os.getcwd(), help="Path to output directory")
    parser.add_argument("--num", "-n", type=int, default=10, help="Number of examples to generate *per length*")
    parser.add_argument("-l", "--lengths", type=int, nargs=2, default=[50, 128], help="Range of lengths to sample from")
    parser.add_argument("-b", "--batchsize", type=int, default=512, help="Batch size to use when sampling")
    parser.add_argument("--fullhistory", action="store_true", help="Store full history, not just final structure")
    parser.add_argument("--testcomparison", action="store_true", help="(not available: needs the CATH data pipeline)")
    psea = parser.add_mutually_exclusive_group()
    psea.add_argument("--psea", action="store_true",
                      help="count the helices and strands of the sampled backbones (P-SEA on the device) into plots/ss_cooccurrence_sampled.json [.pdf]")
    psea.add_argument("--nopsea", action="store_true", help="accepted for compatibility: the P-SEA step runs only with --psea")
    parser.add_argument("--dssp", action="store_true",
                        help="label the sampled backbones with DSSP states from their backbone hydrogen bonds (on the device) into dssp.json")
    parser.add_argument("--clashes", action="store_true",
                        help="count the van der Waals clashes of the sampled backbones (on the device) into clash_counts.json")
    parser.add_argument("--relax", type=int, default=None, metavar="N",
                        help="relax the sampled backbones in torsion space for N iterations (on the device: backbone clashes are pushed apart "
                             "by a descent on phi / psi / omega; no force field) into relaxed_angles/, relaxed_pdb/ and relax_report.json")
    parser.add_argument("--num_steps", type=int, default=None,
                        help="sample in this many network evaluations on a strided schedule with the DDIM update (default: every timestep, "
                             "the reference's ancestral loop); the run's arguments then go to sampling_args.json")
    parser.add_argument("--eta", type=float, default=0.0,
                        help="with --num_steps: 0 = DDIM (deterministic given the start noise) .. 1 = the ancestral update of the respaced chain")
    parser.add_argument("--solver", type=str, default=None, choices=["ddim", "dpm2m"],
                        help="with --num_steps: the update of a visit, ddim (default) or dpm2m, a second-order multistep solver (needs --eta 0)")
    parser.add_argument("--spacing", type=str, default=None, choices=["uniform", "logsnr"],
                        help="with --num_steps: visits spaced evenly in t (default) or in log-SNR")
    parser.add_argument("--lambda_min", type=float, default=None,
                        help="with --spacing logsnr: the log-SNR below which the visits are not spread (default: the library's, -3)")
    parser.add_argument("--seed", type=int, default=SEED, help="Random seed")
    parser.add_argument("--device", type=str, default="cuda:0", help="Device to use")
    return parser


FEW_STEP_FLAGS = ("solver", "spacing", "lambda_min")   # passed on, and recorded, only when given


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.testcomparison:
        raise NotImplementedError("--testcomparison needs the CATH test split and the plotting stack, which are outside this path")
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    outdir = Path(args.outdir)
    # EVERY rank evaluates the same preconditions, before anything is created and before the process group exists; the verdicts
    # are then all-reduced so that either all ranks raise or none does (a rank that exits alone leaves the others blocked in
    # init_process_group / the first collective until the rendezvous or RCCL timeout)
    problem = ""
    if not os.path.isdir(args.model):
        problem = f"{args.model} is not a local model directory (there is no network access here)"
    elif os.path.isdir(outdir) and os.listdir(outdir):
        problem = f"Expected {outdir} to be empty!"  # Be extra cautious so we don't overwrite any results (bin/sample.py:299)
    if world > 1:
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        args.device = f"cuda:{local_rank}"
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(args.device))
        from foldingdiff_amd import distributed as fdist
        if fdist.any_rank_failed(bool(problem), device=torch.device(args.device)):
            dist.destroy_process_group()
            raise AssertionError(problem or "another rank failed its start-up checks (see its log)")
        if sampling.NOISE_MODE == "torch":
            # the reference's draw order needs every rank to draw the WHOLE batch's stream on one host thread: it reproduces the
            # single-process samples bit for bit, but it does not scale (12.6 GB of torch.randn per rank per batch of 4096 x 128)
            logging.warning("world size %d with the default noise mode 'torch': every rank draws the whole batch's noise on the host "
                            "(bit-identical to a single-process run, but it will not scale); set FOLDINGDIFF_AMD_NOISE=philox "
                            "for on-device noise keyed by the global sequence index", world)
    elif problem:
        raise AssertionError(problem)
    if rank == 0:
        os.makedirs(outdir, exist_ok=True)

    train_dset = build_datasets(Path(args.model))
    model = modelling.BertForDiffusionBase.from_dir(
        args.model, copy_to=str(outdir / "model_snapshot") if rank == 0 else "").to(torch.device(args.device))

    sweep_min_len, sweep_max_len = args.lengths
    assert sweep_min_len < sweep_max_len
    assert sweep_max_len <= train_dset.dset.pad

    few_step = {k: getattr(args, k) for k in FEW_STEP_FLAGS if getattr(args, k) is not None}
    torch.manual_seed(args.seed)
    sampled = sampling.sample(model, train_dset, n=args.num, sweep_lengths=(sweep_min_len, sweep_max_len),
                              batch_size=args.batchsize, final_only=not args.fullhistory, num_steps=args.num_steps, eta=args.eta,
                              **few_step)
    if rank == 0 and args.num_steps is not None:   # a strided run says so beside its samples; the solver's flags only when given
        with open(outdir / "sampling_args.json", "w") as sink:
            json.dump({k: v for k, v in vars(args).items() if k not in FEW_STEP_FLAGS or v is not None}, sink, indent=4)
    if rank == 0:
        names = train_dset.feature_names["angles"]
        sampled_dfs = [pd.DataFrame(s[-1], columns=names) for s in sampled]
        sampled_angles_folder = outdir / "sampled_angles"
        os.makedirs(sampled_angles_folder, exist_ok=True)
        logging.info(f"Writing sampled angles to {sampled_angles_folder}")
        for i, s in enumerate(sampled_dfs):
            s.to_csv(sampled_angles_folder / f"generated_{i}.csv.gz")
        final_coords = []
        pdb_files = write_preds_pdb_folder(sampled_dfs, str(outdir / "sampled_pdb"), coords_out=final_coords)
        if args.fullhistory:
            full_history_angles_dir = sampled_angles_folder / "sample_history"
            os.makedirs(full_history_angles_dir)
            full_history_pdb_dir = outdir / "sampled_pdb" / "sample_history"
            os.makedirs(full_history_pdb_dir)
            for i, sampled_series in enumerate(sampled):
                snapshot_dfs = [pd.DataFrame(snapshot, columns=names) for snapshot in sampled_series]
                ith_angle_dir = full_history_angles_dir / f"generated_{i}"
                os.makedirs(ith_angle_dir, exist_ok=True)
                for timestep, snapshot_df in enumerate(snapshot_dfs):
                    snapshot_df.to_csv(ith_angle_dir / f"generated_{i}_timestep_{timestep}.csv.gz")
                write_preds_pdb_folder(snapshot_dfs, str(full_history_pdb_dir / f"generated_{i}"),
                                       basename_prefix=f"generated_{i}_timestep_")
        if args.psea:
            # the reference annotates the files it has just written (make_ss_cooccurrence_plot over sampled_pdb/*.pdb,
            # bin/sample.py:456-469); the same three-decimal coordinates are taken from memory here
            plotdir = outdir / "plots"
            os.makedirs(plotdir, exist_ok=True)
            kept = [(os.path.basename(f), xyz) for f, xyz in zip(pdb_files, final_coords) if f]
            device_index = torch.device(args.device).index or 0
            counts = structures.count_secondary_structures([coords_as_written(xyz[1::3]) for _, xyz in kept], device=device_index)
            structures.write_ss_cooccurrence([name for name, _ in kept], counts, json_file=str(plotdir / "ss_cooccurrence_sampled.json"),
                                             outpdf=str(plotdir / "ss_cooccurrence_sampled.pdf"), title="Secondary structure co-occurrence, sampled")
        if args.dssp:
            # the three-decimal coordinates of the files just written, oxygens added on the device
            kept = [(os.path.basename(f), xyz) for f, xyz in zip(pdb_files, final_coords) if f]
            device_index = torch.device(args.device).index or 0
            chains = structures.add_oxygens([coords_as_written(xyz) for _, xyz in kept], device=device_index)
            labels = structures.dssp(chains, device=device_index)
            counts = structures.dssp_counts(chains, device=device_index)
            with open(outdir / "dssp.json", "w") as sink:
                json.dump({name: {"dssp": "".join(lab), "n_hbonds": int(c[0]), "n_helix": int(c[1]), "n_strand": int(c[2]),
                                  "hbonds_per_residue": int(c[0]) / len(lab)}
                           for (name, _), lab, c in zip(kept, labels, counts)}, sink, indent=4)
        if args.clashes:
            # what bin/vdw_clashes.py counts on the files just written: their three-decimal coordinates as float32
            kept = [(os.path.basename(f), xyz) for f, xyz in zip(pdb_files, final_coords) if f]
            device_index = torch.device(args.device).index or 0
            counts = structures.count_clashes([coords_as_written(xyz).astype("float32") for _, xyz in kept], device=device_index)
            with open(outdir / "clash_counts.json", "w") as sink:
                json.dump({name: int(c) for (name, _), c in zip(kept, counts)}, sink, indent=4)
        if args.relax is not None:
            device_index = torch.device(args.device).index or 0
            structures.relax_to_folder(sampled_dfs, [f"generated_{i}" for i in range(len(sampled_dfs))], str(outdir), device=device_index,
                                       n_iter=args.relax)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
