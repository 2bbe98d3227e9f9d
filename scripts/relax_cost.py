#!/usr/bin/env python3
"""
What the torsion-space relaxer costs: the kernel times of ``fd_nerf`` (one lane per chain) and ``fd_nerf_scan`` (one
workgroup per chain) in the same run on the same box, and the time of one ``fd_relax`` iteration split by launch, at
B = 512, L = 128 and at B = 8, L = 128 (torsions only, uniformly random phi / psi, omega = pi).

Run without arguments it starts, per size, ONE child under ``rocprofv3 --kernel-trace --stats`` with a time limit, reads the
child's kernel trace and host-clock figures, and writes ``profiles/relax_cost.json``; a child that fails or runs out of time
ends the script there.  ``--child B L`` is what the child runs: a warm-up of each entry, then ``fd_nerf`` and
``fd_nerf_scan`` ``--reps`` times each and ``fd_relax`` with 0 and with ``--iters`` iterations (their host-clock difference
over ``--iters`` is an iteration without the upload, the download and the allocations).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

KERNELS = ("nerf_kernel", "nerf_scan_kernel", "restraint_kernel", "soft_clash_kernel", "nerf_vjp_kernel", "relax_step_kernel")
ITERATION = KERNELS[1:]


def child(B, L, reps, iters):
    import ctypes as C

    import numpy as np

    from foldingdiff_amd import _binding
    rng = np.random.default_rng(B)
    feats = np.concatenate([rng.uniform(-np.pi, np.pi, (B, L, 2)), np.full((B, L, 1), np.pi)], axis=2).astype(np.float32)
    lens = np.full(B, L, dtype=np.int32)
    idx = np.array([0, 1, 2, -1, -1, -1, -1, -1, -1], dtype=np.int32)
    lib, P = _binding.load(), _binding.ptr
    coords = np.empty((B, 3 * L, 3))
    prm = _binding.FdRelaxParams()
    for k in range(9):
        prm.feat_idx[k] = int(idx[k])
    for f in range(3):
        prm.is_angle[f] = prm.move[f] = 1
    prm.clash_alpha, prm.clash_margin, prm.w_clash, prm.w_tether = 0.63, 0.15, 1.0, 0.0
    prm.step0, prm.grow, prm.shrink, prm.max_step = 0.01, 1.2, 0.5, 0.5
    offs = np.zeros(B + 1, dtype=np.int32)
    out, energy, accepted = np.empty_like(feats), np.empty((B, 3)), np.empty(B, dtype=np.int32)

    def relax(n):
        t0 = time.perf_counter()
        _binding.check(lib.fd_relax(0, P(feats), None, P(lens), B, L, 3, C.byref(prm), None, P(offs), None, None, None, None, None, n, None,
                                    P(out), P(energy), None, P(accepted)))
        return time.perf_counter() - t0

    def build(entry):
        t0 = time.perf_counter()
        _binding.check(entry(0, P(feats), P(lens), B, L, 3, P(idx), 0, P(coords)))
        return time.perf_counter() - t0

    build(lib.fd_nerf), build(lib.fd_nerf_scan), relax(1)                  # warm-up
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    serial = [build(lib.fd_nerf) for _ in range(reps)]
    scan = [build(lib.fd_nerf_scan) for _ in range(reps)]
    t_zero = [relax(0) for _ in range(reps)]
    t_full = [relax(iters) for _ in range(reps)]
    print("RELAX_COST " + json.dumps({"B": B, "L": L, "reps": reps, "iters": iters, "fd_nerf_call_ms": 1e3 * med(serial),
                                      "fd_nerf_scan_call_ms": 1e3 * med(scan), "fd_relax_0_call_ms": 1e3 * med(t_zero),
                                      "fd_relax_call_ms": 1e3 * med(t_full), "host_us_per_iteration": 1e6 * (med(t_full) - med(t_zero)) / iters,
                                      "accepted_mean": float(accepted.mean()), "clash_energy_mean_after": float(energy[:, 0].mean())}))


def kernel_times(trace_dir):
    """{kernel: {"calls", "median_us", "min_us"}} from the child's kernel trace."""
    durations = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                key = next((k for k in KERNELS if f"::{k}(" in name or f" {k}(" in name or name.startswith(k)), None)
                if key is None:
                    key = next((k for k in sorted(KERNELS, key=len, reverse=True) if k in name), None)
                if key:
                    durations.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "median_us": sorted(v)[len(v) // 2], "min_us": min(v)} for k, v in durations.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", type=int, nargs=2, default=None, metavar=("B", "L"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "relax_cost.json"))
    args = ap.parse_args(argv)
    if args.child:
        return child(args.child[0], args.child[1], args.reps, args.iters)
    results = []
    for B, L in ((512, 128), (8, 128)):
        with tempfile.TemporaryDirectory() as td:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "relax", "--", sys.executable,
                   os.path.abspath(__file__), "--child", str(B), str(L), "--reps", str(args.reps), "--iters", str(args.iters)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:
                sys.exit(f"the child for B={B} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RELAX_COST "))
            res = json.loads(line[len("RELAX_COST "):])
            res["kernels"] = kernel_times(td)
        k = res["kernels"]
        res["iteration_us_by_launch"] = {name: k[name]["median_us"] for name in ITERATION if name in k}
        res["iteration_us_kernels"] = sum(res["iteration_us_by_launch"].values())
        if "nerf_kernel" in k and "nerf_scan_kernel" in k:
            res["nerf_kernel_over_scan"] = k["nerf_kernel"]["median_us"] / k["nerf_scan_kernel"]["median_us"]
        results.append(res)
        print(json.dumps(res), flush=True)
    with open(args.out, "w") as sink:
        json.dump({"sizes": results}, sink, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
