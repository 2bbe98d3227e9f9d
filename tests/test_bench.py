"""bench.py --dump-outputs: what the last timed pass computed, written for output-by-output comparison of two builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import REPO


def test_dump_outputs_fits_the_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    g = torch.Generator().manual_seed(0)
    hist = torch.randn(100, 64, 32, 6, generator=g)   # [T, B, L, F]: 4.9 MB, over the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), hist[-1], hist)
    a = {f: np.load(tmp_path / "a" / f) for f in ("final_angles.npy", "history_sample.npy")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 1 << 20
    assert np.array_equal(a["final_angles.npy"], hist[-1].numpy())   # fits: whole
    s = a["history_sample.npy"]
    assert s.shape[0] == 100 and 0 < s.shape[1] < 64 and s.shape[2:] == (32, 6)
    # every sampled sequence is one of the history's, in increasing order, and the choice repeats
    full = hist.numpy()
    idx = [next(j for j in range(64) if np.array_equal(s[:, i], full[:, j])) for i in range(s.shape[1])]
    assert idx == sorted(set(idx))
    for f, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "c"), hist[-1], None)          # --no-history: the final states only
    assert sorted(os.listdir(tmp_path / "c")) == ["final_angles.npy"]


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_pass(gpu, tmp_path):
    """Two runs that differ only in the number of warm-up passes write the same files, bit for bit: the inputs and the last timed pass
    depend on the arguments alone.  The JSON line reports the requested number of timed steps and the time of one."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--timesteps", "20", "--batch", "64",
           "--no-cpu-baseline", "--no-exact-f32", "--no-c5-extra", "--no-traffic"]
    dumps = []
    for w in (0, 1):
        d = tmp_path / f"warmup{w}"
        r = subprocess.run(cmd + ["--warmup", str(w), "--dump-outputs", str(d)], cwd=REPO, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["final_angles.npy", "history_sample.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 10**6
        dumps.append({f: np.load(d / f) for f in os.listdir(d)})
    fin, hist = dumps[0]["final_angles.npy"], dumps[0]["history_sample.npy"]
    assert fin.dtype == np.float32 and fin.shape == (64, 128, 6) and hist.shape == (20, 64, 128, 6)
    assert np.isfinite(hist).all() and np.array_equal(hist[-1], fin)
    for f, v in dumps[0].items():
        assert np.array_equal(v, dumps[1][f]), f


@pytest.mark.gpu
def test_plain_run_leaves_the_extra_legs_to_full(gpu):
    """At the headline's shape (C2, one GPU) a plain run prints the headline and what its timed region measured, and nothing that
    takes runs of its own; --full adds exact_f32_mode and the extras.  (T = 200: the small-batch leg starts at t = 199.)"""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--timesteps", "200"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-traffic"])):
        r = subprocess.run(cmd + extra, cwd=REPO, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines[name] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["metric"] == "backbones/sec (L=128, T=200, bs=512)" and line["unit"] == "backbones/s" and line["higher_is_better"]
        assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["kernels"] and line["roofline"]["achieved"] > 0 and line["roofline"]["traffic"] is None
    assert not {"exact_f32_mode", "extras", "cpu_baseline"} & set(plain)
    assert full["exact_f32_mode"]["value"] > 0 and "cpu_baseline" not in full
    assert sorted(full["extras"]) == ["c3", "c5", "host_entry", "nerf", "small_batch"]
