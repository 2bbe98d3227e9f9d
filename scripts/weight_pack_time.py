#!/usr/bin/env python3
"""Host time of the weight packer (csrc/weight_pack.h) alone, through the test shim: every image fd_finalize packs for the
released shape (d_model 384, d_ff 768, max_position_embeddings 128), twelve layers' worth.  No GPU.

    python scripts/weight_pack_time.py [repeats]

Prints each repeat, the median and the spread (max - min) in milliseconds."""
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import weight_pack_cases as cases  # noqa: E402


def pack_model(p, layers, n_layers=12):
    for wqkv, wo, wi, wd, demb in layers[:n_layers]:
        d = wo.shape[0]
        p.tiles(wqkv[:2 * d]); p.tiles(wqkv[2 * d:]); p.tiles(wqkv)
        p.seq_attn(wqkv); p.seq_attn16(wqkv)
        p.split(demb)
        p.tiles(wo); p.tiles(wi); p.tiles(wd)
        p.ffn16(wi, wd, wo)


if __name__ == "__main__":
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    d, ff = 384, 768
    layers = [(cases.weights(10 * li, 3 * d, d), cases.weights(10 * li + 1, d, d), cases.weights(10 * li + 2, ff, d),
               cases.weights(10 * li + 3, d, ff), cases.weights(10 * li + 4, 255, 32)) for li in range(12)]
    with tempfile.TemporaryDirectory() as td:
        p = cases.load_packer(td)
        pack_model(p, layers, 1)   # warm: page in the library
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pack_model(p, layers)
            ms.append((time.perf_counter() - t0) * 1e3)
    print("repeats (ms):", " ".join(f"{t:.1f}" for t in ms))
    print(f"median {statistics.median(ms):.1f} ms, spread {max(ms) - min(ms):.1f} ms")
