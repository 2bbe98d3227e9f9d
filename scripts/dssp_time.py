#!/usr/bin/env python3
"""
What oxygens plus DSSP cost next to P-SEA on the same chains, and how their labels compare.

Synthetic chains (tests/dssp_reference.segment_chain, 0.25 A noise): 512 chains of 128 residues, and one chain of 1024.
structures.add_oxygens (fd_backbone_oxygens), structures.dssp (fd_dssp, with and without the kept bonds) and
structures.annotate_sse (fd_annotate_sse, on the CA atoms of the same chains): the median of seven calls after a warm-up,
the host clock around the Python call (packing, uploads, the launch and the download).  Then the fractions of DSSP's H / E
and of P-SEA's a / b on the fixture files and on the synthetic set of tests/test_dssp_gpu.py.

Prints the JSON; ``--out FILE`` also writes it.
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import dssp_reference as dr  # noqa: E402
from foldingdiff_amd import structures  # noqa: E402

def med(fn, n=7):
    fn()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3

rng = np.random.default_rng(0)
out = {}
for name, chains in (("512x128", [dr.segment_chain(rng, 128, 0.25)[:, :3] for _ in range(512)]),
                     ("1x1024", [dr.segment_chain(rng, 1024, 0.25)[:, :3]])):
    with_o = structures.add_oxygens(chains)
    ca = [c[:, 1] for c in chains]
    out[name] = {"oxygens_ms": med(lambda: structures.add_oxygens(chains)),
                 "dssp_ms": med(lambda: structures.dssp(with_o)),
                 "dssp_with_bonds_ms": med(lambda: structures.dssp(with_o, return_hbonds=True)),
                 "psea_ms": med(lambda: structures.annotate_sse(ca))}
# label fractions on the test set of tests/test_dssp_gpu.py
SIZES = list(range(1, 10)) + [20, 46, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512]
NOISE = [0.0, 0.1, 0.25, 0.5]
rng = np.random.default_rng(0)
syn = [dr.segment_chain(rng, SIZES[k % len(SIZES)], NOISE[k % len(NOISE)]) for k in range(120)]
syn.append(dr.segment_chain(rng, 1024, 0.25))
fix = [os.path.join(REPO, "tests", "golden", f) for f in ("1CRN.pdb", "all_residues.pdb")]
for name, chains, labels in (("fixtures", [structures.read_backbone_atoms(f)[0] for f in fix], [structures.dssp_of_pdb(f) for f in fix]),
                             ("synthetic", syn, structures.dssp(syn))):
    d = "".join("".join(l) for l in labels)
    p = "".join("".join(l) for l in structures.annotate_sse([c[:, 1] for c in chains]))
    out[name] = {"residues": len(d), "dssp_H": d.count("H") / len(d), "dssp_HGI": sum(d.count(k) for k in "HGI") / len(d),
                 "dssp_E": d.count("E") / len(d), "psea_a": p.count("a") / len(p), "psea_b": p.count("b") / len(p),
                 "H_and_a": sum(x == "H" and y == "a" for x, y in zip(d, p)) / len(d),
                 "E_and_b": sum(x == "E" and y == "b" for x, y in zip(d, p)) / len(d)}
print(json.dumps(out, indent=1))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as sink:
        json.dump(out, sink, indent=1)
