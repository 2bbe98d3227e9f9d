#!/usr/bin/env python3
"""Golden fixture of the weight packer (tests/weight_pack_cases.py defines the inputs and does the recording; this script only
writes the result down).  It needs the ROCm clang++ and neither a GPU nor the reference:

    python tests/golden/make_golden_weight_images.py

Written: weight_images.json -- image name -> SHA-256 of its bytes (little-endian halves), its length and its scale(s).
Regenerate it only from a ``csrc/weight_pack.h`` whose bytes are the ones to keep: the file in git was written from the packing
functions as they stood in api.hip, moved without a change."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import weight_pack_cases as cases  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as td:
        rec = cases.record_all(cases.load_packer(td))
    with open(cases.GOLDEN, "w") as fh:   # one line per image
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, sort_keys=True, separators=(',', ':'))}"
                                    for k, v in sorted(rec.items())) + "\n}\n")
    print(f"{len(rec)} images -> {cases.GOLDEN} ({os.path.getsize(cases.GOLDEN)} bytes)")
