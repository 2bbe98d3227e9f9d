#!/usr/bin/env python3
"""Golden fixture of the samplers' host side (tests/test_sampling_calls.py defines the scenarios and does the recording;
this script only writes the result down).  It needs neither a GPU nor the reference:

    python tests/golden/make_golden_sampling_calls.py

Written: sampling_calls.json -- scenario -> calls | draws | model | returned.  It holds no drawn value, so it does not depend
on the CPU it was written on.  Regenerate it only from a ``sampling.py`` whose behaviour is the one to keep."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_sampling_calls as calls  # noqa: E402

if __name__ == "__main__":
    with open(calls.GOLDEN, "w") as fh:   # one line per scenario
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, sort_keys=True, separators=(',', ':'))}"
                                    for k, v in sorted(calls.record_all().items())) + "\n}\n")
    print(f"{len(calls.SCENARIOS)} scenarios -> {calls.GOLDEN} ({os.path.getsize(calls.GOLDEN)} bytes)")
