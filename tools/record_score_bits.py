"""Records tests/golden/g13_score_bits.json: the float64 bits `driver.frame_metrics` and `driver.frame_msssim` return on the device for
the cases of tests/_score_cases.py, each beside the SHA-256 of its input bytes.  tests/test_gpu_score_bits.py asserts these bits.

The file pins what the kernels computed BEFORE a change to them: run this in a checkout of the commit the change starts from (it needs
only the two driver calls and tests/_score_cases.py, which may be copied there), commit the file, and never record it from the code
under test.

    python tools/record_score_bits.py [--out tests/golden/g13_score_bits.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import _score_cases as C

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g13_score_bits.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
cases = {}
for case in C.BIT_CASES:
    sha, bits = C.bit_case(*case)
    cases[C.bit_case_key(*case)] = {"input_sha256": sha, "bits": bits}
with open(args.out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
    f.write("\n")
print(f"{len(cases)} cases -> {args.out}")
