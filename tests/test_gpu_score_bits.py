"""The float64 bits of driver.frame_metrics and driver.frame_msssim against tests/golden/g13_score_bits.json, recorded on an MI355X by
tools/record_score_bits.py at the commit before csrc/frame_ssim.h gathered the SSIM window march of the two kernels in one place.

Equality of bits, no tolerance: both sources are built without contraction, every fma is asked for by name and double division is
correctly rounded, so the same operations in the same order give the same bits.  A case that differs means an operation or its order
changed in the kernels: the file is not to be recorded again from the code under test.  Each case carries the SHA-256 of its input
bytes, so a drift of the inputs (tests/_metric_ref.py, the seeding rule) is reported as that.  The cases (tests/_score_cases.py) are
the smallest shapes of tests/test_gpu_metric.py and tests/test_gpu_msssim.py that reach each branch of the march."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import _score_cases as C  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_score_bits.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(C.bit_case_key(*case) for case in C.BIT_CASES) and len(GOLDEN) == 52


@pytest.mark.parametrize("case", C.BIT_CASES, ids=lambda case: C.bit_case_key(*case).replace(" ", "-"))
def test_the_bits_are_the_recorded_ones(case):
    want = GOLDEN[C.bit_case_key(*case)]
    sha, bits = C.bit_case(*case)
    assert sha == want["input_sha256"], "the INPUT bytes differ from the recorded ones (not the kernels)"
    assert bits == want["bits"]
