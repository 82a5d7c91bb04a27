"""tests/_resize_ref.py (the float64 restatement the device tests of libvsr_hip_resize.so compare with) against torch's own antialiased
`interpolate` on the CPU in float64, and the properties of the tables the device tests rely on.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resize_ref as R

GEOMS = [(48, 64, 12, 16), (45, 63, 15, 21), (44, 60, 22, 30), (37, 53, 12, 16), (12, 16, 48, 64), (15, 21, 45, 63), (13, 17, 26, 34)]
BAR = 1e-10   # three orders above the 2.9e-13 a float64 evaluation differs by on 0..255 data; one float32 unit at 255 is 1.5e-5


@pytest.mark.parametrize("kernel", ["bicubic", "bilinear"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_float64_evaluation_equals_torch_antialiased_interpolate(geom, kernel):
    H, W, h, w = geom
    x = np.random.RandomState(H * 100 + W).uniform(0.0, 255.0, size=(2, H, W, 3))
    yf, yw, _ = R.tables64(H, h, kernel)
    xf, xw, _ = R.tables64(W, w, kernel)
    got, _ = R.resize64(x, xf, xw, yf, yw, want_bound=False)
    want = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(h, w), mode=kernel, antialias=True, align_corners=False)
    err = float(np.abs(got - want.permute(0, 2, 3, 1).numpy()).max())
    print(f"[{kernel} {geom}] max |float64 restatement - torch| = {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("kernel", ["bicubic", "bilinear"])
@pytest.mark.parametrize("n_in,n_out", [(64, 16), (63, 21), (60, 30), (53, 16), (16, 64), (21, 63), (17, 34), (11, 11), (7, 1), (3, 1), (2, 8),
                                         (128, 16)])
def test_table_rows_sum_to_one_and_windows_cover_their_span(n_in, n_out, kernel):
    first, weight, spans = R.tables64(n_in, n_out, kernel)
    f32, w32 = R.tables(n_in, n_out, kernel)
    K = weight.shape[1]
    assert K == 2 * int(np.ceil(R.SUPPORT[kernel] * max(n_in / n_out, 1.0))) + 1 and K <= 33
    assert np.array_equal(f32, first) and w32.dtype == np.float32 and f32.dtype == np.int32
    assert np.abs(w32.astype(np.float64).sum(axis=1) - 1.0).max() <= 2 * R.U * K
    for i, (lo, hi) in enumerate(spans):
        assert first[i] == lo and 0 <= lo < hi <= n_in and hi - lo <= K       # the window first .. first + K - 1 covers [lo, hi)
        assert (weight[i, hi - lo:] == 0).all()                               # ... and its unused trailing taps carry weight 0


def test_bound_and_quantise_and_excuse():
    rs = np.random.RandomState(3)
    x = rs.uniform(0, 255, size=(1, 20, 24, 3)).astype(np.float32)
    yf, yw = R.tables(20, 5)
    xf, xw = R.tables(24, 6)
    ref, bound = R.resize64(x, xf, xw, yf, yw)
    assert ref.shape == bound.shape == (1, 5, 6, 3) and (bound > 0).all()
    # of the order of (17 + 17) u times the absolute sum: below 1e-3 on 0..255 data, above one float64 unit by far
    assert bound.max() < 1e-3 and bound.min() > 1e-7
    assert R.gamma(17) == 17 * R.U / (1 - 17 * R.U)
    assert R.quantise64(np.array([-3.0, np.nan, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0])).tolist() == [0, 0, 0, 2, 2, 254, 255, 255]
    ex = R.excused(np.array([10.5, 10.5001, 10.4, 0.0, 255.0, 128.0, -4.0, 255.5]), 1e-3)
    assert ex.tolist() == [True, True, False, True, True, False, False, False]


def test_exact_case_stays_inside_its_budget_and_refuses_to_leave_it():
    case = R.exact_case(np.random.RandomState(0), 2, 9, 11, 5, 7, 5, 3)
    assert case["ref"].shape == (2, 5, 7, 3)
    assert (case["ref"] * 256 == np.rint(case["ref"] * 256)).all()            # multiples of 2^-8
    assert (case["ref"].astype(np.float32).astype(np.float64) == case["ref"]).all()
    assert case["xf"].min() < 0 and case["xf"].max() >= 11                     # the clamp acts on both sides
    with pytest.raises(R.BudgetError):
        R.exact_case(np.random.RandomState(0), 1, 600, 8, 4, 4, 33, 33, density=1.0)   # |sum| of 33 x 33 full taps leaves 2^16
