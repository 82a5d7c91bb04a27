"""tests/_flow_ref.py (the references tests/test_gpu_exact_flow.py judges csrc/flow_ops.hip and csrc/flow_ops_bwd.hip by) checked before
they judge a kernel: each formula reference against float64 autograd over the differentiable restatements -- bit for bit on the exact
operands, within float64 rounding on Gaussian ones --, the correlation against the project's C checker, the budget checks on constructed
over-budget cases, the operand generators' border assertions, and two planted defects read back from `_exact.assert_exact`'s message.
No GPU."""
import numpy as np
import pytest
import torch

import _exact as E
import _flow_ref as R

RESAMPLE_SHAPES = [(1, 1, 1, 1), (2, 3, 17, 29), (1, 5, 7, 301), (3, 2, 5, 1)]   # those of test_gpu_exact_flow.py
# (the autograd comparison leaves out the one large map, FlowNetC's geometry at 48 x 64 with 256 channels: the same geometry runs at 8 x 16)
SMALL_CORR = [i for i, (shape, g) in enumerate(R.CORR_CASES) if int(np.prod(shape)) * (2 * (g["max_displacement"] // g["stride2"]) + 1) ** 2 < 3e7]
F64 = 1e-12   # float64 rounding of sums of a few thousand O(1) terms (2^-53 each), relative to the largest magnitude: 4 orders of margin


def _leaf(t):
    return torch.as_tensor(t).detach().to(torch.float64).clone().requires_grad_(True)


def _autograd_resample(img, flow, gout, bilinear):
    i, f = _leaf(img), _leaf(flow)
    R.ref_resample2d(i, f, bilinear).backward(torch.as_tensor(gout, dtype=torch.float64))
    return i.grad, f.grad


def _autograd_corr(f1, f2, gout, geom):
    a, b = _leaf(f1), _leaf(f2)
    out = R.ref_correlation(a, b, geom["pad_size"], geom["max_displacement"], geom["stride1"], geom["stride2"])
    out.backward(gout)
    return out.detach(), a.grad, b.grad


def _same64(got, want, what):
    assert got.dtype == torch.float64 and want.dtype == torch.float64
    E.assert_exact(got, want, what)


def _near64(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"[{what}] max |reference - autograd| = {err:.3e} on a range of {scale:.3e}")
    assert err <= F64 * scale


# ---------------------------------------------------------------------------------------------------------------- Resample2d
@pytest.mark.parametrize("bilinear", [True, False])
@pytest.mark.parametrize("shape", RESAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resample2d_reference_equals_autograd_on_exact_operands(shape, bilinear):
    """Near flows, and the same with the three far ones on top (1e9, -1e9, 3e10: autograd clamps in float64 before it converts, the
    reference converts with saturation and then clamps; both must pick the border)."""
    for far in (False, True):
        c = R.resample_case(sum(shape), shape, far=far)
        d_img, d_flow = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"], bilinear)
        a_img, a_flow = _autograd_resample(c["img"], c["flow"], c["gout"], bilinear)
        _same64(d_img, a_img, f"d_img {shape} bilinear={bilinear} far={far}")
        if bilinear:
            _same64(d_flow, a_flow, f"d_flow {shape} far={far}")
        else:
            assert a_flow is None and not bool(d_flow.any())
        # every value the kernel must produce is a float32 value
        E.check_storable(d_img, torch.float32, "d_img")
        E.check_storable(d_flow, torch.float32, "d_flow")


def test_resample2d_generator_hits_every_border_and_the_interior():
    """The generators' own assertions (each border, each axis' interior, the interior) pass for every shape the GPU file uses, the share
    per border is of the size the generator promises, and k = 4 puts the nearest build's xf + 0.5 on integers."""
    for shape in RESAMPLE_SHAPES + [(2, 2, 521, 1009)]:
        c = R.resample_case(sum(shape), shape, mag=4 if shape[2] > 500 else None, far=shape[2] < 500)
        h = c["hits"]
        print(f"[resample_case {shape}] " + ", ".join(f"{k} {v}" for k, v in h.items()))
        B, C, H, W = shape
        if H >= 3 and W >= 3:
            assert min(h["left"], h["right"], h["top"], h["bottom"]) >= 1 and h["interior"] >= h["n"] // 4
        if W == 1:
            assert h["in_x"] == 0 and h["left"] + h["right"] >= h["n"]      # a one-pixel axis: every sample clamps
    c = R.resample_case(46, (2, 3, 17, 29))
    h = c["hits"]
    for side, n, m in (("left", 29, 9), ("right", 29, 9), ("top", 17, 5), ("bottom", 17, 5)):
        share, expect = h[side] / h["n"], m / (4.0 * n)
        assert 0.5 * expect <= share <= 2.0 * expect, (side, share, expect)
    x = np.arange(29, dtype=np.float32).reshape(1, 1, 29) + c["flow"][:, 0]
    on_half = (x - np.floor(x)) == 0.5
    assert on_half.any() and np.array_equal((x + np.float32(0.5))[on_half], np.floor(x + np.float32(0.5))[on_half])
    far = R.resample_case(46, (2, 3, 17, 29), far=True)["flow"]
    assert sorted(float(v) for v in far[np.abs(far) > 1e8]) == sorted(float(np.float32(v)) for v in R.FAR)


@pytest.mark.parametrize("bilinear", [True, False])
def test_resample2d_reference_agrees_with_autograd_on_gaussian_operands(bilinear):
    rs = np.random.RandomState(3)
    shape = (2, 3, 17, 29)
    img, gout = rs.randn(*shape), rs.randn(*shape)
    flow = (rs.randn(2, 2, 17, 29) * 6).astype(np.float32)
    d_img, d_flow = R.resample2d_grads_ref(img, flow, gout, bilinear, check=False)
    a_img, a_flow = _autograd_resample(img, flow, gout, bilinear)
    _near64(d_img, a_img, f"d_img bilinear={bilinear}")
    if bilinear:
        # `ref_resample2d` forms x + flow in float32, so autograd hands the flow gradient back through a float32 cast: ONE rounding to float32
        # per element (half a unit, 2^-24 relative) on top of the float64 noise -- the autograd side's, not the reference's
        err = (d_flow - a_flow).abs()
        print(f"[d_flow] max |reference - autograd| = {float(err.max()):.3e} on a range of {float(a_flow.abs().max()):.3e}")
        assert a_flow.dtype == torch.float64 and torch.equal(a_flow, a_flow.float().double())      # it IS float32-rounded
        assert bool((err <= d_flow.abs() * 2.0 ** -24 + F64 * float(d_flow.abs().max())).all())


def test_saturating_conversion():
    got = R.sat_int32(np.array([0.0, -0.9, 1.9, -1.9, 1e9, -1e9, 3e10, -3e10, 2.0 ** 31, -2.0 ** 31, np.nan, np.inf, -np.inf]))
    assert got.tolist() == [0, 0, 1, -1, 10 ** 9, -10 ** 9, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, 2 ** 31 - 1, -2 ** 31]


# ---------------------------------------------------------------------------------------------------------------- Correlation
@pytest.mark.parametrize("i", range(len(R.CORR_CASES)), ids=[R.corr_id(c) for c in R.CORR_CASES])
def test_correlation_case_is_inside_its_budgets(i):
    """Every case of the GPU file builds on the CPU (its three budgets hold, the sums are float32 values) and is not degenerate."""
    c = R.corr_case(i)
    geom = c["geom"]
    R_, D = geom["max_displacement"] // geom["stride2"], 2 * (geom["max_displacement"] // geom["stride2"]) + 1
    assert D <= 31 and R.forward_lds_bytes(geom) <= 64 * 1024 and 1 <= R.window_pieces(geom) <= 15
    assert c["out"].dtype == c["d_f1"].dtype == c["d_f2"].dtype == torch.float32
    for k in ("out", "d_f1", "d_f2"):
        assert bool((c[k] > 0).any()) and bool((c[k] < 0).any()), k
    print(f"[{R.corr_id(R.CORR_CASES[i])}] NP {R.window_pieces(geom)}, D {D}, R {R_}, non-zero: out {float((c['out'] != 0).double().mean()):.0%}, "
          f"d_f1 {float((c['d_f1'] != 0).double().mean()):.0%}, d_f2 {float((c['d_f2'] != 0).double().mean()):.0%}")


def test_correlation_cases_reach_the_window_piece_counts_and_channel_counts():
    nps = sorted(R.window_pieces(g) for _, g in R.CORR_CASES)
    assert set(nps) == {1, 2, 3, 4, 5, 8, 14, 15}, nps
    by_np = {R.window_pieces(g): s[1] for s, g in R.CORR_CASES[len(R.GEOMS) + 1:]}
    assert by_np == {4: 40, 8: 33, 14: 1}
    assert R.CORR_CASES[:len(R.GEOMS)] == R.GEOMS and R.CORR_CASES[len(R.GEOMS)] == ((1, 256, 8, 16), R.FLOWNETC)


@pytest.mark.parametrize("i", SMALL_CORR, ids=[R.corr_id(R.CORR_CASES[i]) for i in SMALL_CORR])
def test_correlation_references_equal_autograd_on_exact_operands(i):
    """The float64 sums against autograd over `ref_correlation` times C (its mean divides; with integer operands mean * C is the exact sum
    only when the division is exact, so the SUMS are compared through a restatement with .sum in place of .mean: ref * C rounded)."""
    c = R.corr_case(i)
    C = c["shape"][1]
    sums = R.correlation_sums_ref(c["f1"], c["f2"], c["geom"])
    g1, g2 = R.correlation_grad_sums_ref(c["f1"], c["f2"], c["gout"], c["geom"])
    # autograd of the restatement with gout * C coming in returns the gradient of the channel SUM: every term an integer, exact in float64
    out, a1, a2 = _autograd_corr(c["f1"], c["f2"], c["gout"] * C, c["geom"])
    if C & (C - 1) == 0:      # a power of two: the mean's division is exact
        _same64(sums, out * C, "correlation sums")
        _same64(g1, a1, "correlation d_f1 sums")
        _same64(g2, a2, "correlation d_f2 sums")
    else:                     # (gout * C) / C inside the mean's backward rounds: the integers are recovered by rounding
        _same64(sums, (out * C).round(), "correlation sums")
        _same64(g1, a1.round(), "correlation d_f1 sums")
        _same64(g2, a2.round(), "correlation d_f2 sums")
        assert float((a1 - a1.round()).abs().max()) < 1e-9 and float((out * C - (out * C).round()).abs().max()) < 1e-9
    # the one float32 rounding, against the correctly rounded quotient: within one unit in the last place, equal for powers of two
    want = (sums / C).to(torch.float32)
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -23
    assert bool(((c["out"].double() - want.double()).abs() <= ulp.double()).all())
    if C & (C - 1) == 0:
        assert torch.equal(c["out"], want)


def test_correlation_references_agree_with_autograd_on_gaussian_operands():
    rs = np.random.RandomState(5)
    for shape, geom in (R.GEOMS[1], R.GEOMS[3], R.GEOMS[4]):
        f1, f2 = torch.from_numpy(rs.randn(*shape)), torch.from_numpy(rs.randn(*shape))
        C = shape[1]
        sums = R.correlation_sums_ref(f1, f2, geom, check=False)
        gout = torch.from_numpy(rs.randn(*sums.shape))
        g1, g2 = R.correlation_grad_sums_ref(f1, f2, gout, geom, check=False)
        out, a1, a2 = _autograd_corr(f1, f2, gout, geom)
        _near64(sums / C, out, f"correlation {shape}")
        _near64(g1 / C, a1, f"correlation d_f1 {shape}")
        _near64(g2 / C, a2, f"correlation d_f2 {shape}")


@pytest.mark.parametrize("shape", [(1, 256, 8, 16), (2, 64, 12, 14), (1, 32, 5, 37), (1, 1, 6, 9)])
def test_correlation_reference_equals_the_c_checker_on_exact_operands(shape):
    """oracle/native_ops.c sums 32 lanes and a tree and DIVIDES by C; on integer operands every order gives the same sum, and for C a
    power of two the division equals the multiplication by the reciprocal: bit equality.  (For any other C the two differ by the rounding
    of 1 / C; the kernels multiply, `correlation_ref` restates that.)"""
    from oracle import native
    rs = np.random.RandomState(sum(shape))
    f1, f2 = E.ints(rs, shape), E.ints(rs, shape)
    want = torch.from_numpy(native.correlation(f1.numpy(), f2.numpy(), 20, 1, 20, 1, 2))
    E.assert_exact(R.correlation_ref(f1, f2, R.FLOWNETC), want, f"correlation_ref against the C checker {shape}")
    # a channel count that is no power of two: the same sums, the quotient within one unit of the product
    shape = (1, 40, 5, 37)
    f1, f2 = E.ints(rs, shape), E.ints(rs, shape)
    want = torch.from_numpy(native.correlation(f1.numpy(), f2.numpy(), 20, 1, 20, 1, 2))
    got = R.correlation_ref(f1, f2, R.FLOWNETC)
    assert bool(((got.double() - want.double()).abs() <= want.abs().double() * 2.0 ** -23).all())
    E.assert_exact(R.correlation_sums_ref(f1, f2, R.FLOWNETC), (want.double() * 40).round(), "sums against the C checker, C = 40")


# ---------------------------------------------------------------------------------------------------------------- ChannelNorm
def test_channelnorm_gradient_reference():
    """Against float64 autograd within float32 rounding of its three operations (4 units of 2^-24 relative, the fourth for the 1e-9),
    float32 throughout, zero at a pixel whose channels are all zero; and exactly the quotient where nothing rounds."""
    rs = np.random.RandomState(9)
    x = rs.randn(2, 3, 17, 19).astype(np.float32)
    x[0, :, 8, 9] = 0.0
    gout = rs.randn(2, 1, 17, 19).astype(np.float32)
    out = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    got = R.channelnorm_grad_ref(x, out, gout)
    assert got.dtype == torch.float32 and not bool(got[0, :, 8, 9].any()) and bool(torch.isfinite(got).all())
    x64 = _leaf(x)
    R.ref_channelnorm(x64).backward(torch.from_numpy(gout).double())
    want = torch.nan_to_num(x64.grad, nan=0.0)
    assert bool(((got.double() - want).abs() <= want.abs() * (4 * 2.0 ** -24) + 1e-30).all())
    # out = 4 (1e-9 is below half a unit of it), reciprocal 0.25: gout * x / 4 exactly
    x = np.full((1, 2, 1, 3), 2.0 * np.sqrt(2.0), dtype=np.float32)
    got = R.channelnorm_grad_ref(x, np.full((1, 1, 1, 3), 4.0, np.float32), np.array([[[[1.0, -3.0, 0.5]]]], np.float32))
    assert torch.equal(got, torch.from_numpy(x) * torch.tensor([0.25, -0.75, 0.125]))


# ---------------------------------------------------------------------------------------------------------------- budgets
def test_scatter_budget_is_taken_per_destination_pixel():
    """16 samples of 2^21 each are far inside the budget one by one; a flow of -10 clamps all of them onto pixel (0, 0): 2^25."""
    img = np.zeros((1, 1, 4, 4))
    gout = np.full((1, 1, 4, 4), 2.0 ** 21)
    R.resample2d_grads_ref(img, np.zeros((1, 2, 4, 4), np.float32), gout)            # spread out: fine
    for bilinear in (True, False):
        with pytest.raises(E.BudgetError, match=r"d_img scatter.*at \(0, 0, 0, 0\)"):
            R.resample2d_grads_ref(img, np.full((1, 2, 4, 4), -10.0, np.float32), gout, bilinear)
    # the flow gradient's channel sum: one pixel of one image over its budget
    img = np.zeros((2, 3, 4, 5))
    img[1, :, 2, 3] = 2.0 ** 23
    flow = np.full((2, 2, 4, 5), 0.5, np.float32)
    with pytest.raises(E.BudgetError, match=r"d_flow channel sum.*at \(1, [01], "):
        R.resample2d_grads_ref(img, flow, np.ones((2, 3, 4, 5)))


def test_correlation_budgets_name_the_coordinate():
    shape, geom = (2, 4, 6, 7), dict(pad_size=2, kernel_size=1, max_displacement=2, stride1=1, stride2=1)
    f1, f2 = torch.ones(shape, dtype=torch.float64), torch.ones(shape, dtype=torch.float64)
    gout = torch.ones((2, 25, 6, 7), dtype=torch.float64)
    R.correlation_ref(f1, f2, geom)
    R.correlation_grads_ref(f1, f2, gout, geom)
    big1 = f1.clone()
    big1[1, :, 3, 4] = 2.0 ** 12
    big2 = f2 * 2.0 ** 11
    with pytest.raises(E.BudgetError, match=r"correlation forward.*at \(1, 0, 3, 4\)"):     # 4 channels x 2^12 x 2^11 = 2^25
        R.correlation_ref(big1, big2, geom)
    g = gout.clone()
    g[0, :, 2, 5] = 2.0 ** 20                                                                 # 25 displacements x 2^20 >= 2^24
    with pytest.raises(E.BudgetError, match=r"correlation d_f1.*at \(0, 0, 2, 5\)"):
        R.correlation_grads_ref(f1, f2, g, geom)
    g = gout.clone()
    for tj in range(-2, 3):                                                                   # one element per output pixel (d_f1 stays inside),
        for ti in range(-2, 3):                                                               # all 25 of them reaching f2 pixel (3, 3)
            g[1, (tj + 2) * 5 + ti + 2, 3 - tj, 3 - ti] = 2.0 ** 20
    with pytest.raises(E.BudgetError, match=r"correlation d_f2.*at \(1, 0, 3, 3\)"):
        R.correlation_grads_ref(f1, f2, g, geom)
    with pytest.raises(E.BudgetError, match="is not a float32 value"):                        # a sum that is no float32 value
        R.scale_inv_c(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64), 3, "sum")


# ---------------------------------------------------------------------------------------------------------------- planted defects
def test_a_dropped_tap_and_a_dropped_clamp_are_reported_with_their_coordinates():
    """In COPIES of the reference: (a) the (yB, xR) tap left out of the scatter, (b) the upper clamp of xR left out.  `assert_exact` names
    the count, the first coordinate and the bounding box; for (b) the box is the last column alone -- where the clamped samples land."""
    shape = (2, 3, 17, 29)
    c = R.resample_case(46, shape)
    good, _ = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"])
    tap, _ = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"], _plant="drop_tap")
    with pytest.raises(AssertionError) as e:
        E.assert_exact(tap.float(), good, "planted: tap dropped")
    msg = str(e.value)
    print(msg)
    m = E.diff_mask(tap.float(), good)
    first = tuple(int(v) for v in torch.nonzero(m)[0])
    assert f"{int(m.sum())} of {m.numel()} elements differ" in msg
    assert "first at (n=%d, c=%d, y=%d, x=%d)" % first in msg
    assert 100 < int(m.sum()) < m.numel()            # alpha * beta is non-zero for (7/8)^2 of the samples; gout is zero for a fifth
    clamp, _ = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"], _plant="drop_clamp")
    with pytest.raises(AssertionError) as e:
        E.assert_exact(clamp.float(), good, "planted: clamp dropped")
    msg = str(e.value)
    print(msg)
    assert "x 28..28]" in msg and "n 0..1" in msg
    # a single sample: flow 0.5 at one pixel of a zero flow -> the dropped tap is one element per channel
    flow = np.zeros((1, 2, 5, 6), np.float32)
    flow[0, :, 2, 3] = 0.5
    img, gout = np.ones((1, 2, 5, 6)), np.ones((1, 2, 5, 6))
    good, _ = R.resample2d_grads_ref(img, flow, gout)
    tap, _ = R.resample2d_grads_ref(img, flow, gout, _plant="drop_tap")
    with pytest.raises(AssertionError, match=r"2 of 60 elements differ.*first at \(n=0, c=0, y=3, x=4\): got 1.0, want 1.25; all inside "
                                             r"\[n 0..0, c 0..1, y 3..3, x 4..4\]"):
        E.assert_exact(tap.float(), good, "planted: one tap")


def test_a_difference_above_the_grid_cap_is_reported_by_trip():
    """`assert_exact_by_trip` on a 521 x 1009 map: a difference planted in a reference copy at the first pixel of the second trip (linear
    index 524,288 = row 519, column 617) and one below it; the same for a 16-byte build (4 pixels per thread) on a 1028 x 2044 map, whose second
    trip begins at pixel 2,097,152; a small map gets the plain message."""
    want = torch.zeros((1, 2, 521, 1009), dtype=torch.float32)
    got = want.clone()
    assert divmod(R.GRID_CAP, 1009) == (519, 617)
    got[0, 1, 519, 617] = 1.0
    with pytest.raises(AssertionError, match=r"1 of 1051378 elements differ.*first at \(n=0, c=1, y=519, x=617\).*first differing pixel at linear "
                                             r"index 524288: AT OR BEYOND the grid cap \(524288 pixels per trip\); differing pixels on the first "
                                             r"trip 0, on the second 1"):
        R.assert_exact_by_trip(got, want, "planted")
    got[0, 0, 519, 616] = 1.0
    with pytest.raises(AssertionError, match=r"index 524287: below the grid cap .*first trip 1, on the second 1"):
        R.assert_exact_by_trip(got, want, "planted")
    with pytest.raises(AssertionError) as e:
        R.assert_exact_by_trip(got[..., :4, :], want[..., :4, :] + 1.0, "small")
    assert "grid cap" not in str(e.value)
    R.assert_exact_by_trip(want, want.double(), "equal")
    want = torch.zeros((1, 1, 1028, 2044), dtype=torch.float32)
    got = want.clone()
    got.view(-1)[4 * R.GRID_CAP - 1] = 1.0
    with pytest.raises(AssertionError, match=r"index 2097151: below the grid cap \(2097152 pixels per trip\).*first trip 1, on the second 0"):
        R.assert_exact_by_trip(got, want, "planted", per_thread=4)
    got.view(-1)[4 * R.GRID_CAP - 1] = 0.0
    got.view(-1)[4 * R.GRID_CAP + 2] = 1.0
    with pytest.raises(AssertionError, match=r"index 2097154: AT OR BEYOND the grid cap .*first trip 0, on the second 1"):
        R.assert_exact_by_trip(got, want, "planted", per_thread=4)
