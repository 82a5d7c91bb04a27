"""tests/_exact.py on the CPU: its float64 references equal an int64 restatement written here, its budget checks fire with the
coordinate, and a planted one-unit defect in one element is found and localised to the footprint the geometry predicts."""
import numpy as np
import pytest
import torch

import _exact as E


# ------------------------------------------------------------------------------------------------ int64 restatements
def conv_i64(x, w, b, stride, pad):
    """x [N,C,H,W], w [Co,C,k,k], b [Co] int64 numpy -> [N,Co,Ho,Wo] int64: one einsum per tap."""
    N, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad), dtype=np.int64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.zeros((N, Co, Ho, Wo), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            out += np.einsum("nchw,oc->nohw", win, w[:, :, ky, kx])
    return out + (0 if b is None else b.reshape(1, -1, 1, 1))


def deconv_i64(x, w, b, stride, pad):
    """x [N,C,H,W], w [C,Co,k,k] int64 -> [N,Co,(H-1)s-2p+k,..] int64: every tap scatters the input grid onto its phase."""
    N, C, H, W = x.shape
    _, Co, kh, kw = w.shape
    full = np.zeros((N, Co, (H - 1) * stride + kh, (W - 1) * stride + kw), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            full[:, :, ky:ky + (H - 1) * stride + 1:stride, kx:kx + (W - 1) * stride + 1:stride] += np.einsum("nchw,co->nohw", x, w[:, :, ky, kx])
    out = full[:, :, pad:full.shape[2] - pad, pad:full.shape[3] - pad]
    return out + (0 if b is None else b.reshape(1, -1, 1, 1))


def _i(t):
    a = t.numpy()
    assert np.array_equal(a, np.round(a))
    return a.astype(np.int64)


@pytest.mark.parametrize("case", [(2, 5, 9, 11, 7, 1, 1, 0), (1, 33, 8, 7, 4, 3, 1, 1), (2, 6, 13, 10, 5, 3, 2, 1), (1, 3, 12, 15, 6, 7, 1, 3),
                                  (1, 4, 11, 9, 3, 7, 2, 3), (1, 8, 2, 2, 3, 7, 1, 3)])
def test_conv_reference_equals_int64_einsum(case):
    N, C, H, W, Co, k, s, p = case
    rs = np.random.RandomState(sum(case))
    x, w, b = E.ints(rs, (N, C, H, W)), E.sparse_weights(rs, (Co, C, k, k), 0.6, 3), E.ints(rs, (Co,), -9, 9)
    ref = E.conv_ref(x, w, b, stride=s, padding=p)
    assert np.array_equal(_i(ref), conv_i64(_i(x), _i(w), _i(b), s, p))


@pytest.mark.parametrize("geom", [(4, 2, 1), (8, 4, 2), (6, 2, 2), (7, 3, 2)])
def test_deconv_reference_equals_int64_einsum(geom):
    k, s, p = geom
    rs = np.random.RandomState(k * 10 + s)
    x, w, b = E.ints(rs, (2, 5, 6, 7)), E.sparse_weights(rs, (5, 4, k, k), 0.6, 3), E.ints(rs, (4,), -9, 9)
    ref = E.deconv_ref(x, w, b, stride=s, padding=p)
    assert ref.shape[2:] == (6 * s, 7 * s)
    assert np.array_equal(_i(ref), deconv_i64(_i(x), _i(w), _i(b), s, p))


def _stage_case(rs, S, N=1, h=5, w=6, slopes=(1.0, 0.0, 1.0), dens=(0.3, 0.3, 0.1)):
    k = S + 4
    return dict(a=E.ints(rs, (N, 32, h, w), -2, 2), up_w=E.sparse_weights(rs, (32, 32, k, k), dens[0], 1), up_b=E.ints(rs, (32,), -2, 2), up_a=slopes[0],
                dt_w=E.sparse_weights(rs, (32, 32), dens[1], 1), dt_b=E.ints(rs, (32,), -2, 2), dt_a=slopes[1],
                dn_w=E.sparse_weights(rs, (32, 32, k, k), dens[2], 1), dn_b=E.ints(rs, (32,), -2, 2), dn_a=slopes[2], S=S)


@pytest.mark.parametrize("S", [4, 2, 3])
def test_stage_reference_equals_int64_einsum(S):
    """Slopes 1 / 0 / 1 keep the restatement in integers: PReLU is then the identity or max(v, 0)."""
    c = _stage_case(np.random.RandomState(S), S)
    ref = E.stage_ref(**c, min_distinct=50)
    hr = deconv_i64(_i(c["a"]), _i(c["up_w"]), _i(c["up_b"]), S, 2)
    t = np.maximum(conv_i64(hr, _i(c["dt_w"]).reshape(32, 32, 1, 1), _i(c["dt_b"]), 1, 0), 0)
    out = conv_i64(t, _i(c["dn_w"]), _i(c["dn_b"]), S, 2)
    assert np.array_equal(_i(ref["hr"]), hr) and np.array_equal(_i(ref["t"]), t) and np.array_equal(_i(ref["out"]), out)


def test_stage_reference_with_dyadic_slopes_equals_scaled_int64():
    """Slopes 0.5 / 0.25 / 0.5: everything times 2, 8 and 16 is an integer; the restatement carries the scale."""
    S = 4
    c = _stage_case(np.random.RandomState(11), S, slopes=(0.5, 0.25, 0.5), dens=(0.2, 0.2, 0.03))
    ref = E.stage_ref(**c, min_distinct=50)
    hr2 = deconv_i64(_i(c["a"]), _i(c["up_w"]), _i(c["up_b"]), S, 2) * 2
    hr2 = np.where(hr2 > 0, hr2, hr2 // 2)                                                      # hr * 2
    t8 = conv_i64(hr2, _i(c["dt_w"]).reshape(32, 32, 1, 1), _i(c["dt_b"]) * 2, 1, 0) * 4
    t8 = np.where(t8 > 0, t8, t8 // 4)                                                          # t * 8
    o16 = conv_i64(t8, _i(c["dn_w"]), _i(c["dn_b"]) * 8, S, 2) * 2
    o16 = np.where(o16 > 0, o16, o16 // 2)                                                      # out * 16
    assert np.array_equal(_i(ref["hr"] * 2), hr2) and np.array_equal(_i(ref["t"] * 8), t8) and np.array_equal(_i(ref["out"] * 16), o16)


# ------------------------------------------------------------------------------------------------ the budget checks fire
def test_sum_budget_overflow_is_refused_with_coordinate():
    x = torch.full((1, 4, 3, 3), 1024.0, dtype=torch.float64)
    w = torch.zeros((2, 4, 1, 1), dtype=torch.float64)
    w[1] = 4096.0          # 4 x 1024 x 4096 = 2^24 at out-channel 1 only
    with pytest.raises(E.BudgetError, match=r"\(0, 1, 0, 0\)"):
        E.conv_ref(x, w)
    w[1] = 2048.0
    E.conv_ref(x, w)       # 2^23: inside
    xq = x / 4             # granularity 1/4 shrinks the budget with it: 4 x 256 x 2048 = 2^21 fits, 4 x 256 x 2^14 = 2^24 does not
    E.conv_ref(xq, w)
    with pytest.raises(E.BudgetError):
        E.conv_ref(xq + 0.25, w * 16)


def test_value_that_is_not_fp16_is_refused_with_coordinate():
    x = torch.zeros((1, 1, 2, 3), dtype=torch.float64)
    x[0, 0, 1, 2] = 2049.0           # odd above 2048: not an fp16 value
    w = torch.ones((1, 1, 1, 1), dtype=torch.float64)
    E.conv_ref(x, w, store=torch.float32)
    with pytest.raises(E.BudgetError, match=r"2049.*\(0, 0, 1, 2\)"):
        E.conv_ref(x, w, store=torch.float16)
    with pytest.raises(E.BudgetError, match="slope"):
        c = _stage_case(np.random.RandomState(0), 2)
        c["up_a"] = 0.1
        E.stage_ref(**c)
    # an intermediate of the stage: a power-of-two slope only moves the exponent, but 0.75 (an fp16 value itself) x -2047 needs 13 bits
    c = _stage_case(np.random.RandomState(0), 2, slopes=(0.75, 1.0, 1.0))
    c["up_w"][:, 5] = 0.0
    c["up_b"][5] = -2047.0
    with pytest.raises(E.BudgetError, match="after PReLU"):
        E.stage_ref(**c, live=False)


def test_degenerate_case_is_refused():
    c = _stage_case(np.random.RandomState(0), 2)
    c["dt_b"] = c["dt_b"] + 500.0        # every downtran sum positive: the PReLU behind it is never exercised
    c["dn_w"] = c["dn_w"] * 0.0          # (and nothing downstream leaves the fp16 range first)
    with pytest.raises(E.BudgetError, match="one sign"):
        E.stage_ref(**c)
    with pytest.raises(E.BudgetError, match="non-zero"):
        E.check_live(torch.zeros(1000, dtype=torch.float64), "zeros")
    with pytest.raises(E.BudgetError, match="distinct"):
        E.check_live(torch.tensor([1.0, -1.0] * 500, dtype=torch.float64), "two values")


def test_leaky_tenth_restates_one_float32_multiply_and_one_fp16_rounding():
    v = torch.arange(-3000, 3000, dtype=torch.float64)
    got = E.leaky_tenth_f16(v)
    tenth = np.float32(0.1)
    want = np.where(v.numpy() >= 0, v.numpy(), (v.numpy().astype(np.float32) * tenth).astype(np.float16).astype(np.float64))
    want = want.astype(np.float16).astype(np.float64)
    assert np.array_equal(got.numpy(), want)
    assert float(E.leaky_tenth_f16(torch.tensor([-5.0], dtype=torch.float64))) == float(np.float16(np.float32(-5.0) * tenth))


# ------------------------------------------------------------------------------------------------ assert_exact and planted defects
def test_assert_exact_message_and_sign_of_zero():
    want = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5) - 60.0
    got = want.to(torch.float16)
    E.assert_exact(got, want, "same")
    got0 = got.clone()
    got0[got0 == 0] = -0.0
    E.assert_exact(got0, want, "the sign of a zero is not compared")
    got[1, 2, 1:3, 4] += 1
    with pytest.raises(AssertionError) as e:
        E.assert_exact(got, want, "planted")
    msg = str(e.value)
    assert "2 of 120" in msg and "n=1, c=2, y=1, x=4" in msg and "n 1..1, c 2..2, y 1..2, x 4..4" in msg and "got" in msg and "want" in msg
    nan = want.to(torch.float32)
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 of 120"):
        E.assert_exact(nan, want, "nan")
    with pytest.raises(E.BudgetError):           # a reference that does not fit the output dtype is a construction error, not a mismatch
        E.assert_exact(got, want + 0.001, "inexact reference")


def _expect_footprint(got, want, predicted):
    with pytest.raises(AssertionError):
        E.assert_exact(got, want, "planted defect")
    m = E.diff_mask(got, want)
    assert torch.equal(m, predicted), (E.bbox(m), E.bbox(predicted))


def test_planted_last_chunk_channel_defect_at_k_9234():
    """cin 1026 (the last 32-channel chunk holds channels 1024, 1025), k 3: K = 9234.  One weight of channel 1025 off by one unit moves
    every pixel of ONE out-channel whose tap sees a non-zero input, and nothing else.

    Under the Gaussian operands of tests/test_gpu_conv.py (x ~ N(0,1), w ~ N(0,1)/sqrt(K)) the same defect -- one of K equal terms
    missing -- moves an output by about sigma / sqrt(K) = 1.04 % of its standard deviation; the range of 48 Gaussian outputs is about
    +-2.3 sigma, so that is about 0.45 % of the range at one element, 2e-3 of it on average over |x|: it sits ON the 2e-3 bar and
    passes or fails by seed.  Here it is 1 unit in every affected output, reported with coordinates."""
    rs = np.random.RandomState(9234)
    x = E.ints(rs, (1, 1026, 4, 6), -3, 3)
    x[x == 0] = 1.0                                   # every input non-zero: the footprint is the whole plane
    w = E.sparse_weights(rs, (2, 1026, 3, 3), 0.05, 2)
    b = E.ints(rs, (2,), -4, 4)
    want = E.conv_ref(x, w, b, padding=1, store=torch.float16)
    w2 = w.clone()
    w2[1, 1025, 1, 1] += 1.0                          # the centre tap sees every pixel
    got = E.conv_ref(x, w2, b, padding=1, store=torch.float16)
    pred = torch.zeros_like(want, dtype=torch.bool)
    pred[:, 1] = True
    _expect_footprint(got.to(torch.float16), want, pred)
    # a corner tap misses one border row and one border column
    w3 = w.clone()
    w3[0, 1024, 0, 0] -= 1.0
    pred = torch.zeros_like(want, dtype=torch.bool)
    pred[:, 0, 1:, 1:] = True
    _expect_footprint(E.conv_ref(x, w3, b, padding=1).to(torch.float16), want, pred)
    # the same defect under Gaussian operands, as a fraction of the range (what the 2e-3 bar sees)
    g = np.random.RandomState(1)
    xg, wg = torch.from_numpy(g.randn(1, 1026, 4, 6)), torch.from_numpy(g.randn(2, 1026, 3, 3) / np.sqrt(9234))
    ref = torch.nn.functional.conv2d(xg, wg, padding=1)
    wg2 = wg.clone()
    wg2[1, 1025, 1, 1] = 0.0
    frac = float((torch.nn.functional.conv2d(xg, wg2, padding=1) - ref).abs().max() / ref.abs().max())
    assert frac < 0.02, frac                          # a percent of the range at most: the scale of the old bar, not above it


@pytest.mark.parametrize("geom", [(4, 2, 1), (8, 4, 2), (7, 3, 2)])
def test_planted_transposed_convolution_tap_defect_hits_one_phase(geom):
    """Tap (ky, kx) of a transposed convolution feeds exactly the outputs (y s + ky - p, x s + kx - p): one phase of the s x s grid,
    clipped at the border, for one out-channel."""
    k, s, p = geom
    rs = np.random.RandomState(k)
    x = E.ints(rs, (2, 6, 5, 7), 1, 3)
    w = E.sparse_weights(rs, (6, 3, k, k), 0.5, 2)
    want = E.deconv_ref(x, w, None, stride=s, padding=p)
    for ky, kx in ((0, 0), (k - 1, 1), (p, p)):
        w2 = w.clone()
        w2[4, 2, ky, kx] += 1.0
        pred = torch.zeros_like(want, dtype=torch.bool)
        for y in range(5):
            for xx in range(7):
                oy, ox = y * s + ky - p, xx * s + kx - p
                if 0 <= oy < want.shape[2] and 0 <= ox < want.shape[3]:
                    pred[:, 2, oy, ox] = True
        assert pred.any()
        _expect_footprint(E.deconv_ref(x, w2, None, stride=s, padding=p).to(torch.float32), want, pred)


def test_planted_bias_slope_and_pixel_defects():
    rs = np.random.RandomState(3)
    x = E.ints(rs, (1, 8, 9, 10), 1, 3)
    w = E.sparse_weights(rs, (5, 8, 3, 3), 1.0, 2)
    w[w == 0] = 1.0
    b = E.ints(rs, (5,), -3, 3)
    pre = E.conv_ref(x, w, b, padding=1)
    want = E.prelu_ref(pre, 0.5)
    # one bias: every pixel of that channel
    b2 = b.clone()
    b2[3] += 1.0
    pred = torch.zeros_like(want, dtype=torch.bool)
    pred[:, 3] = True
    _expect_footprint(E.prelu_ref(E.conv_ref(x, w, b2, padding=1), 0.5).to(torch.float16), want, pred)
    # the slope: exactly the negative outputs
    _expect_footprint(E.prelu_ref(pre, 0.25).to(torch.float16), want, pre < 0)
    # one input pixel: the 3 x 3 neighbourhood in every out-channel (all weights are non-zero)
    x2 = x.clone()
    x2[0, 2, 4, 0] += 1.0
    pred = torch.zeros_like(want, dtype=torch.bool)
    pred[:, :, 3:6, 0:2] = True
    got = E.conv_ref(x2, w, b, padding=1)
    _expect_footprint(got.to(torch.float32), pre, pred)
