"""tests/_exact.py on the CPU: its float64 references equal an int64 restatement written here, its budget checks fire with the
coordinate, and a planted one-unit defect in one element is found and localised to the footprint the geometry predicts."""
import numpy as np
import pytest
import torch

import _exact as E
import _glue_cases as G


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


# ------------------------------------------------------------------------------------------------ the SR net's two ends
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 5), (7, 4)])
def test_bilinear_up_ref_is_atens_upsample(S, shape):
    x = E.ints(np.random.RandomState(S * 10 + shape[1]), (2, 3) + shape, -255, 255, step=0.125)
    want = torch.nn.functional.interpolate(x, scale_factor=S, mode="bilinear", align_corners=False)
    assert torch.equal(E.bilinear_up_ref(x, S), want)


def test_bilinear_up_ref_budget_checks_fire():
    x = E.ints(np.random.RandomState(0), (1, 3, 4, 4), -5, 5)
    with pytest.raises(E.BudgetError, match="not dyadic"):
        E.bilinear_up_ref(x, 3)
    big = x.clone()
    big[0, 1, 2, 3] = 2.0 ** 19 + 1.0          # (2^19 + 1) / 64 needs 26 bits
    with pytest.raises(E.BudgetError, match="lerp may round"):
        E.bilinear_up_ref(big, 4)


def _tail_case(S, seed=0, N=2, h=5, w=6):
    rs = np.random.RandomState(seed)
    k = S + 4
    return dict(hid=E.ints(rs, (N, 32, h, w), -2, 2), out_w=E.sparse_weights(rs, (32, 32, k, k), 1.0, 1), out_b=E.ints(rs, (32,), -3, 3), out_a=0.25,
                cv_w=E.sparse_weights(rs, (3, 32, 3, 3), 1.0, 8, step=0.25), cv_b=E.ints(rs, (3,), -200, 200, step=0.5), S=S)


@pytest.mark.parametrize("S", [2, 3, 4])
def test_tail_ref_is_the_stock_composition(S):
    c = _tail_case(S)
    ref = E.tail_ref(**c)
    out = torch.nn.ConvTranspose2d(32, 32, S + 4, S, 2).double()
    cv = torch.nn.Conv2d(32, 3, 3, padding=1).double()
    act = torch.nn.PReLU(init=c["out_a"]).double()
    with torch.no_grad():
        out.weight.copy_(c["out_w"]), out.bias.copy_(c["out_b"]), cv.weight.copy_(c["cv_w"]), cv.bias.copy_(c["cv_b"])
        hr = act(out(c["hid"]))
        want = cv(hr)
    assert torch.equal(ref["hr"], hr) and torch.equal(ref["raw"], want) and torch.equal(ref["dec"], want[..., ::S, ::S])
    assert ref["raw"].shape[-2:] == (S * 5, S * 6)
    # int64 restatement of the deconvolution sum (in quarters after the PReLU)
    hr0 = deconv_i64(_i(c["hid"]), _i(c["out_w"]), _i(c["out_b"]), S, 2)
    assert np.array_equal(np.where(hr0 > 0, 4 * hr0, hr0), _i(ref["hr"] * 4))


def test_tail_ref_budget_checks_fire():
    c = _tail_case(4)
    bad = dict(c, hid=c["hid"] * 64.0)                      # deconvolution sums of a few thousand: quarters of them are not fp16 values
    with pytest.raises(E.BudgetError, match="tail deconvolution"):
        E.tail_ref(**bad)
    bad = dict(c, cv_w=c["cv_w"] + 2.0 ** -12)
    with pytest.raises(E.BudgetError, match="conv_out weight"):
        E.tail_ref(**bad)
    bad = dict(c, cv_b=c["cv_b"] + 2.0 ** -30)              # float32 sum budget
    with pytest.raises(E.BudgetError, match="conv_out"):
        E.tail_ref(**bad)
    with pytest.raises(E.BudgetError, match="PReLU slope"):
        E.tail_ref(**dict(c, out_a=0.1))
    with pytest.raises(E.BudgetError, match="non-zero|one sign|distinct"):
        E.tail_ref(**dict(c, hid=c["hid"] * 0.0, out_b=c["out_b"] * 0.0))


def test_fold_ref_is_the_stock_composition_and_checks_its_budget():
    rs = np.random.RandomState(1)
    N, h, w = 2, 4, 7
    a, b = E.ints(rs, (N, 32, h, w), -2, 2), E.ints(rs, (N, 32, h, w), -2, 2)
    co_w, co_b, cmap = E.sparse_weights(rs, (32, 64), 0.1, 1), E.ints(rs, (32,), -1, 1), E.ints(rs, (32, h, w), -2, 2)
    got = E.fold_ref(a, b, cmap, co_w, co_b, 0.5)
    want = torch.nn.functional.prelu(torch.nn.functional.conv2d(torch.cat((a, b), 1), co_w.view(32, 64, 1, 1), co_b) + cmap, torch.tensor([0.5], dtype=torch.float64))
    assert torch.equal(got, want)
    with pytest.raises(E.BudgetError, match="compress_out"):
        E.fold_ref(a * 1024.0, b, cmap, co_w, co_b, 0.5)
    with pytest.raises(E.BudgetError, match="constant map"):
        E.fold_ref(a, b, cmap + 2.0 ** -40, co_w, co_b, 0.5)


def test_chain_ref_is_the_stock_composition_and_checks_its_budget():
    rs = np.random.RandomState(2)
    N, P = 2, 50
    x = [E.ints(rs, (N, 32, P), -2, 2) for _ in range(3)]
    w = [E.sparse_weights(rs, (32, 32), 0.15, 1) for _ in range(5)]
    b = [E.ints(rs, (32,), -2, 2) for _ in range(3)]
    cmap = E.ints(rs, (32, P), -4, 4, step=0.5)
    stages = [dict(ins=[(x[0], w[0]), (x[1], w[1])], prev=None, bias=b[0], cmap=cmap, slope=0.5),
              dict(ins=[(x[2], w[2])], prev=w[3], bias=b[1], cmap=None, slope=0.25),
              dict(ins=[], prev=w[4], bias=b[2], cmap=None, slope=2.0)]
    outs = E.chain_ref(stages)
    F = torch.nn.functional
    pr = lambda v, a: torch.where(v > 0, v, a * v)
    c1 = lambda xs, ws, bias: F.conv1d(torch.cat(xs, 1), torch.cat(ws, 1).unsqueeze(-1), bias)
    s0 = pr(c1([x[0], x[1]], [w[0], w[1]], b[0]) + cmap, 0.5)
    s1 = pr(c1([x[2], s0], [w[2], w[3]], b[1]), 0.25)
    s2 = pr(c1([s1], [w[4]], b[2]), 2.0)
    assert torch.equal(outs[0], s0) and torch.equal(outs[1], s1) and torch.equal(outs[2], s2)
    with pytest.raises(E.BudgetError, match="chain stage 1"):
        E.chain_ref([stages[0], dict(stages[1], bias=b[1] + 2.0 ** -20), stages[2]])
    with pytest.raises(E.BudgetError, match="stage 0 weight"):
        E.chain_ref([dict(stages[0], ins=[(x[0], w[0] * (1 + 2.0 ** -12))])])
    with pytest.raises(ValueError, match="no input"):
        E.chain_ref([dict(stages[2])])


def _head_case(f32, seed=3, shape=(2, 6, 9)):
    rs = np.random.RandomState(seed)
    N, h, w = shape
    x = E.ints(rs, (N, 3, h, w), 0, 255 if f32 else 63)
    if f32:
        sub = (torch.ones(3, dtype=torch.float64), -255.0 * torch.tensor((0.5, 0.25, 0.375), dtype=torch.float64))
        return dict(x=x, sub=sub, w_in=E.sparse_weights(rs, (128, 3, 3, 3), 1.0, 3), b_in=E.ints(rs, (128,), -50, 50), a_in=0.5,
                    w_feat=E.sparse_weights(rs, (32, 128), 1.0, 2), b_feat=E.ints(rs, (32,), -50, 50), a_feat=0.25, store=torch.float32)
    sub = (torch.tensor((1.0, 0.5, 2.0), dtype=torch.float64), torch.tensor((-31.5, -16.0, -63.0), dtype=torch.float64))   # (fp16: 6-bit pixels, halves)
    return dict(x=x, sub=sub, w_in=E.sparse_weights(rs, (128, 3, 3, 3), 2.5 / 27, 1), b_in=E.ints(rs, (128,), -4, 4), a_in=0.5,
                w_feat=E.sparse_weights(rs, (32, 128), 2.0 / 128, 1), b_feat=E.ints(rs, (32,), -4, 4), a_feat=0.25, store=torch.float16)


@pytest.mark.parametrize("f32", [False, True])
def test_head_ref_is_the_stock_composition(f32):
    c = _head_case(f32)
    got = E.head_ref(**c)
    F = torch.nn.functional
    t = F.conv2d(c["x"], torch.diag(c["sub"][0]).view(3, 3, 1, 1), c["sub"][1])          # MeanShift
    mid = F.prelu(F.conv2d(t, c["w_in"], c["b_in"], padding=1), torch.tensor([c["a_in"]], dtype=torch.float64))
    want = F.prelu(F.conv2d(mid, c["w_feat"].view(32, 128, 1, 1), c["b_feat"]), torch.tensor([c["a_feat"]], dtype=torch.float64))
    assert torch.equal(got, want)


def test_head_ref_budget_checks_fire():
    c = _head_case(False)
    with pytest.raises(E.BudgetError, match="mean-shifted pixels"):       # 255 + 95.625: eighths above 256
        E.head_ref(**dict(c, sub=(torch.ones(3, dtype=torch.float64), torch.tensor((127.5, 63.75, 95.625), dtype=torch.float64)),
                          x=torch.full_like(c["x"], 255.0)))
    with pytest.raises(E.BudgetError, match="conv_in"):
        E.head_ref(**dict(c, w_in=torch.ones_like(c["w_in"]), x=torch.full_like(c["x"], 255.0)))
    with pytest.raises(E.BudgetError, match="feat_in"):
        E.head_ref(**dict(c, w_feat=torch.ones_like(c["w_feat"]) * 3.0))


def _fc(rs, n):
    w1 = E.sparse_weights(rs, (32, n), 0.7, 2)
    w2 = torch.from_numpy(rs.randint(1, 5, size=32) * 0.5 * np.where(np.arange(32) % 2 == 0, 1.0, -1.0))      # halves of alternating sign
    return w1, E.ints(rs, (32,), -60, 60) - 128.0 * w1.sum(1), w2, E.ints(rs, (1,), -40, 40)


def _fusion_case(S, dec, n=8, seed=4, shape=(3, 5)):
    rs = np.random.RandomState(seed)
    h, w = shape
    ho, wo = (h, w) if dec else (S * h, S * w)
    one = torch.ones(3, dtype=torch.float64)
    mean = 255.0 * torch.tensor((0.5, 0.25, 0.375), dtype=torch.float64)
    return dict(raw=E.ints(rs, (n, 3, ho, wo), -64, 64, step=0.125), x=E.ints(rs, (n, 3, h, w), 0, 255), sub=(one, -mean), add=(one, mean),
                fc=_fc(rs, n),
                S=S, decimate=dec)


@pytest.mark.parametrize("dec", [False, True])
@pytest.mark.parametrize("S", [2, 4])
def test_fusion_ref_is_the_stock_composition(S, dec):
    c = _fusion_case(S, dec)
    got = E.fusion_ref(**c)
    F = torch.nn.functional
    eye = torch.eye(3, dtype=torch.float64).view(3, 3, 1, 1)
    skip = F.interpolate(F.conv2d(c["x"], eye, c["sub"][1]), scale_factor=S, mode="bilinear", align_corners=False)
    if dec:
        skip = skip[..., ::S, ::S]
    planes = F.conv2d(skip + c["raw"], eye, c["add"][1])
    w1, b1, w2, b2 = c["fc"]
    v = planes.permute(1, 2, 3, 0)                                               # the MLP runs over the plane axis
    want = F.relu(F.linear(F.relu(F.linear(v, w1, b1)), w2.view(1, -1), b2)).permute(3, 0, 1, 2)
    assert got.shape == (1, 3) + planes.shape[2:] and torch.equal(got, want)
    assert torch.equal(E.planes_ref(c["raw"], c["x"], c["sub"], c["add"], S, dec), planes)


def test_fusion_ref_budget_checks_fire():
    c = _fusion_case(4, False)
    w1, b1, w2, b2 = c["fc"]
    with pytest.raises(E.BudgetError, match="layer 1"):
        E.fusion_ref(**dict(c, fc=(w1 * 2.0 ** 12 + 1.0, b1, w2, b2)))
    with pytest.raises(E.BudgetError, match="layer 2"):
        E.fusion_ref(**dict(c, fc=(w1, b1, w2 * 2.0 ** 14 + 0.5, b2)))
    with pytest.raises(E.BudgetError, match="skip \\+ raw|lerp|bilinear"):
        E.fusion_ref(**dict(c, raw=c["raw"] + 2.0 ** -20 + 2.0 ** 10))
    with pytest.raises(E.BudgetError, match="non-zero|one sign|distinct"):
        E.fusion_ref(**dict(c, fc=(w1 * 0.0, b1 * 0.0 - 1.0, w2, b2)))          # a dead hidden layer


# ------------------------------------------------------------------------------------------------ the train step's gradient references
def _f32_autograd(fn, operands, gy):
    leaves = [t.to(torch.float32).requires_grad_() for t in operands]
    y = fn(*leaves)
    return y.detach(), [g.detach() for g in torch.autograd.grad(y, leaves, gy.to(torch.float32))]


@pytest.mark.parametrize("case", [("conv", 2, 5, 6, 70, 7, 3, 1, 1), ("conv", 2, 6, 21, 30, 4, 8, 4, 2), ("conv", 1, 9, 5, 7, 3, 1, 1, 0),
                                  ("deconv", 2, 4, 3, 9, 5, 8, 4, 2), ("deconv", 1, 5, 6, 7, 3, 7, 3, 2), ("deconv", 2, 3, 5, 8, 4, 6, 2, 2)])
def test_grads_ref_equals_float32_stock_autograd(case):
    """Inside the budget the float32 CPU operator and its autograd equal the float64 evaluation bit for bit: forward, dX, dW, db."""
    F = torch.nn.functional
    kind, N, cin, H, W, cout, K, s, p = case
    rs = np.random.RandomState(cin * 100 + K)
    x, b = E.ints(rs, (N, cin, H, W), -3, 3), E.ints(rs, (cout,), -4, 4)
    if kind == "conv":
        w = E.ints(rs, (cout, cin, K, K), -2, 2)
        fn = lambda x, w, b: F.conv2d(x, w, b, stride=s, padding=p)             # noqa: E731
    else:
        w = E.ints(rs, (cin, cout, K, K), -2, 2)
        fn = lambda x, w, b: F.conv_transpose2d(x, w, b, stride=s, padding=p)   # noqa: E731
    gy = E.ints(rs, tuple(fn(x, w, b).shape), -3, 3)
    y, grads = E.grads_ref(fn, (x, w, b), gy, kind)
    y32, g32 = _f32_autograd(fn, (x, w, b), gy)
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), y)
    for a, r in zip(g32, grads):
        assert a.shape == r.shape and torch.equal(a.double(), r)
    assert torch.equal(y, (E.conv_ref if kind == "conv" else E.deconv_ref)(x, w, b, stride=s, padding=p))
    y2, g2 = E.grads_ref(lambda x, w: fn(x, w, None), (x, w), gy, kind)          # without a bias: two operands
    assert len(g2) == 2 and torch.equal(g2[0], grads[0]) and torch.equal(g2[1], grads[1])


def test_grads_ref_budget_checks_fire_with_coordinate():
    F = torch.nn.functional
    fn = lambda x, w: F.conv2d(x, w)                                            # noqa: E731
    x = torch.full((1, 4, 3, 3), 1024.0, dtype=torch.float64)
    w = torch.zeros((2, 4, 1, 1), dtype=torch.float64)
    gy = torch.ones((1, 2, 3, 3), dtype=torch.float64)
    w[1] = 4096.0                                     # forward: 4 x 1024 x 4096 = 2^24 at out-channel 1
    with pytest.raises(E.BudgetError, match=r"forward.*\(0, 1, 0, 0\)"):
        E.grads_ref(fn, (x, w), gy)
    w[1] = 1024.0
    E.grads_ref(fn, (x, w), gy)                       # forward 2^22, dX 2^10, dW 9 x 1024: inside
    gy[0, 1, 2, 2] = 2.0 ** 14                        # dX = gy w: 2^24 at that pixel only; forward untouched
    with pytest.raises(E.BudgetError, match=r"gradient of operand 0.*\(0, 0, 2, 2\)"):
        E.grads_ref(fn, (x, w), gy)
    gy[0, 1, 2, 2] = 2.0 ** 13
    gy[0, 0] = 2.0 ** 11                              # dW[0] = sum of 9 pixels x 1024 x 2^11 > 2^24; dX = 2^11 x 0 + ... inside
    with pytest.raises(E.BudgetError, match=r"gradient of operand 1.*\(0, 0, 0, 0\)"):
        E.grads_ref(fn, (x, w), gy)
    with pytest.raises(E.BudgetError):                # a granularity of 1/4 in one operand shrinks every budget with it
        E.grads_ref(fn, (x + 0.25, w * 4), torch.ones_like(gy))


def test_prelu_grads_ref_equals_float32_stock_autograd_and_its_convention_at_zero():
    F = torch.nn.functional
    rs = np.random.RandomState(5)
    v, g = E.ints(rs, (3, 4, 9, 11), -3, 3), E.ints(rs, (3, 4, 9, 11), -3, 3)
    g[g == 0] = 1.0
    assert int((v == 0).sum()) > 50
    for slope in E.SLOPES_LE_ONE + E.SLOPES_SELECT:
        gv, da = E.prelu_grads_ref(v, g, slope)
        v32 = v.float().requires_grad_()
        a32 = torch.tensor([slope], dtype=torch.float32, requires_grad=True)
        y32 = F.prelu(v32, a32)
        y32.backward(g.float())
        assert torch.equal(y32.detach().double(), E.prelu_ref(v, slope))
        assert torch.equal(v32.grad.double(), gv) and torch.equal(a32.grad.double(), da)
        assert torch.equal(gv[v == 0], g[v == 0] * slope)                  # the slope side at v == 0
    gv, da = E.prelu_grads_ref(torch.tensor([0.0, 2.0, -2.0], dtype=torch.float64), torch.tensor([3.0, 3.0, 3.0], dtype=torch.float64), 0.25)
    assert gv.tolist() == [0.75, 3.0, 0.75] and da.tolist() == [-6.0]


def test_prelu_grads_ref_budget_checks_fire():
    v = torch.full((4096,), -64.0, dtype=torch.float64)
    g = torch.full((4096,), 64.0, dtype=torch.float64)
    with pytest.raises(E.BudgetError, match="slope gradient"):             # 4096 x 64 x 64 = 2^24
        E.prelu_grads_ref(v, g, 0.5)
    E.prelu_grads_ref(v[:2048], g[:2048], 0.5)
    with pytest.raises(E.BudgetError, match="input gradient"):             # (2^24 + 2) * 0.75 needs 25 bits
        E.prelu_grads_ref(torch.tensor([-1.0], dtype=torch.float64), torch.tensor([2.0 ** 24 + 2.0], dtype=torch.float64), 0.75)
    with pytest.raises(E.BudgetError, match="slope"):
        E.prelu_grads_ref(v[:8], g[:8], 0.1)


def _mlp_case(seed, n=8, hidden=32, shape=(3, 7)):
    rs = np.random.RandomState(seed)
    planes = E.ints(rs, (n, 3) + shape, -24, 24, step=0.125)
    w1 = E.sparse_weights(rs, (hidden, n), 0.7, 2)
    w2 = torch.from_numpy(rs.randint(1, 5, size=hidden) * 0.5 * np.where(np.arange(hidden) % 2 == 0, 1.0, -1.0))
    return planes, (w1, E.ints(rs, (hidden,), -2, 2), w2, E.ints(rs, (1,), 0, 2)), E.ints(rs, (1, 3) + shape, -3, 3)


@pytest.mark.parametrize("n,hidden", [(8, 32), (1, 5), (16, 32), (3, 7)])
def test_mlp_grads_ref_equals_float32_stock_autograd(n, hidden):
    F = torch.nn.functional
    planes, fc, go = _mlp_case(n, n, hidden)
    grads = E.mlp_grads_ref(planes, fc, go, live=False)
    h, w1, b1, w2, b2 = (t.float().requires_grad_() for t in (planes,) + fc)
    y = F.relu(F.linear(F.relu(F.linear(h.permute(1, 2, 3, 0), w1, b1)), w2.view(1, -1), b2)).permute(3, 0, 1, 2)
    assert torch.equal(y.detach().double(), E.mlp_ref(planes, fc, live=False))
    y.backward(go.float())
    for a, r in zip((h, w1, b1, w2, b2), grads):
        assert a.grad.shape == r.shape and torch.equal(a.grad.double(), r)
    assert all(bool(g.any()) for g in grads[:4])                                # (db2, one sum of signed integers, may well be 0)


def test_mlp_grads_ref_budget_checks_fire():
    planes, fc, go = _mlp_case(0)
    w1, b1, w2, b2 = fc
    E.mlp_grads_ref(planes, fc, go, live=False)
    with pytest.raises(E.BudgetError, match="layer 1"):
        E.mlp_grads_ref(planes, (w1 * 2.0 ** 20 + 1.0, b1, w2, b2), go, live=False)
    with pytest.raises(E.BudgetError, match="dW1|db1|dv|hidden gradient"):     # forward inside, the gradient 2^22 times larger
        E.mlp_grads_ref(planes, fc, go * 2.0 ** 22 + 1.0, live=False)
    big = torch.full_like(go, 2.0 ** 19) + 1.0                                  # 63 pixels x 2^19 > 2^24: the sum over pixels alone
    with pytest.raises(E.BudgetError, match="fusion MLP d"):
        E.mlp_grads_ref(planes, (w1, b1, w2, b2 + 500.0), big, live=False)


# ------------------------------------------------------------------------------------------------ the trunk glue (tests/_glue_cases.py)

def test_osvos_fold_equals_a_plain_loop_for_non_symmetric_weights():
    """weff_b[ky][kx][ci] = sum_co fuse[16 b + co] * up_b[ci][co][ky][kx], tap by tap in int64: an (in, out) swap in the einsum, a fuse
    row read at the wrong branch or a transposed tap would change it (the weights are dense and not symmetric)."""
    from video_super_resolution_amd.trunk_exec import osvos_fold
    c = G.gen_osvos(17, 33)
    got = osvos_fold([u.float() for u in c["up_w"]], c["fuse_w"].float().view(1, 64, 1, 1))
    fuse = _i(c["fuse_w"])
    for b, u in enumerate(c["up_w"]):
        u, k = _i(u), u.shape[-1]
        assert not np.array_equal(u, u.transpose(1, 0, 2, 3))
        want = np.zeros((k, k, 16), dtype=np.int64)
        for ci in range(16):
            for co in range(16):
                for ky in range(k):
                    for kx in range(k):
                        want[ky, kx, ci] += fuse[16 * b + co] * u[ci, co, ky, kx]
        assert got[b].dtype == torch.float16 and tuple(got[b].shape) == (k, k, 16) and got[b].is_contiguous()
        assert np.array_equal(got[b].double().numpy(), want.astype(np.float64)), b
        swapped = np.einsum("oikl,o->kli", u, fuse[16 * b:16 * b + 16])
        assert not np.array_equal(swapped, want)


@pytest.mark.parametrize("case", [c for c in G.OSVOS_CASES if c[2] == 16 or c[:2] not in G.OSVOS_GEOMS], ids=str)
def test_osvos_cases_are_inside_their_budget_and_equal_an_int64_scatter(case):
    """Every geometry of the GPU test: the reference runs (its budget checks pass) and equals a tap-by-tap int64 scatter of the transposed
    convolutions, cropped with slices worked out here."""
    h, w, _, nb = case
    c = G.gen_osvos(h, w, nb)
    ref = G.osvos_ref(c)
    assert E.osvos_sizes(h, w, nb) == [tuple(s.shape[2:]) for s in c["sides"]]
    cat = []
    for b, s in enumerate(c["strides"]):
        full = deconv_i64(_i(c["sides"][b]), _i(c["up_w"][b]), None, s, 0)
        dh, dw = full.shape[2] - h, full.shape[3] - w
        assert dh >= 0 and dw >= 0
        cat.append(full[:, :, dh // 2:dh // 2 + h, dw // 2:dw // 2 + w])
    want = np.einsum("nchw,c->nhw", np.concatenate(cat, 1), _i(c["fuse_w"])) + int(c["bias"])
    assert np.array_equal(_i(ref)[:, 0], want)


def test_osvos_crop_offsets_take_both_parities_where_they_can():
    """The seven geometries between them: the crop excess (hs + 1) s - h odd and even in every branch, in rows and in columns (odd: the
    spare pixel goes at the bottom / right); the offset excess // 2 odd and even in branches 1..3 -- in branch 0 (s = 2, hs = ceil(h / 2))
    the excess is 2 or 3 and the offset 1 at every size; a side map of one row (2 x 3) and, in the added 33 x 1 case, of one column."""
    off = {(b, ax): set() for b in range(4) for ax in (0, 1)}
    exc = {(b, ax): set() for b in range(4) for ax in (0, 1)}
    one = set()
    for h, w in G.OSVOS_GEOMS + [(33, 1)]:
        for b, (hs, ws) in enumerate(E.osvos_sizes(h, w)):
            s = G.OSVOS_STRIDES[b]
            if (h, w) == (33, 1):                                    # (the one-column side maps of more than one row)
                one |= {"col"} if ws == 1 and hs > 1 else set()
                continue
            for ax, e in enumerate(((hs + 1) * s - h, (ws + 1) * s - w)):
                exc[(b, ax)].add(e & 1)
                off[(b, ax)].add((e // 2) & 1 if b else e // 2)
            one |= {"row"} if hs == 1 and ws > 1 else set()
    assert all(v == {0, 1} for v in exc.values()), exc
    assert all(v == ({0, 1} if b else {1}) for (b, _), v in off.items()), off
    assert one == {"row", "col"}


def test_osvos_head_budget_checks_fire():
    c = G.gen_osvos(17, 33)
    fuse = c["fuse_w"].clone()
    fuse[0] = 4097.0                                                 # folded weights 4097 u + a few units: not multiples of 4
    big = dict(c, fuse_w=fuse)
    with pytest.raises(E.BudgetError, match="folded weight of branch"):
        G.osvos_ref(big)
    half = [s.clone() for s in c["sides"]]
    half[2][1, 4, 0, 0] = 0.3
    with pytest.raises(E.BudgetError, match="side map 2"):
        G.osvos_ref(dict(c, sides=half))
    wide = dict(c, sides=[s * 4096.0 for s in c["sides"]])          # fp16 values still, the sum is not below 2^24
    with pytest.raises(E.BudgetError, match="OSVOS head"):
        G.osvos_ref(wide)
    with pytest.raises(E.BudgetError, match="upsamples to less"):
        E.osvos_head_ref(c["sides"], c["up_w"], c["fuse_w"], c["bias"], (40, 33), live=False)


def test_osvos_planted_weight_defect_has_the_footprint_of_one_phase():
    """One unit in one folded weight of branch 3 (tap (13, 20), channel 5) moves at most the pixels of one output phase: (y + oy) % 16 ==
    13 rows, (x + ox) % 16 == 4 columns with the source column one to the left -- and only where the side value is not zero."""
    h, w = 23, 47
    c = G.gen_osvos(h, w)
    d = torch.zeros((16, 1, 32, 32), dtype=torch.float64)
    d[5, 0, 13, 20] = 1.0
    moved = G.osvos_ref(c, dweff=[None, None, None, d]) != G.osvos_ref(c)
    hs, ws = c["sides"][3].shape[2:]
    oy, ox = ((hs + 1) * 16 - h) // 2, ((ws + 1) * 16 - w) // 2
    ys, xs = torch.nonzero(moved)[:, 2], torch.nonzero(moved)[:, 3]
    assert 0 < int(moved.sum()) < moved.numel()
    assert bool((((ys + oy) % 16) == 13).all()) and bool((((xs + ox) % 16) == 4).all())


@pytest.mark.parametrize("case", G.PAIRS_CASES[:-1], ids=lambda c: f"{c[1]}x{c[2]}-B{len(c[4])}")
def test_pairs_reference_is_the_stock_composition(case):
    """`pairs_ref` against models.py:74-79 in float64 stock operators (mean over both frames and all pixels; the division by 255): the
    float32 restatement is within one float32 rounding of each of its two operations, and its layouts are the kernel's three outputs."""
    c = G.gen_pairs(case)
    r = G.pairs_ref(c)
    y0, x0, H, W = c["crop"]
    crop = torch.from_numpy(c["frames"]).double()[:, y0:y0 + H, x0:x0 + W]
    inputs = torch.stack([torch.stack([crop[a], crop[b]]).permute(3, 0, 1, 2) for a, b in c["pairs"]])       # [B,3,2,H,W]
    mean = inputs.contiguous().view(len(c["pairs"]), 3, -1).mean(-1).view(-1, 3, 1, 1, 1)
    want = (inputs - mean) / 255.0
    want = torch.cat((want[:, :, 0], want[:, :, 1]), 1).numpy()
    assert np.abs(r["x"] - want).max() <= 2.0 ** -23                                                     # |x| <= 1: 3 half-ulps
    assert np.array_equal(r["x6h"][..., :6], r["x"].astype(np.float16).transpose(0, 2, 3, 1)) and not r["x6h"][..., 6:].any()
    assert not r["both4"][..., 3].any()


def test_pairs_largest_case_is_inside_its_budget_and_beyond_the_grid_cap():
    case = G.PAIRS_CASES[-1]
    y0, x0, H, W = case[5]
    assert H * W > 2048 * 256 and H % 4 == 0 and W % 4 == 0 and 2 * H * W * case[3] < 2 ** 24
    assert (H, W) == min(((a, b) for a in range(4, 2048, 4) for b in (1020,) if a * b > 2048 * 256), key=lambda s: s[0] * s[1])
    G.pairs_ref(G.gen_pairs(case))


def test_pairs_budget_checks_fire():
    c = G.gen_pairs(G.PAIRS_CASES[-1])
    c["frames"] = c["frames"] * 3.0                                   # values up to 45: the sum passes 2^24
    with pytest.raises(E.BudgetError, match="not below 2\\^24"):
        G.pairs_ref(c)
    c = G.gen_pairs(G.PAIRS_CASES[0])
    c["frames"][0, 5, 5, 1] = 0.5
    with pytest.raises(E.BudgetError, match="integers"):
        G.pairs_ref(c)
    c = G.gen_pairs(G.PAIRS_CASES[0])
    c["crop"] = (10, 4, 12, 16)
    with pytest.raises(E.BudgetError, match="leaves the frame"):
        G.pairs_ref(c)


@pytest.mark.parametrize("bilinear", [1, 0])
@pytest.mark.parametrize("shape", G.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_cases_are_dyadic_and_clamp_on_every_side(shape, bilinear):
    """Every case of the GPU test: the float64 upsampling is a float32 value (checked inside), the twelve channels are finite fp16 values,
    and from 8 x 8 up the targets leave the image on all four sides."""
    B, H, W = shape
    c, out16 = G.warp_ref(shape, bilinear)
    assert out16.shape == (B, H, W, 16) and out16.dtype == np.float16 and np.isfinite(out16.astype(np.float32)).all()
    assert not out16[..., 12:].any() and not out16.flags.writeable
    flow = G.warp_flow_ref(c, bilinear)
    assert np.array_equal(out16[..., :6], c["x6"].numpy().transpose(0, 2, 3, 1).astype(np.float16))
    if H >= 8 and W >= 8:
        assert all(G.warp_leaves_every_side(flow, H, W))
    if bilinear and H >= 8:
        assert len(np.unique(flow)) > 16           # the lerp is live: values between the grid's own


def test_warp_budget_checks_fire():
    c = G.gen_warp((1, 8, 8))
    c["q"] = c["q"] + 2.0 ** -20                                      # no longer multiples of 1/8: float32 lerps would round
    with pytest.raises(E.BudgetError):
        G.warp_flow_ref(c, 1)
    c = G.gen_warp((1, 8, 8))
    c["q"] = c["q"] * 4.0                                            # beyond 2: x 20 leaves the stated range
    with pytest.raises(E.BudgetError, match="beyond 40"):
        G.warp_flow_ref(c, 0)


@pytest.mark.parametrize("sizes", [(26, 22), (14, 46), (21, 69)])
def test_nearest_resize_ref_differs_from_the_rational_index_where_the_cases_say(sizes):
    n_in, n_out = sizes
    assert E.nearest_differs_from_rational(n_in, n_out)
    assert not E.nearest_differs_from_rational(13, 5) and not E.nearest_differs_from_rational(9, 4) and not E.nearest_differs_from_rational(7, 7)
    x = torch.arange(n_in, dtype=torch.float16).view(1, 1, n_in, 1) + 0.5
    got = E.nearest_resize_ref(x, (n_out, 1))
    assert got.dtype == torch.float16 and torch.equal(got[0, 0, :, 0], E.nearest_sources(n_in, n_out).to(torch.float16) + 0.5)


# ------------------------------------------------------------------------------------------------ rounding: round_f16 and its companions
import _round_cases as R  # noqa: E402


def _edge_sweep():
    """Every tie and both of its float32 neighbours at the two ends of each binade from 2^-24 to 2^15 (ties behind an even and behind an
    odd significand), the 65519 / 65520 pair and its neighbours, subnormal ties of both parities, +-0; both signs."""
    v = [0.0, 65504.0, 65519.0, 65520.0, 65535.0, 65536.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -24]
    for e in range(-24, 16):
        q = 2.0 ** max(e - 10, -24)                                    # the fp16 spacing inside [2^e, 2^(e+1))
        lo, hi = 2.0 ** e, 2.0 ** (e + 1)
        v += [lo + q / 2, lo + 3 * q / 2, hi - q / 2, hi - 3 * q / 2, lo, hi - q]
    for k in (0, 1, 2, 3, 510, 511, 1022, 1023):                       # subnormal ties (k + 1/2) 2^-24
        v.append((k + 0.5) * 2.0 ** -24)
    a = np.array(v, dtype=np.float32)
    assert np.array_equal(a.astype(np.float64), np.array(v))           # (each is a float32 value)
    a = np.concatenate([a, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))])
    a = a[np.abs(a) < 3e38]
    return np.concatenate([a, -a])


def test_round_f16_equals_the_torch_and_numpy_casts_on_the_edge_sweep():
    a = _edge_sweep()
    got = E.round_f16(torch.from_numpy(a.astype(np.float64))).numpy()
    with np.errstate(over="ignore"):
        want_np = a.astype(np.float16).astype(np.float64)
    want_t = torch.from_numpy(a).to(torch.float16).to(torch.float64).numpy()
    want_t64 = torch.from_numpy(a.astype(np.float64)).to(torch.float16).to(torch.float64).numpy()
    for want in (want_np, want_t, want_t64):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (a[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the literal corners
    f = lambda x: float(E.round_f16(torch.tensor([x], dtype=torch.float64)))
    assert (f(2049.0), f(2051.0), f(4098.0), f(4102.0)) == (2048.0, 2052.0, 4096.0, 4104.0)
    assert f(65519.0) == 65504.0 and f(65520.0) == float("inf") and f(-65520.0) == float("-inf") and f(65519.99609375) == 65504.0
    assert f(2.0 ** -25) == 0.0 and f(3 * 2.0 ** -25) == 2.0 ** -23 and f(2.0 ** -25 * (1 + 2.0 ** -23)) == 2.0 ** -24      # gradual underflow
    with pytest.raises(E.BudgetError):
        E.round_f16(torch.tensor([0.1], dtype=torch.float64))          # not a float32 value
    with pytest.raises(E.BudgetError):
        E.round_f16(torch.tensor([float("nan")], dtype=torch.float64))


def test_round_f16_equals_an_int64_restatement_on_24_bit_integers():
    rs = np.random.RandomState(24)
    n = np.concatenate([rs.randint(0, 2 ** 24, size=20000), rs.randint(0, 2 ** 16, size=20000), np.arange(2040, 2060), np.arange(65500, 65540)]).astype(np.int64)
    bl = np.floor(np.log2(np.maximum(n, 1))).astype(np.int64) + 1      # bit length (exact: n < 2^24 is a float64 integer)
    s = np.maximum(bl - 11, 0)
    lo = (n >> s) << s
    rem, half = n - lo, (np.int64(1) << s) >> 1
    up = (rem > half) | ((rem == half) & (s > 0) & (((n >> s) & 1) == 1))
    want = (lo + np.where(up, np.int64(1) << s, 0)).astype(np.float64)
    want[want >= 65536] = np.inf
    for sign in (1.0, -1.0):
        got = E.round_f16(torch.from_numpy(n.astype(np.float64) * sign)).numpy()
        assert np.array_equal(got, want * sign)
    # the alternatives differ exactly where they should: truncation wherever a remainder exists and RNE went up, "away" at ties behind even
    x = torch.from_numpy(n[n < 65504].astype(np.float64))
    p = E.rounding_profile(x)
    rne, rtz, away = E.round_f16(x), E.round_f16_alt(x, "rtz"), E.round_f16_alt(x, "away")
    assert torch.equal(rtz != rne, p["inexact"] & (rne.abs() > x.abs())) and bool((rtz.abs() <= x.abs()).all())
    assert torch.equal(away != rne, p["tie_down"]) and int(p["tie_down"].sum()) > 100 and int(p["tie_up"].sum()) > 100
    assert torch.equal(p["tie"], p["tie_up"] | p["tie_down"]) and not bool((p["tie"] & ~p["inexact"]).any())


def test_act_round_and_packed_prelu_references_state_their_operations():
    v = torch.arange(-40000, 40000, 7, dtype=torch.float64)
    # trunk order: float32 multiply by float32(slope), one fp16 rounding (numpy's casts as the independent statement)
    for slope in (0.1, 0.75, 0.2):
        want = np.where(v.numpy() >= 0, v.numpy(), (v.numpy().astype(np.float32) * np.float32(slope)).astype(np.float64)).astype(np.float32).astype(np.float16)
        assert np.array_equal(E.act_round_ref(v, 2, slope).numpy(), want.astype(np.float64))
    assert torch.equal(E.act_round_ref(v, 1), E.round_f16(v.clamp(min=0))) and torch.equal(E.act_round_ref(v, 0), E.round_f16(v))
    assert torch.equal(E.leaky_tenth_f16(v), E.act_round_ref(v, 2, 0.1))
    # SR order: fp16 value times fp16 slope, rounded once, then max / min / select
    v16 = E.round_f16(v)
    for slope, build in ((0.2, "max"), (0.75, "max"), (0.75, "select"), (1.5, "min"), (1.5, "select"), (-0.75, "select"), (-0.75, "max")):
        a = np.float16(np.float32(slope))
        m = (v16.numpy().astype(np.float16).astype(np.float64) * float(a)).astype(np.float16).astype(np.float64)      # (22-bit product: exact in float64)
        want = np.where(v16.numpy() < 0, m, v16.numpy())
        assert np.array_equal(E.prelu_f16_ref(v16, slope, build).numpy(), want), (slope, build)
    assert float(E.prelu_f16_ref(torch.tensor([-3.0], dtype=torch.float64), 0.2)) == float(np.float16(-3.0) * np.float16(0.2))
    assert float(E.prelu_f16_ref(torch.tensor([-3.0], dtype=torch.float64), 0.2)) != float(np.float16(np.float32(-3.0) * np.float32(0.2)))
    with pytest.raises(E.BudgetError, match="PReLU input"):
        E.prelu_f16_ref(torch.tensor([2049.0], dtype=torch.float64), 0.5)


def test_check_rounds_fires_on_each_of_its_conditions():
    rs = np.random.RandomState(1)
    good = torch.from_numpy(rs.randint(-20000, 20000, size=4096).astype(np.float64))
    E.check_rounds(good, "good")
    with pytest.raises(E.BudgetError, match="need rounding"):
        E.check_rounds(torch.from_numpy(rs.randint(-2000, 2000, size=4096).astype(np.float64)), "all exact")
    with pytest.raises(E.BudgetError, match="ties"):
        E.check_rounds(good + 0.25, "no ties")
    with pytest.raises(E.BudgetError, match="overflows"):
        E.check_rounds(torch.cat([good, torch.tensor([65520.0], dtype=torch.float64)]), "overflow")
    with pytest.raises(E.BudgetError, match="too few"):
        E.check_rounds(good[:100], "small")
    pool = []
    E.check_rounds(good[:300], "a", pool=pool)
    with pytest.raises(E.BudgetError, match="fewer than 512"):
        E.check_rounds_pool(pool, "pool")
    E.check_rounds(good[300:600], "b", pool=pool)
    E.check_rounds_pool(pool, "pool")
    up_only = torch.arange(2049, 4096, 4, dtype=torch.float64)          # 2049 + 4 k: every tie sits behind an even significand
    with pytest.raises(E.BudgetError, match="ties go up"):
        E.check_rounds(up_only, "one direction")


def test_local_granularity_sees_the_fine_value_only_where_it_is_read():
    x = torch.zeros((1, 2, 5, 5), dtype=torch.float64) + 4096.0
    x[0, 1, 2, 2] = 2.0 ** -13
    w = torch.zeros((1, 2, 3, 3), dtype=torch.float64)
    w[0, 1, 1, 1] = w[0, 0, 0, 0] = 1.0
    g = E.local_granularity(x, w, padding=1)
    assert float(g[0, 0, 2, 2]) == 2.0 ** -13 and int((g != 1.0).sum()) == 1
    with pytest.raises(E.BudgetError, match=r"\(0, 0, 2, 2\)"):          # 4096 + 2^-13 needs 26 bits
        E.conv_ref(x, w, padding=1, local=True)
    w[0, 0, 0, 0] = 0.0
    E.conv_ref(x, w, padding=1, local=True)                              # one term per output: exact
    with pytest.raises(E.BudgetError):
        E.conv_ref(x, w, padding=1)                                      # the global budget refuses the map: 4096 against a granule of 2^-13


# ------------------------------------------------------------------------------------------------ rounding: every case, and what each defect moves
def _enough(n_moved, numel):
    """At least 5 % of a stored map, or at least 16 elements of a map below 512."""
    return n_moved >= (16 if numel < 512 else max(16, int(np.ceil(0.05 * numel))))


@pytest.mark.parametrize("name", R.names())
def test_trunk_rounding_case_is_live_and_tells_every_defect(name):
    """The case builds (its budget and `check_rounds` run inside) and its reference differs from truncation, ties away from zero, the
    activation behind the rounding (Leaky cases), the slope rounded to fp16 (Leaky 0.1) and a partial sum parked in fp16 in at least 5 % of the map: the device comparison,
    which has no tolerance, fails for each of those defects."""
    c = R.case(name)
    alts = R.alternatives(c)
    assert {"rtz", "away", "partial"} <= set(alts) and (("act_after" in alts) == (c["act"] == R.LEAKY))
    assert ("slope16" in alts) == (c["act"] == R.LEAKY and c["slope"] == 0.1)
    for kind, alt in alts.items():
        assert _enough(R.moved(c, alt), c["want"].numel()), (name, kind, R.moved(c, alt), c["want"].numel())


def test_trunk_composite_cases_are_live():
    """HFlowHead (the flow rounds, the upsampling of the ROUNDED flow rounds again), HHourglassFront, the average pool, the float32-weight
    cases: references, budgets and liveness; a kernel that read the UNROUNDED map or weight would move 5 % of the next one."""
    for i in range(len(R.FLOW_HEAD)):
        c = R.flow_head_case(i)
        other = E.round_f16(E.deconv_ref(c["pre"], c["wu"], c["bu"], stride=2, padding=1))
        assert _enough(int((other != c["up"]).sum()), c["up"].numel())
    for i in range(len(R.HG_FRONT)):
        c = R.hg_front_case(i)
        other = E.act_round_ref(E.conv_ref(torch.relu(c["stem"]["pre"]), c["w1"], c["b1"]), R.RELU)
        assert _enough(int((other != c["one"]).sum()), c["one"].numel())
    for shape in ((2, 9, 7, 16), (3, 5, 33, 40)):
        x16, want = R.avg_pool_case(shape)
        two = torch.nn.functional.avg_pool2d(x16.double()[..., 8:].permute(0, 3, 1, 2), 2, 2)
        assert _enough(int((E.round_f16_alt(two, "rtz") != want).sum()), want.numel())
    for family, shape in (("gather", (1, 33, 6, 11, 17, 3, 1, 1)), ("tile", (1, 33, 11, 12, 65, 3, 1, 1))):
        c = R.w32_case(family, shape)
        assert _enough(R.moved(c, c["unrounded"]), c["want"].numel())


@pytest.mark.parametrize("family", list(R.EDGE_SHAPES))
def test_overflow_and_underflow_cases_hold_their_counts(family):
    c = R.overflow_case(family)
    assert c["n_inf"] >= 8 and c["n_max"] >= 8 and int(torch.isinf(c["want"]).sum()) == c["n_inf"]
    assert int((c["want"].abs() == 65504.0).sum()) >= c["n_max"]
    clamped = torch.clamp(c["want"], -65504.0, 65504.0)                  # a conversion that clamps
    assert int((clamped != c["want"]).sum()) == c["n_inf"]
    u = R.underflow_case(family)
    flushed = torch.where(u["want"].abs() < 2.0 ** -14, torch.zeros_like(u["want"]), u["want"])      # a conversion that flushes subnormals
    assert u["n_sub"] >= 0.25 * u["want"].numel() and int((flushed != u["want"]).sum()) >= 0.25 * u["want"].numel()
    assert torch.equal(u["want"] * 2.0 ** 28 / 16.0, torch.round(u["want"] * 2.0 ** 28 / 16.0))      # multiples of 2^-24


def _sr_defects(evaluate, ref_maps, slopes, parts):
    """Each defect of `_round_cases.DEFECTS` through `evaluate(store, store_out)` -> dict of maps; it must move 5 % of at least one stored map."""
    for kind in R.DEFECTS:
        if kind == "slope" and not R.has_float32_slope(*slopes):
            continue
        store, store_out = R.sr_defect(kind, parts)
        alt = evaluate(store, store_out)
        assert any(_enough(int((alt[k] != ref_maps[k]).sum()), ref_maps[k].numel()) for k in ref_maps), (kind, {k: int((alt[k] != ref_maps[k]).sum()) for k in ref_maps})


STAGE_CASES = [(S, shape, sel, post) for S in (4, 2, 3) for shape in R.SR_SHAPES[S] for sel, post in ((False, False), (False, True), (True, False), (True, True))]


@pytest.mark.parametrize("S,shape,select,post", STAGE_CASES)
def test_stage_rounding_case_is_live_and_tells_every_defect(S, shape, select, post):
    c, ref = R.gen_round_stage(S, shape, select=select, post=post)
    maps = {k: ref[k] for k in (("out", "post") if post else ("out",))}     # (a 2 x 2 map holds 128 elements: the bar is 16 of them)
    parts = {"up": torch.nn.functional.conv_transpose2d(c["a"][:, :16], c["up_w"][:16], None, stride=S, padding=2)}
    _sr_defects(lambda st, so: R.eval_stage(c, post, store=st, store_out=so), maps, (c["up_a"], c["dt_a"], c["dn_a"]) + ((c["post_a"],) if post else ()), parts)


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("S", [4, 2, 3])
def test_a_defect_at_one_storage_point_of_a_stage_is_seen(S, select):
    """The defects one storage point at a time (the third shape of each scale, with POST): a wrong rounding or an activation on the other side
    at the deconvolution, the downtran, the output or the POST store ALONE moves 5 % of a stored map; so does the slope in the other format at
    the one point whose slope is no fp16 value."""
    shape = R.SR_SHAPES[S][2]
    c, ref = R.gen_round_stage(S, shape, select=select, post=True)
    maps = {k: ref[k] for k in ("out", "post")}
    for point in ("up", "dt", "dn", "post"):
        for kind in ("rtz", "away", "act_side") + (("slope",) if point == "post" else ()):
            st, so = R.sr_defect(kind, only=point)
            alt = R.eval_stage(c, True, store=st, store_out=so)
            moved = {k: int((alt[k] != maps[k]).sum()) for k in maps}
            assert any(_enough(moved[k], maps[k].numel()) for k in maps), (point, kind, moved)
            if point == "post":
                assert moved["out"] == 0
    c, ref = R.gen_round_stage(S, shape, select=select, post=False)       # (without POST the output's own slope is 0.2)
    st, so = R.sr_defect("slope", only="dn")
    assert _enough(int((R.eval_stage(c, False, store=st, store_out=so)["out"] != ref["out"]).sum()), ref["out"].numel())


@pytest.mark.parametrize("S", [4, 2, 3])
def test_stage_with_float32_weights_is_live(S):
    R.gen_round_stage_w32(S, R.SR_SHAPES[S][2])       # (raises unless the unrounded weights would move 5 % of the output)


TAIL_CASES = [(S, shape, fold, last) for S in (4, 2, 3) for shape in R.SR_SHAPES[S] for fold in ((False, True) if S == 4 else (True,) if S == 2 else (False,))
              for last in (False, True)]


@pytest.mark.parametrize("S,shape,fold,last", TAIL_CASES)
def test_tail_rounding_case_is_live_and_tells_every_defect(S, shape, fold, last):
    c, ref = R.gen_round_tail(S, shape, fold=fold, last=last)
    if last and ref["raw"].numel() < 512:
        return      # geometry only: with slope 0.2 conv_out reads ONE HR value per plane, 48 to 192 outputs in all; liveness is pooled below
    F = torch.nn.functional
    parts = ({"co": F.conv2d(c["lr_a"], c["co_w"][:, :32].reshape(32, 32, 1, 1))} if fold
             else {"out": F.conv_transpose2d(c["hid"][:, :16], c["out_w"][:16], None, stride=S, padding=2)})
    _sr_defects(lambda st, so: R.eval_tail(c, store=st), {"raw": ref["raw"]}, (c["out_a"],) + ((c["co_a"],) if fold else ()), parts)


@pytest.mark.parametrize("slopes", [(0.75, 0.2), (1.5, 0.1)])
@pytest.mark.parametrize("shape", [(3, 2, 2), (8, 9, 40), (2, 37, 33)])
def test_head_rounding_case_is_live_and_tells_every_defect(shape, slopes):
    c, ref = R.gen_round_head(shape, slopes=slopes)
    t = c["x"] * c["sub"][0].view(1, 3, 1, 1) + c["sub"][1].view(1, 3, 1, 1)
    parts = {"in": torch.nn.functional.conv2d(t[:, :1], c["w_in"][:, :1], None, padding=1)}
    _sr_defects(lambda st, so: R.eval_head(c, store=st), {"out": ref["out"]}, slopes, parts)


CHAIN_ROUND_SPECS = {"2-p": [(2, False, False), (0, True, False)], "2m-1p-p": [(2, False, True), (1, True, False), (0, True, False)],
                     "1m-1p-p": [(1, False, True), (1, True, False), (0, True, False)], "1-2p-1pm": [(1, False, False), (2, True, False), (1, True, True)]}


@pytest.mark.parametrize("N,P", [(2, 65), (3, 1000)])
@pytest.mark.parametrize("name", sorted(CHAIN_ROUND_SPECS))
def test_chain_rounding_case_is_live_and_tells_every_defect(name, N, P):
    stages, outs, _ = R.gen_round_chain(CHAIN_ROUND_SPECS[name], N, P)
    x, wm = stages[0]["ins"][0]
    parts = {"s0": torch.einsum("oc,ncp->nop", wm[:, :16], x[:, :16])}
    maps = {f"s{i}": o for i, o in enumerate(outs)}
    _sr_defects(lambda st, so: {f"s{i}": o for i, o in enumerate(E.chain_round_ref(stages, live=False, store=st)[0])}, maps, [s["slope"] for s in stages], parts)


@pytest.mark.parametrize("slope", [0.2, 1.5])
@pytest.mark.parametrize("nin,cm", [(1, False), (3, True)])
@pytest.mark.parametrize("N,P", [(2, 65), (3, 1000)])
def test_conv1x1_rounding_case_is_live_and_tells_every_defect(N, P, nin, cm, slope):
    stages, outs, _ = R.gen_round_chain([(nin, False, cm)], N, P, slopes=(slope,))
    x, wm = stages[0]["ins"][0]
    parts = {"s0": torch.einsum("oc,ncp->nop", wm[:, :16], x[:, :16])}
    _sr_defects(lambda st, so: {"s0": E.chain_round_ref(stages, live=False, store=st)[0][0]}, {"s0": outs[0]}, (slope,), parts)


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("shape", R.PRE_SHAPES)
def test_folded_chain_stage_rounding_case_is_live_and_tells_every_defect(shape, mode):
    c, ref = R.gen_round_pre(shape, mode)
    parts = {"up": torch.nn.functional.conv_transpose2d(c["a"][:, :16], c["up_w"][:16], None, stride=3, padding=2)}
    _sr_defects(lambda st, so: R.eval_stage(c, True, store=st, store_out=so), {k: ref[k] for k in ("out", "post")}, (c["up_a"], c["dt_a"], c["dn_a"], c["post_a"]), parts)


def test_small_sr_cases_meet_the_liveness_numbers_as_pools():
    """The 2 x 2 stage and tail cases and the 2 x 2 head hold maps below 512 elements: per storage point their pre-rounding sums are pooled
    over the cases, and each pool meets `check_rounds` (a quarter inexact, a twentieth ties, 16 ties each way, no overflow)."""
    pools = R.small_cases()
    assert set(pools) == {"stage output sum", "POST 1x1 sum", "compress_out sum", "feat_in sum"}, sorted(pools)
    for name, cases in pools.items():
        E.check_rounds_pool(list(cases.values()), f"{name}, pooled over {len(cases)} small cases")
