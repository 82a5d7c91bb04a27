"""The float32 FlowNet2 operators of csrc/flow_ops.hip (resample2d, channelnorm, correlation, warp_concat, warp_norms, the flow2img
colouring) and every kernel of csrc/flow_ops_bwd.hip (libvsr_hip_grad.so), bit for bit against references that do not run on the GPU.

References: tests/_flow_ref.py -- the formulas of include/vsr_hip.h and include/vsr_hip_grad.h evaluated in float64 on operands inside
checked budgets (integer images and gradients, flows `integer + k/8`, integer features), where a float32 kernel has exactly one right
answer whatever the order of its adds and whether or not its multiply-adds are contracted; the ChannelNorm gradient's three float32
operations restated in numpy float32 on Gaussian operands; and the project's C checker oracle/native.py for the forwards it restates.
tests/test_flow_ref_helper.py runs every reference and every budget without a GPU.  There is no tolerance in this file: every comparison
is `_exact.assert_exact` (count, first coordinate and bounding box of the differing elements).

Builds reached (per test, in the docstrings): the three template forms of k_resample2d_bwd in both modes, k_channelnorm_bwd<1> and <4>,
k_correlation_bwd with window rows of 1, 2, 3, 4, 5, 8, 14 and 15 pieces, and the first and the second trip of the grid-stride loop of every
thread-per-pixel kernel: they launch at most 2048 workgroups of 256, so above 524,288 pixels (vector elements for k_channelnorm_bwd<4>)
per batch item a thread takes a second one.  521 x 1009 = 525,689 pixels is an odd count 1,401 beyond that; 1028 x 2044 = 4 x 525,308.

What these cases cannot see: rounding behaviour (tests/test_gpu_flow_ops.py and test_gpu_flow_ops_grad.py keep covering it on Gaussian
operands) and overflow."""
import functools

import numpy as np
import pytest
import torch

import _exact as E
import _flow_ref as R
from test_gpu_flow_ops_grad import GEOMS

pytestmark = pytest.mark.gpu

from oracle import native  # noqa: E402
from video_super_resolution_amd import ops  # noqa: E402

assert R.CORR_CASES[:len(GEOMS)] == GEOMS      # every geometry of the gradient test is covered
CAP = R.GRID_CAP
ABOVE = (2, 2, 521, 1009)                      # 525,689 pixels: odd, CAP + 1,401
ABOVE_V4 = (1, 2, 1028, 2044)                  # 2,101,232 pixels = 4 x (CAP + 1,020)


def _dev(a):
    if isinstance(a, torch.Tensor):
        a = a.numpy()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


_exact = R.assert_exact_by_trip   # `_exact.assert_exact`, and above the cap: on which trip of the grid-stride loop the differing pixels lie


# ---------------------------------------------------------------------------------------------------------------- 1: Resample2d gradients
def _resample_grads(c, bilinear, need_img, need_flow):
    img, flow, gout = _dev(c["img"]), _dev(c["flow"]), _dev(c["gout"])
    d_img, d_flow = ops._resample2d_bwd(gout, img, flow, 1, bilinear, need_img, need_flow)
    assert (d_img is not None) == need_img and (d_flow is not None) == need_flow
    return d_img, d_flow


@pytest.mark.parametrize("bilinear", [True, False], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 17, 29), (1, 5, 7, 301), (3, 2, 5, 1)], ids=lambda s: "x".join(map(str, s)))
def test_resample2d_gradients_equal_float64(shape, bilinear):
    """k_resample2d_bwd<true,true>, <true,false> and <false,true>, bilinear and nearest, first trip; one pixel, a ragged last workgroup
    (7 x 301 = 2107 = 8 x 256 + 59), a one-column map, three images.  Samples clamp at each of the four borders and in the interior
    (asserted by the generator); flows of 1e9, -1e9 and 3e10 sit on top (the float -> int conversion saturates, the clamps follow it).
    d_img equals the float64 scatter, d_flow the float64 channel sum, the three forms agree bit for bit, and two runs of d_img are
    bit-identical.  That last claim holds ONLY in this regime: d_img is a scatter of float atomic adds, and on operands whose partial
    sums round the result depends on the order the adds arrive in (include/vsr_hip_grad.h); here no partial sum rounds."""
    c = R.resample_case(sum(shape), shape, far=True)
    r_img, r_flow = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"], bilinear)
    both_i, both_f = _resample_grads(c, bilinear, True, True)
    only_i, _ = _resample_grads(c, bilinear, True, False)
    _, only_f = _resample_grads(c, bilinear, False, True)
    again_i, _ = _resample_grads(c, bilinear, True, False)
    _exact(both_i, r_img, f"d_img (both gradients) {shape}")
    _exact(both_f, r_flow, f"d_flow (both gradients) {shape}")
    _exact(only_i, r_img, f"d_img alone {shape}")
    _exact(only_f, r_flow, f"d_flow alone {shape}")
    _exact(only_i, both_i.cpu(), "d_img alone against d_img of the form computing both")
    _exact(only_f, both_f.cpu(), "d_flow alone against d_flow of the form computing both")
    _exact(again_i, only_i.cpu(), "d_img, second run against the first")
    if not bilinear:
        assert not bool(both_f.any()) and not bool(only_f.any())


# ---------------------------------------------------------------------------------------------------------------- 2, 3: Correlation
CORR_IDS = [R.corr_id(c) for c in R.CORR_CASES]


def _geom_args(g):
    return (g["pad_size"], g["kernel_size"], g["max_displacement"], g["stride1"], g["stride2"])


@pytest.mark.parametrize("i", range(len(R.CORR_CASES)), ids=CORR_IDS)
def test_correlation_forward_equals_float64(i):
    """vsr_correlation_f32 (k_correlation: the float32 kernel of the exact configuration) on integers in [-3, 3]: the channel sum is
    exact in any order and chunking, the one multiplication by float32(1) / float32(C) is restated.  Every geometry of the gradient test,
    FlowNetC's with all 256 channels (8 LDS chunks), and three wide windows; C of 1, 33 and 40 among them (a ragged last chunk)."""
    c = R.corr_case(i)
    got = ops.correlation(_dev(c["f1"]), _dev(c["f2"]), **c["geom"])
    _exact(got, c["out"], f"correlation forward {CORR_IDS[i]}", names="nkyx")


@pytest.mark.parametrize("i", range(len(R.CORR_CASES)), ids=CORR_IDS)
def test_correlation_gradients_equal_float64(i):
    """k_correlation_bwd<false, NP> and <true, NP>; NP (32-column pieces of a window row) = 3, 2, 2, 2, 2, 1, 5, 15 for the gradient
    test's geometries, 3 for FlowNetC's at 8 x 16, and 4, 8, 14: builds no other test launches.  Integer gout in [-2, 2].  d_f1 and d_f2
    each alone (the other pointer null) and both in one call."""
    c = R.corr_case(i)
    f1, f2, gout, geom = _dev(c["f1"]), _dev(c["f2"]), _dev(c["gout"]), _geom_args(c["geom"])
    what = CORR_IDS[i] + f" (NP {R.window_pieces(c['geom'])})"
    both_1, both_2 = ops._correlation_bwd(gout, f1, f2, geom, True, True)
    only_1, none_2 = ops._correlation_bwd(gout, f1, f2, geom, True, False)
    none_1, only_2 = ops._correlation_bwd(gout, f1, f2, geom, False, True)
    assert none_1 is None and none_2 is None
    _exact(both_1, c["d_f1"], f"correlation d_f1 (both) {what}")
    _exact(both_2, c["d_f2"], f"correlation d_f2 (both) {what}")
    _exact(only_1, c["d_f1"], f"correlation d_f1 alone {what}")
    _exact(only_2, c["d_f2"], f"correlation d_f2 alone {what}")


# ---------------------------------------------------------------------------------------------------------------- 4: footprints
FOOT = [((2, 3, 19, 37), dict(pad_size=2, kernel_size=1, max_displacement=4, stride1=2, stride2=2)),    # stride1 2, pad < max_displacement
        ((1, 6, 9, 41), dict(pad_size=6, kernel_size=1, max_displacement=2, stride1=3, stride2=1))]     # pad > max_displacement


@pytest.mark.parametrize("shape,geom", FOOT, ids=[R.corr_id(c) for c in FOOT])
def test_correlation_gradient_footprint_of_one_unit(shape, geom):
    """gout = 1 at one element, 0 elsewhere: at the four output corners and one interior pixel, for the corner displacement
    (tj, ti) = (-R, +R) and the centre one.  With (y1, x1) = (oy, ox) * stride1 + max_displacement - pad_size and
    (y2, x2) = (y1 + tj * stride2, x1 + ti * stride2): d_f1 is f2[b, :, y2, x2] / C at (y1, x1) and d_f2 is f1[b, :, y1, x1] / C at
    (y2, x2) when both positions lie inside the image, and EVERYTHING else is exactly zero (with pad > max_displacement the corner
    output pixels look at the padding: nothing at all may be written but zeros).  Features are integers in [1, 3], so a footprint pixel
    is non-zero in every channel.  The expectation is written out here, element by element, not taken from `correlation_grads_ref`."""
    B, C, H, W = shape
    pad, md, s1, s2, Rr, D, OH, OW = R.corr_geometry(H, W, geom)
    rs = np.random.RandomState(7)
    f1, f2 = E.ints(rs, shape, 1, 3), E.ints(rs, shape, 1, 3)
    inv = np.float32(1.0) / np.float32(C)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W   # noqa: E731
    seen = set()
    for b, (oy, ox) in enumerate([(0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1), (OH // 2, OW // 2)]):
        b = b % B
        for tj, ti in ((-Rr, Rr), (0, 0)):
            gout = torch.zeros((B, D * D, OH, OW), dtype=torch.float64)
            gout[b, (tj + Rr) * D + ti + Rr, oy, ox] = 1.0
            y1, x1 = oy * s1 + md - pad, ox * s1 + md - pad
            y2, x2 = y1 + tj * s2, x1 + ti * s2
            w1, w2 = torch.zeros(shape, dtype=torch.float32), torch.zeros(shape, dtype=torch.float32)
            live = inside(y1, x1) and inside(y2, x2)
            seen.add(live)
            if live:
                w1[b, :, y1, x1] = torch.from_numpy(f2[b, :, y2, x2].numpy().astype(np.float32) * inv)
                w2[b, :, y2, x2] = torch.from_numpy(f1[b, :, y1, x1].numpy().astype(np.float32) * inv)
            d1, d2 = ops._correlation_bwd(_dev(gout), _dev(f1), _dev(f2), _geom_args(geom), True, True)
            what = f"unit at output ({oy}, {ox}) of image {b}, displacement ({tj}, {ti})"
            _exact(d1, w1, "d_f1, " + what)
            _exact(d2, w2, "d_f2, " + what)
            for d in (d1, d2):
                assert int((d != 0).any(1).sum()) == (1 if live else 0) and int((d != 0).sum()) == (C if live else 0), what
            # the formula reference says the same
            r1, r2 = R.correlation_grads_ref(f1, f2, gout, geom)
            assert torch.equal(r1, w1) and torch.equal(r2, w2), what
    assert True in seen, "no footprint inside the image: the case tests nothing"
    if pad > md:
        assert False in seen


# ---------------------------------------------------------------------------------------------------------------- 5: ChannelNorm gradient
def _channelnorm_case(shape, seed=9):
    rs = np.random.RandomState(seed)
    x = rs.randn(*shape).astype(np.float32)
    zy, zx = shape[2] // 2, shape[3] // 2
    x[0, :, zy, zx] = 0.0
    gout = rs.randn(shape[0], 1, shape[2], shape[3]).astype(np.float32)
    out = native.channelnorm(x)        # the forward's result (ops.channelnorm equals it bit for bit: test_gpu_flow_ops.py and below)
    assert out[0, 0, zy, zx] == 0.0
    return x, out, gout, (zy, zx)


def _channelnorm_grad(x, out, gout):
    return ops._channelnorm_bwd(_dev(gout), _dev(x), _dev(out))


@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (1, 2, 64, 128), (3, 7, 5, 1)], ids=lambda s: "x".join(map(str, s)))
def test_channelnorm_gradient_equals_its_float32_restatement(shape):
    """k_channelnorm_bwd<1> (17 x 19 and 5 x 1 pixels: no multiple of 4) and <4> (64 x 128: 16-byte accesses), first trip, Gaussian
    operands: (gout * in) * (1 / (out + 1e-9)) is an addition, a division and two multiplications, no sum and nothing to contract;
    the library is built without fast-math, so the division is the correctly rounded one and the result equals numpy's float32 bit for
    bit.  The pixel whose channels are all zero gets gradient 0."""
    x, out, gout, (zy, zx) = _channelnorm_case(shape)
    got = _channelnorm_grad(x, out, gout)
    _exact(got, R.channelnorm_grad_ref(x, out, gout), f"channelnorm gradient {shape}")
    assert not bool(got[0, :, zy, zx].any())


# ---------------------------------------------------------------------------------------------------------------- 6: above the grid cap
@functools.lru_cache(maxsize=None)
def _gauss_above():
    rs = np.random.RandomState(6)
    B, _, H, W = ABOVE
    x6 = rs.randn(B, 6, H, W).astype(np.float32)
    flow = (rs.randn(B, 2, H, W) * 6).astype(np.float32)
    warped = native.resample2d(x6[:, 3:], flow)
    return x6, flow, warped


def test_above_the_cap_resample2d_and_channelnorm_forward():
    """k_resample2d (bilinear and nearest) and k_channelnorm at 2 x 2 x 521 x 1009, second trip of their loops: bit equality with
    oracle/native_ops.c on Gaussian operands, as at the small sizes of tests/test_gpu_flow_ops.py."""
    x6, flow, _ = _gauss_above()
    img = x6[:, :2]
    assert img.shape == ABOVE and img.shape[2] * img.shape[3] == CAP + 1401
    for bilinear in (True, False):
        got = ops.resample2d(_dev(img), _dev(flow), bilinear=bilinear)
        _exact(got, torch.from_numpy(native.resample2d(img, flow, bilinear=bilinear)), f"resample2d bilinear={bilinear} {ABOVE}")
    _exact(ops.channelnorm(_dev(img)), torch.from_numpy(native.channelnorm(img)), f"channelnorm {ABOVE}")


def test_above_the_cap_fused_warp_concat_and_norms():
    """k_warp_concat and k_warp_norms at 2 x 6 x 521 x 1009, second trip: against their native compositions, as
    tests/test_gpu_flow_ops.py::test_fused_warp_concat_and_norms_bit_exact composes them.  Planes 9 and 10 are flow * inv_div with
    inv_div = float32(1 / 20) as ops.warp_concat passes it: that one float32 multiplication is restated, so these planes are compared
    bit for bit as well (the small-size test holds them to a relative bar against flow / 20)."""
    x6, flow, warped = _gauss_above()
    ndiff = native.channelnorm(x6[:, :3] - warped)
    ref12 = np.concatenate([x6, warped, flow * np.float32(1.0 / 20.0), ndiff], 1)
    assert ref12.dtype == np.float32
    out12 = ops.warp_concat(_dev(x6), _dev(flow), 20.0).cpu()
    _exact(out12[:, :9], torch.from_numpy(ref12[:, :9]), "warp_concat planes 0..8 (x6, warp)")
    _exact(out12[:, 9:11], torch.from_numpy(ref12[:, 9:11]), "warp_concat planes 9, 10 (flow * inv_div)")
    _exact(out12[:, 11:], torch.from_numpy(ref12[:, 11:]), "warp_concat plane 11 (|a - warp|)")
    nf, nd = ops.warp_norms(_dev(x6), _dev(flow))
    _exact(nf, torch.from_numpy(native.channelnorm(flow)), "warp_norms |flow|")
    _exact(nd, torch.from_numpy(ndiff), "warp_norms |a - warp|")


def test_above_the_cap_resample2d_gradients():
    """k_resample2d_bwd<true,true> in both modes at 2 x 2 x 521 x 1009 on exact operands with |flow| <= 4: pixels of the second trip
    scatter into pixels of the first and back (the last 1,401 pixels are rows 519 and 520; a flow of -4 rows reaches row 515)."""
    c = R.resample_case(8, ABOVE, mag=4)
    assert float(np.abs(c["flow"]).max()) <= 4.0
    for bilinear in (True, False):
        r_img, r_flow = R.resample2d_grads_ref(c["img"], c["flow"], c["gout"], bilinear)
        d_img, d_flow = _resample_grads(c, bilinear, True, True)
        _exact(d_img, r_img, f"d_img bilinear={bilinear} {ABOVE}")
        _exact(d_flow, r_flow, f"d_flow bilinear={bilinear} {ABOVE}")


@pytest.mark.parametrize("shape,build", [(ABOVE, 1), (ABOVE_V4, 4)], ids=["one-pixel-build", "16-byte-build"])
def test_above_the_cap_channelnorm_gradient(shape, build):
    """k_channelnorm_bwd<1> at 521 x 1009 (an odd pixel count: 1,401 pixels on the second trip) and k_channelnorm_bwd<4> at 1028 x 2044
    (a multiple of 4; torch's allocations are 16-byte aligned: 525,308 vector elements, 1,020 on the second trip)."""
    hw = shape[2] * shape[3]
    assert (hw % 4 == 0) == (build == 4) and hw // build > CAP
    x, out, gout, (zy, zx) = _channelnorm_case(shape, seed=10 + build)
    got = _channelnorm_grad(x, out, gout)
    _exact(got, R.channelnorm_grad_ref(x, out, gout), f"channelnorm gradient {shape}", per_thread=build)
    assert not bool(got[0, :, zy, zx].any())


# ---------------------------------------------------------------------------------------------------------------- 7: flow2img
def test_above_the_cap_flow2img_commutes_with_a_roll_of_the_rows():
    """k_flow_color at 521 x 1009.  A pixel's colour depends on its own flow and on the global maximum radius alone, and a roll of the
    rows changes neither: flow2img(rolled field) must be the rolled picture, bit for bit -- with 300 rows of shift, pixels coloured on
    the second trip of the loop in one run are coloured on the first trip in the other (and the maximum is reduced in another order)."""
    rs = np.random.RandomState(12)
    H, W = ABOVE[2:]
    field = torch.from_numpy((rs.randn(2, H, W) * rs.choice([0.01, 1.0, 30.0], size=(1, H, W))).astype(np.float32))
    a = ops.flow2img(field.cuda()).cpu()
    b = ops.flow2img(torch.roll(field, 300, dims=1).cuda()).cpu()
    assert tuple(a.shape) == (H, W, 3) and int(torch.unique(a).numel()) > 100
    m = E.diff_mask(b, torch.roll(a, 300, dims=0))
    if bool(m.any()):
        lin = torch.nonzero(m.any(2).flatten()).flatten()      # linear pixel index in the ROLLED picture
        src = (lin + (H - 300) * W) % (H * W)                  # ... and where that pixel sits in the unrolled one
        raise AssertionError(f"flow2img of the rolled field differs from the rolled picture at {int(m.any(2).sum())} pixels; first at linear "
                             f"index {int(lin[0])} (unrolled {int(src[0])}); second-trip pixels among them: {int((lin >= CAP).sum())} in the "
                             f"rolled run, {int((src >= CAP).sum())} in the unrolled run; box {E.bbox(m)}")
