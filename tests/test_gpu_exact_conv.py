"""The guidance trunks' convolutions in EXACT arithmetic: on small-integer / dyadic operands inside the budget that tests/_exact.py
checks, every route of every kernel must equal the float64 CPU evaluation bit for bit -- no tolerance anywhere in this file.

The Gaussian-operand tests (test_gpu_conv.py, test_gpu_conv_f32.py) hold the same kernels to 2e-3 / 2e-5 of the output range, where
one wrong term of a K = 9234 contraction is about as large as the bar; here it is one unit with coordinates.  Those tests stay: they
exercise rounding, which integers do not.

Every test that forces a route sets the cross-check library's switches inside a helper, which the conftest fixture cannot see in the
test's own source text: such tests carry `@pytest.mark.xcheck`, and `_switches` restores every knob in a `finally`.
The routes are asserted from `vsr_last_route()`, so a heuristic change cannot silently move a case to another kernel."""
import contextlib
import functools
import re

import numpy as np
import pytest
import torch

import _conv_cases as CC
import _exact as E
from _conv_cases import (ACTS, C1_CASES, DECONV_MODES, DECONV_SHAPES, GATHER_ROUTES, PAIR_CASES, PATCH_ROUTES, PATCH_SHAPES, PLAN_CONV, PLAN_DECONV, PLAN_STEM,
                         SHAPES, SPLIT_K_FILLS, SPLIT_K_SHAPES, STEM_CASES, TILE_SHAPES, TILE_SPLITS, TILE_WIDTHS)

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import _lib as L, igemm, trunk_f32  # noqa: E402

NONE, RELU, LEAKY = igemm.ACT_NONE, igemm.ACT_RELU, igemm.ACT_LEAKY
_DEFAULTS = (0, 1128, 2001, 4000, 5000, 6001, 7000, 8000, 9001)   # every knob of vsr_conv2d_tuning at its default


@contextlib.contextmanager
def _switches(*modes):
    lib = L.load()
    try:
        for m in modes:
            lib.vsr_conv2d_tuning(m)
        yield lib
    finally:
        for m in _DEFAULTS:
            lib.vsr_conv2d_tuning(m)


def _route():
    return L.load().vsr_last_route().decode()


def make_conv(seed, N, cin, H, W, cout, k, stride, pad, act=NONE, slope=0.1, step=1.0, transposed=False, store=torch.float16, mag_x=3, target=900.0):
    """Operands and float64 reference of one layer.  Weights are sparse so that the sums stay fp16 integers (sigma about 100), but every
    channel of the ragged last 32-chunk and channel 0 are dense: a defect there moves outputs.  Every image of a batch differs."""
    rs = np.random.RandomState(seed)
    x = E.ints(rs, (N, cin, H, W), -mag_x, mag_x, step)
    taps = 4 if transposed else k * k
    dens = min(1.0, target / (cin * taps))
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = E.sparse_weights(rs, shape, dens, 2, step)
    dense = E.sparse_weights(rs, shape, 1.0, 1, step)
    last = 32 * ((cin - 1) // 32)
    if cin - last < 32 or cin == 32:
        idx = [0] + list(range(last, cin)) if cin % 32 else [0, cin - 1]
        for c in idx:
            if transposed:
                w[c] = torch.where(w[c] == 0, dense[c], w[c])
            else:
                w[:, c] = torch.where(w[:, c] == 0, dense[:, c], w[:, c])
    b = E.ints(rs, (cout,), -4, 4, step)
    what = f"case {(N, cin, H, W, cout, k, stride, pad)}"
    pre = (E.deconv_ref if transposed else E.conv_ref)(x, w, b, stride=stride, padding=pad, what=what, store=store)
    E.check_live(pre, what, both_signs=pre.numel() >= 32, min_nonzero=0.5 if pre.numel() >= 32 else 0.0, min_distinct=100)
    want = E.act_ref(pre, act, slope, store=store)
    return dict(x=x, w=w, b=b, pre=pre, want=want, cout=cout, cin=cin, stride=stride, pad=pad, act=act, slope=slope)


def run_hconv(c, in_coff=0, in_extra=0, out_coff=0, out_extra=0, conv=None):
    """The case through igemm.HConv -> (NHWC output tensor, route).  Slices: the input sits at channels [in_coff, +pad32(cin)) of a wider
    buffer whose other channels hold 7.0 (never to be read); the output goes to [out_coff, +cout) of a buffer filled with 3.0."""
    x = c["x"]
    N, cin, H, W = x.shape
    cp = igemm.pad32(cin)
    xs = torch.full((N, H, W, in_coff + cp + in_extra), 7.0, dtype=torch.float16)
    xs[..., in_coff:in_coff + cp] = E.nhwc(x, torch.float16, cp)
    xs = xs.cuda()
    conv = conv or igemm.HConv(c["w"].float().cuda(), c["b"].float().cuda(), stride=c["stride"], pad=c["pad"], act=c["act"], slope=c["slope"])
    out = None
    if out_coff or out_extra:
        Ho, Wo = conv.out_hw(H, W)
        out = torch.full((N, Ho, Wo, igemm.pad32(out_coff + c["cout"]) + out_extra), 3.0, dtype=torch.float16, device="cuda")
    got = conv(xs, out=out, out_coff=out_coff, in_coff=in_coff)
    torch.cuda.synchronize()
    return got, _route()


def check_nhwc(got, c, what, out_coff=0, sliced=False):
    cout = c["cout"]
    E.assert_exact(E.nchw64(got[..., out_coff:out_coff + cout]), c["want"], what)
    rest = torch.cat([got[..., :out_coff], got[..., out_coff + cout:]], 3)
    if rest.numel():
        fill = 3.0 if sliced else 0.0   # a slice's neighbours keep their bits; the padding channels of an own buffer are exactly zero
        assert bool((rest == fill).all()), f"{what}: channels outside [{out_coff}, {out_coff + cout}) are not {fill}"


# ---------------------------------------------------------------------------------------------------------------- the gather kernel
@pytest.mark.xcheck
@pytest.mark.parametrize("route", list(GATHER_ROUTES))
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_gather_routes_equal_float64(i, route):
    """k_conv_igemm_d with 64- and 128-channel tiles, the first gather build k_conv_igemm, the five-set ring, and whatever the
    heuristic picks: each equals the float64 reference; activations cycle over none / ReLU / Leaky 0.25 / Leaky 0.1."""
    act, slope = ACTS[i % 4]
    c = make_conv(100 + i, *SHAPES[i], act=act, slope=slope, step=0.25 if i % 5 == 4 else 1.0)
    modes, pat = GATHER_ROUTES[route]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    if route == "gather128" and igemm._cout_pad(c["cout"]) % 128 == 0:
        assert r.startswith("gather<128>"), r
    check_nhwc(got, c, f"{SHAPES[i]} {r}")


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", SPLIT_K_SHAPES)
def test_gather_split_k_counts_agree_with_each_other_and_the_reference(shape):
    """Sums are exact, so split-K off, the default and every forced fill threshold (another split count each) give the SAME bits as
    each other and as float64 -- not only run-to-run identity."""
    c = make_conv(7, *shape, act=LEAKY, slope=0.1)
    seen = {}
    for fill in SPLIT_K_FILLS:
        with _switches(2000, 11, fill):
            got, r = run_hconv(c)
        assert r.startswith("gather<"), r
        seen[r] = got.clone()
        check_nhwc(got, c, f"{shape} {r}")
    assert any("splitk" not in r for r in seen) and any("splitk" in r for r in seen), sorted(seen)
    if shape[1] * shape[5] ** 2 >= 4000 and shape[4] >= 64:
        assert len([r for r in seen if "splitk" in r]) >= 2, sorted(seen)     # (a long K: several split counts)
    first = next(iter(seen.values()))
    assert all(torch.equal(v, first) for v in seen.values())


# ---------------------------------------------------------------------------------------------------------------- the tile kernel
@pytest.mark.xcheck
@pytest.mark.parametrize("i", range(len(TILE_SHAPES)))
def test_tile_kernel_widths_and_splits_equal_float64(i):
    """csrc/conv_tile.hip forced onto every layer: tile<64> and tile<128> (where the channel count allows), without split-K and with
    split counts 2, 3 and 7 -- all the same bits, all equal to float64."""
    act, slope = ACTS[(i + 1) % 4]
    c = make_conv(200 + i, *TILE_SHAPES[i], act=act, slope=slope, step=0.25 if i % 4 == 3 else 1.0)
    can128 = igemm._cout_pad(c["cout"]) % 128 == 0
    routes = set()
    for bn in TILE_WIDTHS:
        for splits in TILE_SPLITS:
            with _switches(2003, 4000 + bn, 5000 + splits):
                got, r = run_hconv(c)
            assert r.startswith(f"tile<{bn if (bn == 64 or can128) else 64}>"), r
            routes.add(r)
            check_nhwc(got, c, f"{TILE_SHAPES[i]} {r}")
    assert any("splitk" not in r for r in routes)
    if c["cin"] * TILE_SHAPES[i][5] ** 2 >= 32 * 16:
        assert any("splitk" in r for r in routes), routes


# ---------------------------------------------------------------------------------------------------------------- the LDS-patch kernels
_patch_routes_seen = {}


@pytest.mark.xcheck
@pytest.mark.parametrize("route", list(PATCH_ROUTES))
@pytest.mark.parametrize("i", range(len(PATCH_SHAPES)))
def test_patch_kernels_equal_float64(i, route):
    """k_conv_patch_r8, k_conv_patch_lw (weights in LDS), k_conv_patch_pf (modes 9002 / 9003), k_conv_patch_rows and k_conv_patch, each
    forced; a build that does not exist for a kernel size falls to the next one, which the route string shows."""
    N, cin, H, W, cout, k = PATCH_SHAPES[i]
    act, slope = ACTS[(i + 2) % 4]
    c = make_conv(300 + i, N, cin, H, W, cout, k, 1, k // 2, act=act, slope=slope, step=0.25 if i % 3 == 2 else 1.0)
    modes, pat = PATCH_ROUTES[route]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    _patch_routes_seen.setdefault(route, set()).add(r.split("<")[0])
    check_nhwc(got, c, f"{PATCH_SHAPES[i]} {r}")


def test_patch_cases_reached_every_build():
    """(runs after the cases above) each forced build served at least one of the cases that ran."""
    for route, want in (("patch_r8", "patch_r8"), ("patch_lw", "patch_lw"), ("patch_pf64", "patch_pf"), ("patch_pf32", "patch_pf"), ("patch_rows", "patch_rows"),
                        ("patch", "patch")):
        if len(_patch_routes_seen.get(route, ())) or len(_patch_routes_seen) == len(PATCH_ROUTES):
            assert want in _patch_routes_seen.get(route, ()), (route, _patch_routes_seen)


# ---------------------------------------------------------------------------------------------------------------- 1x1 streaming
@pytest.mark.xcheck
@pytest.mark.parametrize("case", C1_CASES)
def test_conv1x1_streaming_and_transposing_builds_equal_float64(case):
    N, cin, H, W, cout, act, slope, coff, extra = case
    c = make_conv(cin + cout, N, cin, H, W, cout, 1, 1, 0, act=act, slope=slope)
    for mode in (7000, 7001):
        with _switches(mode):
            got, r = run_hconv(c, out_coff=coff, out_extra=extra)
        want_r = "conv1x1_t" if (mode == 7001 and cin == 128 and cout % 8 == 0) else f"conv1x1_stream<{igemm.pad32(cin) // 32}>"
        assert r == want_r, (r, want_r)
        check_nhwc(got, c, f"{case} {r}", out_coff=coff, sliced=bool(coff or extra))


# ---------------------------------------------------------------------------------------------------------------- channel slices
@pytest.mark.xcheck
@pytest.mark.parametrize("modes", [(), (2000, 11), (2003,), (2, 2000, 6000, 9000)])
def test_channel_slice_source_and_destination(modes):
    """in_coff / out_coff / out_ld: the input is a slice of a wider buffer (its other channels hold 7.0), the output a slice of a
    buffer filled with 3.0: the slice is exact, every neighbour keeps its bits."""
    c = make_conv(41, 2, 40, 9, 17, 72, 3, 1, 1, act=RELU)
    with _switches(*modes):
        got, r = run_hconv(c, in_coff=24, in_extra=8, out_coff=40, out_extra=16)
    check_nhwc(got, c, f"slices {r}", out_coff=40, sliced=True)
    c = make_conv(42, 1, 64, 6, 20, 16, 3, 1, 1, act=LEAKY, slope=0.1)
    with _switches(*modes):
        got, r = run_hconv(c, in_coff=8, in_extra=24, out_coff=5, out_extra=0)
    check_nhwc(got, c, f"slices {r}", out_coff=5, sliced=True)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.xcheck
@pytest.mark.parametrize("modes", [(), (2000, 11, 1000), (2, 2000, 6000, 9000)])
def test_one_unit_in_one_weight_of_k_9234_is_seen_with_its_footprint(modes):
    """The kernel gets a weight tensor in which ONE element of the last K block (channel 1025, the centre tap, out-channel 1) differs by
    one unit from what the reference gets.  The comparison must fail and the differing outputs must be exactly out-channel 1 at the
    pixels whose centre input is non-zero.  Ordinary data: under the Gaussian tests this defect is at the 2e-3 bar and passes by seed."""
    c = make_conv(9234, 1, 1026, 16, 16, 2, 3, 1, 1)
    w2 = c["w"].clone()
    w2[1, 1025, 1, 1] += 1.0
    conv = igemm.HConv(w2.float().cuda(), c["b"].float().cuda(), stride=1, pad=1)
    with _switches(*modes):
        got, r = run_hconv(c, conv=conv)
    got = E.nchw64(got, 2)
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got, c["want"], r)
    pred = torch.zeros_like(c["want"], dtype=torch.bool)
    pred[:, 1] = c["x"][:, 1025] != 0
    assert pred.sum() > 100 and torch.equal(E.diff_mask(got, c["want"]), pred), (r, E.bbox(E.diff_mask(got, c["want"])))


# ---------------------------------------------------------------------------------------------------------------- other fp16 layers
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_convolution_equals_float64(case):
    N, cin, H, W, cout, k, s, p, act, slope = case
    c = make_conv(cout + k, N, cin, H, W, cout, k, s, p, act=act, slope=slope, mag_x=8)
    stem = igemm.HConvStem(c["w"].float().cuda(), c["b"].float().cuda(), stride=s, pad=p, act=act, slope=slope)
    got = stem(E.nhwc(c["x"], torch.float16, 4).cuda())
    r = _route()
    assert r == ("stem7_rows" if H * W * N >= 65536 else r) and (r.startswith("gather<") or r == "stem7_rows"), r
    check_nhwc(got, c, f"stem {case} {r}")


@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_convolution_stride2_equals_float64(case):
    N, cin, H, W, cout, k, pad = case
    c = make_conv(cin + k + W, N, cin, H, W, cout, k, 2, pad, act=LEAKY, slope=0.1)
    conv = igemm.HConvPairS2(c["w"].float().cuda(), c["b"].float().cuda(), pad=pad, act=LEAKY, slope=0.1)
    got = conv(E.nhwc(c["x"], torch.float16, 16).cuda())
    assert _route().startswith("gather<") or _route().startswith("tile<"), _route()
    check_nhwc(got, c, f"pair {case}")


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", DECONV_SHAPES)
def test_transposed_convolution_k4s2_equals_float64(shape):
    """HDeconv4s2: four phases in one launch, through the heuristic's route, the gather kernel and (wide layers) the tile kernel."""
    N, cin, H, W, cout = shape
    c = make_conv(cin + cout, N, cin, H, W, cout, 4, 2, 1, act=LEAKY, slope=0.1, transposed=True)
    dc = igemm.HDeconv4s2(c["w"].float().cuda(), c["b"].float().cuda(), act=LEAKY, slope=0.1)
    xs = E.nhwc(c["x"], torch.float16, igemm.pad32(cin)).cuda()
    for modes, pat in zip(DECONV_MODES, (r"deconv4s2", r"deconv4s2 gather<", r"deconv4s2 tile<" if cout > 32 else r"deconv4s2")):
        with _switches(*modes):
            got = dc(xs)
            torch.cuda.synchronize()
            r = _route()
        assert re.match(pat, r), r
        check_nhwc(got, c, f"deconv4s2 {shape} {r}")
    if H * W >= 8192:
        with _switches():
            dc(xs)
            assert _route() == "deconv4s2_patch", _route()


FLOW_HEAD_CASES = [(2, 1024, 8, 15, 0, True, True), (1, 1026, 5, 7, 32, True, False), (1, 194, 33, 40, 32, False, False), (1, 33, 21, 50, 0, True, True),
                   (3, 16, 9, 7, 16, False, False), (1, 512, 1, 3, 0, True, False), (1, 31, 6, 1, 0, True, True),
                   (1, 33, 97, 170, 32, False, False), (1, 40, 129, 128, 0, True, True)]   # from 16,384 pixels: the 8 x 8 tiles, ragged in both directions
HG_FRONT_SHAPES = [(2, 9, 11, 48), (1, 16, 32, 8), (1, 5, 64, 208)]
_self_named_seen = []   # the route of every flow-head / hourglass-front case that ran


@pytest.mark.parametrize("case", FLOW_HEAD_CASES)
def test_flow_head_equals_float64(case):
    """HFlowHead: predict_flow (3x3, 2 outputs) and the fused ConvTranspose2d(2, 2, 4, 2, 1) of the kernel's fp16 flow into a slice."""
    N, cin, H, W, extra, with_up, up_bias = case
    c = make_conv(cin + H, N, cin, H, W, 2, 3, 1, 1, target=100.0)
    rs = np.random.RandomState(cin)
    wu = E.sparse_weights(rs, (2, 2, 4, 4), 1.0, 2, 0.25) if with_up else None
    bu = E.ints(rs, (2,), -3, 3, 0.5) if (with_up and up_bias) else None
    head = igemm.HFlowHead(c["w"].float().cuda(), c["b"].float().cuda(), None if wu is None else wu.float().cuda(), None if bu is None else bu.float().cuda())
    cp = igemm.pad32(cin)
    xs = torch.full((N, H, W, cp + extra), 7.0, dtype=torch.float16)
    xs[..., :cp] = E.nhwc(c["x"], torch.float16, cp)
    up_out = torch.full((N, 2 * H, 2 * W, 32), 3.0, dtype=torch.float16, device="cuda") if with_up else None
    flow = head(xs.cuda(), up_out=up_out, up_coff=6)
    r = _route()
    assert r == "flow_head<%s,%d>" % ("4,4" if N * H * W < 16384 else "8,8", 2 if with_up else 1), r
    _self_named_seen.append(r)
    check_nhwc(flow, c, f"flow head {case} {r}")
    if with_up:
        up = E.deconv_ref(c["want"], wu, bu, stride=2, padding=1, what="flow upsampling", store=torch.float16)
        E.assert_exact(E.nchw64(up_out[..., 6:8]), up, f"flow upsampling {case}")
        assert bool((up_out[..., :6] == 3.0).all()) and bool((up_out[..., 8:] == 3.0).all())


@pytest.mark.parametrize("shape", HG_FRONT_SHAPES)
def test_hourglass_front_equals_float64(shape):
    """HHourglassFront: 7x7 stem (3 -> 128) + ReLU, its 2x2 max pool and the 1x1 + ReLU on it, one launch, three outputs."""
    N, H, W, c2 = shape
    s = make_conv(H, N, 3, H, W, 128, 7, 1, 3, act=RELU, mag_x=8)
    rs = np.random.RandomState(W)
    w1 = E.sparse_weights(rs, (c2, 128, 1, 1), 0.1, 1)
    b1 = E.ints(rs, (c2,), -4, 4)
    one = torch.relu(E.conv_ref(s["want"], w1, b1, what="hourglass 1x1", store=torch.float16))
    pool = torch.nn.functional.max_pool2d(s["want"], 2, 2)
    front = igemm.HHourglassFront(igemm.HConvStem(s["w"].float().cuda(), s["b"].float().cuda(), stride=1, pad=3, act=RELU),
                                  igemm.HConv(w1.float().cuda(), b1.float().cuda(), act=RELU))
    out2 = torch.full((N, H, W, igemm.pad32(c2) + 32), 3.0, dtype=torch.float16, device="cuda")
    pooled = torch.full((N, H // 2, W // 2, 128), 3.0, dtype=torch.float16, device="cuda")
    stem_out = torch.full((N, H, W, 160), 3.0, dtype=torch.float16, device="cuda")
    front(E.nhwc(s["x"], torch.float16, 4).cuda(), out2, pooled=pooled, stem_out=stem_out)
    assert _route() == "hg_front"
    _self_named_seen.append(_route())
    E.assert_exact(E.nchw64(stem_out, 128), s["want"], "hourglass stem")
    E.assert_exact(E.nchw64(pooled), pool, "hourglass pooled stem")
    E.assert_exact(E.nchw64(out2, c2), one, "hourglass 1x1")
    assert bool((stem_out[..., 128:] == 3.0).all()) and bool((out2[..., c2:] == 3.0).all())


def test_self_named_routes_of_the_trunks_all_ran():
    """(runs after the cases above) `flow_head<..>` and `hg_front` have no plan function: every such route the trunks launch at the BASELINE
    sizes (tests/golden/g14_trunk_layers.json, `self_named`) was the route of a case above."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_trunk_layers.json")) as f:
        want = {r for r in json.load(f)["self_named"] if r.startswith(("flow_head<", "hg_front"))}
    assert len(want) >= 4
    if len(_self_named_seen) >= len(FLOW_HEAD_CASES) + len(HG_FRONT_SHAPES):   # (the whole file ran, not a selection of its cases)
        assert want <= set(_self_named_seen), sorted(want - set(_self_named_seen))


@pytest.mark.parametrize("shape", [(2, 9, 7, 16), (1, 2, 2, 8), (3, 5, 33, 40), (1, 34, 3, 128)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pool_and_layout_conversions_equal_float64(shape, mode):
    """pool2x2 (max, average, max with ceil_mode) on a channel slice; to_nhwc_half / to_nchw_float.  Multiples of 1/4 in -8..8: the
    average of four is a multiple of 1/16, an fp16 value."""
    N, H, W, C = shape
    rs = np.random.RandomState(H + W + mode)
    x = E.ints(rs, (N, C + 8, H, W), -32, 32, 0.25)
    xs = igemm.to_nhwc_half(x.float().cuda(), C + 8)
    E.assert_exact(E.nchw64(xs), x, "to_nhwc_half")
    E.assert_exact(igemm.to_nchw_float(xs, C + 8), x, "to_nchw_float")
    padded = igemm.to_nhwc_half(x[:, :5].float().cuda())
    E.assert_exact(E.nchw64(padded, 5), x[:, :5], "to_nhwc_half padded")
    assert padded.shape[3] == 32 and bool((padded[..., 5:] == 0).all())
    got = igemm.pool2x2(xs, 8, C, mode)
    xn = x[:, 8:]
    ref = torch.nn.functional.avg_pool2d(xn, 2, 2) if mode == 1 else torch.nn.functional.max_pool2d(xn, 2, 2, ceil_mode=(mode == 2))
    E.assert_exact(E.nchw64(got), ref, f"pool2x2 mode {mode}")


# ---------------------------------------------------------------------------------------------------------------- the route plan
def _plan(kind, conv, N, H, W, in_ld, out_ld, out_coff=0, out_hw=None, stride_x=0):
    """The route vsr_conv2d_plan names for the launch `conv` (an HConv, an HConvStem or phase 0 of an HDeconv4s2) is about to make."""
    from test_conv_route_plan import plan_route
    if kind == 1:
        Ho, Wo = (H + 2 * conv.pad - conv.kh) // conv.stride + 1, (W + 2 * conv.pad - conv.kw) // conv.stride + 1
        args = (4, N, H, W, 32, Ho, Wo, conv.cout, conv.cout_pad, conv.kh, conv.kw, conv.stride, 0, conv.pad, conv.pad, out_ld, out_coff, Ho, Wo, 1, 0, 1, 0)
    else:
        Ho, Wo = out_hw or conv.out_hw(H, W)
        args = (in_ld, N, H, W, conv.cin_pad, Ho, Wo, conv.cout, conv.cout_pad, conv.kh, conv.kw, conv.stride, stride_x, conv.pad_y, conv.pad_x, out_ld, out_coff,
                Ho * conv.oy[0], Wo * conv.ox[0], conv.oy[0], conv.oy[1], conv.ox[0], conv.ox[1])
    return plan_route(L.load(), kind, args, 1, igemm._WS_BYTES)


@pytest.mark.xcheck
@pytest.mark.parametrize("i", range(len(PLAN_CONV)))
def test_plan_names_the_route_the_convolution_takes(i):
    """vsr_conv2d_plan (no launch) and vsr_last_route() after the launch of the same layer, under the same switches: one string; the
    launch equals float64."""
    shape, modes = PLAN_CONV[i]
    c = make_conv(600 + i, *shape, act=ACTS[i % 4][0], slope=ACTS[i % 4][1])
    conv = igemm.HConv(c["w"].float().cuda(), c["b"].float().cuda(), stride=c["stride"], pad=c["pad"], act=c["act"], slope=c["slope"])
    N, cin, H, W = c["x"].shape
    with _switches(*modes):
        planned = _plan(0, conv, N, H, W, igemm.pad32(cin), igemm.pad32(c["cout"]))
        got, r = run_hconv(c, conv=conv)
    assert planned == r, (planned, r)
    check_nhwc(got, c, f"{shape} {r}")


@pytest.mark.xcheck
def test_plan_routes_cover_split_k_and_every_family():
    """The case list itself: the plan of PLAN_CONV's layers under their switches (no launch here; that each launch takes the planned route is
    the test above) names gather with and without split-K, the tile kernel with and without, each patch build and both 1x1 builds."""
    seen = set()
    for shape, modes in PLAN_CONV:
        N, cin, H, W, cout, k, stride, pad = shape
        conv = igemm.HConv(torch.zeros(cout, cin, k, k), None, stride=stride, pad=pad)   # (host tensors: only its geometry is read)
        with _switches(*modes):
            seen.add(re.sub(r"<.*?>|(?<=splitk)\d+", "", _plan(0, conv, N, H, W, igemm.pad32(cin), igemm.pad32(cout))))
    assert seen >= {"gather", "gather+splitk", "tile", "tile+splitk", "patch_pf", "patch_lw", "patch_r8", "patch_rows", "patch", "conv1x1_stream", "conv1x1_t"}, seen


@pytest.mark.xcheck
@pytest.mark.parametrize("case", PLAN_STEM)
def test_plan_names_the_route_the_stem_takes(case):
    N, cin, H, W, cout, k, s, p = case
    c = make_conv(cout + k, N, cin, H, W, cout, k, s, p, act=RELU, mag_x=8)
    stem = igemm.HConvStem(c["w"].float().cuda(), c["b"].float().cuda(), stride=s, pad=p, act=RELU)
    planned = _plan(1, stem, N, H, W, 4, igemm.pad32(cout))
    got = stem(E.nhwc(c["x"], torch.float16, 4).cuda())
    assert planned == _route() and planned == ("stem7_rows" if H * W * N >= 65536 else f"gather<{min(64, igemm._cout_pad(cout))},stem>"), (planned, _route())
    check_nhwc(got, c, f"stem {case} {planned}")


@pytest.mark.xcheck
@pytest.mark.parametrize("shape,modes", PLAN_DECONV)
def test_plan_names_the_route_the_transposed_convolution_takes(shape, modes):
    N, cin, H, W, cout = shape
    c = make_conv(cin + cout, N, cin, H, W, cout, 4, 2, 1, act=LEAKY, slope=0.1, transposed=True)
    dc = igemm.HDeconv4s2(c["w"].float().cuda(), c["b"].float().cuda(), act=LEAKY, slope=0.1)
    xs = E.nhwc(c["x"], torch.float16, igemm.pad32(cin)).cuda()
    with _switches(*modes):
        planned = _plan(2, dc.phases[0], N, H, W, igemm.pad32(cin), igemm.pad32(cout))
        got = dc(xs)
        torch.cuda.synchronize()
        r = _route()
    assert planned == r and r.startswith("deconv4s2"), (planned, r)
    check_nhwc(got, c, f"deconv4s2 {shape} {r}")


@pytest.mark.xcheck
def test_plan_names_the_route_the_pair_convolution_takes():
    N, cin, H, W, cout, k, pad = PAIR_CASES[0]
    c = make_conv(cin + k + W, N, cin, H, W, cout, k, 2, pad, act=LEAKY, slope=0.1)
    conv = igemm.HConvPairS2(c["w"].float().cuda(), c["b"].float().cuda(), pad=pad, act=LEAKY, slope=0.1)
    planned = _plan(0, conv.inner, N, H, W // 2, 32, igemm.pad32(cout), out_hw=((H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1), stride_x=1)
    got = conv(E.nhwc(c["x"], torch.float16, 16).cuda())
    r = _route()
    assert planned == r, (planned, r)
    check_nhwc(got, c, f"pair {r}")


# ---------------------------------------------------------------------------------------------------------------- one case per production build
@functools.lru_cache(maxsize=None)
def _build_case(i):
    """Operands and float64 reference of BUILD_CASES[i]: computed once, shared by the tests below, never modified."""
    kind, shape, _, (act, slope) = CC.BUILD_CASES[i]
    if kind == CC.DECONV:
        N, cin, H, W, cout = shape
        return make_conv(700 + i, N, cin, H, W, cout, 4, 2, 1, act=act, slope=slope, transposed=True)
    return make_conv(700 + i, *shape, act=act, slope=slope, mag_x=8 if kind == CC.STEM else 3)


def _run_build_case(i, w=None):
    """BUILD_CASES[i] through the igemm class of its kind, under its switches, with the weights `w` (default: the reference's) ->
    (planned route, NHWC output, route of the launch)."""
    kind, shape, modes, (act, slope) = CC.BUILD_CASES[i]
    c = _build_case(i)
    w = (c["w"] if w is None else w).float().cuda()
    b = c["b"].float().cuda()
    N, cin, H, W = c["x"].shape
    cout = c["cout"]
    with _switches(*modes):
        if kind == CC.CONV:
            conv = igemm.HConv(w, b, stride=c["stride"], pad=c["pad"], act=act, slope=slope)
            planned = _plan(0, conv, N, H, W, igemm.pad32(cin), igemm.pad32(cout))
            got, r = run_hconv(c, conv=conv)
            return planned, got, r
        if kind == CC.STEM:
            stem = igemm.HConvStem(w, b, stride=c["stride"], pad=c["pad"], act=act, slope=slope)
            planned = _plan(1, stem, N, H, W, 4, igemm.pad32(cout))
            got = stem(E.nhwc(c["x"], torch.float16, 4).cuda())
        elif kind == CC.PAIR:
            k, pad = shape[5], shape[7]
            conv = igemm.HConvPairS2(w, b, pad=pad, act=act, slope=slope)
            planned = _plan(0, conv.inner, N, H, W // 2, 32, igemm.pad32(cout), out_hw=((H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1), stride_x=1)
            got = conv(E.nhwc(c["x"], torch.float16, 16).cuda())
        else:
            dc = igemm.HDeconv4s2(w, b, act=act, slope=slope)
            planned = _plan(2, dc.phases[0], N, H, W, igemm.pad32(cin), igemm.pad32(cout))
            got = dc(E.nhwc(c["x"], torch.float16, igemm.pad32(cin)).cuda())
        torch.cuda.synchronize()
        return planned, got, _route()


@pytest.mark.xcheck
@pytest.mark.parametrize("i", range(len(CC.BUILD_CASES)))
def test_every_production_build_equals_float64(i):
    """One case per kernel build that the trunks launch at the BASELINE sizes and no other table of tests/_conv_cases.py plans to
    (tests/test_conv_build_census.py keeps that list complete): the launch takes the planned route -- the whole string, template
    arguments included -- and equals float64 bit for bit."""
    planned, got, r = _run_build_case(i)
    assert planned == r, (planned, r)
    import test_conv_build_census as census
    assert census.build_key(r, *_kh_stride(i)) == census.case_keys([CC.BUILD_CASES[i]])[0]   # (the census planned the launch that ran)
    check_nhwc(got, _build_case(i), f"{CC.BUILD_CASES[i][:3]} {r}")


def _kh_stride(i):
    kind, shape = CC.BUILD_CASES[i][:2]
    return (2, 1) if kind == CC.DECONV else (shape[5], shape[6])


# one case per template family that gained a build above: (row of BUILD_CASES, the family)
SENSITIVITY = [(3, "patch_r8<11,2>"), (4, "patch_lw<3,4>"), (8, "gather<128>"), (12, "tile<64>"), (16, "conv1x1_stream<8>")]


@pytest.mark.xcheck
@pytest.mark.parametrize("i,route", SENSITIVITY)
def test_one_unit_in_one_weight_of_a_production_build_is_seen_with_its_footprint(i, route):
    """The kernel gets weights in which ONE element differs by one unit from what the reference gets: the last out-channel, the last
    input channel (the ragged 32-chunk), the bottom-left tap.  The comparison with the reference must fail, the outputs that differ
    must be exactly those the changed product reaches THROUGH the activation, and the whole result must equal the float64 evaluation
    with that weight."""
    kind, shape, _, (act, slope) = CC.BUILD_CASES[i]
    assert kind == CC.CONV
    N, cin, H, W, cout, k, s, p = shape
    c = _build_case(i)
    co, ci, ky, kx = cout - 1, cin - 1, k - 1, 0
    w2 = c["w"].clone()
    w2[co, ci, ky, kx] += 1.0
    _, got, r = _run_build_case(i, w=w2)
    assert r.startswith(route), r
    Ho, Wo = c["want"].shape[2:]
    xp = torch.nn.functional.pad(c["x"][:, ci], (p, p, p, p))
    pre2 = c["pre"].clone()
    pre2[:, co] += xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
    want2 = E.act_ref(pre2, act, slope)
    pred = want2 != c["want"]
    assert 50 < int(pred.sum()) and not bool(pred[:, :co].any())
    got = E.nchw64(got, cout)
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got, c["want"], r)
    assert torch.equal(E.diff_mask(got, c["want"]), pred), (r, E.bbox(E.diff_mask(got, c["want"])), E.bbox(pred))
    E.assert_exact(got, want2, f"{shape} {r} with the changed weight")


# ---------------------------------------------------------------------------------------------------------------- the FlowNetC cost volume
def _corr_ref(a, b):
    """[B,C,H,W] float64 -> [B,441,H,W]: sum_c a(y, x) b(y + 2 dy, x + 2 dx) / C for dy, dx in -10..10 (zero outside), dy major."""
    B, C, H, W = a.shape
    bp = torch.nn.functional.pad(b, (20, 20, 20, 20))
    out = torch.empty((B, 441, H, W), dtype=torch.float64)
    asum = torch.empty_like(out)
    for j, dy in enumerate(range(-10, 11)):
        for i, dx in enumerate(range(-10, 11)):
            win = bp[:, :, 20 + 2 * dy:20 + 2 * dy + H, 20 + 2 * dx:20 + 2 * dx + W]
            out[:, j * 21 + i] = (a * win).sum(1)
            asum[:, j * 21 + i] = (a.abs() * win.abs()).sum(1)
    E.check_sum_budget(asum, E.granularity(a) * E.granularity(b), "cost volume")
    return out / C        # (the kernels multiply by 1.0f / C: exact for a power of two)


@pytest.mark.parametrize("shape", [(2, 5, 1, 64), (1, 7, 37, 256), (1, 3, 150, 32), (1, 26, 45, 128)])
def test_flownetc_cost_volume_both_builds_equal_float64(shape):
    """vsr_correlation_f32 and the fp16 NHWC MFMA build (LeakyReLU 0.1 fused, written into a concat-buffer slice whose neighbours keep
    their bits); widths 1, 37, 45 and 150 (several 32-pixel blocks with the widest window)."""
    from video_super_resolution_amd import ops
    B, H, W, C = shape
    rs = np.random.RandomState(H * W)
    a, b = E.ints(rs, (B, C, H, W), -3, 3, 0.5), E.ints(rs, (B, C, H, W), -3, 3)
    ref = _corr_ref(a, b)
    E.check_live(ref, "cost volume", min_nonzero=0.2 if min(H, W) >= 30 else 0.0, min_distinct=50 if min(H, W) >= 3 else 8)
    got32 = ops.correlation(a.float().cuda(), b.float().cuda(), 20, 1, 20, 1, 2)
    E.assert_exact(got32, ref, f"vsr_correlation_f32 {shape}")
    out = torch.full((B, H, W, 480), 7.0, dtype=torch.float16, device="cuda")
    ah, bh = E.nhwc(a).cuda(), E.nhwc(b).cuda()
    L.check(L.load().vsr_flownetc_corr_nhwc_f16(L.dptr(ah, torch.float16), L.dptr(bh, torch.float16), L.dptr(out, torch.float16),
                                                480, 32, B, H, W, C, L.stream()))
    E.assert_exact(E.nchw64(out[..., 32:473]), E.leaky_tenth_f16(ref), f"vsr_flownetc_corr_nhwc_f16 {shape}")
    assert bool((out[..., :32] == 7.0).all()) and bool((out[..., 473:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- float32 routes
F32_CASES = [  # (N, C, H, W, Co, kh, pad, stride, route, route string pattern)
    (1, 64, 9, 21, 16, 11, 5, 1, 2, r"f32 sp16"), (2, 33, 11, 37, 16, 7, 3, 1, 2, r"f32 sp16"), (1, 65, 17, 33, 1, 3, 1, 1, 2, r"f32 sp16"),
    (1, 31, 20, 40, 32, 7, 3, 1, 2, r"f32 sp<"), (2, 64, 19, 37, 65, 3, 1, 1, 2, r"f32 sp<"), (1, 129, 9, 64, 128, 3, 1, 1, 2, r"f32 sp<"),
    (1, 6, 10, 35, 64, 3, 1, 1, 2, r"f32 sp<"), (1, 32, 7, 20, 24, 3, 0, 1, 2, r"f32 sp<"),
    (1, 64, 9, 21, 16, 11, 5, 1, 1, r"f32 flat<1>"), (1, 473, 8, 16, 256, 3, 1, 1, 1, r"f32 flat<4>"), (1, 256, 9, 13, 192, 3, 1, 2, 1, r"f32 flat<2>"),
    (3, 1, 5, 7, 1, 3, 1, 1, 1, r"f32 flat<1>"), (1, 17, 1, 300, 48, 3, 1, 1, 1, r"f32 flat<2>"), (1, 33, 150, 1, 2, 1, 0, 1, 1, r"f32 flat<1>"),
    (2, 1026, 4, 6, 2, 3, 1, 1, 1, r"f32 head"), (1, 256, 8, 15, 2, 3, 1, 1, 1, r"f32 head"), (1, 770, 5, 1, 2, 3, 1, 1, 1, r"f32 head"),
]


@pytest.mark.parametrize("i", range(len(F32_CASES)))
def test_float32_routes_equal_float64(i):
    """trunk_f32.conv2d_fused with the route passed explicitly: flat k_conv_f32, spatial k_conv_f32_sp, thin k_conv_f32_sp16 and
    k_conv_f32_head, with a folded BatchNorm (power-of-two scale, integer shift), ReLU / LeakyReLU and a concat-slice destination.
    float32 holds integers up to 2^24, so the operands are wider (-40..40) than in the fp16 cases."""
    N, C, H, W, Co, k, pad, stride, route, pat = F32_CASES[i]
    rs = np.random.RandomState(500 + i)
    x = E.ints(rs, (N, C, H, W), -40, 40)
    w = E.sparse_weights(rs, (Co, C, k, k), min(1.0, 2000.0 / (C * k * k)), 30)
    w[:, C - 1] = torch.where(w[:, C - 1] == 0, torch.ones_like(w[:, C - 1]), w[:, C - 1])
    b = E.ints(rs, (Co,), -100, 100)
    pre = E.conv_ref(x, w, None, stride=stride, padding=pad, what=f"f32 case {i}", store=torch.float32)
    kind = i % 4          # 0: bias; 1: BatchNorm + ReLU into a slice; 2: LeakyReLU 0.25; 3: BatchNorm + LeakyReLU 0.1
    scale = shift = None
    coff, ctot = (0, Co)
    if kind in (1, 3):
        sc = torch.from_numpy(2.0 ** rs.randint(-2, 3, size=Co))
        ref = pre * sc.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        scale, shift = sc.float().cuda(), b.float().cuda()
        coff, ctot = (8, Co + 19)
    else:
        ref = pre + b.view(1, -1, 1, 1)
        shift = b.float().cuda()
    E.check_storable(ref, torch.float32, "scaled sum")
    act, slope = ((False, 0.0), (True, 0.0), (True, 0.25), (True, 0.1))[kind]
    if act:
        ref = E.leaky_tenth_f32(ref) if slope == 0.1 else torch.nn.functional.leaky_relu(ref, slope)
    wp = trunk_f32._pack(w.float().cuda().contiguous())
    out = torch.full((N, ctot, ref.shape[2], ref.shape[3]), 7.0, dtype=torch.float32, device="cuda")
    trunk_f32.conv2d_fused(x.float().cuda(), wp, scale, shift, act, slope, Co, k, k, stride, pad, pad, route, out=out, coff=coff)
    r = _route()
    assert re.match(pat, r), r
    E.assert_exact(out[:, coff:coff + Co], ref, f"{F32_CASES[i]} {r}")
    rest = torch.cat([out[:, :coff], out[:, coff + Co:]], 1)
    assert bool((rest == 7.0).all()), "channels outside the slice were written"
    if kind == 0 and stride == 1:
        got = trunk_f32.conv2d_packed(x.float().cuda(), wp, b.float().cuda(), Co, k, k, stride, pad, pad)
        E.assert_exact(got, ref, f"conv2d_packed {F32_CASES[i]}")


@pytest.mark.parametrize("case", [(2, 64, 7, 9, 32, True), (1, 1026, 4, 5, 129, True), (1, 2, 16, 30, 2, False), (3, 33, 1, 5, 65, True)])
def test_float32_modules_equal_float64(case, monkeypatch):
    """Conv2dF32 / ConvTranspose2dF32 (k4 s2 as four phase launches) as modules, every shape through the own kernel."""
    monkeypatch.setattr(trunk_f32, "ROUTE", False)
    N, C, H, W, Co, bias = case
    rs = np.random.RandomState(C + Co)
    x = E.ints(rs, (N, C, H, W), -40, 40)
    wt = E.sparse_weights(rs, (C, Co, 4, 4), min(1.0, 500.0 / C), 30)
    b = E.ints(rs, (Co,), -100, 100) if bias else None
    m = trunk_f32.ConvTranspose2dF32(C, Co, 4, 2, 1, bias=bias)
    with torch.no_grad():
        m.weight.copy_(wt.float())
        if bias:
            m.bias.copy_(b.float())
        got = m.cuda()(x.float().cuda())
    assert _route().startswith("f32 flat<"), _route()
    E.assert_exact(got, E.deconv_ref(x, wt, b, stride=2, padding=1, store=torch.float32), f"ConvTranspose2dF32 {case}")
    wc = E.sparse_weights(rs, (Co, C, 3, 3), min(1.0, 500.0 / C), 30)
    m = trunk_f32.Conv2dF32(C, Co, 3, 2, 1, bias=bias)
    with torch.no_grad():
        m.weight.copy_(wc.float())
        if bias:
            m.bias.copy_(b.float())
        got = m.cuda()(x.float().cuda())
    assert _route().startswith("f32 "), _route()
    E.assert_exact(got, E.conv_ref(x, wc, b, stride=2, padding=1, store=torch.float32), f"Conv2dF32 {case}")


def test_fused_sequential_concat_slice_equals_float64(monkeypatch):
    """FusedSequential: Conv2d -> BatchNorm2d(eval) -> ReLU as one launch into a concat-buffer slice.  running_var = 1, eps = 0 and weight 1/2
    give the scale 2^-1 exactly; running_mean and the BatchNorm bias are integers."""
    monkeypatch.setattr(trunk_f32, "MIN_TILES", 0)
    monkeypatch.setattr(trunk_f32, "MIN_WGS", 0)
    rs = np.random.RandomState(77)
    N, C, H, W, Co = 2, 33, 13, 41, 16
    x = E.ints(rs, (N, C, H, W), -40, 40)
    w = E.sparse_weights(rs, (Co, C, 3, 3), 1.0, 30)
    b, mean, beta = E.ints(rs, (Co,), -50, 50) * 2, E.ints(rs, (Co,), -20, 20) * 2, E.ints(rs, (Co,), -9, 9)
    seq = trunk_f32.FusedSequential(trunk_f32.Conv2dF32(C, Co, 3, 1, 1), torch.nn.BatchNorm2d(Co), torch.nn.ReLU())
    bn = seq[1]
    with torch.no_grad():
        seq[0].weight.copy_(w.float())
        seq[0].bias.copy_(b.float())
        bn.running_mean.copy_(mean.float())
        bn.running_var.fill_(1.0)
        bn.eps = 0.0
        bn.weight.fill_(0.5)
        bn.bias.copy_(beta.float())
    seq = seq.cuda().eval()
    ref = torch.relu((E.conv_ref(x, w, b, padding=1, store=torch.float32) - mean.view(1, -1, 1, 1)) * 0.5 + beta.view(1, -1, 1, 1))
    E.check_storable(ref, torch.float32, "BatchNorm output")
    buf = torch.full((N, 40, H, W), 7.0, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        assert seq(x.float().cuda(), into=(buf, 8)) is None
    assert _route().startswith("f32 sp16"), _route()
    E.assert_exact(buf[:, 8:8 + Co], ref, "FusedSequential into a slice")
    assert bool((buf[:, :8] == 7.0).all()) and bool((buf[:, 8 + Co:] == 7.0).all())
