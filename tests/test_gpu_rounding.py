"""Every fp16 store is ONE round-to-nearest-even of a value the kernel's header names.

The exact-arithmetic suites choose operands whose stored values already are fp16 values, so no conversion in them ever rounds; the
Gaussian suites hold a map to 2e-3 of its range, a thousand ulps.  Here the float32 sum is still exact (the budget of tests/_exact.py:
sum |x||w| + |b| below 2^24 granules, so order, split-K, tile and MFMA shape cannot matter) but 13 to 15 bits wide: more than half of
the stored values need rounding and a fifth are exact ties.  The reference is the float64 sum, the kernel's documented float32
activation, one `_exact.round_f16` (integer arithmetic, no library cast) and, in the SR kernels, the packed-fp16 PReLU with an fp16
slope and one rounding of the product.  Every comparison is `E.assert_exact`: there is no tolerance in this file.

The cases are built in tests/_round_cases.py without a GPU; tests/test_exact_helper.py checks there that each meets
`_exact.check_rounds` and that truncation, ties away from zero, an activation on the wrong side of the rounding, a float32 slope and a
partial sum parked in fp16 each move at least 5 % of the map -- so each of those defects in a kernel fails here.

Out of scope: NaN and infinity as INPUTS; subnormal operands of the packed-fp16 PReLU; the float32 routes, which have no fp16 store;
the x3 bilinear skip, which tests/test_gpu_exact_sr_ends.py restates operation by operation."""
import re

import numpy as np
import pytest
import torch

import _exact as E
import _round_cases as R

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import igemm  # noqa: E402
from test_gpu_exact_conv import GATHER_ROUTES, PATCH_ROUTES, _route, _switches, check_nhwc, run_hconv  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- the gather kernel
@pytest.mark.xcheck
@pytest.mark.parametrize("route", list(GATHER_ROUTES))
@pytest.mark.parametrize("name", R.names("gather"))
def test_gather_routes_round_once(name, route):
    """k_conv_igemm_d (64 / 128 channels), the first build, the five-set ring and the heuristic's choice: activation in float32, one
    rounding."""
    c = R.case(name)
    modes, pat = GATHER_ROUTES[route]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    check_nhwc(got, c, f"{name} {r}")


@pytest.mark.xcheck
@pytest.mark.parametrize("name", R.names("splitk"))
def test_gather_split_k_rounds_once_and_every_fill_gives_the_same_bits(name):
    """Split-K adds float32 partial sums from a workspace: exact, so the ONE rounding behind them gives the bits of the unsplit launch."""
    c = R.case(name)
    seen = {}
    for fill in (1000, 1128, 1999):
        with _switches(2000, 11, fill):
            got, r = run_hconv(c)
        assert r.startswith("gather<"), r
        seen[r] = got.clone()
        check_nhwc(got, c, f"{name} {r}")
    assert any("splitk" not in r for r in seen) and any("splitk" in r for r in seen), sorted(seen)
    first = next(iter(seen.values()))
    assert all(torch.equal(v, first) for v in seen.values())


# ---------------------------------------------------------------------------------------------------------------- the tile kernel
@pytest.mark.xcheck
@pytest.mark.parametrize("name", R.names("tile"))
def test_tile_kernel_rounds_once(name):
    c = R.case(name)
    can128 = igemm._cout_pad(c["cout"]) % 128 == 0
    seen = {}
    for bn in (64, 128):
        for splits in (1, 3):
            with _switches(2003, 4000 + bn, 5000 + splits):
                got, r = run_hconv(c)
            assert r.startswith(f"tile<{bn if (bn == 64 or can128) else 64}>"), r
            seen[r] = got.clone()
            check_nhwc(got, c, f"{name} {r}")
    assert any("splitk" not in r for r in seen)
    if c["cin"] * c["w"].shape[-1] ** 2 >= 32 * 16:          # (at least four K steps per split: shorter contractions cannot split)
        assert any("splitk" in r for r in seen), sorted(seen)
    first = next(iter(seen.values()))
    assert all(torch.equal(v, first) for v in seen.values())


# ---------------------------------------------------------------------------------------------------------------- the LDS-patch kernels
@pytest.mark.xcheck
@pytest.mark.parametrize("route", list(PATCH_ROUTES))
@pytest.mark.parametrize("name", R.names("patch"))
def test_patch_kernels_round_once(name, route):
    c = R.case(name)
    modes, pat = PATCH_ROUTES[route]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    check_nhwc(got, c, f"{name} {r}")


# ---------------------------------------------------------------------------------------------------------------- 1x1 streaming
@pytest.mark.xcheck
@pytest.mark.parametrize("name", R.names("one"))
def test_conv1x1_streaming_and_transposing_builds_round_once(name):
    c = R.case(name)
    cin, cout = c["cin"], c["cout"]
    seen = []
    for mode in (7000, 7001):
        with _switches(mode):
            got, r = run_hconv(c)
        want_r = "conv1x1_t" if (mode == 7001 and cin == 128 and cout % 8 == 0) else f"conv1x1_stream<{igemm.pad32(cin) // 32}>"
        assert r == want_r, (r, want_r)
        check_nhwc(got, c, f"{name} {r}")
        seen.append(got.clone())
    assert torch.equal(seen[0], seen[1])


# ---------------------------------------------------------------------------------------------------------------- other fp16 layers
@pytest.mark.parametrize("name", R.names("stem"))
def test_stem_convolution_rounds_once(name):
    c = R.case(name)
    stem = igemm.HConvStem(c["w"].float().cuda(), c["b"].float().cuda(), stride=c["stride"], pad=c["pad"], act=c["act"], slope=c["slope"])
    got = stem(E.nhwc(c["x"], torch.float16, 4).cuda())
    r = _route()
    assert r.startswith("gather<") and "stem" in r, r
    check_nhwc(got, c, f"{name} {r}")


@pytest.mark.parametrize("name", R.names("pair"))
def test_pair_convolution_stride2_rounds_once(name):
    c = R.case(name)
    conv = igemm.HConvPairS2(c["w"].float().cuda(), c["b"].float().cuda(), pad=c["pad"], act=c["act"], slope=c["slope"])
    got = conv(E.nhwc(c["x"], torch.float16, 16).cuda())
    assert _route().startswith("gather<") or _route().startswith("tile<"), _route()
    check_nhwc(got, c, f"{name} {_route()}")


@pytest.mark.xcheck
@pytest.mark.parametrize("name", R.names("deconv"))
def test_transposed_convolution_k4s2_rounds_once(name):
    """HDeconv4s2 through the heuristic's route, the gather kernel and (wide layers) the tile kernel: the same bits."""
    c = R.case(name)
    cin, cout = c["cin"], c["cout"]
    dc = igemm.HDeconv4s2(c["w"].float().cuda(), c["b"].float().cuda(), act=c["act"], slope=c["slope"])
    xs = E.nhwc(c["x"], torch.float16, igemm.pad32(cin)).cuda()
    seen = []
    for modes, pat in (((), r"deconv4s2"), ((1,), r"deconv4s2 gather<"), ((2003,), r"deconv4s2 tile<" if cout > 32 else r"deconv4s2")):
        with _switches(*modes):
            got = dc(xs)
            torch.cuda.synchronize()
            r = _route()
        assert re.match(pat, r), r
        check_nhwc(got, c, f"{name} {r}")
        seen.append(got.clone())
    assert all(torch.equal(v, seen[0]) for v in seen)


@pytest.mark.parametrize("i", range(len(R.FLOW_HEAD)))
def test_flow_head_rounds_the_flow_then_the_upsampling_of_the_rounded_flow(i):
    """HFlowHead, the form with the fused ConvTranspose2d(2, 2, 4, 2, 1) and the form without: the flow rounds once; the transposed
    convolution reads the fp16 flow and its sum rounds once more."""
    c = R.flow_head_case(i)
    cin, (N, _, H, W) = c["cin"], c["x"].shape
    cp = igemm.pad32(cin)
    xs = E.nhwc(c["x"], torch.float16, cp).cuda()
    head = igemm.HFlowHead(c["w"].float().cuda(), c["b"].float().cuda(), c["wu"].float().cuda(), c["bu"].float().cuda())
    up_out = torch.full((N, 2 * H, 2 * W, 32), 3.0, dtype=torch.float16, device="cuda")
    flow = head(xs, up_out=up_out, up_coff=6)
    r = _route()
    assert re.match(r"flow_head<(4,4|8,8),2>", r), r
    check_nhwc(flow, c, f"flow head {i} {r}")
    E.assert_exact(E.nchw64(up_out[..., 6:8]), c["up"], f"flow upsampling {i} {r}")
    assert bool((up_out[..., :6] == 3.0).all()) and bool((up_out[..., 8:] == 3.0).all())
    plain = igemm.HFlowHead(c["w"].float().cuda(), c["b"].float().cuda())
    flow1 = plain(xs)
    r1 = _route()
    assert re.match(r"flow_head<(4,4|8,8),1>", r1), r1
    check_nhwc(flow1, c, f"flow head {i} {r1}")


@pytest.mark.parametrize("i", range(len(R.HG_FRONT)))
def test_hourglass_front_rounds_the_stem_and_reads_the_rounded_stem(i):
    """HHourglassFront: the stem rounds after ReLU; the 2x2 max pool and the 1x1 + ReLU read the ROUNDED stem, and the 1x1 rounds again."""
    c = R.hg_front_case(i)
    s = c["stem"]
    N, _, H, W = s["x"].shape
    c2 = c["one"].shape[1]
    front = igemm.HHourglassFront(igemm.HConvStem(s["w"].float().cuda(), s["b"].float().cuda(), stride=1, pad=3, act=R.RELU),
                                  igemm.HConv(c["w1"].float().cuda(), c["b1"].float().cuda(), act=R.RELU))
    out2 = torch.full((N, H, W, igemm.pad32(c2) + 32), 3.0, dtype=torch.float16, device="cuda")
    pooled = torch.full((N, H // 2, W // 2, 128), 3.0, dtype=torch.float16, device="cuda")
    stem_out = torch.full((N, H, W, 160), 3.0, dtype=torch.float16, device="cuda")
    front(E.nhwc(s["x"], torch.float16, 4).cuda(), out2, pooled=pooled, stem_out=stem_out)
    assert _route() == "hg_front"
    E.assert_exact(E.nchw64(stem_out, 128), s["want"], "hourglass stem")
    E.assert_exact(E.nchw64(pooled), c["pool"], "hourglass pooled stem")
    E.assert_exact(E.nchw64(out2, c2), c["one"], "hourglass 1x1")
    assert bool((stem_out[..., 128:] == 3.0).all()) and bool((out2[..., c2:] == 3.0).all())


@pytest.mark.parametrize("shape", [(2, 9, 7, 16), (3, 5, 33, 40)])
def test_average_pool_rounds_once(shape):
    """pool2x2 average on arbitrary fp16 values: the float32 sum of four fp16 values is exact, times 0.25, one rounding."""
    x16, want = R.avg_pool_case(shape)
    N, H, W, C = shape
    got = igemm.pool2x2(x16.cuda(), 8, C, 1)
    E.assert_exact(E.nchw64(got), want, f"pool2x2 average {shape}")


# ---------------------------------------------------------------------------------------------------------------- overflow, underflow
EDGE_ROUTES = {
    "gather": ((2000,), r"gather<"), "tile": ((2003, 4064, 5001), r"tile<64>"), "patch_r8": ((2, 2000, 6000, 9000), r"patch_r8<"),
    "conv1x1_stream": ((7000,), r"conv1x1_stream<"), "splitk": ((2000, 11, 1999), r"gather<.*splitk"),
}


@pytest.mark.xcheck
@pytest.mark.parametrize("family", list(EDGE_ROUTES))
def test_overflow_gives_infinity_from_65520_and_65504_below(family):
    """IEEE: a magnitude of 65520 or more stores +-inf (no clamp); strictly between 65504 and 65520 it stores +-65504."""
    c = R.overflow_case(family)
    assert c["n_inf"] >= 8 and c["n_max"] >= 8
    modes, pat = EDGE_ROUTES[family]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    check_nhwc(got, c, f"overflow {family} {r}")


@pytest.mark.xcheck
@pytest.mark.parametrize("family", list(EDGE_ROUTES))
def test_underflow_is_gradual(family):
    """Sums scaled by 2^-28 land in fp16's subnormal range: spacing 2^-24, nearest-even, nothing flushed to zero."""
    c = R.underflow_case(family)
    modes, pat = EDGE_ROUTES[family]
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    check_nhwc(got, c, f"underflow {family} {r}")


# ---------------------------------------------------------------------------------------------------------------- float32 weights
@pytest.mark.xcheck
@pytest.mark.parametrize("family", ["gather", "tile"])
def test_packer_rounds_float32_weights_to_nearest_even(family):
    """igemm.HConv gets float32 weights of 12 to 13 significant bits, ties among them: the packer's conversion is `round_f16(w)`."""
    shape, modes, pat = {"gather": ((1, 33, 6, 11, 17, 3, 1, 1), (2000, 11), r"gather<"), "tile": ((1, 33, 11, 12, 65, 3, 1, 1), (2003,), r"tile<")}[family]
    c = R.w32_case(family, shape)
    with _switches(*modes):
        got, r = run_hconv(c)
    assert re.match(pat, r), r
    check_nhwc(got, c, f"float32 weights {family} {r}")


# ---------------------------------------------------------------------------------------------------------------- the SR net: stages
from test_gpu_exact_sr import _in, _new, _run_default, module  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402


def _eq(got, want, what):
    E.assert_exact(E.nchw64(got), want, what)


def _rps_set(h):
    return sorted({h, 1, -3}, key=lambda v: (v < 0, -v))


@pytest.mark.xcheck
@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[4])
def test_x4_stage_rounds_at_every_storage_point(shape, select):
    """k_utd4 through the wrapper and at row segmentations h / 1 / -3, k_utd3<POST>, k_utd3 and k_utd2: the deconvolution, the downtran
    1x1, the strided convolution and the POST 1x1 each round once, each PReLU multiplies fp16 by an fp16 slope and rounds once.
    `select`: a slope of 1.5 (the select builds)."""
    N, h, w = shape
    lib = L.load()
    for post in (False, True):
        c, ref = R.gen_round_stage(4, shape, select=select, post=post)
        m = module(4, c)
        P = m._packed()
        le1 = int(P["slopes_le_one"])
        assert le1 == (0 if select else 1)
        a = _in(c)
        what = f"x4 {shape} select {select} post {post}"
        _eq(m._utd4(a, P["utd4"][0], N, h, w), ref["out"], what + " k_utd4 (wrapper)")
        if post:
            out, p2 = m._utd4(a, P["utd4"][0], N, h, w, post=True)
            _eq(out, ref["out"], what + " k_utd4 (wrapper, POST)")
            _eq(p2, ref["post"], what + " k_utd4 post (wrapper)")
            out, p2 = m._utd_post(a, P["utd_post"][0], N, h, w)
            _eq(out, ref["out"], what + " k_utd3<POST> (wrapper)")
            _eq(p2, ref["post"], what + " k_utd3<POST> post (wrapper)")
        else:
            _eq(m._utd(a, P["utd"][0], N, h, w), ref["out"], what + " k_utd3 (wrapper)")
            _eq(m._utd2(a, P["utd2"][0], N, h, w), ref["out"], what + " k_utd2 (wrapper)")
            try:
                lib.vsr_sr_utd_variant(1)
                out = _new(a)
                L.check(lib.vsr_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(P["utd"][0], torch.uint8), L.dptr(out, torch.float16), N, h, w, h, 0, le1, L.stream()))
                _eq(out, ref["out"], what + " k_utd")
            finally:
                lib.vsr_sr_utd_variant(0)
        if select:
            continue
        for rps in _rps_set(h):
            out, p2 = _new(a), _new(a)
            L.check(lib.vsr_sr_utd4_f16(L.dptr(a, torch.float16), L.dptr(P["utd4"][0], torch.uint8), L.dptr(out, torch.float16), L.dptr(p2, torch.float16),
                                        N, h, w, rps, 1, L.stream()), "sr_utd4_f16")
            _eq(out, ref["out"], f"{what} k_utd4 rps {rps}")
            if post:
                _eq(p2, ref["post"], f"{what} k_utd4 post rps {rps}")
                out, p2 = _new(a), _new(a)
                L.check(lib.vsr_sr_utd_post_f16(L.dptr(a, torch.float16), L.dptr(P["utd_post"][0], torch.uint8), L.dptr(out, torch.float16), L.dptr(p2, torch.float16),
                                                N, h, w, rps, 1, L.stream()), "sr_utd_post_f16")
                _eq(out, ref["out"], f"{what} k_utd3<POST> rps {rps}")
                _eq(p2, ref["post"], f"{what} k_utd3<POST> post rps {rps}")


@pytest.mark.xcheck
@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[2])
def test_x2_stage_rounds_at_every_storage_point(shape, select):
    """vsr_sr_utd_s2_f16 (both variants), vsr_sr_utd_s2_post_f16 through the wrapper, vsr_sr_utd_s2w_f16."""
    N, h, w = shape
    lib = L.load()
    for post in (False, True):
        c, ref = R.gen_round_stage(2, shape, select=select, post=post)
        a = _in(c)
        what = f"x2 {shape} select {select} post {post}"
        m = module(2, c, utd_s2_build=1)
        st = m._packed()["stage"][0]
        assert type(st).__name__ == "_FusedStageS2" and not st.wide and st.has_post
        _eq(st(a, m._chain), ref["out"], what + " k_utd_s2 (wrapper)")
        if post:
            out, p2 = st(a, m._chain, post=True)
            _eq(out, ref["out"], what + " k_utd_s2<POST>")
            _eq(p2, ref["post"], what + " k_utd_s2<POST> post")
        mw = module(2, c, utd_s2_build=2)
        sw = mw._packed()["stage"][0]
        assert sw.wide
        _eq(sw(a, mw._chain), ref["out"], what + " k_utd_s2w (wrapper)")
        if select:
            continue
        try:
            for variant in (0, 1):
                lib.vsr_sr_utd_s2_variant(variant)
                for rps in (h, 1):
                    out = _new(a)
                    L.check(lib.vsr_sr_utd_s2_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 1, L.stream()))
                    _eq(out, ref["out"], f"{what} k_utd_s2 variant {variant} rps {rps}")
        finally:
            lib.vsr_sr_utd_s2_variant(0)
        for rps in (h, 1):
            out = _new(a)
            L.check(lib.vsr_sr_utd_s2w_f16(L.dptr(a, torch.float16), L.dptr(sw.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 1, L.stream()))
            _eq(out, ref["out"], f"{what} k_utd_s2w rps {rps}")


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[3])
def test_x3_stage_and_its_post_build_round_at_every_storage_point(shape, select):
    """k_utd_s3 (wrapper, whole march, 3-row and one-row segments) and the POST build vsr_s3p_sr_utd_post_f16 with both outputs."""
    from test_gpu_utd_s3_post import _launch_post, _stage_post
    N, h, w = shape
    for post in (False, True):
        c, ref = R.gen_round_stage(3, shape, select=select, post=post)
        a = _in(c)
        what = f"x3 {shape} select {select} post {post}"
        m = module(3, c)
        st = m._packed()["stage"][0]
        assert type(st).__name__ == "_FusedStageS3"
        _eq(st(a, m._chain), ref["out"], what + " k_utd_s3 (wrapper)")
        lib = L.load_s3()
        for rps in (0, 3, 1):
            out = _new(a)
            L.check(lib.vsr_s3_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, int(st.slopes_le_one), L.stream()),
                    "sr_utd_s3_f16", lib=lib)
            _eq(out, ref["out"], f"{what} k_utd_s3 rps {rps}")
        if post:
            sp = _stage_post(m)
            out, p2 = sp(a, m._chain)
            _eq(out, ref["out"], what + " POST build out (wrapper)")
            _eq(p2, ref["post"], what + " POST build post (wrapper)")
            for rps in (0, 1):
                out, p2 = _launch_post(sp, a, rps, 0 if select else 1)
                _eq(out, ref["out"], f"{what} POST build out rps {rps}")
                _eq(p2, ref["post"], f"{what} POST build post rps {rps}")


@pytest.mark.parametrize("S", [4, 2, 3])
def test_stage_packer_rounds_float32_weights_to_nearest_even(S):
    """sr_pack gets deconvolution weights that are no fp16 values (12 to 13 significant bits, ties among them)."""
    shape = R.SR_SHAPES[S][2]
    c, ref = R.gen_round_stage_w32(S, shape)
    _eq(_run_default(S, module(S, c), _in(c), shape), ref["out"], f"x{S} float32 weights")


# ---------------------------------------------------------------------------------------------------------------- the SR net: tails, head, chain
from test_gpu_exact_sr_ends import (CHAIN_SPECS, _cmap_nhwc, _head, _nchw1, _raw, _tail3, _tail3_fold, chain_dev, head_module, tail_module)  # noqa: E402
from video_super_resolution_amd import SRProjectionModule  # noqa: E402


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[4])
def test_x4_tail_and_its_fold_build_round_once(shape, last):
    """k_tail3 / k_tail3<DEC> and the FOLD builds: the deconvolution sum rounds, the fp16 PReLU (slope 0.625, or 0.2 with `last`) rounds
    its product, conv_out reads the rounded map in float32; with FOLD the compress_out sum rounds in front of it."""
    N, h, w = shape
    for fold in (False, True):
        c, ref = R.gen_round_tail(4, shape, fold=fold, last=last)
        m = tail_module(c)
        P = m._packed()
        le1 = int(P["slopes_le_one"])
        assert le1 == 1
        what = f"x4 tail {shape} fold {fold} last {last}"
        hid = E.nhwc(c["hid"]).cuda()
        for dec in (False, True):
            want = ref["dec" if dec else "raw"]
            for rps in sorted({h, 1}, reverse=True):
                E.assert_exact(_tail3(P, hid, shape, rps, le1, dec), want, f"{what} k_tail3 dec {dec} rps {rps}")
                if fold:
                    a, b, cm = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"])
                    E.assert_exact(_tail3_fold(P, a, b, cm, shape, rps, le1, dec), want, f"{what} k_tail3<FOLD> dec {dec} rps {rps}")


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[2])
def test_x2_tail_and_its_fold_build_round_once(shape, last):
    N, h, w = shape
    c, ref = R.gen_round_tail(2, shape, fold=True, last=last)
    m = tail_module(c)
    P = m._packed()
    assert P["tail_s2_fold"]
    a, b, cm, hid = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"]), E.nhwc(c["hid"]).cuda()
    lib, le1 = L.load(), int(P["slopes_le_one"])
    what = f"x2 tail {shape} last {last}"
    for dec in (False, True):
        want = ref["dec" if dec else "raw"]
        ho, wo = (h, w) if dec else (2 * h, 2 * w)
        raw = _raw(N, ho, wo)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, want, f"{what} _tail_raw dec {dec}")
        raw = _raw(N, ho, wo)
        m._tail_raw(a, P, dec, raw, fold=(a, b, cm))
        E.assert_exact(raw, want, f"{what} _tail_raw fold dec {dec}")
        for rps in sorted({h, 1}, reverse=True):
            raw = _raw(N, ho, wo)
            L.check(lib.vsr_sr_tail_s2_f16(L.dptr(hid, torch.float16), L.dptr(P["tail_s2"], torch.uint8), L.dptr(raw), N, h, w, rps, le1, int(dec), L.stream()), "sr_tail_s2_f16")
            E.assert_exact(raw, want, f"{what} k_tail_s2 dec {dec} rps {rps}")
            raw = _raw(N, ho, wo)
            L.check(lib.vsr_sr_tail_s2_fold_f16(L.dptr(a, torch.float16), L.dptr(b, torch.float16), L.dptr(cm), L.dptr(P["tail_s2"], torch.uint8), L.dptr(raw),
                                                N, h, w, rps, le1, int(dec), L.stream()), "sr_tail_s2_fold_f16")
            E.assert_exact(raw, want, f"{what} k_tail_s2<FOLD> dec {dec} rps {rps}")


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("shape", R.SR_SHAPES[3])
def test_x3_tail_rounds_once(shape, last):
    """The x3 tail through `_tail_raw`, full and decimated (the x3 geometry has no folded build)."""
    N, h, w = shape
    c, ref = R.gen_round_tail(3, shape, last=last)
    m = tail_module(c)
    P = m._packed()
    hid = E.nhwc(c["hid"]).cuda()
    for dec in (False, True):
        raw = _raw(N, h if dec else 3 * h, w if dec else 3 * w)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, ref["dec" if dec else "raw"], f"x3 tail {shape} last {last} dec {dec}")


@pytest.mark.parametrize("slopes", [(0.75, 0.2), (1.5, 0.1)])
@pytest.mark.parametrize("shape", [(3, 2, 2), (8, 9, 40), (2, 37, 33)])
def test_head_rounds_both_sums(shape, slopes):
    """k_head_h: conv_in and feat_in each round once before their packed-fp16 PReLU."""
    c, ref = R.gen_round_head(shape, slopes=slopes)
    P = head_module(c)._packed()
    E.assert_exact(_head(P, c["x"].float().cuda(), shape), ref["out"], f"head {shape} slopes {slopes}")


@pytest.mark.xcheck
@pytest.mark.parametrize("N,P", [(2, 65), (3, 1000)])
@pytest.mark.parametrize("name", ["2-p", "2m-1p-p", "1m-1p-p", "1-2p-1pm"])
def test_chain_rounds_every_stage(name, N, P):
    """k_chain1x1_h with two and three stages, streaming builds and the generic kernel (vsr_sr_chain_variant 1)."""
    stages, outs, _ = R.gen_round_chain(CHAIN_SPECS[name], N, P)
    dev = chain_dev(stages, P)
    lib = L.load()
    try:
        for variant in (0, 1):
            lib.vsr_sr_chain_variant(variant)
            got = SRProjectionModule._chain(dev, N, P, keep=[True] * len(stages))
            for s in range(len(stages)):
                E.assert_exact(_nchw1(got[s]), outs[s], f"chain {name} N {N} P {P} variant {variant} stage {s}", names="ncp")
    finally:
        lib.vsr_sr_chain_variant(0)


@pytest.mark.parametrize("slope", [0.2, 1.5])
@pytest.mark.parametrize("nin,cm", [(1, False), (3, True)])
@pytest.mark.parametrize("N,P", [(2, 65), (3, 1000)])
def test_conv1x1_f16_rounds_once(N, P, nin, cm, slope):
    """vsr_sr_conv1x1_f16 (SRProjectionModule._c1h): one stage over one and three inputs; the max form and the min form of the PReLU."""
    from test_gpu_exact_sr_ends import _nhwc1, _wide
    stages, outs, _ = R.gen_round_chain([(nin, False, cm)], N, P, slopes=(slope,))
    rs = np.random.RandomState(P)
    st = stages[0]
    ins = [(_nhwc1(x), _wide(rs, wm, 128, 32 * (t + 1)), 32 * (t + 1)) for t, (x, wm) in enumerate(st["ins"])]
    cmap = st["cmap"].t().contiguous().float().cuda() if cm else None
    got = SRProjectionModule._c1h(ins, st["bias"].float().cuda(), slope, N, P, cmap=cmap)
    E.assert_exact(_nchw1(got), outs[0], f"_c1h N {N} P {P} inputs {nin} map {cm} slope {slope}", names="ncp")


# ---------------------------------------------------------------------------------------------------------------- the hourglass inception block
import _hgi_cases as C  # noqa: E402


@pytest.mark.parametrize("hw", C.ROUND_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(C.SIGS))
def test_inception_block_rounds_its_mid_maps_and_its_outputs_once(name, hw):
    """The one-launch block and the four-launch path: each mid map is the one rounding of its 1x1 sum behind ReLU, each k x k reads the
    ROUNDED mid map and rounds once more -- the same bits on both paths."""
    from test_gpu_hg_inception import _block, _run, _wide
    wts = C.round_weights(name)
    inc = _block(wts)
    x = C.round_input(name, hw)
    ref, _ = C.round_ref(wts, x)
    for n, in_coff in ((1, 0), (C.NREF, 32)):
        got, _ = _run(inc, _wide(x[:n], in_coff, 1000.0), in_coff, fused=True)
        E.assert_exact(got, ref[:n], f"block {name} {hw[0]}x{hw[1]} N={n} in_coff={in_coff} (fused)")
    four, _ = _run(inc, _wide(x, 32, 1000.0), 32, fused=False)
    E.assert_exact(four, ref, f"block {name} {hw[0]}x{hw[1]} (four launches)")


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("shape", R.PRE_SHAPES)
def test_x3_stage_behind_the_folded_chain_rounds_at_every_storage_point(shape, mode):
    """vsr_s3f_sr_utd_pre_f16: the chain (exact regime) feeds the stage from its LR load path; the stage's four storage points round."""
    from test_gpu_utd_s3_pre import _exact_ops, _launch_pre, _module, _stage_pre
    c, ref = R.gen_round_pre(shape, mode)
    m = _module(c, R.PRE_CHAIN_SLOPES, ss=(c["up_a"], c["dt_a"], c["dn_a"]), ps=c["post_a"])
    sp = _stage_pre(m)
    ops = _exact_ops(c, shape)
    what = f"x3 PRE{mode} {shape}"
    f, a, b, cmap = ops if mode == 3 else (ops[0], None, None, None)
    out, post = sp(f, a, b, cmap)
    _eq(out, ref["out"], what + " out (wrapper)")
    _eq(post, ref["post"], what + " post (wrapper)")
    _eq(sp(f, a, b, cmap, post=False), ref["out"], what + " out (wrapper, no POST)")
    for rps in (0, 1):
        out, post = _launch_pre(sp, ops, mode, rps, 0)
        _eq(out, ref["out"], f"{what} out rps {rps}")
        _eq(post, ref["post"], f"{what} post rps {rps}")
