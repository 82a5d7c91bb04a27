"""The two ENDS of the SR net in EXACT arithmetic: the head (k_head_h and the float32 head), the 1x1 chain kernel with its own operands,
the tails of every scale (k_tail3 with DEC and FOLD, the LDS-ring k_tail, k_tail_s2 with and without the folded compress_out, the x3
pair _PhaseDeconv + k_convout_planes), the skip + add_mean + fusion MLP kernels and the uint8 conversions either side of the path equal a
float64 CPU evaluation bit for bit, on operands inside the budget tests/_exact.py checks.  tests/test_gpu_exact_sr.py holds the
FeedbackBlock stages between these ends.

As there, weights are set on a deep copy of a seeded SRProjectionModule whose `_packed()` runs the real packers (`pack_utd_blob` with and
without `fold_co`, `pack_conv_out_frags3`, `pack_conv_out_frags`, `pack_tail_s2_blob`, `_PhaseDeconv`, `tail_par`): packer and kernel
are held together against an independent evaluation, not against a sibling build that reads the same fragments.

The tail's raw planes are float32, so conv_out has the whole 2^24 budget and BOTH of its layers can be dense at once (profile "dense");
two more profiles make one layer sparse with wider values.  MeanShift values are dyadic (mean (0.5, 0.25, 0.375), std 1), so the x2 / x4
bilinear skip (weights k/4, k/8) and the MLP are exact in any order.  The x3 skip has weights of thirds: there the kernel's float32
arithmetic (csrc/sr_scale.hip `bil`, `lerp4`, explicit fused multiply-adds, contraction off) is restated operation by operation, each
fused multiply-add rounded once, and equality is required all the same.

A sensitivity case per family moves ONE weight by one unit on the GPU side and asserts that the comparison fails on exactly the predicted
footprint.  Every case passes `E.check_live` inside its reference (both signs before every PReLU, enough distinct values)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import SRProjectionModule  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

_master = {}
MEAN = (0.5, 0.25, 0.375)            # 255 * mean = 127.5, 63.75, 95.625: multiples of 1/8
TAIL_PROFILES = ("dense", "out", "cv")


def _t(v):
    return torch.tensor(v, dtype=torch.float64)


def mean_shifts(mean=MEAN):
    """(sub, add) as (scale [3], bias [3]) float64 pairs: MeanShift of std 1."""
    return (_t((1.0, 1.0, 1.0)), -255.0 * _t(mean)), (_t((1.0, 1.0, 1.0)), 255.0 * _t(mean))


# ---------------------------------------------------------------------------------------------------------------- cases
def gen_tail(seed, S, shape, slope=0.5, profile="dense", fold=False, co_slope=0.5, live=True):
    """Exact operands of the tail (+ of the folded compress_out) and their float64 reference."""
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(seed)
    c = dict(S=S, out_a=slope)
    if fold:
        c.update(lr_a=E.ints(rs, (N, 32, h, w), -2, 2), lr_b=E.ints(rs, (N, 32, h, w), -2, 2), co_w=E.sparse_weights(rs, (32, 64), 0.08, 1),
                 co_b=E.ints(rs, (32,), -1, 1), co_a=co_slope, cmap=E.ints(rs, (32, h, w), -2, 2))
        c["hid"] = E.fold_ref(c["lr_a"], c["lr_b"], c["cmap"], c["co_w"], c["co_b"], c["co_a"], live=live)
    else:
        c["hid"] = E.ints(rs, (N, 32, h, w), -2, 2)
    d_out, hi_out, d_cv, hi_cv = {"dense": (1.0, 1, 1.0, 8), "out": (1.0, 1, 0.08, 4), "cv": (0.06, 2, 1.0, 12)}[profile]
    c.update(out_w=E.sparse_weights(rs, (32, 32, k, k), d_out, hi_out), out_b=E.ints(rs, (32,), -3, 3),
             cv_w=E.sparse_weights(rs, (3, 32, 3, 3), d_cv, hi_cv, step=0.25), cv_b=E.ints(rs, (3,), -200, 200, step=0.5))
    ref = E.tail_ref(c["hid"], c["out_w"], c["out_b"], c["out_a"], c["cv_w"], c["cv_b"], S, live=live)
    return c, ref


def _seeded(S):
    if S not in _master:
        _master[S] = fill_module_(SRProjectionModule(upscale_factor=S).eval(), seed=0, prefix="model.")
    return copy.deepcopy(_master[S]).eval()


def _set_mean_shift(m, sub, add):
    with torch.no_grad():
        for ms, (s, b) in ((m.sub_mean, sub), (m.add_mean, add)):
            ms.weight.copy_(torch.diag(s).view(3, 3, 1, 1))
            ms.bias.copy_(b)


def tail_module(c, **attrs):
    """The seeded module of the case's scale with the case's tail (and compress_out slices of lr3 / lr6) and dyadic MeanShifts, on the GPU."""
    m = _seeded(c["S"])
    with torch.no_grad():
        m.out[0].weight.copy_(c["out_w"])
        m.out[0].bias.copy_(c["out_b"])
        m.out[1].weight.fill_(c["out_a"])
        m.conv_out[0].weight.copy_(c["cv_w"])
        m.conv_out[0].bias.copy_(c["cv_b"])
        if "co_w" in c:
            co = m.block.compress_out
            assert co[0].weight.shape[1] == 192        # six groups: lr3 reads columns 64..95, lr6 columns 160..191
            co[0].weight[:, 64:96, 0, 0] = c["co_w"][:, :32].float()
            co[0].weight[:, 160:192, 0, 0] = c["co_w"][:, 32:].float()
            co[0].bias.copy_(c["co_b"])
            co[1].weight.fill_(c["co_a"])
    _set_mean_shift(m, *mean_shifts())
    m = m.cuda()
    m.precision = "fp16"
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _raw(N, ho, wo):
    return torch.full((N, 3, ho, wo), float("nan"), dtype=torch.float32, device="cuda")


def _cmap_nhwc(cmap):
    return cmap.permute(1, 2, 0).reshape(-1, 32).float().contiguous().cuda()


def _segs(m, N, h, w):
    return sorted({h, min(h, 5), 1, int(m._rows_per_segment(N, h, w))}, reverse=True)


def _tail3(P, hid, shape, rps, le1, dec, S=4):
    N, h, w = shape
    raw = _raw(N, h if dec else S * h, w if dec else S * w)
    L.check(L.load().vsr_sr_tail3_f16(L.dptr(hid, torch.float16), L.dptr(P["utd_out"], torch.uint8), L.dptr(P["cv_frags3"], torch.float16),
                                      L.dptr(P["tail_par"]), L.dptr(raw), N, h, w, rps, le1, int(dec), L.stream()), "sr_tail3_f16")
    return raw


def _tail3_fold(P, a, b, cm, shape, rps, le1, dec):
    N, h, w = shape
    raw = _raw(N, h if dec else 4 * h, w if dec else 4 * w)
    L.check(L.load().vsr_sr_tail3_fold_f16(L.dptr(a, torch.float16), L.dptr(b, torch.float16), L.dptr(cm), L.dptr(P["utd_out_fold"], torch.uint8),
                                           L.dptr(P["cv_frags3"], torch.float16), L.dptr(P["tail_par"]), L.dptr(raw), N, h, w, rps, le1, int(dec),
                                           L.stream()), "sr_tail3_fold_f16")
    return raw


SHAPES4 = [(1, 1, 31), (1, 2, 2), (2, 37, 45), (8, 12, 32), (2, 47, 3), (3, 5, 7), (1, 9, 65), (1, 1, 1)]


# ---------------------------------------------------------------------------------------------------------------- x4 tail
@pytest.mark.parametrize("profile", TAIL_PROFILES)
@pytest.mark.parametrize("shape", SHAPES4)
def test_x4_tail_equals_float64(shape, profile):
    """vsr_sr_tail3_f16 (k_tail3 and k_tail3<DEC>), both activation builds, over the whole march, several row segments and one-row
    segments: raw planes = conv_out(PReLU(out deconvolution)) + bias, bit for bit."""
    N, h, w = shape
    slope = E.SLOPES_LE_ONE[(N + h + w) % 4]
    c, ref = gen_tail(N * 1000 + h * 10 + w, 4, shape, slope=slope, profile=profile)
    m = tail_module(c)
    P = m._packed()
    assert P["slopes_le_one"]
    hid = E.nhwc(c["hid"]).cuda()
    for dec in (False, True):
        for rps in _segs(m, N, h, w):
            for le1 in (1, 0):       # (slopes in [0, 1]: the select build computes the same)
                E.assert_exact(_tail3(P, hid, shape, rps, le1, dec), ref["dec" if dec else "raw"],
                               f"x4 tail {shape} {profile} slope {slope} k_tail3{'<DEC>' if dec else ''} rps {rps} le1 {le1}")


@pytest.mark.parametrize("slope", E.SLOPES_SELECT + (1.0, 0.0, 0.25))
def test_x4_tail_select_build_and_slope_corners(slope):
    """A slope of 2.0 and one of -0.5 (k_tail3<ALLMAX = false>; slopes_le_one as the module derives it) and the corners of the max build."""
    shape = (2, 9, 33)
    c, ref = gen_tail(int(slope * 8) + 77, 4, shape, slope=slope, profile="dense")
    m = tail_module(c)
    P = m._packed()
    assert bool(P["slopes_le_one"]) == (slope <= 1.0)
    hid = E.nhwc(c["hid"]).cuda()
    for dec in (False, True):
        for rps in (9, 4):
            E.assert_exact(_tail3(P, hid, shape, rps, int(P["slopes_le_one"]), dec), ref["dec" if dec else "raw"], f"x4 tail slope {slope} dec {dec} rps {rps}")


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", [(1, 1, 31), (1, 2, 2), (2, 37, 45), (3, 5, 7), (1, 9, 65)])
def test_x4_ring_tail_of_the_cross_check_library_equals_float64(shape):
    """k_tail (LDS ring, `pack_conv_out_frags`; vsr_sr_tail_f16 / vsr_sr_tail_dec_f16) applies skip + add_mean itself: its planes equal
    `planes_ref` of the raw reference, and the plain fusion MLP vsr_sr_fc_planes_f32 behind it equals `mlp_ref` (N = 8)."""
    N, h, w = shape
    c, ref = gen_tail(N * 1000 + h * 10 + w + 5, 4, shape, slope=0.25, profile="dense")
    m = tail_module(c)
    P = m._packed()
    sub, add = mean_shifts()
    rs = np.random.RandomState(h * 10 + w)
    x = E.ints(rs, (N, 3, h, w), 0, 255)
    hid, xg, lib = E.nhwc(c["hid"]).cuda(), x.float().cuda(), L.load_xcheck()
    for dec in (False, True):
        want = E.planes_ref(ref["dec" if dec else "raw"], x, sub, add, 4, decimate=dec)
        for rps in (h, min(h, 5), 1):
            got = _raw(N, h if dec else 4 * h, w if dec else 4 * w)
            fn = lib.vsr_sr_tail_dec_f16 if dec else lib.vsr_sr_tail_f16
            L.check(fn(L.dptr(hid, torch.float16), L.dptr(P["utd_out"], torch.uint8), L.dptr(P["cv_frags"], torch.float16), L.dptr(P["tail_par"]),
                       L.dptr(xg), L.dptr(got), N, h, w, rps, int(P["slopes_le_one"]), L.stream()), "sr_tail_f16")
            E.assert_exact(got, want, f"x4 ring tail {shape} dec {dec} rps {rps}")


@pytest.mark.parametrize("co_slope", [0.5, 2.0])
@pytest.mark.parametrize("shape", [(1, 1, 31), (1, 2, 2), (2, 37, 45), (8, 12, 32), (3, 5, 7), (1, 9, 65)])
def test_x4_folded_tail_and_the_unfolded_pair_equal_float64(shape, co_slope):
    """vsr_sr_tail3_fold_f16 (compress_out inside k_tail3's LR load path, `pack_utd_blob(fold_co=...)`) against fold_ref -> tail_ref, and
    the unfolded pair (`_chain`: one stage, two inputs + constant map, then vsr_sr_tail3_f16) against the same reference: in exact
    arithmetic the permuted K order cannot matter, so both are EQUAL to it."""
    N, h, w = shape
    c, ref = gen_tail(N * 1000 + h * 10 + w + 9, 4, shape, slope=0.5, profile="dense", fold=True, co_slope=co_slope)
    m = tail_module(c)
    P = m._packed()
    assert "utd_out_fold" in P
    a, b, cm = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"])
    hp = h * w
    hid = m._chain([dict(ins=[(a.view(N, hp, 32), P["co_w"], 64), (b.view(N, hp, 32), P["co_w"], 160)], bias=P["co_b"], slope=P["co_a"], cmap=cm)],
                   N, hp, keep=[True])[0]
    E.assert_exact(E.nchw64(hid.view(N, h, w, 32)), c["hid"], f"x4 {shape} compress_out on the chain kernel")
    for dec in (False, True):
        want = ref["dec" if dec else "raw"]
        for rps in _segs(m, N, h, w):
            E.assert_exact(_tail3_fold(P, a, b, cm, shape, rps, int(P["slopes_le_one"]), dec), want, f"x4 folded tail {shape} co slope {co_slope} dec {dec} rps {rps}")
        E.assert_exact(_tail3(P, hid.view(N, h, w, 32), shape, h, int(P["slopes_le_one"]), dec), want, f"x4 unfolded pair {shape} dec {dec}")


# ---------------------------------------------------------------------------------------------------------------- x2 tail
SHAPES2 = [(1, 1, 31), (1, 2, 2), (2, 9, 7), (8, 12, 30), (2, 33, 2), (2, 37, 95), (1, 1, 1)]


@pytest.mark.parametrize("profile", TAIL_PROFILES)
@pytest.mark.parametrize("shape", SHAPES2)
def test_x2_tail_equals_float64(shape, profile):
    """vsr_sr_tail_s2_f16 and vsr_sr_tail_s2_fold_f16 (k_tail_s2 / <FOLD>), through `_tail_raw` (strips of 30 columns, its own
    segmentation) and the ABI (whole march, several segments, one-row segments), full and decimated; `pack_tail_s2_blob` with and
    without `fold_co`."""
    from video_super_resolution_amd.sr import pack_tail_s2_blob
    N, h, w = shape
    slope = E.SLOPES_LE_ONE[(N + h + w + 1) % 4]
    c, ref = gen_tail(N * 1000 + h * 10 + w + 2, 2, shape, slope=slope, profile=profile, fold=True, co_slope=0.5)
    m = tail_module(c)
    P = m._packed()
    assert P["tail_s2_fold"] and "tail_s2" in P
    plain = pack_tail_s2_blob(m.out[0].weight, m.out[0].bias, P["out_a"], m.conv_out[0].weight, m.conv_out[0].bias)
    a, b, cm, hid = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"]), E.nhwc(c["hid"]).cuda()
    lib, le1 = L.load(), int(P["slopes_le_one"])
    what = f"x2 tail {shape} {profile} slope {slope}"
    for dec in (False, True):
        want = ref["dec" if dec else "raw"]
        ho, wo = (h, w) if dec else (2 * h, 2 * w)
        raw = _raw(N, ho, wo)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, want, f"{what} _tail_raw dec {dec}")
        raw = _raw(N, ho, wo)
        m._tail_raw(a, P, dec, raw, fold=(a, b, cm))
        E.assert_exact(raw, want, f"{what} _tail_raw fold dec {dec}")
        for rps in sorted({h, min(h, 5), 1}, reverse=True):
            for blob, name in ((P["tail_s2"], "blob with fold_co"), (plain, "blob without fold_co")):
                raw = _raw(N, ho, wo)
                L.check(lib.vsr_sr_tail_s2_f16(L.dptr(hid, torch.float16), L.dptr(blob, torch.uint8), L.dptr(raw), N, h, w, rps, le1, int(dec), L.stream()), "sr_tail_s2_f16")
                E.assert_exact(raw, want, f"{what} k_tail_s2 {name} dec {dec} rps {rps}")
            raw = _raw(N, ho, wo)
            L.check(lib.vsr_sr_tail_s2_fold_f16(L.dptr(a, torch.float16), L.dptr(b, torch.float16), L.dptr(cm), L.dptr(P["tail_s2"], torch.uint8), L.dptr(raw),
                                                N, h, w, rps, le1, int(dec), L.stream()), "sr_tail_s2_fold_f16")
            E.assert_exact(raw, want, f"{what} k_tail_s2<FOLD> dec {dec} rps {rps}")
            raw = _raw(N, ho, wo)
            L.check(lib.vsr_sr_tail_s2_f16(L.dptr(hid, torch.float16), L.dptr(plain, torch.uint8), L.dptr(raw), N, h, w, rps, 0, int(dec), L.stream()), "sr_tail_s2_f16")
            E.assert_exact(raw, want, f"{what} k_tail_s2 select build dec {dec} rps {rps}")


@pytest.mark.parametrize("slope,co_slope", [(2.0, 0.5), (-0.5, 2.0), (1.0, -0.5)])
def test_x2_tail_select_build(slope, co_slope):
    shape = (2, 9, 33)
    c, ref = gen_tail(int(slope * 8) + 55, 2, shape, slope=slope, profile="dense", fold=True, co_slope=co_slope)
    m = tail_module(c)
    P = m._packed()
    a, b, cm, hid = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"]), E.nhwc(c["hid"]).cuda()
    for dec in (False, True):
        raw = _raw(2, 9 if dec else 18, 33 if dec else 66)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, ref["dec" if dec else "raw"], f"x2 tail slope {slope} dec {dec}")
        raw = _raw(2, 9 if dec else 18, 33 if dec else 66)
        m._tail_raw(a, P, dec, raw, fold=(a, b, cm))
        E.assert_exact(raw, ref["dec" if dec else "raw"], f"x2 folded tail slope {slope} co slope {co_slope} dec {dec}")


# ---------------------------------------------------------------------------------------------------------------- x3 tail
@pytest.mark.parametrize("profile", TAIL_PROFILES)
@pytest.mark.parametrize("shape", [(1, 1, 29), (1, 2, 2), (2, 13, 31), (8, 6, 10), (2, 17, 3), (1, 1, 1)])
def test_x3_tail_equals_float64(shape, profile):
    """`_PhaseDeconv` (nine phase convolutions of the k7 s3 deconvolution on the generic MFMA kernel) + vsr_sr_convout_planes_f16 with
    step 1 and step 3, through `_tail_raw`; the HR map between them is compared too."""
    N, h, w = shape
    slope = E.SLOPES_LE_ONE[(N + h + w + 2) % 4]
    c, ref = gen_tail(N * 1000 + h * 10 + w + 3, 3, shape, slope=slope, profile=profile)
    m = tail_module(c)
    P = m._packed()
    hid = E.nhwc(c["hid"]).cuda()
    E.assert_exact(E.nchw64(P["out_deconv"](hid)), ref["hr"], f"x3 {shape} {profile} _PhaseDeconv")
    for dec in (False, True):
        raw = _raw(N, h if dec else 3 * h, w if dec else 3 * w)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, ref["dec" if dec else "raw"], f"x3 tail {shape} {profile} slope {slope} step {3 if dec else 1}")


# ---------------------------------------------------------------------------------------------------------------- fusion
def gen_fc(rs, n):
    """A small-integer fusion MLP whose two sums take both signs on planes of 0..300: first-layer rows that sum to about zero around a
    bias of either sign, second-layer weights (halves) of alternating sign."""
    w1 = E.sparse_weights(rs, (32, n), 0.7, 2)
    b1 = E.ints(rs, (32,), -60, 60) - 128.0 * w1.sum(1)
    w2 = torch.from_numpy(rs.randint(1, 5, size=32) * 0.5 * np.where(np.arange(32) % 2 == 0, 1.0, -1.0))
    return w1, b1, w2, E.ints(rs, (1,), -40, 40)


def gen_fusion(seed, S, shape, dec, n=8):
    """raw planes (eighths), pixels 0..255, dyadic MeanShifts, a sparse small-integer MLP; -> case, planes, fused frame."""
    h, w = shape
    rs = np.random.RandomState(seed)
    ho, wo = (h, w) if dec else (S * h, S * w)
    sub, add = mean_shifts()
    c = dict(raw=E.ints(rs, (n, 3, ho, wo), -64, 64, step=0.125), x=E.ints(rs, (n, 3, h, w), 0, 255), sub=sub, add=add,
             fc=gen_fc(rs, n))
    planes = E.planes_ref(c["raw"], c["x"], sub, add, S, decimate=dec)
    return c, planes, E.mlp_ref(planes, c["fc"], live=n > 1 and planes[0].numel() >= 64)      # (a handful of pixels need not hold both signs)


def _fc_dev(c):
    f = lambda t: t.float().contiguous().cuda()
    w1, b1, w2, b2 = c["fc"]
    (ss, sb), (as_, ab) = c["sub"], c["add"]
    return f(w1), f(b1), f(w2), f(b2), f(torch.cat((torch.zeros(3, dtype=torch.float64), ss, sb, as_, ab)))


FUSION_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (9, 7), (5, 33), (16, 16)]


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", FUSION_SHAPES)
def test_x4_fusion_with_skip_equals_float64(shape):
    """vsr_sr_fc_planes_skip_f32: four pixels per thread (full frames), one pixel per thread (decimated frames, and full frames under
    vsr_sr_chain_variant(2)), against fusion_ref.  Sizes of 1 and 2 clamp every bilinear tap."""
    h, w = shape
    lib = L.load()
    for dec in (False, True):
        c, planes, want = gen_fusion(h * 100 + w + dec, 4, shape, dec)
        w1, b1, w2, b2, tpar = _fc_dev(c)
        raw, x = c["raw"].float().cuda(), c["x"].float().cuda()
        try:
            for variant in (0, 2):
                lib.vsr_sr_chain_variant(variant)
                out = torch.full((1, 3) + tuple(want.shape[2:]), float("nan"), dtype=torch.float32, device="cuda")
                L.check(lib.vsr_sr_fc_planes_skip_f32(L.dptr(raw), L.dptr(x), L.dptr(tpar), L.dptr(w1), L.dptr(b1), L.dptr(w2), L.dptr(b2), 8, 32, L.dptr(out),
                                                      h, w, int(dec), L.stream()), "sr_fc_planes_skip")
                E.assert_exact(out, want, f"x4 fusion {shape} dec {dec} variant {variant}")
        finally:
            lib.vsr_sr_chain_variant(0)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("shape", FUSION_SHAPES)
def test_scaled_fusion_with_skip_equals_float64(shape, S):
    """vsr_sr_fc_planes_skip_scale_f32 for the dyadic factors, full and decimated."""
    h, w = shape
    for dec in (False, True):
        c, planes, want = gen_fusion(h * 100 + w + dec + S * 7, S, shape, dec)
        w1, b1, w2, b2, tpar = _fc_dev(c)
        out = torch.full((1, 3) + tuple(want.shape[2:]), float("nan"), dtype=torch.float32, device="cuda")
        raw, x = c["raw"].float().cuda(), c["x"].float().cuda()
        L.check(L.load().vsr_sr_fc_planes_skip_scale_f32(L.dptr(raw), L.dptr(x), L.dptr(tpar), L.dptr(w1), L.dptr(b1),
                                                         L.dptr(w2), L.dptr(b2), 8, 32, L.dptr(out), h, w, S, int(dec), L.stream()), "sr_fc_planes_skip_scale")
        E.assert_exact(out, want, f"x{S} fusion {shape} dec {dec}")


@pytest.mark.xcheck
@pytest.mark.parametrize("n", range(1, 9))
def test_plain_fusion_mlps_equal_float64(n):
    """vsr_sr_fc_fuse_f32 for 1..8 planes (NCHW and NHWC output) and, for the eight planes it is built for, vsr_sr_fc_planes_f32 of the
    cross-check library, on finished planes."""
    shape = (7, 9 + n)
    c, planes, want = gen_fusion(900 + n, 4, shape, True, n=n)
    w1, b1, w2, b2, _ = _fc_dev(c)
    pl = planes.float().cuda()
    Pn = shape[0] * shape[1]
    for nhwc in (0, 1):
        out = torch.full((3, Pn) if not nhwc else (Pn, 3), float("nan"), dtype=torch.float32, device="cuda")
        L.check(L.load().vsr_sr_fc_fuse_f32(L.dptr(pl), L.dptr(w1), L.dptr(b1), L.dptr(w2), L.dptr(b2), n, 32, L.dptr(out), Pn, nhwc, L.stream()), "sr_fc_fuse")
        E.assert_exact(out if not nhwc else out.t(), want.view(3, Pn), f"vsr_sr_fc_fuse_f32 {n} planes nhwc {nhwc}", names="cp")
        if n == 8:
            out = torch.full((3, Pn) if not nhwc else (Pn, 3), float("nan"), dtype=torch.float32, device="cuda")
            L.check(L.load_xcheck().vsr_sr_fc_planes_f32(L.dptr(pl), L.dptr(w1), L.dptr(b1), L.dptr(w2), L.dptr(b2), n, 32, L.dptr(out), Pn, nhwc, L.stream()), "sr_fc_planes")
            E.assert_exact(out if not nhwc else out.t(), want.view(3, Pn), f"vsr_sr_fc_planes_f32 nhwc {nhwc}", names="cp")


def _fma32(a, b, c):
    """fused multiply-add of float32 arrays, rounded once: the product of two float32 values is exact in float64; its sum with c is formed
    in float64 with the rounding error recovered (TwoSum) and folded in as a sticky last bit (round to odd), so that the final conversion
    to float32 is the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def fusion_x3_f32(raw, x, tpar, fc, h, w, dec):
    """csrc/sr_scale.hip k_fc_planes_skip_s for S = 3, restated in float32 numpy in the kernel's operation order."""
    S, f = 3, np.float32
    inv = f(1.0 / 3.0)

    def bil(n, dst):
        d = dst.astype(f) + f(0.5)
        src = _fma32(d, np.full_like(d, inv), np.full_like(d, f(-0.5)))      # (`bil` stands in front of the contraction pragma: the compiler fuses it)
        src = np.where(src < 0, f(0), src).astype(f)
        i0 = src.astype(np.int64)
        return i0, i0 + (i0 < n - 1), (src - i0.astype(f)).astype(f)

    ys, xs = np.arange(h if dec else S * h) * (S if dec else 1), np.arange(w if dec else S * w) * (S if dec else 1)
    y0, y1, ly = bil(h, ys)
    x0, x1, lx = bil(w, xs)
    ly, lx = ly[:, None], lx[None, :]
    w1, b1, w2, b2 = (t.numpy().astype(f) for t in fc)
    out = np.zeros((1, 3, len(ys), len(xs)), dtype=f)
    for c in range(3):
        sub_s, sub_b, add_s, add_b = (f(tpar[3 * k + c]) for k in (1, 2, 3, 4))
        v = []
        for i in range(raw.shape[0]):
            t = _fma32(x[i, c], np.full_like(x[i, c], sub_s), np.full_like(x[i, c], sub_b))
            v00, v01, v10, v11 = t[y0][:, x0], t[y0][:, x1], t[y1][:, x0], t[y1][:, x1]
            top = _fma32(np.broadcast_to(lx, v01.shape), v01, ((f(1) - lx) * v00).astype(f))
            bot = _fma32(np.broadcast_to(lx, v11.shape), v11, ((f(1) - lx) * v10).astype(f))
            lerp = _fma32(np.broadcast_to(ly, bot.shape), bot, ((f(1) - ly) * top).astype(f))
            sm = (lerp + raw[i, c]).astype(f)
            v.append(_fma32(sm, np.full_like(sm, add_s), np.full_like(sm, add_b)))
        o = np.full_like(v[0], b2[0])
        for j in range(w1.shape[0]):
            hs = np.full_like(v[0], b1[j])
            for i in range(len(v)):
                hs = _fma32(np.full_like(hs, w1[j, i]), v[i], hs)
            o = _fma32(np.full_like(o, w2[j]), np.maximum(hs, f(0)), o)
        out[0, c] = np.maximum(o, f(0))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 5), (9, 7), (5, 33)])
def test_x3_fusion_equals_its_float32_restatement(shape):
    """The x3 skip's weights are thirds (no exact regime): vsr_sr_fc_planes_skip_scale_f32 with S = 3 against the kernel's own float32
    arithmetic restated in numpy, every fused multiply-add rounded once, in the kernel's order.  Equality, no bar."""
    h, w = shape
    for dec in (False, True):
        rs = np.random.RandomState(h * 100 + w + dec)
        ho, wo = (h, w) if dec else (3 * h, 3 * w)
        sub, add = mean_shifts()
        c = dict(raw=E.ints(rs, (8, 3, ho, wo), -64, 64, step=0.125), x=E.ints(rs, (8, 3, h, w), 0, 255), sub=sub, add=add,
                 fc=gen_fc(rs, 8))
        w1, b1, w2, b2, tpar = _fc_dev(c)
        want = fusion_x3_f32(c["raw"].numpy().astype(np.float32), c["x"].numpy().astype(np.float32), tpar.cpu().numpy(), c["fc"], h, w, dec)
        assert want.size < 64 or ((want > 0).mean() > 0.1 and len(np.unique(want)) > want.size // 16)
        out = torch.full((1, 3, ho, wo), float("nan"), dtype=torch.float32, device="cuda")
        raw, x = c["raw"].float().cuda(), c["x"].float().cuda()
        L.check(L.load().vsr_sr_fc_planes_skip_scale_f32(L.dptr(raw), L.dptr(x), L.dptr(tpar), L.dptr(w1), L.dptr(b1),
                                                         L.dptr(w2), L.dptr(b2), 8, 32, L.dptr(out), h, w, 3, int(dec), L.stream()), "sr_fc_planes_skip_scale")
        E.assert_exact(out, torch.from_numpy(want), f"x3 fusion {shape} dec {dec}")


# ---------------------------------------------------------------------------------------------------------------- 1x1 chain
# per stage: (inputs read from memory, reads the previous stage, constant map).  The first seven go through the streaming builds
# (csrc/sr_f16.hip VSR_CHAIN_CASE), the others through the generic kernel.
CHAIN_SPECS = {
    "1": [(1, False, False)], "2": [(2, False, False)], "1m": [(1, False, True)], "2m": [(2, False, True)],
    "2-p": [(2, False, False), (0, True, False)], "1-p": [(1, False, False), (0, True, False)],
    "2m-1p-p": [(2, False, True), (1, True, False), (0, True, False)], "1m-1p-p": [(1, False, True), (1, True, False), (0, True, False)],
    "2-1p-p": [(2, False, False), (1, True, False), (0, True, False)],
    "1-1p": [(1, False, False), (1, True, False)], "2-pm": [(2, False, False), (0, True, True)],
    "1-2p-1pm": [(1, False, False), (2, True, False), (1, True, True)], "2m-2-2p": [(2, False, True), (2, False, False), (2, True, False)],
}


def gen_chain(seed, spec, N, P, slopes=(0.5, 0.25, 1.0), live=True, n_ins=None):
    rs = np.random.RandomState(seed)
    stages = []
    for s, (nin, prev, cm) in enumerate(spec):
        stages.append(dict(ins=[(E.ints(rs, (N, 32, P), -2, 2), E.sparse_weights(rs, (32, 32), 0.15, 1)) for _ in range(nin)],
                           prev=E.sparse_weights(rs, (32, 32), 0.15, 1) if prev else None, bias=E.ints(rs, (32,), -2, 2),
                           cmap=E.ints(rs, (32, P), -4, 4, step=0.5) if cm else None, slope=slopes[s]))
    return stages, E.chain_ref(stages, live=live and N * P >= 64)


def _nhwc1(x):
    """[N,32,P] float64 -> [N,P,32] fp16 on the device."""
    return E.check_storable(x, torch.float16, "chain input").permute(0, 2, 1).contiguous().to(torch.float16).cuda()


def _wide(rs, wm, ld, col):
    """The [32,32] weight as columns col.. of a [32,ld] float32 matrix whose other columns hold other values."""
    full = torch.from_numpy(rs.randint(-3, 4, size=(32, ld)).astype(np.float32))
    full[:, col:col + 32] = wm.float()
    return full.cuda()


def chain_dev(stages, seed=0):
    rs = np.random.RandomState(seed + 12345)
    dev = []
    for st in stages:
        d = dict(ins=[(_nhwc1(x), _wide(rs, wm, 96, 32 * t), 32 * t) for t, (x, wm) in enumerate(st["ins"])], bias=st["bias"].float().cuda(), slope=st["slope"])
        if st.get("prev") is not None:
            d["prev"] = (_wide(rs, st["prev"], 192, 64 if len(dev) == 1 else 128), 64 if len(dev) == 1 else 128)
        if st.get("cmap") is not None:
            d["cmap"] = st["cmap"].t().contiguous().float().cuda()
        dev.append(d)
    return dev


def _nchw1(t):
    return t.detach().cpu().permute(0, 2, 1).contiguous()


@pytest.mark.xcheck
@pytest.mark.parametrize("N,P", [(1, 1), (2, 63), (1, 64), (3, 65), (2, 3001)])
@pytest.mark.parametrize("name", sorted(CHAIN_SPECS))
def test_chain_with_its_own_operands_equals_float64(name, N, P):
    """SRProjectionModule._chain (vsr_sr_chain1x1_f16): 1-3 stages, 1-2 memory inputs per stage read at a column offset of wider weight
    matrices, `prev` at columns 64 / 128 of a 192-column matrix, constant maps on the first and on later stages, every `keep` pattern
    that keeps the last stage, the streaming builds and the generic kernel (vsr_sr_chain_variant 1)."""
    spec = CHAIN_SPECS[name]
    stages, ref = gen_chain(len(name) * 1000 + N * 100 + P, spec, N, P)
    dev = chain_dev(stages, P)
    n = len(spec)
    keeps = {1: [(1,)], 2: [(0, 1), (1, 1)], 3: [(0, 0, 1), (1, 1, 1), (1, 0, 1)]}[n]
    lib = L.load()
    try:
        for variant in (0, 1):
            lib.vsr_sr_chain_variant(variant)
            for keep in keeps:
                outs = SRProjectionModule._chain(dev, N, P, keep=list(keep))
                for s in range(n):
                    assert (outs[s] is not None) == bool(keep[s])
                    if keep[s]:
                        E.assert_exact(_nchw1(outs[s]), ref[s], f"chain {name} N {N} P {P} variant {variant} keep {keep} stage {s}", names="ncp")
    finally:
        lib.vsr_sr_chain_variant(0)


@pytest.mark.xcheck
@pytest.mark.parametrize("P", [1, 65, 3001])
@pytest.mark.parametrize("name", ["1", "2m", "1-p"])
def test_chain_stage_in_place(name, P):
    """A stage may write over its own input (`outs` = the input tensor): every pixel is read before it is written."""
    N = 2
    spec = CHAIN_SPECS[name]
    stages, ref = gen_chain(P + len(name), spec, N, P)
    lib = L.load()
    try:
        for variant in (0, 1):
            lib.vsr_sr_chain_variant(variant)
            dev = chain_dev(stages, P)
            given = [None] * len(spec)
            given[-1] = dev[0]["ins"][0][0]
            outs = SRProjectionModule._chain(dev, N, P, keep=[False] * (len(spec) - 1) + [True], outs=given)
            assert outs[-1].data_ptr() == dev[0]["ins"][0][0].data_ptr()
            E.assert_exact(_nchw1(outs[-1]), ref[-1], f"chain {name} in place P {P} variant {variant}", names="ncp")
    finally:
        lib.vsr_sr_chain_variant(0)


@pytest.mark.parametrize("slope", E.SLOPES_SELECT + (0.0,))
@pytest.mark.parametrize("nin,cm", [(1, False), (2, True), (3, False), (3, True)])
@pytest.mark.parametrize("N,P", [(1, 1), (2, 65), (3, 1000)])
def test_conv1x1_f16_equals_float64(N, P, nin, cm, slope):
    """SRProjectionModule._c1h (vsr_sr_conv1x1_f16): one stage over 1, 2 and 3 inputs, with and without the constant map; slopes of the
    select form and 0.  The one- and two-input cases go through `_chain` as well."""
    stages, ref = gen_chain(N * 100 + P + nin * 7 + int(slope * 4), [(nin, False, cm)], N, P, slopes=(slope,))
    rs = np.random.RandomState(P)
    st = stages[0]
    ins = [(_nhwc1(x), _wide(rs, wm, 128, 32 * (t + 1)), 32 * (t + 1)) for t, (x, wm) in enumerate(st["ins"])]
    cmap = st["cmap"].t().contiguous().float().cuda() if cm else None
    bias = st["bias"].float().cuda()
    E.assert_exact(_nchw1(SRProjectionModule._c1h(ins, bias, slope, N, P, cmap=cmap)), ref[0], f"_c1h N {N} P {P} inputs {nin} map {cm} slope {slope}", names="ncp")
    if nin <= 2:
        out = SRProjectionModule._chain([dict(ins=ins, bias=bias, slope=slope, cmap=cmap)], N, P, keep=[True])[0]
        E.assert_exact(_nchw1(out), ref[0], f"_chain N {N} P {P} inputs {nin} map {cm} slope {slope}", names="ncp")


# ---------------------------------------------------------------------------------------------------------------- head
# fp16 holds 11 bits: an 8-bit pixel with a 3-bit mean fraction fills them, and a sum of two such values leaves them.  Two profiles:
#   "taps":   6-bit pixels, scales AND biases that differ per channel (halves), ~2.5 conv_in taps per mid channel, ~2 feat_in elements per row;
#   "pixels": pixels 0..255 with mean 0.5 (halves), ONE conv_in tap per mid channel and ONE feat_in element per output channel.
HEAD_SUB = {"taps": (_t((1.0, 0.5, 2.0)), _t((-31.5, -16.0, -63.0))), "pixels": (_t((1.0, 1.0, 1.0)), _t((-127.5, -127.5, -127.5)))}


def _one_per_row(rs, rows, cols):
    wm = np.zeros((rows, cols))
    wm[np.arange(rows), rs.randint(0, cols, size=rows)] = rs.randint(0, 2, size=rows) * 2 - 1
    return torch.from_numpy(wm)


def gen_head(seed, shape, f32=False, slopes=(0.5, 0.25), live=True, profile="taps"):
    N, h, w = shape
    rs = np.random.RandomState(seed)
    c = dict(x=E.ints(rs, (N, 3, h, w), 0, 255 if (f32 or profile == "pixels") else 63), a_in=slopes[0], a_feat=slopes[1])
    if f32:   # float32 holds integers to 2^24: dense small-integer weights, the dyadic means of the tail
        c.update(sub=mean_shifts()[0], w_in=E.sparse_weights(rs, (128, 3, 3, 3), 1.0, 3), b_in=E.ints(rs, (128,), -50, 50),
                 w_feat=E.sparse_weights(rs, (32, 128), 1.0, 2), b_feat=E.ints(rs, (32,), -50, 50))
    elif profile == "pixels":
        c.update(sub=HEAD_SUB[profile], w_in=_one_per_row(rs, 128, 27).view(128, 3, 3, 3), b_in=E.ints(rs, (128,), -4, 4),
                 w_feat=_one_per_row(rs, 32, 128), b_feat=E.ints(rs, (32,), -4, 4))
    else:
        c.update(sub=HEAD_SUB[profile], w_in=E.sparse_weights(rs, (128, 3, 3, 3), 2.5 / 27, 1), b_in=E.ints(rs, (128,), -4, 4),
                 w_feat=E.sparse_weights(rs, (32, 128), 2.0 / 128, 1), b_feat=E.ints(rs, (32,), -4, 4))
    ref = E.head_ref(c["x"], c["sub"], c["w_in"], c["b_in"], c["a_in"], c["w_feat"], c["b_feat"], c["a_feat"],
                     store=torch.float32 if f32 else torch.float16, live=live and N * h * w >= 64)
    return c, ref


def head_module(c):
    m = _seeded(4)
    with torch.no_grad():
        m.conv_in[0].weight.copy_(c["w_in"])
        m.conv_in[0].bias.copy_(c["b_in"])
        m.conv_in[1].weight.fill_(c["a_in"])
        m.feat_in[0].weight.copy_(c["w_feat"].view(32, 128, 1, 1))
        m.feat_in[0].bias.copy_(c["b_feat"])
        m.feat_in[1].weight.fill_(c["a_feat"])
    _set_mean_shift(m, c["sub"], mean_shifts()[1])
    return m.cuda()


def _head(P, x, shape, f16=True):
    N, h, w = shape
    out = torch.full((N, h, w, 32) if f16 else (N, 32, h, w), float("nan"), dtype=torch.float16 if f16 else torch.float32, device="cuda")
    fn = L.load().vsr_sr_head_f16 if f16 else L.load().vsr_sr_head_f32
    L.check(fn(L.dptr(x), L.dptr(P["sub_s"]), L.dptr(P["sub_b"]), L.dptr(P["w_in"]), L.dptr(P["b_in"]), L.cf(P["a_in"]), P["w_in"].shape[0],
               L.dptr(P["w_feat"]), L.dptr(P["b_feat"]), L.cf(P["a_feat"]), L.dptr(out, out.dtype), N, h, w, L.stream()), "sr_head")
    return E.nchw64(out) if f16 else out


HEAD_SHAPES = [(1, 1, 1), (1, 1, 7), (3, 2, 2), (8, 9, 40), (2, 37, 33), (1, 5, 17)]


@pytest.mark.parametrize("profile", ["taps", "pixels"])
@pytest.mark.parametrize("slopes", [(0.5, 0.25), (2.0, -0.5), (1.0, 0.0)])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_f16_equals_float64(shape, slopes, profile):
    """vsr_sr_head_f16 (k_head_h): sub_mean -> conv_in 3x3 + PReLU -> feat_in 1x1 + PReLU -> NHWC fp16, with per-channel scales AND
    biases that differ (a swapped channel is seen), max and select forms of both PReLUs."""
    c, ref = gen_head(sum(shape) * 10 + int(slopes[0] * 4), shape, slopes=slopes, profile=profile)
    P = head_module(c)._packed()
    E.assert_exact(_head(P, c["x"].float().cuda(), shape), ref, f"head fp16 {shape} slopes {slopes} {profile}")


@pytest.mark.xcheck
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_f32_equals_float64(shape, variant):
    """vsr_sr_head_f32, both builds (vsr_sr_f32_variant), dense weights, pixels 0..255 with the dyadic means."""
    c, ref = gen_head(sum(shape) * 10 + 1, shape, f32=True)
    P = head_module(c)._packed()
    lib = L.load()
    try:
        lib.vsr_sr_f32_variant(variant)
        E.assert_exact(_head(P, c["x"].float().cuda(), shape, f16=False), ref, f"head fp32 {shape} variant {variant}")
    finally:
        lib.vsr_sr_f32_variant(0)


# ---------------------------------------------------------------------------------------------------------------- uint8 ends
def u8_ref(v):
    """The HR write-out convention (include/vsr_hip.h vsr_frame_to_u8; the reference project never writes frames): round half to even,
    clamp to 0..255, NaN -> 0; numpy float32."""
    with np.errstate(invalid="ignore"):
        r = np.rint(v.astype(np.float32))
        r = np.where(np.isnan(r), np.float32(0), r)
        return np.clip(r, 0, 255).astype(np.uint8)


def test_frame_to_u8_at_every_half_and_beside_it():
    from video_super_resolution_amd import driver
    f = np.float32
    halves = np.arange(-2, 257, dtype=f) + f(0.5)
    v = np.concatenate([halves, np.nextafter(halves, f(np.inf)), np.nextafter(halves, f(-np.inf)), np.arange(-3, 259, dtype=f),
                        np.array([-0.0, 0.0, 1e-30, -1e-30, 254.99998, 255.00002, 1e9, -1e9, 3e38, -3e38, np.inf, -np.inf, np.nan, -np.nan,
                                  2147483648.0, -2147483648.0, 4294967296.0, 65536.5, 256.0, 511.5], dtype=f)])
    want = u8_ref(v)
    assert want[0] == 0 and want[np.where(halves == f(0.5))[0][0]] == 0 and want[np.where(halves == f(1.5))[0][0]] == 2 and want.max() == 255
    for n in (v.size, v.size - 1, v.size - 2, v.size - 3, 5, 1):       # (four values per thread: every remainder)
        got = driver.frames_to_u8(torch.from_numpy(v[:n].copy()).cuda()).cpu().numpy()
        bad = np.nonzero(got != want[:n])[0]
        assert bad.size == 0, f"vsr_frame_to_u8 n {n}: {bad.size} values differ; first {v[bad[0]]!r} -> {got[bad[0]]} (want {want[bad[0]]})"


def ingest_ref(d, scale):
    """driver.ingest_item in numpy: nearest-neighbour x1/scale of each frame with ATen's index rule src = min(floor(dst * (float)in / out),
    in - 1) in float32, and the float copy.  d uint8 [T,3,H,W,3]."""
    T, _, H, W, _ = d.shape
    h, w = int(H / scale), int(W / scale)
    f = np.float32
    yy = np.minimum(np.floor(np.arange(h, dtype=f) * (f(H) / f(h))).astype(np.int64), H - 1)
    xx = np.minimum(np.floor(np.arange(w, dtype=f) * (f(W) / f(w))).astype(np.int64), W - 1)
    return d[:, :, yy][:, :, :, xx].astype(f), d.astype(f)


@pytest.mark.parametrize("scale", [4, 2, 3])
@pytest.mark.parametrize("T,H,W", [(1, 4, 4), (2, 13, 19), (1, 37, 1031), (3, 9, 7), (1, 5, 4)])
def test_clip_ingest_u8_on_odd_sizes(T, H, W, scale):
    from video_super_resolution_amd import driver
    d = np.random.RandomState(H * 100 + W).randint(0, 256, (T, 3, H, W, 3)).astype(np.uint8)
    d[0, 0, 0, 0], d[-1, -1, -1, -1] = 0, 255
    lr, hr = ingest_ref(d, scale)
    got_lr, target, got_hr = driver.ingest_item(torch.from_numpy(d).cuda(), scale)
    E.assert_exact(got_lr, torch.from_numpy(lr), f"vsr_clip_ingest_u8 LR {T}x{H}x{W} /{scale}", names="tfyxc")
    E.assert_exact(got_hr, torch.from_numpy(hr), f"vsr_clip_ingest_u8 float copy {T}x{H}x{W}", names="tfyxc")
    E.assert_exact(target, torch.from_numpy(hr[:, 1:2]), "target", names="tfyxc")


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _planted(got, planted, ref, what):
    """The kernel follows its own (changed) weights, the comparison with the unchanged reference fails, and it fails exactly where the
    float64 evaluation of the changed weights differs.  -> that mask."""
    E.assert_exact(got, planted, f"{what}: the kernel follows its own weights")
    pred = planted != ref
    assert bool(pred.any()) and not bool(pred.all())
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got, ref, "planted")
    mask = E.diff_mask(got, ref)
    assert torch.equal(mask, pred) and E.bbox(mask) == E.bbox(pred)
    return mask


_TAIL_PLANTS = [("out_w", (31, 9, 0, 5)), ("out_w", (0, 30, 3, 2)), ("cv_w", (1, 31, 2, 0)), ("cv_w", (2, 0, 0, 2)), ("co_w", (5, 63))]


@pytest.mark.parametrize("S,which,idx", [(S, wh, i) for S in (4, 2, 3) for wh, i in _TAIL_PLANTS if not (S == 3 and wh == "co_w")])   # (x3 has no folded build)
def test_one_unit_in_one_tail_weight_is_seen_with_its_footprint(S, which, idx):
    """ONE element of the `out` deconvolution, of conv_out or of the folded compress_out one unit off on the GPU side.  Footprints: a
    deconvolution tap reaches the HR pixels of its phase (in one channel), which conv_out spreads by one pixel; a conv_out element
    changes one output channel only."""
    shape = (2, 7, 33)
    N, h, w = shape
    fold = which == "co_w" or S == 2
    c, ref = gen_tail(S * 10 + len(which), S, shape, slope=1.0, profile="dense", fold=fold, co_slope=1.0)
    c2 = dict(c)
    c2[which] = c[which].clone()
    c2[which][idx] += 1.0
    if which == "co_w":
        c2["hid"] = E.fold_ref(c2["lr_a"], c2["lr_b"], c2["cmap"], c2["co_w"], c2["co_b"], c2["co_a"], live=False)
    planted = E.tail_ref(c2["hid"], c2["out_w"], c2["out_b"], c2["out_a"], c2["cv_w"], c2["cv_b"], S, live=False)
    m = tail_module(c2)
    P = m._packed()
    le1 = int(P["slopes_le_one"])
    if fold:
        a, b, cm = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"])
        if S == 4:
            got = _tail3_fold(P, a, b, cm, shape, h, le1, False)
        else:
            got = _raw(N, S * h, S * w)
            m._tail_raw(a, P, False, got, fold=(a, b, cm))
    elif S == 4:
        got = _tail3(P, E.nhwc(c["hid"]).cuda(), shape, h, le1, False)
    else:
        got = _raw(N, S * h, S * w)
        m._tail_raw(E.nhwc(c["hid"]).cuda(), P, False, got)
    mask = _planted(got, planted["raw"], ref["raw"], f"x{S} planted {which}{idx}")
    if which == "cv_w":
        assert E.bbox(mask)[1] == (idx[0], idx[0])                      # one output channel
    elif which == "out_w":
        hr_diff = planted["hr"] != ref["hr"]
        assert not bool(hr_diff[:, [ch for ch in range(32) if ch != idx[1]]].any())      # one HR channel ...
        ys, xs = torch.nonzero(hr_diff.any(0).any(0), as_tuple=True)
        assert bool(((ys + 2 - idx[2]) % S == 0).all()) and bool(((xs + 2 - idx[3]) % S == 0).all())   # ... at the tap's phase
        box = E.bbox(mask)
        assert box[2][0] >= max(0, int(ys.min()) - 1) and box[2][1] <= min(S * h - 1, int(ys.max()) + 1)
        assert box[3][0] >= max(0, int(xs.min()) - 1) and box[3][1] <= min(S * w - 1, int(xs.max()) + 1)
    else:
        assert not bool((c2["hid"] != c["hid"])[:, [ch for ch in range(32) if ch != idx[0]]].any())   # one channel of the 1x1's output


@pytest.mark.parametrize("stage,term,idx", [(0, 0, (3, 17)), (1, "prev", (31, 0)), (2, "prev", (0, 31)), (1, 0, (16, 8))])
def test_one_unit_in_one_chain_weight_is_seen_with_its_footprint(stage, term, idx):
    """One element of one stage's weight one unit off: that stage's output differs in one channel only (and the stages behind follow)."""
    N, P = 2, 200
    spec = CHAIN_SPECS["2m-1p-p"]
    stages, ref = gen_chain(4242, spec, N, P, slopes=(1.0, 1.0, 1.0))
    st2 = [dict(s) for s in stages]
    if term == "prev":
        st2[stage]["prev"] = stages[stage]["prev"].clone()
        st2[stage]["prev"][idx] += 1.0
    else:
        x, wm = stages[stage]["ins"][term]
        st2[stage]["ins"] = list(stages[stage]["ins"])
        st2[stage]["ins"][term] = (x, wm.clone())
        st2[stage]["ins"][term][1][idx] += 1.0
    planted = E.chain_ref(st2, live=False)
    outs = SRProjectionModule._chain(chain_dev(st2, 1), N, P, keep=[True, True, True])
    for s in range(3):
        if s < stage:
            E.assert_exact(_nchw1(outs[s]), ref[s], f"stage {s} in front of the planted one", names="ncp")
            assert torch.equal(planted[s], ref[s])
    mask = _planted(_nchw1(outs[stage]), planted[stage], ref[stage], f"chain planted stage {stage} {term}{idx}")
    assert E.bbox(mask)[1] == (idx[0], idx[0])
    for s in range(stage + 1, 3):
        E.assert_exact(_nchw1(outs[s]), planted[s], f"stage {s} behind the planted one", names="ncp")


@pytest.mark.parametrize("which,idx", [("w_in", (77, 2, 0, 2)), ("w_in", (0, 0, 2, 0)), ("w_feat", (31, 127))])
def test_one_unit_in_one_head_weight_is_seen_with_its_footprint(which, idx):
    """One conv_in tap (one mid channel, seen through the feat_in rows that read it) or one feat_in element (one output channel)."""
    shape = (2, 9, 40)
    c, ref = gen_head(99, shape, slopes=(1.0, 1.0))
    c2 = dict(c)
    c2[which] = c[which].clone()
    c2[which][idx] += 1.0
    if which == "w_in":      # (seen at the output only through a feat_in element that reads the mid channel: make sure of one)
        for cc in (c, c2):
            cc["w_feat"] = cc["w_feat"].clone()
            cc["w_feat"][5, idx[0]] = 1.0
        ref = E.head_ref(c["x"], c["sub"], c["w_in"], c["b_in"], 1.0, c["w_feat"], c["b_feat"], 1.0)
    planted = E.head_ref(c2["x"], c2["sub"], c2["w_in"], c2["b_in"], 1.0, c2["w_feat"], c2["b_feat"], 1.0, live=False)
    P = head_module(c2)._packed()
    mask = _planted(_head(P, c["x"].float().cuda(), shape), planted, ref, f"head planted {which}{idx}")
    readers = torch.nonzero(c2["w_feat"][:, idx[0]]).flatten().tolist() if which == "w_in" else [idx[0]]
    assert set(torch.nonzero(mask.any(0).any(-1).any(-1)).flatten().tolist()) <= set(readers)
    if which == "w_in":      # a tap at (ky, kx) of channel ci never reaches the output row / column whose neighbour lies outside the frame
        ky, kx = idx[2:]
        box = E.bbox(mask)
        assert (ky != 0 or box[2][0] >= 1) and (ky != 2 or box[2][1] <= shape[1] - 2) and (kx != 0 or box[3][0] >= 1) and (kx != 2 or box[3][1] <= shape[2] - 2)
