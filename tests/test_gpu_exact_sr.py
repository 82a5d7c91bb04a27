"""The SR net's kernels in EXACT arithmetic: the fused FeedbackBlock stage of every scale and build, its POST output, the unfused
stage and the float32 blocks equal a float64 CPU evaluation bit for bit on operands inside the budget tests/_exact.py checks (small
integers, PReLU slopes that are powers of two, every fp16-stored value an fp16 value on both sides of each PReLU).

Weights are set on a deep copy of an SRProjectionModule whose `_packed()` then runs the packers (`pack_utd_blob` layouts 1, 2, 4,
`pack_utd_s2_blob` layouts 1 and 4, `pack_utd_s3_blob`, `_PhaseDeconv`, `pack_dt_frags`): packer and kernel are held together against
an independent evaluation, not against each other.  Three weight profiles make each of the three layers dense in turn (the other two
sparse), because a dense layer is what sees a misplaced fragment element and all three cannot be dense inside the fp16 budget.

A sensitivity case per family gives the kernel a weight tensor with ONE element one unit off and asserts that the comparison fails
with exactly the predicted footprint.

Out of scope: whole `SRProjectionModule.forward` / `VSR.forward` in exact arithmetic (the mean shifts by 255 * mean, the fusion MLP and
three recurrent steps leave the exact regime; the oracle tests cover them), the flow operators already compared bit-exactly with
oracle/native_ops.c, the training kernels of csrc/sr_train.hip (float64 autograd in test_gpu_train_step.py).  The two ends of the net --
the head k_head_h, the 1x1 chain kernel on its own, the tails (k_tail3, k_tail_s2, the x3 tail), the fusion kernels and the uint8
conversions -- have their exact cases in tests/test_gpu_exact_sr_ends.py."""
import copy

import numpy as np
import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import SRProjectionModule  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

_master = {}
PROFILES = ("up", "dt", "dn")       # which of the three layers is dense


def gen_stage(seed, S, shape, slopes=(0.5, 0.5, 0.5), profile="up", post_slope=0.5):
    """Exact operands of one stage (+ the next group's uptran slice for POST) and their float64 reference (`stage_ref` checks the
    budget).  Densities keep the three sums at a few tens, so that with granularity 1/16 at the output everything is an fp16 value."""
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(seed)
    t1, t3 = 32.0 * (k / S) ** 2, 32.0 * k * k          # terms per output of the deconvolution / the strided convolution
    d1, d2, d3 = {"up": (24.0 / t1, 0.12, 3.0 / t3), "dt": (3.0 / t1, 1.0, 4.0 / t3), "dn": (0.5 / t1, 0.03, 0.12)}[profile]
    c = dict(a=E.ints(rs, (N, 32, h, w), -2, 2), up_w=E.sparse_weights(rs, (32, 32, k, k), min(1.0, d1), 1), up_b=E.ints(rs, (32,), -2, 2), up_a=slopes[0],
             dt_w=E.sparse_weights(rs, (32, 32), d2, 1), dt_b=E.ints(rs, (32,), -2, 2), dt_a=slopes[1],
             dn_w=E.sparse_weights(rs, (32, 32, k, k), d3, 1), dn_b=E.ints(rs, (32,), -3, 3), dn_a=slopes[2], S=S)
    ref = E.stage_ref(**c, min_distinct=100)
    post_w, post_b = E.sparse_weights(rs, (32, 32), 0.06, 1), E.ints(rs, (32,), -2, 2)
    p0 = E.conv_ref(ref["out"], post_w.reshape(32, 32, 1, 1), post_b, what="POST 1x1", store=torch.float16)
    ref["post"] = E.check_storable(E.prelu_ref(p0, post_slope), torch.float16, "POST after PReLU")
    c.update(post_w=post_w, post_b=post_b, post_a=post_slope)
    return c, ref


def module(S, c, **attrs):
    """A deep copy of the seeded module of scale S with the case's weights on stage 0 (upBlocks[1], downtranBlocks[1] columns 64..95,
    downBlocks[2]) and on the uptran slice behind it (uptranBlocks[3] columns 128..159), on the GPU; `_packed()` repacks."""
    if S not in _master:
        _master[S] = fill_module_(SRProjectionModule(upscale_factor=S).eval(), seed=0, prefix="model.")
    m = copy.deepcopy(_master[S]).eval()
    b = m.block
    with torch.no_grad():
        b.upBlocks[1][0].weight.copy_(c["up_w"])
        b.upBlocks[1][0].bias.copy_(c["up_b"])
        b.upBlocks[1][1].weight.fill_(c["up_a"])
        assert b.downtranBlocks[1][0].weight.shape[1] >= 96 and b.uptranBlocks[3][0].weight.shape[1] >= 160
        b.downtranBlocks[1][0].weight[:, 64:96, 0, 0] = c["dt_w"].float()
        b.downtranBlocks[1][0].bias.copy_(c["dt_b"])
        b.downtranBlocks[1][1].weight.fill_(c["dt_a"])
        b.downBlocks[2][0].weight.copy_(c["dn_w"])
        b.downBlocks[2][0].bias.copy_(c["dn_b"])
        b.downBlocks[2][1].weight.fill_(c["dn_a"])
        b.uptranBlocks[3][0].weight[:, 128:160, 0, 0] = c["post_w"].float()
        b.uptranBlocks[3][0].bias.copy_(c["post_b"])
        b.uptranBlocks[3][1].weight.fill_(c["post_a"])
    m = m.cuda()
    m.precision = "fp16"
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _in(c):
    return E.nhwc(c["a"]).cuda()


def _new(a):
    return torch.full(tuple(a.shape), float("nan"), dtype=torch.float16, device="cuda")


SHAPES4 = [(1, 1, 31), (1, 2, 2), (2, 37, 45), (8, 12, 32), (2, 47, 3), (3, 5, 7), (1, 9, 65)]


@pytest.mark.xcheck
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("shape", SHAPES4)
def test_x4_stage_every_build_and_segmentation_equals_float64(shape, profile):
    """k_utd4 (the default), k_utd3, k_utd (vsr_sr_utd_variant 1), k_utd2, and k_utd3<POST> / k_utd4 with its post output, over the
    whole march, several row segments, one-row segments and the flat split (shares inside a strip, across strips and across planes):
    every launch equals the float64 reference, not only the others."""
    N, h, w = shape
    c, ref = gen_stage(N * 1000 + h * 10 + w, 4, shape, profile=profile)
    m = module(4, c)
    P = m._packed()
    le1 = int(P["slopes_le_one"])
    assert le1 == 1 and P["post_slopes_le_one"]
    a, lib = _in(c), L.load()
    what = f"x4 {shape} {profile}"
    E.assert_exact(E.nchw64(m._utd4(a, P["utd4"][0], N, h, w)), ref["out"], what + " k_utd4 (wrapper)")
    for rps in (h, 5, 1, -3, -7, -50, -1000):
        out, post = _new(a), _new(a)
        L.check(lib.vsr_sr_utd4_f16(L.dptr(a, torch.float16), L.dptr(P["utd4"][0], torch.uint8), L.dptr(out, torch.float16), L.dptr(post, torch.float16),
                                    N, h, w, rps, 1, L.stream()), "sr_utd4_f16")
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd4 rps {rps}")
        E.assert_exact(E.nchw64(post), ref["post"], f"{what} k_utd4 post rps {rps}")
        out, post = _new(a), _new(a)
        L.check(lib.vsr_sr_utd_post_f16(L.dptr(a, torch.float16), L.dptr(P["utd_post"][0], torch.uint8), L.dptr(out, torch.float16), L.dptr(post, torch.float16),
                                        N, h, w, rps, 1, L.stream()), "sr_utd_post_f16")
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd3<POST> rps {rps}")
        E.assert_exact(E.nchw64(post), ref["post"], f"{what} k_utd3<POST> post rps {rps}")
    try:
        for variant, name in ((0, "k_utd3"), (1, "k_utd")):
            lib.vsr_sr_utd_variant(variant)
            for rps in ((h, 5, 1, -3, -7, -50) if variant == 0 else (h, 5, 1)):
                out = _new(a)
                L.check(lib.vsr_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(P["utd"][0], torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 0, le1, L.stream()))
                E.assert_exact(E.nchw64(out), ref["out"], f"{what} {name} rps {rps}")
    finally:
        lib.vsr_sr_utd_variant(0)
    for rps in (h, 5, 1):
        out = _new(a)
        L.check(lib.vsr_sr_utd2_f16(L.dptr(a, torch.float16), L.dptr(P["utd2"][0], torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, le1, L.stream()))
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd2 rps {rps}")


SHAPES2 = [(1, 1, 31), (1, 2, 2), (2, 37, 95), (8, 12, 30), (2, 47, 3), (3, 5, 7)]


@pytest.mark.xcheck
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("shape", SHAPES2)
def test_x2_stage_every_build_equals_float64(shape, profile):
    """k_utd_s2 with its uniform branches and branch-free (vsr_sr_utd_s2_variant 1), k_utd_s2<POST>, k_utd_s2w, and _UnfusedStage."""
    from video_super_resolution_amd.sr import _UnfusedStage
    N, h, w = shape
    c, ref = gen_stage(N * 1000 + h * 10 + w + 2, 2, shape, profile=profile)
    a, lib = _in(c), L.load()
    what = f"x2 {shape} {profile}"
    m = module(2, c, utd_s2_build=1)
    P = m._packed()
    st = P["stage"][0]
    assert type(st).__name__ == "_FusedStageS2" and not st.wide and st.has_post
    E.assert_exact(E.nchw64(st(a, m._chain)), ref["out"], what + " k_utd_s2 (wrapper)")
    out, post = st(a, m._chain, post=True)
    E.assert_exact(E.nchw64(out), ref["out"], what + " k_utd_s2<POST>")
    E.assert_exact(E.nchw64(post), ref["post"], what + " k_utd_s2<POST> post")
    try:
        for variant in (0, 1):
            lib.vsr_sr_utd_s2_variant(variant)
            for rps in (h, 5, 1):
                out = _new(a)
                L.check(lib.vsr_sr_utd_s2_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 1, L.stream()))
                E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd_s2 variant {variant} rps {rps}")
    finally:
        lib.vsr_sr_utd_s2_variant(0)
    mw = module(2, c, utd_s2_build=2)
    sw = mw._packed()["stage"][0]
    assert sw.wide
    E.assert_exact(E.nchw64(sw(a, mw._chain)), ref["out"], what + " k_utd_s2w (wrapper)")
    for rps in (h, 5, 1):
        out = _new(a)
        L.check(lib.vsr_sr_utd_s2w_f16(L.dptr(a, torch.float16), L.dptr(sw.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 1, L.stream()))
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd_s2w rps {rps}")
    b = m.block
    unf = _UnfusedStage(b.upBlocks[1], P["dt_w"][1], 64, P["dt_b"][1], P["dt_a"][1], b.downBlocks[2], 2)
    E.assert_exact(E.nchw64(unf(a, m._chain)), ref["out"], what + " _UnfusedStage")


SHAPES3 = [(1, 1, 29), (1, 2, 30), (2, 37, 31), (8, 12, 59), (2, 47, 3), (1, 5, 61), (1, 1, 1)]   # (x3 marches 30 LR pixels per step)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("shape", SHAPES3)
def test_x3_stage_equals_float64(shape, profile):
    """k_utd_s3 (libvsr_hip_s3.so) over whole marches, segments and one-row segments, and _UnfusedStage at x3."""
    from video_super_resolution_amd.sr import _UnfusedStage
    N, h, w = shape
    c, ref = gen_stage(N * 1000 + h * 10 + w + 3, 3, shape, profile=profile)
    a = _in(c)
    what = f"x3 {shape} {profile}"
    m = module(3, c)
    P = m._packed()
    st = P["stage"][0]
    assert type(st).__name__ == "_FusedStageS3"
    E.assert_exact(E.nchw64(st(a, m._chain)), ref["out"], what + " k_utd_s3 (wrapper)")
    lib = L.load_s3()
    for rps in (0, 16, 3, 1):
        out = _new(a)
        L.check(lib.vsr_s3_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, rps, 1, L.stream()),
                "sr_utd_s3_f16", lib=lib)
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} k_utd_s3 rps {rps}")
    b = m.block
    unf = _UnfusedStage(b.upBlocks[1], P["dt_w"][1], 64, P["dt_b"][1], P["dt_a"][1], b.downBlocks[2], 3)
    E.assert_exact(E.nchw64(unf(a, m._chain)), ref["out"], what + " _UnfusedStage")


@pytest.mark.xcheck
@pytest.mark.parametrize("slopes", [(2.0, 0.5, -0.5), (-0.5, 2.0, 1.0), (1.0, 0.0, 0.25)])
@pytest.mark.parametrize("S", [4, 2, 3])
def test_stage_select_builds_and_slope_corners_equal_float64(S, slopes):
    """A slope of 2.0 and one of -0.5 (the select builds, slopes_le_one 0) and the corners 1 / 0 of the max builds, per scale."""
    shape = (2, 9, 33)
    c, ref = gen_stage(S * 100 + int(slopes[0] * 8), S, shape, slopes=slopes, profile="dt", post_slope=2.0 if slopes[0] > 1 else 0.25)
    N, h, w = shape
    m = module(S, c)
    P = m._packed()
    le1 = all(0 <= s <= 1.0 for s in slopes)
    assert bool(P["slopes_le_one"]) == all(s <= 1.0 for s in slopes)
    a = _in(c)
    what = f"x{S} slopes {slopes}"
    if S == 4:
        out, post = m._utd4(a, P["utd4"][0], N, h, w, post=True)
        E.assert_exact(E.nchw64(out), ref["out"], what + " k_utd4")
        E.assert_exact(E.nchw64(post), ref["post"], what + " k_utd4 post")
        out, post = m._utd_post(a, P["utd_post"][0], N, h, w)
        E.assert_exact(E.nchw64(out), ref["out"], what + " k_utd3<POST>")
        E.assert_exact(E.nchw64(post), ref["post"], what + " k_utd3<POST> post")
        E.assert_exact(E.nchw64(m._utd(a, P["utd"][0], N, h, w)), ref["out"], what + " k_utd3")
        E.assert_exact(E.nchw64(m._utd2(a, P["utd2"][0], N, h, w)), ref["out"], what + " k_utd2")
    else:
        st = P["stage"][0]
        E.assert_exact(E.nchw64(st(a, m._chain)), ref["out"], what + " fused")
        if st.has_post:
            out, post = st(a, m._chain, post=True)
            E.assert_exact(E.nchw64(out), ref["out"], what + " fused <POST>")
            E.assert_exact(E.nchw64(post), ref["post"], what + " fused <POST> post")
    if le1 and S != 4:      # the select build computes the same while the slopes are in [0, 1]
        st = P["stage"][0]
        out = _new(a)
        if S == 2:
            L.check(L.load().vsr_sr_utd_s2_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, h, 0, L.stream()))
        else:
            lib = L.load_s3()
            L.check(lib.vsr_s3_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, h, 0, L.stream()), "s3", lib=lib)
        E.assert_exact(E.nchw64(out), ref["out"], what + " select build")


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _run_default(S, m, a, shape):
    N, h, w = shape
    P = m._packed()
    return m._utd4(a, P["utd4"][0], N, h, w) if S == 4 else P["stage"][0](a, m._chain)


@pytest.mark.parametrize("S,which,idx", [
    (4, "dn", (5, 31, 7, 7)),                                  # x4: an element of the last K block of the strided convolution (channel 31, last tap)
    (4, "up", (31, 9, 0, 5)),                                  # x4: one deconvolution tap
    (2, "up", (3, 30, 5, 0)), (2, "dn", (17, 0, 0, 5)),
    (3, "up", (7, 11, 0, 6)),                                  # x3: a tap of a 4-tap phase (ky 0 / kx 6: phases with two taps per axis)
    (3, "up", (30, 2, 2, 3)),                                  # x3: a tap of a 6-tap phase (ky 2: three taps along y, kx 3: two along x)
    (3, "up", (0, 31, 5, 2)),                                  # x3: a tap of the 9-tap phase (ky 5, kx 2: three taps per axis)
    (3, "dn", (31, 31, 6, 6)),
])
def test_one_unit_in_one_stage_weight_is_seen_with_its_footprint(S, which, idx):
    """The kernel's weights differ from the reference's by ONE unit in ONE element.  The comparison must fail, and the differing
    outputs must be exactly where a float64 evaluation of the changed weights differs: for a deconvolution tap, the outputs whose
    receptive field holds an affected HR pixel of that tap's phase; for a strided-convolution element, one out-channel."""
    shape = (2, 7, 33)
    c, ref = gen_stage(S * 10, S, shape, slopes=(1.0, 1.0, 1.0), profile="dt")     # (slopes 1: nothing is clipped away before the output)
    c2 = dict(c)
    key = "up_w" if which == "up" else "dn_w"
    c2[key] = c[key].clone()
    c2[key][idx] += 1.0
    planted = E.stage_ref(**{k: v for k, v in c2.items() if not k.startswith("post")}, live=False)
    pred = planted["out"] != ref["out"]
    assert pred.any() and not pred.all()
    if which == "dn":
        only = torch.zeros_like(pred)
        only[:, idx[0]] = True
        assert not (pred & ~only).any()                          # one out-channel
    else:
        k, (ky, kx) = S + 4, idx[2:]
        hr_diff = planted["hr"] != ref["hr"]
        ys, xs = torch.nonzero(hr_diff.any(0).any(0), as_tuple=True)
        assert bool(((ys + 2 - ky) % S == 0).all()) and bool(((xs + 2 - kx) % S == 0).all())   # the HR pixels of one phase only
        assert hr_diff[:, [ch for ch in range(32) if ch != idx[1]]].sum() == 0 and k == c[key].shape[-1]
    a = _in(c)
    got = E.nchw64(_run_default(S, module(S, c2), a, shape))
    E.assert_exact(got, planted["out"], f"x{S} planted {which}{idx}: the kernel follows its own weights")
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got, ref["out"], "planted")
    assert torch.equal(E.diff_mask(got, ref["out"]), pred)


# ---------------------------------------------------------------------------------------------------------------- float32 blocks
@pytest.mark.xcheck
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("S,shape", [(4, (2, 9, 13)), (4, (1, 1, 33)), (2, (2, 17, 9)), (2, (1, 2, 2)), (3, (2, 7, 31)), (3, (8, 5, 3))])
def test_float32_blocks_equal_float64(S, shape, variant):
    """vsr_sr_deconv_f32 (with and without the downtran 1x1 fused into its epilogue, `pack_dt_frags`), vsr_sr_conv1x1_f32 and
    vsr_sr_conv_f32 of the float32 configuration, matrix-core builds (variant 0) and one pixel per thread (variant 1).  float32 holds
    integers to 2^24: operands in -9..9, dense weights in -3..3 (sums of a few thousand eighths); one planted unit in one deconvolution weight is seen."""
    from video_super_resolution_amd.sr import pack_dt_frags
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(S * 100 + h)
    x = E.ints(rs, (N, 32, h, w), -9, 9)
    up_w, up_b = E.sparse_weights(rs, (32, 32, k, k), 1.0, 3), E.ints(rs, (32,), -50, 50)
    dt_w, dt_b = E.sparse_weights(rs, (32, 32), 1.0, 2), E.ints(rs, (32,), -50, 50)
    dn_w, dn_b = E.sparse_weights(rs, (32, 32, k, k), 0.2, 1), E.ints(rs, (32,), -50, 50)
    hr = E.check_storable(E.prelu_ref(E.deconv_ref(x, up_w, up_b, stride=S, padding=2, store=torch.float32), 0.5), torch.float32, "hr")
    t = E.check_storable(E.prelu_ref(E.conv_ref(hr, dt_w.reshape(32, 32, 1, 1), dt_b, store=torch.float32), 0.25), torch.float32, "t")
    lr = E.check_storable(E.prelu_ref(E.conv_ref(t, dn_w, dn_b, stride=S, padding=2, store=torch.float32), 0.5), torch.float32, "lr")
    if S not in _master:
        _master[S] = fill_module_(SRProjectionModule(upscale_factor=S).eval(), seed=0, prefix="model.")
    m = copy.deepcopy(_master[S]).cuda().eval()
    f = lambda v: v.float().cuda().contiguous()
    upw, dnw = f(up_w.permute(2, 3, 0, 1)), f(dn_w.permute(2, 3, 1, 0))     # [ky][kx][in][out], as SRProjectionModule._packed lays them out
    dtw = torch.zeros((32, 96), dtype=torch.float32, device="cuda")
    dtw[:, 64:] = f(dt_w)
    lib = L.load()
    try:
        lib.vsr_sr_f32_variant(variant)
        got_hr = m._up(f(x), upw, f(up_b), 0.5, N, h, w)
        E.assert_exact(got_hr, hr, f"x{S} {shape} vsr_sr_deconv_f32 variant {variant}")
        got_t = m._c1([(got_hr.view(N, 32, -1), dtw, 64)], f(dt_b), 0.25, N, S * S * h * w).view(N, 32, S * h, S * w)
        E.assert_exact(got_t, t, f"x{S} {shape} vsr_sr_conv1x1_f32 variant {variant}")
        if variant == 0:      # (the fused 1x1 epilogue exists in the matrix-core build only)
            got_t2 = m._up(f(x), upw, f(up_b), 0.5, N, h, w, dt=(pack_dt_frags(dtw, 64), f(dt_b), 0.25))
            E.assert_exact(got_t2, t, f"x{S} {shape} vsr_sr_deconv_f32 + fused downtran")
        E.assert_exact(m._down(got_t, dnw, f(dn_b), 0.5, N, h, w), lr, f"x{S} {shape} vsr_sr_conv_f32 variant {variant}")
        # sensitivity: one unit in one deconvolution weight
        up2 = up_w.clone()
        up2[31, 4, k - 1, 0] += 1.0
        hr2 = E.prelu_ref(E.deconv_ref(x, up2, up_b, stride=S, padding=2, store=torch.float32), 0.5)
        got2 = m._up(f(x), f(up2.permute(2, 3, 0, 1)), f(up_b), 0.5, N, h, w)
        E.assert_exact(got2, hr2, "planted weight: the kernel follows its own weights")
        if bool((hr2 != hr).any()):
            with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
                E.assert_exact(got2, hr, "planted")
            assert torch.equal(E.diff_mask(got2, hr), hr2 != hr) and not bool((hr2 != hr)[:, [ch for ch in range(32) if ch != 4]].any())
    finally:
        lib.vsr_sr_f32_variant(0)
