"""The glue between the trunk convolutions, bit for bit against references that do not run on the GPU: the OSVOS head (k_osvos_fuse behind
trunk_exec.osvos_fold / OSVOSExec.fuse_sides), the hourglass's resize-add (vsr_resize_add_segs_nhwc_f16 through igemm.resize_add) and
FlowNet2's frame glue of csrc/flow_ops.hip (prepare_pairs, up_warp_concat16 in both modes and both builds, fusion_input, assemble_planes,
resize_estimate).

References: float64 stock torch operators on the CPU (`E.osvos_head_ref`), the project's C checker oracle/native.py for the warps, and for
pure data movement the float32 CPU `F.interpolate` (`E.nearest_resize_ref`).  Operands are integers or dyadic fractions inside the budgets
tests/_exact.py and tests/_glue_cases.py check (tests/test_exact_helper.py runs every case's reference without a GPU), or, where the kernel
only moves values and adds two of them, arbitrary Gaussian fp16 values with the one correctly rounded operation restated.  There is no
tolerance in this file.

Sizes: every flow_ops kernel walks its pixels in a grid-stride loop capped at 2048 workgroups of 256 = 524,288 pixels; 516 x 1020 =
526,320 is the smallest map with sides that are multiples of 4 beyond it, so the loop's second trip runs under a comparison."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _exact as E
import _glue_cases as G
from test_gpu_poisoned_buffers import RESIZE_ADD_CASES

pytestmark = pytest.mark.gpu

from oracle import native  # noqa: E402
from video_super_resolution_amd import _lib as L, igemm  # noqa: E402
from video_super_resolution_amd.trunk_exec import OSVOSExec, osvos_fold  # noqa: E402

BIG = (516, 1020)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want, what, names="nyxc"):
    """Equality of bits for arbitrary values (no budget to check): both tensors of one dtype."""
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    E.assert_exact(got, want, what, names=names)


# ---------------------------------------------------------------------------------------------------------------- A: OSVOS head
def _head(c, weff=None):
    """An OSVOSExec holding only what `fuse_sides` reads, its folded weights from the product's own `osvos_fold` on the device."""
    ex = OSVOSExec.__new__(OSVOSExec)
    ex.up_s = list(c["strides"])
    ex.weff = weff if weff is not None else osvos_fold([u.float().cuda() for u in c["up_w"]], c["fuse_w"].float().cuda())
    ex.fuse_b = c["bias"]
    return ex


def _run_head(c, ld, weff=None, sides=None):
    h, w = c["hw"]
    dev = [G.osvos_side_nhwc(s, ld).cuda() for s in (sides or c["sides"])]
    out = _head(c, weff).fuse_sides(dev, h, w)
    assert out.dtype == torch.float32 and tuple(out.shape) == (dev[0].shape[0], 1, h, w)
    return out.cpu()


@pytest.mark.parametrize("case", G.OSVOS_CASES)
def test_osvos_head_equals_the_float64_composition(case):
    """Four (or three) transposed convolutions k = 2s / stride s, centre crops, concat and the 64 -> 1 fuse as stock float64 operators
    against the one launch on folded weights: integer operands, every sum exact in any order.  Side maps come from the ceil-mode halving
    chain; the sizes take an odd and an even crop excess in every branch (both parities of the offset where it can vary), one-row and
    one-column side maps, h and w either side of a multiple of 16, a ragged last workgroup; channels 16.. of an ld = 32 side map hold 7.0."""
    h, w, ld, nb = case
    c = G.gen_osvos(h, w, nb)
    E.assert_exact(_run_head(c, ld), G.osvos_ref(c), f"OSVOS head {case}")


def test_osvos_head_one_unit_in_one_folded_weight_moves_exactly_its_pixels():
    """Branch 3 (s = 16), tap (13, 20), input channel 5, + 1 on the device side only: the result equals the reference carrying the same
    term, and differs from the unperturbed reference exactly where that term is non-zero (one output phase of the branch)."""
    h, w, ld = 23, 47, 32
    c = G.gen_osvos(h, w)
    ref = G.osvos_ref(c)
    d = torch.zeros((16, 1, 32, 32), dtype=torch.float64)
    d[5, 0, 13, 20] = 1.0
    ref_p = G.osvos_ref(c, dweff=[None, None, None, d])
    predicted = ref_p != ref
    n = int(predicted.sum())
    assert 0 < n < predicted.numel(), n
    weff = osvos_fold([u.float().cuda() for u in c["up_w"]], c["fuse_w"].float().cuda())
    weff[3][13, 20, 5] += 1.0
    got = _run_head(c, ld, weff=weff)
    E.assert_exact(got, ref_p, "OSVOS head, one folded weight + 1")
    assert torch.equal(E.diff_mask(got, ref), predicted), (int(E.diff_mask(got, ref).sum()), n, E.bbox(E.diff_mask(got, ref)), E.bbox(predicted))
    print(f"[OSVOS head] one unit in weff[3][13][20][5]: {n} of {predicted.numel()} pixels move, inside {E.bbox(predicted)}")


def test_osvos_head_one_unit_in_one_side_value_at_a_map_corner():
    """Image 1, branch 0, channel 3, the bottom-right corner of the side map, + 1 on both sides: the result follows, and differs from the
    unperturbed one exactly on the reference's footprint (the corner's taps inside the crop, image 1 only)."""
    h, w, ld = 17, 33, 16
    c = G.gen_osvos(h, w)
    ref = G.osvos_ref(c)
    sides = [s.clone() for s in c["sides"]]
    sides[0][1, 3, -1, -1] += 1.0
    cp = dict(c, sides=sides)
    ref_p = G.osvos_ref(cp)
    predicted = ref_p != ref
    n = int(predicted.sum())
    assert 0 < n < predicted.numel() and not bool(predicted[0].any()), n
    got = _run_head(cp, ld)
    E.assert_exact(got, ref_p, "OSVOS head, one side value + 1")
    assert torch.equal(E.diff_mask(got, ref), predicted), (int(E.diff_mask(got, ref).sum()), n, E.bbox(E.diff_mask(got, ref)), E.bbox(predicted))
    print(f"[OSVOS head] one unit in side 0 at its corner: {n} of {predicted.numel()} pixels move, inside {E.bbox(predicted)}")


# ---------------------------------------------------------------------------------------------------------------- B: resize_add
def _ra(N, Ha, Wa, H, W, c, a_nseg, b_nseg, up2, b_up2):
    return (N, Ha, Wa, H, W, c, a_nseg, b_nseg, up2, b_up2)


# (N, Ha, Wa, H, W, c, segments of a, segments of b (0: no addend), up2, b_up2)
RA_CASES = [_ra(N, Ha, Wa, H, W, c, na, 1 if with_b else 0, up2, b_up2) for N, Ha, Wa, H, W, c, na, with_b, up2, b_up2 in RESIZE_ADD_CASES] + [
    _ra(1, 13, 9, 5, 4, 32, 2, 1, False, False),        # downsizing rows and columns
    _ra(2, 7, 9, 7, 9, 16, 1, 1, False, False),         # the identity size
    _ra(1, 7, 9, 7, 9, 16, 2, 0, False, False),
    _ra(1, 5, 6, 11, 13, 64, 4, 2, False, False),       # segment counts of a and b independently
    _ra(1, 5, 6, 11, 13, 64, 1, 4, False, False),
    _ra(1, 5, 6, 11, 13, 64, 2, 1, False, False),
    _ra(1, 5, 6, 11, 13, 64, 4, 4, False, False),
    _ra(1, 5, 6, 11, 13, 64, 1, 2, False, False),
    _ra(1, 5, 6, 10, 12, 64, 2, 4, True, True),
    _ra(3, 6, 5, 13, 11, 32, 2, 2, False, False),       # N = 3
    _ra(3, 4, 5, 16, 22, 16, 1, 1, True, True),
]
# sizes at which ATen's float32 index floor(dst * float(in / out)) differs from the rational floor(dst * in / out) at some row / column
RA_FLOAT_CASES = [
    _ra(1, 26, 14, 22, 46, 16, 1, 1, False, False),
    _ra(2, 21, 26, 69, 22, 32, 2, 2, False, False),
    _ra(1, 14, 21, 46, 69, 16, 2, 0, False, False),
    _ra(1, 13, 7, 22, 46, 32, 4, 1, True, False),       # up2: the resize indexes the doubled map, 26 -> 22 and 14 -> 46
    _ra(2, 13, 7, 22, 46, 16, 1, 2, True, True),
]


def _segments(rs, N, h, w, c, nseg, pads):
    """`nseg` tensors [N,h,w,left + c / nseg + right] of Gaussian fp16 values, the live slice of each at its own offset: a wrong `coff` or
    `ld` reads the extra channels.  -> [(tensor, coff)], the live channels concatenated [N,c,h,w]."""
    cs = c // nseg
    segs = []
    for i in range(nseg):
        left, right = pads[i % len(pads)]
        segs.append((torch.from_numpy(rs.randn(N, h, w, left + cs + right).astype(np.float16)), left))
    live = torch.cat([t[..., co:co + cs] for t, co in segs], 3).permute(0, 3, 1, 2).contiguous()
    return segs, live


def _resize_add_case(case):
    N, Ha, Wa, H, W, c, a_nseg, b_nseg, up2, b_up2 = case
    rs = np.random.RandomState(Ha * 131 + W * 7 + c + a_nseg + 5 * b_nseg)
    a_segs, a_live = _segments(rs, N, Ha, Wa, c, a_nseg, [(8, 8), (16, 8), (8, 0), (24, 16)])
    up = nn.UpsamplingNearest2d(scale_factor=2)
    src = up(a_live.float()).half() if up2 else a_live
    want = E.nearest_resize_ref(src, (H, W))
    assert want.dtype == torch.float16 and tuple(want.shape) == (N, c, H, W)
    b_segs = None
    if b_nseg:
        hb, wb = (H // 2, W // 2) if b_up2 else (H, W)
        b_segs, b_live = _segments(rs, N, hb, wb, c, b_nseg, [(16, 8), (8, 16), (0, 8), (8, 8)])
        addend = up(b_live.float()).half() if b_up2 else b_live
        # ONE correctly rounded fp16 add: the exact sum in float64, rounded once (numpy converts float64 -> float16 directly)
        want = torch.from_numpy((want.numpy().astype(np.float64) + addend.numpy().astype(np.float64)).astype(np.float16))

    def operand(segs):
        dev = [(t.cuda(), co) for t, co in segs]
        return (igemm.SegMap(dev), 0) if len(dev) > 1 else dev[0]

    a_op, a_coff = operand(a_segs)
    b_op, b_coff = operand(b_segs) if b_segs else (None, 0)
    got = igemm.resize_add(a_op, a_coff, c, (H, W), b_op, b_coff, up2=up2, b_up2=b_up2)
    assert tuple(got.shape) == (N, H, W, c) and got.dtype == torch.float16
    _bits_equal(got.cpu(), want.permute(0, 2, 3, 1).contiguous(), f"resize_add {case}")


@pytest.mark.parametrize("case", RA_CASES)
def test_resize_add_equals_interpolate_and_one_fp16_add(case):
    """AddResized / UpsamplingNearest2d in one pass against F.interpolate(size) in float32 on the CPU (a move) and one correctly rounded
    fp16 add; `up2` is the interpolation of the materialised UpsamplingNearest2d(2)(a), `b_up2` the materialised UpsamplingNearest2d(2)(b).
    Every segment tensor has spare channels either side of its live slice."""
    _resize_add_case(case)


@pytest.mark.parametrize("case", RA_FLOAT_CASES)
def test_resize_add_where_the_float_index_is_not_the_rational_one(case):
    """The same at sizes where float32 `floor(dst * (in / out))` and the integer `dst * in // out` name different source rows or columns
    (asserted: the case cannot lose its point): a kernel indexing in integers, or in double, fails here."""
    N, Ha, Wa, H, W, c, a_nseg, b_nseg, up2, b_up2 = case
    assert E.nearest_differs_from_rational(Ha << up2, H) or E.nearest_differs_from_rational(Wa << up2, W), case
    _resize_add_case(case)


# ---------------------------------------------------------------------------------------------------------------- C: prepare_pairs
@pytest.mark.parametrize("case", G.PAIRS_CASES, ids=lambda c: f"F{c[0]}-{c[1]}x{c[2]}-B{len(c[4])}-crop{'x'.join(map(str, c[5]))}")
def test_prepare_pairs_bit_exact(case):
    """x = (frames - rgb_mean) / 255 for pairs picked from a frame stack behind a crop: integer frames whose sums are exact in any order,
    so `x` is held bit for bit (a mean and two float32 operations per element), `x6h` / `both4` are its fp16 rounding and their padding
    channels exactly zero.  B = 1..4, a pair (i, i), descending pairs, a frame used twice, crops on each border of a larger frame, a
    4 x 4 crop, and 516 x 1020 where the normalising loop takes a second trip."""
    c = G.gen_pairs(case)
    ref = G.pairs_ref(c)
    Fn, h, w, _ = c["frames"].shape
    y0, x0, H, W = c["crop"]
    B = len(c["pairs"])
    frames = _cuda(c["frames"])
    x = torch.full((B, 6, H, W), float("nan"), device="cuda")
    x6h = torch.full((B, H, W, 32), 7.0, dtype=torch.float16, device="cuda")
    both4 = torch.full((2 * B, H, W, 4), 7.0, dtype=torch.float16, device="cuda")
    ws = torch.full((B * 128 * 3,), float("nan"), device="cuda")
    ia = (ctypes.c_int * B)(*[p[0] for p in c["pairs"]])
    ib = (ctypes.c_int * B)(*[p[1] for p in c["pairs"]])
    L.check(L.load().vsr_flownet_prepare_pairs(L.dptr(frames), Fn, h, w, ia, ib, B, y0, x0, H, W, L.dptr(ws), L.dptr(x), L.dptr(x6h, torch.float16),
                                               L.dptr(both4, torch.float16), L.stream()), "prepare_pairs")
    _bits_equal(x.cpu(), torch.from_numpy(ref["x"]), f"prepare_pairs x {case[:4]}", names="bcyx")
    _bits_equal(x6h.cpu(), torch.from_numpy(ref["x6h"]), "prepare_pairs x6h", names="byxc")
    _bits_equal(both4.cpu(), torch.from_numpy(ref["both4"]), "prepare_pairs both4", names="byxc")
    assert not x6h[..., 6:].any() and not both4[..., 3].any()


# ---------------------------------------------------------------------------------------------------------------- D: up_warp_concat16
@pytest.mark.xcheck
@pytest.mark.parametrize("bilinear", [1, 0])
@pytest.mark.parametrize("shape", G.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_up_warp_concat16_bit_exact(shape, bilinear):
    """Upsample x4 (bilinear or nearest) x div_flow -> warp frame b -> concat, both builds (gathers, LDS-staged tile) and ld = 32 / 2,
    against F.interpolate in float64 on the CPU (dyadic flows: the result is a float32 value, checked) and the C checker's resample2d /
    channelnorm, rounded once to fp16.  Two float32 steps are restated, not derived: channels 9 and 10 are float32(flow) * float32(1 / 20)
    (the kernel multiplies by the reciprocal it is given), and the square root inside channelnorm is float32 `sqrtf` on both sides.
    Border cells of the flow point 40 pixels outwards, so the warp clamps on every side."""
    B, H, W = shape
    c, want = G.warp_ref(shape, bilinear)
    if H >= 8 and W >= 8:
        assert all(G.warp_leaves_every_side(G.warp_flow_ref(c, bilinear), H, W))
    x6 = _cuda(c["x6"].to(torch.float32).numpy())
    want = torch.from_numpy(want.copy())   # (the cached reference itself stays read-only)
    lib = L.load()
    try:
        for variant in (1, 0):
            L.check(lib.vsr_flownet_warp_variant(variant))
            for ld in (32, 2):
                f2 = G.flow_nhwc(c["q"], ld).cuda()
                out16 = torch.full((B, H, W, 16), 7.0, dtype=torch.float16, device="cuda")
                L.check(lib.vsr_flownet_up_warp_concat16_f16(L.dptr(x6), L.dptr(f2, torch.float16), ld, bilinear, L.cf(G.WARP_MUL), L.cf(1 / G.WARP_MUL),
                                                             L.dptr(out16, torch.float16), B, H, W, L.stream()), "up_warp_concat16")
                _bits_equal(out16.cpu(), want, f"up_warp_concat16 {shape} bilinear {bilinear} variant {variant} ld {ld}", names="byxc")
    finally:
        lib.vsr_flownet_warp_variant(1)


# ---------------------------------------------------------------------------------------------------------------- E: the remaining glue
def _up4_nearest(t):
    """[B,h4,w4,ld] fp16 (CPU) -> channels 0, 1 upsampled x4 (nearest) [B,2,H,W] float32 numpy: a move."""
    return F.interpolate(t[..., :2].permute(0, 3, 1, 2).float(), scale_factor=4, mode="nearest").numpy()


@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 36, 200), (1,) + BIG], ids=lambda s: "x".join(map(str, s)))
def test_fusion_input_bit_exact(shape):
    """The fusion network's input (models.py:106-125) against its composition from the C checker: the two nearest-upsampled flows
    (FlowNetSD / div_flow, FlowNetS #2 x div_flow: one float32 operation each), their norms, the two brightness errors of the warps.
    Gaussian operands (the warps restate the reference's arithmetic: equality is required as it is of resample2d itself); the two flow maps
    have different leading dimensions, their spare channels hold 7.0."""
    B, H, W = shape
    rs = np.random.RandomState(H + W)
    x = (rs.randn(B, 6, H, W) * 0.3).astype(np.float32)
    ld_sd, ld_s2 = 32, 8
    g2 = torch.full((B, H // 4, W // 4, ld_sd), 7.0, dtype=torch.float16)
    g2[..., :2] = torch.from_numpy((rs.randn(B, H // 4, W // 4, 2) * 30).astype(np.float16))
    f2 = torch.full((B, H // 4, W // 4, ld_s2), 7.0, dtype=torch.float16)
    f2[..., :2] = torch.from_numpy((rs.randn(B, H // 4, W // 4, 2) * 0.4).astype(np.float16))
    fsd = _up4_nearest(g2) / np.float32(20.0)
    fs2 = _up4_nearest(f2) * np.float32(20.0)
    assert fsd.dtype == fs2.dtype == np.float32
    parts = [x[:, :3], fsd, fs2, native.channelnorm(fsd), native.channelnorm(fs2)]
    parts += [native.channelnorm(x[:, :3] - native.resample2d(x[:, 3:], fl)) for fl in (fsd, fs2)]
    want = np.zeros((B, H, W, 32), np.float16)
    want[..., :11] = np.concatenate(parts, 1).transpose(0, 2, 3, 1).astype(np.float16)
    out32 = torch.full((B, H, W, 32), 7.0, dtype=torch.float16, device="cuda")
    dx, dg2, df2 = _cuda(x), g2.cuda(), f2.cuda()
    L.check(L.load().vsr_flownet_fusion_input_f16(L.dptr(dx), L.dptr(dg2, torch.float16), ld_sd, L.dptr(df2, torch.float16), ld_s2,
                                                  L.cf(20.0), L.dptr(out32, torch.float16), B, H, W, L.stream()), "fusion_input")
    _bits_equal(out32.cpu(), torch.from_numpy(want), f"fusion_input {shape}", names="byxc")


# (h, w, Hc, Wc, Hp, Wp): output size, size of the flow pictures, size of the previous output
PLANES_CASES = [
    (66, 70, 64, 64, 264, 280),          # the case of tests/test_gpu_flow_ops.py
    (22, 46, 26, 14, 26, 14),            # float32 index != rational index (26 -> 22, 14 -> 46): Hc > h, Wc < w
    (69, 22, 21, 26, 21, 26),            # ... 21 -> 69, 26 -> 22: Hc < h, Wc > w
    (1, 9, 5, 3, 4, 36),                 # one row
    (7, 1, 3, 4, 28, 1),                 # one column
    (12, 20, 12, 20, 12, 20),            # the identity size
    BIG + (128, 240, 1032, 510),         # 526,320 pixels: the grid-stride loops take a second trip
]


@pytest.mark.parametrize("first_call", [True, False])
@pytest.mark.parametrize("case", PLANES_CASES, ids=lambda c: "-".join(map(str, c)))
def test_plane_assembly_and_estimate_resize_equal_the_stock_expressions(case, first_call):
    """video_super_resolution.py:33-40 / :57-62 as stock operators on the CPU (float32 `interpolate`: moves; (a + b) / 2: one rounding)
    against vsr_assemble_planes_f32 and vsr_resize_estimate_f32, over non-square sizes, one row, one column, pictures larger and smaller
    than the frame, sizes where the float32 nearest index is not the rational one, and a map beyond the capped grid."""
    from video_super_resolution_amd.vsr import VSR, maskprocess
    h, w, Hc, Wc, Hp, Wp = case
    if (Hc, h) in ((26, 22), (21, 69)):
        assert E.nearest_differs_from_rational(Hc, h) and E.nearest_differs_from_rational(Wc, w) and E.nearest_differs_from_rational(Hp, h)
    rs = np.random.RandomState(h * 3 + w + Hc)
    d = torch.from_numpy(rs.randint(0, 256, (3, h, w, 3)).astype(np.float32))
    pics = torch.from_numpy(rs.randint(0, 256, (2, Hc, Wc, 3)).astype(np.float32))
    z = [torch.from_numpy(rs.randn(1, 1, h, w).astype(np.float32)) for _ in range(3)]
    frames = d.permute(0, 3, 1, 2)
    depth = torch.stack([maskprocess(torch.squeeze(torch.mean(torch.stack([z[0], z[1]]), 0)[0]).reshape(h, w)),
                         maskprocess(torch.squeeze(torch.mean(torch.stack([z[1], z[2]]), 0)[0]).reshape(h, w))])
    fl = F.interpolate(pics.permute(0, 3, 1, 2), (h, w))
    dz = [t.cuda() for t in z]
    if first_call:
        want = torch.cat((frames, fl, depth, frames[0:1]), 0)
        got = VSR._assemble(d.cuda(), pics.cuda(), dz)
    else:
        prev = torch.from_numpy(rs.randint(0, 256, (1, Hp, Wp, 3)).astype(np.float32))
        est = torch.full((3, h, w), float("nan"), device="cuda")
        est_hw3 = torch.full((h, w, 3), float("nan"), device="cuda")
        dprev = prev.cuda()
        L.check(L.load().vsr_resize_estimate_f32(L.dptr(dprev), Hp, Wp, L.dptr(est), L.dptr(est_hw3), h, w, L.stream()), "resize_estimate")
        want_est = F.interpolate(prev.permute(0, 3, 1, 2), (h, w))[0]
        _bits_equal(est.cpu(), want_est.contiguous(), f"resize_estimate {case} (planes)", names="cyx")
        _bits_equal(est_hw3.cpu(), want_est.permute(1, 2, 0).contiguous(), f"resize_estimate {case} (frame)", names="yxc")
        mask = (torch.from_numpy(rs.rand(h, w).astype(np.float32)) > 0.5).float()
        masked = torch.where(maskprocess(mask) != 0, torch.zeros_like(want_est), want_est).unsqueeze(0)
        want = torch.cat((frames, fl, depth, masked), 0)
        got = VSR._assemble(d.cuda(), pics.cuda(), dz, est, mask.cuda())
    _bits_equal(got.cpu(), want.contiguous(), f"assemble_planes {case} first_call {first_call}", names="pcyx")
