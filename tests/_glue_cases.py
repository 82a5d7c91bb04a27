"""Cases and CPU references of tests/test_gpu_exact_glue.py, importable without a GPU: tests/test_exact_helper.py builds every one of them
and runs its reference, so that a case outside its budget fails there.

  A  the OSVOS head (k_osvos_fuse behind trunk_exec.osvos_fold / OSVOSExec.fuse_sides): integer operands, `E.osvos_head_ref`.
  C  FlowNet2's input normalisation (vsr_flownet_prepare_pairs): integer frames whose sums are exact in any order.
  D  upsample -> warp -> concat (vsr_flownet_up_warp_concat16_f16): dyadic flows and frames, oracle/native.py for the warp.

References are stock torch operators on the CPU and the project's C checker; none restates a kernel's index code."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _exact as E

# ---------------------------------------------------------------------------------------------------------------- A: OSVOS head
OSVOS_STRIDES = (2, 4, 8, 16)
# (h, w, ld, branches).  An odd and an even crop excess (hs + 1) s - h in every branch, both parities of the crop offset excess // 2 in
# branches 1..3 (branch 0's is 1 at every size), side maps of one pixel and of one row, h and w just above and just below a multiple of
# 16; 21 x 37: 777 pixels per image, 1554 in all (six full workgroups and a ragged seventh); 33 x 1: side maps of one column.
OSVOS_GEOMS = [(1, 1), (2, 3), (16, 32), (17, 33), (31, 18), (23, 47), (15, 49)]
OSVOS_CASES = [(h, w, ld, 4) for h, w in OSVOS_GEOMS for ld in (16, 32)] + [(21, 37, 32, 4), (33, 1, 16, 4), (17, 33, 16, 3), (18, 31, 32, 3)]


def gen_osvos(h, w, nb=4, N=2, seed=0):
    """Sides: integers in -8..8; upscale weights: DENSE integers in -2..2, not symmetric in (in, out); fuse row: integers in -2..2; an
    integer bias.  -> dict(sides [N,16,hs,ws] per branch, up_w, fuse_w [16 nb], bias, strides, hw)."""
    rs = np.random.RandomState(1000 * h + w + 7 * nb + seed)
    sizes = E.osvos_sizes(h, w, nb)
    c = dict(hw=(h, w), strides=list(OSVOS_STRIDES[:nb]), bias=float(rs.randint(-9, 10)),
             sides=[E.ints(rs, (N, 16, hs, ws), -8, 8) for hs, ws in sizes],
             up_w=[E.ints(rs, (16, 16, 2 * s, 2 * s), -2, 2) for s in OSVOS_STRIDES[:nb]], fuse_w=E.ints(rs, (16 * nb,), -2, 2))
    for b, u in enumerate(c["up_w"]):
        if torch.equal(u, u.transpose(0, 1)):
            raise E.BudgetError(f"upscale weight {b} is symmetric in (in, out): an in/out swap in the fold would go unseen")
    if N > 1 and all(torch.equal(s[0], s[1]) for s in c["sides"]):
        raise E.BudgetError("image 1 equals image 0")
    return c


def osvos_ref(c, dweff=None):
    h, w = c["hw"]
    return E.osvos_head_ref(c["sides"], c["up_w"], c["fuse_w"], c["bias"], c["hw"], dweff=dweff, live=h * w >= 256)


def osvos_side_nhwc(side, ld):
    """[N,16,hs,ws] float64 -> [N,hs,ws,ld] fp16 (CPU); channels 16 and up hold 7.0: a read beyond the 16 live ones changes the sum."""
    N, C, hs, ws = side.shape
    out = torch.full((N, hs, ws, ld), 7.0, dtype=torch.float16)
    out[..., :16] = E.check_storable(side, torch.float16, "side map").permute(0, 2, 3, 1).to(torch.float16)
    return out


# ---------------------------------------------------------------------------------------------------------------- C: prepare_pairs
# (frames F, frame h, w, value range, pairs, crop (y0, x0, H, W))
PAIRS_CASES = [
    (2, 20, 28, 255, [(1, 1)], (4, 4, 12, 16)),                                  # B = 1, a pair (i, i)
    (3, 20, 28, 255, [(2, 0), (0, 1)], (0, 4, 12, 16)),                          # B = 2, descending order; the crop touches the top
    (3, 20, 28, 255, [(0, 1), (1, 2), (2, 1)], (8, 4, 12, 16)),                  # B = 3, frame 1 in three pairs; ... the bottom
    (4, 20, 28, 255, [(3, 2), (2, 1), (1, 0), (1, 3)], (4, 0, 12, 16)),          # B = 4; ... the left border
    (3, 20, 28, 255, [(0, 2), (2, 2)], (4, 12, 12, 16)),                         # ... the right border
    (3, 70, 134, 255, [(0, 1), (1, 2)], (3, 3, 64, 128)),                        # 8192 pixels: every one of the 128 partial sums is live
    (2, 9, 11, 255, [(0, 1), (1, 0)], (5, 7, 4, 4)),                             # 4 x 4: all but one of the 128 partial sums are empty
    (2, 518, 1024, 15, [(1, 0)], (1, 2, 516, 1020)),                             # 526,320 pixels: above the cap of 2048 workgroups of 256
]


def gen_pairs(case):
    F_, h, w, vmax, pairs, crop = case
    rs = np.random.RandomState(h * 31 + w + len(pairs))
    return dict(frames=rs.randint(0, vmax + 1, (F_, h, w, 3)).astype(np.float32), pairs=list(pairs), crop=crop)


def pairs_ref(c):
    """models.py:74-79 behind a static crop: rgb_mean over both frames of a pair and all cropped pixels per colour, x = (inputs - rgb_mean)
    / 255.  The sum of both crops is an integer below 2^24 (checked), so float32 adds it without rounding in ANY order and the mean is ONE
    correctly rounded float32 division; the float64 mean cast to float32 is that value (the quotient of two integers below 2^24 rounds the
    same way through double).  Then two correctly rounded float32 operations per element, in numpy.
    -> dict(x [B,6,H,W] float32, x6h [B,H,W,32] fp16, both4 [2B,H,W,4] fp16), numpy."""
    fr, pairs, (y0, x0, H, W) = c["frames"], c["pairs"], c["crop"]
    if not np.array_equal(fr, np.round(fr)) or fr.min() < 0:
        raise E.BudgetError("prepare_pairs: frames must hold non-negative integers")
    if not (0 <= y0 and 0 <= x0 and y0 + H <= fr.shape[1] and x0 + W <= fr.shape[2]):
        raise E.BudgetError("prepare_pairs: the crop leaves the frame")
    crop = fr[:, y0:y0 + H, x0:x0 + W].astype(np.float64)
    B = len(pairs)
    x = np.zeros((B, 6, H, W), np.float32)
    for b, (i, j) in enumerate(pairs):
        total = crop[i].sum((0, 1)) + crop[j].sum((0, 1))
        if total.max() >= 2.0 ** 24:
            raise E.BudgetError(f"prepare_pairs: pair {b} sums to {total.max()}, not below 2^24: the float32 sum depends on its order")
        mean = (total / (2.0 * H * W)).astype(np.float32)                                  # [3]
        for k, f in enumerate((i, j)):
            v = (crop[f].astype(np.float32) - mean[None, None, :]) / np.float32(255.0)      # float32 throughout
            assert v.dtype == np.float32
            x[b, 3 * k:3 * k + 3] = v.transpose(2, 0, 1)
    xh = x.astype(np.float16)
    x6h = np.zeros((B, H, W, 32), np.float16)
    x6h[..., :6] = xh.transpose(0, 2, 3, 1)
    both4 = np.zeros((2 * B, H, W, 4), np.float16)
    both4[:B, ..., :3] = xh[:, :3].transpose(0, 2, 3, 1)
    both4[B:, ..., :3] = xh[:, 3:].transpose(0, 2, 3, 1)
    return dict(x=x, x6h=x6h, both4=both4)


# ---------------------------------------------------------------------------------------------------------------- D: up_warp_concat16
WARP_SHAPES = [(1, 4, 4), (2, 36, 200), (1, 132, 76), (1, 516, 1020)]
WARP_MUL = 20.0


def gen_warp(shape):
    """Quarter-resolution flows: multiples of 1/8 in -2..2 (fp16 values); frames: multiples of 1/16 in -2..2.  The flow's border cells
    point outwards by the full 2 (x 20 = 40 pixels), so targets leave the image on every side."""
    B, H, W = shape
    rs = np.random.RandomState(H * 7 + W)
    q = E.ints(rs, (B, 2, H // 4, W // 4), -16, 16, step=0.125)
    q[:, 0, :, 0], q[:, 0, :, -1] = -2.0, 2.0
    q[:, 1, 0, :], q[:, 1, -1, :] = -2.0, 2.0
    return dict(shape=shape, q=E.check_storable(q, torch.float16, "quarter-resolution flow"), x6=E.ints(rs, (B, 6, H, W), -32, 32, step=0.0625))


def warp_flow_ref(c, bilinear):
    """nn.Upsample(scale_factor=4) of the quarter-resolution flow times div_flow, in float64 on the CPU; the result must be a float32 value
    (weights of eighths on multiples of 1/8: nothing rounds).  -> [B,2,H,W] float32 numpy."""
    E._threads()
    up = F.interpolate(c["q"], scale_factor=4, mode="bilinear", align_corners=False) if bilinear else F.interpolate(c["q"], scale_factor=4, mode="nearest")
    flow = E.check_storable(up * WARP_MUL, torch.float32, "upsampled flow")
    if E.granularity(flow) < 2.0 ** -10 or float(flow.abs().max()) > 2 * WARP_MUL:
        raise E.BudgetError("upsampled flow: finer than 1/1024 or beyond 40 pixels: the kernel's float32 lerp may round")
    return flow.to(torch.float32).numpy()


def warp_leaves_every_side(flow, H, W):
    """(left, right, top, bottom): does a target x + u / y + v leave the image there?"""
    xs, ys = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    tx, ty = xs + flow[:, 0], ys + flow[:, 1]
    return bool((tx < 0).any()), bool((tx > W - 1).any()), bool((ty < 0).any()), bool((ty > H - 1).any())


@functools.lru_cache(maxsize=None)
def warp_ref(shape, bilinear):
    """The twelve live channels as tests/test_gpu_flow_ops.py::test_fused_warp_concat_and_norms_bit_exact composes them from the C checker
    (frames, frame b warped by the flow, flow / div_flow, |a - warped|), rounded once to fp16; channels 12..15 zero.
    -> (case, out16 [B,H,W,16] fp16 numpy).  Cached: shared by the builds and leading dimensions tested against it, never modified."""
    from oracle import native
    c = gen_warp(shape)
    flow = warp_flow_ref(c, bilinear)
    x6 = E.check_storable(c["x6"], torch.float16, "frames").to(torch.float32).numpy()
    warped = native.resample2d(x6[:, 3:], flow)
    ndiff = native.channelnorm(x6[:, :3] - warped)
    ref12 = np.concatenate([x6, warped, flow * np.float32(1.0 / WARP_MUL), ndiff], 1)
    assert ref12.dtype == np.float32
    B, H, W = shape
    out16 = np.zeros((B, H, W, 16), np.float16)
    out16[..., :12] = ref12.transpose(0, 2, 3, 1).astype(np.float16)
    out16.setflags(write=False)
    return c, out16


def flow_nhwc(q, ld):
    """[B,2,h4,w4] float64 -> [B,h4,w4,ld] fp16 (CPU), channels 2 and up (if any) hold 7.0."""
    B, _, h4, w4 = q.shape
    out = torch.full((B, h4, w4, ld), 7.0, dtype=torch.float16)
    out[..., :2] = q.permute(0, 2, 3, 1).to(torch.float16)
    return out
