"""CPU references of FlowNet2's three native operators and of their gradients (csrc/flow_ops.hip, csrc/flow_ops_bwd.hip), for
tests/test_gpu_exact_flow.py.  numpy / torch float64, no GPU; tests/test_flow_ref_helper.py checks every reference here before it judges
a kernel.

Two kinds of restatement:
  * `ref_resample2d`, `ref_channelnorm`, `ref_correlation`: the three forwards as differentiable torch expressions (stock autograd gives
    their gradients).  tests/test_gpu_flow_ops_grad.py compares the kernels with them on Gaussian operands within a range-relative bar.
  * `resample2d_grads_ref`, `correlation_ref`, `correlation_grads_ref`, `channelnorm_grad_ref`: the FORMULAS as include/vsr_hip.h and
    include/vsr_hip_grad.h write them, evaluated directly (no autograd), every sum in float64, each checking the budget inside which a float32
    kernel must equal it bit for bit: for every destination element sum |term| < 2^24 g, g the granularity of the terms (`_exact.py`).  A
    case outside its budget raises `_exact.BudgetError` naming the destination coordinate.

The exact regime of Resample2d: integer images and incoming gradients, flows `integer + k/8`.  Then x + flow is a float32 value, alpha and
beta are multiples of 1/8, the four weights multiples of 1/64, every product and every partial sum of the image gradient's scatter and of
the flow gradient's channel sum a float32 value: the order of the atomic adds cannot matter and an FMA contraction cannot either
(flow_ops_bwd.hip is built with contraction allowed, so on Gaussian operands its bits are not restatable).  k = 4 puts the nearest build's
`xf + 0.5` exactly on an integer.  The correlation's regime: integer features and gradients; its one rounding, the multiplication of the
exact sum by float32(1) / float32(C), is restated in float32, so any C is exact, not only powers of two.  ChannelNorm's gradient has no
sum: three correctly rounded float32 operations per element, restated in numpy float32 on arbitrary operands.

What these cases cannot see is what `_exact.py` says: rounding behaviour (the Gaussian-operand tests keep covering it) and overflow."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _exact as E

GRID_CAP = 2048 * 256   # pixels per batch item that one pass of a capped thread-per-pixel kernel covers (grid_for of both .hip files)


# ----------------------------------------------------------------------------------------------------------------------
# restatements (differentiable by stock autograd)
# ----------------------------------------------------------------------------------------------------------------------
def ref_resample2d(img, flow, bilinear=True):
    B, C, H, W = img.shape
    f32 = flow.to(torch.float32)
    xf32 = torch.arange(W, device=img.device, dtype=torch.float32).view(1, 1, W) + f32[:, 0]
    yf32 = torch.arange(H, device=img.device, dtype=torch.float32).view(1, H, 1) + f32[:, 1]
    bi = torch.arange(B, device=img.device).view(B, 1, 1, 1)
    ci = torch.arange(C, device=img.device).view(1, C, 1, 1)

    def at(yy, xx):
        return img[bi, ci, yy.unsqueeze(1), xx.unsqueeze(1)]

    if not bilinear:
        xN = (xf32 + 0.5).floor().clamp(0, W - 1).long()
        yN = (yf32 + 0.5).floor().clamp(0, H - 1).long()
        return at(yN, xN)
    xf, yf = xf32.to(img.dtype), yf32.to(img.dtype)
    fx, fy = xf.floor(), yf.floor()
    a, b = (xf - fx).unsqueeze(1), (yf - fy).unsqueeze(1)
    xL, xR = fx.clamp(0, W - 1).long(), (fx + 1).clamp(0, W - 1).long()
    yT, yB = fy.clamp(0, H - 1).long(), (fy + 1).clamp(0, H - 1).long()
    return (1 - a) * (1 - b) * at(yT, xL) + a * (1 - b) * at(yT, xR) + (1 - a) * b * at(yB, xL) + a * b * at(yB, xR)


def ref_channelnorm(x):
    return (x * x).sum(1, keepdim=True).sqrt()


def ref_correlation(f1, f2, pad, md, s1, s2):
    """zero-pad -> shift -> multiply -> mean over channels -> stack, displacement index tj-major."""
    B, C, H, W = f1.shape
    R = md // s2
    p1, p2 = F.pad(f1, (pad,) * 4), F.pad(f2, (pad,) * 4)
    OH, OW = -(-(H + 2 * pad - 2 * md) // s1), -(-(W + 2 * pad - 2 * md) // s1)
    a = p1[:, :, md:md + (OH - 1) * s1 + 1:s1, md:md + (OW - 1) * s1 + 1:s1]
    outs = []
    for tj in range(-R, R + 1):
        for ti in range(-R, R + 1):
            y0, x0 = md + tj * s2, md + ti * s2
            outs.append((a * p2[:, :, y0:y0 + (OH - 1) * s1 + 1:s1, x0:x0 + (OW - 1) * s1 + 1:s1]).mean(1))
    return torch.stack(outs, 1)


FLOWNETC = dict(pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2)

GEOMS = [((1, 256, 48, 64), dict(pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2)),   # FlowNetC
         ((2, 5, 20, 70), dict(pad_size=4, kernel_size=1, max_displacement=4, stride1=2, stride2=2)),
         ((1, 40, 33, 47), dict(pad_size=3, kernel_size=1, max_displacement=3, stride1=2, stride2=1)),
         ((2, 33, 19, 37), dict(pad_size=2, kernel_size=1, max_displacement=4, stride1=1, stride2=2)),     # pad < max_disp
         ((1, 6, 9, 41), dict(pad_size=6, kernel_size=1, max_displacement=2, stride1=3, stride2=1)),       # pad > max_disp
         # window rows of 1, 5 and 15 pieces of 32 columns (FlowNetC's: 3): no displacement; D = 31; the widest the LDS admits
         ((2, 7, 11, 45), dict(pad_size=0, kernel_size=1, max_displacement=0, stride1=1, stride2=1)),
         ((1, 3, 20, 70), dict(pad_size=60, kernel_size=1, max_displacement=60, stride1=1, stride2=4)),
         ((1, 2, 12, 500), dict(pad_size=210, kernel_size=1, max_displacement=210, stride1=1, stride2=14))]


# ----------------------------------------------------------------------------------------------------------------------
# small tools
# ----------------------------------------------------------------------------------------------------------------------
def _np(t, dtype=np.float64):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


def _t64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def _budget(abs_sum, gran, what):
    E.check_sum_budget(torch.as_tensor(abs_sum, dtype=torch.float64), gran, what)


def assert_exact_by_trip(got, want, what, names="ncyx", per_thread=1):
    """`_exact.assert_exact` for [.., H, W] maps; where the map is large enough that a thread of a capped kernel takes a second element
    (H * W / per_thread > GRID_CAP; per_thread: pixels per thread, 4 for the 16-byte builds) the failure also says on which trip of the
    grid-stride loop the differing pixels lie: whether the first one's linear index y * W + x is at or beyond the cap, and the count
    of differing pixels on either side."""
    got = got.detach().cpu()
    want = torch.as_tensor(want)
    try:
        E.assert_exact(got, want, what, names=names)
    except AssertionError as e:
        hw = got.shape[-2] * got.shape[-1]
        if hw // per_thread <= GRID_CAP:
            raise
        m = E.diff_mask(got, want).reshape(-1, hw)
        lin = torch.nonzero(m.any(0)).flatten()
        first, n1, n2 = int(lin[0]), int((lin // per_thread < GRID_CAP).sum()), int((lin // per_thread >= GRID_CAP).sum())
        raise AssertionError(f"{e}; first differing pixel at linear index {first}: {'AT OR BEYOND' if first // per_thread >= GRID_CAP else 'below'} "
                             f"the grid cap ({GRID_CAP * per_thread} pixels per trip); differing pixels on the first trip {n1}, on the second {n2}") from None


def sat_int32(v):
    """float -> int32 as a SATURATING conversion with NaN -> 0 (what the device's v_cvt_i32_f32 does and the kernels' comments rely on;
    a plain C cast of 1e9 + x or 3e10 is undefined).  -> int64 array holding int32 values."""
    v = np.asarray(v, dtype=np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(np.trunc(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------------
# Resample2d: include/vsr_hip_grad.h, the comment of vsr_grad_resample2d_f32
# ----------------------------------------------------------------------------------------------------------------------
def resample2d_taps(flow, H, W, bilinear=True):
    """The sampling geometry of every output pixel: xf = x + flow[b,0,y,x], yf = y + flow[b,1,y,x] formed in FLOAT32 as the kernels form
    them (so both pick the same cell where the sum rounds onto an integer), alpha = xf - floor(xf) and beta (exact in float32), then
    float64; the four indices converted with `sat_int32` and clamped independently.  Nearest: floor(xf + 0.5), the addition in float32.
    -> dict of [B,H,W] arrays: bilinear alpha, beta, xL, xR, yT, yB (and fx, fy: the unclamped floors); nearest xN, yN."""
    f = _np(flow, np.float32)
    xf = np.arange(W, dtype=np.float32).reshape(1, 1, W) + f[:, 0]
    yf = np.arange(H, dtype=np.float32).reshape(1, H, 1) + f[:, 1]
    assert xf.dtype == np.float32 and yf.dtype == np.float32
    if not bilinear:
        half = np.float32(0.5)
        return dict(xN=np.clip(sat_int32(np.floor(xf + half)), 0, W - 1), yN=np.clip(sat_int32(np.floor(yf + half)), 0, H - 1))
    fx, fy = np.floor(xf), np.floor(yf)
    alpha, beta = (xf - fx).astype(np.float64), (yf - fy).astype(np.float64)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    return dict(alpha=alpha, beta=beta, fx=fx, fy=fy,
                xL=np.clip(sat_int32(fx), 0, W - 1), xR=np.clip(sat_int32(fx + 1.0), 0, W - 1),
                yT=np.clip(sat_int32(fy), 0, H - 1), yB=np.clip(sat_int32(fy + 1.0), 0, H - 1))


def resample2d_grads_ref(img, flow, gout, bilinear=True, check=True, _plant=None):
    """d_img [B,C,H,W] and d_flow [B,2,H,W] of out = resample2d(img, flow) for the incoming gradient gout, float64 tensors:
      d_img  += gout[b,c,y,x] * {(1-alpha)(1-beta), alpha(1-beta), (1-alpha)beta, alpha beta} at (yT,xL), (yT,xR), (yB,xL), (yB,xR)
      d_flow[b,0,y,x] = sum_c gout * ((1-beta)(I[yT,xR]-I[yT,xL]) + beta (I[yB,xR]-I[yB,xL]))
      d_flow[b,1,y,x] = sum_c gout * ((1-alpha)(I[yB,xL]-I[yT,xL]) + alpha(I[yB,xR]-I[yT,xR]))
    nearest: d_img is the scatter of gout to the one rounded pixel, d_flow is zero.  The scatter is one np.bincount in float64.
    `check`: the float32 budgets -- for the scatter PER DESTINATION PIXEL (at a border many samples clamp onto one pixel: that is summed,
    not assumed), for the flow gradient per pixel over the channels; granularity = that of gout x weights (x img).
    `_plant` (tests/test_flow_ref_helper.py only) makes a defective COPY: "drop_tap" leaves the (yB, xR) tap out of the scatter,
    "drop_clamp" leaves out the upper clamp of xR: samples whose right column lies beyond the image vanish instead of landing on column W-1."""
    img, gout = _np(img), _np(gout)
    B, C, H, W = img.shape
    hw = H * W
    assert gout.shape == img.shape and tuple(np.shape(flow)) == (B, 2, H, W)
    t = resample2d_taps(flow, H, W, bilinear)
    plane = (np.arange(B * C, dtype=np.int64) * hw).reshape(B, C, 1, 1)
    if bilinear:
        a, b = t["alpha"], t["beta"]
        taps = [(t["yT"], t["xL"], (1 - a) * (1 - b)), (t["yT"], t["xR"], a * (1 - b)),
                (t["yB"], t["xL"], (1 - a) * b), (t["yB"], t["xR"], a * b)]
        if _plant == "drop_tap":
            taps = taps[:3]
        elif _plant == "drop_clamp":
            keep = (t["fx"] + 1.0 <= W - 1).astype(np.float64)
            taps[1] = (taps[1][0], taps[1][1], taps[1][2] * keep)
            taps[3] = (taps[3][0], taps[3][1], taps[3][2] * keep)
        else:
            assert _plant is None
    else:
        assert _plant is None
        taps = [(t["yN"], t["xN"], np.ones((B, H, W)))]
    idx = np.concatenate([(plane + (yy * W + xx)[:, None]).ravel() for yy, xx, _ in taps])
    wgt = np.concatenate([(gout * w[:, None]).ravel() for _, _, w in taps])
    d_img = np.bincount(idx, weights=wgt, minlength=B * C * hw).reshape(B, C, H, W)
    g_w = E.granularity(*[torch.from_numpy(w) for _, _, w in taps]) if check else None
    if check:
        mag = np.bincount(idx, weights=np.abs(wgt), minlength=B * C * hw).reshape(B, C, H, W)
        _budget(mag, E.granularity(torch.from_numpy(gout)) * g_w, f"resample2d d_img scatter ({'bilinear' if bilinear else 'nearest'})")
    d_flow = np.zeros((B, 2, H, W))
    if bilinear:
        bi, ci = np.arange(B).reshape(B, 1, 1, 1), np.arange(C).reshape(1, C, 1, 1)
        at = lambda yy, xx: img[bi, ci, yy[:, None], xx[:, None]]   # noqa: E731
        i00, i01, i10, i11 = at(t["yT"], t["xL"]), at(t["yT"], t["xR"]), at(t["yB"], t["xL"]), at(t["yB"], t["xR"])
        a, b = t["alpha"][:, None], t["beta"][:, None]
        d_flow[:, 0] = (gout * ((1 - b) * (i01 - i00) + b * (i11 - i10))).sum(1)
        d_flow[:, 1] = (gout * ((1 - a) * (i10 - i00) + a * (i11 - i01))).sum(1)
        if check:
            g = E.granularity(torch.from_numpy(gout)) * E.granularity(torch.from_numpy(img)) * E.granularity(torch.from_numpy(a), torch.from_numpy(b))
            i00, i01, i10, i11 = np.abs(i00), np.abs(i01), np.abs(i10), np.abs(i11)
            mx = (np.abs(gout) * ((1 - b) * (i01 + i00) + b * (i11 + i10))).sum(1)
            my = (np.abs(gout) * ((1 - a) * (i10 + i00) + a * (i11 + i01))).sum(1)
            _budget(np.stack([mx, my], 1), g, "resample2d d_flow channel sum")
    return torch.from_numpy(d_img), torch.from_numpy(d_flow)


def border_hits(flow, H, W):
    """How many samples clamp at each of the four borders (the LEFT / TOP index below 0, the RIGHT / BOTTOM index beyond the last), how many
    clamp on neither side of an axis, and how many on no side at all.  -> dict of counts plus n (the number of samples)."""
    t = resample2d_taps(flow, H, W)
    left, right = t["fx"] < 0, t["fx"] + 1 > W - 1
    top, bottom = t["fy"] < 0, t["fy"] + 1 > H - 1
    in_x, in_y = ~left & ~right, ~top & ~bottom
    return dict(left=int(left.sum()), right=int(right.sum()), top=int(top.sum()), bottom=int(bottom.sum()), in_x=int(in_x.sum()),
                in_y=int(in_y.sum()), interior=int((in_x & in_y).sum()), n=int(left.size))


FAR = (1e9, -1e9, 3e10)   # flows far outside: x + 1e9 rounds in float32, 3e10 is beyond int32 (the conversion saturates)


def resample_case(seed, shape, mag=None, far=False):
    """Exact operands of a Resample2d gradient: img integers in [-3, 3], gout integers in [-2, 2], flow = whole + k/8 with whole in
    [-m, m - 1] per axis (m = `mag`, or a third of the axis but at least 2: a known share of the samples, about m / 4n per side, clamps at
    each border) and k in 0..7, k = 4 guaranteed.  `far`: three flows far outside the image on top, as tests/test_gpu_flow_ops.py places
    them.  On every axis of 3 pixels or more, samples clamped at the low border, at the high border and at neither are asserted to occur
    (a one-pixel axis has no interior: every sample clamps there), and with both axes that long, samples that clamp nowhere.
    -> dict(img, gout [B,C,H,W] float64, flow [B,2,H,W] float32, hits)."""
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    img = rs.randint(-3, 4, size=shape).astype(np.float64)
    gout = rs.randint(-2, 3, size=shape).astype(np.float64)
    mx, my = (mag, mag) if mag else (max(2, W // 3), max(2, H // 3))
    whole = np.stack([rs.randint(-mx, mx, size=(B, H, W)), rs.randint(-my, my, size=(B, H, W))], 1)
    k = rs.randint(0, 8, size=(B, 2, H, W))
    k.flat[0] = 4
    flow = (whole + k / 8.0).astype(np.float32)
    assert np.array_equal(flow.astype(np.float64), whole + k / 8.0) and float(np.abs(flow).max()) <= max(mx, my)
    hits = border_hits(flow, H, W)   # of the near flows: the far ones are placed on top
    if far:
        flow[0, 0, 0, 0] = FAR[0]
        flow[0, 1, -1, -1] = FAR[1]
        flow[-1, 0, -1, 0] = FAR[2]
    assert (k == 4).any()
    if W >= 3:
        assert hits["left"] > 0 and hits["right"] > 0 and hits["in_x"] > 0, hits
    if H >= 3:
        assert hits["top"] > 0 and hits["bottom"] > 0 and hits["in_y"] > 0, hits
    if W >= 3 and H >= 3:
        assert hits["interior"] > 0, hits
    return dict(img=img, gout=gout, flow=flow, hits=hits)


# ----------------------------------------------------------------------------------------------------------------------
# ChannelNorm: d_in = gout * in / (out + 1e-9)
# ----------------------------------------------------------------------------------------------------------------------
def channelnorm_grad_ref(x, out, gout):
    """(gout * x) * (float32(1) / (out + float32(1e-9))): an addition, a division and two multiplications per element, each a correctly
    rounded float32 operation of numpy.  x [B,C,H,W], out and gout [B,1,H,W] -> float32 tensor [B,C,H,W].  A pixel whose channels are
    all zero has out = 0, a finite reciprocal and gradient 0."""
    x, out, gout = _np(x, np.float32), _np(out, np.float32), _np(gout, np.float32)
    r = np.float32(1.0) / (out + np.float32(1e-9))
    d = (gout * x) * r
    assert d.dtype == np.float32 and r.dtype == np.float32
    return torch.from_numpy(d)


# ----------------------------------------------------------------------------------------------------------------------
# Correlation: include/vsr_hip.h (forward) and include/vsr_hip_grad.h (the two gradients), kernel_size 1
# ----------------------------------------------------------------------------------------------------------------------
def corr_geometry(H, W, geom):
    """-> pad, md, s1, s2, R, D, OH, OW (vsr_correlation_out_shape)."""
    assert geom["kernel_size"] == 1
    pad, md, s1, s2 = geom["pad_size"], geom["max_displacement"], geom["stride1"], geom["stride2"]
    R = md // s2
    OH, OW = -(-(H + 2 * pad - 2 * md) // s1), -(-(W + 2 * pad - 2 * md) // s1)
    assert OH > 0 and OW > 0
    return pad, md, s1, s2, R, 2 * R + 1, OH, OW


def window_pieces(geom):
    """NP of launch_correlation_bwd: 32-column pieces of a window row, ceil((32 + 2 R stride2) / 32)."""
    R = geom["max_displacement"] // geom["stride2"]
    return (32 + 2 * R * geom["stride2"] + 31) // 32


def forward_lds_bytes(geom):
    """The forward's LDS need (vsr_correlation_f32 refuses beyond 64 KiB): 32 channels x (32 + window) floats."""
    R = geom["max_displacement"] // geom["stride2"]
    return 4 * 32 * (32 + 31 * geom["stride1"] + 2 * R * geom["stride2"] + 1)


def scale_inv_c(sums, C, what):
    """The kernels' one rounding: the exact sum (a float32 value by the budget, checked) times float32(1) / float32(C), in float32."""
    s32 = E.check_storable(sums, torch.float32, what).to(torch.float32).numpy()
    inv = np.float32(1.0) / np.float32(C)
    out = s32 * inv
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def _sl(o, n, s):
    return slice(o, o + (n - 1) * s + 1, s)


def correlation_sums_ref(f1, f2, geom, check=True):
    """sum_c f1[b,c,y1,x1] * f2[b,c,y1+tj*s2,x1+ti*s2] in float64 (zero outside the image), [B,D*D,OH,OW], channel (tj+R)*D + ti+R, with
    (y1, x1) = (oy, ox) * stride1 + max_displacement - pad_size.  In padded coordinates (pad_size zeros on every side) the f1 position is
    (oy, ox) * s1 + md and every displaced position stays inside the padded map.  Budget per output pixel: (sum_c |f1|) * max |f2|, an
    upper bound of sum |terms| for every displacement."""
    E._threads()
    f1, f2 = _t64(f1), _t64(f2)
    B, C, H, W = f1.shape
    pad, md, s1, s2, R, D, OH, OW = corr_geometry(H, W, geom)
    p1, p2 = F.pad(f1, (pad,) * 4), F.pad(f2, (pad,) * 4)
    a = p1[:, :, _sl(md, OH, s1), _sl(md, OW, s1)]
    if check:
        _budget(a.abs().sum(1, keepdim=True) * float(f2.abs().max()), E.granularity(f1) * E.granularity(f2), "correlation forward")
    out = torch.empty((B, D * D, OH, OW), dtype=torch.float64)
    for tj in range(-R, R + 1):
        for ti in range(-R, R + 1):
            out[:, (tj + R) * D + ti + R] = (a * p2[:, :, _sl(md + tj * s2, OH, s1), _sl(md + ti * s2, OW, s1)]).sum(1)
    return out


def correlation_ref(f1, f2, geom):
    """The float32 correlation of exact operands: float64 sums, then the one float32 multiplication.  -> float32 tensor."""
    return scale_inv_c(correlation_sums_ref(f1, f2, geom), f1.shape[1], "correlation sum")


def correlation_grad_sums_ref(f1, f2, gout, geom, check=True):
    """The two gradient sums before the 1 / C, float64 [B,C,H,W] each:
      d_f1[b,c,y1,x1] = sum_{tj,ti} gout[b,k,oy,ox] * f2[b,c,y1+tj*s2,x1+ti*s2]
      d_f2[b,c,y2,x2] = sum_{tj,ti} gout[b,k,oy',ox'] * f1[b,c,y2-tj*s2,x2-ti*s2], (oy', ox') the output pixel of that f1 position
    accumulated per displacement on zero-padded maps (inside one displacement no destination repeats) and cropped: what falls on the
    padding is a position outside the image and has no gradient.  Budgets per destination pixel, an upper bound for every channel:
    (sum of |gout| over the elements that reach the pixel) * max |other map|."""
    E._threads()
    f1, f2, gout = _t64(f1), _t64(f2), _t64(gout)
    B, C, H, W = f1.shape
    pad, md, s1, s2, R, D, OH, OW = corr_geometry(H, W, geom)
    assert tuple(gout.shape) == (B, D * D, OH, OW)
    p1, p2 = F.pad(f1, (pad,) * 4), F.pad(f2, (pad,) * 4)
    d1, d2 = torch.zeros_like(p1), torch.zeros_like(p2)
    m2 = torch.zeros((B, 1) + tuple(p1.shape[2:]), dtype=torch.float64)
    ys, xs = _sl(md, OH, s1), _sl(md, OW, s1)
    a = p1[:, :, ys, xs]
    for tj in range(-R, R + 1):
        for ti in range(-R, R + 1):
            g = gout[:, (tj + R) * D + ti + R].unsqueeze(1)
            yd, xd = _sl(md + tj * s2, OH, s1), _sl(md + ti * s2, OW, s1)
            d1[:, :, ys, xs] += g * p2[:, :, yd, xd]
            d2[:, :, yd, xd] += g * a
            m2[:, :, yd, xd] += g.abs()
    crop = lambda t: t[:, :, pad:pad + H, pad:pad + W].contiguous()   # noqa: E731
    if check:
        gran = E.granularity(f1) * E.granularity(f2) * E.granularity(gout)
        m1 = torch.zeros_like(m2)
        m1[:, :, ys, xs] = gout.abs().sum(1, keepdim=True)
        _budget(crop(m1) * float(f2.abs().max()), gran, "correlation d_f1")
        _budget(crop(m2) * float(f1.abs().max()), gran, "correlation d_f2")
    return crop(d1), crop(d2)


def correlation_grads_ref(f1, f2, gout, geom):
    """-> (d_f1, d_f2), float32 tensors: the float64 sums, each times float32(1) / float32(C) in float32."""
    s1, s2 = correlation_grad_sums_ref(f1, f2, gout, geom)
    C = f1.shape[1]
    return scale_inv_c(s1, C, "correlation d_f1 sum"), scale_inv_c(s2, C, "correlation d_f2 sum")


# every geometry the gradient test runs, FlowNetC's on a small map with all 256 channels, and one geometry for each of three window-piece
# counts (NP of launch_correlation_bwd) no other test builds: 4, 8 and 14 (the others here: 3, 2, 2, 2, 2, 1, 5, 15)
CORR_CASES = list(GEOMS) + [
    ((1, 256, 8, 16), FLOWNETC),
    ((2, 40, 9, 70), dict(pad_size=40, kernel_size=1, max_displacement=40, stride1=1, stride2=4)),      # NP 4: 32 + 80 columns, D = 21
    ((1, 33, 6, 45), dict(pad_size=105, kernel_size=1, max_displacement=105, stride1=2, stride2=7)),   # NP 8: 32 + 210, D = 31
    ((1, 1, 5, 37), dict(pad_size=195, kernel_size=1, max_displacement=195, stride1=1, stride2=13)),  # NP 14: 32 + 390, D = 31
]


def corr_id(case):
    shape, g = case
    return "x".join(map(str, shape)) + f"-p{g['pad_size']}m{g['max_displacement']}s{g['stride1']}{g['stride2']}"


@functools.lru_cache(maxsize=None)
def corr_case(i):
    """Case i of CORR_CASES with its references, computed once and shared (treat as read-only): f1, f2 integers in [-3, 3], gout integers
    in [-2, 2] (float64 tensors), out / d_f1 / d_f2 the float32 references."""
    shape, geom = CORR_CASES[i]
    rs = np.random.RandomState(1000 + i)
    f1, f2 = E.ints(rs, shape), E.ints(rs, shape)
    out = correlation_ref(f1, f2, geom)
    gout = E.ints(rs, tuple(out.shape), -2, 2)
    d_f1, d_f2 = correlation_grads_ref(f1, f2, gout, geom)
    return dict(shape=shape, geom=geom, f1=f1, f2=f2, gout=gout, out=out, d_f1=d_f1, d_f2=d_f2)
