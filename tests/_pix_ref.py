"""float64 numpy restatements of the 4:2:2 / 4:4:4 conversions of include/vsr_hip_pix.h, for tests/test_gpu_pix.py (pinned on the CPU to
tests/_yuv_ref.py by tests/test_pix_ref_helper.py).  The interface of _yuv_ref.py; they take the float32 coefficients the kernel
received, as float64."""
import numpy as np

FORMATS = ("yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le")
SITINGS = ("left", "center")


def depth(fmt):
    return 10 if fmt.endswith("10le") else 8


def is422(fmt):
    return "422" in fmt


def chroma_width(fmt, W):
    return W // 2 if is422(fmt) else W


def frame_bytes(fmt, H, W):
    return (H * W + 2 * H * chroma_width(fmt, W)) * (2 if depth(fmt) == 10 else 1)


def pack(Y, Cb, Cr, fmt):
    """Code values (integer arrays Y [F,H,W], Cb / Cr [F,H,Wc]) -> uint8 [F, frame_bytes]."""
    F = Y.shape[0]
    s = np.concatenate([Y.reshape(F, -1), Cb.reshape(F, -1), Cr.reshape(F, -1)], axis=1).astype(np.int64)
    if depth(fmt) == 8:
        return s.astype(np.uint8)
    return np.ascontiguousarray(s.astype("<u2")).view(np.uint8).reshape(F, -1)


def unpack(frames, fmt, H, W):
    """uint8 [F, frame_bytes] -> the code values (Y, Cb, Cr) as int64, after the mask of the 10-bit formats."""
    F = frames.shape[0]
    s = np.ascontiguousarray(frames)
    s = (s.view("<u2").astype(np.int64) & 0x3FF) if depth(fmt) == 10 else s.astype(np.int64)
    Wc = chroma_width(fmt, W)
    n = H * Wc
    return s[:, :H * W].reshape(F, H, W), s[:, H * W:H * W + n].reshape(F, H, Wc), s[:, H * W + n:].reshape(F, H, Wc)


def upsample(c, siting, fmt):
    """Chroma plane [F,H,Wc] -> [F,H,W], float64.  4:4:4: the samples; 4:2:2: along the row only, with x the luma column, k = x // 2 and
    the indices clamped -- LEFT: even c[k], odd (c[k] + c[k+1]) / 2; CENTER: even c[k-1] / 4 + 3 c[k] / 4, odd 3 c[k] / 4 + c[k+1] / 4."""
    c = c.astype(np.float64)
    if not is422(fmt):
        return c
    Wc = c.shape[2]
    x = np.arange(2 * Wc)
    k, odd = x // 2, (x % 2) == 1
    before, after = np.maximum(k - 1, 0), np.minimum(k + 1, Wc - 1)
    if siting == "left":
        return np.where(odd, 0.5 * c[:, :, k] + 0.5 * c[:, :, after], c[:, :, k])
    return np.where(odd, 0.75 * c[:, :, k] + 0.25 * c[:, :, after], 0.25 * c[:, :, before] + 0.75 * c[:, :, k])


def aten_nearest_index(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def nested(A, o, c, x0, x1, x2):
    """fma(A[c][2], x2, fma(A[c][1], x1, fma(A[c][0], x0, o[c]))) without its roundings."""
    return A[c, 2] * x2 + (A[c, 1] * x1 + (A[c, 0] * x0 + o[c]))


def ingest(frames, fmt, coef12, siting, H, W, h=None, w=None):
    """-> (lr [F,h,w,3], hr [F,H,W,3], the largest partial sum's magnitude), float64."""
    k = np.asarray(coef12, dtype=np.float32).astype(np.float64)
    A, o = k[:9].reshape(3, 3), k[9:]
    Y, Cb, Cr = unpack(frames, fmt, H, W)
    Y, Cb, Cr = Y.astype(np.float64), upsample(Cb, siting, fmt), upsample(Cr, siting, fmt)
    big = 0.0
    out = []
    for c in range(3):
        s1 = A[c, 0] * Y + o[c]
        s2 = A[c, 1] * Cb + s1
        s3 = A[c, 2] * Cr + s2
        big = max(big, np.abs(s1).max(), np.abs(s2).max(), np.abs(s3).max())
        out.append(np.clip(s3, 0.0, 255.0))
    hr = np.stack(out, axis=-1)
    h, w = (H if h is None else h), (W if w is None else w)
    lr = hr[:, aten_nearest_index(H, h)][:, :, aten_nearest_index(W, w)]
    return lr, hr, big


def filtered(rgb, siting, fmt):
    """Clamped R'G'B' [F,H,W,3] float64 -> the chroma-site values [F,H,Wc,3]: the down-sampling filter before the matrix."""
    if not is422(fmt):
        return rgb
    if siting == "center":
        return (rgb[:, :, 0::2] + rgb[:, :, 1::2]) / 2.0
    c = np.arange(0, rgb.shape[2], 2)
    return ((rgb[:, :, np.maximum(c - 1, 0)] + rgb[:, :, c + 1]) + 2.0 * rgb[:, :, c]) / 4.0


def write_values(rgb, coef12, siting, fmt):
    """float32 R'G'B' [F,H,W,3] -> the real-valued (Y [F,H,W], Cb, Cr [F,H,Wc]) before rounding, float64."""
    k = np.asarray(coef12, dtype=np.float32).astype(np.float64)
    A, o = k[:9].reshape(3, 3), k[9:]
    x = rgb.astype(np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    x = np.clip(x, 0.0, 255.0)
    m = filtered(x, siting, fmt)
    return (nested(A, o, 0, x[..., 0], x[..., 1], x[..., 2]), nested(A, o, 1, m[..., 0], m[..., 1], m[..., 2]),
            nested(A, o, 2, m[..., 0], m[..., 1], m[..., 2]))


def quantise(v, fmt):
    return np.clip(np.rint(v), 0, 2 ** depth(fmt) - 1).astype(np.int64)   # np.rint: ties to even


def write(rgb, fmt, coef12, siting):
    """-> uint8 [F, frame_bytes]."""
    return pack(*(quantise(v, fmt) for v in write_values(rgb, coef12, siting, fmt)), fmt)


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_pix.py
# (F, H, W, scale) -- which branch of csrc/clip_pix.hip each reaches is listed in that file's docstring
SHAPES_BOTH = [(2, 6, 10, 2), (1, 14, 518, 2), (3, 18, 26, 4), (1, 34, 46, 3), (2, 6, 12, 2), (2, 4, 16, 2), (2, 6, 8, 2), (1, 2, 2064, 2),
               (3, 3, 6, 2), (2, 3, 8, 2)]
SHAPES_444 = [(2, 5, 7, 2), (1, 1, 1, 1), (3, 1, 3, 1)]
WRITE_EXTRA = [(2, 38, 42)]
SPECIAL = [-3.2, 0.0, 255.0, 255.49, 300.0, float("nan")]


def shapes(fmt):
    return SHAPES_BOTH + ([] if is422(fmt) else SHAPES_444)


def write_shapes(fmt):
    return [(F, H, W) for F, H, W, _ in shapes(fmt)] + WRITE_EXTRA


def write_case(F, H, W):
    """The RGB clip of the real-coefficient write-out test for one shape: uniform in -20..280 with the special values planted, as
    tests/test_gpu_yuv.py plants them (the first six floats) where the clip has 64 pixels or more.  That makes pixel 0 (0, 0, 255) after
    the clamp, whose 4:4:4 Cb under a full-range matrix is 128 + 255 / 2, a tie: one sample of a case, which only a case of 50 samples
    or more may hold under the 2 % cap.  Smaller clips get the values in the R channel of their first pixels instead, as many as fit."""
    rs = np.random.RandomState(H * 7 + W)
    rgb = rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)
    flat = rgb.reshape(-1)
    if F * H * W >= 64:
        flat[:len(SPECIAL)] = SPECIAL
    else:
        n = min(len(SPECIAL), F * H * W)
        flat[0:3 * n:3] = SPECIAL[:n]
    return rgb


def near_tie(v, eps):
    return np.abs(v - np.floor(v) - 0.5) < eps
