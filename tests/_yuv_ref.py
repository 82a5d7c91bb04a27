"""float64 numpy restatements of the 4:2:0 conversions of include/vsr_hip_yuv.h, for tests/test_gpu_yuv.py (and checked on the CPU
against hand-worked values by tests/test_yuv_ref_helper.py).  They take the float32 coefficients the kernel received, as float64."""
import numpy as np

FORMATS = ("yuv420p", "nv12", "yuv420p10le", "p010le")
SITINGS = ("left", "center")


def depth(fmt):
    return 10 if fmt in ("yuv420p10le", "p010le") else 8


def frame_bytes(fmt, H, W):
    return H * W * 3 // 2 * (2 if depth(fmt) == 10 else 1)


def pack(Y, Cb, Cr, fmt):
    """Code values (integer arrays Y [F,H,W], Cb / Cr [F,H/2,W/2]) -> uint8 [F, frame_bytes]."""
    F = Y.shape[0]
    if fmt in ("nv12", "p010le"):
        c = np.stack([Cb, Cr], axis=-1).reshape(F, -1)
    else:
        c = np.concatenate([Cb.reshape(F, -1), Cr.reshape(F, -1)], axis=1)
    s = np.concatenate([Y.reshape(F, -1), c], axis=1).astype(np.int64)
    if depth(fmt) == 8:
        return s.astype(np.uint8)
    if fmt == "p010le":
        s = s << 6
    return np.ascontiguousarray(s.astype("<u2")).view(np.uint8).reshape(F, -1)


def unpack(frames, fmt, H, W):
    """uint8 [F, frame_bytes] -> the code values (Y, Cb, Cr) as int64, after the mask (yuv420p10le) / the shift (p010le)."""
    F = frames.shape[0]
    s = np.ascontiguousarray(frames)
    if depth(fmt) == 10:
        s = s.view("<u2").astype(np.int64)
        s = (s >> 6) if fmt == "p010le" else (s & 0x3FF)
    else:
        s = s.astype(np.int64)
    Y = s[:, :H * W].reshape(F, H, W)
    c = s[:, H * W:]
    if fmt in ("nv12", "p010le"):
        c = c.reshape(F, H // 2, W // 2, 2)
        return Y, c[..., 0], c[..., 1]
    n = (H // 2) * (W // 2)
    return Y, c[:, :n].reshape(F, H // 2, W // 2), c[:, n:].reshape(F, H // 2, W // 2)


def _taps(n_luma, midway):
    """Per luma index: (i0, i1, w0) -- the two chroma samples (clamped) and the weight of the first."""
    i = np.arange(n_luma)
    k, odd, n = i // 2, (i % 2) == 1, n_luma // 2
    if midway:
        i0 = np.where(odd, k, np.maximum(k - 1, 0))
        i1 = np.where(odd, np.minimum(k + 1, n - 1), k)
        w0 = np.where(odd, 0.75, 0.25)
    else:
        i0 = k
        i1 = np.where(odd, np.minimum(k + 1, n - 1), k)
        w0 = np.where(odd, 0.5, 1.0)
    return i0, i1, w0


def upsample(c, siting):
    """Chroma plane [F,H/2,W/2] -> [F,H,W], float64: bilinear on the chroma grid with edge clamp."""
    c = c.astype(np.float64)
    H, W = 2 * c.shape[1], 2 * c.shape[2]
    i0, i1, w0 = _taps(H, True)
    v = w0[None, :, None] * c[:, i0] + (1 - w0)[None, :, None] * c[:, i1]
    j0, j1, u0 = _taps(W, siting == "center")
    return u0[None, None, :] * v[:, :, j0] + (1 - u0)[None, None, :] * v[:, :, j1]


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
    Y, Cb, Cr = Y.astype(np.float64), upsample(Cb, siting), upsample(Cr, siting)
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


def filtered(rgb, siting):
    """Clamped R'G'B' [F,H,W,3] float64 -> the chroma-site values [F,H/2,W/2,3]: the down-sampling filter before the matrix."""
    if siting == "center":
        return (rgb[:, 0::2, 0::2] + rgb[:, 0::2, 1::2] + rgb[:, 1::2, 0::2] + rgb[:, 1::2, 1::2]) / 4.0
    W = rgb.shape[2]
    c = np.arange(0, W, 2)
    rows = (rgb[:, :, np.maximum(c - 1, 0)] + 2.0 * rgb[:, :, c] + rgb[:, :, c + 1]) / 4.0
    return (rows[:, 0::2] + rows[:, 1::2]) / 2.0


def write_values(rgb, coef12, siting):
    """float32 R'G'B' [F,H,W,3] -> the real-valued (Y [F,H,W], Cb, Cr [F,H/2,W/2]) before rounding, float64."""
    k = np.asarray(coef12, dtype=np.float32).astype(np.float64)
    A, o = k[:9].reshape(3, 3), k[9:]
    x = rgb.astype(np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    x = np.clip(x, 0.0, 255.0)
    m = filtered(x, siting)
    return (nested(A, o, 0, x[..., 0], x[..., 1], x[..., 2]), nested(A, o, 1, m[..., 0], m[..., 1], m[..., 2]),
            nested(A, o, 2, m[..., 0], m[..., 1], m[..., 2]))


def quantise(v, fmt):
    return np.clip(np.rint(v), 0, 2 ** depth(fmt) - 1).astype(np.int64)   # np.rint: ties to even


def write(rgb, fmt, coef12, siting):
    """-> uint8 [F, frame_bytes]."""
    return pack(*(quantise(v, fmt) for v in write_values(rgb, coef12, siting)), fmt)
