"""The float64 numpy restatement of include/vsr_hip_metric.h: quantise, luma, shave, SSE (summed with math.fsum), and the separable
valid-window SSIM of Wang et al. 2004.  tests/test_metric_ref_helper.py pins it (against scipy, and against planted defects);
tests/test_gpu_metric.py compares the device with it.

Every function takes float32 RGB frames [F,H,W,3] (numpy) and follows the header's order: quantise, shave, channels.  The optional
`defect` arguments plant the mistakes the helper test must see; the device tests never pass them."""
import math

import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
TAPS = 11


def window(centre: float = 5.0) -> np.ndarray:
    """exp(-(i - 5)^2 / (2 * 1.5^2)) over its sum, 11 taps, float64 (`centre` other than 5: the window shifted, a planted defect)."""
    g = np.exp(-((np.arange(TAPS, dtype=np.float64) - centre) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def quantise(x: np.ndarray, truncate: bool = False) -> np.ndarray:
    """What write-out stores: negatives and NaN -> 0, above 255 -> 255, round half to even; float32 in, float32 out."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(x >= 0, x, np.float32(0))
        v = np.where(v > 255, np.float32(255), v)
    return (np.floor(v) if truncate else np.rint(v)).astype(np.float32)


def luma(rgb: np.ndarray, luma4) -> np.ndarray:
    """y = ((o + a0 R) + a1 G) + a2 B in double from the four float32 values {a0, a1, a2, o}."""
    a0, a1, a2, o = (np.float64(np.float32(v)) for v in luma4)
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    return ((o + a0 * r) + a1 * g) + a2 * b


def planes(x: np.ndarray, channels: str, quant: bool, shave: int, luma4=None, truncate: bool = False) -> np.ndarray:
    """float32 [F,H,W,3] -> float64 [F,P,h,w]: P = 3 ("rgb") or 1 ("y")."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 4 and x.shape[3] == 3
    if quant:
        x = quantise(x, truncate)
    if shave:
        x = x[:, shave:x.shape[1] - shave, shave:x.shape[2] - shave]
    if channels == "y":
        return luma(x, luma4)[:, None]
    assert channels == "rgb"
    return np.ascontiguousarray(np.moveaxis(x.astype(np.float64), 3, 1))


def sse(pa: np.ndarray, pb: np.ndarray):
    """One frame's planes [P,h,w] -> (the exactly rounded sum of the terms d * d, each rounded once in double; their number)."""
    d = pa - pb
    t = (d * d).reshape(-1)
    return math.fsum(t.tolist()), t.size


def _rows_then_columns(v: np.ndarray, win: np.ndarray) -> np.ndarray:
    """The valid 11 x 11 windowed sum of v [..., h, w], separably: along the rows first, then down the columns."""
    h, w = v.shape[-2:]
    r = np.zeros(v.shape[:-1] + (w - TAPS + 1,), dtype=np.float64)
    for k in range(TAPS):
        r = r + win[k] * v[..., :, k:k + w - TAPS + 1]
    c = np.zeros(v.shape[:-2] + (h - TAPS + 1, w - TAPS + 1), dtype=np.float64)
    for k in range(TAPS):
        c = c + win[k] * r[..., k:k + h - TAPS + 1, :]
    return c


def ssim_map(pa: np.ndarray, pb: np.ndarray, win=None) -> np.ndarray:
    """Planes [..., h, w] float64 -> the SSIM map [..., h - 10, w - 10], the formula as the header writes it."""
    win = window() if win is None else win
    ma, mb = _rows_then_columns(pa, win), _rows_then_columns(pb, win)
    eaa, ebb, eab = _rows_then_columns(pa * pa, win), _rows_then_columns(pb * pb, win), _rows_then_columns(pa * pb, win)
    maa, mbb, mab = ma * ma, mb * mb, ma * mb
    saa, sbb, sab = eaa - maa, ebb - mbb, eab - mab
    return ((2.0 * mab + C1) * (2.0 * sab + C2)) / (((maa + mbb) + C1) * ((saa + sbb) + C2))


def metrics(a: np.ndarray, b: np.ndarray, channels: str = "rgb", quant: bool = True, shave: int = 0, luma4=None, win=None,
            want_ssim: bool = True, truncate: bool = False) -> np.ndarray:
    """float32 [F,H,W,3] twice -> float64 [F,4] = {sse, n_sse, ssim_sum, n_ssim} per frame (the SSIM slots 0 without `want_ssim`)."""
    pa, pb = planes(a, channels, quant, shave, luma4, truncate), planes(b, channels, quant, shave, luma4, truncate)
    out = np.zeros((pa.shape[0], 4), dtype=np.float64)
    for f in range(pa.shape[0]):
        out[f, 0], out[f, 1] = sse(pa[f], pb[f])
        if want_ssim:
            m = ssim_map(pa[f], pb[f], win)
            out[f, 2], out[f, 3] = math.fsum(m.reshape(-1).tolist()), m.size
    return out


# ------------------------------------------------------------------------------------------------ test images (float32 [F,H,W,3])
def textured(rs, F, H, W):
    """A textured pair: smooth structure plus detail, and a degraded copy (blur-like mix and noise), values over 0..255 and beyond."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 70 * np.sin(xx / 3.1)[None, :, :, None] * np.cos(yy / 4.3)[None, :, :, None]
    a = base + rs.uniform(-60, 60, (F, H, W, 3))
    b = 0.9 * a + 0.1 * base + rs.normal(0, 6, (F, H, W, 3))
    return a.astype(np.float32), b.astype(np.float32)


def near_flat(rs, F, H, W):
    """The case float32 window sums cannot score: 255 everywhere against 255 - {0, 1}."""
    a = np.full((F, H, W, 3), 255, dtype=np.float32)
    b = (255 - rs.randint(0, 2, (F, H, W, 3))).astype(np.float32)
    return a, b


def gaussian(rs, F, H, W):
    """Gaussian floats (for quantise = 0): nothing integral, some values outside 0..255."""
    a = rs.normal(128, 60, (F, H, W, 3))
    b = a + rs.normal(0, 5, (F, H, W, 3))
    return a.astype(np.float32), b.astype(np.float32)


def awkward(rs, F, H, W, nan: bool = True):
    """What quantisation must handle: values below 0 and above 255, exact .5 ties on both parities, and (with `nan`) NaN."""
    a = rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)
    b = rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)
    for x in (a, b):
        flat = x.reshape(-1)
        idx = rs.permutation(flat.size)[:max(flat.size // 8, 12)]
        flat[idx] = rs.randint(0, 256, idx.size).astype(np.float32) + np.float32(0.5)     # ties: even and odd neighbours
        special = [-3.2, -0.0, 0.5, 1.5, 2.5, 253.5, 254.5, 255.5, 300.0] + ([float("nan")] * 3 if nan else [])
        flat[idx[:len(special)]] = special
    return a, b
