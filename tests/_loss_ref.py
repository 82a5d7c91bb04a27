"""The float64 numpy restatement of include/vsr_hip_loss.h: the mask by flat index, truncation and the low eight bits, the six SSEs
and the eight TV sums with math.fsum, the 14 sums and the 6 x 2 terms, and the NHWC-4 half frames.  tests/test_loss_ref_helper.py pins
it (against the reference's own masked arrays of fixture g10 and against loss.SR_loss on the CPU); tests/test_gpu_loss.py compares the
device with it.

outputs float32 [3,H,W,3] = O0, O1, O2; target float32 [H,W,3]; mask: 3*H*W values of any shape, nonzero = masked."""
import math

import numpy as np

# (a, b) of the six SSEs and the frame whose TV each SR_loss call takes, as indices into O0, O1, O2, T, mO0, mO1, mO2, mT
SSE_PAIRS = [(0, 3), (5, 7), (0, 1), (1, 2), (4, 5), (5, 6)]
TV_FRAMES = [0, 1, 4, 5]           # the h / w pairs of `sums`, from slot 6
TERM_TV = [0, 5, 0, 1, 4, 5]       # genSR, objSR, flow(0,1), flow(1,2), objflow(0,1), objflow(1,2)


def masked_frame(x: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """m(v) = mask[e] ? 0 : (float)((int)v & 255), element e of the frame against element e of the mask; float32 in and out.  For finite
    |v| < 2^63 (the device claims equality only below 2^31)."""
    x = np.asarray(x, dtype=np.float32)
    m = np.asarray(mask).reshape(-1) != 0
    assert m.size == x.size
    i = np.trunc(x.astype(np.float64)).astype(np.int64) & 255
    return np.where(m.reshape(x.shape), 0, i).astype(np.float32)


def frames8(outputs: np.ndarray, target: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """float32 [8,H,W,3] = O0, O1, O2, T, mO0, mO1, mO2, mT."""
    outputs = np.asarray(outputs, dtype=np.float32)
    H, W = outputs.shape[1:3]
    assert outputs.shape == (3, H, W, 3)
    plain = np.concatenate([outputs, np.asarray(target, dtype=np.float32).reshape(1, H, W, 3)])
    return np.concatenate([plain, np.stack([masked_frame(f, mask) for f in plain])])


def _fsum_sq(d: np.ndarray) -> float:
    return math.fsum((d * d).reshape(-1).tolist())   # every term rounded once in double, the sum exactly rounded


def sse(a: np.ndarray, b: np.ndarray) -> float:
    return _fsum_sq(a.astype(np.float64) - b.astype(np.float64))


def tv(a: np.ndarray):
    """-> (h, w): the sums over a[y+1] - a[y] and a[:,x+1] - a[:,x] of one [H,W,3] frame."""
    a = a.astype(np.float64)
    return _fsum_sq(a[1:] - a[:-1]), _fsum_sq(a[:, 1:] - a[:, :-1])


def sums14(f8: np.ndarray) -> np.ndarray:
    """float64 [14] = {sse[6], h / w of O0, O1, mO0, mO1}."""
    out = [sse(f8[a], f8[b]) for a, b in SSE_PAIRS]
    for k in TV_FRAMES:
        out += list(tv(f8[k]))
    return np.array(out, dtype=np.float64)


def terms_from_sums(s: np.ndarray, H: int, W: int) -> np.ndarray:
    """float32 [6,2] = {image, tv}: image = sse / (3 H W), tv = 2 (h / (3 (H-1) W) + w / (3 H (W-1))), in double, rounded once."""
    s = np.asarray(s, dtype=np.float64)
    n, count_h, count_w = np.float64(3 * H * W), np.float64(3 * (H - 1) * W), np.float64(3 * H * (W - 1))
    out = np.empty((6, 2), dtype=np.float32)
    for k in range(6):
        slot = 6 + 2 * TV_FRAMES.index(TERM_TV[k])
        out[k, 0] = np.float32(s[k] / n)
        out[k, 1] = np.float32(np.float64(2.0) * (s[slot] / count_h + s[slot + 1] / count_w))
    return out


def nhwc4(f8: np.ndarray) -> np.ndarray:
    """float16 [8,H,W,4]: every float rounded to half (ties to even, overflow to infinity), channel 3 = 0."""
    out = np.zeros(f8.shape[:3] + (4,), dtype=np.float16)
    with np.errstate(over="ignore"):
        out[..., :3] = f8.astype(np.float16)
    return out


def pixel_terms(outputs, target, mask):
    """-> (sums float64 [14], terms float32 [6,2], masked float32 [4,H,W,3], nhwc4 float16 [8,H,W,4])."""
    f8 = frames8(outputs, target, mask)
    H, W = f8.shape[1:3]
    s = sums14(f8)
    return s, terms_from_sums(s, H, W), f8[4:], nhwc4(f8)
