"""The float64 numpy restatement of include/vsr_hip_msssim.h, on top of tests/_metric_ref.py's `planes` and `_rows_then_columns`: the
2 x 2 mean with the last row / column repeated, five levels, the contrast-structure and SSIM maps per level, and the combination of
Wang, Simoncelli and Bovik 2003.  tests/test_msssim_ref_helper.py pins it (against scipy, and against planted defects);
tests/test_gpu_msssim.py compares the device with it.

The `defect` arguments plant the mistakes the helper test must see; the device tests never pass them."""
import math

import numpy as np

import _metric_ref as R

LEVELS = 5
BETA = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIZE = 161


def level_sizes(h: int, w: int):
    out = []
    for _ in range(LEVELS):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def pool(p: np.ndarray, floor: bool = False) -> np.ndarray:
    """Planes [..., h, w] -> [..., ceil(h / 2), ceil(w / 2)]: ((p00 + p01) + (p10 + p11)) * 0.25, an odd size repeating its last row /
    column.  `floor` (a planted defect): the odd last row / column is dropped instead."""
    h, w = p.shape[-2:]
    if floor:
        p = p[..., :h - h % 2, :w - w % 2]
    else:
        if h % 2:
            p = np.concatenate([p, p[..., -1:, :]], axis=-2)
        if w % 2:
            p = np.concatenate([p, p[..., :, -1:]], axis=-1)
    return ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * 0.25


def maps(pa: np.ndarray, pb: np.ndarray, win=None, cs_with_c1: bool = False):
    """Planes [..., h, w] float64 -> (the cs map, the SSIM map), each [..., h - 10, w - 10], the formulas as the header writes them.
    `cs_with_c1` (a planted defect): C1 in the place of C2 in cs."""
    win = R.window() if win is None else win
    f = R._rows_then_columns
    ma, mb = f(pa, win), f(pb, win)
    eaa, ebb, eab = f(pa * pa, win), f(pb * pb, win), f(pa * pb, win)
    maa, mbb, mab = ma * ma, mb * mb, ma * mb
    saa, sbb, sab = eaa - maa, ebb - mbb, eab - mab
    c = R.C1 if cs_with_c1 else R.C2
    cs = (2.0 * sab + c) / ((saa + sbb) + c)
    ssim = ((2.0 * mab + R.C1) * (2.0 * sab + R.C2)) / (((maa + mbb) + R.C1) * ((saa + sbb) + R.C2))
    return cs, ssim


def sums(a: np.ndarray, b: np.ndarray, channels: str = "rgb", quant: bool = True, shave: int = 0, luma4=None, win=None,
         floor: bool = False, cs_with_c1: bool = False) -> np.ndarray:
    """float32 [F,H,W,3] twice -> float64 [F,P,5,2] = {cs_sum, ssim_sum} per frame, plane and level (each summed with math.fsum)."""
    pa, pb = R.planes(a, channels, quant, shave, luma4), R.planes(b, channels, quant, shave, luma4)
    F, P = pa.shape[:2]
    out = np.zeros((F, P, LEVELS, 2), dtype=np.float64)
    for j in range(LEVELS):
        cs, ssim = maps(pa, pb, win, cs_with_c1)
        for f in range(F):
            for p in range(P):
                out[f, p, j, 0] = math.fsum(cs[f, p].reshape(-1).tolist())
                out[f, p, j, 1] = math.fsum(ssim[f, p].reshape(-1).tolist())
        if j + 1 < LEVELS:
            pa, pb = pool(pa, floor), pool(pb, floor)
    return out


def counts(h: int, w: int, floor: bool = False) -> np.ndarray:
    """n_j = (h_j - 10) (w_j - 10) of the five levels of a plane of h x w."""
    if floor:
        sizes = [(h >> j, w >> j) for j in range(LEVELS)]
    else:
        sizes = level_sizes(h, w)
    return np.array([(hj - 10) * (wj - 10) for hj, wj in sizes], dtype=np.float64)


def means(s: np.ndarray, h: int, w: int, floor: bool = False) -> np.ndarray:
    """Sums [F,P,5,2] -> the level means [F,P,5,2]."""
    return s / counts(h, w, floor)[None, None, :, None]


def combine(s: np.ndarray, h: int, w: int, beta=BETA, pooled_channels: bool = False, floor: bool = False) -> np.ndarray:
    """Sums [F,P,5,2] -> MS-SSIM [F]: per plane prod_{j<5} max(mcs_j, 0)^beta_j * max(mssim_5, 0)^beta_5, then the mean over planes.
    `pooled_channels` (a planted defect): the level means are averaged over the planes first, then combined once."""
    m = means(np.asarray(s, dtype=np.float64), h, w, floor)
    if pooled_channels:
        m = m.mean(axis=1, keepdims=True)
    terms = np.concatenate([m[:, :, :-1, 0], m[:, :, -1:, 1]], axis=2)
    return np.prod(np.maximum(terms, 0.0) ** np.asarray(beta, dtype=np.float64), axis=2).mean(axis=1)
