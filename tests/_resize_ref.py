"""float64 restatement of the table-driven resampler (include/vsr_hip_resize.h, driver.resize_tables) for the device tests.

  * `tables64` / `tables`: the antialiased filter tables of one axis, restated output by output from the definition (Pillow's convention,
    Keys' cubic with a = -0.5 or the triangle), independently of driver.py: float64, and rounded to float32 as the device gets them.
  * `resize64`: the two passes in float64 from any tables (float32-rounded real ones, or the exact tests' dyadic ones), index clamp
    included, and per element the rounding bound of the two float32 fma chains the library evaluates.
  * `quantise64`: rint(clip(v, 0, 255)), ties to even, NaN to 0: step 3 of the header.
  * `exact_case`: tables and pixels inside the budget of tests/_exact.py, on which float32 cannot round.

The bound is derived, not measured.  With u = 2^-24 and gamma_n = n u / (1 - n u), a chain t = fma(w_k, x_k, t) of n terms from t = 0
returns sum w_k x_k (1 + theta_k) with |theta_k| <= gamma_n.  Row pass: |t^ - t| <= gamma_KX A, A = sum_j |wx_j x_j|, so |t^| <= (1 +
gamma_KX) A.  Column pass over the computed t^: |s^ - s| <= gamma_KY sum_k |wy_k| |t^_k| + sum_k |wy_k| |t^_k - t_k|
  <= gamma_KY sum_k |wy_k| A_k + (1 + gamma_KY) gamma_KX sum_k |wy_k| A_k,
formed here from the absolute sums in float64.  (The float64 evaluation's own rounding is nine orders below it.)
"""
import math

import numpy as np

from _exact import BudgetError  # noqa: F401  (re-exported: the exact cases raise it)

U = 2.0 ** -24
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}


def gamma(n):
    return n * U / (1.0 - n * U)


def cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


def triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def tables64(n_in, n_out, kernel="bicubic"):
    """(first int64 [n_out], weight float64 [n_out, K], spans [(lo, hi)]) of one axis, from the definition, one output at a time."""
    filt = {"bicubic": cubic, "bilinear": triangle}[kernel]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[kernel] * fs
    K = 2 * int(math.ceil(support)) + 1
    first = np.zeros(n_out, dtype=np.int64)
    weight = np.zeros((n_out, K), dtype=np.float64)
    spans = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        ws = [filt((j + lo - c + 0.5) / fs) for j in range(hi - lo)]
        total = math.fsum(ws)
        weight[i, :hi - lo] = [v / total for v in ws]
        first[i] = lo
        spans.append((lo, hi))
    return first, weight, spans


def tables(n_in, n_out, kernel="bicubic"):
    """What the device gets: (first int32, weight float32)."""
    first, weight, _ = tables64(n_in, n_out, kernel)
    return first.astype(np.int32), weight.astype(np.float32)


def _gather(n, first, K):
    return np.clip(first.astype(np.int64)[:, None] + np.arange(K, dtype=np.int64)[None, :], 0, n - 1)


def resize64(src, xf, xw, yf, yw, want_bound=True):
    """src [F,H,W,3] -> (out float64 [F,h,w,3], bound float64 [F,h,w,3] | None): s[Y][X] = sum_k yw[Y][k] t[clamp(yf[Y] + k)][X],
    t[r][X] = sum_k xw[X][k] src[r][clamp(xf[X] + k)], the tables converted to float64 as they are."""
    src = np.asarray(src, dtype=np.float64)
    F, H, W, _ = src.shape
    xw64, yw64 = np.asarray(xw, dtype=np.float64), np.asarray(yw, dtype=np.float64)
    ix, iy = _gather(W, np.asarray(xf), xw64.shape[1]), _gather(H, np.asarray(yf), yw64.shape[1])

    def passes(a, wx, wy):
        t = np.einsum("xk,frxkc->frxc", wx, a[:, :, ix, :])          # [F,H,w,3]
        return np.einsum("yk,fykxc->fyxc", wy, t[:, iy, :, :])       # [F,h,w,3]

    out = passes(src, xw64, yw64)
    if not want_bound:
        return out, None
    mag = passes(np.abs(src), np.abs(xw64), np.abs(yw64))            # sum_k |wy_k| A_k
    gx, gy = gamma(xw64.shape[1]), gamma(yw64.shape[1])
    return out, (gy + (1.0 + gy) * gx) * mag


def quantise64(v):
    v = np.where(np.isnan(v), 0.0, v)
    return np.rint(np.clip(v, 0.0, 255.0))


def excused(ref, bound):
    """Where the float64 value is within `bound` of a rounding tie (k + 0.5, k = 0..254) or of a clamp edge (0, 255): the only places
    where a result inside the bound may quantise to the neighbouring code."""
    tie = np.abs(ref - (np.floor(ref) + 0.5)) <= bound
    tie &= (ref > 0.0 - bound) & (ref < 255.0 + bound)
    edge = (np.abs(ref) <= bound) | (np.abs(ref - 255.0) <= bound)
    return tie | edge


# ---------------------------------------------------------------------------------------------------------------- exact cases
def exact_case(rs, F, H, W, h, w, KX, KY, density=0.3):
    """Pixels: integers 0..255.  Weights: multiples of 2^-4 in [-1, 1], zero on 1 - density of the taps, no unit sum.  `first`: anywhere
    from -(K + 2) to n + 2, so the clamp acts on both sides, in no order.  Every partial sum of the row pass is then a multiple of 2^-4,
    of the column pass a multiple of 2^-8; `BudgetError` if the absolute sum of any element reaches 2^24 of those.
    -> dict(src float32 [F,H,W,3], xf, xw, yf, yw, ref float64 [F,h,w,3])."""
    from _exact import check_sum_budget
    import torch

    def axis(n_in, n_out, K):
        first = rs.randint(-(K + 2), n_in + 3, size=n_out).astype(np.int32)
        if n_out >= 2:   # both ends are reached in every case: every tap of one output clamps to 0, of another to n - 1
            first[rs.randint(0, n_out // 2)], first[rs.randint(n_out // 2, n_out)] = -(K + 2), n_in + 2
        wt = rs.randint(-16, 17, size=(n_out, K)) * (rs.random_sample((n_out, K)) < density) / 16.0
        return first, wt.astype(np.float32)

    src = rs.randint(0, 256, size=(F, H, W, 3)).astype(np.float32)
    xf, xw = axis(W, w, KX)
    yf, yw = axis(H, h, KY)
    ix = _gather(W, xf, KX)
    row_mag = np.einsum("xk,frxkc->frxc", np.abs(xw.astype(np.float64)), np.abs(src.astype(np.float64))[:, :, ix, :])
    check_sum_budget(torch.from_numpy(row_mag), 2.0 ** -4, "resize row pass")
    ref, _ = resize64(src, xf, xw, yf, yw, want_bound=False)
    col_mag = np.einsum("yk,fykxc->fyxc", np.abs(yw.astype(np.float64)), row_mag[:, _gather(H, yf, KY), :, :])
    check_sum_budget(torch.from_numpy(col_mag), 2.0 ** -8, "resize column pass")
    return dict(src=src, xf=xf, xw=xw, yf=yf, yw=yw, ref=ref)
