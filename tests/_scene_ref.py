"""A float64 numpy restatement of include/vsr_hip_scene.h, line by line: the sums behind the scene score of a pair of LR frames, the
cut rule on them, the window and fed-back estimate composed under the rule's flags, and the host step `driver.scene_cuts`.  Pinned on
hand-computed cases by tests/test_scene_ref_helper.py; tests/test_gpu_scene.py compares the device against it.

Also the inputs of those tests: frame pairs of three kinds, the table of decide cases, and the two-scene clip the clip runs use."""
from collections import namedtuple

import numpy as np

WG_PIXELS = 1024        # VSR_SCENE_WG_PIXELS: pixels of one workgroup of the sums launch
FINISH_THREADS = 256    # VSR_SCENE_FINISH_THREADS
THRESHOLDS = (15.0, 2.0)

# {a0, a1, a2, o}: the BT.601 limited-range luma row as float32 (what frames._luma4("y", "bt601", False) gives; the helper test checks
# that it does) and an arbitrary one
_GY, _KR, _KB = 219.0 / 255.0, 0.299, 0.114
LUMA_BT601 = np.array([_GY * _KR, _GY * (1.0 - _KR - _KB), _GY * _KB, 16.0], dtype=np.float32)
LUMA_ODD = np.array([0.7312, -0.2158, 0.4801, 3.25], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the three entries
def luma_code(frames, luma4):
    """Steps 1 to 4 of vsr_scene_pair_sums: float32 [...,3] -> the 8-bit luma code per pixel, float64 [...]."""
    a0, a1, a2, o = (np.float64(v) for v in np.asarray(luma4, dtype=np.float32))
    f = np.asarray(frames, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = ((o + a0 * f[..., 0]) + a1 * f[..., 1]) + a2 * f[..., 2]
        q = np.where(y >= 0.0, y, 0.0)        # negatives and NaN
        q = np.where(q > 255.0, 255.0, q)
    return np.rint(q)                          # ties to even


def pair_sums(a, b, luma4=LUMA_BT601):
    """vsr_scene_pair_sums: a, b [P,h,w,3] (or [h,w,3]) -> float64 [P,2] = {sad, n}."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.ndim == 3:
        a, b = a[None], b[None]
    d = np.abs(luma_code(a, luma4) - luma_code(b, luma4))
    out = np.empty((a.shape[0], 2), dtype=np.float64)
    out[:, 0] = d.reshape(a.shape[0], -1).sum(axis=1)   # integers below 2^53: exact in any order
    out[:, 1] = float(a.shape[1] * a.shape[2])
    return out


def decide(sums, prev=None, t_abs=THRESHOLDS[0], ratio=THRESHOLDS[1]):
    """vsr_scene_decide: sums [P,2], prev {sad, n} of the pair before or None -> int32 [P]."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    flags = np.zeros(s.shape[0], dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(s.shape[0]):
            m = s[p, 0] / s[p, 1]
            if p > 0:
                m_prev = s[p - 1, 0] / s[p - 1, 1]
            elif prev is not None:
                m_prev = np.float64(prev[0]) / np.float64(prev[1])
            else:
                m_prev = np.float64(0.0)
            bar = np.float64(ratio) * m_prev
            flags[p] = 1 if (m >= t_abs and m >= bar) else 0
    return flags


def window(a, b, c, prev_est=None, flag_ab=0, flag_bc=0):
    """vsr_scene_window: frames [h,w,3], prev_est [1,H,W,3] or None -> (x3 [3,h,w,3], est [1,h,w,3] | None); copies only."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    x3 = np.stack([b if flag_ab else a, b, b if flag_bc else c])
    if prev_est is None:
        return x3, None
    prev_est = np.asarray(prev_est, dtype=np.float32)
    h, w = a.shape[:2]
    H, W = prev_est.shape[1:3]
    assert H % h == 0 and W % w == 0 and H // h == W // w
    S = H // h
    est = b[None].copy() if flag_ab else prev_est[:, ::S, ::S][:, :h, :w].copy()
    return x3, est


def cuts(sums, thresholds=None):
    """driver.scene_cuts: the rule over consecutive pairs with no pair before the first -> (cuts bool [P], m float64 [P])."""
    t_abs, ratio = THRESHOLDS if thresholds is None else thresholds
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s[:, 0] / s[:, 1]
    return decide(s, None, t_abs, ratio).astype(bool), m


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ------------------------------------------------------------------------------------------------ inputs: frame pairs
# the sizes of the GPU test: one pixel; one row narrower than a wave; h * w % 4 != 0 (15, 561, 8385 pixels: the element path whatever the
# base) and % 4 == 0 (4096: the 16-byte path on an aligned base); 17 x 33 and 64 x 64 within one workgroup, 65 x 129 = 8385 pixels in 9;
# and 513 x 512 = 262656 pixels = 256.5 workgroups of WG_PIXELS -> 257 partials > FINISH_THREADS: the finish launch's strided loop runs twice
FINISH_SIZE = (FINISH_THREADS * WG_PIXELS // 512 + 1, 512)
SIZES = [(1, 1), (1, 7), (5, 3), (17, 33), (64, 64), (65, 129), FINISH_SIZE]
KINDS = ("integer", "float", "salted")


def n_workgroups(h, w):
    return -(-h * w // WG_PIXELS)


def make_pair(kind, P, h, w, seed=0):
    """(a, b) float32 [P,h,w,3].  integer: whole numbers in 0..255; float: general floats in about -20..280; salted: the float kind with
    NaN, +inf, -inf, negatives and values above 255 written over a share of the elements (at least one of each where the size allows)."""
    rs = np.random.RandomState(1000 * seed + 31 * h + w + 7 * P + KINDS.index(kind))
    shape = (P, h, w, 3)
    if kind == "integer":
        return tuple(rs.randint(0, 256, shape).astype(np.float32) for _ in range(2))
    a, b = (rs.uniform(-20.0, 280.0, shape).astype(np.float32) for _ in range(2))
    if kind == "salted":
        salt = np.array([np.nan, np.inf, -np.inf, -3.0, 300.0, 1e30, -1e30], dtype=np.float32)
        for t in (a, b):
            flat = t.reshape(-1)
            k = max(1, flat.size // 9)
            at = rs.choice(flat.size, size=min(flat.size, k), replace=False)
            flat[at] = salt[np.arange(at.size) % salt.size]
    return a, b


# ------------------------------------------------------------------------------------------------ inputs: decide
DecideCase = namedtuple("DecideCase", "name sums prev t_abs ratio want")
_N = 4.0
DECIDE_CASES = [
    # m = 15 exactly at t_abs, m_prev = 7.5 so that ratio * m_prev = 15 exactly: both comparisons at equality
    DecideCase("equal_both", [[60.0, _N]], [30.0, _N], 15.0, 2.0, [1]),
    DecideCase("below_t_abs", [[59.0, _N]], [4.0, _N], 15.0, 2.0, [0]),
    DecideCase("below_ratio", [[60.0, _N]], [31.0, _N], 15.0, 2.0, [0]),
    DecideCase("no_prev", [[60.0, _N]], None, 15.0, 2.0, [1]),
    DecideCase("no_prev_below", [[59.0, _N]], None, 15.0, 2.0, [0]),
    # a run: quiet, quiet, cut, (the pair after a cut is not one), sustained fast motion (no run of cuts after its onset), and the second of
    # two cuts one pair apart is missed (the header's two limits)
    DecideCase("run", [[12.0, _N], [16.0, _N], [400.0, _N], [20.0, _N], [80.0, _N], [88.0, _N], [96.0, _N], [400.0, _N], [440.0, _N]], None,
               15.0, 2.0, [0, 0, 1, 0, 1, 0, 0, 1, 0]),
    DecideCase("run_with_prev", [[100.0, _N], [400.0, _N]], [60.0, _N], 15.0, 2.0, [0, 1]),
    DecideCase("open", [[0.0, _N], [3.0, _N], [1.0, _N]], [1000.0, _N], 0.0, 0.0, [1, 1, 1]),
    DecideCase("closed", [[1020.0, _N], [0.0, _N], [1020.0, _N]], None, 1e30, 2.0, [0, 0, 0]),
    DecideCase("closed_ratio", [[8.0, _N], [1020.0, _N]], [4.0, _N], 0.0, 1e30, [0, 0]),
    # a product that is not exact: 0.1 * 3 rounds to 0.30000000000000004 > 0.3
    DecideCase("rounded_product", [[3.0, 10.0], [3.0, 10.0]], [3.0, 1.0], 0.0, 0.1, [0, 1]),
]


# ------------------------------------------------------------------------------------------------ inputs: the two-scene clip
CLIP_S, CLIP_LR = 2, 64                 # the clip runs: LR frames of 64 x 64 (the smallest VSR.forward accepts), x2
CLIP_A, CLIP_B = 4, 4                   # frames of scene A and of scene B: the cut is the pair (CLIP_A - 1, CLIP_A)


def scene_video(n, H, W, seed, invert=False):
    """uint8 RGB [n,H,W,3]: blurred noise in 0..160 translated by one pixel per frame down and right (half an LR pixel at x2: slow
    motion, a small score between frames); `invert`: 255 - frame, values in 95..255 (a large score against any other scene)."""
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(seed)
    base = gaussian_filter(rs.uniform(0, 255, size=(H + n, W + n, 3)).astype(np.float32), sigma=(3, 3, 0))
    base = (base - base.min()) / (base.max() - base.min()) * 160.0
    v = np.stack([np.floor(base[k:k + H, k:k + W]) for k in range(n)]).astype(np.uint8)
    return 255 - v if invert else v


def two_scene_video(nA=CLIP_A, nB=CLIP_B, H=CLIP_S * CLIP_LR, W=CLIP_S * CLIP_LR):
    """Scene A (seed 11) then scene B (the inverse of seed 12): uint8 [nA + nB,H,W,3]; the one cut is the pair (nA - 1, nA)."""
    return np.concatenate([scene_video(nA, H, W, 11), scene_video(nB, H, W, 12, invert=True)])


def clip_m(video, S=CLIP_S, luma4=LUMA_BT601):
    """The score of every consecutive pair of the clip's LR frames, from the RGB frames as floats decimated as the runner's nearest
    decimation does (no 4:2:0 round trip): float64 [T-1]."""
    lr = np.asarray(video)[:, ::S, ::S].astype(np.float32)
    s = pair_sums(lr[:-1], lr[1:], luma4)
    return s[:, 0] / s[:, 1]
