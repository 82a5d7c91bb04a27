"""A numpy restatement of include/vsr_hip_cell.h and of the host steps on its map (`frames.cell_cuts`, `patch_score`,
`patch_table_select`): the 8-bit luma code in float64 (steps 1 to 4 of include/vsr_hip_scene.h, `_scene_ref.luma_code`), every sum in
int64.  tests/test_driver_select_host.py pins it on brute-force sums and hand-made cases; tests/test_gpu_cell_stats.py and
tests/test_gpu_train_select.py compare the device against it.

Also the inputs of those tests: frames of four kinds."""
import numpy as np

from _scene_ref import LUMA_BT601, luma_code

CELL = 16              # VSR_CELL
TILE = (16, 64)        # VSR_CELL_TILE_H, VSR_CELL_TILE_W: pixels of one workgroup
MAX_G = 65535          # VSR_CELL_MAX_G
MAX_VALUE = CELL * CELL * 2 * 255
TRANSPOSE = 4          # VSR_PATCH_TRANSPOSE
LUMA_TIES = np.array([0.5, 0.25, 0.25, 0.0], dtype=np.float32)   # on integers y is k, k + 0.25, k + 0.5 or k + 0.75: exact ties


def cells(H, W):
    return -(-H // CELL), -(-W // CELL)


def codes(frames, luma4=LUMA_BT601):
    """float32 [G,H,W,3] -> the luma code per pixel, int64 [G,H,W]."""
    return luma_code(np.asarray(frames, dtype=np.float32), luma4).astype(np.int64)


def pixel_terms(q):
    """Steps 5 and 6 per pixel: codes int64 [G,H,W] -> (activity, temporal) int64 [G,H,W]; a neighbour outside the frame adds nothing."""
    act = np.zeros_like(q)
    act[:, :, :-1] += np.abs(q[:, :, :-1] - q[:, :, 1:])
    act[:, :-1, :] += np.abs(q[:, :-1, :] - q[:, 1:, :])
    sad = np.zeros_like(q)
    sad[1:] = np.abs(q[1:] - q[:-1])
    return act, sad


def cell_stats(frames, luma4=LUMA_BT601):
    """vsr_cell_stats: float32 [G,H,W,3] -> int32 [G,Ch,Cw,2]."""
    q = codes(frames, luma4)
    G, H, W = q.shape
    Ch, Cw = cells(H, W)
    out = np.zeros((G, Ch, Cw, 2), dtype=np.int64)
    for c, term in enumerate(pixel_terms(q)):
        full = np.zeros((G, Ch * CELL, Cw * CELL), dtype=np.int64)   # the pixels that do not exist add nothing
        full[:, :H, :W] = term
        out[..., c] = full.reshape(G, Ch, CELL, Cw, CELL).sum(axis=(2, 4))
    assert out.max() <= MAX_VALUE
    return out.astype(np.int32)


def cell_cuts(stats, shape, thresholds=(15.0, 2.0)):
    """frames.cell_cuts: the rule of `scene_cuts` on the map's sums, no pair before a group's first -> (cuts bool [G-1], m float64 [G-1])."""
    s = np.asarray(stats).astype(np.int64)
    n = np.float64(shape[0] * shape[1])
    m = np.array([np.float64(int(s[p + 1, :, :, 1].sum())) / n for p in range(s.shape[0] - 1)], dtype=np.float64)
    cuts = np.zeros(m.size, dtype=bool)
    for p in range(m.size):
        m_prev = m[p - 1] if p > 0 else np.float64(0.0)
        cuts[p] = bool(m[p] >= thresholds[0] and m[p] >= np.float64(thresholds[1]) * m_prev)
    return cuts, m


def crop(row, patch):
    """(ch, cw): the crop of table row {t0, y0, x0, flags} for the patch (Ph, Pw)."""
    Ph, Pw = (patch, patch) if np.isscalar(patch) else patch
    return (Pw, Ph) if int(row[3]) & TRANSPOSE else (Ph, Pw)


def patch_score(stats, row, n, patch):
    """frames.patch_score: the cells wholly inside the crop, the frames t0 .. t0 + n - 1, one division in double."""
    s = np.asarray(stats).astype(np.int64)
    t0, y0, x0 = int(row[0]), int(row[1]), int(row[2])
    ch, cw = crop(row, patch)
    total = count = 0
    for i in range(s.shape[1]):
        for j in range(s.shape[2]):
            if CELL * i >= y0 and CELL * (i + 1) <= y0 + ch and CELL * j >= x0 and CELL * (j + 1) <= x0 + cw:
                count += 1
                total += int(s[t0:t0 + n, i, j, 0].sum())
    assert count > 0
    return float(np.float64(total) / np.float64(n * count * CELL * CELL))


def patch_score_pixels(frames, row, n, patch, luma4=LUMA_BT601):
    """The same number with no map: per pixel of the frames, over the pixels of the cells wholly inside the crop."""
    act, _ = pixel_terms(codes(frames, luma4))
    t0, y0, x0 = int(row[0]), int(row[1]), int(row[2])
    ch, cw = crop(row, patch)
    ya, yb = -(-y0 // CELL) * CELL, (y0 + ch) // CELL * CELL
    xa, xb = -(-x0 // CELL) * CELL, (x0 + cw) // CELL * CELL
    assert yb > ya and xb > xa
    total = int(act[t0:t0 + n, ya:yb, xa:xb].sum())
    return float(np.float64(total) / np.float64(n * (yb - ya) * (xb - xa)))


def select(rng, B, G, n, shape, patch, S, augment=True, transpose=None, cuts=None, stats=None, act_min=None, tries=8):
    """frames.patch_table_select, and every candidate it drew -> (table int32 [B',4], scores [B'], tried [B'], candidates): candidates[b] is
    the list of (row, score) drawn for row b, in order (score NaN without act_min)."""
    Ph, Pw = (patch, patch) if np.isscalar(patch) else patch
    H, W = shape
    may_transpose = (Ph == Pw) if transpose is None else bool(transpose)
    valid = [t0 for t0 in range(G - n + 1) if cuts is None or not any(bool(cuts[p]) for p in range(t0, t0 + n - 1))]
    if not valid:
        return np.zeros((0, 4), np.int32), np.zeros(0), np.zeros(0, np.int32), []
    table, scores, tried, candidates = [], [], [], []
    for b in range(B):
        drawn = []
        while True:
            flags = int(rng.randint(16)) if augment else 0
            if not may_transpose:
                flags &= ~TRANSPOSE
            ch, cw = (Pw, Ph) if flags & TRANSPOSE else (Ph, Pw)
            t0 = valid[int(rng.randint(len(valid)))]
            y0 = int(rng.randint((H - ch) // S + 1)) * S
            x0 = int(rng.randint((W - cw) // S + 1)) * S
            row = (t0, y0, x0, flags)
            drawn.append((row, float("nan") if act_min is None else patch_score(stats, row, n, (Ph, Pw))))
            if act_min is None or drawn[-1][1] >= act_min or len(drawn) == tries:
                break
        pick = len(drawn) - 1
        if act_min is not None and not drawn[-1][1] >= act_min:   # none qualified: the largest score, the first among equals
            pick = max(range(len(drawn)), key=lambda k: (drawn[k][1], -k))
        table.append(drawn[pick][0])
        scores.append(drawn[pick][1])
        tried.append(len(drawn))
        candidates.append(drawn)
    return np.array(table, dtype=np.int32), np.array(scores, dtype=np.float64), np.array(tried, dtype=np.int32), candidates


def straddles(row, n, cuts):
    """Whether the sample of `row` holds both frames of a set pair."""
    t0 = int(row[0])
    return any(bool(cuts[p]) for p in range(t0, t0 + n - 1))


# ------------------------------------------------------------------------------------------------ inputs
# G x H x W of the GPU test: one cell and no temporal term; a frame smaller than a cell; one pixel of ragged cells each way on the element
# path (W % 4 != 0); a general ragged size over two tiles across (W % 4 != 0: element path) ; the right-hand neighbour of the last full
# cell is the frame's last column (W = 65: the halo column of the first tile is the last pixel); a walk of nine frames on the 16-byte path
SIZES = [(1, 16, 16), (2, 5, 7), (3, 33, 17), (3, 45, 70), (2, 32, 65), (9, 48, 64)]
KINDS = ("bytes", "salted", "ties", "constant")


def make_frames(kind, G, H, W, seed=0):
    """float32 [G,H,W,3].  bytes: whole numbers in 0..255; salted: floats in about -20..280 with NaN, infinities, negatives, values above
    255 and signed zeros planted; ties: whole numbers (with LUMA_TIES the luma falls on k + 0.5 for a share of the pixels); constant: 77."""
    rs = np.random.RandomState(7919 * seed + 101 * G + 31 * H + W + KINDS.index(kind))
    shape = (G, H, W, 3)
    if kind == "constant":
        return np.full(shape, 77.0, dtype=np.float32)
    if kind in ("bytes", "ties"):
        return rs.randint(0, 256, shape).astype(np.float32)
    f = rs.uniform(-20.0, 280.0, shape).astype(np.float32)
    salt = np.array([np.nan, np.inf, -np.inf, -3.0, 300.0, 0.0, -0.0, 1e30, -1e30], dtype=np.float32)
    flat = f.reshape(-1)
    at = rs.choice(flat.size, size=max(salt.size, flat.size // 9), replace=False)
    flat[at] = salt[np.arange(at.size) % salt.size]
    return f


def luma_of(kind):
    return LUMA_TIES if kind == "ties" else LUMA_BT601
