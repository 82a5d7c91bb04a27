"""numpy restatement of include/vsr_hip_patch.h (plain index arithmetic on uint32 views: bits, not numbers) and of the draw order of
`frames.patch_table`, both written from the header and the docstring, not from the code under test."""
import numpy as np

MAX_B = 64
TILE = 32
FLIP_X, FLIP_Y, TRANSPOSE, REVERSE_TIME = 1, 2, 4, 8


def crop(flags, Ph, Pw):
    """(ch, cw): the crop a row takes from the source."""
    return (Pw, Ph) if flags & TRANSPOSE else (Ph, Pw)


def row_ok(row, G, n, H, W, Ph, Pw, S=1, lr_src=False):
    """The library's own rule for one table row."""
    t0, y0, x0, flags = (int(v) for v in row)
    ch, cw = crop(flags, Ph, Pw)
    ok = flags & ~15 == 0 and 0 <= t0 <= G - n and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw
    if lr_src:
        ok = ok and y0 % S == 0 and x0 % S == 0
    return bool(ok)


def _index(flags, n, oh, ow, step):
    """For an output of oh x ow: (kk [n], rows [oh,ow], cols [oh,ow]) relative to the origin, the source walked with `step`."""
    k = np.arange(n)
    kk = n - 1 - k if flags & REVERSE_TIME else k
    i, j = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    u, v = (j, i) if flags & TRANSPOSE else (i, j)
    ch, cw = (ow, oh) if flags & TRANSPOSE else (oh, ow)
    ii = step * ch - 1 - step * u if flags & FLIP_Y else step * u
    jj = step * cw - 1 - step * v if flags & FLIP_X else step * v
    return kk, ii, jj


def gather_hr(src, table, n, Ph, Pw):
    """src [G,H,W,3] (any 4-byte dtype) -> hr [B,n,Ph,Pw,3] as uint32: steps 1 to 6 of the header."""
    s = np.ascontiguousarray(src).view(np.uint32)
    out = np.empty((len(table), n, Ph, Pw, 3), dtype=np.uint32)
    for b, (t0, y0, x0, flags) in enumerate(np.asarray(table).tolist()):
        kk, ii, jj = _index(flags, n, Ph, Pw, 1)
        out[b] = s[(t0 + kk)[:, None, None], (y0 + ii)[None], (x0 + jj)[None]]
    return out


def gather_lr_nearest(src, table, n, Ph, Pw, S):
    """lr[b][k][i][j] = hr[b][k][i S][j S]: the decimation of the augmented patch."""
    return np.ascontiguousarray(gather_hr(src, table, n, Ph, Pw)[:, :, ::S, ::S])


def gather_lr_nearest_wrong_phase(src, table, n, Ph, Pw, S):
    """What the header warns against: the frames decimated first, the decimated crop augmented afterwards."""
    t = np.asarray(table).copy()
    t[:, 1:3] //= S
    return gather_hr(np.ascontiguousarray(np.asarray(src)[:, ::S, ::S]), t, n, Ph // S, Pw // S)


def gather_lr_src(lr_src, table, n, Ph, Pw, S):
    """The header's second mode: steps 1 to 6 on lr_src with y0 / S, x0 / S and the patch of Ph / S x Pw / S."""
    t = np.asarray(table).copy()
    assert (t[:, 1:3] % S == 0).all()
    t[:, 1:3] //= S
    return gather_hr(lr_src, t, n, Ph // S, Pw // S)


def draw_table(seed_or_rng, B, G, n, H, W, Ph, Pw, S, augment=True, transpose=None):
    """The draw order of `frames.patch_table`, restated: flags, t0, y0, x0 per row; bit 4 masked off after the draw."""
    rng = np.random.RandomState(seed_or_rng) if isinstance(seed_or_rng, int) else seed_or_rng
    allow_t = (Ph == Pw) if transpose is None else transpose
    rows = []
    for _ in range(B):
        flags = int(rng.randint(16)) if augment else 0
        if not allow_t:
            flags &= 11
        ch, cw = crop(flags, Ph, Pw)
        t0 = int(rng.randint(G - n + 1))
        y0 = int(rng.randint((H - ch) // S + 1)) * S
        x0 = int(rng.randint((W - cw) // S + 1)) * S
        rows.append((t0, y0, x0, flags))
    return np.array(rows, dtype=np.int32)
