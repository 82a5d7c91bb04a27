"""numpy restatement of include/vsr_hip_deint.h, written from the header's rule, step by step, in int32 (the kernel's source is not
consulted): one plane (`deint_plane`), a packed frame of any layout of `frames.PIX_FORMATS` (`deint_frame`: the planes come from the
layout's definition here, not from `frames.deint_planes`, which the tests check against this), and a whole clip (`deint_clip`: the
neighbours and parities spelled out from the issue's words, not from `frames.deint_schedule`)."""
import numpy as np

FORMATS = ("yuv420p", "nv12", "yuv420p10le", "p010le", "yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le")


def deint_plane(P, C, N, keep, kept_first, shift=0):
    """P, C, N: one plane of prev, cur, next as integer words [rows, samples per row] (comps = 2: the interleaved row as it lies in
    memory; a sample meets only its own column) -> the output words, dtype of C."""
    rows = C.shape[0]
    assert rows >= 2 and P.shape == C.shape == N.shape and keep in (0, 1) and kept_first in (0, 1)
    sP, sC, sN = (a.astype(np.int32) >> shift for a in (P, C, N))
    out = C.copy()                                     # rows y with y % 2 == keep: a bit copy of cur
    for y in range(rows):
        if y % 2 == keep:
            continue
        yu, yd = y - 1, y + 1                          # 1.
        if yu < 0:
            yu = yd
        if yd >= rows:
            yd = yu
        c, e = sC[yu], sC[yd]                          # 2.
        B, A = (sP, sC) if kept_first else (sC, sN)    # 3.
        b, a = B[y], A[y]
        t, sp = (b + a) >> 1, (c + e) >> 1             # 4.
        td0 = np.abs(b - a)                            # 5.
        td1 = (np.abs(sP[yu] - c) + np.abs(sP[yd] - e)) >> 1   # 6.
        td2 = (np.abs(sN[yu] - c) + np.abs(sN[yd] - e)) >> 1
        d = np.maximum(td0 >> 1, np.maximum(td1, td2))          # 7.
        v = np.minimum(np.maximum(sp, t - d), t + d)            # 8.
        out[y] = (v << shift).astype(C.dtype)
    return out


def layout(fmt, H, W):
    """(planes [(offset in bytes, rows, samples per row)], sample_bytes, shift, frame bytes) of one packed frame, from the formats'
    definitions: Y, then Cb and Cr planes (or one interleaved CbCr plane: nv12, p010le), chroma halved both ways (420), across (422) or
    not at all (444); 10-bit names in little-endian 16-bit words, p010le's value in the high 10 bits."""
    assert fmt in FORMATS
    sb = 2 if fmt.endswith("10le") else 1
    if "422" in fmt:
        ch, cw = H, W // 2
    elif "444" in fmt:
        ch, cw = H, W
    else:
        ch, cw = H // 2, W // 2
    if fmt in ("nv12", "p010le"):
        planes = [(0, H, W), (H * W * sb, ch, 2 * cw)]
    else:
        planes = [(0, H, W), (H * W * sb, ch, cw), ((H * W + ch * cw) * sb, ch, cw)]
    return planes, sb, (6 if fmt == "p010le" else 0), (H * W + 2 * ch * cw) * sb


def _plane(frame, off, rows, n, sb):
    raw = frame[off:off + rows * n * sb]
    return (raw.view("<u2") if sb == 2 else raw).reshape(rows, n)


def deint_frame(prev, cur, nxt, shape, fmt, keep, kept_first):
    """Packed uint8 frames [frame bytes] -> the deinterlaced packed frame."""
    planes, sb, shift, fb = layout(fmt, *shape)
    prev, cur, nxt = (np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(-1)) for a in (prev, cur, nxt))
    assert prev.size == cur.size == nxt.size == fb
    out = np.empty(fb, dtype=np.uint8)
    for off, rows, n in planes:
        o = deint_plane(_plane(prev, off, rows, n, sb), _plane(cur, off, rows, n, sb), _plane(nxt, off, rows, n, sb), keep, kept_first, shift)
        out[off:off + rows * n * sb] = o.astype("<u2" if sb == 2 else np.uint8).reshape(-1).view(np.uint8)
    return out


def neighbours(i, T):
    """(prev, next) of frame i in a clip of T: i - 1 and i + 1; at a clip end the missing one is the other neighbour; T = 1: itself."""
    if T == 1:
        return 0, 0
    if i == 0:
        return 1, 1
    if i == T - 1:
        return T - 2, T - 2
    return i - 1, i + 1


def deint_clip(frames, shape, fmt, mode, tff=True):
    """uint8 [T, frame bytes] -> [T, ...] ("frame": the first field in time kept) or [2 T, ...] ("field": then the second field's frame)."""
    assert mode in ("frame", "field")
    frames = np.asarray(frames)
    T = frames.shape[0]
    first = 0 if tff else 1
    out = []
    for i in range(T):
        p, n = neighbours(i, T)
        out.append(deint_frame(frames[p], frames[i], frames[n], shape, fmt, first, 1))
        if mode == "field":
            out.append(deint_frame(frames[p], frames[i], frames[n], shape, fmt, 1 - first, 0))
    return np.stack(out)
