"""libvsr_hip_deint.so on the device against the numpy restatement of its header (tests/_deint_ref.py), bit for bit.

csrc/clip_deint.hip covers a plane with workgroups of VSR_DEINT_TILE_ROWS rows by VSR_DEINT_TILE_BYTES bytes (read from the header), a
thread taking 16 bytes of a pair of rows; a plane is moved with 16-byte accesses where every base, its offset and its row pitch are
multiples of 16 and sample by sample otherwise.  The smallest shapes at which each of these can go wrong:

  rows 2, 3, 4, 5, 7      one pair; a pair and a half (the half a kept row with keep = 0, a rebuilt one with keep = 1: the reflection at the
                          bottom); two pairs; two and a half; more than one workgroup's 4 pairs is left to the frame sizes below
  row bytes 1, 2, 3, 15, 16, 17, 33, 48    a ragged run alone (1 .. 15), one 16-byte access (16), three (48), and pitches that are no
                          multiple of 16 with one and two full runs before the ragged one (17, 33), where the whole plane goes sample by
                          sample
  frames 4 x 6, 6 x 10, 3 x 6 (4:2:2, 4:4:4), 5 x 7 (4:4:4)   every layout's plane table; planes at odd offsets (18, 27; 35, 70)
  frames (8 TILE_ROWS + 6) x (TILE_BYTES + 6) = 70 x 1030 and 70 x (2 TILE_BYTES + 32) = 70 x 2080   more than one workgroup both ways; the
                          first sample by sample (1030 and 515 are no multiples of 16), the second with 16-byte accesses in every plane
                          (2080, 1040 and, in 16-bit layouts, twice that), chroma planes of 35 rows in 4:2:0
all with the four (keep, kept_first), 8-bit words over 0 .. 255, 16-bit words over 0 .. 65535 (so p010le's low 6 bits are set)."""
import functools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _deint_ref as R  # noqa: E402
import _lag as G  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import _lib, driver  # noqa: E402

FLAGS = [(0, 1), (0, 0), (1, 1), (1, 0)]   # (keep, kept_first)
ROWS = (2, 3, 4, 5, 7)
ROW_BYTES = (1, 2, 3, 15, 16, 17, 33, 48)


@functools.lru_cache(maxsize=None)
def tile():
    with open(_lib.DEINTHEADER_PATH) as f:
        defs = dict(re.findall(r"^#define (VSR_DEINT_TILE_[A-Z]+) (\d+)", f.read(), re.M))
    return int(defs["VSR_DEINT_TILE_ROWS"]), int(defs["VSR_DEINT_TILE_BYTES"])


def big_sizes():
    tr, tb = tile()
    return [(8 * tr + 6, tb + 6), (8 * tr + 6, 2 * tb + 32)]


def frame_sizes(fmt):
    small = [(4, 6), (6, 10)] + ([(3, 6)] if "420" not in fmt and fmt not in ("nv12", "p010le") else []) + ([(5, 7)] if "444" in fmt else [])
    return small + big_sizes()


def random_bytes(rs, n):
    return rs.randint(0, 256, size=n).astype(np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ref_plane(P, C, N, rows, nbytes, sb, shift, keep, kept_first):
    """The restatement on one dense plane given as bytes."""
    view = (lambda a: a.view("<u2").reshape(rows, nbytes // 2)) if sb == 2 else (lambda a: a.reshape(rows, nbytes))
    out = R.deint_plane(view(P), view(C), view(N), keep, kept_first, shift)
    return np.ascontiguousarray(out).reshape(-1).view(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. one plane, every small shape
@pytest.mark.parametrize("sb, shift", [(1, 0), (2, 0), (2, 6)])
def test_one_plane_of_every_small_shape_equals_the_restatement(sb, shift):
    rs = np.random.RandomState(10 * sb + shift)
    widths = [w for w in ROW_BYTES if w % sb == 0] + ([34] if sb == 2 else [])   # 16-bit rows: an even number of bytes (34: two runs and a sample)
    seen = 0
    for rows in ROWS:
        for nbytes in widths:
            n = rows * nbytes
            P, C, N = (random_bytes(rs, n) for _ in range(3))
            dP, dC, dN = dev(P), dev(C), dev(N)
            assert dC.data_ptr() % 16 == 0   # so the 16-byte path runs where the pitch allows it
            for comps in ((1, 2) if (nbytes // sb) % 2 == 0 else (1,)):   # comps only changes how the row's samples are counted
                planes = [(0, rows, nbytes // sb // comps, comps)]
                for keep, kept_first in FLAGS:
                    out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
                    driver.deinterlace_planes(dP, dC, dN, planes, sb, shift, keep, kept_first, out)
                    want = ref_plane(P, C, N, rows, nbytes, sb, shift, keep, kept_first)
                    assert np.array_equal(host(out), want), (rows, nbytes, comps, keep, kept_first)
                    seen += 1
    assert seen >= len(ROWS) * len(widths) * 4


def test_three_planes_of_unlike_shapes_in_one_launch_and_the_path_does_not_change_the_bits():
    """Planes of 7 x 48, 3 x 17 and 5 x 16 bytes in one frame, in one call: each plane has its own run of workgroups in the one grid.
    Then the same frame one byte further into its buffers: every plane goes sample by sample and gives the same bytes."""
    rs = np.random.RandomState(1)
    shapes = [(7, 48), (3, 17), (5, 16)]
    planes, at = [], 0
    for rows, nb in shapes:
        planes.append((at, rows, nb, 1))
        at += rows * nb
    assert planes[2][0] % 16 != 0   # 336 + 51: the third plane's pitch allows wide accesses, its offset does not
    P, C, N = (random_bytes(rs, at) for _ in range(3))
    for keep, kept_first in FLAGS:
        want = np.concatenate([ref_plane(P[o:o + r * c], C[o:o + r * c], N[o:o + r * c], r, c, 1, 0, keep, kept_first) for o, r, c, _ in planes])
        out = torch.zeros(at, dtype=torch.uint8, device="cuda")
        driver.deinterlace_planes(dev(P), dev(C), dev(N), planes, 1, 0, keep, kept_first, out)
        assert np.array_equal(host(out), want)
        shifted = [torch.zeros(at + 1, dtype=torch.uint8, device="cuda") for _ in range(4)]
        for t, a in zip(shifted, (P, C, N)):
            t[1:] = dev(a)
        driver.deinterlace_planes(shifted[0][1:], shifted[1][1:], shifted[2][1:], planes, 1, 0, keep, kept_first, shifted[3][1:])
        assert np.array_equal(host(shifted[3][1:]), want) and int(shifted[3][0]) == 0


# ------------------------------------------------------------------------------------------------ 2. every layout
@functools.lru_cache(maxsize=None)
def clip3(fmt, H, W):
    """(host frames uint8 [3, bytes], the same on the device): random bytes, so 16-bit words cover 0 .. 65535."""
    rs = np.random.RandomState(H * 1000 + W + len(fmt))
    a = rs.randint(0, 256, size=(3, driver.pix_frame_bytes(fmt, H, W))).astype(np.uint8)
    d = dev(a)
    a.setflags(write=False)
    return a, d


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_layout_at_every_size_equals_the_restatement(fmt):
    for H, W in frame_sizes(fmt):
        a, d = clip3(fmt, H, W)
        for keep, kept_first in FLAGS:
            got = driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (a.shape[1],)
            want = R.deint_frame(a[0], a[1], a[2], (H, W), fmt, keep, kept_first)
            bad = np.flatnonzero(host(got) != want)
            assert bad.size == 0, f"{fmt} {H}x{W} keep {keep} kept_first {kept_first}: {bad.size} bytes differ, first at {bad[0]}"


def test_the_big_sizes_leave_one_workgroup_both_ways_and_take_both_paths():
    tr, tb = tile()
    (H1, W1), (H2, W2) = big_sizes()
    assert (tr, tb) == (8, 1024) and (H1, W1) == (70, 1030) and (H2, W2) == (70, 2080)
    assert H1 > tr and H1 // 2 > tr and W1 > tb and W1 // 2 < tb < W2 // 2   # chroma of the second is wider than a workgroup too
    assert W1 % 16 and (W1 // 2) % 16 and W2 % 16 == 0 and (W2 // 2) % 16 == 0 and (H2 * W2) % 16 == 0
    assert (H1 // 2) % 2 == 1   # 4:2:0 chroma: 35 rows, half a pair at the bottom


@pytest.mark.parametrize("fmt", ["yuv420p", "p010le", "yuv444p10le"])
def test_static_content_is_the_identity_and_kept_rows_are_bit_copies(fmt):
    H, W = big_sizes()[1]
    a, d = clip3(fmt, H, W)
    planes, sb, shift = driver.deint_planes(fmt, H, W)
    for keep, kept_first in FLAGS:
        still = host(driver.deinterlace(d[1], d[1], d[1], (H, W), fmt, keep, kept_first))
        moving = host(driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first))
        for off, rows, cols, comps in planes:
            nb = cols * comps * sb
            cur, s, m = (x[off:off + rows * nb].reshape(rows, nb) for x in (a[1], still, moving))
            assert np.array_equal(m[keep::2], cur[keep::2]) and np.array_equal(s[keep::2], cur[keep::2])
            if shift == 0:
                assert np.array_equal(s, cur)       # weave: out == cur bit for bit
            else:                                   # p010le: the rebuilt rows carry the value, their low 6 bits are 0
                assert np.array_equal(s.view("<u2") >> 6, cur.view("<u2") >> 6) and (s[1 - keep::2].view("<u2") & 63 == 0).all()


def test_refusals_of_the_python_side_and_of_the_entry():
    a = torch.zeros(driver.pix_frame_bytes("yuv420p", 2, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="holds no two fields"):
        driver.deinterlace(a, a, a, (2, 4), "yuv420p", 0, 1)
    b = torch.zeros(driver.pix_frame_bytes("yuv444p", 2, 4), dtype=torch.uint8, device="cuda")
    for ins in ((b, a.new_zeros(24), a.new_zeros(24)), (a.new_zeros(24), b, b), (a.new_zeros(24), a.new_zeros(24), b)):
        with pytest.raises(_lib.VsrHipError, match="out is one of the inputs"):
            driver.deinterlace(*ins, (2, 4), "yuv444p", 0, 1, out=b)
    with pytest.raises(ValueError, match="must be uint8 of 24 bytes"):
        driver.deinterlace(b, b, b, (2, 4), "yuv444p", 0, 1, out=a)


# ------------------------------------------------------------------------------------------------ 3. aliasing, offsets
@pytest.mark.parametrize("fmt, H, W", [("nv12", 6, 10), ("yuv422p10le", 70, 2080)])
def test_inputs_that_are_one_another(fmt, H, W):
    a, d = clip3(fmt, H, W)
    for keep, kept_first in FLAGS:
        for idx in ((1, 1, 2), (0, 1, 1), (0, 1, 0), (1, 1, 1)):   # prev is cur, next is cur, prev is next, all three
            p, c, n = (d[i] for i in idx)
            got = driver.deinterlace(p, c, n, (H, W), fmt, keep, kept_first)
            want = R.deint_frame(*(a[i] for i in idx), (H, W), fmt, keep, kept_first)
            assert np.array_equal(host(got), want), (idx, keep, kept_first)


@pytest.mark.parametrize("fmt, off", [("yuv420p", 1), ("yuv444p", 1), ("yuv420p10le", 2), ("p010le", 2)])
def test_frames_inside_larger_buffers(fmt, off):
    """All four frames start `off` bytes into a larger buffer (no 16-byte access fits: the sample-by-sample path on a shape whose
    planes would otherwise go wide), then the output alone; the bytes either side of the output stay as they were."""
    H, W = big_sizes()[1]
    a, d = clip3(fmt, H, W)
    n = a.shape[1]
    bufs = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(4)]
    for t, i in zip(bufs, range(3)):
        t[off:off + n] = d[i]
    for keep, kept_first in FLAGS[:2] if off == 2 else FLAGS:
        want = R.deint_frame(a[0], a[1], a[2], (H, W), fmt, keep, kept_first)
        for ins in ([t[off:off + n] for t in bufs[:3]], [d[0], d[1], d[2]]):
            assert ins[0].data_ptr() % 16 in (off, 0)
            bufs[3].fill_(0xA5)
            driver.deinterlace(ins[0], ins[1], ins[2], (H, W), fmt, keep, kept_first, out=bufs[3][off:off + n])
            got = host(bufs[3])
            assert np.array_equal(got[off:off + n], want) and (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all()
    if off == 2:
        with pytest.raises(_lib.VsrHipError, match="16-bit samples at an odd byte address"):
            driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, 0, 1, out=bufs[3][1:1 + n])


# ------------------------------------------------------------------------------------------------ 4. every byte, none beyond
@pytest.mark.parametrize("fmt, H, W", [("yuv422p", 3, 6), ("yuv444p", 5, 7), ("nv12", 70, 1030), ("yuv420p10le", 70, 2080)])
def test_poisoned_output_every_byte_written_and_nothing_else(fmt, H, W):
    a, d = clip3(fmt, H, W)
    n = a.shape[1]
    for keep, kept_first in FLAGS:
        want = R.deint_frame(a[0], a[1], a[2], (H, W), fmt, keep, kept_first)
        with poisoned(package_state=False) as arena:   # (frames.py keeps no buffer between calls)
            out = driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first)
            assert arena.n_allocated == 1 and arena.find(out) is not None
            assert np.array_equal(host(out), want)
            arena.check()
        for fill in (0x00, 0xFF):   # every byte written whatever was there before; guard bytes on both sides untouched
            big = torch.full((16 + n + 16,), fill, dtype=torch.uint8, device="cuda")
            driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first, out=big[16:16 + n])
            got = host(big)
            assert np.array_equal(got[16:16 + n], want) and (got[:16] == fill).all() and (got[16 + n:] == fill).all()


# ------------------------------------------------------------------------------------------------ 5. stream order, repeatability
def test_a_call_on_a_side_stream_with_a_lagging_main_stream_gives_the_same_bits():
    """The call is enqueued on the current stream alone (tests/_lag.py, policy pre:0: one lag on the main stream before the call): on a
    side stream that has the inputs it neither waits for the main stream nor needs anything from it."""
    fmt = "yuv420p"
    H, W = big_sizes()[1]
    a, d = clip3(fmt, H, W)
    want = R.deint_frame(a[0], a[1], a[2], (H, W), fmt, 0, 1)
    main = torch.cuda.current_stream()
    backend = G.TorchBackend()
    side = None
    for _ in range(4):   # a side stream on a hardware queue of its own (streams may share one: the lag would hold both)
        cand = torch.cuda.Stream()
        if all(G.probe_independence([main, cand], backend, lag_ms=10.0).values()):
            side = cand
            break
    assert side is not None, "no side stream independent of the main stream among four"
    out = torch.zeros(a.shape[1], dtype=torch.uint8, device="cuda")

    def call():
        with torch.cuda.stream(side):
            driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, 0, 1, out=out)

    torch.cuda.synchronize()
    host_ms = G.warm_host_ms(call, side.synchronize)
    out.zero_()
    torch.cuda.synchronize()
    with G.Lagger("pre:0", G.lag_for(host_ms), pool=[main, side], backend=backend) as lg:
        call()
        side.synchronize()            # the side stream has finished ...
    assert lg.failures == [] and len(lg.lags) == 1 and lg.lags[0]["held"], lg.report()   # ... while the main stream still lagged
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want)


def test_two_runs_give_the_same_bits():
    for fmt in ("p010le", "yuv444p"):
        H, W = big_sizes()[0]
        _, d = clip3(fmt, H, W)
        for keep, kept_first in FLAGS:
            one = driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first)
            two = driver.deinterlace(d[0], d[1], d[2], (H, W), fmt, keep, kept_first)
            assert torch.equal(one, two)


def test_deinterlace_clip_follows_the_schedule():
    fmt, H, W = "yuv422p", 6, 10
    rs = np.random.RandomState(5)
    frames = rs.randint(0, 256, size=(4, driver.pix_frame_bytes(fmt, H, W))).astype(np.uint8)
    for mode in ("frame", "field"):
        for tff in (True, False):
            got = driver.deinterlace_clip(frames, (H, W), fmt, mode, tff)
            assert isinstance(got, np.ndarray) and got.shape == ((8 if mode == "field" else 4), frames.shape[1])
            assert np.array_equal(got, R.deint_clip(frames, (H, W), fmt, mode, tff))
    assert np.array_equal(driver.deinterlace_clip(frames[:1], (H, W), fmt, "frame"), frames[:1])   # T = 1: itself either side
