"""Planar 4:2:2 / 4:4:4 frames in and out on the device (include/vsr_hip_pix.h, driver.pix_ingest / pix_write and the functions above
them) against the float64 restatements of tests/_pix_ref.py, which evaluate the formulas of the header with the float32 coefficients
the kernel received.  The structure of tests/test_gpu_yuv.py.

Shapes (F, H, W, scale), the smallest that reach every branch of csrc/clip_pix.hip (`_pix_ref.shapes`) --
  2 x  6 x 10    4:2:2: W % 4 == 2, element paths both ways; 5 chroma columns: the clamps on both sides; 4:4:4: H W = 60, the wide paths
  1 x 14 x 518   259 chroma columns: a second, ragged 256-lane block of the 4:2:2 element write-out and of the LR kernel
  3 x 18 x 26 at scale 4, 1 x 34 x 46 at scale 3   non-integer decimation ratios (as tests/test_gpu_driver.py)
  2 x  6 x 12    4:2:2: W % 4 == 0 but not % 8: the ingest's one-load luma path, the write-out's element path
  2 x  4 x 16    W % 8 == 0: the wide paths of both
  2 x  6 x 8     the wide paths with frames of 96 (4:2:2) / 144 (4:4:4) bytes at 8 bit: the 4:2:2 Cr plane starts 24 samples after Cb
  1 x  2 x 2064  W / 8 = 258 threads: the wide 4:2:2 write-out's second block, ragged; 4:4:4: 1032 groups, a second block
  3 x  3 x 6     4:2:2: H W = 18 = 2 mod 4, odd H: planes at 18 and 27 of a 36-byte frame, groups of the full-size kernel that straddle
                 two frames, F H W = 54: a ragged last group of 2; 4:4:4: the same through its element paths
  2 x  3 x 8     4:2:2: the wide write-out with an odd H: the Cr plane starts 12 samples after Cb (a multiple of 4, not of 8 or 16)
  2 x  5 x 7, 1 x 1 x 1, 3 x 1 x 3   4:4:4 only: odd W, F H W = 70 / 1 / 9 not a multiple of 4 -- the ragged last group of 2, 1 and 1
                 pixels, groups that straddle frames (H W = 35, 3), planes at odd offsets
every one also at h == H (the plain conversion), all four formats, both sitings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pix_ref as R  # noqa: E402
import _yuv_ref as Y420  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402

IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
COLOUR = [(m, fr) for m in ("bt601", "bt709", "bt2020") for fr in (False, True)]


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def random_frames(rs, fmt, F, H, W, garbage=True):
    """Random code values over the whole code range, packed; bits 10..15 of the 10-bit formats, which the ingest must ignore, hold
    garbage."""
    top = 2 ** R.depth(fmt)
    Wc = R.chroma_width(fmt, W)
    Yc, Cb, Cr = rs.randint(0, top, (F, H, W)), rs.randint(0, top, (F, H, Wc)), rs.randint(0, top, (F, H, Wc))
    b = R.pack(Yc, Cb, Cr, fmt).copy()
    if garbage and R.depth(fmt) == 10:
        b[:, 1::2] |= (rs.randint(0, 64, b[:, 1::2].shape) << 2).astype(np.uint8)
    got = R.unpack(b, fmt, H, W)
    assert np.array_equal(got[0], Yc) and np.array_equal(got[1], Cb) and np.array_equal(got[2], Cr)
    return b


def gpu_ingest(frames, fmt, coef, siting, H, W, h, w):
    lr, hr = driver.pix_ingest(torch.from_numpy(frames).cuda(), (H, W), fmt, coef, siting, (h, w), want_hr=True)
    return lr.cpu(), hr.cpu()


def lr_size(H, W, s):
    return max(int(H / s), 1), max(int(W / s), 1)


# ------------------------------------------------------------------------------------------------ 1. exact, bit for bit
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_identity_coefficients_is_the_interpolation_bit_for_bit(fmt):
    """coef12 = identity, zero offsets: the ingest returns (Y, Cb', Cr') themselves, clamped to 0..255.  The weights are dyadic, so the
    float64 interpolation is exactly representable in float32 and the comparison is `torch.equal`.  The 10-bit formats run a second
    time with 2^-2 * identity (still exact), where only code values above 1020 clamp; garbage in bits 10..15 is ignored; for 4:4:4 the
    two sitings give equal results."""
    for F, H, W, s in R.shapes(fmt):
        rs = np.random.RandomState(H * W + len(fmt))
        frames = random_frames(rs, fmt, F, H, W)
        coefs = [IDENT] + ([IDENT * np.float32(0.25)] if R.depth(fmt) == 10 else [])
        by_siting = {}
        for siting in R.SITINGS:
            for coef in coefs:
                for h, w in (lr_size(H, W, s), (H, W)):
                    lr, hr = gpu_ingest(frames, fmt, coef, siting, H, W, h, w)
                    want_lr, want_hr, _ = R.ingest(frames, fmt, coef, siting, H, W, h, w)
                    assert np.array_equal(want_hr.astype(np.float32).astype(np.float64), want_hr)   # exactly representable
                    assert lr.shape == (F, h, w, 3) and hr.shape == (F, H, W, 3)
                    assert torch.equal(hr, torch.from_numpy(want_hr.astype(np.float32))), (F, H, W, siting, h, w)
                    assert torch.equal(lr, torch.from_numpy(want_lr.astype(np.float32))), (F, H, W, siting, h, w)
            by_siting[siting] = (lr, hr)
            if R.depth(fmt) == 10:   # the garbage bits are ignored: the same clip with those bits clear gives the same result
                clean = R.pack(*R.unpack(frames, fmt, H, W), fmt)
                assert not np.array_equal(clean, frames)
                a, b = gpu_ingest(frames, fmt, coefs[1], siting, H, W, H, W), gpu_ingest(clean, fmt, coefs[1], siting, H, W, H, W)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        same = torch.equal(by_siting["left"][1], by_siting["center"][1])
        assert same if not R.is422(fmt) else (not same or W <= 2)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_write_identity_coefficients_is_the_filter_bit_for_bit(fmt):
    """Integer-valued RGB under identity coefficients: the luma plane is R, the chroma planes are G and B (4:4:4) or their filtered
    rows (4:2:2: multiples of 1/4, exact in float32 in any order), rounded with ties to even -- bytes compared exactly.  The 10-bit
    formats run a second time with 4 * identity (codes up to 1020)."""
    for F, H, W, _ in R.shapes(fmt):
        rs = np.random.RandomState(H * W + len(fmt) + 1)
        rgb = rs.randint(0, 256, (F, H, W, 3)).astype(np.float32)
        got_by = {}
        for siting in R.SITINGS:
            for coef in [IDENT] + ([IDENT * np.float32(4)] if R.depth(fmt) == 10 else []):
                vals = R.write_values(rgb, coef, siting, fmt)
                if coef is IDENT and R.is422(fmt) and F * H * W >= 100:
                    assert sum(int((np.abs(v - np.floor(v) - 0.5) == 0).sum()) for v in vals[1:]) > 0, "the case holds no tie"
                got = driver.pix_write(torch.from_numpy(rgb).cuda(), fmt, coef, siting).cpu().numpy()
                want = R.write(rgb, fmt, coef, siting)
                assert got.shape == (F, R.frame_bytes(fmt, H, W)) and np.array_equal(got, want), (F, H, W, siting, np.flatnonzero(got != want)[:8])
            got_by[siting] = got
        if not R.is422(fmt):
            assert np.array_equal(got_by["left"], got_by["center"])


# ------------------------------------------------------------------------------------------------ 2. real coefficients
@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_real_coefficients_within_three_roundings(fmt, matrix, full_range):
    """The kernel evaluates fma(A2, Cr', fma(A1, Cb', fma(A0, Yc, o))) on exact inputs: three roundings, one per fma, each at most half
    an ulp of its result; the clamp moves no value away from the reference's.  Every partial sum stays below 1024 in magnitude
    (asserted on the float64 partial sums), where half an ulp is at most 2^-15 = 3.05e-5: |error| <= 3 * 2^-15 = 9.2e-5 < 1e-4."""
    coef = driver.pix_coefficients(fmt, matrix, full_range, inverse=True)
    worst = 0.0
    for F, H, W, s in R.shapes(fmt):
        rs = np.random.RandomState(H + W)
        frames = random_frames(rs, fmt, F, H, W)
        for siting in R.SITINGS:
            for h, w in (lr_size(H, W, s), (H, W)):
                lr, hr = gpu_ingest(frames, fmt, coef, siting, H, W, h, w)
                want_lr, want_hr, big = R.ingest(frames, fmt, coef, siting, H, W, h, w)
                assert big < 1024.0
                assert not torch.isnan(hr).any() and hr.min() >= 0 and hr.max() <= 255
                e = max(np.abs(hr.numpy().astype(np.float64) - want_hr).max(), np.abs(lr.numpy().astype(np.float64) - want_lr).max())
                worst = max(worst, e)
                assert e <= 1e-4, (F, H, W, siting, h, w, e)
    print(f"[pix ingest {fmt} {matrix} full_range={full_range}] max |error| {worst:.3e} (bound 1e-4)")


@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_write_real_coefficients_equal_rint_of_float64_except_near_ties(fmt, matrix, full_range):
    """The code equals rint of the float64 value, except where that value lies within eps = 5e-5 * 2^(d-8) of a tie: there one code of
    difference is allowed.  eps is the bound derived in tests/test_gpu_yuv.py for the 4:2:0 filter; the 4:2:2 filter has fewer roundings
    (LEFT (l + r), + 2c, times 1/4; CENTER one sum, times 1/2 -- no second row) and 4:4:4 none before the three fmas.  Such samples
    may be at most 2 % of a case: a condition on the inputs (`_pix_ref.write_case`), which tests/test_pix_ref_helper.py checks on the
    reference alone for these seeds."""
    coef = driver.pix_coefficients(fmt, matrix, full_range)
    d = R.depth(fmt)
    eps = 2.0 ** (d - 8) * 5e-5
    n_near = n_diff = 0
    for F, H, W in R.write_shapes(fmt):
        rgb = R.write_case(F, H, W)
        for siting in R.SITINGS:
            vals = R.write_values(rgb, coef, siting, fmt)
            raw = driver.pix_write(torch.from_numpy(rgb).cuda(), fmt, coef, siting).cpu().numpy()
            got = R.unpack(raw, fmt, H, W)
            near_total = 0
            for v, g in zip(vals, got):
                want = R.quantise(v, fmt)
                near = R.near_tie(v, eps)
                near_total += int(near.sum())
                assert np.array_equal(g[~near], want[~near]), (F, H, W, siting, int((g != want)[~near].sum()))
                assert (np.abs(g - want)[near] <= 1).all()
                n_diff += int((g != want).sum())
            n_near += near_total
            assert near_total <= 0.02 * sum(v.size for v in vals), "construction error: too many samples within eps of a tie"
            if d == 10:   # the high 6 bits of every word are zero
                assert not (raw[:, 1::2] & 0xFC).any()
    print(f"[pix write {fmt} {matrix} full_range={full_range}] eps {eps:.1e}: {n_near} samples near a tie, {n_diff} of them one code off")


# ------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_round_trip_returns_the_input_bytes(fmt, matrix, full_range):
    """In-gamut codes with one chroma pair per frame (up-sampling and filtering then change nothing): ingest at h == H and write-out
    give the input bytes back.  Luma 48..200, chroma within 10 of neutral (times 2^(d-8)): every R'G'B' value stays inside 0..255, the
    float32 errors of the two matrices (1e-4 each way) are far from the half code that would change a byte."""
    m = 2 ** (R.depth(fmt) - 8)
    for F, H, W, _ in R.shapes(fmt):
        rs = np.random.RandomState(H + 3 * W)
        Wc = R.chroma_width(fmt, W)
        Yc = rs.randint(48 * m, 200 * m + 1, (F, H, W))
        cb, cr = rs.randint(118 * m, 138 * m + 1, F), rs.randint(118 * m, 138 * m + 1, F)
        frames = R.pack(Yc, np.broadcast_to(cb[:, None, None], (F, H, Wc)), np.broadcast_to(cr[:, None, None], (F, H, Wc)), fmt)
        t = torch.from_numpy(frames).cuda().view(F, 1, -1).expand(F, 3, -1).contiguous()
        for siting in R.SITINGS:
            data, target, hf = driver.ingest_item_pix(t, (H, W), fmt, scale=1, matrix=matrix, full_range=full_range, siting=siting)
            assert data.shape == (F, 3, H, W, 3) and target.shape == (F, 1, H, W, 3) and hf.shape == (F, 3, H, W, 3)
            assert torch.equal(data, hf) and torch.equal(target[:, 0], hf[:, 1]) and target.data_ptr() != hf[:, 1].data_ptr()
            assert hf.min() > 0 and hf.max() < 255
            back = driver.frames_to_pix(hf, fmt, matrix=matrix, full_range=full_range, siting=siting)
            assert back.shape == (F, 3, frames.shape[1])
            assert np.array_equal(back[:, 2].cpu().numpy(), frames), (F, H, W, siting)


# ------------------------------------------------------------------------------------------------ 4. the 4:2:0 kernels against these
@pytest.mark.parametrize("fmt422,fmt420", [("yuv422p", "yuv420p"), ("yuv422p10le", "yuv420p10le")])
def test_old_kernels_against_new_on_the_equal_rows_constructions(fmt422, fmt420):
    """The constructions of tests/test_pix_ref_helper.py on the device: a 4:2:2 frame all of whose chroma rows are one row ingests to
    what `yuv_ingest` makes of the 4:2:0 frame with that row (`torch.equal`: the same fma nest on the same exact inputs), and an RGB clip
    whose rows come in equal pairs writes 4:2:2 chroma rows equal to the 4:2:0 chroma row, the luma planes being equal.  Through the
    pix_* functions a 4:2:0 name gives `yuv_*`'s bytes."""
    top = 2 ** R.depth(fmt422)
    for F, H, W in ((2, 6, 10), (2, 4, 16), (1, 6, 520)):
        rs = np.random.RandomState(W)
        Yc = rs.randint(0, top, (F, H, W))
        cb, cr = rs.randint(0, top, (F, 1, W // 2)), rs.randint(0, top, (F, 1, W // 2))
        f420 = torch.from_numpy(Y420.pack(Yc, np.repeat(cb, H // 2, 1), np.repeat(cr, H // 2, 1), fmt420)).cuda()
        f422 = torch.from_numpy(R.pack(Yc, np.repeat(cb, H, 1), np.repeat(cr, H, 1), fmt422)).cuda()
        half = rs.uniform(-20, 280, (F, H // 2, W, 3)).astype(np.float32)
        half.reshape(-1)[:6] = R.SPECIAL
        rgb = torch.from_numpy(np.repeat(half, 2, axis=1)).cuda()
        for matrix, full_range in COLOUR[1:5:3]:
            inv, fwd = driver.pix_coefficients(fmt422, matrix, full_range, inverse=True), driver.pix_coefficients(fmt422, matrix, full_range)
            for siting in R.SITINGS:
                for lr_shape in ((H // 2, W // 2), (H, W)):
                    a = driver.pix_ingest(f422, (H, W), fmt422, inv, siting, lr_shape, want_hr=True)
                    b = driver.yuv_ingest(f420, (H, W), fmt420, inv, siting, lr_shape, want_hr=True)
                    c = driver.pix_ingest(f420, (H, W), fmt420, inv, siting, lr_shape, want_hr=True)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])
                w2 = driver.pix_write(rgb, fmt422, fwd, siting).cpu().numpy()
                w0 = driver.yuv_write(rgb, fmt420, fwd, siting).cpu().numpy()
                assert np.array_equal(driver.pix_write(rgb, fmt420, fwd, siting).cpu().numpy(), w0)
                y2, cb2, cr2 = R.unpack(w2, fmt422, H, W)
                y0, cb0, cr0 = Y420.unpack(w0, fmt420, H, W)
                assert np.array_equal(y2, y0)
                for c2, c0 in ((cb2, cb0), (cr2, cr0)):
                    assert np.array_equal(c2[:, 0::2], c0) and np.array_equal(c2[:, 1::2], c0), (F, H, W, siting)


# ------------------------------------------------------------------------------------------------ alignment: element accesses, no refusal
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_frames_at_unaligned_addresses_take_the_element_paths(fmt):
    """A clip whose base address allows no wide access (8-bit: odd; 16-bit: even but not a multiple of 4) at widths that would
    otherwise take the wide paths: the same values, and on write-out not a byte outside the frames."""
    off = 2 if R.depth(fmt) == 10 else 1
    coef_in, coef_out = driver.pix_coefficients(fmt, inverse=True), driver.pix_coefficients(fmt)
    for F, H, W in ((2, 4, 16), (2, 6, 12), (2, 3, 8)):
        rs = np.random.RandomState(W)
        frames = random_frames(rs, fmt, F, H, W)
        n = frames.size
        buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        buf[off:off + n] = torch.from_numpy(frames.reshape(-1)).cuda()
        view = buf[off:off + n].view(F, -1)
        assert view.data_ptr() % 4 == off
        rgb = torch.from_numpy(rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)).cuda()
        for siting in R.SITINGS:
            lr, hr = driver.pix_ingest(view, (H, W), fmt, coef_in, siting, (H // 2, W // 2), want_hr=True)
            lr0, hr0 = driver.pix_ingest(torch.from_numpy(frames).cuda(), (H, W), fmt, coef_in, siting, (H // 2, W // 2), want_hr=True)
            assert torch.equal(lr, lr0) and torch.equal(hr, hr0)
            out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            driver.pix_write(rgb, fmt, coef_out, siting, out=out[off:off + n].view(F, -1))
            assert torch.equal(out[off:off + n].view(F, -1), driver.pix_write(rgb, fmt, coef_out, siting))
            assert (out[:off] == 0xA5).all() and (out[off + n:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 5. poisoned buffers
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_poisoned_buffers_every_byte_written_and_nothing_else(fmt):
    """Outputs allocated through tests/_poison.py (all-ones: NaN in float32, guard bands either side): afterwards no element holds the
    pattern, the values equal the run on ordinary buffers, the bands and the round-up slack are intact; the byte after the last
    frame of a write-out into a larger buffer is untouched under both fills."""
    coef_in, coef_out = driver.pix_coefficients(fmt, inverse=True), driver.pix_coefficients(fmt)
    for F, H, W, s in R.shapes(fmt):
        rs = np.random.RandomState(H + W + 5)
        frames = torch.from_numpy(random_frames(rs, fmt, F, H, W)).cuda()
        rgb = torch.from_numpy(rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)).cuda()
        for siting in R.SITINGS:
            for h, w in (lr_size(H, W, s), (H, W)):
                plain = driver.pix_ingest(frames, (H, W), fmt, coef_in, siting, (h, w), want_hr=True)
                with poisoned(package_state=False) as arena:   # (frames.py keeps no buffer between calls)
                    lr, hr = driver.pix_ingest(frames, (H, W), fmt, coef_in, siting, (h, w), want_hr=True)
                    assert arena.n_allocated == 2
                    arena.assert_written(lr, "lr")
                    arena.assert_written(hr, "hr")
                    assert not torch.isnan(lr).any() and not torch.isnan(hr).any()
                    assert torch.equal(lr, plain[0]) and torch.equal(hr, plain[1])
                    arena.check()
            plain = driver.pix_write(rgb, fmt, coef_out, siting)
            with poisoned(package_state=False) as arena:
                out = driver.pix_write(rgb, fmt, coef_out, siting)
                assert arena.n_allocated == 1 and arena.find(out) is not None
                assert torch.equal(out, plain)
                arena.check()
            n = plain.numel()
            for fill in (0x00, 0xFF):   # every byte written whatever was there before; the byte after the last frame untouched
                big = torch.full((n + 1,), fill, dtype=torch.uint8, device="cuda")
                driver.pix_write(rgb, fmt, coef_out, siting, out=big[:n].view(F, -1))
                assert torch.equal(big[:n].view(F, -1), plain) and int(big[n]) == fill
