"""Y'CbCr 4:2:0 frames in and out on the device (include/vsr_hip_yuv.h, driver.yuv_ingest / yuv_write and the functions above them)
against the float64 restatements of tests/_yuv_ref.py, which evaluate the formulas of the header with the float32 coefficients the
kernel received.

Shapes (F, H, W, scale): the smallest that reach every branch of csrc/clip_yuv.hip --
  2 x  6 x 10    a frame is 90 bytes (frames not 4-byte aligned: element accesses); 3 chroma rows, 5 columns: the clamps on both sides
  1 x 14 x 518   259 chroma columns: more than one 256-lane block and a ragged last block (write-out, element path)
  3 x 18 x 26 at scale 4, 1 x 34 x 46 at scale 3   non-integer decimation ratios (as tests/test_gpu_driver.py)
  2 x  6 x 12    W % 4 == 0 but not % 8: the ingest's one-load luma path, the write-out's element path
  2 x  4 x 16    W % 8 == 0: the wide paths of both
  2 x  6 x 8     the wide paths with H * W % 32 == 16: an 8-bit frame is 72 bytes, so frame 1 and its planes start 8 bytes off a
                 multiple of 16 (the wide write-out stores 8 bytes of luma / nv12 chroma and 4 of planar chroma there, never 16)
  1 x  2 x 2064  W / 8 = 258 threads: the wide write-out's second block, ragged; one chroma row (both row clamps at once)
every one also at h == H (the plain conversion), all four formats, both sitings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _yuv_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402

SHAPES = [(2, 6, 10, 2), (1, 14, 518, 2), (3, 18, 26, 4), (1, 34, 46, 3), (2, 6, 12, 2), (2, 4, 16, 2), (2, 6, 8, 2), (1, 2, 2064, 2)]
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
COLOUR = [(m, fr) for m in ("bt601", "bt709", "bt2020") for fr in (False, True)]


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def random_frames(rs, fmt, F, H, W, garbage=True):
    """Random code values over the whole code range, packed; the bits the ingest must ignore (10..15 of yuv420p10le, 0..5 of p010le)
    hold garbage."""
    top = 2 ** R.depth(fmt)
    Y, Cb, Cr = rs.randint(0, top, (F, H, W)), rs.randint(0, top, (F, H // 2, W // 2)), rs.randint(0, top, (F, H // 2, W // 2))
    b = R.pack(Y, Cb, Cr, fmt).copy()
    if garbage and fmt == "yuv420p10le":
        b[:, 1::2] |= (rs.randint(0, 64, b[:, 1::2].shape) << 2).astype(np.uint8)
    if garbage and fmt == "p010le":
        b[:, 0::2] |= rs.randint(0, 64, b[:, 0::2].shape).astype(np.uint8)
    got = R.unpack(b, fmt, H, W)
    assert np.array_equal(got[0], Y) and np.array_equal(got[1], Cb) and np.array_equal(got[2], Cr)
    return b


def gpu_ingest(frames, fmt, coef, siting, H, W, h, w):
    lr, hr = driver.yuv_ingest(torch.from_numpy(frames).cuda(), (H, W), fmt, coef, siting, (h, w), want_hr=True)
    return lr.cpu(), hr.cpu()


# ------------------------------------------------------------------------------------------------ 1. exact, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_identity_coefficients_is_the_interpolation_bit_for_bit(shape, fmt):
    """coef12 = identity, zero offsets: the ingest returns (Y, Cb', Cr') themselves, clamped to 0..255 as the formula says.  The
    up-sampling weights are dyadic, so the float64 interpolation is exactly representable in float32 and the comparison is
    `torch.equal`.  The 10-bit formats carry codes up to 1023, which the clamp at 255 would hide: they run a second time with
    2^-2 * identity (still exact: a multiple of 1/64 below 256), where only code values above 1020 clamp."""
    F, H, W, s = shape
    rs = np.random.RandomState(H * W + len(fmt))
    frames = random_frames(rs, fmt, F, H, W)
    coefs = [IDENT] + ([IDENT * np.float32(0.25)] if R.depth(fmt) == 10 else [])
    for siting in R.SITINGS:
        for coef in coefs:
            for h, w in ((int(H / s), int(W / s)), (H, W)):
                lr, hr = gpu_ingest(frames, fmt, coef, siting, H, W, h, w)
                want_lr, want_hr, _ = R.ingest(frames, fmt, coef, siting, H, W, h, w)
                assert np.array_equal(want_hr.astype(np.float32).astype(np.float64), want_hr)   # exactly representable
                assert lr.shape == (F, h, w, 3) and hr.shape == (F, H, W, 3)
                assert torch.equal(hr, torch.from_numpy(want_hr.astype(np.float32))), (siting, h, w)
                assert torch.equal(lr, torch.from_numpy(want_lr.astype(np.float32))), (siting, h, w)
        if R.depth(fmt) == 10:   # the garbage bits are ignored: the same clip with those bits clear gives the same result
            clean = R.pack(*R.unpack(frames, fmt, H, W), fmt)
            assert not np.array_equal(clean, frames)
            a, b = gpu_ingest(frames, fmt, coefs[1], siting, H, W, H, W), gpu_ingest(clean, fmt, coefs[1], siting, H, W, H, W)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_write_identity_coefficients_is_the_filter_bit_for_bit(shape, fmt):
    """Integer-valued RGB under identity coefficients: the luma plane is R, the chroma planes are the filtered G and B (multiples of
    1/8: exact in float32 in any order), rounded with ties to even -- bytes compared exactly.  The 10-bit formats run a second time
    with 4 * identity (codes up to 1020, ties kept)."""
    F, H, W, _ = shape
    rs = np.random.RandomState(H * W + len(fmt) + 1)
    rgb = rs.randint(0, 256, (F, H, W, 3)).astype(np.float32)
    for siting in R.SITINGS:
        for coef in [IDENT] + ([IDENT * np.float32(4)] if R.depth(fmt) == 10 else []):
            vals = R.write_values(rgb, coef, siting)
            ties = sum(int((np.abs(v - np.floor(v) - 0.5) == 0).sum()) for v in vals[1:])
            if coef is IDENT:   # (4 x a multiple of 1/4 is an integer: the CENTER filter has no tie under 4 * identity)
                assert ties > 0, "the case holds no tie"
            got = driver.yuv_write(torch.from_numpy(rgb).cuda(), fmt, coef, siting).cpu().numpy()
            want = R.write(rgb, fmt, coef, siting)
            assert got.shape == (F, R.frame_bytes(fmt, H, W)) and np.array_equal(got, want), (siting, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------------------------------------ 2. real coefficients
@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_real_coefficients_within_three_roundings(fmt, matrix, full_range):
    """The kernel evaluates fma(A2, Cr', fma(A1, Cb', fma(A0, Yc, o))) on exact inputs: three roundings, one per fma, each at most half
    an ulp of its result; the clamp moves no value away from the reference's.  Over all code values every partial sum stays below
    1024 in magnitude (asserted on the float64 partial sums: the largest over the twelve coefficient sets and the corners of the code
    cube is 553, full-range codes through a limited-range matrix), where half an ulp is at most 2^-15 = 3.05e-5: |error| <= 3 * 2^-15 = 9.2e-5 < 1e-4."""
    coef = driver.yuv_coefficients(fmt, matrix, full_range, inverse=True)
    worst = 0.0
    for F, H, W, s in SHAPES:
        rs = np.random.RandomState(H + W)
        frames = random_frames(rs, fmt, F, H, W)
        for siting in R.SITINGS:
            for h, w in ((int(H / s), int(W / s)), (H, W)):
                lr, hr = gpu_ingest(frames, fmt, coef, siting, H, W, h, w)
                want_lr, want_hr, big = R.ingest(frames, fmt, coef, siting, H, W, h, w)
                assert big < 1024.0
                assert not torch.isnan(hr).any() and hr.min() >= 0 and hr.max() <= 255
                e = max(np.abs(hr.numpy().astype(np.float64) - want_hr).max(), np.abs(lr.numpy().astype(np.float64) - want_lr).max())
                worst = max(worst, e)
                assert e <= 1e-4, (F, H, W, siting, h, w, e)
    print(f"[yuv ingest {fmt} {matrix} full_range={full_range}] max |error| {worst:.3e} (bound 1e-4)")


WRITE_SHAPES = [(F, H, W) for F, H, W, _ in SHAPES] + [(2, 38, 42)]
SPECIAL = [-3.2, 0.0, 255.0, 255.49, 300.0, float("nan")]


@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_write_real_coefficients_equal_rint_of_float64_except_near_ties(fmt, matrix, full_range):
    """The code equals rint of the float64 value, except where that value lies within eps of a tie: there one code of difference is
    allowed.  eps from the float32 error of the kernel's order, with m = 2^(d-8) and every partial sum below 256 m (offsets 16 m / 128 m
    plus at most 219 m / 112 m; full range at most 255.75 m), where half an ulp is at most 2^-17 * 2 m = 7.6e-6 m:
      luma: three fma roundings on exact (clamped) inputs                                               <= 2.3e-5 m
      chroma: the filter first -- CENTER (a+b), (c+d) below 512: 2^-16 each, their sum below 1024: 2^-15, times 1/4: 1.5e-5;
        LEFT per row (l+r) 2^-16, + 2c below 1024 2^-15, times 1/4: 1.15e-5, the two rows' sum below 512: 2^-16, times 1/2: 1.9e-5 --
        then through gains whose magnitudes sum to at most 1.003 m per row (|Cb row| = gc (Kr + Kg) / (2 (1 - Kb)) + gc / 2 = gc):
        1.9e-5 m, plus the three fma roundings                                                          <= 4.3e-5 m
    eps = 5e-5 m (the issue's ceiling is 1e-3 m).  Such samples may be at most 2 % of a case: a condition on the construction."""
    coef = driver.yuv_coefficients(fmt, matrix, full_range)
    d = R.depth(fmt)
    eps = 2.0 ** (d - 8) * 5e-5
    assert eps <= 2.0 ** (d - 8) * 1e-3
    n_near = n_diff = 0
    for F, H, W in WRITE_SHAPES:
        rs = np.random.RandomState(H * 7 + W)
        rgb = rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)
        rgb.reshape(-1)[:len(SPECIAL)] = SPECIAL
        for siting in R.SITINGS:
            vals = R.write_values(rgb, coef, siting)
            got = R.unpack(driver.yuv_write(torch.from_numpy(rgb).cuda(), fmt, coef, siting).cpu().numpy(), fmt, H, W)
            near_total = 0
            for v, g in zip(vals, got):
                want = R.quantise(v, fmt)
                near = np.abs(v - np.floor(v) - 0.5) < eps
                near_total += int(near.sum())
                assert np.array_equal(g[~near], want[~near]), (F, H, W, siting, int((g != want)[~near].sum()))
                assert (np.abs(g - want)[near] <= 1).all()
                n_diff += int((g != want).sum())
            n_near += near_total
            assert near_total <= 0.02 * (F * H * W * 3 // 2), "construction error: too many samples within eps of a tie"
        if R.depth(fmt) == 10 and fmt == "p010le":   # the low 6 bits of every word are zero
            raw = driver.yuv_write(torch.from_numpy(rgb).cuda(), fmt, coef, "left").cpu().numpy()
            assert not (raw[:, 0::2] & 0x3F).any()
    print(f"[yuv write {fmt} {matrix} full_range={full_range}] eps {eps:.1e}: {n_near} samples near a tie, {n_diff} of them one code off")


# ------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("matrix,full_range", COLOUR, ids=_ids)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_round_trip_returns_the_input_bytes(fmt, matrix, full_range):
    """In-gamut codes with one chroma pair per frame (up-sampling and filtering then change nothing): ingest at h == H and write-out
    give the input bytes back.  Luma 48..200, chroma within 10 of neutral (times 2^(d-8)): every R'G'B' value stays inside 0..255, the
    float32 errors of the two matrices (1e-4 each way) are far from the half code that would change a byte."""
    m = 2 ** (R.depth(fmt) - 8)
    for F, H, W, _ in SHAPES:
        rs = np.random.RandomState(H + 3 * W)
        Y = rs.randint(48 * m, 200 * m + 1, (F, H, W))
        cb, cr = rs.randint(118 * m, 138 * m + 1, F), rs.randint(118 * m, 138 * m + 1, F)
        Cb = np.broadcast_to(cb[:, None, None], (F, H // 2, W // 2))
        Cr = np.broadcast_to(cr[:, None, None], (F, H // 2, W // 2))
        frames = R.pack(Y, Cb, Cr, fmt)
        t = torch.from_numpy(frames).cuda().view(F, 1, -1).expand(F, 3, -1).contiguous()
        for siting in R.SITINGS:
            data, target, hf = driver.ingest_item_yuv(t, (H, W), fmt, scale=1, matrix=matrix, full_range=full_range, siting=siting)
            assert data.shape == (F, 3, H, W, 3) and target.shape == (F, 1, H, W, 3) and hf.shape == (F, 3, H, W, 3)
            assert torch.equal(data, hf) and torch.equal(target[:, 0], hf[:, 1]) and target.data_ptr() != hf[:, 1].data_ptr()
            assert hf.min() > 0 and hf.max() < 255
            back = driver.frames_to_yuv(hf, fmt, matrix=matrix, full_range=full_range, siting=siting)
            assert back.shape == (F, 3, frames.shape[1])
            assert np.array_equal(back[:, 2].cpu().numpy(), frames), (F, H, W, siting)


def test_ingest_item_yuv_shapes_and_lr_only():
    F, H, W = 2, 18, 26
    frames = torch.from_numpy(random_frames(np.random.RandomState(1), "nv12", F * 3, H, W)).cuda().view(F, 3, -1)
    data, target, hf = driver.ingest_item_yuv(frames, (H, W), "nv12", 4)
    assert data.shape == (F, 3, 4, 6, 3) and target.shape == (F, 1, H, W, 3) and hf.shape == (F, 3, H, W, 3)
    coef = driver.yuv_coefficients("nv12", inverse=True)
    want_lr, want_hr, _ = R.ingest(frames.cpu().numpy().reshape(F * 3, -1), "nv12", coef, "left", H, W, 4, 6)
    assert np.abs(data.cpu().numpy().reshape(F * 3, 4, 6, 3) - want_lr).max() <= 1e-4
    assert np.abs(hf.cpu().numpy().reshape(F * 3, H, W, 3) - want_hr).max() <= 1e-4
    d2, t2, h2 = driver.ingest_item_yuv(frames, (H, W), "nv12", 4, want_hr=False)
    assert t2 is None and h2 is None and torch.equal(d2, data)
    with pytest.raises(ValueError):
        driver.ingest_item_yuv(frames[:, :2], (H, W), "nv12", 4)
    with pytest.raises(ValueError):
        driver.yuv_ingest(frames[..., :-1].contiguous(), (H, W), "nv12", coef)


# ------------------------------------------------------------------------------------------------ alignment: element accesses, no refusal
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_frames_at_unaligned_addresses_take_the_element_paths(fmt):
    """A clip whose base address allows no wide access (8-bit: odd; 16-bit: even but not a multiple of 4) at widths that would
    otherwise take the wide paths: the same values, and on write-out not a byte outside the frames."""
    off = 2 if R.depth(fmt) == 10 else 1
    coef_in, coef_out = driver.yuv_coefficients(fmt, inverse=True), driver.yuv_coefficients(fmt)
    for F, H, W in ((2, 4, 16), (2, 6, 12)):
        rs = np.random.RandomState(W)
        frames = random_frames(rs, fmt, F, H, W)
        n = frames.size
        buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        buf[off:off + n] = torch.from_numpy(frames.reshape(-1)).cuda()
        view = buf[off:off + n].view(F, -1)
        assert view.data_ptr() % 4 == off
        rgb = torch.from_numpy(rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)).cuda()
        for siting in R.SITINGS:
            lr, hr = driver.yuv_ingest(view, (H, W), fmt, coef_in, siting, (H // 2, W // 2), want_hr=True)
            lr0, hr0 = driver.yuv_ingest(torch.from_numpy(frames).cuda(), (H, W), fmt, coef_in, siting, (H // 2, W // 2), want_hr=True)
            assert torch.equal(lr, lr0) and torch.equal(hr, hr0)
            out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            driver.yuv_write(rgb, fmt, coef_out, siting, out=out[off:off + n].view(F, -1))
            assert torch.equal(out[off:off + n].view(F, -1), driver.yuv_write(rgb, fmt, coef_out, siting))
            assert (out[:off] == 0xA5).all() and (out[off + n:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 4. poisoned buffers
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_poisoned_buffers_every_byte_written_and_nothing_else(fmt):
    """Outputs allocated through tests/_poison.py (all-ones: NaN in float32, guard bands either side): afterwards no element holds the
    pattern, the values equal the run on ordinary buffers, the bands and the round-up slack are intact; the byte after the last
    frame of a write-out into a larger buffer is untouched."""
    coef_in, coef_out = driver.yuv_coefficients(fmt, inverse=True), driver.yuv_coefficients(fmt)
    for F, H, W, s in SHAPES:
        rs = np.random.RandomState(H + W + 5)
        frames = torch.from_numpy(random_frames(rs, fmt, F, H, W)).cuda()
        # (0xFF is a legitimate byte of a frame, so the uint8 output is compared with the run on ordinary buffers and its bands are
        # checked; it is not scanned for the pattern)
        rgb = torch.from_numpy(rs.uniform(-20, 280, (F, H, W, 3)).astype(np.float32)).cuda()
        for siting in R.SITINGS:
            for h, w in ((int(H / s), int(W / s)), (H, W)):
                plain = driver.yuv_ingest(frames, (H, W), fmt, coef_in, siting, (h, w), want_hr=True)
                with poisoned(package_state=False) as arena:   # (driver.py keeps no buffer between calls)
                    lr, hr = driver.yuv_ingest(frames, (H, W), fmt, coef_in, siting, (h, w), want_hr=True)
                    assert arena.n_allocated == 2
                    arena.assert_written(lr, "lr")
                    arena.assert_written(hr, "hr")
                    assert not torch.isnan(lr).any() and not torch.isnan(hr).any()
                    assert torch.equal(lr, plain[0]) and torch.equal(hr, plain[1])
                    arena.check()
            plain = driver.yuv_write(rgb, fmt, coef_out, siting)
            with poisoned(package_state=False) as arena:   # (driver.py keeps no buffer between calls)
                out = driver.yuv_write(rgb, fmt, coef_out, siting)
                assert arena.n_allocated == 1 and arena.find(out) is not None
                assert torch.equal(out, plain)
                arena.check()
            n = plain.numel()
            for fill in (0x00, 0xFF):   # every byte written whatever was there before; the byte after the last frame untouched
                big = torch.full((n + 1,), fill, dtype=torch.uint8, device="cuda")
                driver.yuv_write(rgb, fmt, coef_out, siting, out=big[:n].view(F, -1))
                assert torch.equal(big[:n].view(F, -1), plain) and int(big[n]) == fill


# ------------------------------------------------------------------------------------------------ 5. the streamed clip runner
def test_clip_runner_overlapped_equals_serial_equals_the_item_loop(gpu_vsr):
    """A 6-frame 256x256 nv12 clip, decimated by 4 and super-resolved by 4: the overlapped runner, the serial one, a second run of
    the same object and `run_item` on windows built by `ingest_item_yuv` give the same bytes; every source frame crosses to the
    device once."""
    H = W = 256
    fmt = "nv12"
    fb = driver.yuv_frame_bytes(fmt, H, W)
    video = torch.from_numpy(driver.synthetic_video(6, H, W, seed=7)).cuda().float()
    clip = driver.frames_to_yuv(video, fmt).cpu().numpy()
    assert clip.shape == (6, fb)

    over = driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4, overlap=True)
    a = over.run(clip)
    assert a.dtype == np.uint8 and a.shape == (4, fb)
    assert over.frames_in == 6 and over.h2d_bytes == 6 * fb and over.h2d_bytes_per_frame == fb   # not three times it
    assert over.frames_out == 4 and over.d2h_bytes == 4 * fb
    a2 = over.run(clip)   # slot reuse: the second run of the same object ...
    serial = driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4, overlap=False)
    b = serial.run(clip)  # ... equals a fresh object's
    assert np.array_equal(a, b) and np.array_equal(a2, b)
    assert over.h2d_bytes_per_frame == fb and serial.h2d_bytes_per_frame == fb
    assert over.frames_in == 6 and over.h2d_bytes == 6 * fb and over.d2h_bytes == 4 * fb   # the counters are per run

    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(4)])).cuda()
    data, target, hf = driver.ingest_item_yuv(windows, (H, W), fmt, scale=4, want_hr=False)
    assert data.shape == (4, 3, 64, 64, 3) and target is None and hf is None
    outs, _, _ = driver.run_item(gpu_vsr, data, None, None)
    want = driver.frames_to_yuv(outs, fmt).cpu().numpy()
    for t in range(4):
        assert np.array_equal(a[t], want[t]), t
    assert len(np.unique(a)) > 16   # a picture, not a constant
    with pytest.raises(ValueError):
        over.run(clip[:2])
