"""Host-side checks of the deinterlacer's Python side (no GPU): the plane tables of every layout against `pix_frame_bytes` and against
the restatement's own layouts, the properties of the rule the header states (on the restatement, tests/_deint_ref.py, which the GPU
tests then compare the kernel with bit for bit), the margin of the rule over weave on the project's synthetic clip, the neighbours and
parities of a clip (`deint_schedule`), y4m's `interlaced` argument and the refusals of the command line."""
import numpy as np
import pytest

import _deint_ref as R
from video_super_resolution_amd import driver, y4m
from video_super_resolution_amd.clip_runner import ClipRunner

SIZES = {"420": [(4, 6), (6, 10)], "422": [(4, 6), (6, 10), (3, 6)], "444": [(4, 6), (6, 10), (3, 6), (5, 7)]}
FLAGS = [(0, 1), (0, 0), (1, 1), (1, 0)]   # (keep, kept_first)


def _chroma(fmt):
    return "422" if "422" in fmt else "444" if "444" in fmt else "420"


# ------------------------------------------------------------------------------------------------ 1. plane tables
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_plane_tables_tile_the_frame_and_equal_the_layouts_definition(fmt):
    assert sorted(R.FORMATS) == sorted(driver.PIX_FORMATS)
    for H, W in SIZES[_chroma(fmt)]:
        planes, sb, shift = driver.deint_planes(fmt, H, W)
        fb = driver.pix_frame_bytes(fmt, H, W)
        assert sb == (2 if fmt.endswith("10le") else 1) and shift == (6 if fmt == "p010le" else 0)
        at = 0
        for off, rows, cols, comps in planes:   # in order, back to back, no gap
            assert off == at and rows > 0 and cols > 0 and comps == (2 if fmt in ("nv12", "p010le") and off else 1)
            at += rows * cols * comps * sb
        assert at == fb
        ref, rsb, rshift, rfb = R.layout(fmt, H, W)
        assert (rsb, rshift, rfb) == (sb, shift, fb)
        assert [(o, r, c * k) for o, r, c, k in planes] == ref
    # the odd offsets the header speaks of
    assert [p[0] for p in driver.deint_planes("yuv422p", 3, 6)[0]] == [0, 18, 27]
    assert [p[0] for p in driver.deint_planes("yuv444p", 5, 7)[0]] == [0, 35, 70]


def test_plane_tables_refuse_what_the_layout_cannot_hold():
    with pytest.raises(ValueError, match="unknown pixel format"):
        driver.deint_planes("rgb24", 4, 6)
    with pytest.raises(ValueError, match="even"):
        driver.deint_planes("yuv420p", 5, 6)
    with pytest.raises(ValueError, match="even W"):
        driver.deint_planes("yuv422p", 4, 7)


# ------------------------------------------------------------------------------------------------ 2. the rule's properties
def words(rs, shape, bits):
    return rs.randint(0, 2 ** bits, size=shape).astype(np.uint16 if bits == 16 else np.uint8)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("keep, kept_first", FLAGS)
def test_restatement_properties_on_random_words(bits, keep, kept_first):
    rs = np.random.RandomState(bits + 2 * keep + kept_first)
    for rows, n in ((2, 5), (3, 4), (7, 33), (16, 16)):
        P, C, N = (words(rs, (rows, n), bits) for _ in range(3))
        out = R.deint_plane(P, C, N, keep, kept_first)
        assert out.dtype == C.dtype and out.shape == C.shape
        assert np.array_equal(out[keep::2], C[keep::2])                        # kept rows are copies
        lo = np.minimum(np.minimum(P, C), N).min(axis=0)                       # per column: a sample meets only its own column
        hi = np.maximum(np.maximum(P, C), N).max(axis=0)
        assert (out >= lo).all() and (out <= hi).all()                         # within the input range: no overflow, no clamp
        assert np.array_equal(R.deint_plane(C, C, C, keep, kept_first), C)     # the static clip is the identity (weave)
        # a column alone gives the same column: nothing crosses columns (comps = 2 needs no rule of its own)
        j = n // 2
        assert np.array_equal(R.deint_plane(P[:, j:j + 1], C[:, j:j + 1], N[:, j:j + 1], keep, kept_first), out[:, j:j + 1])
        # the three inputs that are not read do not matter: the missing-parity rows of the far neighbour
        far = N if kept_first else P
        far2 = far.copy()
        far2[1 - keep::2] = words(rs, far2[1 - keep::2].shape, bits)
        again = R.deint_plane(P, C, far2, keep, kept_first) if kept_first else R.deint_plane(far2, C, N, keep, kept_first)
        assert np.array_equal(again, out)


@pytest.mark.parametrize("keep, kept_first", FLAGS)
def test_restatement_with_the_p010_shift(keep, kept_first):
    rs = np.random.RandomState(7 + keep)
    P, C, N = (words(rs, (6, 9), 16) for _ in range(3))                        # full-range words: the low 6 bits are set too
    out = R.deint_plane(P, C, N, keep, kept_first, shift=6)
    assert np.array_equal(out[keep::2], C[keep::2])                            # bit copies, low bits included
    assert (out[1 - keep::2] & 63 == 0).all()                                  # rebuilt words: the value in the high 10 bits, low bits 0
    assert np.array_equal(out[1 - keep::2] >> 6, R.deint_plane(P >> 6, C >> 6, N >> 6, keep, kept_first)[1 - keep::2])
    still = R.deint_plane(C, C, C, keep, kept_first, shift=6)
    assert np.array_equal(still >> 6, C >> 6) and np.array_equal(still[keep::2], C[keep::2])


def test_a_hand_worked_sample():
    # one column, rows 0..2, keep = 0, kept_first = 1: row 1 is rebuilt from c = C[0], e = C[2], b = P[1], a = C[1]
    P = np.array([[10], [100], [30]], dtype=np.uint8)
    C = np.array([[20], [60], [40]], dtype=np.uint8)
    N = np.array([[22], [0], [44]], dtype=np.uint8)
    # t = 80, sp = 30, td0 = 40, td1 = (10 + 10) >> 1 = 10, td2 = (2 + 4) >> 1 = 3, d = max(20, 10, 3) = 20, v = clamp(30, 60, 100) = 60
    assert R.deint_plane(P, C, N, 0, 1)[:, 0].tolist() == [20, 60, 40]
    # kept_first = 0: b = C[1] = 60, a = N[1] = 0: t = 30, td0 = 60, d = 30, v = clamp(30, 0, 60) = 30
    assert R.deint_plane(P, C, N, 0, 0)[:, 0].tolist() == [20, 30, 40]
    # keep = 1: rows 0 and 2 are rebuilt, both with yu = yd = 1 (reflection): c = e = 60, sp = 60
    # row 0, kept_first = 1: b = 10, a = 20, t = 15, td0 = 10, td1 = (40 + 40) >> 1 = 40, td2 = 60, d = 60, v = clamp(60, -45, 75) = 60
    # row 2: b = 30, a = 40, t = 35, td0 = 10, d = 60, v = clamp(60, -25, 95) = 60
    assert R.deint_plane(P, C, N, 1, 1)[:, 0].tolist() == [60, 60, 60]


# ------------------------------------------------------------------------------------------------ 3. the margin over weave
def test_the_rule_beats_weave_by_ten_db_on_every_frame_of_the_synthetic_clip():
    """`synthetic_video(12, 64, 96, seed=0)` interlaced as 6 frames (the top field of frame t from picture 2 t, the bottom field from
    picture 2 t + 1), every channel a plane, one progressive frame per field: each of the 12 against its true picture.  Measured when the
    rule was chosen: 45.1 .. 46.9 dB for the rule, 27.8 .. 28.0 dB for the woven frame; the test asks for 10 dB between them."""
    v = driver.synthetic_video(12, 64, 96, seed=0)
    T = 6
    woven = np.empty((T,) + v.shape[1:], dtype=np.uint8)
    woven[:, 0::2] = v[0::2, 0::2]
    woven[:, 1::2] = v[1::2, 1::2]

    def psnr(a, b):
        return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))

    for q, (p, i, n, keep, kept_first) in enumerate(driver.deint_schedule(T, "field", tff=True)):
        got = np.stack([R.deint_plane(woven[p, :, :, c], woven[i, :, :, c], woven[n, :, :, c], keep, kept_first) for c in range(3)], axis=-1)
        rule, weave = psnr(got, v[q]), psnr(woven[i], v[q])
        assert rule >= weave + 10.0, (q, rule, weave)


# ------------------------------------------------------------------------------------------------ 4. the clip's schedule
def test_schedule_reflects_at_both_ends_and_orders_the_fields_in_time():
    S = driver.deint_schedule
    assert driver.DEINTERLACE == (None, "frame", "field") and ClipRunner.DEINTERLACE == driver.DEINTERLACE
    assert S(4, "frame") == [(1, 0, 1, 0, 1), (0, 1, 2, 0, 1), (1, 2, 3, 0, 1), (2, 3, 2, 0, 1)]        # the OTHER neighbour, not the frame
    assert S(4, "frame", tff=False) == [(1, 0, 1, 1, 1), (0, 1, 2, 1, 1), (1, 2, 3, 1, 1), (2, 3, 2, 1, 1)]
    assert S(1, "frame") == [(0, 0, 0, 0, 1)] and S(1, "field", tff=False) == [(0, 0, 0, 1, 1), (0, 0, 0, 0, 0)]
    assert S(2, "frame") == [(1, 0, 1, 0, 1), (0, 1, 0, 0, 1)]
    assert S(3, "field") == [(1, 0, 1, 0, 1), (1, 0, 1, 1, 0), (0, 1, 2, 0, 1), (0, 1, 2, 1, 0), (1, 2, 1, 0, 1), (1, 2, 1, 1, 0)]
    for T in (1, 2, 3, 5):
        for tff in (True, False):
            assert [(p, n) for p, _, n, _, _ in S(T, "frame", tff)] == [R.neighbours(i, T) for i in range(T)]
            field = S(T, "field", tff)
            assert len(field) == 2 * T and field[0::2] == S(T, "frame", tff)
            assert all(a[:3] == b[:3] and b[3] == 1 - a[3] and (a[4], b[4]) == (1, 0) for a, b in zip(field[0::2], field[1::2]))
    for bad in (None, "bob", "weave"):
        with pytest.raises(ValueError, match="'frame' or 'field'"):
            S(3, bad)
    with pytest.raises(ValueError, match="at least one frame"):
        S(0, "frame")


def test_the_restated_clip_follows_the_same_schedule():
    rs = np.random.RandomState(3)
    H, W, fmt = 4, 6, "yuv420p"
    frames = rs.randint(0, 256, size=(3, driver.pix_frame_bytes(fmt, H, W))).astype(np.uint8)
    for mode in ("frame", "field"):
        for tff in (True, False):
            want = np.stack([R.deint_frame(frames[p], frames[i], frames[n], (H, W), fmt, k, kf)
                             for p, i, n, k, kf in driver.deint_schedule(3, mode, tff)])
            assert np.array_equal(R.deint_clip(frames, (H, W), fmt, mode, tff), want)
    one = R.deint_clip(frames[:1], (H, W), fmt, "frame")   # T = 1: both neighbours are the frame itself: weave, the identity
    assert np.array_equal(one, frames[:1])


# ------------------------------------------------------------------------------------------------ 5. y4m
def test_y4m_interlaced_argument_every_token_and_both_defaults():
    head = "YUV4MPEG2 W6 H4 F30000:1001 %sA1:1 C420mpeg2"
    for token, tff in (("It ", True), ("Ib ", False), ("Ip ", None), ("", None)):
        info = y4m.parse_header((head % token).encode(), interlaced=True)
        assert info["tff"] is tff and info["shape"] == (4, 6) and info["fmt"] == "yuv420p" and info["fps"] == (30000, 1001)
    with pytest.raises(ValueError, match=r"'Im'.*mixed"):
        y4m.parse_header((head % "Im ").encode(), interlaced=True)
    with pytest.raises(ValueError, match=r"'Ix'.*interlaced clips are out of scope"):
        y4m.parse_header((head % "Ix ").encode(), interlaced=True)
    # the default: today's refusal, word for word, and progressive headers as before (tff None)
    for token in ("It", "Ib", "Im"):
        for kwargs in ({}, {"interlaced": False}):
            with pytest.raises(ValueError) as e:
                y4m.parse_header((head % (token + " ")).encode(), **kwargs)
            assert str(e.value) == f"Y4M header: {token!r}: interlaced clips are out of scope (only Ip, or no I token)"
    assert y4m.parse_header((head % "Ip ").encode())["tff"] is None and y4m.parse_header((head % "").encode())["tff"] is None


def _write_y4m(path, token, frames, H=4, W=6):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F25:1 {token}A1:1 C420mpeg2\n".encode())
        for fr in frames:
            f.write(b"FRAME\n" + fr.tobytes())


def test_y4m_reader_passes_the_argument_on_and_the_writer_stays_progressive(tmp_path):
    frames = np.arange(3 * 36, dtype=np.uint8).reshape(3, 36)
    for token, tff in (("It ", True), ("Ib ", False), ("Ip ", None), ("", None)):
        path = str(tmp_path / f"clip_{token.strip() or 'none'}.y4m")
        _write_y4m(path, token, frames)
        with y4m.Y4MReader(path, interlaced=True) as r:
            assert r.tff is tff and len(r) == 3 and np.array_equal(np.stack(list(r)), frames)   # the frames as they lie in the file
        if tff is None:
            with y4m.Y4MReader(path) as r:
                assert r.tff is None
        else:
            with pytest.raises(ValueError, match="interlaced clips are out of scope"):
                y4m.Y4MReader(path)
    assert b" Ip " in y4m.header_line((4, 6), "yuv420p", (50, 1), "left", False)
    raw = str(tmp_path / "clip.yuv")
    frames.tofile(raw)
    r = y4m.RawReader(raw, (4, 6), "yuv420p")
    assert r.tff is None
    r.close()


# ------------------------------------------------------------------------------------------------ 6. refusals that need no device
def test_command_line_refusals(tmp_path, capsys):
    frames = np.zeros((3, 36), dtype=np.uint8)
    it, ip, raw = (str(tmp_path / n) for n in ("it.y4m", "ip.y4m", "clip.yuv"))
    _write_y4m(it, "It ", frames)
    _write_y4m(ip, "Ip ", frames)
    frames.tofile(raw)

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            driver.main(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err

    refused(["--deinterlace", "frame"], "--deinterlace needs --input")
    refused(["--field-order", "tff"], "--field-order needs --deinterlace")
    refused(["--input", it, "--field-order", "bff"], "--field-order needs --deinterlace")
    refused(["--input", raw, "--size", "4x6", "--pix-fmt", "yuv420p", "--deinterlace", "field"], "needs --field-order tff|bff")
    refused(["--input", it, "--deinterlace", "frame", "--train-steps", "1"], "takes no --deinterlace")
    refused(["--input", it, "--deinterlace", "bob"], "invalid choice")
    refused(["--input", it, "--deinterlace", "frame", "--field-order", "top"], "invalid choice")
    # an interlaced header without --deinterlace: an error that names the option, raised before the device is touched
    with pytest.raises(ValueError, match=r"interlaced \(It\): pass --deinterlace frame\|field"):
        driver.main(["--input", it])
    # a header that does not say which field comes first, and no --field-order
    with pytest.raises(ValueError, match=r"--deinterlace needs --field-order tff\|bff"):
        driver.main(["--input", ip, "--deinterlace", "frame"])
    with pytest.raises(ValueError, match="field_order must be None, 'tff' or 'bff'"):
        driver.run_file(it, deinterlace="frame", field_order="top")
    with pytest.raises(ValueError, match="field_order is given but the clip is not deinterlaced"):
        driver.run_file(ip, field_order="tff")


def test_clip_runner_refuses_a_field_order_without_deinterlacing_and_an_unknown_mode():
    # (both are refused before the model is looked at)
    with pytest.raises(ValueError, match="tff is given but the frames are not deinterlaced"):
        ClipRunner(None, (4, 6), "yuv420p", "yuv420p", tff=True)
    with pytest.raises(ValueError, match="tff is given"):
        ClipRunner(None, (4, 6), "yuv420p", "yuv420p", tff=False)
    with pytest.raises(ValueError, match="deinterlace must be None, 'frame' or 'field'"):
        ClipRunner(None, (4, 6), "yuv420p", "yuv420p", deinterlace="bob")
