"""The YUV4MPEG2 reader and writer (video_super_resolution_amd/y4m.py) and the frame sizes of every name of `PIX_FORMATS`, on the host:
headers spelled out here in ffmpeg's form, every accepted colour tag, every refusal by its message, write-then-read, the frame count
from the file's size."""
import numpy as np
import pytest

from video_super_resolution_amd import driver, y4m

FFMPEG_HEADER = b"YUV4MPEG2 W10 H6 F30000:1001 Ip A1:1 C422p10 XYSCSS=422P10 XCOLORRANGE=LIMITED\n"
ALL_FORMATS = ["yuv420p", "nv12", "yuv420p10le", "p010le", "yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le"]


def _file(tmp_path, header: bytes, frames, name="a.y4m", marker=b"FRAME\n"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(header)
        for fr in frames:
            f.write(marker)
            f.write(bytes(fr))
    return p


def test_frame_bytes_of_all_eight_names():
    assert list(driver.PIX_FORMATS) == ALL_FORMATS
    assert {k: driver.PIX_FORMATS[k] for k in driver.YUV_FORMATS} == driver.YUV_FORMATS
    assert [driver.PIX_FORMATS[k] for k in ALL_FORMATS[4:]] == [0, 1, 2, 3]   # the codes of include/vsr_hip_pix.h
    assert [driver.pix_frame_bytes(f, 6, 10) for f in ALL_FORMATS] == [90, 90, 180, 180, 120, 180, 240, 360]
    assert driver.pix_frame_bytes("yuv422p10le", 2160, 3840) == 2160 * 3840 * 4 and driver.pix_frame_bytes("yuv444p", 2160, 3840) == 2160 * 3840 * 3
    assert driver.pix_frame_bytes("yuv422p", 3, 6) == 36 and driver.pix_frame_bytes("yuv444p", 5, 7) == 105 and driver.pix_frame_bytes("yuv444p10le", 1, 1) == 6
    for f in ALL_FORMATS[:4]:
        assert driver.pix_frame_bytes(f, 6, 10) == driver.yuv_frame_bytes(f, 6, 10)
        with pytest.raises(ValueError, match="even"):
            driver.pix_frame_bytes(f, 5, 10)
    with pytest.raises(ValueError, match="even W"):
        driver.pix_frame_bytes("yuv422p", 6, 9)
    for bad in ((0, 10), (6, -2)):
        with pytest.raises(ValueError, match="positive"):
            driver.pix_frame_bytes("yuv444p", *bad)
    with pytest.raises(ValueError, match="unknown pixel format"):
        driver.pix_frame_bytes("yuv411p", 6, 10)
    # the 4:2:0 functions keep their behaviour: the new names are unknown to them
    assert driver.YUV_FORMATS == {"yuv420p": 0, "nv12": 1, "yuv420p10le": 2, "p010le": 3}
    with pytest.raises(ValueError, match="unknown pixel format"):
        driver.yuv_frame_bytes("yuv422p", 6, 10)
    with pytest.raises(ValueError, match="unknown pixel format"):
        driver.yuv_coefficients("yuv444p")
    # the coefficients depend on the depth alone
    for m in ("bt601", "bt709", "bt2020"):
        for fr in (False, True):
            for inv in (False, True):
                assert np.array_equal(driver.pix_coefficients("yuv422p", m, fr, inv), driver.yuv_coefficients("nv12", m, fr, inv))
                assert np.array_equal(driver.pix_coefficients("yuv444p10le", m, fr, inv), driver.yuv_coefficients("p010le", m, fr, inv))
                assert np.array_equal(driver.pix_coefficients("nv12", m, fr, inv), driver.yuv_coefficients("nv12", m, fr, inv))


def test_ffmpegs_header_and_the_same_tokens_in_another_order(tmp_path):
    fb = driver.pix_frame_bytes("yuv422p10le", 6, 10)
    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, (3, fb)).astype(np.uint8)
    shuffled = b"YUV4MPEG2 XCOLORRANGE=LIMITED C422p10 A1:1 H6 XYSCSS=422P10 F30000:1001 W10 Ip\n"
    for k, header in enumerate((FFMPEG_HEADER, shuffled)):
        with y4m.Y4MReader(_file(tmp_path, header, frames, f"h{k}.y4m")) as r:
            assert r.shape == (6, 10) and r.fmt == "yuv422p10le" and r.siting == "left" and r.full_range is False
            assert r.fps == (30000, 1001) and r.aspect == (1, 1) and len(r) == 3 and r.frame_bytes == fb
            assert sorted(r.extra) == ["XCOLORRANGE=LIMITED", "XYSCSS=422P10"]   # kept verbatim, the unknown one ignored
            buf = np.empty(fb, dtype=np.uint8)
            for i in range(3):
                assert r.read_into(buf) is True and np.array_equal(buf, frames[i])
            assert r.read_into(buf) is False and r.read_into(buf) is False
            r.rewind()
            assert [f.tolist() for f in r] == frames.tolist()
    # what the writer emits for such a clip is ffmpeg's line, byte for byte
    assert y4m.header_line((6, 10), "yuv422p10le", (30000, 1001), "left", False) == FFMPEG_HEADER
    assert y4m.header_line((6, 10), "yuv420p", (25, 1), "center", True, (4, 3)) == \
        b"YUV4MPEG2 W10 H6 F25:1 Ip A4:3 C420jpeg XYSCSS=420JPEG XCOLORRANGE=FULL\n"


TAGS = [("C420jpeg", "yuv420p", "center"), ("C420mpeg2", "yuv420p", "left"), ("C420", "yuv420p", "center"), (None, "yuv420p", "center"),
        ("C420p10", "yuv420p10le", "left"), ("C422", "yuv422p", "left"), ("C422p10", "yuv422p10le", "left"), ("C444", "yuv444p", "left"),
        ("C444p10", "yuv444p10le", "left")]


@pytest.mark.parametrize("tag,fmt,siting", TAGS, ids=[t[0] or "none" for t in TAGS])
def test_every_accepted_tag_with_its_format_siting_and_range(tmp_path, tag, fmt, siting):
    fb = driver.pix_frame_bytes(fmt, 4, 6)
    for rng, full in ((None, False), ("LIMITED", False), ("FULL", True)):
        for interlace in ("Ip ", ""):   # Ip, or no I token
            header = ("YUV4MPEG2 W6 H4 F24:1 " + interlace + "A0:0" + (" " + tag if tag else "") +
                      (" XCOLORRANGE=" + rng if rng else "") + "\n").encode()
            with y4m.Y4MReader(_file(tmp_path, header, [bytes(fb)] * 2)) as r:
                assert (r.fmt, r.siting, r.full_range, r.shape, len(r), r.aspect) == (fmt, siting, full, (4, 6), 2, (0, 0))
            with y4m.Y4MReader(_file(tmp_path, header, [bytes(fb)]), siting="center") as r:   # the caller's siting wins
                assert r.siting == "center"


def test_every_refusal_names_its_token(tmp_path):
    def refuse(tokens, match, **kw):
        with pytest.raises(ValueError, match=match):
            y4m.Y4MReader(_file(tmp_path, ("YUV4MPEG2 " + tokens + "\n").encode(), [bytes(36)]), **kw)

    for t in ("It", "Ib", "Im"):
        refuse(f"W6 H4 F24:1 {t} C420jpeg", f"'{t}'.*interlaced")
    refuse("W6 H4 F24:1 Ip C420paldv", "'C420paldv'.*siting")
    with y4m.Y4MReader(_file(tmp_path, b"YUV4MPEG2 W6 H4 F24:1 Ip C420paldv\n", [bytes(36)]), siting="left") as r:
        assert (r.fmt, r.siting, len(r)) == ("yuv420p", "left", 1)
    for t in ("Cmono", "C411", "C444alpha"):
        refuse(f"W6 H4 F24:1 Ip {t}", f"'{t}'.*out of scope")
    for t, bits in (("C420p12", 12), ("C422p16", 16), ("C444p9", 9), ("C444p14", 14)):
        refuse(f"W6 H4 F24:1 Ip {t}", f"'{t}'.*{bits} bits")
    refuse("W6 H4 F24:1 Ip XCOLORRANGE=WIDE", "XCOLORRANGE=WIDE")
    refuse("W6 F24:1 Ip", "no W / H")
    refuse("W6 H0 F24:1", "'H0'")
    refuse("W6 H4 F24 Ip", "'F24'")
    refuse("W6 H4 F24:1 Q7", "unknown token 'Q7'")
    refuse("W5 H4 F24:1 C422", "even W")          # a shape the layout cannot hold
    refuse("W6 H3 F24:1 C420jpeg", "even")
    refuse("W6 H4 F24:1 C444", "unknown siting", siting="top")
    with pytest.raises(ValueError, match="not a YUV4MPEG2 file"):
        y4m.Y4MReader(_file(tmp_path, b"RIFF....\n", []))
    with pytest.raises(ValueError, match="not a YUV4MPEG2 file"):
        y4m.parse_header(b"YUV4MPEG W6 H4")
    # the writer: planar formats only, a siting its tag can say
    for fmt in ("nv12", "p010le"):
        with pytest.raises(ValueError, match="headerless"):
            y4m.Y4MWriter(str(tmp_path / "x.y4m"), (4, 6), fmt, (24, 1), "left", False)
    with pytest.raises(ValueError, match="no colour tag"):
        y4m.header_line((4, 6), "yuv422p", (24, 1), "center", False)
    with pytest.raises(ValueError, match="even W"):
        y4m.header_line((4, 5), "yuv422p", (24, 1), "left", False)


@pytest.mark.parametrize("fmt", y4m.PLANAR)
def test_write_then_read_gives_the_bytes_back(tmp_path, fmt):
    assert sorted(y4m.PLANAR) == sorted(f for f in ALL_FORMATS if f not in ("nv12", "p010le"))
    H, W = (6, 10)
    fb = driver.pix_frame_bytes(fmt, H, W)
    rs = np.random.RandomState(len(fmt))
    frames = rs.randint(0, 256, (5, fb)).astype(np.uint8)
    for siting, full in (("left", False), ("center", True)):
        if siting == "center" and fmt != "yuv420p" and "444" not in fmt:
            continue   # (Y4M has no tag for it)
        p = str(tmp_path / f"{fmt}_{siting}.y4m")
        with y4m.Y4MWriter(p, (H, W), fmt, (60000, 1001), siting, full, aspect=(16, 15)) as w:
            for j, fr in enumerate(frames):
                w(j, fr) if j % 2 else w.write(fr)   # the sink form and the plain one
            assert w.frames == 5
            with pytest.raises(ValueError, match="uint8 frame"):
                w.write(frames[0][:-1])
        with y4m.Y4MReader(p) as r:
            want_siting = "left" if "444" in fmt else siting
            assert (r.shape, r.fmt, r.siting, r.full_range, r.fps, r.aspect, len(r)) == ((H, W), fmt, want_siting, full, (60000, 1001), (16, 15), 5)
            got = np.stack(list(r))
            assert np.array_equal(got, frames)
            with pytest.raises(ValueError, match="contiguous uint8 array"):
                r.rewind()
                r.read_into(np.empty(fb + 1, dtype=np.uint8))


def test_frame_count_comes_from_the_size_and_damaged_files_are_refused(tmp_path):
    fb = driver.pix_frame_bytes("yuv444p", 5, 7)
    header = b"YUV4MPEG2 W7 H5 F30:1 Ip A1:1 C444\n"
    for n in (0, 1, 7):
        with y4m.Y4MReader(_file(tmp_path, header, [bytes(fb)] * n)) as r:
            assert len(r) == n and (r.read() is None) == (n == 0)
    p = _file(tmp_path, header, [bytes(fb)] * 3)
    data = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(data[:-7])   # a truncated file
    with pytest.raises(ValueError, match="not a whole number of frames"):
        y4m.Y4MReader(p)
    with pytest.raises(ValueError, match="FRAME line with parameters"):
        y4m.Y4MReader(_file(tmp_path, header, [bytes(fb)] * 3, marker=b"FRAME Ix\n"))
    # ... also where only a later frame carries them (the sizes then add up only by accident: 3 more bytes, 3 fewer in the last frame)
    p = _file(tmp_path, header, [bytes(fb)])
    with open(p, "ab") as f:
        f.write(b"FRAME Ix\n" + bytes(fb - 3))
    r = y4m.Y4MReader(p)
    assert len(r) == 2 and r.read() is not None
    with pytest.raises(ValueError, match="FRAME line with parameters"):
        r.read()
    r.close()
    # a headerless clip: the same interface, the count from the size
    raw = str(tmp_path / "clip.yuv")
    np.arange(4 * fb, dtype=np.uint8).tofile(raw)
    rr = y4m.RawReader(raw, (5, 7), "yuv444p")
    buf = np.empty(fb, dtype=np.uint8)
    assert len(rr) == 4 and rr.read_into(buf) and np.array_equal(buf, np.arange(fb, dtype=np.uint8))
    rr.close()
    with pytest.raises(ValueError, match="not a whole number"):
        y4m.RawReader(raw, (5, 6), "yuv444p")
    with y4m.RawWriter(str(tmp_path / "out.yuv"), fb) as w:
        w(0, buf)
    assert open(str(tmp_path / "out.yuv"), "rb").read() == bytes(buf)
