"""`ClipRunner(deinterlace=...)` and the command line's `--deinterlace` against the definition: the run over the interlaced frames equals
the plain run over `deinterlace_clip` of them, byte for byte.  One x2 float32 model for the module; 4 interlaced frames of 128 x 128,
decimated by 2 (LR 64 x 64) and super-resolved by 2, so the output has the source's shape and can be scored."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import VSR, driver, y4m  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

H = W = 128
T = 4
FPS = (30000, 1001)
MODES = [("frame", True), ("frame", False), ("field", True), ("field", False)]


@pytest.fixture(scope="module")
def model():
    m = fill_module_(VSR(upscale_factor=2).eval(), seed=0).cuda()
    m.precision = m.model.precision = "fp32"
    return m


def interlaced(fmt, seed):
    """Interlaced frames uint8 [T, bytes]: 2 T pictures of a moving synthetic clip, the top field of frame t from picture 2 t, the bottom
    field from picture 2 t + 1, woven plane by plane in the packed layout."""
    video = torch.from_numpy(driver.synthetic_video(2 * T, H, W, seed=seed)).cuda().float()
    prog = driver.frames_to_pix(video, fmt).cpu().numpy()
    planes, sb, _ = driver.deint_planes(fmt, H, W)
    woven = prog[0::2].copy()
    for off, rows, cols, comps in planes:
        nb = cols * comps * sb
        a = woven[:, off:off + rows * nb].reshape(T, rows, nb)
        a[:, 1::2] = prog[1::2, off:off + rows * nb].reshape(T, rows, nb)[:, 1::2]
    assert not np.array_equal(woven, prog[0::2])
    return woven


@pytest.fixture(scope="module")
def clips():
    return {fmt: interlaced(fmt, 11) for fmt in ("yuv420p", "yuv422p10le")}


def runner(model, fmt, **kw):
    return driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=2, **kw)


@pytest.fixture(scope="module")
def wanted(model, clips):
    """(fmt, mode, tff) -> the plain run over the clip deinterlaced beforehand: computed once, shared, left unchanged."""
    plain = {fmt: runner(model, fmt) for fmt in clips}
    out = {}
    for fmt, clip in clips.items():
        for mode, tff in MODES:
            want = plain[fmt].run(driver.deinterlace_clip(clip, (H, W), fmt, mode, tff))
            want.setflags(write=False)
            out[fmt, mode, tff] = want
    return out


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
@pytest.mark.parametrize("mode, tff", MODES)
def test_the_deinterlacing_run_equals_the_run_over_the_deinterlaced_clip(model, clips, wanted, fmt, mode, tff):
    clip, want = clips[fmt], wanted[fmt, mode, tff]
    Tp = 2 * T if mode == "field" else T
    fb = driver.pix_frame_bytes(fmt, H, W)
    assert want.shape == (Tp - 2, fb) and len(np.unique(want)) > 16
    for overlap in (True, False):
        r = runner(model, fmt, deinterlace=mode, tff=tff, overlap=overlap)
        got = r.run(clip)
        assert got.shape == want.shape and np.array_equal(got, want), (overlap, int((got != want).sum()))
        assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, Tp - 2, T * r.in_bytes, (Tp - 2) * r.out_bytes)
        assert r.in_bytes == fb and r.h2d_bytes_per_frame == fb and (r.deinterlace, r.tff) == (mode, tff)


def test_run_stream_counts_orders_and_repeats(model, clips, wanted):
    fmt, clip = "yuv420p", clips["yuv420p"]
    r = runner(model, fmt, deinterlace="field", tff=True)
    order, got = [], []

    def sink(j, f):
        order.append(j)
        got.append(f.copy())

    assert r.run_stream(driver.ArraySource(clip), sink) == 2 * T - 2 and order == list(range(2 * T - 2))
    assert np.array_equal(np.stack(got), wanted[fmt, "field", True])
    got.clear()
    assert r.run_stream(driver.ArraySource(clip), sink, frames=2) == 2 and r.frames_in == 2   # the first two frames: four fields
    assert np.array_equal(np.stack(got), runner(model, fmt).run(driver.deinterlace_clip(clip[:2], (H, W), fmt, "field", True)))
    with pytest.raises(ValueError, match="ended before frame 4"):
        r.run_stream(driver.ArraySource(clip), sink, frames=5)
    assert np.array_equal(r.run(clip), wanted[fmt, "field", True])   # ... and the object is usable afterwards


def test_the_field_order_and_the_mode_matter(wanted):
    for fmt in ("yuv420p", "yuv422p10le"):
        assert not np.array_equal(wanted[fmt, "frame", True], wanted[fmt, "frame", False])
        assert not np.array_equal(wanted[fmt, "field", True][:2], wanted[fmt, "frame", True])


@pytest.mark.parametrize("mode, tff", [("frame", True), ("field", False)])
def test_with_scene_detection_and_scores(model, clips, mode, tff):
    """`scene="sad"` and `score=`: outputs, cuts and metrics equal those of the plain run over the deinterlaced clip (the truth of a
    scored run is the deinterlaced frame)."""
    fmt = "yuv420p"
    clip = clips[fmt].copy()
    clip[2:] = interlaced(fmt, 4321)[2:]   # a cut before interlaced frame 2
    pre = driver.deinterlace_clip(clip, (H, W), fmt, mode, tff)
    Tp = pre.shape[0]
    plain = runner(model, fmt, scene="sad", score="y")
    want = plain.run(pre)
    r = runner(model, fmt, scene="sad", score="y", deinterlace=mode, tff=tff)
    got = r.run(clip)
    assert np.array_equal(got, want)
    assert r.cuts.shape == (Tp - 1,) and np.array_equal(r.cuts, plain.cuts) and np.array_equal(r.scene_m, plain.scene_m)
    k = 2 if mode == "frame" else 4   # the progressive pair that straddles the cut
    assert int(np.argmax(r.scene_m)) == k - 1
    assert sorted(r.metrics) == sorted(plain.metrics) == ["psnr", "ssim"]
    for k in r.metrics:
        assert r.metrics[k].shape == (Tp - 2,) and np.array_equal(r.metrics[k], plain.metrics[k])
    serial = runner(model, fmt, scene="sad", score="y", deinterlace=mode, tff=tff, overlap=False)
    assert np.array_equal(serial.run(clip), want) and all(np.array_equal(serial.metrics[k], plain.metrics[k]) for k in plain.metrics)


def test_refusals(model, clips):
    with pytest.raises(ValueError, match="tff is given but the frames are not deinterlaced"):
        runner(model, "yuv420p", tff=True)
    with pytest.raises(ValueError, match="deinterlace must be None, 'frame' or 'field'"):
        runner(model, "yuv420p", deinterlace="weave")
    with pytest.raises(ValueError, match=r"yuv420p 2x128 has a plane of 1 row\(s\)"):
        driver.ClipRunner(model, (2, 128), "yuv420p", "yuv420p", deinterlace="frame")
    r = runner(model, "yuv420p", deinterlace="frame")
    assert r.tff is True
    with pytest.raises(ValueError, match=r"expected uint8 \[T >= 3"):
        r.run(clips["yuv420p"][:2])
    f = runner(model, "yuv420p", deinterlace="field")
    assert f.run(clips["yuv420p"][:2]).shape[0] == 2          # two frames are four fields: two windows
    with pytest.raises(ValueError, match=r"expected uint8 \[T >= 2"):
        f.run(clips["yuv420p"][:1])
    with pytest.raises(ValueError, match="at least 3 progressive frames"):
        f.run_stream(driver.ArraySource(clips["yuv420p"][:1]), lambda j, fr: None)


def _write_interlaced(path, clip, fmt, token):
    tag = {"yuv420p": "420mpeg2", "yuv422p10le": "422p10"}[fmt]
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F{FPS[0]}:{FPS[1]} {token} A1:1 C{tag}\n".encode())
        for fr in clip:
            f.write(y4m.FRAME + fr.tobytes())
    return str(path)


@pytest.mark.parametrize("mode", ["frame", "field"])
def test_command_line_on_an_interlaced_file(model, clips, wanted, tmp_path, capsys, mode):
    fmt = "yuv420p"
    src = _write_interlaced(tmp_path / "in.y4m", clips[fmt], fmt, "It")
    dst = str(tmp_path / "out.y4m")
    Tp = 2 * T if mode == "field" else T
    rate = (FPS[0] * (2 if mode == "field" else 1), FPS[1])
    driver.main(["--input", src, "--output", dst, "--scale-down", "2", "--scale", "2", "--deinterlace", mode])   # (the seeded x2 model: the fixture's)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["deinterlace"], line["tff"], line["frames_out"], line["frames"], line["windows"]) == (mode, True, Tp - 2, T, Tp - 2)
    assert line["fps"] == list(FPS) and line["h2d_bytes_per_frame"] == driver.pix_frame_bytes(fmt, H, W)
    with open(dst, "rb") as f:
        head = f.readline().decode().split()
    assert "Ip" in head and f"F{rate[0]}:{rate[1]}" in head   # progressive; a frame per field doubles the rate
    with y4m.Y4MReader(dst) as r:
        got = np.stack(list(r))
        assert (r.shape, r.fmt, len(r), r.fps) == ((H, W), fmt, Tp - 2, rate)
    assert np.array_equal(got, wanted[fmt, mode, True])
    # without --deinterlace the interlaced header is an error that names the option
    with pytest.raises(ValueError, match=r"--deinterlace frame\|field"):
        driver.main(["--input", src, "--scale-down", "2", "--scale", "2"])
    # --field-order overrides the header
    line = driver.run_file(src, dst, scale_down=2, scale=2, model=model, deinterlace=mode, field_order="bff")
    assert line["tff"] is False and line["frames_out"] == Tp - 2
    with y4m.Y4MReader(dst) as r:
        assert np.array_equal(np.stack(list(r)), wanted[fmt, mode, False])
    # a headerless file: the field order comes from the option, the rate is the default's (doubled per field)
    raw, rawout = str(tmp_path / "clip.yuv"), str(tmp_path / "rawout.y4m")
    clips[fmt].tofile(raw)
    line = driver.run_file(raw, rawout, size=(H, W), pix_fmt=fmt, scale_down=2, scale=2, model=model, deinterlace=mode, field_order="tff")
    assert (line["tff"], line["frames_out"]) == (True, Tp - 2)
    with y4m.Y4MReader(rawout) as r:
        assert r.fps == (25 * (2 if mode == "field" else 1), 1) and np.array_equal(np.stack(list(r)), wanted[fmt, mode, True])
