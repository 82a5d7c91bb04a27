"""`ClipRunner.run_stream`: a clip streamed from a source to a sink, frame by frame, against `run` on the same frames as one array, and
the command line's `--input` on top of it.  6-frame 256 x 256 clips, decimated by 4 and super-resolved by 4, as the runner test of
tests/test_gpu_yuv.py."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import driver, y4m  # noqa: E402

H = W = 256
FPS = (30000, 1001)


@pytest.fixture(scope="module")
def video():
    return torch.from_numpy(driver.synthetic_video(6, H, W, seed=7)).cuda().float()


def _clip(video, fmt):
    return driver.frames_to_pix(video, fmt).cpu().numpy()


def _write_y4m(path, clip, fmt, siting="left"):
    with y4m.Y4MWriter(str(path), (H, W), fmt, FPS, siting, False, aspect=(1, 1)) as w:
        for fr in clip:
            w.write(fr)
    return str(path)


def _read_all(path):
    with y4m.Y4MReader(path) as r:
        return r, np.stack(list(r))


def test_run_stream_from_a_y4m_file_into_a_y4m_file_gives_runs_bytes(gpu_vsr, video, tmp_path):
    """Reader -> runner -> writer equals `run(array)`; the sink sees j = 0..3 in order; the counters are `run`'s; overlapped, serial and
    a second run of the same object are equal."""
    fmt = "yuv420p"
    clip = _clip(video, fmt)
    fb = driver.pix_frame_bytes(fmt, H, W)
    src = _write_y4m(tmp_path / "in.y4m", clip, fmt)
    over = driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4, overlap=True)
    want = over.run(clip)
    counters = (over.frames_in, over.h2d_bytes, over.frames_out, over.d2h_bytes)
    assert want.shape == (4, fb) and counters == (6, 6 * fb, 4, 4 * fb) and len(np.unique(want)) > 16

    seen = []
    for k, runner in enumerate((over, over, driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4, overlap=False))):
        dst = str(tmp_path / f"out{k}.y4m")
        with y4m.Y4MReader(src) as reader, y4m.Y4MWriter(dst, runner.out_shape, fmt, reader.fps, reader.siting, reader.full_range) as writer:
            order = []

            def sink(j, frame, writer=writer, order=order):
                assert frame.dtype == np.uint8 and frame.shape == (fb,)
                order.append(j)
                writer(j, frame)

            assert runner.run_stream(reader, sink) == 4
        assert order == [0, 1, 2, 3]
        assert (runner.frames_in, runner.h2d_bytes, runner.frames_out, runner.d2h_bytes) == counters and runner.h2d_bytes_per_frame == fb
        r, got = _read_all(dst)
        assert (r.shape, r.fmt, r.fps, len(r)) == ((H, W), fmt, FPS, 4)
        assert np.array_equal(got, want), k
        seen.append(got)
    # frames=T takes the first T frames of a longer source; a source that ends early is an error, as is a clip below one window
    with y4m.Y4MReader(src) as reader:
        part = []
        assert over.run_stream(reader, lambda j, f: part.append(f.copy()), frames=4) == 2
    assert np.array_equal(np.stack(part), want[:2]) and over.frames_in == 4
    with y4m.Y4MReader(src) as reader, pytest.raises(ValueError, match="ended before frame 6"):
        over.run_stream(reader, lambda j, f: None, frames=7)
    with pytest.raises(ValueError, match="at least 3"):
        over.run_stream(driver.ArraySource(clip[:2]), lambda j, f: None)
    assert np.array_equal(over.run(clip), want)   # ... and the object is usable afterwards


def test_422_10_bit_in_and_444_out_equals_the_item_loop(gpu_vsr, video, tmp_path):
    fmt_in, fmt_out = "yuv422p10le", "yuv444p"
    clip = _clip(video, fmt_in)
    assert clip.shape == (6, H * W * 4)
    src = _write_y4m(tmp_path / "in422.y4m", clip, fmt_in)
    runner = driver.ClipRunner(gpu_vsr, (H, W), fmt_in, fmt_out, scale_down=4)
    assert runner.in_bytes == H * W * 4 and runner.out_bytes == H * W * 3
    out = []
    with y4m.Y4MReader(src) as reader:
        assert (reader.fmt, reader.siting) == (fmt_in, "left")
        runner.run_stream(reader, lambda j, f: out.append(f.copy()))
    out = np.stack(out)
    assert np.array_equal(out, runner.run(clip))
    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(4)])).cuda()
    data, target, hf = driver.ingest_item_pix(windows, (H, W), fmt_in, scale=4, want_hr=False)
    assert data.shape == (4, 3, 64, 64, 3) and target is None and hf is None
    outs, _, _ = driver.run_item(gpu_vsr, data, None, None)
    want = driver.frames_to_pix(outs, fmt_out).cpu().numpy()
    assert want.shape == out.shape and np.array_equal(out, want)
    assert len(np.unique(out)) > 16
    # an output shape the output format cannot hold is refused when the runner is built
    # (__init__ reads the factor and the device of the model only: a x3 stand-in makes 6 x 10 / 2 into 9 x 15)
    x3 = torch.nn.Linear(1, 1).cuda()
    x3.model = torch.nn.Identity()
    x3.model.upscale_factor = 3
    for bad in ("yuv422p", "yuv422p10le", "yuv420p", "nv12"):
        with pytest.raises(ValueError, match=f"9 x 15 do not fit {bad}"):
            driver.ClipRunner(x3, (6, 10), "yuv444p", bad, scale_down=2)
    assert driver.ClipRunner(x3, (6, 10), "yuv422p", "yuv444p10le", scale_down=2).out_bytes == 9 * 15 * 6
    with pytest.raises(ValueError, match="unknown pixel format"):
        driver.ClipRunner(gpu_vsr, (H, W), "yuv411p", fmt_out)


def test_scored_stream_equals_the_scored_run(gpu_vsr, video, tmp_path):
    fmt = "yuv444p10le"
    clip = _clip(video, fmt)
    clip[3:] = _clip(torch.from_numpy(driver.synthetic_video(6, H, W, seed=4321)).cuda().float(), fmt)[3:]   # a cut before frame 3
    src = _write_y4m(tmp_path / "in444.y4m", clip, fmt)
    runner = driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4, score="y", scene="sad")
    want = runner.run(clip)
    metrics, cuts, scene_m = runner.metrics, runner.cuts, runner.scene_m
    assert cuts.shape == (5,) and scene_m.shape == (5,) and scene_m[2] > 2 * max(scene_m[1], scene_m[3])   # the pair (2, 3) stands out
    got = []
    with y4m.Y4MReader(src) as reader:
        runner.run_stream(reader, lambda j, f: got.append(f.copy()))
    assert np.array_equal(np.stack(got), want)
    assert sorted(runner.metrics) == sorted(metrics) == ["psnr", "ssim"]
    for k in metrics:
        assert np.array_equal(runner.metrics[k], metrics[k]) and runner.metrics[k].shape == (4,)
    assert np.array_equal(runner.cuts, cuts) and np.array_equal(runner.scene_m, scene_m)


def test_command_line_input_writes_a_y4m_file_of_the_runners_frames(gpu_vsr, video, tmp_path, capsys):
    fmt = "yuv422p10le"
    clip = _clip(video, fmt)
    src = _write_y4m(tmp_path / "in.y4m", clip, fmt)
    dst = str(tmp_path / "out.y4m")
    driver.main(["--input", src, "--output", dst, "--scale-down", "4", "--scale", "4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["input"] == src and line["frames"] == 6 and line["windows"] == 4 and line["weights"] == "seeded"
    assert (line["pix_fmt_in"], line["pix_fmt_out"], line["siting"], line["full_range"]) == (fmt, fmt, "left", False)
    r, got = _read_all(dst)
    assert (r.shape, r.fmt, r.fps, r.aspect, r.siting, r.full_range, len(r)) == ((H, W), fmt, FPS, (1, 1), "left", False, 4)
    want = driver.ClipRunner(gpu_vsr, (H, W), fmt, fmt, scale_down=4).run(clip)
    assert np.array_equal(got, want)
