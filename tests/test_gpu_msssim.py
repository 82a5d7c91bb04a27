"""Multi-scale SSIM on the device (include/vsr_hip_msssim.h, driver.frame_msssim / msssim / ClipRunner(multiscale=True)) against the
float64 restatement of tests/_msssim_ref.py (pinned by tests/test_msssim_ref_helper.py).

csrc/frame_msssim.hip pools in tiles of 16 x 64 level-1 pixels (no loop inside a tile: the grid walks them), scores every level in tiles
of SW = 64 map columns (a strip) by SR = 64 map rows (a row segment), four input rows per step, the tiles of the five levels in one
grid, and sums a level's per-tile partials with FT = 64 threads.  Shapes (F, H, W, shave), the smallest that reach every branch:
  1 x  161 x  161, 0    the minimum: every level odd (clamped last row and column), level 5 holds one window; 3 x 3 tiles at level 1
                        (map 151 x 151) and 2 x 2 at level 2 (map 71 x 71): the second strip and segment of both; element loads
  2 x  176 x  208, 0    every level even, nothing clamped; two frames; the 16-byte load path (aligned bases, W % 4 == 0)
  1 x  189 x  211, 4    shave and odd sizes: element loads; 181 x 203 -> 91 x 102 -> 46 x 51 -> 23 x 26 -> 12 x 13
  2 x  176 x  208, 0    the same from a flat buffer at a storage offset of one float: bases not 16-byte aligned, element loads
  1 x  516 x 1020, 4    16 x 8 = 128 level-1 tiles > FT: the second trip of the finish kernel's loop; the second strip and segment of
                        level 3 (map 117 x 243) and the second strip of level 4 (map 54 x 117)
  1 x  161 x 1200, 0    w_5 = 75: the second strip of level 5 (map 1 x 65), several strips of level 4
  1 x 1190 x  161, 0    h_4 = 149, h_5 = 75: the second segment of levels 4 and 5 (maps 139 x 11, 65 x 1)
every one in RGB and Y, with quantise 0 and 1.

The scored clip run uses the setup of tests/test_gpu_metric.py at x4: a 5-frame nv12 clip of 256 x 256 (LR 64 x 64), shave 4."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _msssim_ref as M  # noqa: E402
from _poison import poisoned  # noqa: E402
from _score_cases import MODES, _ids, _luma4, images, to_device  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402

SHAPES = [(1, 161, 161, 0, False), (2, 176, 208, 0, False), (1, 189, 211, 4, False), (2, 176, 208, 0, True), (1, 516, 1020, 4, False),
          (1, 161, 1200, 0, False), (1, 1190, 161, 0, False)]
BAR = 1e-10   # the absolute bound tests/test_gpu_metric.py has for a frame's SSIM mean


def plane_size(shape):
    return shape[1] - 2 * shape[3], shape[2] - 2 * shape[3]


@functools.lru_cache(maxsize=None)
def reference(kind, shape, channels, quant):
    """float64 [F,P,5,2] of the restatement, once per case and shared by the tests that need it."""
    a, b = images(kind, shape)
    s = M.sums(a, b, channels, bool(quant), shape[3], _luma4())
    s.setflags(write=False)
    return s


def gpu(a, b, shape, channels, quant):
    got = driver.frame_msssim(to_device(a, shape[4]), to_device(b, shape[4]), channels, bool(quant), shape[3])
    assert got.shape == (shape[0], 3 if channels == "rgb" else 1, 5, 2) and got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the level means
# a textured pair, a near-flat bright pair and Gaussian floats in every mode, the awkward pair (NaN, ties, out of range) where
# quantisation handles it; the two long shapes are there for the loop trips of levels 4 and 5 alone: one image per mode
def _kinds(shape, q):
    if max(shape[1], shape[2]) >= 1100:
        return ("textured",) if q else ("gaussian",)
    return ("textured", "near_flat", "gaussian") + (("awkward",) if q else ())


MEAN_CASES = [(shape, ch, q, kind) for shape in SHAPES for ch, q in MODES for kind in _kinds(shape, q)]


@pytest.mark.parametrize("shape,channels,quant,kind", MEAN_CASES, ids=_ids)
def test_level_means_within_1e_10_of_float64(shape, channels, quant, kind):
    """|sum / n_j - reference| <= 1e-10 for cs and ssim, per frame, plane and level.  Both sides are float64 and pool with the same
    operations in the same order (the pooled planes are the reference's bit for bit); they differ in fma against multiply-add in the
    window sums and in the order of the final sum, as the single-scale metric does: about 3e-12 per position (tests/test_gpu_metric.py),
    and the bar sits more than 3 orders below the smallest planted defect of the helper test.  The means are compared, not the final
    power: its slope is unbounded at 0."""
    a, b = images(kind, shape)
    h, w = plane_size(shape)
    want = M.means(reference(kind, shape, channels, quant), h, w)
    got = M.means(gpu(a, b, shape, channels, quant), h, w)
    err = np.abs(got - want)
    print(f"[msssim {channels} q{quant} {kind} {shape[:4]}] cs means {got[0, 0, :, 0].round(6).tolist()} ssim_5 {got[0, 0, 4, 1]:.6f} "
          f"max |error| per level {err.max(axis=(0, 1, 3)).tolist()} (bar {BAR})")
    assert np.isfinite(got).all()
    assert (err <= BAR).all()


# ------------------------------------------------------------------------------------------------ 2. equal frames
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_equal_frames_give_every_count_exactly_and_msssim_one(shape, channels, quant):
    h, w = plane_size(shape)
    n = M.counts(h, w)
    for kind in (("awkward",) if quant else ("awkward_no_nan", "gaussian")):
        a, _ = images(kind, shape)
        got = gpu(a, a.copy(), shape, channels, quant)
        assert (got[..., 0] == n).all() and (got[..., 1] == n).all(), kind
        assert (driver.msssim(got, h, w) == 1.0).all()


# ------------------------------------------------------------------------------------------------ 3. level 1 is the single-scale SSIM
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_level_1_ssim_is_frame_metrics_ssim(shape, channels, quant):
    """The level-1 ssim sums over the planes, over P n_1, against driver.frame_metrics' SSIM mean: the same formula on the same planes
    with the same window sums, only the partial sums are grouped otherwise (per plane here): within the same 1e-10."""
    kind = "textured" if quant else "gaussian"
    a, b = images(kind, shape)
    ta, tb = to_device(a, shape[4]), to_device(b, shape[4])
    h, w = plane_size(shape)
    got = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3]).cpu().numpy()
    _, ssim = driver.psnr_ssim(driver.frame_metrics(ta, tb, channels, bool(quant), shape[3], "ssim"))
    mine = got[:, :, 0, 1].sum(axis=1) / (got.shape[1] * (h - 10) * (w - 10))
    print(f"[level 1 vs frame_metrics {channels} q{quant} {shape[:4]}] {mine.tolist()} vs {ssim.tolist()}")
    assert (np.abs(mine - ssim) <= BAR).all()


# ------------------------------------------------------------------------------------------------ 4. determinism and batching
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ids)
def test_two_runs_give_the_same_bits_and_a_frame_does_not_depend_on_its_batch(shape, channels, quant):
    kind = "textured" if quant else "gaussian"
    a, b = images(kind, shape)
    ta, tb = to_device(a, shape[4]), to_device(b, shape[4])
    one = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3])
    two = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3])
    assert torch.equal(one, two) and torch.isfinite(one).all()
    for f in range(shape[0]):
        single = driver.frame_msssim(ta[f:f + 1], tb[f:f + 1], channels, bool(quant), shape[3])
        assert torch.equal(single[0], one[f]), f
        assert torch.equal(driver.frame_msssim(ta[f], tb[f], channels, bool(quant), shape[3]), single)   # [H,W,3] is one frame
    # ... nor on its place in the batch: three frames, the pair's in another order with one of them twice
    perm = [1, 0, 1]
    moved = driver.frame_msssim(ta[perm].contiguous(), tb[perm].contiguous(), channels, bool(quant), shape[3])
    assert torch.equal(moved, one[perm])


# ------------------------------------------------------------------------------------------------ 5. poisoned buffers
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[2]], ids=_ids)
def test_poisoned_workspace_and_sums(shape, channels, quant):
    """The workspace and the sums allocated through tests/_poison.py (all-ones: NaN in float64, guard bands either side): the results
    are finite and equal in their bits to the run on ordinary buffers, every element of the sums is written, the bands are intact:
    the library reads nothing of the workspace it has not written and writes nothing outside."""
    kind = "textured" if quant else "gaussian"
    a, b = images(kind, shape)
    ta, tb = to_device(a, False), to_device(b, False)
    plain = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3])
    with poisoned(package_state=False) as arena:   # (frames.py keeps no buffer between calls)
        got = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3])
        assert arena.n_allocated == 2 and arena.find(got) is not None     # the sums and the workspace
        arena.assert_written(got, "sums")
        assert torch.isfinite(got).all() and torch.equal(got, plain)
        arena.check()
    # into rows of a larger tensor: the rows beside them are untouched
    P = got.shape[1]
    big = torch.full((shape[0] + 2, P, 5, 2), -7.0, dtype=torch.float64, device="cuda")
    driver.frame_msssim(ta, tb, channels, bool(quant), shape[3], out=big[1:1 + shape[0]])
    assert torch.equal(big[1:1 + shape[0]], plain)
    assert (big[0] == -7.0).all() and (big[-1] == -7.0).all()


def test_python_surface_refuses_what_the_library_would():
    x = torch.zeros(160, 200, 3, device="cuda")
    with pytest.raises(ValueError, match="161 pixels each way"):
        driver.frame_msssim(x, x)
    y = torch.zeros(176, 200, 3, device="cuda")
    with pytest.raises(ValueError, match="161 pixels each way"):
        driver.frame_msssim(y, y, shave=8)
    with pytest.raises(ValueError, match="unknown channels"):
        driver.frame_msssim(y, y, channels="yuv")
    assert driver.msssim_levels(176, 200) == M.level_sizes(176, 200)


# ------------------------------------------------------------------------------------------------ 6. the scored clip run
def _build(cpu_vsr):
    m = copy.deepcopy(cpu_vsr).cuda().eval()
    m.precision = m.model.precision = "fp32"
    return m


def test_scored_clip_run_multiscale(cpu_vsr):
    """The 5-frame nv12 clip of tests/test_gpu_metric.py at x4 (LR 64 x 64 -> 256 x 256, shave 4), scored on luma and on RGB with
    multiscale=True: `metrics["msssim"]` equals `msssim(frame_msssim(...))` of (the float frames of a `run_item` evaluation of the same
    windows, `yuv_ingest` of source frame j + 1) bit for bit, with and without overlap and with a bicubic baseline; the output bytes, the
    byte counters, `psnr` and `ssim` are those of the run without it."""
    S, fmt, T = 4, "nv12", 5
    H = W = 64 * S
    fb = driver.yuv_frame_bytes(fmt, H, W)
    model = _build(cpu_vsr)
    video = torch.from_numpy(driver.synthetic_video(T, H, W, seed=11)).cuda().float()
    clip = driver.frames_to_yuv(video, fmt).cpu().numpy()

    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(T - 2)])).cuda()
    data, _, _ = driver.ingest_item_yuv(windows, (H, W), fmt, scale=S, want_hr=False)
    outs, _, _ = driver.run_item(model, data, None, None)
    truth, _ = driver.yuv_ingest(torch.from_numpy(clip[1:T - 1]).cuda(), (H, W), fmt, driver.yuv_coefficients(fmt, inverse=True))
    assert truth.shape == outs.shape == (T - 2, H, W, 3)
    h = w = H - 2 * S

    for score in ("y", "rgb"):
        want = driver.msssim(driver.frame_msssim(outs, truth, score, True, S), h, w)
        assert want.shape == (T - 2,) and ((want > 0) & (want < 1)).all()
        without = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score=score)
        want_bytes = without.run(clip)
        assert "msssim" not in without.metrics and without.multiscale is False
        for overlap in (True, False):
            r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=overlap, score=score, multiscale=True)
            assert r.multiscale and r.shave == S
            for again in range(2 if overlap else 1):   # (slot reuse: a second run of the same object)
                got_bytes = r.run(clip)
                assert np.array_equal(got_bytes, want_bytes), (score, overlap)
                assert r.metrics["msssim"].shape == (T - 2,) and "msssim_baseline" not in r.metrics
                assert np.array_equal(r.metrics["msssim"], want), (score, overlap)
                assert np.array_equal(r.metrics["psnr"], without.metrics["psnr"]) and np.array_equal(r.metrics["ssim"], without.metrics["ssim"])
                assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
                assert (without.frames_in, without.frames_out, without.h2d_bytes, without.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
        print(f"[scored clip x{S} {score}] MS-SSIM {want.round(6).tolist()}")

    # with a baseline: the bicubic enlargement of the middle LR frame, scored against the same truth
    score = "y"
    want = driver.msssim(driver.frame_msssim(outs, truth, score, True, S), h, w)
    assert data.shape == (T - 2, 3, H // S, W // S, 3)
    base = driver.FrameResizer((H // S, W // S), (H, W))(data[:, 1].contiguous())
    want_base = driver.msssim(driver.frame_msssim(base, truth, score, True, S), h, w)
    without = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score=score, baseline="bicubic")
    want_bytes = without.run(clip)
    for overlap in (True, False):
        r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=overlap, score=score, baseline="bicubic", multiscale=True)
        assert np.array_equal(r.run(clip), want_bytes)
        assert np.array_equal(r.metrics["msssim"], want) and np.array_equal(r.metrics["msssim_baseline"], want_base), overlap
        for k in ("psnr", "ssim", "psnr_baseline", "ssim_baseline"):
            assert np.array_equal(r.metrics[k], without.metrics[k]), k
        assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
    assert driver.sums_layout(T, "y", "bicubic") == {"estimate": (0, T - 2, "frame"), "baseline": (T - 2, T - 2, "frame")}


def test_multiscale_needs_a_score_and_161_pixels():
    """At x2 the clip of LR 64 x 64 is 128 x 128: too small for five levels, and construction says so before it allocates anything (a
    stand-in with the model's one attribute read by then will do); without `score` it says that."""
    from types import SimpleNamespace
    x2, x4 = (SimpleNamespace(model=SimpleNamespace(upscale_factor=s)) for s in (2, 4))
    with pytest.raises(ValueError, match="161 pixels each way"):
        driver.ClipRunner(x2, (128, 128), "nv12", "nv12", scale_down=2, score="y", multiscale=True)
    with pytest.raises(ValueError, match="needs score"):
        driver.ClipRunner(x4, (256, 256), "nv12", "nv12", scale_down=4, multiscale=True)
    with pytest.raises(ValueError, match="161 pixels each way"):
        driver.ClipRunner(x4, (256, 256), "nv12", "nv12", scale_down=4, score="y", shave=48, multiscale=True)
