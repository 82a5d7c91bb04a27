"""The frame metric on the device (include/vsr_hip_metric.h, driver.frame_metrics / psnr_ssim / ClipRunner(score=...)) against the
float64 restatement of tests/_metric_ref.py (pinned by tests/test_metric_ref_helper.py).

csrc/frame_metric.hip scores a frame in tiles of SW = 64 map columns (a strip) by SR = 64 map rows (a row segment), four input rows per
step, and sums a frame's per-tile partials with FT = 64 threads.  Shapes (F, H, W, shave), the smallest that reach every branch:
  1 x  11 x   11, 0    one window: one map position, one tile
  2 x  12 x   75, 0    65 map columns: one past a strip; a row pitch of 900 bytes is no multiple of 16: element loads; two frames
  1 x  23 x  140, 3    shave; 124 map columns: a ragged second strip; 7 map rows: the ring turns over (17 input rows through 14 slots)
  1 x  75 x   64, 0    SR + 11 rows: 65 map rows, one row past a segment
  3 x  16 x   64, 2    the 16-byte load path: aligned bases, W % 4 == 0; three frames
  2 x  16 x   64, 2    the same from a flat buffer at a storage offset of one float: bases not 16-byte aligned, element loads
  1 x 516 x 1020, 4    16 strips x 8 segments = 128 partials > FT: the second trip of the finish kernel's loop
every one in RGB and Y, with quantise 0 and 1, and for the SSE both alone (tiles without halo) and beside SSIM (tiles with halo: the
last strip and segment own their halo pixels).

The scored clip run uses LR frames of 64 x 64, the smallest VSR.forward accepts (FlowNet2's centre crop to multiples of 64): a 5-frame
nv12 clip of 128 x 128 at x2 and of 256 x 256 at x4."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _metric_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from _score_cases import MODES, _ids, _luma4, images, to_device  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402

SW, SR, FT = 64, 64, 64
SHAPES = [(1, 11, 11, 0, False), (2, 12, 75, 0, False), (1, 23, 140, 3, False), (1, SR + 11, SW, 0, False), (3, 16, 64, 2, False),
          (2, 16, 64, 2, True), (1, 516, 1020, 4, False)]


@functools.lru_cache(maxsize=None)
def reference(kind, shape, channels, quant, want_ssim=True):
    """float64 [F,4] of the restatement, once per case and shared by the tests that need it."""
    a, b = images(kind, shape)
    return R.metrics(a, b, channels, bool(quant), shape[3], _luma4(), want_ssim=want_ssim)


def gpu(a, b, shape, channels, quant, what=("psnr", "ssim")):
    got = driver.frame_metrics(to_device(a, shape[4]), to_device(b, shape[4]), channels, bool(quant), shape[3], what)
    assert got.shape == (shape[0], 4) and got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


def counts(shape, channels):
    F, H, W, s, _ = shape
    P = 3 if channels == "rgb" else 1
    return P * (H - 2 * s) * (W - 2 * s), P * (H - 2 * s - 10) * (W - 2 * s - 10)


# ------------------------------------------------------------------------------------------------ 1. SSE, exact
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sse_of_quantised_rgb_is_the_integer_sum_exactly(shape):
    """quantise = 1, RGB, inputs with values below 0, above 255, NaN and exact .5 ties on both parities: every term is the square of an
    integer difference and every partial sum an integer below 2^53, so any order of summation is exact: sse == the int64 sum, as a
    double.  The quantisation itself is driver.frames_to_u8's."""
    F, H, W, s, _ = shape
    a, b = images("awkward", shape)
    assert np.isnan(a).any() and (a < 0).any() and (a > 255).any()
    ties = a[np.abs(a - np.floor(a) - 0.5) == 0]
    assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any()
    qa = driver.frames_to_u8(to_device(a, False)).cpu().numpy()
    qb = driver.frames_to_u8(to_device(b, False)).cpu().numpy()
    assert np.array_equal(qa, R.quantise(a)) and np.array_equal(qb, R.quantise(b))     # the restatement quantises as write-out does
    d = qa.astype(np.int64) - qb.astype(np.int64)
    want = (d * d)[:, s:H - s, s:W - s].reshape(F, -1).sum(axis=1)
    assert want.max() < 2 ** 53
    n_sse, n_ssim = counts(shape, "rgb")
    for what in ("psnr", ("psnr", "ssim")):
        got = gpu(a, b, shape, "rgb", 1, what)
        print(f"[sse exact {shape[:4]} what={what}] got {got[:, 0].tolist()} want {want.tolist()}")
        assert (got[:, 0] == want.astype(np.float64)).all(), what
        assert (got[:, 1] == n_sse).all()
        if what == "psnr":
            assert (got[:, 2:] == 0).all()
        else:
            assert (got[:, 3] == n_ssim).all() and np.isfinite(got[:, 2]).all()
    assert (reference("awkward", shape, "rgb", 1, False)[:, 0] == want).all()


# ------------------------------------------------------------------------------------------------ 2. SSE, other modes
@pytest.mark.parametrize("channels,quant,kind", [("y", 1, "awkward"), ("y", 0, "awkward_no_nan"), ("rgb", 0, "awkward_no_nan"),
                                                 ("y", 0, "gaussian"), ("rgb", 0, "gaussian")])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sse_other_modes_within_the_summation_bound(shape, channels, quant, kind):
    """The terms are formed as the header says (luma nested in double without contraction, d * d rounded once), so they are the
    reference's bit for bit; only the order of the sum differs and every term is non-negative: |got - fsum| <= (n + 2) 2^-53 fsum."""
    a, b = images(kind, shape)
    want = reference(kind, shape, channels, quant, kind == "gaussian")   # (the gaussian cases share theirs with the SSIM test)
    n_sse, _ = counts(shape, channels)
    for what in ("psnr", ("psnr", "ssim")):
        got = gpu(a, b, shape, channels, quant, what)
        err = np.abs(got[:, 0] - want[:, 0])
        bound = (n_sse + 2) * 2.0 ** -53 * want[:, 0]
        print(f"[sse {channels} q{quant} {kind} {shape[:4]} what={what}] |got - fsum| {err.max():.3e}, bound {bound.min():.3e}")
        assert np.isfinite(got).all() and (want[:, 0] > 0).all()
        assert (err <= bound).all(), (err, bound)
        assert (got[:, 1] == n_sse).all() and (want[:, 1] == n_sse).all()


# ------------------------------------------------------------------------------------------------ 3. SSIM
# a textured pair and a near-flat bright pair (255 against 255 - {0, 1}) in every mode, Gaussian floats where nothing rounds them
# (the largest shape is there for the finish kernel's loop alone: one image per mode, the reference of 1.5 M map positions once each)
SSIM_CASES = [(shape, ch, q, kind) for shape in SHAPES for ch, q in MODES
              for kind in ((("textured", "near_flat") + (() if q else ("gaussian",))) if shape[1] < 500 else (("textured",) if q else ("gaussian",)))]


@pytest.mark.parametrize("shape,channels,quant,kind", SSIM_CASES, ids=_ids)
def test_ssim_frame_mean_within_1e_10_of_float64(shape, channels, quant, kind):
    """|ssim_sum / n_ssim - reference| <= 1e-10.  Both sides are float64; they differ in fma against multiply-add and in the order of
    the final sum.  Per moment the relative error is at most about 24 * 2^-53 on values up to 65025, divided by C2 = 58.5: about 3e-12
    per pixel; the bar leaves 30 x over that and sits more than 3 orders below the smallest planted defect of the helper test (7.0e-7)."""
    a, b = images(kind, shape)
    want = reference(kind, shape, channels, quant)
    _, n_ssim = counts(shape, channels)
    got = gpu(a, b, shape, channels, quant)
    only = gpu(a, b, shape, channels, quant, "ssim")
    err = np.abs(got[:, 2] / got[:, 3] - want[:, 2] / want[:, 3])
    print(f"[ssim {channels} q{quant} {kind} {shape[:4]}] ssim {got[:, 2] / got[:, 3]} |error| {err.max():.3e} (bar 1e-10)")
    assert (got[:, 3] == n_ssim).all() and (want[:, 3] == n_ssim).all()
    assert (err <= 1e-10).all()
    assert np.array_equal(only[:, 2:], got[:, 2:]) and (only[:, :2] == 0).all()      # SSIM alone: the same bits, the SSE slots 0


# ------------------------------------------------------------------------------------------------ 4. equal frames
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_equal_frames_give_zero_sse_and_ssim_exactly_one(shape, channels, quant):
    n_sse, n_ssim = counts(shape, channels)
    for kind in (("awkward",) if quant else ("awkward_no_nan", "gaussian")):
        a, _ = images(kind, shape)
        got = gpu(a, a.copy(), shape, channels, quant)
        assert (got[:, 0] == 0.0).all() and (got[:, 1] == n_sse).all()
        assert (got[:, 2] == got[:, 3]).all() and (got[:, 3] == n_ssim).all(), kind
        psnr, ssim = driver.psnr_ssim(got)
        assert np.isposinf(psnr).all() and (ssim == 1.0).all()


# ------------------------------------------------------------------------------------------------ 5. determinism and batching
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]], ids=_ids)
def test_two_runs_give_the_same_bits_and_a_frame_does_not_depend_on_its_batch(shape, channels, quant):
    kind = "textured" if quant else "gaussian"
    a, b = images(kind, shape)
    ta, tb = to_device(a, shape[4]), to_device(b, shape[4])
    one = driver.frame_metrics(ta, tb, channels, bool(quant), shape[3])
    two = driver.frame_metrics(ta, tb, channels, bool(quant), shape[3])
    assert torch.equal(one, two) and torch.isfinite(one).all()
    for f in range(shape[0]):
        single = driver.frame_metrics(ta[f:f + 1], tb[f:f + 1], channels, bool(quant), shape[3])
        assert torch.equal(single[0], one[f]), f
        assert torch.equal(driver.frame_metrics(ta[f], tb[f], channels, bool(quant), shape[3]), single)   # [H,W,3] is one frame
    if shape[0] == 3:   # ... nor on its place in the batch
        perm = [2, 0, 1]
        moved = driver.frame_metrics(ta[perm].contiguous(), tb[perm].contiguous(), channels, bool(quant), shape[3])
        assert torch.equal(moved, one[perm])


# ------------------------------------------------------------------------------------------------ 6. poisoned buffers
@pytest.mark.parametrize("channels,quant", MODES, ids=_ids)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=_ids)
def test_poisoned_workspace_and_sums(shape, channels, quant):
    """The workspace and the sums allocated through tests/_poison.py (all-ones: NaN in float64, guard bands either side): the results
    are finite and equal in their bits to the run on ordinary buffers, every slot is written (0 where not asked for), the bands are
    intact: the library reads nothing of the workspace it has not written and writes nothing outside."""
    kind = "textured" if quant else "gaussian"
    a, b = images(kind, shape)
    ta, tb = to_device(a, False), to_device(b, False)
    for what in (("psnr", "ssim"), "psnr", "ssim"):
        plain = driver.frame_metrics(ta, tb, channels, bool(quant), shape[3], what)
        with poisoned(package_state=False) as arena:   # (driver.py keeps no buffer between calls)
            got = driver.frame_metrics(ta, tb, channels, bool(quant), shape[3], what)
            assert arena.n_allocated == 2 and arena.find(got) is not None     # the sums and the workspace
            arena.assert_written(got, "sums")
            assert torch.isfinite(got).all() and torch.equal(got, plain), what
            if what == "psnr":
                assert (got[:, 2:] == 0).all()
            if what == "ssim":
                assert (got[:, :2] == 0).all()
            arena.check()
    # into a row of a larger tensor: the rows beside it are untouched
    big = torch.full((shape[0] + 2, 4), -7.0, dtype=torch.float64, device="cuda")
    driver.frame_metrics(ta, tb, channels, bool(quant), shape[3], out=big[1:1 + shape[0]])
    assert torch.equal(big[1:1 + shape[0]], driver.frame_metrics(ta, tb, channels, bool(quant), shape[3]))
    assert (big[0] == -7.0).all() and (big[-1] == -7.0).all()


# ------------------------------------------------------------------------------------------------ 7. the scored clip run
_masters = {}


def _vsr_master(cpu_vsr, scale):
    from video_super_resolution_amd import VSR
    from video_super_resolution_amd.weights import fill_module_
    if scale == 4:
        return cpu_vsr
    if scale not in _masters:
        m = VSR(upscale_factor=scale).eval()
        m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
        fill_module_(m.model, seed=0, prefix="model.")
        _masters[scale] = m
    return _masters[scale]


def _build(cpu_vsr, scale):
    m = copy.deepcopy(_vsr_master(cpu_vsr, scale)).cuda().eval()
    m.precision = m.model.precision = "fp32"
    return m


@pytest.mark.parametrize("scale", [2, 4])
def test_scored_clip_run(cpu_vsr, scale):
    """A 5-frame nv12 clip whose LR frames are 64 x 64, decimated and super-resolved by S, scored on luma and on RGB: the runner's
    metrics equal `frame_metrics` of (the float frames of a `run_item` evaluation of the same windows, `yuv_ingest` of source frame
    j + 1) bit for bit, with and without overlap; scoring changes neither the output bytes nor the byte counters; under poisoned
    buffers (the runner's HR buffer, the sums, the workspace) the same bits again."""
    S, fmt, T = scale, "nv12", 5
    H = W = 64 * S
    fb = driver.yuv_frame_bytes(fmt, H, W)
    model = _build(cpu_vsr, S)
    video = torch.from_numpy(driver.synthetic_video(T, H, W, seed=11)).cuda().float()
    clip = driver.frames_to_yuv(video, fmt).cpu().numpy()

    plain = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S)
    assert plain.score is None
    want_bytes = plain.run(clip)
    assert plain.metrics is None

    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(T - 2)])).cuda()
    data, _, _ = driver.ingest_item_yuv(windows, (H, W), fmt, scale=S, want_hr=False)
    outs, _, _ = driver.run_item(model, data, None, None)
    assert outs.shape == (T - 2, H, W, 3) and outs.dtype == torch.float32
    truth, _ = driver.yuv_ingest(torch.from_numpy(clip[1:T - 1]).cuda(), (H, W), fmt, driver.yuv_coefficients(fmt, inverse=True))
    assert truth.shape == outs.shape

    for score in ("y", "rgb"):
        want = driver.frame_metrics(outs, truth, score, True, S)
        want_psnr, want_ssim = driver.psnr_ssim(want)
        assert np.isfinite(want_psnr).all() and ((want_ssim > -1) & (want_ssim < 1)).all()
        for overlap in (True, False):
            r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=overlap, score=score)
            assert r.shave == S
            for again in range(2 if overlap else 1):   # (slot reuse: a second run of the same object)
                got_bytes = r.run(clip)
                assert np.array_equal(got_bytes, want_bytes), (score, overlap)
                assert r.metrics["psnr"].shape == r.metrics["ssim"].shape == (T - 2,)
                assert np.array_equal(r.metrics["psnr"], want_psnr) and np.array_equal(r.metrics["ssim"], want_ssim), (score, overlap)
                assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
                assert (plain.frames_in, plain.frames_out, plain.h2d_bytes, plain.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
        print(f"[scored clip x{S} {score}] PSNR {want_psnr.round(3).tolist()} dB, SSIM {want_ssim.round(5).tolist()}")
    shaved = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", shave=0)
    shaved.run(clip)
    p0, s0 = driver.psnr_ssim(driver.frame_metrics(outs, truth, "y", True, 0))
    assert np.array_equal(shaved.metrics["psnr"], p0) and np.array_equal(shaved.metrics["ssim"], s0)

    if S == 4:
        want_psnr, want_ssim = driver.psnr_ssim(driver.frame_metrics(outs, truth, "y", True, S))
        with poisoned() as arena:
            m = _build(cpu_vsr, S)   # a fresh object: its caches are born inside the block
            r = driver.ClipRunner(m, (H, W), fmt, fmt, scale_down=S, score="y")
            assert arena.find(r._truth) is not None
            got_bytes = r.run(clip)
            assert np.array_equal(got_bytes, want_bytes)
            assert np.isfinite(r.metrics["psnr"]).all() and np.isfinite(r.metrics["ssim"]).all()
            assert np.array_equal(r.metrics["psnr"], want_psnr) and np.array_equal(r.metrics["ssim"], want_ssim)
            arena.check()
