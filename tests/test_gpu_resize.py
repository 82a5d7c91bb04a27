"""The table-driven resampler on the device (include/vsr_hip_resize.h, driver.resize_frames / FrameResizer / ClipRunner(decimate=,
baseline=)) against the float64 restatement of tests/_resize_ref.py (pinned by tests/test_resize_ref_helper.py).

csrc/frame_resize.hip gives a workgroup a tile of TW = 32 output columns by TH = 16 output rows and takes the tile's rows in groups whose
source rows fit 80 rows of LDS; 16-byte stores where dst is 16-byte aligned and w % 4 == 0, element stores otherwise.  Geometries
(H, W) -> (h, w), the smallest that reach every branch:
   48 x  64 -> 12 x 16   x4 down, 17 taps, the 16-byte route          45 x 63 -> 15 x 21   x3, 13 taps, odd w: element stores
   44 x  60 -> 22 x 30   x2, 9 taps, two tile rows                    37 x 53 -> 12 x 16   a non-integer ratio, 15 taps
   12 x  16 -> 48 x 64   x4 up, 5 taps, 3 x 2 tiles                   13 x 17 -> 26 x 34   x2 up, odd everything, a second tile column of 2
    9 x  11 ->  9 x 11   1 : 1                                         7 x  5 ->  1 x  1   one output pixel
    3 x   2 ->  1 x  1 and 2 x 3 -> 8 x 12: a source narrower than the taps: the clamp works on both sides
   (TH -+ 1) x (TW -+ 1) outputs at x2: one pixel short of a tile and one past it, each way
   20 x 138 -> 10 x 69   an output wider than two tiles
  136 x  40 -> 17 x  5   x8 down, 33 taps: a tile's 16 rows need 153 source rows, so three groups per tile, and a second tile row
with F = 1 and 3, and from flat buffers at a storage offset of one float (4-byte alignment only).

The clip run uses LR frames of 64 x 64, the smallest VSR.forward accepts: a 5-frame nv12 clip of 256 x 256 at x4."""
import copy
import functools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _exact as E  # noqa: E402
import _resize_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import _lib, driver  # noqa: E402


def _define(name):
    with open(_lib.RESIZEHEADER_PATH) as f:
        return int(re.search(rf"#define {name} (\d+)", f.read()).group(1))


TW, TH = _define("VSR_RESIZE_TILE_W"), _define("VSR_RESIZE_TILE_H")
GEOMS = [(48, 64, 12, 16), (45, 63, 15, 21), (44, 60, 22, 30), (37, 53, 12, 16), (12, 16, 48, 64), (13, 17, 26, 34), (9, 11, 9, 11), (7, 5, 1, 1),
         (3, 2, 1, 1), (2, 3, 8, 12),
         (2 * (TH - 1), 2 * (TW - 1), TH - 1, TW - 1), (2 * (TH + 1), 2 * (TW + 1), TH + 1, TW + 1),
         (2 * (TH - 1), 2 * (TW + 1), TH - 1, TW + 1), (2 * (TH + 1), 2 * (TW - 1), TH + 1, TW - 1),
         (20, 4 * TW + 10, 10, 2 * TW + 5), (136, 40, 17, 5)]
OFFSET_GEOMS = [(48, 64, 12, 16), (45, 63, 15, 21), (12, 16, 48, 64)]   # the first and last take 16-byte stores when aligned
CASES = [(g, F, False) for g in GEOMS for F in (1, 3)] + [(g, 3, True) for g in OFFSET_GEOMS]


def _ids(v):
    if isinstance(v, tuple) and len(v) == 3 and isinstance(v[0], tuple):
        return "x".join(map(str, v[0])) + f"-F{v[1]}" + ("-off4" if v[2] else "")
    return "x".join(str(int(i)) for i in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def real_case(geom, F, kernel="bicubic"):
    """Random float32 pixels in 0..255, the float32 tables of the restatement, the float64 result and its bound: made once, read-only."""
    H, W, h, w = geom
    src = np.random.RandomState(H * 131 + W + 7 * F).uniform(0.0, 255.0, size=(F, H, W, 3)).astype(np.float32)
    yf, yw = R.tables(H, h, kernel)
    xf, xw = R.tables(W, w, kernel)
    ref, bound = R.resize64(src, xf, xw, yf, yw)
    for a in (src, xf, xw, yf, yw, ref, bound):
        a.setflags(write=False)
    return dict(src=src, xf=xf, xw=xw, yf=yf, yw=yw, ref=ref, bound=bound)


def to_device(x, offset=False):
    """The array on the device; `offset`: inside a flat buffer at a storage offset of one float (4 bytes past a 16-byte boundary)."""
    t = torch.tensor(np.asarray(x))   # (a copy: the cached arrays are read-only)
    if not offset:
        return t.cuda()
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    buf[1:1 + t.numel()] = t.reshape(-1).cuda()
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def device_run(case, out_shape, quantise, offset=False, out=None):
    src = to_device(case["src"], offset)
    tabs = [to_device(case[k]) for k in ("xf", "xw", "yf", "yw")]
    if out is None and offset:
        F = src.shape[0]
        n = F * out_shape[0] * out_shape[1] * 3
        buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
        out = buf[1:1 + n].view(F, out_shape[0], out_shape[1], 3)
        got = driver.resize_frames(src, out_shape, *tabs, quantise=quantise, out=out)
        assert torch.isnan(buf[0]) and torch.isnan(buf[1 + n:]).all()   # nothing either side of the view
        return got
    return driver.resize_frames(src, out_shape, *tabs, quantise=quantise, out=out)


# ------------------------------------------------------------------------------------------------ 1. exact
EXACT = [(2, 20, 30, TH + 1, TW + 1, 5, 3, 1), (1, 9, 70, 35, 2 * TW + 5, 17, 7, 2), (3, 50, 7, 40, 5, 1, 33, 3), (1, 6, 6, 16, 36, 33, 33, 4),
         (2, 100, 12, TH, 8, 2, 17, 5)]


@functools.lru_cache(maxsize=None)
def exact_case(spec):
    F, H, W, h, w, KX, KY, seed = spec
    return R.exact_case(np.random.RandomState(seed), F, H, W, h, w, KX, KY)


@pytest.mark.parametrize("spec", EXACT, ids=_ids)
def test_exact(spec):
    """Integer pixels, dyadic sparse weights without a unit sum, firsts in no order and beyond both ends: float32 cannot round, so every
    summation order and tiling equals float64 bit for bit; a wrong tap, a wrong clamp or a tile seam does not."""
    case = exact_case(spec)
    h, w = spec[3], spec[4]
    for offset in (False, True):
        got = device_run(case, (h, w), False, offset)
        E.assert_exact(got, torch.from_numpy(case["ref"]), f"resize {spec} offset {offset}", names="fyxc")
        gotq = device_run(case, (h, w), True, offset)
        E.assert_exact(gotq, torch.from_numpy(R.quantise64(case["ref"])), f"resize quantised {spec} offset {offset}", names="fyxc")
    assert (case["ref"] < 0).any() and (case["ref"] > 255).any()   # the unquantised mode showed values outside 0..255 as they are


def test_exact_reports_a_planted_defect_with_coordinates():
    """One weight off by one unit (2^-4) and one first off by one, planted in the helper's copy of the tables: the comparison fails and
    names the column, or the row, the defect sits in."""
    spec = EXACT[0]
    case = exact_case(spec)
    got = device_run(case, (spec[3], spec[4]), False)
    E.assert_exact(got, torch.from_numpy(case["ref"]), "undamaged", names="fyxc")
    xd = int(np.argmax((case["xw"] != 0).sum(axis=1)))               # a column with live taps
    xw = case["xw"].copy()
    xw[xd, int(np.argmax(case["xw"][xd] != 0))] += 2.0 ** -4
    bad, _ = R.resize64(case["src"], case["xf"], xw, case["yf"], case["yw"], want_bound=False)
    m = E.diff_mask(got, torch.from_numpy(bad))
    assert int(m.sum()) > 0 and E.bbox(m)[2] == (xd, xd)
    with pytest.raises(AssertionError, match=rf"first at \(f=\d+, y=\d+, x={xd}, c=\d\).*x {xd}\.\.{xd}"):
        E.assert_exact(got, torch.from_numpy(bad), "weight defect", names="fyxc")
    inside = np.nonzero((case["yf"] > 0) & (case["yf"] + spec[6] < spec[1]) & ((case["yw"] != 0).sum(axis=1) > 0))[0]
    yd = int(inside[0])                                              # a row whose taps all lie inside: shifting it moves every tap
    yf = case["yf"].copy()
    yf[yd] += 1
    bad, _ = R.resize64(case["src"], case["xf"], case["xw"], yf, case["yw"], want_bound=False)
    m = E.diff_mask(got, torch.from_numpy(bad))
    assert int(m.sum()) > 0 and E.bbox(m)[1] == (yd, yd)
    with pytest.raises(AssertionError, match=rf"y {yd}\.\.{yd}"):
        E.assert_exact(got, torch.from_numpy(bad), "first defect", names="fyxc")


# ------------------------------------------------------------------------------------------------ 2. real tables, float results
@pytest.mark.parametrize("case_id", CASES, ids=_ids)
def test_real_tables_within_the_derived_bound(case_id):
    geom, F, offset = case_id
    case = real_case(geom, F)
    got = device_run(case, geom[2:], False, offset).cpu().numpy().astype(np.float64)
    err = np.abs(got - case["ref"])
    worst = float((err / case["bound"]).max())
    print(f"[resize {_ids(case_id)}] max |device - float64| = {err.max():.3e}, bound there {case['bound'].reshape(-1)[err.argmax()]:.3e}, "
          f"largest share of the bound used {worst:.3f}")
    assert (err <= case["bound"]).all()
    if offset:   # the element route gives the bits of the 16-byte route
        assert np.array_equal(got, device_run(case, geom[2:], False, False).cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("geom", [(48, 64, 12, 16), (13, 17, 26, 34)], ids=_ids)
def test_bilinear_tables_through_the_same_kernel(geom):
    """The tables, not the kernel, carry the filter: the triangle's tables within their own bound."""
    case = real_case(geom, 2, "bilinear")
    got = device_run(case, geom[2:], False).cpu().numpy().astype(np.float64)
    assert (np.abs(got - case["ref"]) <= case["bound"]).all()
    assert not np.array_equal(case["ref"], real_case(geom, 2)["ref"][:2])


def test_frame_resizer_uses_the_tables_of_the_restatement():
    geom = (48, 64, 12, 16)
    case = real_case(geom, 3)
    r = driver.FrameResizer(geom[:2], geom[2:])
    for name, t in (("xf", r.x_first), ("xw", r.x_weight), ("yf", r.y_first), ("yw", r.y_weight)):
        assert np.array_equal(t.cpu().numpy(), case[name]), name
    src = to_device(case["src"])
    got = r(src)
    assert torch.equal(got, device_run(case, geom[2:], False))
    assert torch.equal(r(src[1]), got[1]) and r(src[1]).shape == (12, 16, 3)          # [H,W,3] in, [h,w,3] out
    with pytest.raises(ValueError, match=r"expected float32 \[F,48,64,3\]"):
        r(src[:, :40])
    with pytest.raises(_lib.VsrHipError, match="expected torch.float32"):
        r(src.double())
    with pytest.raises(_lib.VsrHipError, match="src and dst overlap"):
        driver.resize_frames(src, (48, 64), r.x_first.new_zeros(64), r.x_weight.new_ones(64, 1), r.y_first.new_zeros(48),
                             r.y_weight.new_ones(48, 1), out=src)


# ------------------------------------------------------------------------------------------------ 3. real tables, quantised
MAX_EXCUSED = 0.005


@pytest.mark.parametrize("case_id", CASES, ids=_ids)
def test_real_tables_quantised_codes(case_id):
    """quantise = 1: the code is rint(clip(float64)) wherever the float64 value is farther than the bound from a tie or a clamp edge;
    elsewhere it may be the neighbouring code.  The share of such pixels is a condition of the case (from the reference alone)."""
    geom, F, offset = case_id
    case = real_case(geom, F)
    ex = R.excused(case["ref"], case["bound"])
    assert ex.mean() <= MAX_EXCUSED, f"{ex.sum()} of {ex.size} elements within the bound of a tie or an edge: choose another seed"
    want = R.quantise64(case["ref"])
    got = device_run(case, geom[2:], True, offset).cpu().numpy().astype(np.float64)
    assert np.array_equal(got[~ex], want[~ex])
    assert (np.abs(got[ex] - want[ex]) <= 1).all() and (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255


@pytest.mark.parametrize("geom", [(48, 64, 12, 16), (12, 16, 48, 64), (9, 11, 9, 11), (37, 53, 12, 16)], ids=_ids)
def test_constant_frames_stay_constant(geom):
    H, W, h, w = geom
    r = driver.FrameResizer((H, W), (h, w))
    for v in (0.0, 128.0, 255.0):
        got = r(torch.full((2, H, W, 3), v, device="cuda"), quantise=True)
        assert (got == v).all(), v


# ------------------------------------------------------------------------------------------------ 4. repeatability, independence
@pytest.mark.parametrize("geom", [(48, 64, 12, 16), (45, 63, 15, 21), (12, 16, 48, 64), (136, 40, 17, 5)], ids=_ids)
@pytest.mark.parametrize("quantise", [False, True])
def test_same_bits_again_per_frame_and_under_graph_replay(geom, quantise):
    case = real_case(geom, 3)
    a = device_run(case, geom[2:], quantise)
    b = device_run(case, geom[2:], quantise)
    assert torch.equal(a, b)
    src = to_device(case["src"])
    tabs = [to_device(case[k]) for k in ("xf", "xw", "yf", "yw")]
    for f in range(3):
        one = driver.resize_frames(src[f:f + 1].clone(), geom[2:], *tabs, quantise=quantise)
        assert torch.equal(one[0], a[f]), f
    out = torch.full_like(a, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        driver.resize_frames(src, geom[2:], *tabs, quantise=quantise, out=out)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)


# ------------------------------------------------------------------------------------------------ 5. poisoned buffers
@pytest.mark.parametrize("geom", [(48, 64, 12, 16), (45, 63, 15, 21), (13, 17, 26, 34), (136, 40, 17, 5)], ids=_ids)
def test_poisoned_buffers(geom):
    """dst allocated through tests/_poison.py (all-ones: NaN, guard bands either side): every element is written, nothing beyond it,
    and the bits are those of the run on ordinary buffers."""
    case = real_case(geom, 3)
    src = to_device(case["src"])
    tabs = [to_device(case[k]) for k in ("xf", "xw", "yf", "yw")]
    for quantise in (False, True):
        plain = driver.resize_frames(src, geom[2:], *tabs, quantise=quantise)
        with poisoned(package_state=False) as arena:   # (driver.py keeps no buffer between calls)
            got = driver.resize_frames(src, geom[2:], *tabs, quantise=quantise)
            assert arena.n_allocated == 1 and arena.find(got) is not None
            arena.assert_written(got, "dst")
            assert torch.isfinite(got).all() and torch.equal(got, plain)
            arena.check()


# ------------------------------------------------------------------------------------------------ 6. the clip run
def _build(cpu_vsr):
    m = copy.deepcopy(cpu_vsr).cuda().eval()
    m.precision = m.model.precision = "fp32"
    return m


def test_bicubic_clip_run(cpu_vsr):
    """A 5-frame nv12 clip of 256 x 256, LR frames of 64 x 64 made by the antialiased bicubic reduction, super-resolved by 4 and scored on
    luma beside the bicubic baseline: output bytes and both metric pairs equal the composition yuv_ingest at full size ->
    FrameResizer(quantise) -> run_item -> frame_metrics, and FrameResizer up -> frame_metrics, bit for bit, with and without overlap and
    in a second run; the defaults give what decimate="nearest" and the existing composition give; the byte counters do not move; under
    poisoned buffers the same bits."""
    S, fmt, T = 4, "nv12", 5
    H = W = 64 * S
    fb = driver.yuv_frame_bytes(fmt, H, W)
    model = _build(cpu_vsr)
    video = torch.from_numpy(driver.synthetic_video(T, H, W, seed=11)).cuda().float()
    clip = driver.frames_to_yuv(video, fmt).cpu().numpy()
    coef = driver.yuv_coefficients(fmt, inverse=True)

    # ---- the composition
    full, _ = driver.yuv_ingest(torch.from_numpy(clip).cuda(), (H, W), fmt, coef)
    assert full.shape == (T, H, W, 3)
    lr = driver.FrameResizer((H, W), (H // S, W // S))(full, quantise=True)
    assert (lr == lr.round()).all() and lr.min() >= 0 and lr.max() <= 255
    data = torch.stack([lr[t:t + 3] for t in range(T - 2)])
    outs, _, _ = driver.run_item(model, data, None, None)
    truth = full[1:T - 1]
    want_bytes = driver.frames_to_yuv(outs, fmt).cpu().numpy()
    want = driver.psnr_ssim(driver.frame_metrics(outs, truth, "y", True, S))
    base = driver.FrameResizer((H // S, W // S), (H, W))(lr[1:T - 1].contiguous())
    want_base = driver.psnr_ssim(driver.frame_metrics(base, truth, "y", True, S))
    assert np.isfinite(want[0]).all() and np.isfinite(want_base[0]).all()

    def check(r, got_bytes):
        assert np.array_equal(got_bytes, want_bytes)
        m = r.metrics
        assert sorted(m) == ["psnr", "psnr_baseline", "ssim", "ssim_baseline"] and all(v.shape == (T - 2,) for v in m.values())
        assert np.array_equal(m["psnr"], want[0]) and np.array_equal(m["ssim"], want[1])
        assert np.array_equal(m["psnr_baseline"], want_base[0]) and np.array_equal(m["ssim_baseline"], want_base[1])
        assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)

    for overlap in (True, False):
        r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=overlap, score="y", decimate="bicubic", baseline="bicubic")
        assert r._full is not None and r._full is not r._truth and r._full.data_ptr() != r._truth.data_ptr()
        for again in range(2 if overlap else 1):   # (slot reuse: a second run of the same object)
            check(r, r.run(clip))
    gain = want[0] - want_base[0]
    print(f"[bicubic clip x{S}] PSNR {want[0].round(3).tolist()} dB, bicubic baseline {want_base[0].round(3).tolist()} dB, "
          f"gain {gain.round(3).tolist()} dB (synthetic weights: the sign means nothing)")

    # ---- the defaults: the parent path.  decimate="nearest" spelled out, the defaults, and the existing composition agree
    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(T - 2)])).cuda()
    ndata, _, _ = driver.ingest_item_yuv(windows, (H, W), fmt, scale=S, want_hr=False)
    nouts, _, _ = driver.run_item(model, ndata, None, None)
    nbytes = driver.frames_to_yuv(nouts, fmt).cpu().numpy()
    nwant = driver.psnr_ssim(driver.frame_metrics(nouts, truth, "y", True, S))
    default = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y")
    spelled = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", decimate="nearest", baseline=None)
    assert (default.decimate, default.baseline, default._full, default._base) == ("nearest", None, None, None)
    for r in (default, spelled):
        assert np.array_equal(r.run(clip), nbytes)
        assert sorted(r.metrics) == ["psnr", "ssim"]
        assert np.array_equal(r.metrics["psnr"], nwant[0]) and np.array_equal(r.metrics["ssim"], nwant[1])
        assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
    assert not np.array_equal(nbytes, want_bytes)   # the two decimations are different LR frames
    # the baseline alone changes no output byte of the nearest path
    nb = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", baseline="bicubic")
    assert np.array_equal(nb.run(clip), nbytes) and np.array_equal(nb.metrics["psnr"], nwant[0])

    with poisoned() as arena:
        m = _build(cpu_vsr)   # a fresh object: its caches are born inside the block
        r = driver.ClipRunner(m, (H, W), fmt, fmt, scale_down=S, score="y", decimate="bicubic", baseline="bicubic")
        assert all(arena.find(t) is not None for t in (r._truth, r._full, r._base))
        check(r, r.run(clip))
        arena.check()
