"""The temporal warping error on the device (include/vsr_hip_warp.h, driver.truth_flows / warp_error / ewarp / ClipRunner(temporal="warp"))
against the float64 restatement of tests/_warp_ref.py (pinned by tests/test_warp_ref_helper.py, which also asserts that every case below
has a valid share in [0.2, 0.95] and loses pixels to each of the three conditions alone).

csrc/frame_warp_error.hip scores a pair in tiles of TW = VSR_WARP_TILE_W = 64 columns by TH = VSR_WARP_TILE_H = 16 rows of the scored
region, four rows in flight, and sums a pair's per-tile partials with FT = VSR_WARP_FINISH_THREADS = 256 threads.  The cases
(_warp_ref.CASES: P, frame H x W, crop (y0, x0, h, w), shave), the smallest that reach every branch:
  tiny     3 x     1 x  1, (0, 0, 1, 1), 0          the smallest region the refusals allow: one pixel, one tile, every neighbour and
                                                    every gather clamped onto the pixel itself; three pairs
  cols     1 x     9 x 65, the frame, 0             TW + 1 columns: one lane of a second tile; W is odd: a row pitch of 780 bytes is no
                                                    multiple of 16
  rows     1 x    17 x 12, the frame, 0             TH + 1 rows: one row of a second tile row; a tile narrower than a wave
  crop     2 x    70 x 75, (3, 5, 64, 64), 2        a frame larger than its crop, y0 and x0 not 0, a shave inside the crop; two pairs
  aligned  3 x    16 x 64, the frame, 0             bases on 16 bytes and W % 4 == 0, where a 16-byte path would apply: the kernel loads
                                                    elements only (see the header), this case and the next pin that alignment changes
                                                    nothing; three pairs
  offset   2 x    16 x 64, the frame, 0             frames and flows in flat buffers at a storage offset of one element
  finish   1 x  2049 x 65, the frame, 0             129 x 2 = 258 partials > FT: the second trip of the finish kernel's loop
every one in RGB and Y, with quantise 0 and 1, and with the flows as planar float32 [P,2,h,w] and as NHWC half [P,h,w,32] (the flow in
channels 0 and 1, NaN in the other 30).

The scored clip run uses LR frames of 64 x 64, the smallest VSR.forward accepts: a 6-frame nv12 clip of 128 x 128 at x2.  The seeded
synthetic weights make FlowNet2 a noise source (flows of a few pixels that differ by about a pixel between neighbours and by a few pixels
between the two directions): under the published occlusion constants no pixel is valid and E_warp is NaN, which the run checks as such;
the same run with the rule opened to OPEN_OCC, under which a good part of the pixels counts, checks the numbers."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _warp_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402

NAMES = [c.name for c in R.CASES]
OPEN_OCC = (0.01, 30.0, 0.01, 20.0)   # c2 and g2 sized to the synthetic weights' flows (|f + b|^2 around 14, squared differences 4 to 100)
MODES = [(ch, q) for ch in ("rgb", "y") for q in (0, 1)]


def to_device(x, offset, dtype=torch.float32):
    """The array on the device; `offset`: inside a flat buffer at a storage offset of one element."""
    t = torch.tensor(np.ascontiguousarray(x)).to(dtype)
    if not offset:
        return t.cuda()
    buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
    buf[1:1 + t.numel()] = t.reshape(-1).cuda()
    view = buf[1:1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def flow_to_device(f, form, offset):
    """[P,2,h,w] float32 -> the planar float32 tensor, or the NHWC half map [P,h,w,32] with NaN in the channels that are not the flow."""
    if form == "f32":
        return to_device(f, offset)
    P, _, h, w = f.shape
    m = np.full((P, h, w, R.LD), np.nan, dtype=np.float16)
    m[..., 0], m[..., 1] = f[:, 0], f[:, 1]
    assert np.array_equal(m[..., 0].astype(np.float32), f[:, 0]), "the values must be ones half can hold"
    return to_device(m, offset, torch.float16)


def gpu(name, kind, form, channels, quant, luma="bt601", out=None, inputs=None, pairs=None):
    """driver.warp_error of a case -> the device tensor [P,4]."""
    c = R.CASE[name]
    a, b, fwd, bwd = inputs if inputs is not None else R.make_case(name, kind, form, quant)
    if pairs is not None:
        a, b, fwd, bwd = a[pairs], b[pairs], fwd[pairs], bwd[pairs]
    flows = (flow_to_device(fwd, form, c.offset), flow_to_device(bwd, form, c.offset), c.crop)
    got = driver.warp_error(to_device(a, c.offset), to_device(b, c.offset), flows, channels, bool(quant), c.shave, out=out,
                            luma4=R.LUMA_DYADIC if luma == "dyadic" else None)
    assert got.shape == (a.shape[0], 4) and got.dtype == torch.float64 and got.is_cuda
    return got


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_exact_inputs_give_the_restatements_bits(name, channels, quant, form):
    """Flows in multiples of 1/4 pixel, frames that are integers in 0..255 once quantised (quantise 1: from floats below 0, above 255,
    on .5 ties and NaN; quantise 0: the same already quantised), Y with the dyadic luma {1/4, 1/2, 1/4, 16}: every weight is a multiple
    of 1/4, every plane value of 1/4, every bilinear value of 2^-6, every term of 2^-12 and below 2^18, every partial sum below 2^53
    (tests/test_warp_ref_helper.py): all of it is exact in double, so any order of summation gives the same bits, and all four numbers
    equal the restatement's."""
    want = R.reference(name, "exact", form, channels, quant, "dyadic").sums
    got = gpu(name, "exact", form, channels, quant, "dyadic").cpu().numpy()
    print(f"[exact {name} {channels} q{quant} {form}] got {got.tolist()} want {want.tolist()}")
    assert np.isfinite(got).all() and np.array_equal(got, want)
    assert (want[:, 2] > 0).any() and (want[:, 2] < want[:, 3]).any()


# ------------------------------------------------------------------------------------------------ 2. general
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_general_inputs_same_mask_and_sse_within_the_summation_bound(name, channels, quant, form):
    """Gaussian-perturbed smooth float32 flows (for the half form: rounded to half first) and float frames, BT.601 luma.  The mask is the
    same sequence of IEEE operations on both sides: n_valid and n_pixels (and n_terms) are equal exactly.  The terms are the
    restatement's bit for bit and non-negative; only the order of the sum differs: |sse - fsum| <= (n_terms + 2) 2^-53 fsum."""
    want = R.reference(name, "general", form, channels, quant).sums
    got = gpu(name, "general", form, channels, quant).cpu().numpy()
    err = np.abs(got[:, 0] - want[:, 0])
    bound = (want[:, 1] + 2) * 2.0 ** -53 * want[:, 0]
    print(f"[general {name} {channels} q{quant} {form}] n_valid {got[:, 2].tolist()} of {got[:, 3].tolist()}, |sse - fsum| {err.max():.3e}, "
          f"bound {bound[bound > 0].min() if (bound > 0).any() else 0.0:.3e}")
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, 1:], want[:, 1:])
    assert (err <= bound).all(), (err, bound)
    assert (want[:, 0] > 0).any()


# ------------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_zero_flows_and_equal_frames_give_zero_error_everywhere(name, channels, quant, form):
    c = R.CASE[name]
    a, _, fwd, _ = R.make_case(name, "general" if not quant else "exact", form, quant)
    zero = np.zeros_like(fwd)
    got = gpu(name, None, form, channels, quant, inputs=(a, a.copy(), zero, zero)).cpu().numpy()
    n = (c.crop[2] - 2 * c.shave) * (c.crop[3] - 2 * c.shave)
    planes = 3 if channels == "rgb" else 1
    assert (got == np.array([0.0, planes * n, n, n])).all(), got
    e, share = driver.ewarp(got)
    assert (e == 0).all() and (share == 1).all()


@pytest.mark.parametrize("dy,dx", [(2, 3), (-1, 4), (0, 0), (-3, -2)])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", ["cols", "rows", "crop", "offset"])
def test_integer_translation_gives_the_closed_form_count_and_zero_error(name, form, dy, dx):
    """Frame b is frame a moved by (dy, dx) inside the crop and the flows say so: every scored pixel whose target lies in the crop is
    valid (samples on the last column and row exactly: the clamped neighbour carries weight 0) and its error is 0."""
    c = R.CASE[name]
    y0, x0, h, w = c.crop
    s = c.shave
    rs = np.random.RandomState(5)
    a = rs.randint(0, 256, (c.P, c.H, c.W, 3)).astype(np.float32)
    b = rs.randint(0, 256, (c.P, c.H, c.W, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ok = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
    b[:, y0 + (ys + dy)[ok], x0 + (xs + dx)[ok]] = a[:, y0 + ys[ok], x0 + xs[ok]]
    fwd = np.empty((c.P, 2, h, w), dtype=np.float32)
    fwd[:, 0], fwd[:, 1] = dx, dy
    n = max(0, min(w - s, w - dx) - max(s, -dx)) * max(0, min(h - s, h - dy) - max(s, -dy))
    n_pixels = (h - 2 * s) * (w - 2 * s)
    assert 0 < n <= n_pixels
    for channels, planes in (("rgb", 3), ("y", 1)):
        got = gpu(name, None, form, channels, 1, inputs=(a, b, fwd, -fwd)).cpu().numpy()
        assert (got == np.array([0.0, planes * n, n, n_pixels])).all(), (channels, got)


@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_the_half_flow_form_equals_the_float_form_of_the_same_values(name, channels, quant):
    """Half to double is exact: the NHWC half map and planar float32 flows holding the same values give the same bits."""
    for kind in R.KINDS:
        inputs = R.make_case(name, kind, "f16", quant)      # (flows that half can hold, as float32)
        as_float = gpu(name, kind, "f32", channels, quant, inputs=inputs)
        as_half = gpu(name, kind, "f16", channels, quant, inputs=inputs)
        assert torch.equal(as_float, as_half), kind


# ------------------------------------------------------------------------------------------------ 4. determinism and batching
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", ["tiny", "crop", "aligned", "offset"])
def test_two_runs_give_the_same_bits_and_a_pair_does_not_depend_on_its_batch(name, channels, quant, form):
    c = R.CASE[name]
    one = gpu(name, "general", form, channels, quant)
    two = gpu(name, "general", form, channels, quant)
    assert torch.equal(one, two) and torch.isfinite(one).all()
    for p in range(c.P):
        single = gpu(name, "general", form, channels, quant, pairs=[p])
        assert torch.equal(single[0], one[p]), p
    if c.P == 3:   # ... nor on its place in the batch
        perm = [2, 0, 1]
        assert torch.equal(gpu(name, "general", form, channels, quant, pairs=perm), one[perm])
    if name == "crop":   # [H,W,3] frames are one pair
        a, b, fwd, bwd = R.make_case(name, "general", form, quant)
        flows = (flow_to_device(fwd[:1], form, False), flow_to_device(bwd[:1], form, False), c.crop)
        got = driver.warp_error(to_device(a[0], False), to_device(b[0], False), flows, channels, bool(quant), c.shave)
        assert torch.equal(got, one[:1])


# ------------------------------------------------------------------------------------------------ 5. poisoned buffers
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("channels,quant", MODES)
@pytest.mark.parametrize("name", ["cols", "crop", "aligned"])
def test_poisoned_workspace_and_sums(name, channels, quant, form):
    """The workspace and the sums allocated through tests/_poison.py (all-ones: NaN in float64, guard bands either side): the results
    are finite and equal in their bits to the run on ordinary buffers, every slot is written, the bands are intact: the library reads
    nothing of the workspace it has not written and writes nothing outside."""
    c = R.CASE[name]
    a, b, fwd, bwd = R.make_case(name, "general", form, quant)
    ta, tb = to_device(a, False), to_device(b, False)
    flows = (flow_to_device(fwd, form, False), flow_to_device(bwd, form, False), c.crop)
    plain = driver.warp_error(ta, tb, flows, channels, bool(quant), c.shave)
    with poisoned(package_state=False) as arena:   # (driver.py keeps no buffer between calls)
        got = driver.warp_error(ta, tb, flows, channels, bool(quant), c.shave)
        assert arena.n_allocated == 2 and arena.find(got) is not None     # the sums and the workspace
        arena.assert_written(got, "sums")
        assert torch.isfinite(got).all() and torch.equal(got, plain)
        arena.check()
    # into the middle rows of a larger tensor: the rows beside them are untouched
    big = torch.full((c.P + 2, 4), -7.0, dtype=torch.float64, device="cuda")
    driver.warp_error(ta, tb, flows, channels, bool(quant), c.shave, out=big[1:1 + c.P])
    assert torch.equal(big[1:1 + c.P], plain)
    assert (big[0] == -7.0).all() and (big[-1] == -7.0).all()


# ------------------------------------------------------------------------------------------------ 6. the scored clip run
_masters = {}


def _vsr_master(cpu_vsr, scale):
    from video_super_resolution_amd import VSR
    from video_super_resolution_amd.weights import fill_module_
    if scale not in _masters:
        m = VSR(upscale_factor=scale).eval()
        m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
        fill_module_(m.model, seed=0, prefix="model.")
        _masters[scale] = m
    return _masters[scale]


def _build(cpu_vsr, scale, precision):
    m = copy.deepcopy(_vsr_master(cpu_vsr, scale)).cuda().eval()
    m.precision = m.model.precision = precision
    return m


@functools.lru_cache(maxsize=None)
def _clip(T, H, W, fmt):
    video = torch.from_numpy(driver.synthetic_video(T, H, W, seed=11)).cuda().float()
    return driver.frames_to_yuv(video, fmt).cpu().numpy()


def _standalone(model, clip, T, H, W, S, fmt, score, occ=None):
    """E_warp of the item loop's outputs, of the truth frames and the valid share, pair by pair as the runner batches them."""
    windows = torch.from_numpy(np.stack([clip[t:t + 3] for t in range(T - 2)])).cuda()
    data, _, _ = driver.ingest_item_yuv(windows, (H, W), fmt, scale=S, want_hr=False)
    outs, _, _ = driver.run_item(model, data, None, None)
    truth, _ = driver.yuv_ingest(torch.from_numpy(clip[1:T - 1]).cuda(), (H, W), fmt, driver.yuv_coefficients(fmt, inverse=True))
    assert outs.shape == truth.shape == (T - 2, H, W, 3)
    est, tru = [], []
    for j in range(1, T - 2):
        flows = driver.truth_flows(model, truth[j - 1], truth[j])
        assert flows[2] == (0, 0, H, W)
        est.append(driver.warp_error(outs[j - 1], outs[j], flows, score, True, S, occ))
        tru.append(driver.warp_error(truth[j - 1], truth[j], flows, score, True, S, occ))
    e, share = driver.ewarp(torch.cat(est))
    e_truth, share_truth = driver.ewarp(torch.cat(tru))
    assert np.array_equal(share, share_truth)
    print(f"[warp clip {model.precision} x{S} {score} occ {occ}] E_warp {e.tolist()} truth {e_truth.tolist()} valid share {share.tolist()}")
    return e, e_truth, share


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_scored_clip_run_reports_the_warping_error(cpu_vsr):
    """A 6-frame nv12 clip whose LR frames are 64 x 64, decimated and super-resolved by 2 in fp32: the runner's `ewarp`, `ewarp_truth` and
    `valid_share` equal `ewarp(warp_error(...))` of (the float frames of a `run_item` evaluation of the same windows, `yuv_ingest` of the
    source frames, `truth_flows` of consecutive source frames) bit for bit, with and without overlap and on a second run of the same
    object; output bytes, PSNR / SSIM and the four counters are those of a runner with temporal=None; a clip of three frames gives empty
    arrays; temporal without score raises.  Under OPEN_OCC (see the module docstring) and under the published constants."""
    S, fmt, T = 2, "nv12", 6
    H = W = 64 * S
    fb = driver.yuv_frame_bytes(fmt, H, W)
    model = _build(cpu_vsr, S, "fp32")
    clip = _clip(T, H, W, fmt)

    with pytest.raises(ValueError, match="needs score"):
        driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, temporal="warp")
    with pytest.raises(ValueError, match="temporal must be None or 'warp'"):
        driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", temporal="tof")

    with pytest.raises(ValueError, match="no temporal score"):
        driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", occ=OPEN_OCC)

    for score, occ in (("y", OPEN_OCC), ("rgb", OPEN_OCC), ("y", None)):
        plain = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score=score)
        want_bytes = plain.run(clip)
        assert isinstance(plain._truth, torch.Tensor) and set(plain.metrics) == {"psnr", "ssim"}
        want_e, want_truth, want_share = _standalone(model, clip, T, H, W, S, fmt, score, occ)
        if occ is not None:   # (not vacuous: pixels are scored, and not all of them)
            assert np.isfinite(want_e).all() and (want_e > 0).all() and np.isfinite(want_truth).all() and (want_truth > 0).all()
            assert ((want_share > 0.05) & (want_share < 0.95)).all()
        else:
            assert np.isnan(want_e[want_share == 0]).all() and np.isfinite(want_e[want_share > 0]).all()
        for overlap in (True, False):
            r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=overlap, score=score, temporal="warp", occ=occ)
            assert len(r._truth) == 2
            for again in range(2 if overlap else 1):   # (slot reuse: a second run of the same object)
                got_bytes = r.run(clip)
                m = r.metrics
                assert np.array_equal(got_bytes, want_bytes), (score, overlap)
                assert np.array_equal(m["psnr"], plain.metrics["psnr"]) and np.array_equal(m["ssim"], plain.metrics["ssim"])
                assert m["ewarp"].shape == m["ewarp_truth"].shape == m["valid_share"].shape == (T - 3,) and "ewarp_baseline" not in m
                assert _same(m["ewarp"], want_e) and _same(m["ewarp_truth"], want_truth), (score, overlap, again)
                assert np.array_equal(m["valid_share"], want_share)
                assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
                assert (plain.frames_in, plain.frames_out, plain.h2d_bytes, plain.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)

    # three frames: one window, no pair
    r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", temporal="warp")
    out3 = r.run(clip[:3])
    assert np.array_equal(out3, want_bytes[:1])
    assert all(r.metrics[k].shape == (0,) for k in ("ewarp", "ewarp_truth", "valid_share")) and r.metrics["psnr"].shape == (1,)

    # with a baseline: its pairs along the same flows
    rb = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", baseline="bicubic", temporal="warp", occ=OPEN_OCC)
    pb = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", baseline="bicubic")
    assert np.array_equal(rb.run(clip), pb.run(clip)) and len(rb._base) == 2
    want_e, want_truth, want_share = _standalone(model, clip, T, H, W, S, fmt, "y", OPEN_OCC)
    for k in ("psnr", "ssim", "psnr_baseline", "ssim_baseline"):
        assert np.array_equal(rb.metrics[k], pb.metrics[k]), k
    assert np.array_equal(rb.metrics["ewarp"], want_e) and np.array_equal(rb.metrics["ewarp_truth"], want_truth)
    assert rb.metrics["ewarp_baseline"].shape == (T - 3,) and np.isfinite(rb.metrics["ewarp_baseline"]).all()
    assert (rb.metrics["ewarp_baseline"] > 0).all()


def test_scored_clip_run_in_fp16_equals_the_standalone_evaluation(cpu_vsr):
    """The same clip with precision="fp16": the flows come from the executor's NHWC half map, read in place.  Only that the runner
    equals the standalone evaluation, under OPEN_OCC and under the published constants."""
    S, fmt, T = 2, "nv12", 6
    H = W = 64 * S
    model = _build(cpu_vsr, S, "fp16")
    clip = _clip(T, H, W, fmt)
    flows = driver.truth_flows(model, *(torch.zeros((H, W, 3), device="cuda") + v for v in (1.0, 2.0)))
    assert flows[0].dtype == torch.float16 and flows[0].shape[:3] == (1, H, W) and flows[0].is_contiguous() and flows[2] == (0, 0, H, W)
    for occ in (OPEN_OCC, None):
        want_e, want_truth, want_share = _standalone(model, clip, T, H, W, S, fmt, "y", occ)
        r = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", temporal="warp", occ=occ)
        r.run(clip)
        assert _same(r.metrics["ewarp"], want_e) and _same(r.metrics["ewarp_truth"], want_truth)
        assert np.array_equal(r.metrics["valid_share"], want_share)
        if occ is not None:
            assert np.isfinite(want_e).all() and ((want_share > 0.05) & (want_share < 0.95)).all()
