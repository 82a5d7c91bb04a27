"""Scene cuts on the device (include/vsr_hip_scene.h, driver.scene_sums / scene_flags / scene_window / ClipRunner(scene="sad")) against
the float64 restatement of tests/_scene_ref.py (pinned by tests/test_scene_ref_helper.py, which also checks that the clip used below keeps
a factor of two from the default thresholds on every side).

csrc/clip_scene.hip sums a pair in workgroups of WG = VSR_SCENE_WG_PIXELS = 1024 consecutive pixels, on 16-byte loads where both bases are
16-byte aligned and h * w % 4 == 0 and on element loads otherwise, and adds a pair's partials with FT = VSR_SCENE_FINISH_THREADS = 256
threads.  The sizes (_scene_ref.SIZES): 1 x 1, 1 x 7, 5 x 3, 17 x 33 (one workgroup, h * w % 4 != 0: element loads), 64 x 64 (4 workgroups,
16-byte loads), 65 x 129 (9 workgroups, the last one partly filled, element loads) and FINISH_SIZE = (FT * WG / 512 + 1) x 512 = 513 x 512:
FT + 1 = 257 partials, so the finish launch's strided loop runs twice for thread 0 (derived from the two constants, which
tests/test_abi_scene.py reads from the header).

Both sums are integers below 2^53, so every comparison of sums is for equal bits.  The clip runs use LR frames of 64 x 64, the smallest
VSR.forward accepts: an nv12 clip of 128 x 128 at x2 of 4 + 4 frames of two scenes (_scene_ref.two_scene_video), the seeded synthetic model
of tests/test_gpu_warp_error.py, in fp32 and fp16, with and without overlap."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _scene_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402
from video_super_resolution_amd.driver import scene_cuts, scene_flags, scene_sums, scene_window  # noqa: E402

LUMAS = {"bt601": R.LUMA_BT601, "odd": R.LUMA_ODD}
OPEN_OCC = (0.01, 30.0, 0.01, 20.0)   # as tests/test_gpu_warp_error.py: sized to the synthetic weights' flows


def to_device(x, offset=False, dtype=torch.float32):
    """The array on the device; `offset`: inside a flat buffer at a storage offset of one element (a base 4 bytes past a multiple of 16)."""
    t = torch.tensor(np.ascontiguousarray(x)).to(dtype)
    if not offset:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.zeros(t.numel() + 8, dtype=dtype, device="cuda")
    buf[1:1 + t.numel()] = t.reshape(-1).cuda()
    view = buf[1:1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(kind, P, h, w, luma):
    """The inputs of a case and the restatement's sums, computed once."""
    a, b = R.make_pair(kind, P, h, w)
    return a, b, R.pair_sums(a, b, LUMAS[luma])


# ------------------------------------------------------------------------------------------------ 1. sums
@pytest.mark.parametrize("luma", sorted(LUMAS))
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("h,w", R.SIZES)
def test_sums_equal_the_restatements_bits(h, w, P, kind, luma):
    a, b, want = _case(kind, P, h, w, luma)
    got = scene_sums(to_device(a), to_device(b), luma4=LUMAS[luma])
    assert got.shape == (P, 2) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    print(f"[sums {h}x{w} P{P} {kind} {luma}] got {got.tolist()} want {want.tolist()}")
    assert np.isfinite(got).all() and R.same_bits(got, want)
    assert (want[:, 1] == h * w).all() and (h * w < 4 or (want[:, 0] > 0).all())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("h,w", R.SIZES)
def test_a_base_offset_by_four_bytes_changes_nothing(h, w, kind):
    """Bases 4 bytes past a multiple of 16 take element loads whatever the size; the aligned run of 64 x 64 and of FINISH_SIZE takes
    16-byte loads: same bits.  The default luma4 is BT.601."""
    a, b, want = _case(kind, 3, h, w, "bt601")
    shifted = scene_sums(to_device(a, True), to_device(b, True))
    mixed = scene_sums(to_device(a), to_device(b, True))
    aligned = scene_sums(to_device(a), to_device(b))
    assert torch.equal(shifted, aligned) and torch.equal(mixed, aligned) and R.same_bits(shifted.cpu().numpy(), want)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("h,w", [(5, 3), (64, 64), (65, 129)])
def test_sums_identities(h, w, kind):
    a, b, want = _case(kind, 3, h, w, "bt601")
    ta, tb = to_device(a), to_device(b)
    n = float(h * w)
    assert scene_sums(ta, ta).cpu().tolist() == [[0.0, n]] * 3                 # a == b (one buffer, and a copy of it)
    assert scene_sums(ta, ta.clone()).cpu().tolist() == [[0.0, n]] * 3
    one = scene_sums(ta, tb)
    assert torch.equal(scene_sums(tb, ta), one)                                 # swapped
    assert torch.equal(scene_sums(ta, tb), one)                                 # again: the same bits
    for p in range(3):                                                          # a pair's row does not depend on the P it travelled in
        assert torch.equal(scene_sums(ta[p:p + 1], tb[p:p + 1])[0], one[p]), p
        assert torch.equal(scene_sums(ta[p], tb[p])[0], one[p]), p              # [h,w,3] frames are one pair
    perm = [2, 0, 1]                                                            # ... nor on its place
    assert torch.equal(scene_sums(ta[perm].contiguous(), tb[perm].contiguous()), one[perm])
    big = torch.full((5, 2), -7.0, dtype=torch.float64, device="cuda")          # into the middle rows of a larger tensor
    scene_sums(ta, tb, out=big[1:4])
    assert torch.equal(big[1:4], one) and (big[0] == -7.0).all() and (big[4] == -7.0).all()


# ------------------------------------------------------------------------------------------------ 2. decide
@pytest.mark.parametrize("case", R.DECIDE_CASES, ids=[c.name for c in R.DECIDE_CASES])
def test_decide_cases_equal_the_restatement(case):
    sums = torch.tensor(case.sums, dtype=torch.float64, device="cuda")
    prev = None if case.prev is None else torch.tensor(case.prev, dtype=torch.float64, device="cuda")
    got = scene_flags(sums, prev, (case.t_abs, case.ratio))
    assert got.dtype == torch.int32 and got.shape == (len(case.sums),)
    want = R.decide(case.sums, case.prev, case.t_abs, case.ratio)
    assert got.cpu().tolist() == want.tolist() == case.want
    # row by row with the row above as the pair before, as ClipRunner calls it: the same flags
    out = torch.full((len(case.sums) + 2,), -7, dtype=torch.int32, device="cuda")
    for p in range(len(case.sums)):
        scene_flags(sums[p:p + 1], sums[p - 1] if p else prev, (case.t_abs, case.ratio), out=out[1 + p:2 + p])
    assert out.cpu().tolist() == [-7] + case.want + [-7]


def test_decide_on_the_sums_of_real_pairs_and_the_host_step_agree():
    a, b, want = _case("float", 3, 17, 33, "bt601")
    sums = scene_sums(to_device(a), to_device(b))
    for thresholds in (None, (0.0, 0.0), (1e30, 2.0), (50.0, 0.5), (50.0, 1.5)):
        got = scene_flags(sums, thresholds=thresholds).cpu().numpy()
        cuts, m = scene_cuts(sums, thresholds)
        assert np.array_equal(got != 0, cuts) and np.array_equal(cuts, R.cuts(want, thresholds)[0]), thresholds
        assert R.same_bits(m, want[:, 0] / want[:, 1])
    assert scene_flags(sums, thresholds=(0.0, 0.0)).cpu().tolist() == [1, 1, 1]
    assert scene_flags(sums, thresholds=(1e30, 2.0)).cpu().tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 3. window
def _window_inputs(h, w, S, kind="salted"):
    fr, est = R.make_pair(kind, 3, h, w, seed=S)[0], R.make_pair(kind, 1, S * h, S * w, seed=S + 10)[1]
    return fr[0], fr[1], fr[2], est


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (17, 33), (64, 64)])
def test_window_is_torch_indexing_bit_for_bit(h, w, S):
    """All four flag combinations, flags given as device words and (where 0) as null pointers, with and without the previous estimate;
    the frames are salted with NaN and infinities: the outputs are compared as 32-bit words."""
    a, b, c, prev = (to_device(v) for v in _window_inputs(h, w, S))
    flags = torch.tensor([0, 1, 7, -1], dtype=torch.int32, device="cuda")    # any word that is not 0 sets a flag
    zero, one = flags[0:1], flags[1:2]
    for fab in (0, 1):
        for fbc in (0, 1):
            want_x = torch.stack([b if fab else a, b, b if fbc else c])
            want_est = b[None] if fab else prev[:, ::S, ::S]
            forms = [(one if fab else zero, one if fbc else zero), (one if fab else None, one if fbc else None)]
            if fab and fbc:
                forms.append((flags[2:3], flags[3:4]))
            for f_ab, f_bc in forms:
                x, est = scene_window(a, b, c, prev, f_ab, f_bc)
                assert x.shape == (3, h, w, 3) and est.shape == (1, h, w, 3) and x.is_contiguous() and est.is_contiguous()
                assert torch.equal(bits(x), bits(want_x)) and torch.equal(bits(est), bits(want_est)), (fab, fbc)
                x0, none = scene_window(a, b, c, None, f_ab, f_bc)
                assert none is None and torch.equal(bits(x0), bits(want_x))
                # [H,W,3] is taken as [1,H,W,3]; a permuted view of the estimate (what the model returns) as its contiguous copy
                x1, est1 = scene_window(a, b, c, prev[0].permute(2, 0, 1).contiguous().permute(1, 2, 0), f_ab, f_bc)
                assert torch.equal(bits(x1), bits(want_x)) and torch.equal(bits(est1), bits(want_est))
    # fresh tensors on every call (VSR.temporal_cache keys on storage identity)
    x, est = scene_window(a, b, c, prev)
    x2, est2 = scene_window(a, b, c, prev)
    assert len({x.data_ptr(), x2.data_ptr(), est.data_ptr(), est2.data_ptr()}) == 4
    assert x._version == 0 and est._version == 0


def test_window_on_bases_offset_by_four_bytes():
    S, h, w = 2, 17, 33
    a, b, c, prev = (to_device(v, True) for v in _window_inputs(h, w, S))
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    x, est = scene_window(a, b, c, prev, None, one)
    assert torch.equal(bits(x), bits(torch.stack([a, b, b]))) and torch.equal(bits(est), bits(prev[:, ::S, ::S]))


# ------------------------------------------------------------------------------------------------ 4. poisoned buffers
@pytest.mark.parametrize("h,w", [(17, 33), (64, 64), (65, 129)])
def test_poisoned_sums_and_workspace(h, w):
    """The sums and the workspace allocated through tests/_poison.py (all-ones: NaN in float64, guard bands either side): finite results
    equal in their bits to the run on ordinary buffers, every slot written, the bands intact, the inputs untouched."""
    a, b, want = _case("salted", 3, h, w, "bt601")
    ta, tb = to_device(a), to_device(b)
    keep = bits(ta).clone(), bits(tb).clone()
    plain = scene_sums(ta, tb)
    with poisoned(package_state=False) as arena:
        got = scene_sums(ta, tb)
        assert arena.n_allocated == 2 and arena.find(got) is not None     # the sums and the workspace
        arena.assert_written(got, "sums")
        assert torch.isfinite(got).all() and torch.equal(got, plain) and R.same_bits(got.cpu().numpy(), want)
        arena.check()
    assert torch.equal(bits(ta), keep[0]) and torch.equal(bits(tb), keep[1])


def test_poisoned_flags():
    case = next(c for c in R.DECIDE_CASES if c.name == "run")
    sums = torch.tensor(case.sums, dtype=torch.float64, device="cuda")
    keep = sums.clone()
    with poisoned(package_state=False, extra_dtypes=(torch.int32,)) as arena:
        got = scene_flags(sums, None, (case.t_abs, case.ratio))
        assert arena.n_allocated == 1 and arena.find(got) is not None
        arena.assert_written(got, "flags")
        assert got.cpu().tolist() == case.want
        arena.check()
    assert torch.equal(sums, keep)


@pytest.mark.parametrize("with_est", [True, False])
@pytest.mark.parametrize("h,w", [(5, 3), (17, 33), (64, 64)])
def test_poisoned_window(h, w, with_est):
    """Integer frames (no element holds the all-ones pattern): both outputs fully written, nothing beyond them, the inputs untouched."""
    S = 3
    a, b, c, prev = (to_device(v) for v in _window_inputs(h, w, S, "integer"))
    keep = [bits(t).clone() for t in (a, b, c, prev)]
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    for f_ab, f_bc in ((None, None), (one, None), (None, one), (one, one)):
        with poisoned(package_state=False) as arena:
            x, est = scene_window(a, b, c, prev if with_est else None, f_ab, f_bc)
            assert arena.n_allocated == (2 if with_est else 1) and arena.find(x) is not None
            arena.assert_written(x, "x")
            if with_est:
                arena.assert_written(est, "est")
                assert torch.equal(est, b[None] if f_ab is not None else prev[:, ::S, ::S])
            assert torch.equal(x, torch.stack([b if f_ab is not None else a, b, b if f_bc is not None else c]))
            arena.check()
    assert all(torch.equal(bits(t), k) for t, k in zip((a, b, c, prev), keep)) and one.item() == 1


# ------------------------------------------------------------------------------------------------ 5. clip runs
S, FMT = R.CLIP_S, "nv12"
H = W = R.CLIP_S * R.CLIP_LR
T, CUT = R.CLIP_A + R.CLIP_B, R.CLIP_A - 1      # the one cut is the pair (CUT, CUT + 1)
CLOSED, OPEN = (1e30, 2.0), (0.0, 0.0)
_masters, _models, _plain = {}, {}, {}


def _model(cpu_vsr, precision):
    """The seeded model of the warping-error clip tests, one per precision for the whole module."""
    from video_super_resolution_amd import VSR
    from video_super_resolution_amd.weights import fill_module_
    if precision not in _models:
        if S not in _masters:
            m = VSR(upscale_factor=S).eval()
            m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
            fill_module_(m.model, seed=0, prefix="model.")
            _masters[S] = m
        m = copy.deepcopy(_masters[S]).cuda().eval()
        m.precision = m.model.precision = precision
        _models[precision] = m
    return _models[precision]


@functools.lru_cache(maxsize=None)
def _clips():
    """The two-scene clip as nv12 frames on the host, and the clips of the two separate runs: A ++ [A[-1]] and [B[0]] ++ B."""
    video = torch.from_numpy(R.two_scene_video()).cuda().float()
    clip = driver.frames_to_yuv(video, FMT).cpu().numpy()
    nA = R.CLIP_A
    return clip, np.concatenate([clip[:nA], clip[nA - 1:nA]]), np.concatenate([clip[nA:nA + 1], clip[nA:]])


def _runner(model, **kw):
    return driver.ClipRunner(model, (H, W), FMT, FMT, scale_down=S, **kw)


def _plain_runs(cpu_vsr, precision):
    """Output bytes of scene=None runs over the clip and over the clips of the two separate runs, computed once per precision."""
    if precision not in _plain:
        r = _runner(_model(cpu_vsr, precision))
        _plain[precision] = tuple(r.run(c).copy() for c in _clips())
        assert r.cuts is None and r.scene_m is None
    return _plain[precision]


def _lr_frames(clip):
    """The LR frames the runner's ring holds: the conversion's own nearest decimation of every source frame, float32 [T,h,w,3]."""
    lr, _ = driver.yuv_ingest(torch.from_numpy(clip).cuda(), (H, W), FMT, driver.yuv_coefficients(FMT, inverse=True), "left", (H // S, W // S))
    return lr


def _bytes_of(out):
    return driver.yuv_write(out[0], FMT, driver.yuv_coefficients(FMT)).cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_clip_closed_thresholds_change_no_byte(cpu_vsr, precision):
    """(a) t_abs = 1e30: no pair is a cut, and the window and the estimate chosen on the device are the ones torch.stack and the model's own
    resize give: the output bytes of scene=None.  `scene_m` is the restatement's score of the ring's frames, bit for bit."""
    model, clip = _model(cpu_vsr, precision), _clips()[0]
    want = _plain_runs(cpu_vsr, precision)[0]
    fb = driver.yuv_frame_bytes(FMT, H, W)
    lr = _lr_frames(clip).cpu().numpy()
    want_sums = R.pair_sums(lr[:-1], lr[1:])
    for overlap in (True, False):
        r = _runner(model, overlap=overlap, scene="sad", scene_thresholds=CLOSED)
        for again in range(2 if overlap else 1):   # (a second run of the same object)
            got = r.run(clip)
            assert np.array_equal(got, want), (overlap, again)
            assert r.cuts.dtype == np.bool_ and r.cuts.shape == (T - 1,) and not r.cuts.any()
            assert r.scene_m.dtype == np.float64 and R.same_bits(r.scene_m, want_sums[:, 0] / want_sums[:, 1])
            assert (r.frames_in, r.frames_out, r.h2d_bytes, r.d2h_bytes) == (T, T - 2, T * fb, (T - 2) * fb)
    # the scores keep the distance from the defaults the CPU test asserts for the float frames (here: after the 4:2:0 round trip)
    m = want_sums[:, 0] / want_sums[:, 1]
    print(f"[clip {precision}] scene_m {m.tolist()}")
    assert m[CUT] >= R.THRESHOLDS[0] and (np.delete(m, CUT) < R.THRESHOLDS[0]).all()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_clip_with_one_cut_restarts_the_recurrence_at_the_cut(cpu_vsr, precision):
    """(b) A ++ B under the default thresholds: the one cut is found; the output bytes are those of per-window model calls whose window and
    estimate are composed here by the header's rule, and those of scene=None runs over A ++ [A[-1]] and over [B[0]] ++ B, concatenated."""
    model, (clip, part1, part2) = _model(cpu_vsr, precision), _clips()
    _, want1, want2 = _plain_runs(cpu_vsr, precision)
    cuts = np.zeros(T - 1, dtype=bool)
    cuts[CUT] = True
    # per-window calls, the flags known by construction
    lr = _lr_frames(clip)
    est, composed = None, []
    with torch.no_grad():
        for i in range(2, T):
            a, b, c = lr[i - 2], lr[i - 1], lr[i]
            fab, fbc = cuts[i - 2], cuts[i - 1]
            x = torch.stack([b if fab else a, b, b if fbc else c])
            fed = None if est is None else (b[None].clone() if fab else est[:, ::S, ::S].contiguous())
            est, _ = model(x, None, None, fed, train=False)
            composed.append(_bytes_of(est))
    composed = np.stack(composed)
    for overlap in (True, False):
        r = _runner(model, overlap=overlap, scene="sad")
        assert r.scene_thresholds == driver.SCENE_THRESHOLDS
        got = r.run(clip)
        assert np.array_equal(r.cuts, cuts), r.scene_m
        assert got.shape == composed.shape and np.array_equal(got, composed), overlap
        assert np.array_equal(got, np.concatenate([want1, want2])), overlap
    assert not np.array_equal(got, _plain_runs(cpu_vsr, precision)[0])      # (not vacuous: the cut changes the output)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_clip_open_thresholds_make_every_window_a_fresh_start(cpu_vsr, precision):
    """(c) thresholds (0, 0): every pair is a cut, every window is (b, b, b) with the recurrence restarted."""
    model, clip = _model(cpu_vsr, precision), _clips()[0]
    lr = _lr_frames(clip)
    with torch.no_grad():
        fresh = np.stack([_bytes_of(model(torch.stack([lr[i - 1]] * 3), None, None, None, train=False)[0]) for i in range(2, T)])
    for overlap in (True, False):
        r = _runner(model, overlap=overlap, scene="sad", scene_thresholds=OPEN)
        got = r.run(clip)
        assert r.cuts.all() and np.array_equal(got, fresh), overlap


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_clip_warping_error_is_nan_across_the_cut_and_unchanged_elsewhere(cpu_vsr, precision):
    """(d) temporal="warp" under OPEN_OCC: row r is scored along the flows between source frames r + 1 and r + 2, so it is NaN exactly
    where cuts[r + 1]; the rows before are those of the run over A ++ [A[-1]], the rows after those of the run over [B[0]] ++ B;
    `valid_share` stays as computed; PSNR and SSIM are the separate runs' too."""
    model, (clip, part1, part2) = _model(cpu_vsr, precision), _clips()
    sep = []
    for part in (part1, part2):
        r = _runner(model, score="y", temporal="warp", occ=OPEN_OCC)
        r.run(part)
        sep.append(r.metrics)
    n1 = len(sep[0]["ewarp"])
    assert n1 == R.CLIP_A - 2 and len(sep[1]["ewarp"]) == R.CLIP_B - 2
    for overlap in (True, False):
        r = _runner(model, overlap=overlap, score="y", temporal="warp", occ=OPEN_OCC, scene="sad")
        r.run(clip)
        m = r.metrics
        assert np.flatnonzero(r.cuts).tolist() == [CUT]
        for k in ("ewarp", "ewarp_truth"):
            assert m[k].shape == (T - 3,)
            assert np.array_equal(np.isnan(m[k]), r.cuts[1:T - 2]), (k, m[k])
            assert np.flatnonzero(np.isnan(m[k])).tolist() == [CUT - 1]
            assert np.array_equal(m[k][:n1], sep[0][k]) and np.array_equal(m[k][n1 + 1:], sep[1][k]), k
            assert np.isfinite(sep[0][k]).all() and np.isfinite(sep[1][k]).all()
        assert np.isfinite(m["valid_share"]).all()
        assert np.array_equal(m["valid_share"][:n1], sep[0]["valid_share"]) and np.array_equal(m["valid_share"][n1 + 1:], sep[1]["valid_share"])
        for k in ("psnr", "ssim"):
            assert np.array_equal(m[k], np.concatenate([sep[0][k], sep[1][k]])), k


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_clip_with_the_temporal_cache_on_gives_the_same_bytes(cpu_vsr, precision):
    """(e) VSR.temporal_cache keys on storage identity and version; scene_window's results are fresh tensors, so no stale entry is served."""
    model, clip = _model(cpu_vsr, precision), _clips()[0]
    _, want1, want2 = _plain_runs(cpu_vsr, precision)
    model.reset_temporal_cache()
    model.temporal_cache = True
    try:
        for overlap in (True, False):
            r = _runner(model, overlap=overlap, scene="sad")
            got = r.run(clip)
            assert np.flatnonzero(r.cuts).tolist() == [CUT]
            assert np.array_equal(got, np.concatenate([want1, want2])), overlap
    finally:
        model.temporal_cache = False
        model.reset_temporal_cache()


def test_clip_scene_refusals_with_a_real_model(cpu_vsr):
    model = _model(cpu_vsr, "fp32")
    with pytest.raises(ValueError, match="scene must be None or 'sad'"):
        _runner(model, scene="flow")
    with pytest.raises(ValueError, match="no scene detection is asked for"):
        _runner(model, scene_thresholds=(15.0, 2.0))
