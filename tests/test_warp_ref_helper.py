"""tests/_warp_ref.py pinned on the CPU: the float64 restatement of include/vsr_hip_warp.h that tests/test_gpu_warp_error.py compares the
device against agrees with an independent bilinear sampler, has the closed-form answer where there is one, sees every planted
defect, and the inputs it generates for the GPU cases exercise all three conditions of the occlusion rule."""
import numpy as np
import pytest
import torch

import _warp_ref as R


def _translation_inputs(h, w, dy, dx, H=None, W=None, y0=0, x0=0, seed=3):
    """Frame b is frame a moved by (dy, dx) inside the crop; forward flow (dx, dy), backward flow its negative."""
    H, W = H or h, W or w
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (1, H, W, 3)).astype(np.float32)
    b = rs.randint(0, 256, (1, H, W, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ok = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
    b[0, y0 + (ys + dy)[ok], x0 + (xs + dx)[ok]] = a[0, y0 + ys[ok], x0 + xs[ok]]
    fwd = np.empty((1, 2, h, w), dtype=np.float32)
    fwd[0, 0], fwd[0, 1] = dx, dy
    return a, b, fwd, -fwd


def closed_form_count(h, w, dy, dx, s):
    """Scored pixels (s <= x < w - s, s <= y < h - s) whose target (x + dx, y + dy) lies in the crop."""
    nx = max(0, min(w - s, w - dx) - max(s, -dx))
    ny = max(0, min(h - s, h - dy) - max(s, -dy))
    return nx * ny


def test_warped_plane_agrees_with_grid_sample_in_float64():
    """At in-frame samples the warped plane is torch's bilinear grid_sample (align_corners=True: sample coordinates are pixel
    centres) in float64 within 1e-10: the two differ in the normalisation round trip of the coordinates (about 64 * 2^-52 of a pixel
    on values up to 255) and in the order of the four products."""
    for name, kind in (("crop", "general"), ("rows", "general"), ("cols", "exact")):
        c = R.CASE[name]
        for channels, quant in (("rgb", 0), ("y", 1)):
            a, b, fwd, bwd = R.make_case(name, kind, "f32", quant)
            r = R.reference(name, kind, "f32", channels, quant)
            y0, x0, h, w = c.crop
            pb = R.planes(b, channels, bool(quant), R.luma_bt601())[..., y0:y0 + h, x0:x0 + w]
            xf, yf = r.sample
            grid = np.stack([2.0 * xf / (w - 1) - 1.0, 2.0 * yf / (h - 1) - 1.0], axis=-1)
            want = torch.nn.functional.grid_sample(torch.from_numpy(pb), torch.from_numpy(grid), mode="bilinear", align_corners=True).numpy()
            inside = np.broadcast_to(r.in_frame[:, None], want.shape)
            assert inside.sum() > 0.5 * inside.size
            err = np.abs(r.warped - want)[inside].max()
            print(f"[grid_sample {name} {kind} {channels} q{quant}] max |difference| {err:.3e} (bar 1e-10)")
            assert err <= 1e-10
            assert np.isnan(r.warped[~inside]).all()


@pytest.mark.parametrize("dy,dx", [(0, 0), (2, 3), (-1, 4), (3, -2), (-5, -1)])
@pytest.mark.parametrize("shave", [0, 2])
def test_integer_translation_has_zero_error_and_the_closed_form_count(dy, dx, shave):
    h, w, H, W, y0, x0 = 19, 23, 25, 31, 4, 6
    a, b, fwd, bwd = _translation_inputs(h, w, dy, dx, H, W, y0, x0)
    for channels in ("rgb", "y"):
        r = R.warp_error(a, b, fwd, bwd, (y0, x0, h, w), channels, True, shave)
        n = closed_form_count(h, w, dy, dx, shave)
        planes = 3 if channels == "rgb" else 1
        assert 0 < n <= (h - 2 * shave) * (w - 2 * shave)
        assert r.sums[0].tolist() == [0.0, planes * n, n, (h - 2 * shave) * (w - 2 * shave)]
    e, share = R.ewarp(r.sums)
    assert e[0] == 0.0 and share[0] == n / ((h - 2 * shave) * (w - 2 * shave))
    assert np.isnan(R.ewarp(np.array([[0.0, 0.0, 0.0, 12.0]]))[0][0])


DEFECTS = ["sign_flipped", "uv_swapped", "backward_at_pixel", "xb_clamp_missing", "shave_off_by_one", "crop_offset_dropped"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_restatement_sees_planted_defects(defect):
    """A defect loses the closed-form answer of an integer translation and moves the sse of a generated case (one of the two for the
    defects that a constant flow, or a sample off the last column, cannot show)."""
    dy, dx = (2, 3)
    h, w, H, W, y0, x0 = 19, 23, 25, 31, 4, 6
    a, b, fwd, bwd = _translation_inputs(h, w, dy, dx, H, W, y0, x0)
    n = closed_form_count(h, w, dy, dx, 1)
    ok = R.warp_error(a, b, fwd, bwd, (y0, x0, h, w), "rgb", True, 1)
    assert ok.sums[0, 0] == 0.0 and ok.sums[0, 2] == n
    t = R.warp_error(a, b, fwd, bwd, (y0, x0, h, w), "rgb", True, 1, defect=defect)
    print(f"[defect {defect}] translation: good {ok.sums[0].tolist()} bad {t.sums[0].tolist()}")
    if defect != "backward_at_pixel":   # (a constant backward flow is the same at the pixel and at the sample)
        assert not (t.sums[0, 0] == 0.0 and t.sums[0, 2] == n), "the closed form survives the defect"
    if defect == "xb_clamp_missing":
        return   # (visible only where a sample lies on the last column exactly, as the translation's do: weight 0 on what lies beyond the row)
    name = "crop"   # a frame larger than its crop, a shave, two pairs
    c = R.CASE[name]
    a, b, fwd, bwd = R.make_case(name, "general")
    good = R.reference(name, "general", "f32", "rgb", 1)
    bad = R.warp_error(a, b, fwd, bwd, c.crop, "rgb", True, c.shave, defect=defect)
    print(f"[defect {defect}] generated: good {good.sums[0].tolist()} bad {bad.sums[0].tolist()}")
    assert (bad.sums[:, 0] != good.sums[:, 0]).all(), "the sse of every pair moves"


def test_generated_inputs_exercise_all_three_conditions():
    """Asserted here so that no GPU test passes vacuously: in every case the GPU file uses (both kinds, both flow forms) the valid share
    of the case lies in [0.2, 0.95], and each of in frame / consistent / smooth alone removes at least one pixel the other two keep.
    (The tiny case is one pixel per pair: its three pairs are valid, inconsistent alone and out of frame alone; a crop of one pixel has no
    neighbour, so nothing there can be a motion boundary.)"""
    for c in R.CASES:
        for kind in R.KINDS:
            for form in R.FORMS:
                r = R.reference(c.name, kind, form, "rgb", 1)
                share = r.sums[:, 2].sum() / r.sums[:, 3].sum()
                only_frame = int((~r.in_frame & r.consistent & r.smooth).sum())
                only_cons = int((r.in_frame & ~r.consistent & r.smooth).sum())
                only_smooth = int((r.in_frame & r.consistent & ~r.smooth).sum())
                print(f"[{c.name} {kind} {form}] valid share {share:.3f}; removed alone: frame {only_frame}, consistent {only_cons}, smooth {only_smooth}")
                assert 0.2 <= share <= 0.95, (c.name, kind, form, share)
                assert only_frame >= 1 and only_cons >= 1
                assert only_smooth >= 1 or c.name == "tiny"
                assert (r.sums[:, 3] == (c.crop[2] - 2 * c.shave) * (c.crop[3] - 2 * c.shave)).all()
                # the masks are the same whatever is scored: Y and the unquantised frames share them
                y = R.reference(c.name, kind, form, "y", 0)
                assert np.array_equal(y.sums[:, 2:], r.sums[:, 2:]) and (y.sums[:, 1] * 3 == r.sums[:, 1]).all()
    # the case list reaches what its names say
    assert R.n_tiles(R.CASE["tiny"]) == R.n_tiles(R.CASE["aligned"]) == 1 and R.n_tiles(R.CASE["cols"]) == R.n_tiles(R.CASE["rows"]) == 2
    assert R.CASE["rows"].crop[2] == R.TILE_H + 1 and R.CASE["cols"].W % 2 == 1 and (R.CASE["cols"].W * 12) % 16 != 0
    assert R.n_tiles(R.CASE["finish"]) == R.FINISH_THREADS + 2


def test_exact_inputs_are_exact():
    """The "exact" kind: flows in multiples of 1/4 pixel (half holds them), frames that are integers in 0..255 once quantised: every
    bilinear weight is a multiple of 1/4, every product and term a multiple of 2^-8 (2^-12 with the dyadic luma) far below 2^53."""
    for c in R.CASES:
        for quant in (0, 1):
            a, b, fwd, bwd = R.make_case(c.name, "exact", "f32", quant)
            assert np.array_equal(fwd * 4, np.rint(fwd * 4)) and np.array_equal(bwd * 4, np.rint(bwd * 4))
            assert np.array_equal(fwd, fwd.astype(np.float16).astype(np.float32))
            qa = R.quantise(a)
            assert np.array_equal(qa, np.rint(qa)) and qa.min() >= 0 and qa.max() <= 255
            if not quant:
                assert np.array_equal(qa, a)
            for channels, luma in (("rgb", "bt601"), ("y", "dyadic")):
                r = R.reference(c.name, "exact", "f32", channels, quant, luma)
                assert np.array_equal(r.sums[:, 0] * 4096, np.rint(r.sums[:, 0] * 4096)) and r.sums[:, 0].max() * 4096 < 2 ** 53
    a, _, _, _ = R.make_case("aligned", "exact", "f32", 1)
    assert np.isnan(a).any() and (a < 0).any() and (a > 255).any() and (np.abs(a - np.floor(a) - 0.5) == 0).any()
