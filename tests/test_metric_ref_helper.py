"""tests/_metric_ref.py, the float64 restatement the device metric is compared with, pinned on the CPU: it agrees with an independent
scipy evaluation per pixel, gives exactly 1 for equal frames, and sees the defects a wrong kernel would have (a window shifted by one
tap, a shave off by one, a quantise that truncates)."""
import numpy as np
import pytest

import _metric_ref as R

SIZES = [(11, 11), (12, 75), (23, 140), (76, 64)]
IMAGES = [("textured", R.textured), ("near_flat", R.near_flat)]


def _pair(make, H, W):
    a, b = make(np.random.RandomState(H * 1000 + W), 1, H, W)
    return a, b


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name,make", IMAGES, ids=[n for n, _ in IMAGES])
def test_ssim_map_agrees_with_scipy_per_pixel(name, make, size):
    """scipy's gaussian_filter with sigma 1.5 truncated at 3.5 sigma is the same 11-tap window; cropped by 5 its `reflect` border never
    enters.  Both sides are float64 and differ only in the order of their sums: per pixel within 1e-10 (measured: at most 1.24e-12, on the
    near-flat images; 2.5e-14 on the textured ones)."""
    ndi = pytest.importorskip("scipy.ndimage")
    a, b = _pair(make, *size)
    pa, pb = R.planes(a, "rgb", True, 0)[0], R.planes(b, "rgb", True, 0)[0]

    def g(v):
        return np.stack([ndi.gaussian_filter(p, sigma=1.5, truncate=3.5, mode="reflect")[5:-5, 5:-5] for p in v])

    ma, mb = g(pa), g(pb)
    saa, sbb, sab = g(pa * pa) - ma * ma, g(pb * pb) - mb * mb, g(pa * pb) - ma * mb
    want = ((2 * ma * mb + R.C1) * (2 * sab + R.C2)) / ((ma * ma + mb * mb + R.C1) * (saa + sbb + R.C2))
    got = R.ssim_map(pa, pb)
    assert got.shape == want.shape == (3, size[0] - 10, size[1] - 10)
    err = float(np.abs(got - want).max())
    print(f"[ssim ref vs scipy {name} {size}] max |diff| per pixel {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equal_frames_give_exactly_one_everywhere(size):
    for _, make in IMAGES + [("gaussian", R.gaussian)]:
        a, _ = _pair(make, *size)
        for channels, luma4 in (("rgb", None), ("y", LUMA)):
            for quant in (False, True):
                p = R.planes(a, channels, quant, 0, luma4)
                assert (R.ssim_map(p, p.copy()) == 1.0).all()
                m = R.metrics(a, a.copy(), channels, quant, 0, luma4)
                assert m[0, 0] == 0.0 and m[0, 2] == m[0, 3] == p.shape[1] * (size[0] - 10) * (size[1] - 10)


LUMA = np.array([0.25678825, 0.5041294, 0.09790588, 16.0], dtype=np.float32)   # BT.601 limited range, 8 bit: {a0, a1, a2, o}


def test_window_sums_to_one_and_is_symmetric():
    w = R.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) <= 2 ** -52 and np.array_equal(w, w[::-1]) and w.argmax() == 5


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name,make", IMAGES, ids=[n for n, _ in IMAGES])
def test_a_window_shifted_by_one_tap_moves_the_frame_mean(name, make, size):
    """The bar of the device test (1e-10) must sit far below what a real defect does: a window centred on tap 6 instead of 5 moves the
    frame mean by more than 1e-7 on every test image (measured: 7.0e-7 on the near-flat 76 x 64 image at least, 4.5e-6 .. 9.6e-4 textured)."""
    a, b = _pair(make, *size)
    good = R.metrics(a, b)[0]
    bad = R.metrics(a, b, win=R.window(centre=6.0))[0]
    diff = abs(good[2] / good[3] - bad[2] / bad[3])
    print(f"[shifted window {name} {size}] frame mean moves by {diff:.2e}")
    assert diff > 1e-7


@pytest.mark.parametrize("size", [(23, 140), (76, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_shave_off_by_one_and_a_truncating_quantise_change_the_sse(size):
    rs = np.random.RandomState(size[0])
    a, b = R.awkward(rs, 1, *size)
    good = R.metrics(a, b, shave=3, want_ssim=False)[0]
    assert good[1] == 3 * (size[0] - 6) * (size[1] - 6)
    for bad in (R.metrics(a, b, shave=2, want_ssim=False)[0], R.metrics(a, b, shave=4, want_ssim=False)[0],
                R.metrics(a, b, shave=3, want_ssim=False, truncate=True)[0]):
        assert bad[0] != good[0]
    # the quantisation itself: ties to even on both parities, the clamps, NaN -> 0
    q = R.quantise(np.array([0.5, 1.5, 2.5, 253.5, 254.5, 255.5, -3.2, 300.0, np.nan, -0.0], dtype=np.float32))
    assert q.tolist() == [0, 2, 2, 254, 254, 255, 0, 255, 0, 0]


def test_luma_follows_the_nested_form_in_double():
    rgb = np.array([[[[10.0, 200.0, 33.0]]]], dtype=np.float32)
    a0, a1, a2, o = (float(v) for v in LUMA)
    assert R.luma(rgb, LUMA)[0, 0, 0] == ((o + a0 * 10.0) + a1 * 200.0) + a2 * 33.0
    assert R.planes(rgb, "y", True, 0, LUMA).shape == (1, 1, 1, 1)
