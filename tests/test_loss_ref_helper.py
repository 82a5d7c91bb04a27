"""tests/_loss_ref.py (the float64 restatement the device tests of libvsr_hip_loss.so compare with) against the reference's own masked
arrays (fixture g10, written by the imported reference) and against the torch float32 arithmetic of loss.SR_loss on the CPU."""
import numpy as np
import pytest
import torch

import _loss_ref as R
from video_super_resolution_amd import loss as LS


def _g10_case(g, rep):
    """outputs = [hr0, out_rep, hr2] (high_frames at loss time: frame 1 overwritten by the output, video_super_resolution.py:66),
    target = hr1."""
    hr = g["hr"].astype(np.float32)
    return np.stack([hr[0], g[f"out{rep}"][0], hr[2]]), hr[1]


@pytest.mark.parametrize("rep", [0, 1])
def test_masked_frames_equal_the_references_arrays_exactly(golden, rep):
    g = golden("g10_loss")
    outputs, target = _g10_case(g, rep)
    f8 = R.frames8(outputs, target, g["mask"])
    assert np.array_equal(f8[:3], outputs) and np.array_equal(f8[3], target)
    assert np.array_equal(f8[4:7], g[f"masked_flow{rep}"].astype(np.float32))          # getFlowMaskedOutputs: mO0, mO1, mO2
    assert np.array_equal(f8[5:6], g[f"masked_sr_out{rep}"].astype(np.float32))        # getSRMaskedOutputs: mO1 ...
    if rep == 0:
        assert np.array_equal(f8[7:8], g["masked_sr_tgt0"].astype(np.float32))         # ... and mT
    m = g["mask"].reshape(-1)
    assert 0 < m.sum() < m.size                                                        # both branches of the rule were used
    assert (f8[4:].reshape(4, -1)[:, m] == 0).all()
    # the mask is read at the element's own flat index: the per-pixel reading (mask[c, y, x]) gives other frames on this fixture
    per_pixel = np.moveaxis(g["mask"], 0, 2)
    assert not np.array_equal(R.masked_frame(outputs[1], per_pixel), f8[5])


def test_masking_rule_examples():
    v = np.array([255.9, 256.5, 300.2, -0.5, -3.7, -256.0, 0.0, -0.0, 2147483520.0, 255.0, 256.0, -1.0], dtype=np.float32)
    got = R.masked_frame(v, np.zeros(v.size, dtype=bool))
    assert got.tolist() == [255.0, 0.0, 44.0, 0.0, 253.0, 0.0, 0.0, 0.0, 128.0, 255.0, 0.0, 255.0]
    assert not np.signbit(got).any()
    assert np.array_equal(got, v.astype(np.int64).astype(np.uint8).astype(np.float32))   # numpy's own C cast, where it is defined
    assert (R.masked_frame(v, np.ones(v.size, dtype=np.uint8)) == 0).all()
    h = R.nhwc4(np.broadcast_to(v[:9].reshape(1, 1, 3, 3), (8, 1, 3, 3)).copy())
    assert h.shape == (8, 1, 3, 4) and (h[..., 3] == 0).all() and np.isinf(h[0, 0, 2, 2]) and np.signbit(h[0, 0, 2, 1])


def _cases(golden):
    g = golden("g10_loss")
    rs = np.random.RandomState(5)
    small = (rs.uniform(-40, 300, (3, 17, 23, 3)).astype(np.float32), rs.uniform(-40, 300, (17, 23, 3)).astype(np.float32),
             rs.rand(3 * 17 * 23) < 0.4)
    return [small, _g10_case(g, 1) + (g["mask"],)]


def test_image_and_tv_terms_agree_with_sr_loss_in_float32(golden):
    """loss.SR_loss forms `mse_loss(output, target)` and `tv_loss(output)` in float32 on the permuted frames.  With u = 2^-24: every
    term (a - b)^2 carries at most 3 roundings (the difference, the square and, for MSE's mean, none more), a float32 sum of n
    non-negative terms in any order at most n - 1 more, the division(s), the factor 2 and the final addition of TV at most 4, and the
    helper's own rounding of its float64 value to float32 one: |torch - helper| <= gamma(n + 8) * helper with gamma(k) = k u / (1 - k u),
    n the number of terms of the longest sum (3 H W for the image term, 3 H (W - 1) or 3 (H - 1) W for TV)."""
    u = 2.0 ** -24
    mse, tvl = LS.SR_loss().mse_loss, LS.SR_loss().tv_loss
    for outputs, target, mask in _cases(golden):
        H, W = outputs.shape[1:3]
        n = 3 * H * W
        bound = (n + 8) * u / (1 - (n + 8) * u)
        s, terms, masked, _ = R.pixel_terms(outputs, target, mask)
        f8 = R.frames8(outputs, target, mask)
        for k, (a, b) in enumerate(R.SSE_PAIRS):
            ta = torch.from_numpy(f8[a:a + 1]).permute(0, 3, 1, 2)
            tb = torch.from_numpy(f8[b:b + 1]).permute(0, 3, 1, 2)
            image, tv = float(mse(ta, tb)), float(tvl(ta))
            assert R.TERM_TV[k] == a                                   # the TV of the call's first frame
            print(f"[{H}x{W} term {k}] image {image:.6f} vs {terms[k, 0]:.6f}, tv {tv:.6f} vs {terms[k, 1]:.6f}, bound {bound:.2e}")
            assert abs(image - float(terms[k, 0])) <= bound * float(terms[k, 0])
            assert abs(tv - float(terms[k, 1])) <= bound * float(terms[k, 1])
        assert np.array_equal(masked, f8[4:])


def test_integer_inputs_give_integer_sums():
    rs = np.random.RandomState(2)
    outputs = rs.randint(-300, 601, (3, 5, 7, 3)).astype(np.float32)
    target = rs.randint(-300, 601, (5, 7, 3)).astype(np.float32)
    mask = rs.rand(105) < 0.5
    f8 = R.frames8(outputs, target, mask).astype(np.int64)
    s = R.sums14(f8.astype(np.float32))
    want = [((f8[a] - f8[b]) ** 2).sum() for a, b in R.SSE_PAIRS]
    for k in R.TV_FRAMES:
        want += [((f8[k][1:] - f8[k][:-1]) ** 2).sum(), ((f8[k][:, 1:] - f8[k][:, :-1]) ** 2).sum()]
    assert s.tolist() == [float(v) for v in want]
