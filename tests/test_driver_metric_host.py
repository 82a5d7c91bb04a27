"""The host side of the frame metric in driver.py, without a GPU: the SSIM window, the step from the device's sums to PSNR / SSIM, the
argument errors of `frame_metrics`, and `ClipRunner(score=...)` refusing at construction what it cannot score."""
import types

import numpy as np
import pytest
import torch

import _metric_ref as R
from video_super_resolution_amd import _lib, driver


def test_ssim_window_sums_to_one_and_is_symmetric():
    w = driver.ssim_window()
    assert w.dtype == np.float64 and w.shape == (11,)
    assert abs(w.sum() - 1.0) <= 2 ** -52 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert np.array_equal(w, R.window())                       # the restatement the device is compared with uses the same taps
    assert w[5] / w[4] == pytest.approx(np.exp(1 / 4.5))       # sigma 1.5


def test_psnr_ssim_is_the_host_step_and_handles_a_zero_sse():
    sums = np.array([[0.0, 300.0, 290.0, 300.0],              # equal frames: PSNR inf
                     [65025.0 * 3, 300.0, 150.0, 200.0],      # MSE = 255^2 / 100 -> 20 dB
                     [12.0, 48.0, 0.0, 0.0]])                 # SSIM not asked for
    psnr, ssim = driver.psnr_ssim(sums)
    assert psnr.shape == ssim.shape == (3,)
    assert np.isposinf(psnr[0]) and psnr[1] == pytest.approx(20.0, abs=1e-12) and psnr[2] == 10 * np.log10(255.0 ** 2 * 48 / 12)
    assert ssim[0] == 290.0 / 300.0 and ssim[1] == 0.75 and np.isnan(ssim[2])
    p2, s2 = driver.psnr_ssim(torch.from_numpy(sums))          # a tensor is copied to the host
    assert np.array_equal(p2, psnr) and np.array_equal(s2, ssim, equal_nan=True)
    p3, _ = driver.psnr_ssim(np.array([0.0, 0.0, 5.0, 10.0]))  # one row; PSNR not asked for
    assert np.isnan(p3[0])


def test_frame_metrics_argument_errors():
    a = torch.zeros(2, 16, 20, 3)
    with pytest.raises(ValueError, match="unknown channels"):
        driver.frame_metrics(a, a, channels="yuv")
    with pytest.raises(ValueError, match="what must name"):
        driver.frame_metrics(a, a, what=("mse",))
    with pytest.raises(ValueError, match="what must name"):
        driver.frame_metrics(a, a, what=())
    with pytest.raises(ValueError, match="one shape"):
        driver.frame_metrics(a, a[:1])
    with pytest.raises(ValueError, match="one shape"):
        driver.frame_metrics(a[..., :2], a[..., :2])
    with pytest.raises(ValueError, match="one shape"):
        driver.frame_metrics(a[None], a[None])
    with pytest.raises(ValueError, match="shave"):
        driver.frame_metrics(a, a, shave=8)
    with pytest.raises(ValueError, match="shave"):
        driver.frame_metrics(a, a, shave=-1)
    with pytest.raises(ValueError, match="SSIM needs 11"):
        driver.frame_metrics(a, a, shave=3)                    # 16 - 6 = 10
    with pytest.raises(ValueError, match="unknown matrix"):
        driver.frame_metrics(a, a, channels="y", matrix="bt470")
    # no CPU fallback: tensors that pass every check still have to live on the device
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.frame_metrics(a, a)
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.frame_metrics(a[0], a[0], channels="y", what="psnr", shave=3)


def _model(S):
    """What ClipRunner reads of a model before it allocates anything."""
    return types.SimpleNamespace(model=types.SimpleNamespace(upscale_factor=S))


@pytest.mark.parametrize("score", ["rgb", "y"])
def test_clip_runner_refuses_to_score_frames_of_another_shape(score):
    with pytest.raises(ValueError, match="needs output frames of the source's shape"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=1, score=score)      # 256 x 384 out
    with pytest.raises(ValueError, match="needs output frames of the source's shape"):
        driver.ClipRunner(_model(2), (64, 96), "nv12", "nv12", scale_down=4, score=score)      # 32 x 48 out
    with pytest.raises(ValueError, match="needs output frames of the source's shape"):
        driver.ClipRunner(_model(4), (66, 96), "nv12", "nv12", scale_down=4, score=score)      # 66 // 4 * 4 = 64


def test_clip_runner_refuses_unknown_scores_and_shaves():
    with pytest.raises(ValueError, match="score must be"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, score="ssim")
    with pytest.raises(ValueError, match="nothing is scored"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, shave=4)
    with pytest.raises(ValueError, match="leaves less than SSIM's 11 pixels"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, score="y", shave=27)
    with pytest.raises(ValueError, match="leaves less than SSIM's 11 pixels"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, score="y", shave=-1)


def test_the_luma_of_frame_metrics_is_row_0_of_yuv_coefficients():
    """BT.601 limited range by default: Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255."""
    c = driver.yuv_coefficients("yuv420p", "bt601", False)
    assert c.dtype == np.float32
    assert np.allclose(c[:3] * 255, [65.481, 128.553, 24.966], rtol=1e-6) and c[9] == 16.0
