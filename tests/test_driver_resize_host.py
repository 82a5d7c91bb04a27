"""Host side of the resampler (driver.resize_tables, FrameResizer, ClipRunner's decimate / baseline switches): shapes, dtypes and tap
counts of the tables, their agreement with the independent restatement of tests/_resize_ref.py, and the refusals.  No GPU."""
import numpy as np
import pytest
import torch

import _resize_ref as R
from video_super_resolution_amd import _lib, driver


@pytest.mark.parametrize("n_in,n_out,K", [(64, 32, 9), (63, 21, 13), (64, 16, 17), (128, 16, 33), (11, 11, 5), (53, 16, 15), (16, 64, 5), (17, 34, 5),
                                           (45, 63, 5), (7, 1, 29), (3, 1, 13), (2, 8, 5)])
def test_bicubic_tables(n_in, n_out, K):
    first, weight = driver.resize_tables(n_in, n_out)
    assert first.shape == (n_out,) and first.dtype == np.int32 and weight.shape == (n_out, K) and weight.dtype == np.float32
    assert weight.flags["C_CONTIGUOUS"] and (first >= 0).all() and (first < n_in).all()
    f64, w64, spans = R.tables64(n_in, n_out, "bicubic")
    assert np.array_equal(first, f64)
    # the same definition evaluated twice in float64 and rounded once: within one float32 rounding of the restatement
    assert (np.abs(weight.astype(np.float64) - w64) <= R.U * np.abs(w64) + 1e-15).all()
    assert all((weight[i, hi - lo:] == 0).all() for i, (lo, hi) in enumerate(spans))
    assert np.abs(weight.astype(np.float64).sum(axis=1) - 1.0).max() <= 2 * R.U * K


@pytest.mark.parametrize("n_in,n_out,K", [(64, 32, 5), (64, 16, 9), (128, 16, 17), (11, 11, 3), (16, 64, 3), (53, 16, 9)])
def test_bilinear_tables(n_in, n_out, K):
    first, weight = driver.resize_tables(n_in, n_out, "bilinear")
    assert weight.shape == (n_out, K) and weight.dtype == np.float32 and first.dtype == np.int32
    f64, w64, _ = R.tables64(n_in, n_out, "bilinear")
    assert np.array_equal(first, f64) and (np.abs(weight.astype(np.float64) - w64) <= R.U * np.abs(w64) + 1e-15).all()
    assert (weight >= 0).all()


def test_identity_and_refusals_of_resize_tables():
    first, weight = driver.resize_tables(9, 9)
    # 1 : 1: the cubic is 1 at 0 and 0 at the other integers: every row is a single 1
    assert np.array_equal(weight.sum(axis=1), np.ones(9, dtype=np.float32)) and ((weight == 0) | (weight == 1)).all()
    assert all(first[i] + int(np.argmax(weight[i])) == i for i in range(9))
    with pytest.raises(ValueError, match="unknown kernel 'lanczos'"):
        driver.resize_tables(8, 4, "lanczos")
    with pytest.raises(ValueError, match="sizes must be positive"):
        driver.resize_tables(0, 4)
    with pytest.raises(ValueError, match="needs 37 taps, beyond the 33"):
        driver.resize_tables(90, 10)


def test_frame_resizer_refuses_cpu_tensors_and_wrong_shapes():
    r = driver.FrameResizer((8, 12), (4, 6), device="cpu")   # (the tables are plain tensors; nothing is launched)
    assert r.x_first.dtype == torch.int32 and tuple(r.x_weight.shape) == (6, 9) and tuple(r.y_weight.shape) == (4, 9)
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        r(torch.zeros(1, 8, 12, 3))
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.resize_frames(torch.zeros(1, 8, 12, 3), (4, 6), r.x_first, r.x_weight, r.y_first, r.y_weight)
    with pytest.raises(ValueError, match="tables do not fit"):
        driver.resize_frames(torch.zeros(1, 8, 12, 3), (4, 7), r.x_first, r.x_weight, r.y_first, r.y_weight)


class _Net(torch.nn.Module):
    upscale_factor = 4


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = _Net()


def test_clip_runner_refuses_unknown_switches_before_touching_the_device():
    m = _Model()
    with pytest.raises(ValueError, match="decimate must be 'nearest' or 'bicubic', got 'area'"):
        driver.ClipRunner(m, (256, 256), "nv12", "nv12", scale_down=4, decimate="area")
    with pytest.raises(ValueError, match="baseline must be None or 'bicubic', got 'nearest'"):
        driver.ClipRunner(m, (256, 256), "nv12", "nv12", scale_down=4, score="y", baseline="nearest")
    with pytest.raises(ValueError, match="baseline='bicubic' is scored beside the estimate: it needs score"):
        driver.ClipRunner(m, (256, 256), "nv12", "nv12", scale_down=4, baseline="bicubic")


def test_cli_refuses_a_baseline_without_a_score(capsys):
    with pytest.raises(SystemExit):
        driver.main(["--pix-fmt", "nv12", "--baseline", "bicubic"])
    assert "--baseline needs --score" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        driver.main(["--decimate", "bicubic"])
    assert "--decimate needs --pix-fmt" in capsys.readouterr().err
