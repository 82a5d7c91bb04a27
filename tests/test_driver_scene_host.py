"""The host side of scene-cut detection, without a GPU: `driver.scene_cuts`, the argument errors of the device bindings that are raised
before the device is touched, `ClipRunner(scene=...)` refusing at construction, and the CLI's refusals."""
import types

import numpy as np
import pytest
import torch

from video_super_resolution_amd import _lib, driver


def _model(S):
    """What ClipRunner reads of a model before it allocates anything."""
    return types.SimpleNamespace(model=types.SimpleNamespace(upscale_factor=S))


def test_scene_names_resolve_through_the_driver():
    from video_super_resolution_amd import frames
    for name in ("scene_sums", "scene_flags", "scene_window", "scene_cuts", "SCENE_THRESHOLDS"):
        assert getattr(driver, name) is getattr(frames, name)
    assert driver.SCENE_THRESHOLDS == (15.0, 2.0) and driver.ClipRunner.SCENE == (None, "sad")


def test_scene_cuts_applies_the_rule_on_the_host():
    sums = np.array([[3.0, 1.0], [4.0, 1.0], [100.0, 1.0], [5.0, 1.0], [20.0, 1.0], [22.0, 1.0], [100.0, 1.0], [110.0, 1.0]])
    cuts, m = driver.scene_cuts(sums)
    assert cuts.dtype == np.bool_ and m.dtype == np.float64 and cuts.shape == m.shape == (8,)
    assert m.tolist() == [3.0, 4.0, 100.0, 5.0, 20.0, 22.0, 100.0, 110.0]
    # the cut; the onset of fast motion (one false cut, none after it); a cut; the second of two cuts one pair apart is missed
    assert cuts.tolist() == [False, False, True, False, True, False, True, False]
    assert driver.scene_cuts(sums, (0.0, 0.0))[0].all() and not driver.scene_cuts(sums, (1e30, 2.0))[0].any()
    assert driver.scene_cuts(sums, (15.0, 0.0))[0].tolist() == [False, False, True, False, True, True, True, True]
    # equality flags, at both thresholds; the first pair has no pair before it
    assert driver.scene_cuts([[15.0, 1.0]])[0].tolist() == [True]
    assert driver.scene_cuts([[7.5, 1.0], [15.0, 1.0]])[0].tolist() == [False, True]
    assert driver.scene_cuts([[7.625, 1.0], [15.0, 1.0]])[0].tolist() == [False, False]
    # a tensor of sums is taken as well; no pair: empty results
    cuts_t, m_t = driver.scene_cuts(torch.from_numpy(sums))
    assert np.array_equal(cuts_t, cuts) and np.array_equal(m_t, m)
    cuts0, m0 = driver.scene_cuts(np.zeros((0, 2)))
    assert cuts0.shape == m0.shape == (0,)


@pytest.mark.parametrize("bad", [(15.0,), (15.0, 2.0, 1.0), (-1.0, 2.0), (15.0, -0.5), (float("nan"), 2.0), (15.0, float("inf"))])
def test_thresholds_are_two_finite_values_that_are_not_negative(bad):
    with pytest.raises(ValueError, match="scene thresholds are"):
        driver.scene_cuts([[1.0, 1.0]], bad)
    with pytest.raises(ValueError, match="scene thresholds are"):
        driver.scene_flags(torch.zeros((1, 2), dtype=torch.float64), thresholds=bad)
    with pytest.raises(ValueError, match="scene thresholds are"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, scene="sad", scene_thresholds=bad)


def test_clip_runner_refuses_unknown_scene_switches_before_touching_the_device():
    with pytest.raises(ValueError, match="scene must be None or 'sad', got 'hist'"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, scene="hist")
    with pytest.raises(ValueError, match="scene_thresholds is given but no scene detection is asked for"):
        driver.ClipRunner(_model(4), (64, 96), "nv12", "nv12", scale_down=4, scene_thresholds=(15.0, 2.0))


def test_bindings_refuse_wrong_shapes_and_cpu_tensors():
    f = torch.zeros((4, 6, 3))
    with pytest.raises(ValueError, match="expected two float32 tensors of one shape"):
        driver.scene_sums(f, torch.zeros((4, 5, 3)))
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.scene_sums(f, f)
    with pytest.raises(ValueError, match=r"expected float64 sums \[P,2\]"):
        driver.scene_flags(torch.zeros((3, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="prev must be two float64 values"):
        driver.scene_flags(torch.zeros((3, 2), dtype=torch.float64), prev=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.scene_flags(torch.zeros((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="expected three float32 frames of one shape"):
        driver.scene_window(f, f, torch.zeros((4, 6, 4)))
    with pytest.raises(ValueError, match=r"prev_est must be float32 \[1,H,W,3\] or \[H,W,3\]"):
        driver.scene_window(f, f, f, prev_est=torch.zeros((2, 8, 12, 3)))
    with pytest.raises(ValueError, match="no integer multiple"):
        driver.scene_window(f, f, f, prev_est=torch.zeros((1, 9, 12, 3)))
    with pytest.raises(ValueError, match="no integer multiple"):
        driver.scene_window(f, f, f, prev_est=torch.zeros((1, 8, 18, 3)))      # x2 down, x3 across
    with pytest.raises(ValueError, match="flag_ab must be one int32 element"):
        driver.scene_window(f, f, f, flag_ab=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.VsrHipError, match="CPU tensor"):
        driver.scene_window(f, f, f)


@pytest.mark.parametrize("argv,words", [
    (["--scene", "sad"], "--scene needs --pix-fmt"),
    (["--pix-fmt", "nv12", "--scene-thresholds", "15", "2"], "--scene-thresholds needs --scene"),
    (["--cut-at", "2", "--frames", "6"], "--cut-at needs --pix-fmt"),
    (["--pix-fmt", "nv12", "--cut-at", "6", "--frames", "6"], "--cut-at needs --pix-fmt and a frame index inside the clip"),
    (["--pix-fmt", "nv12", "--cut-at", "0", "--frames", "6"], "--cut-at needs --pix-fmt and a frame index inside the clip"),
])
def test_cli_refuses_scene_switches_that_make_no_sense(argv, words, capsys):
    with pytest.raises(SystemExit):
        driver.main(argv)
    assert words in capsys.readouterr().err
