"""Host side of the training patches (no GPU): `patch_table`'s draw order, its rows against the library's bounds rule, `patch_item`'s
storage, the pixel phase of the nearest LR patch in the reference module, and the command line's new options."""
import numpy as np
import pytest
import torch

import _patch_ref as R
from video_super_resolution_amd import driver, frames


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
def test_patch_table_is_the_restated_draw(seed):
    for (B, G, n, H, W, Ph, Pw, S) in ((16, 8, 3, 144, 160, 128, 128, 2), (5, 4, 4, 96, 120, 64, 64, 4), (9, 6, 3, 90, 130, 60, 90, 3),
                                      (64, 3, 3, 64, 64, 64, 64, 1)):
        got = driver.patch_table(np.random.RandomState(seed), B, G, n, (H, W), (Ph, Pw), S)
        assert got.dtype == np.int32 and got.shape == (B, 4)
        assert np.array_equal(got, R.draw_table(seed, B, G, n, H, W, Ph, Pw, S)), (seed, B, G, n, H, W, Ph, Pw, S)
    # one stream drawn twice in a row continues: the second table is the restated second draw
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    for _ in range(2):
        assert np.array_equal(driver.patch_table(a, 4, 8, 3, (144, 160), 128, 2), R.draw_table(b, 4, 8, 3, 144, 160, 128, 128, 2))
    assert driver.PATCH_FLAGS is frames.PATCH_FLAGS


@pytest.mark.parametrize("H, W, patch, S", [(128, 128, 128, 2),       # H - ch == 0
                                            (130, 132, 128, 2),       # H - ch == S
                                            (135, 139, 128, 4),       # H - ch is no multiple of S
                                            (100, 77, (60, 75), 3)])  # not square
def test_every_row_passes_the_librarys_bounds_rule(H, W, patch, S):
    Ph, Pw = (patch, patch) if isinstance(patch, int) else patch
    t = driver.patch_table(np.random.RandomState(5), 64, 6, 3, (H, W), patch, S)
    for row in t:
        assert R.row_ok(row, 6, 3, H, W, Ph, Pw, S, lr_src=True), row   # (origins are multiples of S: both LR modes take the row)
    assert (t[:, 1] % S == 0).all() and (t[:, 2] % S == 0).all()
    if Ph == Pw:   # few origins: 64 draws reach every one of them, the last included
        assert set(t[:, 1]) == set(range(0, H - Ph + 1, S)) and set(t[:, 2]) == set(range(0, W - Pw + 1, S))


def test_the_draws_cover_flags_frames_and_origins():
    t = driver.patch_table(np.random.RandomState(0), 256, 8, 3, (144, 160), 128, 2)
    assert set(t[:, 3]) == set(range(16))
    assert set(t[:, 0]) == set(range(6))
    assert t[:, 1].min() == 0 and t[:, 1].max() == 16
    assert t[:, 2].min() == 0 and t[:, 2].max() == 32


def test_augment_off_and_non_square_patches():
    t = driver.patch_table(np.random.RandomState(3), 64, 8, 3, (144, 160), 128, 2, augment=False)
    assert (t[:, 3] == 0).all()
    assert np.array_equal(t, R.draw_table(3, 64, 8, 3, 144, 160, 128, 128, 2, augment=False))
    t = driver.patch_table(np.random.RandomState(3), 128, 8, 3, (144, 160), (64, 96), 2)
    assert (t[:, 3] & 4 == 0).all() and len(set(t[:, 3])) == 8
    t = driver.patch_table(np.random.RandomState(3), 128, 8, 3, (144, 160), (64, 96), 2, transpose=True)
    assert (t[:, 3] & 4).any() and np.array_equal(t, R.draw_table(3, 128, 8, 3, 144, 160, 64, 96, 2, transpose=True))
    for row in t:
        assert R.row_ok(row, 8, 3, 144, 160, 64, 96, 2, lr_src=True)
    t = driver.patch_table(np.random.RandomState(3), 128, 8, 3, (144, 160), 128, 2, transpose=False)
    assert (t[:, 3] & 4 == 0).all()
    with pytest.raises(ValueError, match="does not fit"):
        driver.patch_table(np.random.RandomState(0), 1, 8, 3, (144, 160), (64, 150), 2, transpose=True)   # transposed it is 150 rows
    with pytest.raises(ValueError, match="does not fit"):
        driver.patch_table(np.random.RandomState(0), 1, 8, 3, (100, 160), 128, 2)
    with pytest.raises(ValueError, match="multiple of S"):
        driver.patch_table(np.random.RandomState(0), 1, 8, 3, (144, 160), 127, 2)
    with pytest.raises(ValueError, match="n <= G"):
        driver.patch_table(np.random.RandomState(0), 1, 2, 3, (144, 160), 128, 2)


def _storage(t):
    return t.untyped_storage().data_ptr()


def test_patch_item_windows_and_storage():
    B, n, Hp, Wp, S = 2, 5, 8, 12, 2
    hr = torch.arange(B * n * Hp * Wp * 3, dtype=torch.float32).reshape(B, n, Hp, Wp, 3)
    lr = -torch.arange(B * n * (Hp // S) * (Wp // S) * 3, dtype=torch.float32).reshape(B, n, Hp // S, Wp // S, 3)
    hr0 = hr.clone()
    data, target, high_frames = driver.patch_item(hr, lr, 1)
    assert tuple(data.shape) == (n - 2, 3, Hp // S, Wp // S, 3) and tuple(target.shape) == (n - 2, 1, Hp, Wp, 3)
    assert tuple(high_frames.shape) == (n - 2, 3, Hp, Wp, 3)
    for t in range(n - 2):
        assert torch.equal(data[t], lr[1, t:t + 3]) and data[t].is_contiguous()
        assert torch.equal(high_frames[t], hr[1, t:t + 3]) and torch.equal(target[t, 0], hr[1, t + 1])
    # own storage: what VSR.forward does to high_frames[t][1] reaches neither the next window, the target nor hr
    assert len({_storage(hr), _storage(target), _storage(high_frames)}) == 3
    assert high_frames.is_contiguous() and target.is_contiguous()
    high_frames[0][1].fill_(-1.0)
    assert torch.equal(hr, hr0) and torch.equal(high_frames[1][0], hr[1, 1]) and torch.equal(target[0, 0], hr[1, 1])
    with pytest.raises(ValueError, match="n >= 3"):
        driver.patch_item(hr[:, :2], lr[:, :2], 0)


def test_the_reference_keeps_the_inference_phase_under_a_flip():
    G, H, W, S, P = 3, 12, 16, 2, 8
    src = np.arange(G * H * W * 3, dtype=np.float32).reshape(G, H, W, 3)
    for flags in (R.FLIP_Y, R.FLIP_X, R.FLIP_X | R.FLIP_Y):
        table = np.array([[0, 2, 4, flags]], dtype=np.int32)
        hr = R.gather_hr(src, table, 3, P, P)
        lr = R.gather_lr_nearest(src, table, 3, P, P, S)
        assert np.array_equal(lr, hr[:, :, ::S, ::S])                      # LR[i][j] = HR[iS][jS] of the augmented patch
        wrong = R.gather_lr_nearest_wrong_phase(src, table, 3, P, P, S)   # decimate first, flip afterwards: HR[iS+S-1]
        assert wrong.shape == lr.shape and not np.array_equal(lr, wrong)
        if flags == R.FLIP_Y:
            assert np.array_equal(wrong, hr[:, :, S - 1::S, ::S])
    # without a flip (and with the transposition alone) the two orders agree: the phase only moves under a flip
    for flags in (0, R.TRANSPOSE, R.REVERSE_TIME):
        table = np.array([[0, 2, 4, flags]], dtype=np.int32)
        assert np.array_equal(R.gather_lr_nearest(src, table, 3, P, P, S), R.gather_lr_nearest_wrong_phase(src, table, 3, P, P, S))
    # bits, not numbers: a NaN payload and a negative zero come through
    odd = src.copy().view(np.uint32)
    odd[0, 2, 4] = (0x7FC12345, 0x80000000, 0xFFFFFFFF)
    hr = R.gather_hr(odd.view(np.float32), np.array([[0, 2, 4, 0]], dtype=np.int32), 3, P, P)
    assert hr.dtype == np.uint32 and tuple(hr[0, 0, 0, 0]) == (0x7FC12345, 0x80000000, 0xFFFFFFFF)


def test_patch_gather_refuses_host_tensors_and_bad_tables():
    src = torch.zeros(4, 16, 16, 3)
    with pytest.raises(Exception, match="CPU tensor"):
        driver.patch_gather(src, np.zeros((1, 4), np.int32), 3, 8, 2)
    with pytest.raises(ValueError, match=r"int32 \[B,4\]"):
        driver.patch_gather(src, np.zeros((4,), np.int32), 3, 8, 2)
    with pytest.raises(ValueError, match="multiple of S"):
        driver.patch_gather(src, np.zeros((1, 4), np.int32), 3, 9, 2)
    with pytest.raises(ValueError, match="lr_src must be"):
        driver.patch_gather(src, np.zeros((1, 4), np.int32), 3, 8, 2, lr_src=torch.zeros(4, 8, 7, 3))


@pytest.mark.parametrize("argv, words", [
    (["--patch", "64"], "--patch needs --input and --train-steps"),
    (["--train-steps", "2", "--group", "4"], "--group needs --input and --train-steps"),
    (["--input", "a.y4m", "--frames-per-sample", "3"], "--frames-per-sample needs --input and --train-steps"),
    (["--input", "a.y4m", "--seed", "3"], "--seed needs --input and --train-steps"),
    (["--input", "a.y4m", "--save", "out"], "--save needs --input and --train-steps"),
    (["--input", "a.y4m", "--train-steps", "2", "--output", "o.y4m"], "it takes no --output"),
    (["--input", "a.y4m", "--train-steps", "2", "--score", "y"], "it takes no --score"),
    (["--input", "a.y4m", "--train-steps", "2", "--scene", "sad"], "it takes no --scene"),
    (["--input", "a.y4m", "--train-steps", "2", "--scale-down", "2"], "it takes no --scale-down"),
    (["--input", "a.y4m", "--train-steps", "0"], "--input with --train-steps takes a positive count"),
    (["--input", "a.y4m", "--train-steps", "2", "--patch", "0"], "--patch is a positive LR patch edge"),
    (["--input", "a.y4m", "--train-steps", "2", "--frames-per-sample", "2"], "--frames-per-sample is at least 3"),
    (["--input", "a.y4m", "--train-steps", "2", "--frames-per-sample", "5", "--group", "4"], "--group must hold a sample"),
    (["--input", "a.y4m", "--train-steps", "2", "--size", "64x64"], "a .y4m file carries its size and format"),
    (["--input", "a.y4m", "--cut-at", "2"], "--input takes no --cut-at"),
    (["--input", "a.y4m", "--loss-path", "fused"], "--loss-path needs --train-steps"),
    (["--checkpoint", "c.pth.tar", "--train-steps", "2"], "--checkpoint needs --input"),
])
def test_cli_refuses_training_switches_that_make_no_sense(argv, words, capsys):
    with pytest.raises(SystemExit):
        driver.main(argv)
    assert words in capsys.readouterr().err
