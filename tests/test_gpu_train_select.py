"""`ClipTrainer(avoid_cuts=..., act_min=...)`: no sample across a scene cut, none preferred on a flat patch, and nothing changed with both
options off.  An 8-frame 160 x 192 yuv420p clip in a Y4M file: five frames of one `driver.synthetic_video` seed, three of another, the
left 64 columns a constant band; a x2 model (fp32), LR patches of 64 x 64, one group of 8 frames.

The two scenes have the same statistics and a third of the frame is the band, so the pair across the cut differs by about 12 luma codes per
pixel against 4.8 for the motion inside a scene: below the default t_abs = 15, which is meant for real cuts.  The runs here pass
cut_thresholds = (8, 2).  act_min = 5: the textured cells have 3.6 to 9.7 per pixel, a crop that starts in the band averages below 5."""
import copy
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _cell_ref as R  # noqa: E402
from video_super_resolution_amd import VSR, driver, optim, y4m  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

H, W, TA, TB, S, FMT = 160, 192, 5, 3, 2, "yuv420p"
T, CUT = TA + TB, TA - 1          # the planted pair is (CUT, CUT + 1)
BAND = 64
THRESHOLDS, ACT_MIN = (8.0, 2.0), 5.0
KW = dict(patch=64, group=8, frames_per_sample=3, samples_per_group=2, seed=3)


@pytest.fixture(scope="module")
def clip_bytes():
    video = np.concatenate([driver.synthetic_video(TA, H, W, seed=1234), driver.synthetic_video(TB, H, W, seed=77)]).copy()
    video[:, :, :BAND] = 16
    return driver.frames_to_pix(torch.from_numpy(video).cuda().float(), FMT).cpu().numpy()


@pytest.fixture(scope="module")
def clip(clip_bytes, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_select") / "in.y4m")
    with y4m.Y4MWriter(path, (H, W), FMT, (25, 1), "left", False) as w:
        for fr in clip_bytes:
            w.write(fr)
    return path


@pytest.fixture(scope="module")
def base_model():
    m = fill_module_(VSR(upscale_factor=S).eval(), seed=0).cuda()
    m.precision = m.model.precision = "fp32"
    return m


@pytest.fixture(scope="module")
def resident(clip_bytes):
    """The group as the trainer holds it: the file's frames converted at full size, float32 [T,H,W,3] on the device."""
    coef = driver.pix_coefficients(FMT, "bt709", False, inverse=True)
    src = torch.empty((T, H, W, 3), dtype=torch.float32, device="cuda")
    for g in range(T):
        driver.pix_ingest(torch.from_numpy(clip_bytes[g]).cuda(), (H, W), FMT, coef, "left", lr_out=src[g])
    return src


def _trainer(base_model, **kw):
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    return m, opt, driver.ClipTrainer(m, opt, (H, W), FMT, **{**KW, **kw})


@pytest.fixture(scope="module")
def selected(base_model, clip):
    _, _, tr = _trainer(base_model, avoid_cuts=True, cut_thresholds=THRESHOLDS, act_min=ACT_MIN)
    with y4m.Y4MReader(clip) as src:
        steps = tr.run_stream(src)
    return tr, steps


def test_the_planted_cut_is_found_and_no_sample_straddles_it(selected, resident):
    tr, steps = selected
    assert steps == 2 and tr.losses.shape == (2,) and np.isfinite(tr.losses).all()
    assert tr.cuts == [CUT] and tr.cut_m.shape == (1,) and tr.cut_m[0] >= THRESHOLDS[0]
    assert tr.samples_skipped == 0 and (tr.avoid_cuts, tr.cut_thresholds, tr.act_min, tr.tries) == (True, THRESHOLDS, ACT_MIN, 8)
    cuts = np.zeros(T - 1, dtype=bool)
    cuts[CUT] = True
    assert len(tr.tables) == 1 and tr.tables[0].shape == (2, 4) and not any(R.straddles(row, 3, cuts) for row in tr.tables[0])
    # the device map of the resident group is the restatement's, and the cut's m is `scene_sums`' on the same frames
    stats = driver.cell_stats(resident).cpu().numpy()
    assert np.array_equal(stats, R.cell_stats(resident.cpu().numpy()))
    got_cuts, m = driver.cell_cuts(stats, (H, W), THRESHOLDS)
    assert np.array_equal(got_cuts, cuts) and m[CUT] == tr.cut_m[0]
    print(f"m per pair: {m.round(3).tolist()}")


def test_every_row_obeys_the_selection_rule_against_the_restatement(selected, resident):
    tr, _ = selected
    stats = driver.cell_stats(resident).cpu().numpy()
    cuts, _ = R.cell_cuts(stats, (H, W), THRESHOLDS)
    table, scores, tried, candidates = R.select(np.random.RandomState(KW["seed"]), 2, T, 3, (H, W), 128, S, cuts=cuts, stats=stats,
                                                act_min=ACT_MIN, tries=8)
    assert np.array_equal(tr.tables[0], table) and np.array_equal(tr.scores, scores) and np.array_equal(tr.tried, tried)
    assert tr.scores.dtype == np.float64 and tr.tried.dtype == np.int32
    print(f"rows {table.tolist()}, scores {scores.round(3).tolist()}, tried {tried.tolist()}")
    for b in range(2):
        drawn = candidates[b]
        if scores[b] >= ACT_MIN:
            assert all(sc < ACT_MIN for _, sc in drawn[:-1]) and tuple(table[b]) == drawn[-1][0]
        else:
            best = max(sc for _, sc in drawn)
            assert tried[b] == 8 and scores[b] == best and tuple(table[b]) == next(row for row, sc in drawn if sc == best)


def _hand_made_step(base_model, resident, table):
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    m.train()
    hr, lr = driver.patch_gather(resident, table, 3, 128, S)
    data, target, high_frames = driver.patch_item(hr, lr, 0)
    return float(driver.train_item(m, opt, data, target, high_frames))


def test_both_options_off_is_the_trainer_as_it_was(base_model, clip, resident):
    """The tables are a plain `patch_table` replay and the first loss is the hand-made step's, within the hand-made step's own run-to-run
    difference (as tests/test_gpu_train_clip.py measures it)."""
    _, _, tr = _trainer(base_model)
    calls = []
    from video_super_resolution_amd import clip_trainer
    real = clip_trainer.cell_stats
    clip_trainer.cell_stats = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        with y4m.Y4MReader(clip) as src:
            assert tr.run_stream(src) == 2
    finally:
        clip_trainer.cell_stats = real
    assert calls == []                                        # no launch is added
    rng = np.random.RandomState(KW["seed"])
    want = driver.patch_table(rng, 2, T, 3, (H, W), 128, S)
    assert len(tr.tables) == 1 and np.array_equal(tr.tables[0], want)
    assert tr.cuts == [] and tr.samples_skipped == 0 and tr.scores.shape == (0,) and tr.tried.shape == (0,) and tr.cut_m.shape == (0,)
    a = _hand_made_step(base_model, resident, tr.tables[0])
    b = _hand_made_step(base_model, resident, tr.tables[0])
    got = float(np.float32(tr.losses[0]))
    print(f"first loss: hand-made {a!r} and {b!r} (difference {abs(a - b)!r}), trainer {got!r} (difference {abs(got - a)!r})")
    assert math.isfinite(a) and abs(got - a) <= abs(a - b)


def test_a_group_without_a_run_free_of_cuts_is_skipped_and_counted(base_model, clip):
    """Groups of three frames, a sample is the whole group: frames 0..2 train, frames 3..5 hold the cut, frames 6..7 are a short group."""
    _, _, tr = _trainer(base_model, group=3, samples_per_group=1, avoid_cuts=True, cut_thresholds=THRESHOLDS)
    with y4m.Y4MReader(clip) as src:
        assert tr.run_stream(src) == 1
    assert tr.cuts == [CUT] and tr.samples_skipped == 1 and tr.frames_skipped == 2
    assert [t.shape for t in tr.tables] == [(1, 4), (0, 4)]
    assert np.array_equal(tr.tables[0], driver.patch_table(np.random.RandomState(KW["seed"]), 1, 3, 3, (H, W), 128, S))
    assert np.isnan(tr.scores).all() and tr.tried.tolist() == [1]      # no activity bar: the first candidate


def test_the_trainer_refuses_options_that_make_no_sense(base_model):
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="cut_thresholds is given but cuts are not avoided"):
        driver.ClipTrainer(m, opt, (H, W), FMT, cut_thresholds=(15.0, 2.0))
    with pytest.raises(ValueError, match="tries = 4 is given but no activity bar is set"):
        driver.ClipTrainer(m, opt, (H, W), FMT, tries=4)
    with pytest.raises(ValueError, match="tries must be at least 1"):
        driver.ClipTrainer(m, opt, (H, W), FMT, act_min=1.0, tries=0)
    with pytest.raises(ValueError, match="scene thresholds are"):
        driver.ClipTrainer(m, opt, (H, W), FMT, avoid_cuts=True, cut_thresholds=(-1.0, 2.0))


TODAYS_KEYS = ["config", "input", "frames", "pix_fmt_in", "precision", "weights", "train_steps", "patch", "frames_per_sample", "group", "seed",
               "decimate", "loss_path", "learning_rate", "max_grad_norm", "frames_skipped", "loss", "grad_norm", "checkpoint"]


def test_without_the_options_the_result_line_has_the_keys_it_had(base_model, clip):
    line, _ = driver.run_file_train(clip, 1, scale=S, patch=64, group=8, seed=3, model=copy.deepcopy(base_model))
    assert list(line) == TODAYS_KEYS
    line, _ = driver.run_file_train(clip, 1, scale=S, patch=64, group=8, seed=3, model=copy.deepcopy(base_model), act_min=ACT_MIN)
    assert list(line) == TODAYS_KEYS + ["avoid_cuts", "cut_thresholds", "act_min", "tries", "cuts", "samples_skipped", "act_mean"]
    assert (line["avoid_cuts"], line["cut_thresholds"], line["cuts"], line["tries"]) == (False, None, [], 8) and line["act_mean"] > 0


def test_command_line_prints_the_cuts_and_the_new_keys(clip, capsys):
    argv = ["--input", clip, "--train-steps", "2", "--patch", "64", "--scale", "2", "--group", "8", "--seed", "3"]
    driver.main(argv + ["--avoid-cuts", "--cut-thresholds", "8", "2", "--act-min", "5"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["train_steps"] == 2 and len(line["loss"]) == 2 and all(math.isfinite(v) and v > 0 for v in line["loss"])
    assert (line["avoid_cuts"], line["cut_thresholds"], line["act_min"], line["tries"]) == (True, [8.0, 2.0], 5.0, 8)
    assert line["cuts"] == [CUT] and line["samples_skipped"] == 0 and line["act_mean"] > 0
    new = {"avoid_cuts", "cut_thresholds", "act_min", "tries", "cuts", "samples_skipped", "act_mean"}
    assert new <= set(line) and {"frames_skipped", "loss", "grad_norm", "checkpoint", "seed"} <= set(line) - new
