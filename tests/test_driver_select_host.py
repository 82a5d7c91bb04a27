"""Host-side checks of the steps on the map of `cell_stats` (no GPU): `patch_table_select` draws what `patch_table` draws and leaves the
generator where it leaves it, keeps every row off a set pair, and picks by `patch_score` as its docstring says; `patch_score` equals a
per-pixel sum; `cell_cuts` is `scene_cuts` on the map's sums; one table is pinned; the command line refuses the new switches where they
make no sense.  The map comes from the numpy restatement (tests/_cell_ref.py)."""
import numpy as np
import pytest

import _cell_ref as R
from video_super_resolution_amd import driver


def _state_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# (G, n, (H, W), patch, S, transpose)
SHAPES = [(8, 3, (160, 192), 128, 2, None), (5, 3, (96, 120), (64, 112), 2, None), (4, 4, (130, 131), 64, 4, None),
          (6, 5, (128, 160), (64, 96), 2, True)]


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("G, n, shape, patch, S, transpose", SHAPES)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_no_cut_and_no_bar_is_patch_table_and_leaves_the_generator_where_it_does(seed, G, n, shape, patch, S, transpose, augment):
    a, b, c = (np.random.RandomState(seed) for _ in range(3))
    want = driver.patch_table(a, 5, G, n, shape, patch, S, augment, transpose)
    table, scores, tried = driver.patch_table_select(b, 5, G, n, shape, patch, S, augment, transpose)
    assert table.dtype == np.int32 and np.array_equal(table, want) and _state_equal(a, b)
    assert scores.dtype == np.float64 and np.isnan(scores).all() and tried.dtype == np.int32 and (tried == 1).all()
    # a cut array with no pair set changes nothing either
    table, _, _ = driver.patch_table_select(c, 5, G, n, shape, patch, S, augment, transpose, cuts=np.zeros(G - 1, dtype=bool))
    assert np.array_equal(table, want) and _state_equal(a, c)


def test_rows_never_straddle_a_set_pair():
    G, n, shape = 8, 3, (160, 192)
    for seed, pairs in ((0, [3]), (1, [0]), (2, [6]), (3, [2, 5]), (4, [1, 4])):
        cuts = np.zeros(G - 1, dtype=bool)
        cuts[pairs] = True
        table, _, _ = driver.patch_table_select(np.random.RandomState(seed), 64, G, n, shape, 128, 2, cuts=cuts)
        assert table.shape == (64, 4) and not any(R.straddles(row, n, cuts) for row in table)
        valid = [t0 for t0 in range(G - n + 1) if not cuts[t0:t0 + n - 1].any()]
        assert sorted(set(table[:, 0].tolist())) == valid, (pairs, valid)      # and every valid t0 is reached in 64 draws
        want, _, _, _ = R.select(np.random.RandomState(seed), 64, G, n, shape, 128, 2, cuts=cuts)
        assert np.array_equal(table, want)


def test_no_valid_t0_gives_an_empty_table_and_draws_nothing():
    rng, untouched = np.random.RandomState(5), np.random.RandomState(5)
    cuts = np.array([0, 1, 0, 1, 0, 1, 0], dtype=bool)    # every run of three frames holds a cut
    table, scores, tried = driver.patch_table_select(rng, 4, 8, 3, (160, 192), 128, 2, cuts=cuts)
    assert table.shape == (0, 4) and table.dtype == np.int32 and scores.shape == (0,) and tried.shape == (0,) and tried.dtype == np.int32
    assert _state_equal(rng, untouched)
    with pytest.raises(ValueError, match="cuts must hold the G - 1 = 7 pairs"):
        driver.patch_table_select(rng, 4, 8, 3, (160, 192), 128, 2, cuts=cuts[:6])


@pytest.fixture(scope="module")
def ragged():
    """Frames of 75 x 100 (the last cells hold 11 rows and 4 columns) and their map."""
    f = R.make_frames("bytes", 4, 75, 100, seed=1)
    return f, R.cell_stats(f)


@pytest.mark.parametrize("name, row, patch", [
    ("cell-aligned", (0, 16, 32, 0), (32, 48)),
    ("y0 % 16 = 4", (1, 4, 16, 3), (44, 32)),
    ("both origins odd", (0, 7, 9, 9), (40, 50)),
    ("touching the last ragged cell", (1, 27, 36, 0), (48, 64)),      # the crop ends at (75, 100): the ragged cells are not counted
    ("transposed crop of a non-square patch", (0, 8, 20, 4), (64, 36)),   # the crop is 36 rows x 64 columns
])
def test_patch_score_equals_the_per_pixel_sum(ragged, name, row, patch):
    f, stats = ragged
    n = 3 if row[0] == 0 else 2
    got = driver.patch_score(stats, row, n, patch)
    assert isinstance(got, float) and got == R.patch_score(stats, row, n, patch) == R.patch_score_pixels(f, row, n, patch), name
    assert got > 0


def test_patch_score_counts_whole_cells_only_and_refuses_a_crop_without_one(ragged):
    _, stats = ragged
    # rows 27..74 hold the cells i = 2, 3 (32..63); the ragged cell i = 4 (64..74) is left out although the crop covers what exists of it
    a = driver.patch_score(stats, (0, 27, 36, 0), 2, (48, 64))
    s = stats.astype(np.int64)
    assert a == float(np.float64(int(s[0:2, 2:4, 3:6, 0].sum())) / np.float64(2 * 2 * 3 * 256))
    with pytest.raises(ValueError, match="holds no whole cell"):
        driver.patch_score(stats, (0, 1, 0, 0), 2, (30, 64))      # rows 1..30: no cell row inside
    assert driver.patch_score(stats, (0, 1, 0, 0), 2, (31, 64)) > 0   # 31 always has one
    with pytest.raises(ValueError, match="leaves the map"):
        driver.patch_score(stats, (3, 0, 0, 0), 2, (32, 32))


@pytest.fixture(scope="module")
def banded():
    """Four 160 x 320 frames of random bytes whose left 128 columns are constant, and their map."""
    f = R.make_frames("bytes", 4, 160, 320, seed=0)
    f[:, :, :128] = 50.0
    return R.cell_stats(f)


@pytest.mark.parametrize("act_min, tries", [(80.0, 8), (97.5, 3), (1000.0, 4), (0.0, 1)])
def test_the_selection_rule(banded, act_min, tries):
    kw = dict(stats=banded, act_min=act_min, tries=tries)
    table, scores, tried = driver.patch_table_select(np.random.RandomState(7), 24, 4, 3, (160, 320), 64, 2, **kw)
    want, wscores, wtried, candidates = R.select(np.random.RandomState(7), 24, 4, 3, (160, 320), 64, 2, **kw)
    assert np.array_equal(table, want) and np.array_equal(scores, wscores) and np.array_equal(tried, wtried)
    accepted = fallback = 0
    for b in range(24):
        drawn = candidates[b]
        assert len(drawn) == tried[b] <= tries and scores[b] == driver.patch_score(banded, table[b], 3, 64)
        if scores[b] >= act_min:      # accepted: the first that qualifies
            assert tuple(table[b]) == drawn[-1][0] and all(sc < act_min for _, sc in drawn[:-1])
            accepted += 1
        else:                          # fallback: all were drawn, the largest score, the first among equals
            best = max(sc for _, sc in drawn)
            assert tried[b] == tries and scores[b] == best
            assert tuple(table[b]) == next(row for row, sc in drawn if sc == best)
            fallback += 1
    if act_min == 1000.0:
        assert fallback == 24
    elif act_min == 97.5:
        assert accepted > 0 and fallback > 0
    else:
        assert fallback == 0 and (act_min == 0.0 or (tried > 1).any())


def test_first_among_equals_on_a_flat_map():
    """Every candidate scores 0: the fallback row is the first one drawn, which is `patch_table`'s first row; the generator has moved on by
    `tries` candidates per row."""
    stats = np.zeros((4, 10, 20, 2), dtype=np.int32)
    rng, plain = np.random.RandomState(2), np.random.RandomState(2)
    table, scores, tried = driver.patch_table_select(rng, 3, 4, 3, (160, 320), 64, 2, stats=stats, act_min=1.0, tries=5)
    every = driver.patch_table(plain, 15, 4, 3, (160, 320), 64, 2)
    assert np.array_equal(table, every[::5]) and (scores == 0).all() and (tried == 5).all() and _state_equal(rng, plain)


def test_one_pinned_table(banded):
    """Seed 0, a 64 x 96 patch that may be transposed, act_min = 80 (chosen on the restatement: a patch with 18 % of its whole cells in
    the constant band still passes, one that lies in the band does not): row 1 was the second candidate, no row is a fallback."""
    kw = dict(transpose=True, stats=banded, act_min=80.0, tries=8)
    table, scores, tried = driver.patch_table_select(np.random.RandomState(0), 4, 4, 3, (160, 320), (64, 96), 2, **kw)
    assert table.tolist() == [[1, 0, 134, 12], [1, 72, 174, 3], [0, 48, 116, 6], [0, 78, 174, 1]]
    assert tried.tolist() == [1, 2, 1, 1] and (scores >= 80.0).all()
    want, wscores, _, candidates = R.select(np.random.RandomState(0), 4, 4, 3, (160, 320), (64, 96), 2, **kw)
    assert np.array_equal(table, want) and np.array_equal(scores, wscores)
    assert candidates[1][0] == ((1, 78, 18, 11), 0.0)       # the candidate that lay in the band


def test_select_refuses_what_it_cannot_use(banded):
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError, match="act_min needs stats"):
        driver.patch_table_select(rng, 1, 4, 3, (160, 320), 64, 2, act_min=1.0)
    with pytest.raises(ValueError, match="tries must be at least 1"):
        driver.patch_table_select(rng, 1, 4, 3, (160, 320), 64, 2, stats=banded, act_min=1.0, tries=0)
    with pytest.raises(ValueError, match="is not that of 5 frames of 160 x 320"):
        driver.patch_table_select(rng, 1, 5, 3, (160, 320), 64, 2, stats=banded, act_min=1.0)
    with pytest.raises(ValueError, match="does not fit the frames"):
        driver.patch_table_select(rng, 1, 4, 3, (160, 320), 192, 2)


def test_cell_cuts_is_scene_cuts_on_the_maps_sums():
    f = np.concatenate([R.make_frames("constant", 3, 40, 50), R.make_frames("bytes", 2, 40, 50, seed=3), R.make_frames("constant", 2, 40, 50)])
    stats = R.cell_stats(f)
    cuts, m = driver.cell_cuts(stats, (40, 50))
    sums = np.stack([stats[1:, :, :, 1].astype(np.int64).sum(axis=(1, 2)).astype(np.float64), np.full(6, 2000.0)], axis=1)
    wcuts, wm = driver.scene_cuts(sums)
    assert cuts.dtype == bool and m.dtype == np.float64 and np.array_equal(cuts, wcuts) and np.array_equal(m, wm)
    rcuts, rm = R.cell_cuts(stats, (40, 50))
    assert np.array_equal(cuts, rcuts) and np.array_equal(m.view(np.uint64), rm.view(np.uint64))
    # constant | two frames of noise | constant: the pair into the noise is a cut; the next two pairs are as large but not twice the pair
    # before them (the rule's second limit, include/vsr_hip_scene.h: the second of two cuts one frame apart is missed)
    assert cuts.tolist() == [False, False, True, False, False, False] and m[0] == 0 and (m[2:5] > 15).all() and m[5] == 0
    # thresholds reach the rule; the first pair of a group has no pair before it
    assert driver.cell_cuts(stats, (40, 50), (0.0, 0.0))[0].all() and not driver.cell_cuts(stats, (40, 50), (1e9, 2.0))[0].any()
    assert driver.cell_cuts(stats[3:], (40, 50))[0].tolist() == [True, False, False]      # (3, 4) opens the group: judged on t_abs alone
    assert "m_{-1} = 0 AT THE START OF EVERY GROUP" in driver.cell_cuts.__doc__
    one = driver.cell_cuts(stats[:1], (40, 50))
    assert one[0].shape == (0,) and one[1].shape == (0,)
    with pytest.raises(ValueError, match="is not that of frames of 64 x 50"):
        driver.cell_cuts(stats, (64, 50))


def test_driver_re_exports_the_names():
    from video_super_resolution_amd import frames
    for name in ("CELL", "cell_shape", "cell_stats", "cell_cuts", "patch_score", "patch_table_select"):
        assert getattr(driver, name) is getattr(frames, name), name


def test_cell_stats_refuses_host_tensors_and_other_shapes():
    import torch
    with pytest.raises(Exception, match="CPU tensor"):
        driver.cell_stats(torch.zeros(2, 16, 16, 3))
    with pytest.raises(ValueError, match=r"float32 \[G,H,W,3\]"):
        driver.cell_stats(torch.zeros(16, 16, 3))


@pytest.mark.parametrize("argv, words", [
    (["--avoid-cuts"], "--avoid-cuts needs --input and --train-steps"),
    (["--train-steps", "2", "--act-min", "4"], "--act-min needs --input and --train-steps"),
    (["--input", "a.y4m", "--tries", "3"], "--tries needs --input and --train-steps"),
    (["--input", "a.y4m", "--cut-thresholds", "15", "2"], "--cut-thresholds needs --input and --train-steps"),
    (["--input", "a.y4m", "--train-steps", "2", "--cut-thresholds", "15", "2"], "--cut-thresholds needs --avoid-cuts"),
    (["--input", "a.y4m", "--train-steps", "2", "--tries", "3"], "--tries needs --act-min"),
    (["--input", "a.y4m", "--train-steps", "2", "--act-min", "4", "--tries", "0"], "--tries is at least 1"),
    (["--input", "a.y4m", "--train-steps", "2", "--avoid-cuts", "--scene", "sad"], "it takes no --scene"),
])
def test_cli_refuses_selection_switches_that_make_no_sense(argv, words, capsys):
    with pytest.raises(SystemExit):
        driver.main(argv)
    assert words in capsys.readouterr().err
