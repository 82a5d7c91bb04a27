"""`clip_runner.sums_layout` without a GPU: the rows of the one tensor of sums a scored `ClipRunner.run` fills, per series."""
import itertools

from video_super_resolution_amd import clip_runner, driver

ORDER = ("estimate", "baseline", "ewarp", "ewarp_truth", "ewarp_baseline")   # the documented order of the rows
KIND = {"estimate": "frame", "baseline": "frame", "ewarp": "pair", "ewarp_truth": "pair", "ewarp_baseline": "pair"}


def test_sums_layout_tiles_the_rows_in_the_documented_order():
    assert driver.sums_layout is clip_runner.sums_layout
    for T, baseline, temporal in itertools.product((3, 4, 6), (None, "bicubic"), (None, "warp")):
        want = [n for n in ORDER if (baseline is not None or "baseline" not in n) and (temporal is not None or not n.startswith("ewarp"))]
        for score in ("rgb", "y"):
            layout = clip_runner.sums_layout(T, score, baseline, temporal)
            assert list(layout) == want                                    # absent series are absent, the present ones in order
            at = 0
            for name, (row0, rows, kind) in layout.items():
                assert kind == KIND[name] and rows == (T - 2 if kind == "frame" else T - 3) and rows >= 0
                assert row0 == at                                          # disjoint, no gap: the ranges cover [0, rows) exactly
                at += rows
            assert at == (T - 2) * (1 + (baseline is not None)) + (T - 3) * (0 if temporal is None else 2 + (baseline is not None))
            assert set(layout) <= set(clip_runner.METRIC_KEYS)             # every series has its keys in `metrics`
        assert clip_runner.sums_layout(T, None, baseline, temporal) is None   # nothing scored: no layout
