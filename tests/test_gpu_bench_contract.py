"""bench.py prints ONE JSON line that keeps the driver's contract (metric, value, unit, n_gpus, steps, warmup, ms_per_step,
higher_is_better, scaling, vs_baseline, dtype, data, config.workload) plus the `roofline` object; run at a small size so the
check costs seconds.  A plain run does nothing beyond its steps; the extra loops, the CPU baseline, the accuracy against the oracle
and the other configurations belong to `--full` and keep their own switches there."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FULL_LEGS = ("streaming", "graph_replay", "pcie_inclusive", "cpu_baseline", "accuracy", "psnr_vs_oracle_db", "max_rel_err", "configs")


@pytest.mark.parametrize("extra", [["--full", "--no-cpu-baseline", "--no-extras", "--accuracy"], ["--config", "C3B"], ["--clips", "2"]])
def test_bench_line_contract(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--lr-h", "64", "--lr-w", "96"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "f16"
    assert "workload" in d["config"] and d["value"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.02     # one GPU: frames/s x seconds per forward call = 1
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "whole_frame"):
        assert k in r, k
    assert r["bound"] in ("mfma", "hbm") and 0 < r["frac"] < 1
    # the multi-GPU decomposition fields exist at one rank too (per-rank frames/s, gather waits, the root's resident bytes)
    assert len(d["ranks"]["frames_per_s"]) == 1 and d["ranks"]["frames_per_s"][0] >= d["value"] * 0.99
    assert d["gather"]["rounds"] >= 1 and d["gather"]["root_resident_bytes"] > 0
    if "--full" not in extra:
        assert not [k for k in FULL_LEGS if k in d]
    if "--accuracy" in extra:   # PSNR / max relative error of this build against the oracle, in the line itself
        # (the maximum sits on the few pixels where a DISCRETE guidance plane flipped by a whole step: tests/test_gpu_vsr.py)
        assert d["psnr_vs_oracle_db"] > 58.0 and 0 <= d["max_rel_err"] < 0.5 and d["accuracy"]["p99_rel_err"] < 1e-2, d["accuracy"]
        assert 0 <= d["accuracy"]["sr_stack_max_rel_err_identical_planes"] < 1e-3, d["accuracy"]   # north_star: 1e-3 relative (fp16 storage: ~1e-4)
        assert "oracle" in d["accuracy"]["tile"]


def test_dump_outputs_writes_the_last_timed_frame_and_two_runs_agree(tmp_path):
    """`--dump-outputs DIR`: the HR frame the last timed step returned, as DIR/hr_frame.npy in float32; inputs and weights are seeded, so
    a second run with the same arguments writes the same values (what lets two builds be compared output for output)."""
    import numpy as np
    frames = []
    for run in ("a", "b"):
        out = tmp_path / run
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--lr-h", "64", "--lr-w", "96",
               "--dump-outputs", str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dump_outputs"]["step"] == 3
        assert sorted(os.listdir(out)) == ["hr_frame.npy"] and list(d["dump_outputs"]["arrays"]) == ["hr_frame"]
        a = np.load(out / "hr_frame.npy")
        assert a.dtype == np.float32 and a.shape == (1, 256, 384, 3) and a.nbytes <= 64 << 20
        assert np.isfinite(a).all() and a.std() > 1.0     # a picture (pixel values 0..255-ish), not a cleared buffer
        frames.append(a)
    assert np.array_equal(frames[0], frames[1])


def test_a_plain_run_stops_after_its_steps_and_full_adds_the_other_legs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` sets up, warms up, times the steps and prints the line: no extra loop, no CPU oracle, no
    other configuration.  `--full` runs those legs after the same steps and reports them beside the same headline fields; the frame
    `--dump-outputs` writes is the same in both (it is written before any leg runs the model again)."""
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--lr-h", "64", "--lr-w", "96"]
    lines, frames = {}, {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--accuracy"])):   # (the CPU baseline's timing alone is a minute)
        p = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1
        lines[name], frames[name] = json.loads(out[0]), np.load(tmp_path / name / "hr_frame.npy")
    plain, full = lines["plain"], lines["full"]
    assert not [k for k in FULL_LEGS if k in plain]
    assert "extras_error" not in full, full["extras_error"]
    for k in ("streaming", "graph_replay", "pcie_inclusive", "accuracy", "psnr_vs_oracle_db", "max_rel_err"):
        assert k in full, k
    assert full["graph_replay"]["bit_identical_to_eager"] is True and full["streaming"]["value"] > 0 and full["pcie_inclusive"]["value"] > 0
    assert "configs" not in full     # (the short runs of the other configurations go with the default C3-A geometry only)
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "dtype", "data", "config"):
        assert plain[k] == full[k], k
    assert sorted(set(plain) - {"dump_outputs"}) == sorted(set(full) - set(FULL_LEGS) - {"dump_outputs"})
    assert np.array_equal(frames["plain"], frames["full"])

