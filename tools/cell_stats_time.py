"""Time of the per-cell measure of a resident group (libvsr_hip_cell.so) on eight 2160x3840 frames, beside a device copy of the same bytes
and beside `scene_sums` over the same seven pairs (the way to the cut sums alone before this library), and of the clip trainer with and
without the options that use it.  Device events, rounds interleaved, best of the rounds (and all rounds shown).  The lines go to the
terminal and to profiles/cell_stats_time.txt (--out).

  part 1, one group of eight 2160x3840 float32 RGB frames per call (796 MB: three times the 256 MiB Infinity Cache by itself; the legs
          still rotate over SETS groups): vsr_cell_stats (one launch; bytes = the group read once), a device copy that moves the same
          bytes (half of them read, half written), and vsr_scene_pair_sums over the pairs (g, g + 1), P = 7 in one call (both launches;
          its own bytes are 14 frames: every inner frame is read twice).
  part 2, ClipTrainer on a 2160x3840 yuv420p clip of eight frames (x2, fp32, LR patches of 64, one group, four samples): options off /
          avoid_cuts + act_min, legs interleaved, in train steps per second, host clock around `run` (which ends in the copy of the
          losses).  The thresholds are closed (t_abs = 1e30) and act_min = 0, so both legs train on the same tables, which the tool checks.

    python tools/cell_stats_time.py [--rounds 3] [--skip-trainer] [--out profiles/cell_stats_time.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import numpy as np
import torch

from video_super_resolution_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-trainer", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_stats_time.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
G, H, W, SETS, REPS = 8, 2160, 3840, 2, 40
lines = ["# python tools/cell_stats_time.py " + " ".join(sys.argv[1:]) + "     (one MI355X, one process; device events for part 1, host clock "
         "to the last copy for part 2)"]


def say(text):
    print(text, flush=True)
    lines.append(text)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


# ------------------------------------------------------------------------------------------------ part 1
group_bytes = G * H * W * 12
groups = []
for k in range(SETS):   # smooth frames that drift: a luma that moves by a few codes per pixel and per frame, as footage does
    small = torch.rand(G, 3, H // 8, W // 8, device=dev) * 255
    groups.append(torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear").permute(0, 2, 3, 1).contiguous())
    del small
stats = torch.empty((G,) + driver.cell_shape((H, W)) + (2,), dtype=torch.int32, device=dev)
sums = torch.empty((G - 1, 2), dtype=torch.float64, device=dev)
src = [torch.empty(group_bytes // 2, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(SETS)]
dst = [torch.empty(group_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(SETS)]
legs = {"vsr_cell_stats (one launch, the group read once)": (lambda i: driver.cell_stats(groups[i % SETS], out=stats), group_bytes),
        "device copy moving the group's bytes": (lambda i: dst[i % SETS].copy_(src[i % SETS]), group_bytes),
        "vsr_scene_pair_sums, P = 7 (pixels + finish; 14 frames read)":
            (lambda i: driver.scene_sums(groups[i % SETS][:-1], groups[i % SETS][1:], out=sums), 2 * (G - 1) * H * W * 12)}
times = {k: [] for k in legs}
for rnd in range(args.rounds):
    for name, (fn, _) in legs.items():
        fn(0)
        times[name].append(events(fn, REPS))
say(f"part 1: one group of {G} frames of {H}x{W} per call ({group_bytes / 1e6:.0f} MB), {SETS} groups in rotation, {args.rounds} interleaved "
    f"rounds of {REPS} calls, best round (all rounds)")
for name, (_, nb) in legs.items():
    best = min(times[name])
    say(f"  {name:62s} {best:8.1f} us  {nb / 1e6:7.1f} MB  {nb / best * 1e-6:5.2f} TB/s   rounds us: " + " ".join(f"{t:.1f}" for t in times[name]))
host = stats.cpu().numpy().astype(np.int64)
_, m = driver.cell_cuts(host, (H, W))
_, wm = driver.scene_cuts(sums)
say(f"  (the last group timed: m {m.min():.3f} .. {m.max():.3f}, equal to scene_sums' bit for bit: {np.array_equal(m, wm)}; activity per pixel "
    f"{host[..., 0].sum() / (G * H * W):.3f}; the map is {stats.numel() * 4 / 1e6:.2f} MB)")
del groups, src, dst, legs
torch.cuda.empty_cache()

if not args.skip_trainer:
    # -------------------------------------------------------------------------------------------- part 2
    from video_super_resolution_amd import VSR, optim  # noqa: E402
    from video_super_resolution_amd.weights import fill_module_  # noqa: E402

    S, fmt = 2, "yuv420p"
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = "fp32"
    small = torch.rand(G, 3, H // 8, W // 8, device=dev) * 255
    rgb = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear").permute(0, 2, 3, 1).contiguous()
    clip = np.stack([driver.frames_to_pix(rgb[t], fmt).cpu().numpy() for t in range(G)])
    del small, rgb
    kw = dict(patch=64, group=G, frames_per_sample=3, samples_per_group=4, seed=0)
    optimizer = optim.Adam(model.parameters(), lr=0.0)      # (a step that moves nothing: every run trains the same weights)
    off = driver.ClipTrainer(model, optimizer, (H, W), fmt, **kw)
    on = driver.ClipTrainer(model, optimizer, (H, W), fmt, avoid_cuts=True, cut_thresholds=(1e30, 2.0), act_min=0.0, **kw)

    def timed(tr):
        tr.rng = np.random.RandomState(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = tr.run(clip)
        return steps / (time.perf_counter() - t0)

    runs = {"ClipTrainer, options off       ": off, "ClipTrainer, avoid_cuts + act_min": on}
    for tr in runs.values():   # warm-up: packing, executors, allocator
        timed(tr)
    same = np.array_equal(off.tables[0], on.tables[0])
    rate = {k: [] for k in runs}
    for rnd in range(args.rounds):
        for name, tr in runs.items():
            rate[name].append(timed(tr))
    say(f"part 2: ClipTrainer on {G} frames of {H}x{W} {fmt} (x{S}, fp32, LR patch 64, 4 samples), {args.rounds} interleaved rounds; thresholds "
        f"closed and act_min = 0, tables with and without the options equal: {same}")
    for name, v in rate.items():
        say(f"  {name} best {max(v):6.3f} steps/s   spread of the rounds {max(v) - min(v):.3f}   rounds: " + " ".join(f"{x:.3f}" for x in v))
    b0, b1 = (max(v) for v in rate.values())
    spread = max(4 / min(v) - 4 / max(v) for v in rate.values()) * 1e3
    say(f"  with the options a group of 4 steps takes {(4 / b1 - 4 / b0) * 1e3:+.2f} ms (best against best); the rounds of one leg spread over "
        f"{spread:.2f} ms")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
