"""Time of scene-cut detection (libvsr_hip_scene.so) at the LR frame sizes of the headline configurations, beside a device copy of the
same bytes and beside what the window launch replaces, and of the streamed clip runner with and without it.  Device events, rounds
interleaved, best of the rounds (and all rounds shown).  The lines go to the terminal and to profiles/scene_time.txt (--out).

  part 1, 540x960 and 1080x1920, one pair per call: vsr_scene_pair_sums (both launches) and vsr_scene_decide (one pair, with the pair
          before).  Every leg rotates over SETS pairs of frames (beyond the 256 MiB Infinity Cache), so the rate is algorithmic bytes (both
          frames read once: 24 B per pixel) over time against HBM.  Beside it a device copy that moves the same bytes (half of them read,
          half written).
  part 2, the same sizes, x4: vsr_scene_window (three LR frames and the previous estimate in, the window and the LR estimate out) beside
          torch.stack of the three frames plus vsr_resize_estimate_f32 of the estimate, what the default runner and VSR.forward launch
          for the same result.
  part 3, C3-A (540x960 x4, fp16): ClipRunner on a 2160x3840 nv12 clip (decimated by 4) with scene=None / "sad", legs interleaved, in
          frames/s, host clock around work that ends in a wait for the last copy.  The thresholds are closed (t_abs = 1e30): the bytes are
          those of scene=None, which the tool checks.

    python tools/scene_time.py [--frames 12] [--rounds 3] [--skip-runner] [--out profiles/scene_time.txt]
"""
import argparse
import ctypes
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

from video_super_resolution_amd import _lib as L, driver, frames

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12, help="frames of the clip of part 3 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-runner", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_time.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
S, REPS = 4, 24
lines = ["# python tools/scene_time.py " + " ".join(sys.argv[1:]) + "     (one MI355X, one process; device events for parts 1 and 2, host clock "
         "to the last copy for part 3)"]


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


def rounds_of(legs, rounds):
    times = {k: [] for k in legs}
    for rnd in range(rounds):
        for name, (fn, _) in legs.items():
            fn(0)
            times[name].append(events(fn, REPS))
    return times


def report(legs, times):
    for name, (_, nb) in legs.items():
        best = min(times[name])
        say(f"  {name:58s} {best:8.1f} us  {nb / 1e6:6.1f} MB  {nb / best * 1e-6:5.2f} TB/s   rounds us: " + " ".join(f"{t:.1f}" for t in times[name]))


M = L.load_scene()
luma4 = frames._luma4("y", "bt601", False)
pl = luma4.ctypes.data_as(ctypes.c_void_p)
for h, w in ((540, 960), (1080, 1920)):
    # ---------------------------------------------------------------------------------------------- part 1
    frame_bytes = h * w * 12
    SETS = max(3, -(-3 * (256 << 20) // (2 * frame_bytes)))       # pairs in rotation: three times the Infinity Cache
    fa = [torch.rand(h, w, 3, device=dev) * 300 - 20 for _ in range(SETS)]
    fb = [(fa[k] + torch.randn(h, w, 3, device=dev) * 9).contiguous() for k in range(SETS)]
    sums = torch.empty(2, 2, dtype=torch.float64, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(M.vsr_scene_ws_bytes(1, h, w)), dtype=torch.uint8, device=dev)

    def leg_sums(i):
        k = i % SETS
        L.check(M.vsr_scene_pair_sums(L.dptr(fa[k]), L.dptr(fb[k]), 1, h, w, pl, L.dptr(sums[1:2], torch.float64), L.dptr(ws, torch.uint8),
                                      L.stream()), "scene_pair_sums", lib=M)

    def leg_decide(i):
        L.check(M.vsr_scene_decide(L.dptr(sums[1:2], torch.float64), 1, L.dptr(sums[0], torch.float64), 15.0, 2.0, L.dptr(flags[1:2], torch.int32),
                                   L.stream()), "scene_decide", lib=M)

    nbytes = 2 * frame_bytes
    src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(SETS)]
    dst = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(SETS)]
    driver.scene_sums(fa[0], fb[0], out=sums[0:1])
    legs = {"vsr_scene_pair_sums (pixels + finish)": (leg_sums, nbytes), "vsr_scene_decide (one pair, with the pair before)": (leg_decide, 36),
            "device copy moving the frames' bytes": (lambda i: dst[i % SETS].copy_(src[i % SETS]), nbytes)}
    times = rounds_of(legs, args.rounds)
    say(f"part 1: one {h}x{w} pair per call, {SETS} pairs in rotation, {args.rounds} interleaved rounds of {REPS} calls, best round (all rounds)")
    report(legs, times)
    cuts, m = driver.scene_cuts(sums)
    say(f"  (m of set 0 and of the last set timed: {m[0]:.4f}, {m[1]:.4f}; flag of the last decide: {int(flags[1])})")
    del src, dst, legs

    # ---------------------------------------------------------------------------------------------- part 2
    H, W = S * h, S * w
    NEST = max(3, -(-3 * (256 << 20) // (H * W * 12)))
    est = [torch.rand(1, H, W, 3, device=dev) * 255 for _ in range(NEST)]
    one = torch.ones(1, dtype=torch.int32, device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    x3 = torch.empty(3, h, w, 3, device=dev)
    e_hwc = torch.empty(1, h, w, 3, device=dev)
    e_chw = torch.empty(3, h, w, device=dev)

    def leg_window(i, f_ab=zero, f_bc=zero):
        k = i % (SETS - 2)
        L.check(M.vsr_scene_window(L.dptr(fa[k]), L.dptr(fa[k + 1]), L.dptr(fa[k + 2]), L.dptr(est[i % NEST]), H, W, L.dptr(f_ab, torch.int32),
                                   L.dptr(f_bc, torch.int32), L.dptr(x3), L.dptr(e_hwc), h, w, L.stream()), "scene_window", lib=M)

    def leg_stack(i):
        k = i % (SETS - 2)
        torch.stack([fa[k], fa[k + 1], fa[k + 2]], out=x3)
        L.check(L.load().vsr_resize_estimate_f32(L.dptr(est[i % NEST]), H, W, L.dptr(e_chw), L.dptr(e_hwc), h, w, L.stream()), "resize_estimate")

    moved = 7 * frame_bytes + frame_bytes      # three frames and the estimate's LR pixels in (sectors of it: counted as one LR frame), four out
    legs = {"vsr_scene_window, no flag set": (leg_window, moved),
            "vsr_scene_window, both flags set (a and c not read)": (lambda i: leg_window(i, one, one), moved - 3 * frame_bytes),
            "torch.stack + vsr_resize_estimate_f32 (two launches)": (leg_stack, moved + frame_bytes)}
    times = rounds_of(legs, args.rounds)
    say(f"part 2: the window of three {h}x{w} frames and the x{S} estimate of {H}x{W} at its LR pixels, {NEST} estimates in rotation, "
        f"{args.rounds} interleaved rounds of {REPS} calls, best round (all rounds)")
    report(legs, times)
    del fa, fb, est, legs
    torch.cuda.empty_cache()

if not args.skip_runner:
    # ------------------------------------------------------------------------------------------------ part 3
    from video_super_resolution_amd import VSR  # noqa: E402
    from video_super_resolution_amd.weights import fill_module_  # noqa: E402

    H, W, T, fmt = 2160, 3840, args.frames, "nv12"
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = "fp16"
    fbytes = driver.yuv_frame_bytes(fmt, H, W)
    rs = np.random.RandomState(0)
    small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
    clip = np.stack([driver.frames_to_yuv(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                          .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
    off = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True)
    on = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, scene="sad", scene_thresholds=(1e30, 2.0))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (T - 2) / (time.perf_counter() - t0)

    runs = {'ClipRunner scene=None ': lambda: off.run(clip), 'ClipRunner scene="sad"': lambda: on.run(clip)}
    for fn in runs.values():   # warm-up: packing, executors, allocator
        fn()
    same = np.array_equal(off.run(clip), on.run(clip))
    fps = {k: [] for k in runs}
    for rnd in range(args.rounds):
        for name, fn in runs.items():
            fps[name].append(timed(fn))
    say(f"part 3: C3-A (540x960 x4 -> {H}x{W}, fp16, {fmt} in / out, {fbytes / 1e6:.1f} MB per frame each way), {T - 2} windows per run, "
        f"{args.rounds} interleaved rounds; thresholds closed, bytes with and without scene equal: {same}")
    for name, v in fps.items():
        say(f"  {name} best {max(v):6.2f} frames/s   spread of the rounds {max(v) - min(v):.2f}   rounds: " + " ".join(f"{x:.2f}" for x in v))
    b0, b1 = (max(v) for v in fps.values())
    say(f"  scene detection costs {1e3 / b1 - 1e3 / b0:+.3f} ms per frame (best against best)")
    say(f"  (independent random frames: scene_m {on.scene_m.min():.2f} .. {on.scene_m.max():.2f}, cuts under the closed thresholds: {int(on.cuts.sum())})")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
