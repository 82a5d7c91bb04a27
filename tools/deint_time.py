"""Time of the deinterlacer (libvsr_hip_deint.so) beside a device copy of the same bytes, and of the streamed clip runner with and without
it.  Device events, rounds interleaved, best of the rounds and every round (the spread); the pattern of tools/pix_io_time.py.

  part 1, 1080x1920 and 2160x3840, one frame per call: vsr_deint_frame (keep = 0, kept_first = 1, three distinct frames) for yuv420p, nv12
          and yuv422p10le; beside each a device-to-device copy of exactly the bytes the kernel has to move, 3.5 frame sizes: cur read once,
          out written once, half of prev and of next at the kept rows, half of one of them at the rebuilt rows (the copy reads 1.75 and
          writes 1.75).  Every leg rotates over enough buffer sets to pass 320 MB (beyond the 256 MiB Infinity Cache), so the rate is
          algorithmic bytes over time against HBM.  The yardstick is the kernel's share of its copy's rate, beside the 0.63 .. 0.89 the
          4:2:0 and 4:2:2 converters reach in profiles/pix_io_time.txt.
  part 2, C3-A (540x960 x4, fp16, nv12): ClipRunner (overlap=True) on a 2160x3840 clip decimated by 4, deinterlace=None against
          deinterlace="frame", in frames/s, host clock around work that ends in a wait for the last copy; the difference per frame.

    python tools/deint_time.py [--frames 12] [--rounds 3] [--skip-runner] [--out profiles/deint_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import numpy as np
import torch

from video_super_resolution_amd import _lib as L, driver

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12, help="frames of the clip of part 2 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3, help="rounds of part 2")
ap.add_argument("--skip-runner", action="store_true")
ap.add_argument("--out", default=None, help="also write the table there")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ROUNDS, CALLS, BEYOND = 5, 40, 320e6
YARDSTICK = (0.63, 0.89)   # the converters' share of a copy, profiles/pix_io_time.txt
lines = []
D = L.load_deint()


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


# ------------------------------------------------------------------------------------------------ part 1
say(f"part 1: one frame per call, buffer sets in rotation beyond {BEYOND / 1e6:.0f} MB, {ROUNDS} interleaved rounds of {CALLS} calls, best round (all rounds);")
say("        bytes: 3.5 frame sizes (cur, out, half of prev and next at the kept rows, half of one at the rebuilt rows); copy: a device copy of the same bytes; share: of the copy's rate")
worst = None
for H, W in ((1080, 1920), (2160, 3840)):
    legs = {}
    for fmt in ("yuv420p", "nv12", "yuv422p10le"):
        fb = driver.pix_frame_bytes(fmt, H, W)
        sets = max(4, int(np.ceil(BEYOND / (4 * fb))))
        bufs = [[torch.empty(fb, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(3)] + [torch.empty(fb, dtype=torch.uint8, device=dev)]
                for _ in range(sets)]
        nbytes = int(3.5 * fb)
        src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(sets)]
        dst = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(sets)]

        planes, sb, shift = driver.deint_planes(fmt, H, W)
        arr = (L.DeintPlane * len(planes))(*[L.DeintPlane(*q) for q in planes])
        ptrs = [[L.dptr(t, torch.uint8) for t in row] for row in bufs]   # (the entry itself: the bindings' checks stay out of the timed loop)

        def de(i, ptrs=ptrs, arr=arr, n=len(planes), sb=sb, shift=shift, sets=sets):
            p, c, x, o = ptrs[i % sets]
            L.check(D.vsr_deint_frame(p, c, x, o, arr, n, sb, shift, 0, 1, L.stream()), lib=D)

        def cp(i, src=src, dst=dst, sets=sets):
            dst[i % sets].copy_(src[i % sets])

        legs[f"deint {fmt}"] = (de, nbytes, sets)
        legs[f"copy  {fmt}"] = (cp, nbytes, sets)
    times = {k: [] for k in legs}
    for rnd in range(ROUNDS):
        for name, (fn, _, _) in legs.items():
            fn(0)
            times[name].append(events(fn, CALLS))
    say(f"  {H}x{W}")
    for name, (_, nbytes, sets) in legs.items():
        t = times[name]
        best = min(t)
        share = min(times["copy  " + name[6:]]) / best
        spread = (max(t) - best) / best
        say(f"    {name:18s} {best:7.1f} us  {nbytes / 1e6:6.1f} MB  {nbytes / best * 1e-6:5.2f} TB/s  share {share:4.2f}  spread {spread * 100:4.1f} %  "
            f"({sets} sets)  rounds us: " + " ".join(f"{x:.1f}" for x in t))
        if name.startswith("deint") and (worst is None or share < worst[0]):
            worst = (share, spread, f"{name} {H}x{W}")
    del legs
    torch.cuda.empty_cache()
say(f"  lowest share {worst[0]:.2f} ({worst[2]}, spread {worst[1] * 100:.1f} %) against the converters' {YARDSTICK[0]:.2f} .. {YARDSTICK[1]:.2f}: "
    + ("below the lowest of them by more than its spread" if worst[0] < YARDSTICK[0] * (1 - worst[1]) else "not below the lowest of them by more than its spread"))

# ------------------------------------------------------------------------------------------------ part 2
if not args.skip_runner:
    from video_super_resolution_amd import VSR  # noqa: E402
    from video_super_resolution_amd.weights import fill_module_  # noqa: E402

    H, W, S, T, fmt = 2160, 3840, 4, args.frames, "nv12"
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = "fp16"
    rs = np.random.RandomState(0)
    small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
    clip = np.stack([driver.frames_to_pix(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                          .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
    runs = {}
    for name, mode in (("deinterlace=None", None), ("deinterlace='frame'", "frame")):
        runner = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, deinterlace=mode)
        runs[name] = (lambda runner=runner: runner.run(clip))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (T - 2) / (time.perf_counter() - t0)

    for fn in runs.values():   # warm-up: packing, executors, allocator
        fn()
    fps = {k: [] for k in runs}
    for rnd in range(args.rounds):
        for name, fn in runs.items():
            fps[name].append(timed(fn))
    say(f"part 2: C3-A (540x960 x4 -> {H}x{W}, fp16, {fmt} in and out), ClipRunner overlap=True, {T - 2} windows per run, {args.rounds} interleaved rounds")
    for name, v in fps.items():
        say(f"  {name:20s} best {max(v):6.2f} frames/s  = {1e3 / max(v):7.2f} ms per frame   rounds: " + " ".join(f"{x:.2f}" for x in v))
    a, b = max(fps["deinterlace=None"]), max(fps["deinterlace='frame'"])
    say(f"  difference per frame (best rounds): {1e3 / b - 1e3 / a:+.2f} ms")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# python tools/deint_time.py --frames {args.frames} --rounds {args.rounds}" + (" --skip-runner" if args.skip_runner else "") +
                "     (one MI355X, one process; device events for part 1, host clock to the last copy for part 2)\n")
        f.write("\n".join(lines) + "\n")
