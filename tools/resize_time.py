"""Time of the table-driven resampler (libvsr_hip_resize.so) at the headline frame sizes, reported and not gated: beside a plain copy of
the bytes each case must move and beside torch's own antialiased `interpolate` on the device, and of the streamed clip runner with
decimate="nearest" against "bicubic".  Device events, rounds interleaved over the legs, best round (and all rounds shown).

  part 1, vsr_resize_frames with the bicubic tables of driver.resize_tables, quantise = 1 down and 0 up:
            2160x3840 -> 540x960 (F = 1 and 3), 1440x2560 -> 720x1280, 540x960 -> 2160x3840, 720x1280 -> 2160x3840.
          Every leg rotates over SETS source / destination sets (3 x 99.5 MB of source at 2160x3840: beyond the 256 MiB Infinity Cache).
          Bytes = the source read once + the result written once.  "copy": `copy_` of a float32 buffer of half those bytes (it reads and
          writes each of its bytes once, so it moves the same total), the yardstick of tools/loss_time.py.  "torch": F.interpolate(mode=
          "bicubic", antialias=True) on the same frames as NCHW views (its layout), float result, without the quantise step.
  part 2, C3-A (540x960 x4, fp16): ClipRunner on a 2160x3840 nv12 clip with decimate="nearest" and decimate="bicubic" (both scored on
          luma, the second also with the bicubic baseline), legs interleaved, frames/s by the host clock around runs that end in a wait.

    python tools/resize_time.py [--frames 12] [--rounds 3] [--skip-runner]
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
import torch.nn.functional as F

from video_super_resolution_amd import driver

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12, help="frames of the clip of part 2 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-runner", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
SETS, REPS = 3, 9
CASES = [(1, 2160, 3840, 540, 960), (3, 2160, 3840, 540, 960), (1, 1440, 2560, 720, 1280), (1, 540, 960, 2160, 3840), (1, 720, 1280, 2160, 3840)]


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


print(f"# python tools/resize_time.py --frames {args.frames} --rounds {args.rounds}     (one MI355X, one process)")
print(f"part 1: bicubic (antialiased), {SETS} buffer sets in rotation, {args.rounds} interleaved rounds of {REPS} calls, best round (all rounds); "
      "MB = source read once + result written once")
for Fn, H, W, h, w in CASES:
    down = h < H
    src = [torch.rand(Fn, H, W, 3, device=dev) * 255.0 for _ in range(SETS)]
    dst = [torch.empty(Fn, h, w, 3, device=dev) for _ in range(SETS)]
    nbytes = 12 * Fn * (H * W + h * w)
    ca = [torch.empty(nbytes // 8, dtype=torch.float32, device=dev) for _ in range(SETS)]
    cb = [torch.empty(nbytes // 8, dtype=torch.float32, device=dev) for _ in range(SETS)]
    r = driver.FrameResizer((H, W), (h, w), "bicubic", dev)
    nchw = [s.permute(0, 3, 1, 2) for s in src]   # (views: torch's channels-last layout of the same memory)
    legs = {
        "vsr_resize_frames": lambda i: r(src[i % SETS], quantise=down, out=dst[i % SETS]),
        "copy of the same bytes": lambda i: cb[i % SETS].copy_(ca[i % SETS]),
        "torch interpolate(antialias)": lambda i: F.interpolate(nchw[i % SETS], size=(h, w), mode="bicubic", antialias=True, align_corners=False),
    }
    times = {k: [] for k in legs}
    TORCH = "torch interpolate(antialias)"
    refused = None
    for k in list(legs):
        try:
            legs[k](0)
        except RuntimeError as e:   # (torch's antialiased kernel refuses some supports: shown, not hidden)
            if k != TORCH:
                raise
            refused = str(e).splitlines()[0]
            del legs[k], times[k]
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(events(fn, REPS))
    agree = f"torch refused: {refused}"
    if refused is None:
        got = r(src[0], quantise=False)
        ref = F.interpolate(nchw[0], size=(h, w), mode="bicubic", antialias=True, align_corners=False).permute(0, 2, 3, 1)
        agree = f"max |ours - torch| on 0..255: {float((got - ref).abs().max()):.2e}"
        del got, ref
    print(f"  F = {Fn}, {H}x{W} -> {h}x{w}, {r.x_weight.shape[1]} x {r.y_weight.shape[1]} taps, {nbytes / 1e6:.1f} MB   ({agree})")
    for k in legs:
        best = min(times[k])
        print(f"    {k:30s} {best:9.1f} us  {nbytes / best * 1e-6:5.2f} TB/s   rounds us: " + " ".join(f"{t:.1f}" for t in times[k]))
    print(f"    -> {min(times['vsr_resize_frames']) / min(times['copy of the same bytes']):.2f} x the time of the copy"
          + (f", torch takes {min(times[TORCH]) / min(times['vsr_resize_frames']):.2f} x ours" if refused is None else ""))
    del src, dst, ca, cb, nchw, legs
    torch.cuda.empty_cache()
if args.skip_runner:
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ part 2
from video_super_resolution_amd import VSR  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

S, T, H, W = 4, args.frames, 2160, 3840
model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
model.precision = model.model.precision = "fp16"
fmt = "nv12"
rs = np.random.RandomState(0)
small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
clip = np.stack([driver.frames_to_yuv(F.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                      .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
runners = {
    'decimate="nearest", score="y"': driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y"),
    'decimate="bicubic", score="y"': driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", decimate="bicubic"),
    'decimate="bicubic" + baseline': driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, score="y", decimate="bicubic", baseline="bicubic"),
}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (T - 2) / (time.perf_counter() - t0)


for r in runners.values():   # warm-up: packing, executors, allocator
    r.run(clip)
fps = {k: [] for k in runners}
for _ in range(args.rounds):
    for k, r in runners.items():
        fps[k].append(timed(lambda: r.run(clip)))
print(f"part 2: C3-A (540x960 x4 -> {H}x{W}, fp16, {fmt} in / out), {T - 2} windows per run, {args.rounds} interleaved rounds")
for k, v in fps.items():
    print(f"  ClipRunner {k} best {max(v):6.2f} frames/s   spread of the rounds {max(v) - min(v):.2f}   rounds: " + " ".join(f"{x:.2f}" for x in v))
b = {k: max(v) for k, v in fps.items()}
k0, k1, k2 = list(b)
print(f"  bicubic LR frames cost {1e3 / b[k1] - 1e3 / b[k0]:+.3f} ms per frame, the baseline {1e3 / b[k2] - 1e3 / b[k1]:+.3f} ms more (best against best)")
m = runners[k2].metrics
print(f"  (synthetic weights restore nothing; the numbers only show the path: PSNR {m['psnr'].mean():.3f} dB, bicubic baseline "
      f"{m['psnr_baseline'].mean():.3f} dB, SSIM {m['ssim'].mean():.4f} against {m['ssim_baseline'].mean():.4f})")
