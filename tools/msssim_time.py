"""Time of multi-scale SSIM (libvsr_hip_msssim.so) at the headline frame size beside the single-scale launch it restates, and of the
streamed clip runner with and without `multiscale`.  Device events, rounds interleaved, best of the rounds (and all rounds shown).

  part 1, 2160x3840, one frame per call (F = 1, quantise = 1, shave = 4): vsr_msssim_frames for RGB and Y beside vsr_metric_frames
          SSE + SSIM on the same box in the same run.  Every leg rotates over SETS pairs of frames (3 x 199 MB: beyond the 256 MiB
          Infinity Cache).  The ratio to the single-scale launch is shown beside what the work accounts for: the pyramid holds
          sum_j n_j / n_1 (about 4/3) of level 1's map positions, and one pass more reads both frames (24 B per pixel) and writes a third
          of their pixels as doubles per plane.
  part 2, C3-A (540x960 x4, fp16): ClipRunner on a 2160x3840 nv12 clip (decimated by 4) with score="y" and with multiscale=True on
          top, legs interleaved, in frames/s, host clock around work that ends in a wait for the last copy.

    python tools/msssim_time.py [--frames 22] [--rounds 3] [--skip-runner] [--unaligned]

--unaligned: part 1 on frames at a storage offset of one float (bases 4 bytes past a 16-byte boundary): the element-load path.
"""
import argparse
import ctypes
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
ap.add_argument("--frames", type=int, default=22, help="frames of the clip of part 2 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-runner", action="store_true")
ap.add_argument("--unaligned", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
H, W, SETS, SHAVE, REPS = 2160, 3840, 3, 4, 12


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def placed(x):
    if not args.unaligned:
        return x.contiguous()
    buf = torch.zeros(x.numel() + 8, dtype=torch.float32, device=dev)
    buf[1:1 + x.numel()] = x.reshape(-1)
    view = buf[1:1 + x.numel()].view(x.shape)
    assert view.data_ptr() % 16 == 4
    return view


# ------------------------------------------------------------------------------------------------ part 1
M, MS = L.load_metric(), L.load_msssim()
fa = [placed(torch.rand(H, W, 3, device=dev) * 300 - 20) for _ in range(SETS)]
fb = [placed(fa[k] + torch.randn(H, W, 3, device=dev) * 4) for k in range(SETS)]
sums = torch.empty(1, 4, dtype=torch.float64, device=dev)
win = driver.ssim_window()
c = driver.yuv_coefficients("yuv420p", "bt601", False)
luma4 = np.ascontiguousarray(np.array([c[0], c[1], c[2], c[9]], dtype=np.float32))
pw, pl = win.ctypes.data_as(ctypes.c_void_p), luma4.ctypes.data_as(ctypes.c_void_p)
legs = {}
for ch_name, ch in (("RGB", 0), ("Y", 1)):
    ws1 = torch.empty(int(M.vsr_metric_ws_bytes(1, H, W, SHAVE, 3)), dtype=torch.uint8, device=dev)
    ws5 = torch.empty(int(MS.vsr_msssim_ws_bytes(1, H, W, SHAVE, ch)), dtype=torch.uint8, device=dev)
    sums5 = torch.empty(1, 3 if ch == 0 else 1, 5, 2, dtype=torch.float64, device=dev)

    def single(i, ch=ch, ws=ws1):
        k = i % SETS
        L.check(M.vsr_metric_frames(L.dptr(fa[k]), L.dptr(fb[k]), 1, H, W, 3, ch, 1, SHAVE, pl, pw, L.dptr(sums, torch.float64),
                                    L.dptr(ws, torch.uint8), L.stream()), lib=M)

    def multi(i, ch=ch, ws=ws5, out=sums5):
        k = i % SETS
        L.check(MS.vsr_msssim_frames(L.dptr(fa[k]), L.dptr(fb[k]), 1, H, W, ch, 1, SHAVE, pl, pw, L.dptr(out, torch.float64),
                                     L.dptr(ws, torch.uint8), L.stream()), lib=MS)

    legs[f"vsr_metric_frames {ch_name:3s} SSE + SSIM"] = single
    legs[f"vsr_msssim_frames {ch_name:3s}"] = multi

times = {k: [] for k in legs}
for rnd in range(5):
    for name, fn in legs.items():
        fn(0)
        times[name].append(events(fn, REPS))
levels = driver.msssim_levels(H - 2 * SHAVE, W - 2 * SHAVE)
n = [(h - 10) * (w - 10) for h, w in levels]
pooled = sum(h * w for h, w in levels[1:])
print(f"part 1: one {H}x{W} frame per call (quantise 1, shave {SHAVE}{', unaligned bases' if args.unaligned else ''}), {SETS} buffer sets "
      f"in rotation, 5 interleaved rounds of {REPS} "
      "calls, best round (all rounds)")
for name in legs:
    print(f"  {name:36s} {min(times[name]):8.1f} us   rounds us: " + " ".join(f"{t:.1f}" for t in times[name]))
print(f"  levels {levels}: map positions {sum(n)} = {sum(n) / n[0]:.4f} x level 1's; the pyramid pass reads {H * W * 24 / 1e6:.1f} MB and "
      f"writes {pooled * 16 / 1e6:.1f} MB per plane")
for ch_name in ("RGB", "Y"):
    t1, t5 = min(times[f"vsr_metric_frames {ch_name:3s} SSE + SSIM"]), min(times[f"vsr_msssim_frames {ch_name:3s}"])
    print(f"  {ch_name:3s}: multi-scale / single-scale = {t5 / t1:.3f} (best against best; {t5 - t1:+.1f} us)")
s = driver.frame_msssim(fa[0], fb[0], "y", True, SHAVE)
print(f"  (the pair of set 0 on luma: MS-SSIM {driver.msssim(s, H - 2 * SHAVE, W - 2 * SHAVE)[0]:.6f})")
del fa, fb, legs
torch.cuda.empty_cache()
if args.skip_runner:
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ part 2
from video_super_resolution_amd import VSR  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

S, T = 4, args.frames
model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
model.precision = model.model.precision = "fp16"
fmt = "nv12"
fbytes = driver.yuv_frame_bytes(fmt, H, W)
rs = np.random.RandomState(0)
small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
clip = np.stack([driver.frames_to_yuv(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                      .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
scored = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, score="y")
multi = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, score="y", multiscale=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (T - 2) / (time.perf_counter() - t0)


runs = {'ClipRunner score="y"                  ': lambda: scored.run(clip), 'ClipRunner score="y", multiscale=True': lambda: multi.run(clip)}
for fn in runs.values():   # warm-up: packing, executors, allocator
    fn()
same = np.array_equal(scored.run(clip), multi.run(clip))
fps = {k: [] for k in runs}
for rnd in range(args.rounds):
    for name, fn in runs.items():
        fps[name].append(timed(fn))
print(f"part 2: C3-A (540x960 x4 -> {H}x{W}, fp16, {fmt} in / out, {fbytes / 1e6:.1f} MB per frame each way), {T - 2} windows per run, "
      f"{args.rounds} interleaved rounds; the same output bytes: {same}")
for name, v in fps.items():
    print(f"  {name} best {max(v):6.2f} frames/s   spread of the rounds {max(v) - min(v):.2f}   rounds: " + " ".join(f"{x:.2f}" for x in v))
b0, b1 = (max(v) for v in fps.values())
print(f"  multiscale costs {1e3 / b1 - 1e3 / b0:+.3f} ms per frame (best against best)")
m = multi.metrics
print(f"  (the synthetic weights restore nothing; the numbers only show the path: SSIM {m['ssim'].min():.4f} .. {m['ssim'].max():.4f}, "
      f"MS-SSIM {m['msssim'].min():.4f} .. {m['msssim'].max():.4f} over {T - 2} frames)")
