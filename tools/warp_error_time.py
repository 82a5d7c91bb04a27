"""Time of the temporal warping error (libvsr_hip_warp.so) at the headline frame size, beside a copy that moves the same bytes and beside
the FlowNet2 pass that makes its flows, and of the streamed clip runner with and without it.  Device events, rounds interleaved, best of
the rounds (and all rounds shown).

  part 1, 2160x3840, one pair per call (P = 1, quantise = 1, shave = 4, the crop FlowNet2 sees: 2112x3840): vsr_warp_error (both
          launches) for RGB and Y with planar float32 flows, and for Y with the fp16 executor's NHWC half map (ld = 32).  Every leg
          rotates over SETS sets of frames and flows (3 x 329 MB with float32 flows: beyond the 256 MiB Infinity Cache), so the rate is
          algorithmic bytes (both frames of the crop and both flows read once: 24 + 16 B per pixel, 24 + 8 B with half flows; the map's
          other 30 channels are not counted) over time against HBM.  Beside it a device copy that moves the same bytes (half of them
          read, half written).
  part 2, the same frames: driver.truth_flows, FlowNet2 forward and backward as one batch of two on the fp16 executor.
  part 3, C3-A (540x960 x4, fp16): ClipRunner on a 2160x3840 nv12 clip (decimated by 4) with score="y" and temporal=None / "warp", legs
          interleaved, in frames/s, host clock around work that ends in a wait for the last copy.  The occlusion rule is opened (c2 = g2 =
          1e6) so that every in-frame pixel is scored.

    python tools/warp_error_time.py [--frames 12] [--rounds 3] [--skip-runner]
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
ap.add_argument("--frames", type=int, default=12, help="frames of the clip of part 3 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-runner", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
H, W, SETS, SHAVE, REPS, LD = 2160, 3840, 3, 4, 12, 32
h, w = (H // 64) * 64, (W // 64) * 64
y0, x0 = (H - h) // 2, (W - w) // 2


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


# ------------------------------------------------------------------------------------------------ part 1
M = L.load_warp()
fa = [torch.rand(H, W, 3, device=dev) * 300 - 20 for _ in range(SETS)]
fb = [(fa[k] + torch.randn(H, W, 3, device=dev) * 4).contiguous() for k in range(SETS)]
# smooth flows of a few pixels with a little noise, the backward flow the negative: most pixels are valid and every gather runs
yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
f32, f16 = [], []
for k in range(SETS):
    u = 2.5 + 1.5 * torch.sin(yy / 211.0 + k) + 0.004 * torch.randn(h, w, device=dev)
    v = -1.5 + 1.0 * torch.cos(xx / 173.0 - k) + 0.004 * torch.randn(h, w, device=dev)
    fwd = torch.stack([u, v])[None].contiguous()
    f32.append((fwd, (-fwd).contiguous()))
    maps = []
    for t in f32[-1]:
        m = torch.zeros((1, h, w, LD), dtype=torch.float16, device=dev)
        m[..., :2] = t[0].permute(1, 2, 0)
        maps.append(m)
    f16.append(tuple(maps))
sums = torch.empty(1, 4, dtype=torch.float64, device=dev)
ws = torch.empty(int(M.vsr_warp_ws_bytes(1, h, w, SHAVE)), dtype=torch.uint8, device=dev)
c = driver.yuv_coefficients("yuv420p", "bt601", False)
luma4 = np.ascontiguousarray(np.array([c[0], c[1], c[2], c[9]], dtype=np.float32))
occ = np.ascontiguousarray(np.array(driver.WARP_OCC, dtype=np.float64))
pl, po = luma4.ctypes.data_as(ctypes.c_void_p), occ.ctypes.data_as(ctypes.c_void_p)
legs = {}
for name, ch, flows, ftype, strides, fdt, bpp in (("RGB, float32 flows", 0, f32, 0, (2 * h * w, h * w, 1), torch.float32, 40),
                                                  ("Y,   float32 flows", 1, f32, 0, (2 * h * w, h * w, 1), torch.float32, 40),
                                                  ("Y,   half map ld 32", 1, f16, 1, (h * w * LD, 1, LD), torch.float16, 32)):
    def leg(i, ch=ch, flows=flows, ftype=ftype, strides=strides, fdt=fdt):
        k = i % SETS
        L.check(M.vsr_warp_error(L.dptr(fa[k]), L.dptr(fb[k]), 1, H, W, y0, x0, h, w, L.dptr(flows[k][0], fdt), L.dptr(flows[k][1], fdt), ftype,
                                 strides[0], strides[1], strides[2], ch, 1, SHAVE, pl, po, L.dptr(sums, torch.float64), L.dptr(ws, torch.uint8),
                                 L.stream()), "warp_error", lib=M)

    legs[f"vsr_warp_error {name}"] = (leg, h * w * bpp)
nbytes = h * w * 40
src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(SETS)]
dst = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(SETS)]
legs["device copy moving the same bytes"] = (lambda i: dst[i % SETS].copy_(src[i % SETS]), nbytes)
times = {k: [] for k in legs}
for rnd in range(5):
    for name, (fn, _) in legs.items():
        fn(0)
        times[name].append(events(fn, REPS))
print(f"part 1: one {H}x{W} pair per call over the crop {h}x{w} (quantise 1, shave {SHAVE}), {SETS} buffer sets in rotation, 5 interleaved "
      f"rounds of {REPS} calls, best round (all rounds)")
for name, (_, nb) in legs.items():
    best = min(times[name])
    print(f"  {name:36s} {best:8.1f} us  {nb / 1e6:6.1f} MB  {nb / best * 1e-6:5.2f} TB/s   rounds us: " + " ".join(f"{t:.1f}" for t in times[name]))
e, share = driver.ewarp(driver.warp_error(fa[0], fb[0], (f32[0][0], f32[0][1], (y0, x0, h, w)), "y", True, SHAVE))
print(f"  (the pair of set 0 on luma: E_warp {e[0]:.6f}, valid share {share[0]:.4f})")
del f32, f16, src, dst, legs
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------ part 2
from video_super_resolution_amd import VSR  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

S, T = 4, args.frames
model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
model.precision = model.model.precision = "fp16"
driver.truth_flows(model, fa[0], fb[0])   # warm-up: the executor and its buffers
flow_us = []
for rnd in range(args.rounds):
    flow_us.append(events(lambda i: driver.truth_flows(model, fa[i % SETS], fb[i % SETS]), 3))
print(f"part 2: driver.truth_flows at {H}x{W} (FlowNet2 forward and backward over {h}x{w} as one batch of two, fp16 executor), {args.rounds} "
      f"rounds of 3 calls: best {min(flow_us) / 1e3:8.2f} ms   rounds ms: " + " ".join(f"{t / 1e3:.2f}" for t in flow_us))
del fa, fb
torch.cuda.empty_cache()
if args.skip_runner:
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ part 3
fmt = "nv12"
fbytes = driver.yuv_frame_bytes(fmt, H, W)
rs = np.random.RandomState(0)
small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
clip = np.stack([driver.frames_to_yuv(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                      .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
off = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, score="y")
# (the synthetic weights estimate no motion: under the published constants no pixel would be valid and the kernel would skip its frame
# gathers; the rule is opened so that every in-frame pixel is scored, the kernel's most expensive case)
on = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True, score="y", temporal="warp", occ=(0.01, 1e6, 0.01, 1e6))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (T - 2) / (time.perf_counter() - t0)


runs = {'ClipRunner score="y" temporal=None  ': lambda: off.run(clip), 'ClipRunner score="y" temporal="warp"': lambda: on.run(clip)}
for fn in runs.values():   # warm-up: packing, executors, allocator
    fn()
same = np.array_equal(off.run(clip), on.run(clip))
fps = {k: [] for k in runs}
for rnd in range(args.rounds):
    for name, fn in runs.items():
        fps[name].append(timed(fn))
print(f"part 3: C3-A (540x960 x4 -> {H}x{W}, fp16, {fmt} in / out, {fbytes / 1e6:.1f} MB per frame each way), {T - 2} windows per run, "
      f"{args.rounds} interleaved rounds; bytes with and without temporal equal: {same}")
for name, v in fps.items():
    print(f"  {name} best {max(v):6.2f} frames/s   spread of the rounds {max(v) - min(v):.2f}   rounds: " + " ".join(f"{x:.2f}" for x in v))
b0, b1 = (max(v) for v in fps.values())
print(f"  the warping error costs {1e3 / b1 - 1e3 / b0:+.3f} ms per frame (best against best)")
m = on.metrics
print(f"  (the synthetic weights estimate no motion; the numbers only show the path: E_warp {np.nanmin(m['ewarp']):.6f} .. {np.nanmax(m['ewarp']):.6f}, "
      f"truth {np.nanmin(m['ewarp_truth']):.6f} .. {np.nanmax(m['ewarp_truth']):.6f}, valid share {m['valid_share'].min():.4f} .. "
      f"{m['valid_share'].max():.4f} over {T - 3} pairs)")
