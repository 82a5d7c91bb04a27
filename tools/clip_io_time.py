"""Time of the 4:2:0 boundary (libvsr_hip_yuv.so) beside the RGB one it stands next to, and of the streamed clip runner beside the
serial RGB loop.  Device events, rounds interleaved, best of the rounds (and the spread of the rounds for the end-to-end legs).

  part 1, 2160x3840, one frame per call: vsr_yuv_write and vsr_yuv_ingest (h == H, no second copy) for nv12 and p010le, beside
          vsr_frame_to_u8 and vsr_clip_ingest_u8 (h == H) on the same box.  Every leg rotates over SETS buffer pairs (4 x 112 MB and
          more: beyond the 256 MiB Infinity Cache), so the rate is algorithmic bytes (the frame read once, written once) over time
          against HBM, to be read beside profiles/r03_stream_rates.txt (hand-written streaming kernels: 5.1-5.6 TB/s for a read/write mix,
          4.2-4.6 TB/s for pure writes).
  part 2, C3-A (540x960 x4, fp16): ClipRunner with overlap=True / False on a 2160x3840 nv12 clip (decimated by 4, as the protocol of
          the benchmark has it; and once from a 1080x1920 source decimated by 2), beside a loop that restates bench.py's `pcie_inclusive` leg (uint8 RGB window from pinned memory,
          ingest_item, forward, frames_to_u8, copy back; serial on one stream), in frames/s, host clock around work that ends in a
          wait for the last copy.

    python tools/clip_io_time.py [--frames 22] [--rounds 3] [--skip-runner]
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
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
H, W, SETS = 2160, 3840, 4


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


# ------------------------------------------------------------------------------------------------ part 1
Y, M = L.load_yuv(), L.load()
rgb = [torch.rand(H, W, 3, device=dev) * 300 - 20 for _ in range(SETS)]
rgb_out = [torch.empty(H, W, 3, device=dev) for _ in range(SETS)]
u8 = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev) for _ in range(SETS)]
u8_out = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(SETS)]
legs = {}
for fmt in ("nv12", "p010le"):
    fb = driver.yuv_frame_bytes(fmt, H, W)
    cf_, ci_ = driver.yuv_coefficients(fmt), driver.yuv_coefficients(fmt, inverse=True)
    pf, pi = cf_.ctypes.data_as(ctypes.c_void_p), ci_.ctypes.data_as(ctypes.c_void_p)
    code = driver.YUV_FORMATS[fmt]
    # frames: valid codes of the format (a converted random picture)
    frames = [driver.frames_to_yuv(rgb[k], fmt) for k in range(SETS)]
    out = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(SETS)]

    def wr(i, code=code, pf=pf, out=out, keep=cf_):
        k = i % SETS
        L.check(Y.vsr_yuv_write(L.dptr(rgb[k]), L.dptr(out[k], torch.uint8), code, pf, 0, 1, H, W, L.stream()), lib=Y)

    def ing(i, code=code, pi=pi, frames=frames, keep=ci_):
        k = i % SETS
        L.check(Y.vsr_yuv_ingest(L.dptr(frames[k], torch.uint8), code, pi, 0, L.dptr(rgb_out[k]), None, 1, H, W, H, W, L.stream()), lib=Y)

    legs[f"vsr_yuv_write  {fmt}"] = (wr, H * W * 12 + fb)
    legs[f"vsr_yuv_ingest {fmt}"] = (ing, H * W * 12 + fb)


def to_u8(i):
    k = i % SETS
    L.check(M.vsr_frame_to_u8(L.dptr(rgb[k]), L.dptr(u8_out[k], torch.uint8), ctypes.c_size_t(H * W * 3), L.stream()))


def from_u8(i):
    k = i % SETS
    L.check(M.vsr_clip_ingest_u8(L.dptr(u8[k], torch.uint8), L.dptr(rgb_out[k]), None, 1, H, W, H, W, L.stream()))


legs["vsr_frame_to_u8    (RGB)"] = (to_u8, H * W * 15)
legs["vsr_clip_ingest_u8 (RGB)"] = (from_u8, H * W * 15)
times = {k: [] for k in legs}
for rnd in range(5):
    for name, (fn, _) in legs.items():
        fn(0)
        times[name].append(events(fn, 40))
print(f"part 1: one {H}x{W} frame per call, {SETS} buffer sets in rotation, 5 interleaved rounds of 40 calls, best round (all rounds)")
for name, (_, nbytes) in legs.items():
    best = min(times[name])
    print(f"  {name:28s} {best:7.1f} us  {nbytes / 1e6:6.1f} MB  {nbytes / best * 1e-6:5.2f} TB/s   rounds us: "
          + " ".join(f"{t:.1f}" for t in times[name]))
del rgb, rgb_out, u8, u8_out, legs
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
fb = driver.yuv_frame_bytes(fmt, H, W)
rs = np.random.RandomState(0)
small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
clip = np.stack([driver.frames_to_yuv(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                      .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
over = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True)
serial = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=False)
# the same LR frames from a source of half the size each way (1080x1920, decimated by 2): 3.1 MB per upload
H2, W2 = H // 2, W // 2
clip2 = np.ascontiguousarray(clip[:, :driver.yuv_frame_bytes(fmt, H2, W2)])
over2 = driver.ClipRunner(model, (H2, W2), fmt, fmt, scale_down=S // 2, overlap=True)
win_host = torch.randint(0, 256, (1, 3, H, W, 3), dtype=torch.uint8).pin_memory()
out_host = torch.empty((H, W, 3), dtype=torch.uint8).pin_memory()
hf = torch.zeros((3, H, W, 3), dtype=torch.float32, device=dev)


def rgb_loop():
    """bench.py's `pcie_inclusive` leg, restated: every window crosses as three uint8 RGB frames, all on the compute stream."""
    e = None
    with torch.no_grad():
        for t in range(T - 2):
            win = win_host.to(dev, non_blocking=True)
            data, _, _ = driver.ingest_item(win, S, want_hr=False)
            e, _ = model(data[0], None, hf, e, train=False)
            out_host.copy_(driver.frames_to_u8(e[0]), non_blocking=True)
        torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (T - 2) / (time.perf_counter() - t0)


runs = {"ClipRunner overlap=True  (nv12 in / out)": lambda: over.run(clip), "ClipRunner overlap=False (nv12 in / out)": lambda: serial.run(clip),
        "ClipRunner overlap=True, 1080x1920 in   ": lambda: over2.run(clip2), "RGB loop (pcie_inclusive restated)      ": rgb_loop}
for fn in runs.values():   # warm-up: packing, executors, allocator
    fn()
same = np.array_equal(over.run(clip), serial.run(clip))
fps = {k: [] for k in runs}
for rnd in range(args.rounds):
    for name, fn in runs.items():
        fps[name].append(timed(fn))
print(f"part 2: C3-A (540x960 x4 -> {H}x{W}, fp16), {T - 2} windows per run, {args.rounds} interleaved rounds; overlapped == serial bytes: {same}")
print(f"  per frame: ClipRunner {fb / 1e6:.1f} MB in ({over2.in_bytes / 1e6:.1f} MB from 1080x1920), {fb / 1e6:.1f} MB out | RGB loop {win_host.numel() / 1e6:.1f} MB in, {out_host.numel() / 1e6:.1f} MB out")
for name, v in fps.items():
    print(f"  {name} best {max(v):6.2f} frames/s   rounds: " + " ".join(f"{x:.2f}" for x in v))
