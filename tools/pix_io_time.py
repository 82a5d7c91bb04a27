"""Time of the 4:2:2 / 4:4:4 boundary (libvsr_hip_pix.so) beside a device copy of the same bytes and beside the 4:2:0 kernel of the same
depth (libvsr_hip_yuv.so), and of the streamed clip runner with the new formats in and out beside nv12.  Device events, rounds
interleaved, best of the rounds and every round (the spread); the pattern of tools/clip_io_time.py.

  part 1, 2160x3840, one frame per call: vsr_pix_ingest (h == H, no second copy) and vsr_pix_write for yuv422p, yuv444p, yuv422p10le and
          yuv444p10le; for each leg a device-to-device copy of exactly the bytes it moves (the frame read once and written once: 12 bytes
          of float32 RGB per pixel + the packed frame), and the same two entries of the 4:2:0 library at 8 bit (yuv420p) and 10 bit
          (yuv420p10le).  Every leg rotates over SETS buffer sets (4 x 100 MB and more: beyond the 256 MiB Infinity Cache), so the rate
          is algorithmic bytes over time against HBM.  The yardstick is each kernel's share of its copy's rate, beside the share the
          4:2:0 kernel of the same depth reaches in the same run.
  part 2, C3-A (540x960 x4, fp16): ClipRunner (overlap=True) on a 2160x3840 clip decimated by 4, yuv422p10le in and out and yuv444p in
          and out beside nv12 in and out, in frames/s, host clock around work that ends in a wait for the last copy.

    python tools/pix_io_time.py [--frames 12] [--rounds 3] [--skip-runner] [--out profiles/pix_io_time.txt]
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
ap.add_argument("--frames", type=int, default=12, help="frames of the clip of part 2 (windows = frames - 2)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-runner", action="store_true")
ap.add_argument("--out", default=None, help="also write the table there")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
H, W, SETS, ROUNDS, CALLS = 2160, 3840, 4, 5, 40
lines = []


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
rgb = [torch.rand(H, W, 3, device=dev) * 300 - 20 for _ in range(SETS)]
rgb_out = [torch.empty(H, W, 3, device=dev) for _ in range(SETS)]
legs = {}      # name -> (fn, bytes)
groups = []    # (format, depth): the rows of the table
for fmt in ("yuv422p", "yuv444p", "yuv420p", "yuv422p10le", "yuv444p10le", "yuv420p10le"):
    side = "yuv" if fmt in driver.YUV_FORMATS else "pix"
    lib = getattr(L, "load_" + side)()
    fb = driver.pix_frame_bytes(fmt, H, W)
    cf_, ci_ = driver.pix_coefficients(fmt), driver.pix_coefficients(fmt, inverse=True)
    pf, pi = cf_.ctypes.data_as(ctypes.c_void_p), ci_.ctypes.data_as(ctypes.c_void_p)
    code = driver.PIX_FORMATS[fmt]
    frames = [driver.frames_to_pix(rgb[k], fmt) for k in range(SETS)]   # valid codes of the format (a converted random picture)
    out = [torch.empty(fb, dtype=torch.uint8, device=dev) for _ in range(SETS)]
    nbytes = H * W * 12 + fb
    # the copy beside them: the same number of bytes read and written, device to device
    src = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(SETS)]
    dst = [torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(SETS)]
    wr_entry, in_entry = getattr(lib, f"vsr_{side}_write"), getattr(lib, f"vsr_{side}_ingest")

    def wr(i, code=code, pf=pf, out=out, keep=cf_, lib=lib, entry=wr_entry):
        k = i % SETS
        L.check(entry(L.dptr(rgb[k]), L.dptr(out[k], torch.uint8), code, pf, 0, 1, H, W, L.stream()), lib=lib)

    def ing(i, code=code, pi=pi, frames=frames, keep=ci_, lib=lib, entry=in_entry):
        k = i % SETS
        L.check(entry(L.dptr(frames[k], torch.uint8), code, pi, 0, L.dptr(rgb_out[k]), None, 1, H, W, H, W, L.stream()), lib=lib)

    def cp(i, src=src, dst=dst):
        k = i % SETS
        dst[k].copy_(src[k])

    legs[f"ingest {fmt}"] = (ing, nbytes)
    legs[f"write  {fmt}"] = (wr, nbytes)
    legs[f"copy   {fmt}"] = (cp, nbytes)
    groups.append(fmt)

times = {k: [] for k in legs}
for rnd in range(ROUNDS):
    for name, (fn, _) in legs.items():
        fn(0)
        times[name].append(events(fn, CALLS))
say(f"part 1: one {H}x{W} frame per call, {SETS} buffer sets in rotation, {ROUNDS} interleaved rounds of {CALLS} calls, best round (all rounds);")
say("        bytes: the frame read once and written once (float32 RGB + the packed frame); copy: a device copy of the same bytes; share: of the copy's rate")
share = {}
for fmt in groups:
    copy_best = min(times[f"copy   {fmt}"])
    for leg in ("ingest", "write ", "copy  "):
        name = f"{leg} {fmt}"
        nbytes = legs[name][1]
        best = min(times[name])
        share[name] = copy_best / best
        say(f"  {name:20s} {best:7.1f} us  {nbytes / 1e6:6.1f} MB  {nbytes / best * 1e-6:5.2f} TB/s  share {share[name]:4.2f}   rounds us: "
            + " ".join(f"{t:.1f}" for t in times[name]))
say("  share of the copy's rate, new kernel against the 4:2:0 kernel of the same depth (spread: (worst - best) / best over the rounds of the new kernel):")
for fmt in groups:
    if fmt in driver.YUV_FORMATS:
        continue
    ref = "yuv420p10le" if fmt.endswith("10le") else "yuv420p"
    for leg in ("ingest", "write "):
        t = times[f"{leg} {fmt}"]
        say(f"    {leg} {fmt:12s} {share[f'{leg} {fmt}']:4.2f}  vs {ref:12s} {share[f'{leg} {ref}']:4.2f}   spread {(max(t) - min(t)) / min(t) * 100:4.1f} %")
del rgb, rgb_out, legs
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------ part 2
if not args.skip_runner:
    from video_super_resolution_amd import VSR  # noqa: E402
    from video_super_resolution_amd.weights import fill_module_  # noqa: E402

    S, T = 4, args.frames
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = "fp16"
    rs = np.random.RandomState(0)
    small = torch.from_numpy(rs.uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
    big = [torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear").permute(0, 2, 3, 1).contiguous()[0]
           for t in range(T)]
    runs, sizes = {}, {}
    for fmt in ("nv12", "yuv422p10le", "yuv444p"):
        clip = np.stack([driver.frames_to_pix(big[t], fmt).cpu().numpy() for t in range(T)])
        runner = driver.ClipRunner(model, (H, W), fmt, fmt, scale_down=S, overlap=True)
        runs[fmt] = (lambda runner=runner, clip=clip: runner.run(clip))
        sizes[fmt] = (runner.in_bytes, runner.out_bytes)
    del big

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
    say(f"part 2: C3-A (540x960 x4 -> {H}x{W}, fp16), ClipRunner overlap=True, {T - 2} windows per run, {args.rounds} interleaved rounds")
    for name, v in fps.items():
        say(f"  {name:12s} in / out  {sizes[name][0] / 1e6:5.1f} MB in, {sizes[name][1] / 1e6:5.1f} MB out per frame   best {max(v):6.2f} frames/s   rounds: "
            + " ".join(f"{x:.2f}" for x in v))

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# python tools/pix_io_time.py --frames {args.frames} --rounds {args.rounds}" + (" --skip-runner" if args.skip_runner else "") +
                "     (one MI355X, one process; device events for part 1, host clock to the last copy for part 2)\n")
        f.write("\n".join(lines) + "\n")
