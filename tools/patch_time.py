"""Time of the training-patch gather (libvsr_hip_patch.so) at the size a x4 training run on 4K frames has, beside a device copy of the same
bytes and beside the torch composition that does the same work, and of a `ClipTrainer` step with the gather's share of it.  Device events,
rounds interleaved, best of the rounds (and all rounds shown).  The lines go to the terminal and to profiles/patch_time.txt (--out).

  part 1, one call: B = 16 samples of n = 3 frames, HR patch 256 x 256 out of --group frames of 2160 x 3840, S = 4, hr and the nearest lr.
          Tables with all 16 flag values, with flags 0 alone and with flags 4 (the transposition) alone; every call takes another table
          (random origins and first frames) and another pair of output buffers out of SETS (beyond the 256 MiB Infinity Cache), so the
          rate is algorithmic bytes (every output word read once and written once) over time against HBM.  Beside it a device copy that
          moves the same bytes, and the composition of torch slicing / flip / transpose / contiguous / strided slicing per sample.
  part 2, ClipTrainer on a 2160 x 3840 yuv420p clip, x4, fp32, LR patch 64, groups of 8 frames, 4 samples each: host clock per step around
          a run that ends in the copy of the losses, and the device time of the run's gathers (events around each).

    python tools/patch_time.py [--rounds 3] [--group 12] [--frames 16] [--skip-trainer] [--out profiles/patch_time.txt]
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
ap.add_argument("--group", type=int, default=12, help="resident frames of part 1")
ap.add_argument("--frames", type=int, default=16, help="frames of the clip of part 2 (two groups of 8)")
ap.add_argument("--skip-trainer", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_time.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
H, W, S, B, N, P, REPS = 2160, 3840, 4, 16, 3, 256, 24
lines = ["# python tools/patch_time.py " + " ".join(sys.argv[1:]) + "     (one MI355X, one process; device events for part 1, host clock to the "
         "last copy and device events around the gathers for part 2)"]


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


# ---------------------------------------------------------------------------------------------------- part 1
G = args.group
src = torch.rand(G, H, W, 3, device=dev) * 255
hr_bytes, lr_bytes = B * N * P * P * 12, B * N * (P // S) * (P // S) * 12
nbytes = 2 * (hr_bytes + lr_bytes)
SETS = max(3, -(-3 * (256 << 20) // (hr_bytes + lr_bytes)))
hr = [torch.empty(B, N, P, P, 3, device=dev) for _ in range(SETS)]
lr = [torch.empty(B, N, P // S, P // S, 3, device=dev) for _ in range(SETS)]
rs = np.random.RandomState(0)


def tables(flags):
    out = []
    for _ in range(REPS):
        t = driver.patch_table(rs, B, G, N, (H, W), P, S)
        t[:, 3] = flags
        out.append(t)
    return out


def torch_gather(table, hr_out, lr_out):
    """The same work by torch indexing: one crop, its flips, transposition and time reversal, a dense copy, a strided one, per sample."""
    for b, (t0, y0, x0, f) in enumerate(table.tolist()):
        v = src[t0:t0 + N, y0:y0 + P, x0:x0 + P]
        dims = [d for d, bit in ((0, 8), (1, 2), (2, 1)) if f & bit]
        if dims:
            v = v.flip(dims)
        if f & 4:
            v = v.transpose(1, 2)
        hr_out[b].copy_(v)
        lr_out[b].copy_(hr_out[b][:, ::S, ::S])


T_ALL, T_0, T_4 = tables(np.arange(16, dtype=np.int32)), tables(0), tables(4)
# the composition is the kernel's result (flags: flip of the crop first, then the transposition, as the header's steps read backwards)
driver.patch_gather(src, T_ALL[0], N, P, S, hr_out=hr[0], lr_out=lr[0])
torch_gather(T_ALL[0], hr[1], lr[1])
same = torch.equal(hr[0], hr[1]) and torch.equal(lr[0], lr[1])
c_src = [torch.empty((hr_bytes + lr_bytes), dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(SETS)]
c_dst = [torch.empty((hr_bytes + lr_bytes), dtype=torch.uint8, device=dev) for _ in range(SETS)]
legs = {
    "vsr_patch_gather, all 16 flag values": lambda i: driver.patch_gather(src, T_ALL[i % REPS], N, P, S, hr_out=hr[i % SETS], lr_out=lr[i % SETS]),
    "vsr_patch_gather, flags 0 (plain rows)": lambda i: driver.patch_gather(src, T_0[i % REPS], N, P, S, hr_out=hr[i % SETS], lr_out=lr[i % SETS]),
    "vsr_patch_gather, flags 4 (transposed, through LDS)": lambda i: driver.patch_gather(src, T_4[i % REPS], N, P, S, hr_out=hr[i % SETS], lr_out=lr[i % SETS]),
    "device copy moving the same bytes": lambda i: c_dst[i % SETS].copy_(c_src[i % SETS]),
    "torch slicing / flip / transpose / copies, all 16 flags": lambda i: torch_gather(T_ALL[i % REPS], hr[i % SETS], lr[i % SETS]),
}
times = {k: [] for k in legs}
for rnd in range(args.rounds):
    for name, fn in legs.items():
        fn(0)
        times[name].append(events(fn, REPS))
say(f"part 1: B = {B} samples of n = {N} frames, HR patch {P}x{P} and its x{S} nearest LR patch out of {G} frames of {H}x{W}; {SETS} output sets "
    f"and {REPS} tables in rotation, {args.rounds} interleaved rounds of {REPS} calls, best round (all rounds); torch composition equals the "
    f"kernel bit for bit: {same}")
for name in legs:
    best = min(times[name])
    say(f"  {name:58s} {best:8.1f} us  {nbytes / 1e6:6.1f} MB  {nbytes / best * 1e-6:5.2f} TB/s   rounds us: " + " ".join(f"{t:.1f}" for t in times[name]))
b_all, b_0, b_4, b_copy, b_torch = (min(times[k]) for k in legs)
say(f"  transposed / plain {b_4 / b_0:.2f}, transposed / copy {b_4 / b_copy:.2f}, plain / copy {b_0 / b_copy:.2f}, torch composition / "
    f"all flags {b_torch / b_all:.2f}")
del src, hr, lr, c_src, c_dst, legs
torch.cuda.empty_cache()

if not args.skip_trainer:
    # ------------------------------------------------------------------------------------------------ part 2
    from video_super_resolution_amd import VSR, optim  # noqa: E402
    from video_super_resolution_amd.weights import fill_module_  # noqa: E402

    T, fmt = args.frames, "yuv420p"
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = "fp32"
    small = torch.from_numpy(np.random.RandomState(0).uniform(0, 255, (T, H // 8, W // 8, 3)).astype(np.float32)).to(dev)
    clip = np.stack([driver.frames_to_pix(torch.nn.functional.interpolate(small[t:t + 1].permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
                                          .permute(0, 2, 3, 1).contiguous()[0], fmt).cpu().numpy() for t in range(T)])
    for loss_path in ("reference", "fused"):
        opt = optim.Adam(model.parameters(), lr=1e-4)
        tr = driver.ClipTrainer(model, opt, (H, W), fmt, patch=P // S, group=8, samples_per_group=4, seed=0, loss_path=loss_path)
        tr.run(clip[:8])                     # warm-up: packing, executors, allocator, the solver's choices
        tr.gather_events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = tr.run(clip)
        dt = time.perf_counter() - t0
        gather_ms = [a.elapsed_time(b) for a, b in tr.gather_events]
        say(f"part 2: ClipTrainer, {T} {fmt} frames of {H}x{W}, x{S} fp32, LR patch {P // S}, groups of 8, 4 samples each, loss_path={loss_path}: "
            f"{steps} steps in {dt:.2f} s = {dt / steps * 1e3:.1f} ms per step; {len(gather_ms)} gathers of " +
            " ".join(f"{g * 1e3:.0f}" for g in gather_ms) + f" us = {sum(gather_ms) / (dt * 1e3) * 100:.4f} % of the run; "
            f"{tr.h2d_bytes / 1e6:.1f} MB uploaded; losses {tr.losses[0]:.2f} .. {tr.losses[-1]:.2f}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
