"""Time of the training loss (VSR.loss_calculate) with loss_path "reference" beside "fused", and of the pixel-terms launch of
libvsr_hip_loss.so alone, reported and not gated.

  part 1, loss.pixel_terms on three 0..255 float frames, a target and a random mask (40 % set): the sums alone, with the masked float
          frames (what the fp32 configuration asks for), with the NHWC-4 half frames (fp16) and with both.  Bytes per element of a frame
          = 17 read (four floats and the mask byte) + 16 for `masked` + 64/3 for `nhwc4`; achieved bytes/s against the HBM peak of
          8.0 TB/s and against 6.3 TB/s measured for a float4 copy.  A round is REPS calls between two device events and the host clock
          around the same loop without a wait; rounds are interleaved over the legs in one process; best round and spread are shown.
  part 2, the whole loss call on the same frames through a VSR with the synthetic weights and the mask already cached (the first call's
          OSVOS run is not part of a window's cost): today's path, a CPU tensor, against the fused one, a device tensor; both precisions.

    python tools/loss_time.py [--rounds 5] [--reps 20] [--loss-reps 3] [--sizes 512x512,2160x3840]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import torch

from video_super_resolution_amd import VSR
from video_super_resolution_amd import loss as LS
from video_super_resolution_amd.weights import fill_module_

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--loss-reps", type=int, default=3)
ap.add_argument("--sizes", default="512x512,2160x3840")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12


def timed(fn, reps):
    """-> (us per call between device events, us per call of host time to enqueue)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, host * 1e6 / reps


def show(name, rounds, extra=""):
    devs = [r[0] for r in rounds]
    hosts = [r[1] for r in rounds]
    print(f"  {name:46s} {min(devs):10.1f} us   spread {max(devs) - min(devs):8.1f}   host {min(hosts):10.1f} us{extra}   rounds us: "
          + " ".join(f"{d:.1f}" for d in devs))


def interleaved(legs, rounds, reps):
    for fn in legs.values():   # warm-up: code objects, packing, algorithm choice, the allocator
        fn()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(timed(fn, reps))
    return out


print(f"# python tools/loss_time.py --rounds {args.rounds} --reps {args.reps} --loss-reps {args.loss_reps} --sizes {args.sizes}"
      "     (one MI355X, one process)")
model = fill_module_(VSR().eval(), seed=0).to(dev)
for size in args.sizes.split(","):
    H, W = (int(v) for v in size.split("x"))
    g = torch.Generator(device=dev).manual_seed(H * 7 + W)
    outputs = torch.rand((3, H, W, 3), device=dev, generator=g) * 255.0
    target = torch.rand((1, H, W, 3), device=dev, generator=g) * 255.0
    mask = torch.stack((torch.rand((H, W), device=dev, generator=g) < 0.4,) * 3)
    n = 3 * H * W

    # -------------------------------------------------------------------------------------------- part 1
    print(f"part 1: {H}x{W}, {n} elements per frame; {args.rounds} interleaved rounds of {args.reps} calls, best round; us per call "
          "between device events, and of host time")
    legs, per_el = {}, {}
    for name, masked, nhwc4 in (("sums and terms alone", False, False), ("+ masked float frames (fp32)", True, False),
                                ("+ NHWC-4 half frames (fp16)", False, True), ("+ both", True, True)):
        per_el[name] = 17 + 16 * masked + 64 / 3 * nhwc4
        legs[f"pixel_terms {name}"] = lambda masked=masked, nhwc4=nhwc4: LS.pixel_terms(outputs, target, mask, masked, nhwc4)
    rounds = interleaved(legs, args.rounds, args.reps)
    for name in per_el:
        k = f"pixel_terms {name}"
        rate = per_el[name] * n / (min(r[0] for r in rounds[k]) * 1e-6)
        show(k, rounds[k], f"   {per_el[name]:5.1f} B per element   {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the 8.0 TB/s peak, "
                           f"{100 * rate / HBM_COPY:5.1f} % of a float4 copy")

    # -------------------------------------------------------------------------------------------- part 2
    print(f"part 2: {H}x{W}, the whole loss call, mask cached; {args.rounds} interleaved rounds of {args.loss_reps} calls, best round")
    model.loss4object.mask = mask
    values = {}

    def call(precision, path):
        model.precision, model.loss_path = precision, path
        values[(precision, path)] = model.loss_calculate(target, outputs)

    legs = {f"loss_calculate {precision} loss_path={path}": (lambda precision=precision, path=path: call(precision, path))
            for precision in ("fp32", "fp16") for path in ("reference", "fused")}
    rounds = interleaved(legs, args.rounds, args.loss_reps)
    for k in legs:
        show(k, rounds[k])
    for precision in ("fp32", "fp16"):
        a, b = float(values[(precision, "reference")]), float(values[(precision, "fused")])
        best = {path: min(r[0] for r in rounds[f"loss_calculate {precision} loss_path={path}"]) for path in ("reference", "fused")}
        print(f"  {precision}: fused / reference time {best['fused'] / best['reference']:.3f}; loss {b!r} against {a!r} "
              f"(rel {abs(a - b) / abs(a):.1e}); the fused value is a {values[(precision, 'fused')].device.type} tensor, "
              f"the reference's a {values[(precision, 'reference')].device.type} one")
    model.loss4object.reset()
    del outputs, target, mask
    torch.cuda.empty_cache()
