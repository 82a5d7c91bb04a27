"""Time of the fused x3 stage (vsr_s3_sr_utd_f16, csrc/sr_utd_s3.hip) beside the unfused launches it replaces (sr.py:_UnfusedStage:
nine phase deconvolutions, in-place 1x1, strided convolution) at 8 x 720 x 1280 (720p -> 2160p) and at one small size; device
events, rounds interleaved, best of the rounds.  Then VSR.forward at LR 720 x 1280, x3, fp16 with fused_s3 on and off.  Prints us
per launch, the algorithmic FLOP rate at 219,136 FLOP per LR pixel and plane, and ms per frame.
usage: utd_s3_time.py [--no-frame]"""
import os, sys
os.environ.setdefault('MIOPEN_FIND_MODE', '2'); os.environ.setdefault('MIOPEN_LOG_LEVEL', '2')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from video_super_resolution_amd import SRProjectionModule, VSR
from video_super_resolution_amd.sr import _UnfusedStage
from video_super_resolution_amd.weights import fill_module_

assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.set_grad_enabled(False)
FLOP_PER_PIXEL = 2 * 32 * 32 * (49 + 49 + 9)    # 219,136


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


m = fill_module_(SRProjectionModule(upscale_factor=3).eval(), 0, "model.").cuda()
m.fused_s3 = True
P = m._packed()
fused = P["stage"][0]
assert type(fused).__name__ == "_FusedStageS3"
b = m.block
unfused = _UnfusedStage(b.upBlocks[1], P["dt_w"][1], 64, P["dt_b"][1], P["dt_a"][1], b.downBlocks[2], 3)
for N, h, w, reps in ((8, 90, 160, 20), (8, 720, 1280, 3)):
    a = torch.from_numpy((np.random.RandomState(0).randn(N, h, w, 32) * 20).astype(np.float16)).cuda()
    out = torch.empty_like(a)
    t = {"fused": [], "unfused": []}
    for rnd in range(3):
        for name, st in (("fused", fused), ("unfused", unfused)):
            fn = lambda st=st: st(a, m._chain, out=out)
            fn()
            t[name].append(events(fn, reps))
    flop = float(FLOP_PER_PIXEL) * N * h * w
    bf, bu = min(t["fused"]), min(t["unfused"])
    rows = fused.rows_fn(N, h, w, cus=256, strip=30)
    print(f"x3 stage {N} x {h} x {w}: fused {bf:10.1f} us = {flop / bf * 1e-6:6.1f} TFLOP/s (rows per segment {rows}) | "
          f"unfused {bu:10.1f} us = {flop / bu * 1e-6:6.1f} TFLOP/s | unfused / fused {bu / bf:5.2f}")
    del a, out
torch.cuda.empty_cache()

if "--no-frame" not in sys.argv:
    h, w = 720, 1280
    v = fill_module_(VSR(upscale_factor=3).eval(), 0).cuda()
    v.precision = v.model.precision = "fp16"
    clip = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (6, h, w, 3)).astype(np.float32)).cuda()
    res = {}
    for rnd in range(2):
        for name, on in (("fused_s3 = True", True), ("fused_s3 = False", False)):
            v.model.fused_s3 = on
            v.model._pack = None
            est, _ = v(clip[0:3], None, None, None, train=False)      # first call: untimed (packing, buffers)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for t_ in range(1, 4):
                est, _ = v(clip[t_:t_ + 3], None, None, est, train=False)
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(e0.elapsed_time(e1) / 3)
    for name, ms in res.items():
        print(f"VSR.forward LR {h} x {w} x3 fp16, {name}: {min(ms):8.2f} ms per frame (best of {len(ms)} rounds of 3 recurrent frames)")
