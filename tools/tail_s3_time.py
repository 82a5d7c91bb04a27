"""Time of the one-launch x3 tail (vsr_s3t_sr_tail_f16 / _fold_f16, csrc/sr_tail_s3.hip) beside the unfused route it replaces
(sr.py:_PhaseDeconv: nine phase convolutions, + vsr_sr_convout_planes_f16, in chunks of planes) at 8 x 90 x 160 and 8 x 720 x 1280
(720p -> 2160p), full and decimated, plain and with the folded compress_out (+ the chain launch the fold replaces); device events,
unfused first, rounds interleaved, best of the rounds.  Then VSR.forward at LR 720 x 1280, x3, fp16 with fused_tail_s3 on / off and
share_tail on / off.  Prints us per call, the algorithmic FLOP rate at 115,904 FLOP per LR pixel and plane (full frames), and ms
per frame.
usage: tail_s3_time.py [--no-frame]"""
import os, sys
os.environ.setdefault('MIOPEN_FIND_MODE', '2'); os.environ.setdefault('MIOPEN_LOG_LEVEL', '2')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from video_super_resolution_amd import SRProjectionModule, VSR
from video_super_resolution_amd.weights import fill_module_

assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.set_grad_enabled(False)
FLOP_PER_PIXEL = 2 * 32 * 32 * 49 + 9 * 2 * 32 * 3 * 9    # 115,904


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def module(tail):
    m = fill_module_(SRProjectionModule(upscale_factor=3).eval(), 0, "model.").cuda()
    m.precision, m.fused_tail_s3 = "fp16", tail
    return m


mf, mu = module(True), module(False)
Pf, Pu = mf._packed(), mu._packed()
assert "tail_s3" in Pf and Pf["tail_s3_fold"] and "tail_s3" not in Pu
for N, h, w, reps in ((8, 90, 160, 20), (8, 720, 1280, 3)):
    rs = np.random.RandomState(0)
    lr3, lr6 = (torch.from_numpy(rs.randn(N, h, w, 32).astype(np.float16)).cuda() for _ in range(2))
    cmap = torch.from_numpy(rs.randn(h * w, 32).astype(np.float32)).cuda()
    co = dict(ins=[(lr3.view(N, h * w, 32), Pf["co_w"], 64), (lr6.view(N, h * w, 32), Pf["co_w"], 160)], bias=Pf["co_b"], slope=Pf["co_a"], cmap=cmap)
    hid = mf._chain([co], N, h * w, keep=[True])[0].view(N, h, w, 32)
    flop = float(FLOP_PER_PIXEL) * N * h * w
    for dec in (False, True):
        raw = torch.empty((N, 3, h if dec else 3 * h, w if dec else 3 * w), dtype=torch.float32, device="cuda")
        cases = {
            "unfused": lambda: mu._tail_raw(hid, Pu, dec, raw),
            "fused": lambda: mf._tail_raw(hid, Pf, dec, raw),
            "chain": lambda: mf._chain([co], N, h * w, keep=[True]),
            "fold": lambda: mf._tail_raw(lr3, Pf, dec, raw, fold=(lr3, lr6, cmap)),
        }
        t = {k: [] for k in cases}
        for rnd in range(3):
            for name, fn in cases.items():
                fn()
                t[name].append(events(fn, reps))
        b = {k: min(v) for k, v in t.items()}
        rows = mf._rows_per_segment(N, h, w, cus=512, strip=30)
        print(f"x3 tail {N} x {h} x {w} {'dec ' if dec else 'full'}: unfused {b['unfused']:9.1f} us | fused {b['fused']:9.1f} us"
              + (f" = {flop / b['fused'] * 1e-6:6.1f} TFLOP/s" if not dec else "") + f" (rows per segment {rows}) | unfused / fused {b['unfused'] / b['fused']:5.2f} | "
              f"chain {b['chain']:8.1f} us, chain + fused {b['chain'] + b['fused']:9.1f} us | fold {b['fold']:9.1f} us", flush=True)
        del raw
    del lr3, lr6, cmap, hid, co
torch.cuda.empty_cache()

if "--no-frame" not in sys.argv:
    h, w = 720, 1280
    v = fill_module_(VSR(upscale_factor=3).eval(), 0).cuda()
    v.precision = v.model.precision = "fp16"
    clip = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (6, h, w, 3)).astype(np.float32)).cuda()
    res = {}
    for rnd in range(2):
        for tail, share in ((False, True), (True, True), (True, False)):
            name = f"fused_tail_s3 = {tail}, share_tail = {share}"
            v.model.fused_tail_s3, v.share_tail = tail, share
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
        print(f"VSR.forward LR {h} x {w} x3 fp16, {name}: {min(ms):8.2f} ms per frame (best of {len(ms)} rounds of 3 recurrent frames)", flush=True)
