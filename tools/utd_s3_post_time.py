"""Time of the x3 stage pair of a FeedbackBlock step with and without the uptran slice inside the first stage's launch:
  (a) plain stage (vsr_s3_sr_utd_f16) + one-stage 1x1 chain launch + plain stage   -- what `fuse_uptran = False` issues,
  (b) POST stage (vsr_s3p_sr_utd_post_f16, csrc/sr_utd_s3p.hip) + plain stage,
also the chain launch alone, the plain stage alone and the POST stage alone; at 8, 5, 3 and 1 planes of 720 x 1280 and at 8 x 90 x 160.
Device events, the sides interleaved in one process (one untimed pass first), best of the rounds and their spread (max - min) printed.
Then VSR.forward at LR 720 x 1280, x3, fp16, ms per frame over recurrent frames: fuse_uptran off / on, and with fuse_uptran on,
early_scales without / with 3 at the given early_planes levels.
usage: utd_s3_post_time.py [--no-frame | --frame-only] [--rounds R] [--levels 1,2,3]"""
import os, sys
os.environ.setdefault('MIOPEN_FIND_MODE', '2'); os.environ.setdefault('MIOPEN_LOG_LEVEL', '2')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from video_super_resolution_amd import SRProjectionModule, VSR
from video_super_resolution_amd.weights import fill_module_

assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.set_grad_enabled(False)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROUNDS = max(3, int(arg("--rounds", 5)))
LEVELS = [int(v) for v in arg("--levels", "1").split(",")]


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def show(ts):
    return f"{min(ts):9.1f} us (spread {max(ts) - min(ts):6.1f})"


if "--frame-only" not in sys.argv:
    m = fill_module_(SRProjectionModule(upscale_factor=3).eval(), 0, "model.").cuda()
    P = m._packed()
    st0, st3, sp0 = P["stage"][0], P["stage"][3], P["stage_post"][0]
    assert type(sp0).__name__ == "_FusedStageS3Post" and type(st0).__name__ == "_FusedStageS3"
    ut3 = lambda src: dict(ins=[(src, P["ut_w"][3], 32 * 4)], bias=P["ut_b"][3], slope=P["ut_a"][3])
    for N, h, w, reps in ((8, 90, 160, 50), (1, 720, 1280, 10), (3, 720, 1280, 6), (5, 720, 1280, 6), (8, 720, 1280, 6)):
        a = torch.from_numpy((np.random.RandomState(0).randn(N, h, w, 32) * 20).astype(np.float16)).cuda()
        o3, o6, a3 = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a).view(N, h * w, 32)

        def chain():
            m._chain([ut3(o3.view(N, h * w, 32))], N, h * w, keep=[True], outs=[a3])

        def pair_a():
            st0(a, m._chain, out=o3)
            chain()
            st3(a3.view(N, h, w, 32), m._chain, out=o6)

        def pair_b():
            _, nxt = sp0(a, m._chain, out=o3)
            st3(nxt, m._chain, out=o6)
        sides = (("pair (a) plain + chain + plain", pair_a), ("pair (b) POST + plain", pair_b), ("chain launch alone", chain),
                 ("plain stage alone", lambda: st0(a, m._chain, out=o3)), ("POST stage alone", lambda: sp0(a, m._chain, out=o3)))
        t = {name: [] for name, _ in sides}
        pair_a()
        want3, want6 = o3.clone(), o6.clone()
        pair_b()
        assert torch.equal(o3, want3) and torch.equal(o6, want6), "the two sides differ"
        for name, fn in sides:   # untimed: clocks and caches settle before the first round
            events(fn, reps)
        for rnd in range(ROUNDS):
            for name, fn in sides:
                fn()
                t[name].append(events(fn, reps))
        print(f"x3 stage pair, {N} x {h} x {w} (rows per segment {sp0.rows_fn(N, h, w, cus=256, strip=30)}), best of {ROUNDS} rounds:")
        for name, _ in sides:
            print(f"    {name:34s} {show(t[name])}")
        ta, tb = t["pair (a) plain + chain + plain"], t["pair (b) POST + plain"]
        print(f"    (a) - (b) = {min(ta) - min(tb):8.1f} us; larger spread of the two sides {max(max(ta) - min(ta), max(tb) - min(tb)):6.1f} us; "
              f"POST - plain stage = {min(t['POST stage alone']) - min(t['plain stage alone']):7.1f} us")
        del a, o3, o6, a3, want3, want6
    del m, P
    torch.cuda.empty_cache()

if "--no-frame" not in sys.argv:
    h, w = 720, 1280
    v = fill_module_(VSR(upscale_factor=3).eval(), 0).cuda()
    v.precision = v.model.precision = "fp16"
    clip = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (6, h, w, 3)).astype(np.float32)).cuda()
    configs = [("fuse_uptran off", False, (4,), 1), ("fuse_uptran on", True, (4,), 1)]
    configs += [(f"fuse_uptran on, early_scales (4, 3), early_planes {lv}", True, (4, 3), lv) for lv in LEVELS]
    res, frames = {}, {}
    for rnd in range(ROUNDS):
        for name, post, scales, level in configs:
            v.model.fuse_uptran, v.early_scales, v.early_planes = post, scales, level
            est, _ = v(clip[0:3], None, None, None, train=False)      # first call: untimed (packing, buffers)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for t_ in range(1, 4):
                est, _ = v(clip[t_:t_ + 3], None, None, est, train=False)
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(e0.elapsed_time(e1) / 3)
            frames.setdefault(name, est.clone())
    ref = frames[configs[0][0]]
    for name, ms in res.items():
        print(f"VSR.forward LR {h} x {w} x3 fp16, {name}: {min(ms):8.2f} ms per frame (best of {len(ms)} rounds of 3 recurrent frames, "
              f"spread {max(ms) - min(ms):5.2f} ms; last frame equal to the first configuration's: {bool(torch.equal(frames[name], ref))})")
