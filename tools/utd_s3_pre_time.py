"""Time of a FeedbackBlock step at x3 with and without its opening 1x1 chain folded into the first stage's LR load path, for both
modes (PRE3: compress_out -> compress_in -> uptran slice 0, the steps >= 1; PRE2: compress_in -> uptran slice 0, step 0):
  (a) chain launch + POST stage (vsr_s3p_sr_utd_post_f16) + plain stage (vsr_s3_sr_utd_f16)   -- what `fold_chain = False` issues,
  (b) PRE + POST stage (vsr_s3f_sr_utd_pre_f16, csrc/sr_utd_s3f.hip) + plain stage,
also the chain launch alone, the POST stage alone and the PRE + POST stage alone; at 8 x 90 x 160 and at 1, 3, 5 and 8 planes of
720 x 1280.  Device events, the sides interleaved in one process (one untimed pass first), best of the rounds and their spread
(max - min) printed.  Per mode the decision line applies the rule: the fold is worth routing to when (b) beats (a) by more than the
larger of the two spreads at 8 x 720 x 1280.
Then VSR.forward at LR 720 x 1280, x3, fp16, ms per frame: best of 4 rounds of 3 recurrent frames, fold_chain off / on in one process.
usage: utd_s3_pre_time.py [--no-frame | --frame-only] [--rounds R] [--sizes small|large|all]"""
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
SIZES = {"small": ((8, 90, 160, 50), (1, 720, 1280, 10)), "large": ((3, 720, 1280, 6), (5, 720, 1280, 6), (8, 720, 1280, 6))}
SIZES["all"] = SIZES["small"] + SIZES["large"]


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
    st3, sp0, sf0 = P["stage"][3], P["stage_post"][0], P["stage_pre"][0]
    assert type(sp0).__name__ == "_FusedStageS3Post" and type(sf0).__name__ == "_FusedStageS3Pre"
    for N, h, w, reps in SIZES[arg("--sizes", "all")]:
        hp = h * w
        rs = np.random.RandomState(0)
        feat, la, lb = (torch.from_numpy(rs.randn(N, h, w, 32).astype(np.float16)).cuda() for _ in range(3))
        cmap = torch.from_numpy(rs.randn(hp, 32).astype(np.float32)).cuda()
        o3, o6, x = torch.empty_like(feat), torch.empty_like(feat), torch.empty_like(feat).view(N, hp, 32)
        ut0 = dict(ins=[], prev=(P["ut_w"][0], 32), bias=P["ut_b"][0], slope=P["ut_a"][0])
        f_ = feat.view(N, hp, 32)
        stages = {3: [dict(ins=[(la.view(N, hp, 32), P["co_w"], 64), (lb.view(N, hp, 32), P["co_w"], 160)], bias=P["co_b"], slope=P["co_a"], cmap=cmap),
                      dict(ins=[(f_, P["ci_w"], 0)], prev=(P["ci_w"], 32), bias=P["ci_b"], slope=P["ci_a"]), ut0],
                  2: [dict(ins=[(f_, P["ci_w"], 0), (f_, P["ci_w"], 32)], bias=P["ci_b"], slope=P["ci_a"]), ut0]}
        for mode in (3, 2):
            keep = [False] * (mode - 1) + [True]
            pre_in = (la, lb, cmap) if mode == 3 else (None, None, None)

            def chain():
                m._chain(stages[mode], N, hp, keep=keep, outs=[None] * (mode - 1) + [x])

            def step_a():
                chain()
                _, nxt = sp0(x.view(N, h, w, 32), m._chain, out=o3)
                st3(nxt, m._chain, out=o6)

            def step_b():
                _, nxt = sf0(feat, *pre_in, out=o3)
                st3(nxt, m._chain, out=o6)
            sides = (("step (a) chain + POST + plain", step_a), ("step (b) PRE+POST + plain", step_b), ("chain launch alone", chain),
                     ("POST stage alone", lambda: sp0(x.view(N, h, w, 32), m._chain, out=o3)), ("PRE+POST stage alone", lambda: sf0(feat, *pre_in, out=o3)))
            t = {name: [] for name, _ in sides}
            step_a()
            want3, want6 = o3.clone(), o6.clone()
            step_b()
            assert torch.equal(o3, want3) and torch.equal(o6, want6), "the two sides differ"
            for name, fn in sides:   # untimed: clocks and caches settle before the first round
                events(fn, reps)
            for rnd in range(ROUNDS):
                for name, fn in sides:
                    fn()
                    t[name].append(events(fn, reps))
            print(f"x3 step, PRE{mode}, {N} x {h} x {w} (rows per segment {sf0.rows_fn(N, h, w, cus=256, strip=30)}), best of {ROUNDS} rounds:")
            for name, _ in sides:
                print(f"    {name:34s} {show(t[name])}")
            ta, tb = t["step (a) chain + POST + plain"], t["step (b) PRE+POST + plain"]
            gain, spread = min(ta) - min(tb), max(max(ta) - min(ta), max(tb) - min(tb))
            print(f"    (a) - (b) = {gain:8.1f} us; larger spread of the two sides {spread:6.1f} us; "
                  f"PRE+POST - POST stage = {min(t['PRE+POST stage alone']) - min(t['POST stage alone']):7.1f} us", flush=True)
            if (N, h, w) == (8, 720, 1280):
                print(f"    rule at 8 x 720 x 1280, PRE{mode}: the fold {'WINS' if gain > spread else 'does NOT win'} ((a) - (b) {gain:.1f} us against {spread:.1f} us)")
            del want3, want6
        del feat, la, lb, cmap, o3, o6, x, f_, stages
    del m, P
    torch.cuda.empty_cache()

if "--no-frame" not in sys.argv:
    h, w = 720, 1280
    v = fill_module_(VSR(upscale_factor=3).eval(), 0).cuda()
    v.precision = v.model.precision = "fp16"
    clip = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (6, h, w, 3)).astype(np.float32)).cuda()
    configs = [("fold_chain off", False), ("fold_chain on", True)]
    res, frames = {}, {}
    for rnd in range(4):
        for name, fold in configs:
            v.model.fold_chain = fold
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
