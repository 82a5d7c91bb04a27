"""Time of the one-launch inception block (libvsr_hip_hgi.so, trunk_exec._Inception.fused) against the launches it replaces.  Device
events, rounds interleaved in one process, best of the rounds and their spread.  The lines go to the terminal and to
profiles/hg_inception_time.txt (--out).

  part 1, per block signature (_A to _G), map size (33x60, 67x120, 66x120, 135x240, 132x240) and N (1, 4): the four-launch path
          (fused 1x1 + three k x k, split-K finishes included) against the fused launch, REPS calls per round on one input.  The
          verdict per (signature, size): the fused launch is faster by more than the larger of the two legs' round-to-round spreads at
          BOTH N, or the pair stays on the four launches.
  part 2, the whole hourglass at 1 x and 4 x 540 x 960 with the switch off and on.
  part 3, `bench.py --gpus 1 --steps K --warmup W` in child processes with VSR_HG_INCEPTION=0 and =1, rounds interleaved.

    python tools/hg_inception_time.py [--rounds 3] [--bench-rounds 3] [--skip-bench] [--out profiles/hg_inception_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import numpy as np
import torch

from video_super_resolution_amd import VSR, _lib as L, depth
from video_super_resolution_amd.trunk_exec import _Inception
from video_super_resolution_amd.weights import fill_module_

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--skip-bench", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hg_inception_time.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
REPS = 20
SIZES = [(33, 60), (67, 120), (66, 120), (135, 240), (132, 240)]
SIGS = {"A": depth._A, "B": depth._B, "C": depth._C, "D": depth._D, "E": depth._E, "F": depth._F, "G": depth._G}
lines = ["# python tools/hg_inception_time.py " + " ".join(sys.argv[1:]) + "     (one MI355X; device events around REPS calls; rounds interleaved)"]


def say(text):
    print(text, flush=True)
    lines.append(text)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def interleaved(legs, rounds, reps):
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(events(fn, reps))
    return times


# ------------------------------------------------------------------------------------------------------------ part 1
say(f"part 1: one block per call, {args.rounds} interleaved rounds of {REPS} calls; us = best round (spread of the rounds); "
    f"launches = what the four-launch path issues; verdict per (signature, size) over both N")
torch.manual_seed(0)
verdict = {}
for name, node in SIGS.items():
    inc = _Inception(depth._build(node).eval().to(dev))
    sig = inc.signature()
    for hw in SIZES:
        ok_all = True
        for N in (1, 4):
            x = torch.randn((N,) + hw + (inc.cin,), device=dev).to(torch.float16)
            inc.fused_small = False
            L.ROUTES.calls, L.ROUTES.enabled = [], True
            inc(x, 0)
            L.ROUTES.enabled = False
            routes = [r for _, r in L.ROUTES.calls]
            nlaunch = sum(2 if "splitk" in r else 1 for r in routes)

            def four():
                inc.fused_small = False
                inc(x, 0)

            def fused():
                inc.fused(x, 0)

            t = interleaved({"four": four, "fused": fused}, args.rounds, REPS)
            b4, bf = min(t["four"]), min(t["fused"])
            s4, sf = max(t["four"]) - b4, max(t["fused"]) - bf
            ok = b4 - bf > max(s4, sf)
            ok_all = ok_all and ok
            say(f"  {name} c{sig[0]} mid{sig[1]} k{sig[2]} out{sig[3]} o0 {sig[4]}  {hw[0]:3d}x{hw[1]:3d} N={N}: four launches {b4:7.1f} us ({s4:4.1f}) "
                f"[{nlaunch} launches: {', '.join(routes)}]   fused {bf:7.1f} us ({sf:4.1f})   {L.load_hgi().vsr_hgi_workgroups(N, *hw)} workgroups   "
                f"{'fused wins' if ok else 'four launches stay'}")
        verdict[(name, hw)] = ok_all
say("verdict (fused by default only where it wins at both N): " +
    "; ".join(f"{n} {h}x{w}: {'FUSED' if v else 'four'}" for (n, (h, w)), v in verdict.items()))
rule = {(n, hw): _Inception.fused_rule(_Inception(depth._build(SIGS[n]).eval().to(dev)).signature(), *hw) for (n, hw) in verdict}
differ = [f"{n} {h}x{w}" for (n, (h, w)), v in verdict.items() if v != rule[(n, (h, w))]]
say("the default rule (_Inception.fused_rule) " + ("routes exactly the pairs of this verdict" if not differ else "differs from this verdict at: " + ", ".join(differ)))

# ------------------------------------------------------------------------------------------------------------ part 2
model = fill_module_(VSR().eval(), 0).to(dev)
hx = model._depth_exec.get()
fr = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (4, 540, 960, 3)).astype(np.float32)).to(dev)
old = _Inception.fused_small
say(f"part 2: the hourglass at 540x960, {args.rounds} interleaved rounds of 5 calls, ms = best round (spread); the switch as the environment "
    f"set it: {'on' if old else 'off'}")
for N in (1, 4):
    def run(on, n=N):
        _Inception.fused_small = on
        hx(fr[:n])

    t = interleaved({"off": lambda: run(False), "on": lambda: run(True)}, args.rounds, 5)
    _Inception.fused_small = False
    a = hx(fr[:N]).clone()
    _Inception.fused_small = True
    b = hx(fr[:N]).clone()
    d = float((a - b).abs().max() / a.abs().max())
    say(f"  N={N}: four launches {min(t['off']) / 1e3:6.3f} ms ({(max(t['off']) - min(t['off'])) / 1e3:.3f})   fused blocks "
        f"{min(t['on']) / 1e3:6.3f} ms ({(max(t['on']) - min(t['on'])) / 1e3:.3f})   predictions differ by {d:.2e} of range")
_Inception.fused_small = old
del model, hx, fr
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------------------ part 3
if not args.skip_bench:
    say(f"part 3: bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} in child processes, {args.bench_rounds} interleaved rounds")
    vals = {"0": [], "1": []}
    unit = ""
    for rnd in range(args.bench_rounds):
        for sw in ("0", "1"):
            env = dict(os.environ, VSR_HG_INCEPTION=sw)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                                 env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                say(f"  bench.py failed (VSR_HG_INCEPTION={sw}, round {rnd}): exit {out.returncode}\n{out.stderr[-2000:]}")
                raise SystemExit(1)
            line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            vals[sw].append((float(line["value"]), float(line["ms_per_step"])))
            unit = f"{line['metric']} [{line['unit']}]"
            say(f"  round {rnd} VSR_HG_INCEPTION={sw}: {line['value']} {line['unit']}, {line['ms_per_step']} ms per step")
    m = {sw: sum(v[1] for v in vals[sw]) / len(vals[sw]) for sw in vals}
    s = {sw: max(v[1] for v in vals[sw]) - min(v[1] for v in vals[sw]) for sw in vals}
    say(f"  {unit}; ms per step, mean of the rounds (spread): off {m['0']:.3f} ({s['0']:.3f})   on {m['1']:.3f} ({s['1']:.3f})   "
        f"difference {m['0'] - m['1']:+.3f} ms: {'beyond' if abs(m['0'] - m['1']) > max(s.values()) else 'within'} the spread of the rounds")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
