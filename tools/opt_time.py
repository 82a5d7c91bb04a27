"""Time of the train step's update (libvsr_hip_opt.so through optim.Adam) beside torch.optim.Adam, reported and not gated.

  part 1, the x4 SR net's real parameter set (the tensors that receive a gradient from the module alone: 81 of 91; 87 inside VSR) with the
          gradients of one forward_train and backward of (out ** 2).mean() at LR 12 x 20: optim.Adam without and with max_grad_norm; torch.optim.Adam with foreach=False,
          foreach=True and fused=True, each alone and behind torch.nn.utils.clip_grad_norm_.  Every leg owns copies of the parameters
          and gradients.  A round is REPS steps of one leg between two device events (so it holds the gaps the host leaves when it
          cannot enqueue fast enough) and the host clock around the same loop without a wait (what the step costs the host); rounds are
          interleaved over the legs in one process; best round and the spread over rounds are shown.
  part 2, one tensor of 64 Mi elements (1 GiB of p, g, m, v: beyond the 256 MiB Infinity Cache): vsr_opt_adam_f32 (16 B read and 12 B
          written per element) and vsr_opt_grad_norm (4 B read), achieved bytes/s against the HBM peak of 8.0 TB/s (6.3 TB/s measured
          for a float4 copy).

    python tools/opt_time.py [--rounds 5] [--reps 20]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import numpy as np
import torch

from video_super_resolution_amd import SRProjectionModule, optim
from video_super_resolution_amd.weights import fill_module_

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU (no fallback)"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12


def timed(fn, reps):
    """-> (us per step between device events, us per step of host time to enqueue)."""
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
    print(f"  {name:46s} {min(devs):8.1f} us   spread {max(devs) - min(devs):6.1f}   host {min(hosts):7.1f} us{extra}   rounds us: "
          + " ".join(f"{d:.1f}" for d in devs))


# ------------------------------------------------------------------------------------------------ part 1
sr = fill_module_(SRProjectionModule().train(), seed=0, prefix="model.").to(dev)
x = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (8, 3, 12, 20)).astype(np.float32)).to(dev)
(sr(x) ** 2).mean().backward()
live = [p for p in sr.parameters() if p.grad is not None]
n_el = sum(p.numel() for p in live)
norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in live)))
MAX_NORM = norm / 2


def clones():
    ps = [torch.nn.Parameter(p.detach().clone()) for p in live]
    for q, p in zip(ps, live):
        q.grad = p.grad.detach().clone()
    return ps


legs = {}


def add(name, make, clip):
    ps = clones()
    opt = make(ps)

    def step():
        if clip:
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()
    legs[name] = step


add("optim.Adam", lambda ps: optim.Adam(ps), False)
add("optim.Adam(max_grad_norm=)", lambda ps: optim.Adam(ps, max_grad_norm=MAX_NORM), False)
for label, kw in (("foreach=False", dict(foreach=False)), ("foreach=True", dict(foreach=True)), ("fused=True", dict(fused=True))):
    add(f"torch.optim.Adam({label})", lambda ps, kw=kw: torch.optim.Adam(ps, **kw), False)
    add(f"clip_grad_norm_ + torch.optim.Adam({label})", lambda ps, kw=kw: torch.optim.Adam(ps, **kw), True)

print(f"# python tools/opt_time.py --rounds {args.rounds} --reps {args.reps}     (one MI355X, one process)")
print(f"part 1: the x4 SR net, {len(live)} tensors with a gradient, {n_el} elements, gradient norm {norm:.4g} (clipped at half of it); "
      f"{args.rounds} interleaved rounds of {args.reps} steps, best round; us per step between device events, and of host time")
for fn in legs.values():   # warm-up: state, plans, the allocator
    for _ in range(3):
        fn()
rounds = {k: [] for k in legs}
for _ in range(args.rounds):
    for k, fn in legs.items():
        rounds[k].append(timed(fn, args.reps))
for k in legs:
    show(k, rounds[k])

# ------------------------------------------------------------------------------------------------ part 2
N = 64 << 20
big = torch.nn.Parameter(torch.randn(N, device=dev))
big.grad = torch.randn(N, device=dev)
plain = optim.Adam([big])
plain.step()
plan = next(iter(plain._plans.values()))
from video_super_resolution_amd import _lib as L   # noqa: E402
O = L.load_opt()
ctl = torch.empty(2, dtype=torch.float64, device=dev)
ws = torch.empty(int(O.vsr_opt_norm_ws_bytes(plan.host)) // 8, dtype=torch.float64, device=dev)
sc = optim.adam_scalars(1e-3, 0.9, 0.999, 1e-8, 0.0, 2.0)


def adam_only():
    L.check(O.vsr_opt_adam_f32(plan.host, plan.dev.data_ptr(), None, *sc, L.stream()), "opt_adam_f32", lib=O)


def norm_only():
    L.check(O.vsr_opt_grad_norm(plan.host, plan.dev.data_ptr(), 1.0, ctl.data_ptr(), ws.data_ptr(), L.stream()), "opt_grad_norm", lib=O)


print(f"part 2: one tensor of {N} elements ({4 * N * 4 / 2 ** 30:.0f} GiB of p, g, m, v), {plan.n_chunks} workgroups; "
      f"{args.rounds} interleaved rounds of {args.reps} calls, best round")
big_legs = {"vsr_opt_adam_f32 (28 B per element)": (adam_only, 28 * N), "vsr_opt_grad_norm (4 B per element)": (norm_only, 4 * N)}
for fn, _ in big_legs.values():
    fn()
rounds = {k: [] for k in big_legs}
for _ in range(args.rounds):
    for k, (fn, _) in big_legs.items():
        rounds[k].append(timed(fn, args.reps))
for k, (_, nbytes) in big_legs.items():
    rate = nbytes / (min(r[0] for r in rounds[k]) * 1e-6)
    show(k, rounds[k], f"   {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:5.1f} % of a float4 copy")
