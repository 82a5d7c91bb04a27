"""Stream order under adverse timing: every forked path of the package equals its serial evaluation bit for bit when any one stream lags.

The forward forks its work onto side streams (vsr.py `_guidance`, `forward`; trunk_exec.py `HourglassExec._fan_out`, `FlowNet2Exec.run_pairs`)
and `ClipRunner` adds two copy streams.  On an idle GPU at test sizes every kernel takes microseconds, so a consumer that lacks its wait
or a buffer that lacks its `record_stream` still sees finished data.  Here timing is an input (tests/_lag.py): a bounded spin kernel
holds one stream back at chosen moments, so that a missing edge makes the consumer read old -- but sane -- data from valid memory.

Order within every case (`_prepare`, `_lagged`):
  1. want = f(B) under `_lib.serial_streams()` (the runner: an `overlap=False` instance), once per case;
  2. f(A) forked and unlagged, another seed: what lies in freed memory is A's;
  3. f(B) forked under the policy (`waiter`, `waited`, every `pre:<k>` of the case's pool);
  4. bit equality of every tap in stage order (the first that differs names the stage), all lags held, the hooked forks and joins at
     least the number the code has for the configuration (`min_waits`, derived at each case below).
Nothing is poisoned: stale data is a previous call's data.

The lag of a case is twice the host time of its warm serial call (at least 5 ms); the lags of one call may not pass 2 s ("lag budget").

Independence: the lag tells nothing when the lagged stream and the one that races it share a hardware queue.  Before a case runs, every
ordered pair of its pool is probed (`_lag.probe_independence`); a serialised pair that the package forks or joins fails the case.  A
process here has four hardware queues by default and the cases use up to six streams, so the cases run in ONE fresh child process
started with GPU_MAX_HW_QUEUES=16 (`MODE = "child"`; chosen by what the probe showed on an MI355X, LAB_NOTES.md "Stream-order tests"):
the child writes one JSON of per-case results, the parametrised tests read it.  `MODE = "inprocess"` runs the same functions here.
Sixteen queues do not make every pair independent either (which pool stream lands on which queue is the runtime's choice), so before a
case takes its streams `_align` tries the pool's next ones and leaves the case a set that the probe found clean.
"""
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "2")   # (as tests/conftest.py: read at library load, and the child has no conftest)
os.environ.setdefault("MIOPEN_DEBUG_ENABLE_AI_IMMED_MODE_FALLBACK", "0")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "2")
import copy
import json
import subprocess
import sys
import tempfile
import time
import traceback
from collections import OrderedDict

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _lag as G  # noqa: E402

pytestmark = pytest.mark.gpu

MODE = os.environ.get("VSR_LAG_MODE", "child")   # "child" | "inprocess" (see the module docstring)
CHILD_QUEUES = "16"
CHILD_TIMEOUT_S = 900
# Intervals in which a lag may have ended because the code makes a host wait by design, by the site that placed the lag.  None in a
# warm call.  The cold cases (D) rebuild the packs and the executors inside the call, and a rebuild waits on the host: the SR packers read
# every PReLU slope as a Python float (sr.py:161-182, `float(...weight.detach())`: the kernels take it by value), OSVOSExec reads the fuse
# bias the same way (trunk_exec.py:624), and the rebuilt packs need new memory from the driver while the old ones are still referenced.
#   vsr.py:334  `s_sr.wait_stream(main)`: the interval holds `precompute_shared`, which rebuilds the SR packs on s_sr;
#   vsr.py:196  `s_vos.wait_stream(main)`: the interval holds `_depth_exec.get()`, `_vos_exec.get()` and `_flow_exec.get()`.
_COLD_REBUILDS = ("video_super_resolution_amd/vsr.py:334", "video_super_resolution_amd/vsr.py:196")
EXEMPT = {"D": _COLD_REBUILDS}


def _exempt(cid):
    return EXEMPT.get(cid.split("-")[0], ())


# ================================================================================================ the toy: what the harness is for
def _toy(inp, variant, streams, serial=False):
    """Producer on stream a, consumer on stream b, plain element-wise torch ops on small tensors.  `variant`: correct | nojoin | nofork |
    norecord (the producer's tensor is dropped on the host and a same-sized one allocated and overwritten on the producing stream; without
    `record_stream` the allocator hands out the block the consumer may not have read yet).  Only old values of live allocations are read."""
    import torch
    main = torch.cuda.current_stream()
    a, b = (main, main) if serial else streams
    x = inp * 0.5 + 1.0                      # on main: what the fork orders
    if variant != "nofork":
        a.wait_stream(main)
    with torch.cuda.stream(a):
        t = x * 3.0 - 2.0                    # the producer
        if variant != "norecord":
            t.record_stream(b)
    x.record_stream(a)
    _host_work(a)
    if variant != "nojoin":
        b.wait_stream(a)
    with torch.cuda.stream(b):
        y = t + 7.0                          # the consumer
        y.record_stream(main)
    _host_work(b)
    del t
    with torch.cuda.stream(a):
        us = [torch.empty_like(x) for _ in range(8)]   # same size, the producing stream: one is the block of `t` if nothing holds it
        for u in us:
            u.fill_(-5.0)
            u.record_stream(main)
    main.wait_stream(b)
    main.wait_stream(a)
    return OrderedDict(y=y.clone(), u=us[0].clone())


def _host_work(stream, n=64):
    """A fixed stretch of host time between two launches, as the package has between its own (Python, argument marshalling): natural
    timing then lets a microsecond kernel finish before the next launch, which is how a missing edge passes unlagged.  No wait: the
    answers are not looked at."""
    for _ in range(n):
        stream.query()


class _ToyCase:
    n_pool, min_waits = 3, 2

    def __init__(self, variant):
        import torch
        self.variant = variant
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        rs = np.random.RandomState(3)
        self.inp = {k: torch.from_numpy(rs.uniform(0, 255, 1 << 14).astype(np.float32)).cuda() for k in "AB"}
        self.min_waits = 4 - (variant in ("nojoin", "nofork"))

    def pool(self):
        import torch
        return [torch.cuda.current_stream()] + self.streams

    def serial(self, k):
        return _toy(self.inp[k], "correct", self.streams, serial=True)

    def forked(self, k):
        return _toy(self.inp[k], self.variant, self.streams)


# ================================================================================================ models
_MASTERS, _MODELS = {}, {}


def _master(scale):
    """The seeded synthetic weights of tests/conftest.py `cpu_vsr`; x2 / x3: its guidance trunks and a seeded SR net of that scale."""
    import torch
    from video_super_resolution_amd import VSR
    from video_super_resolution_amd.weights import fill_module_
    if 4 not in _MASTERS:
        torch.manual_seed(0)
        _MASTERS[4] = fill_module_(VSR().eval(), seed=0)
    if scale not in _MASTERS:
        m = VSR(upscale_factor=scale).eval()
        m.load_state_dict({k: v for k, v in _MASTERS[4].state_dict().items() if not k.startswith("model.")}, strict=False)
        fill_module_(m.model, seed=0, prefix="model.")
        _MASTERS[scale] = m
    return _MASTERS[scale]


def _model(scale, precision, own=None):
    """One model per (scale, precision) for all the cases that only flip switches; `own`: a copy for a case that changes weights."""
    key = (scale, precision, own)
    if key not in _MODELS:
        m = copy.deepcopy(_master(scale)).cuda().eval()
        m.precision = m.model.precision = precision
        _MODELS[key] = m
    return _MODELS[key]


def _frames(seed, n, h, w):
    """[n,h,w,3] float32 frames of a smooth scene that moves (the trunks see structure), as tests/test_gpu_weight_freshness.py `window`."""
    import torch
    from scipy.ndimage import gaussian_filter
    base = gaussian_filter(np.random.RandomState(seed).uniform(0, 255, size=(h + 16, w + 32, 3)).astype(np.float32), sigma=(2, 2, 0))
    return torch.from_numpy(np.stack([np.floor(base[k:k + h, 2 * k:2 * k + w]) for k in range(n)]).astype(np.float32)).cuda()


SEEDS = {"A": 160, "B": 161}


# ================================================================================================ A. FlowNet2Exec.run_pairs
class _FlowCase:
    """run_pairs forks FlowNetSD onto `_sd_stream` (trunk_exec.py `side.wait_stream(main)`) and joins before fusion_input
    (`main.wait_stream(side)`): 2 hooked waits.  Pool: main, the FlowNetSD stream."""
    n_pool, min_waits = 2, 2

    def __init__(self, n, h, w):
        from video_super_resolution_amd.trunk_exec import FlowNet2Exec
        self.ex = FlowNet2Exec(_model(4, "fp16").FlowModule.net)
        self.frames = {k: _frames(s, n, h, w) for k, s in SEEDS.items()}
        self.pairs = [(2 * i, 2 * i + 1) for i in range(n // 2)]

    def pool(self):
        import torch
        return [torch.cuda.current_stream(), self.ex._sd_stream(self.frames["A"].device)]

    def forked(self, k):
        return OrderedDict(flow=self.ex.run_pairs(self.frames[k], self.pairs).clone())

    def serial(self, k):
        from video_super_resolution_amd import _lib as L
        with L.serial_streams():
            return self.forked(k)


# ================================================================================================ B. HourglassExec, concurrent
class _HourglassCase:
    """`_fan_out` forks the first arm of a level onto that level's side stream and joins at the sum: 2 hooked waits per level that fans
    out.  depth.py nests four levels (_L1.._L4: levels 0..3); with the fused front the program's level 0 is evaluated by `_run_fused_front`
    without a fan-out, so levels 1..3 fork: 6 waits; without it 8.  Pool: main, then the side streams of the levels that fork."""

    def __init__(self, fused_front, n, h, w):
        from video_super_resolution_amd.trunk_exec import HourglassExec
        self.ex = HourglassExec(_model(4, "fp16").DepthModule.model.netG)
        self.ex.concurrent, self.ex.fused_front = True, fused_front
        self.levels = (1, 2, 3) if fused_front else (0, 1, 2, 3)
        self.n_pool, self.min_waits = 1 + len(self.levels), 2 * len(self.levels)
        self.frames = {k: _frames(s, n, h, w) for k, s in SEEDS.items()}

    def pool(self):
        import torch
        dev = self.frames["A"].device
        return [torch.cuda.current_stream()] + [self.ex._side(dev, lv) for lv in self.levels]

    def forked(self, k):
        return OrderedDict(depth=self.ex(self.frames[k]).clone())

    def serial(self, k):
        from video_super_resolution_amd import _lib as L
        with L.serial_streams():
            return self.forked(k)


# ================================================================================================ C - F. VSR.forward
TAPS = ("pass1_input", "pass1_decimated", "vos_mask", "pass2_input")   # in stage order; then the output frame


class _VsrCase:
    """One VSR.forward call at 66 x 70.  Hooked waits, from vsr.py and trunk_exec.py, fp16 configuration: `forward` forks the shared planes
    onto s_sr and joins them behind pass 1's guidance (2); `_guidance`, twice: forks s_depth and s_vos (2), joins them (2), and FlowNet2's
    run_pairs forks and joins FlowNetSD inside it (2): 2 + 2 x 6 = 14; early_planes >= 3 (x4 only) adds `wait_event(ev_packed)`: 15.
    float32 configuration with f32_streams: the stock FlowNet2 forks nothing: 2 + 2 x 4 = 10.
    Pool: main, the two side streams, and in the fp16 configuration the FlowNetSD stream."""

    def __init__(self, scale=4, precision="fp16", recurrent=False, own=None, **switches):
        self.scale, self.precision, self.recurrent, self.own, self.switches = scale, precision, recurrent, own, switches
        self.m = _model(scale, precision, own)
        early3 = scale == 4 and precision == "fp16" and switches.get("early_planes", self.m.early_planes) >= 3
        self.min_waits = (14 + early3) if precision == "fp16" else 10
        self.n_pool = 4 if precision == "fp16" else 3
        self.data = {k: _frames(s, 3, 66, 70) for k, s in SEEDS.items()}
        self.est = {}

    def _switched(self):
        m, sw = self.m, self.switches

        class ctx:
            def __enter__(self_):
                self_.old = {k: getattr(m, k) for k in sw}
                for k, v in sw.items():
                    setattr(m, k, v)

            def __exit__(self_, *exc):
                for k, v in self_.old.items():
                    setattr(m, k, v)
                m.plane_taps = None
        return ctx()

    def pool(self):
        import torch
        dev = self.data["A"].device
        p = [torch.cuda.current_stream()] + list(self.m._side_streams(dev))
        if self.precision == "fp16" and self.n_pool == 4:
            p.append(self.m._flow_exec.get()._sd_stream(dev))
        return p

    def _estimate(self, k):
        """The recurrent call's `estimated_image`: the serial first call's frame of the same window, computed once."""
        if k not in self.est:
            from video_super_resolution_amd import _lib as L
            with L.serial_streams(), self._switched():
                self.est[k] = self.m(self.data[k], None, None, None, train=False)[0].clone()
        return self.est[k]

    def call(self, m, k):
        est = self._estimate(k) if self.recurrent else None
        m.plane_taps = {}
        out, _ = m(self.data[k], None, None, est, train=False)
        res = OrderedDict((t, m.plane_taps[t]) for t in TAPS)
        res["output"] = out.clone()
        m.plane_taps = None
        return res

    def forked(self, k):
        with self._switched():
            return self.call(self.m, k)

    def serial(self, k):
        from video_super_resolution_amd import _lib as L
        if self.recurrent:
            self._estimate(k)
        with L.serial_streams():
            return self.forked(k)


class _ColdVsrCase(_VsrCase):
    """D.  As C, but cold: between step 2 and step 3 every SR weight and one weight of each trunk is multiplied in place, so the packs, the
    constant maps and the three trunk executors are rebuilt inside the lagged call, on whichever stream touches them first, while the
    previous packs still lie in memory.  `want` comes from a deep copy that carries the changed weights.  The rebuilt FlowNet2 executor
    takes a new FlowNetSD stream inside the call, so the pool is main and the two side streams; the FlowNetSD stream is lagged by
    `waiter` and `waited`.  The lag is twice the host time of the COLD serial call (the copy's), which is what the host takes here."""
    cold = True

    def __init__(self, **kw):
        super().__init__(own="cold-%s-%s" % (kw.get("early_planes"), kw.get("recurrent")), **kw)
        self.n_pool = 3

    def mutate(self, m=None):
        import torch
        m = self.m if m is None else m
        with torch.no_grad():
            for p in m.model.parameters():
                p.mul_(1.01)
            for net in (m.FlowModule.net, m.DepthModule.model.netG, m.VOSModule.net):
                convs = [p for p in net.parameters() if p.dim() == 4]
                convs[len(convs) // 2].mul_(1.01)

    def cold_want(self, k):
        """(want, host ms) from a deep copy that gets the change `mutate()` will make (the same product of the same values: the same
        bits): its first call, serial, is as cold as the lagged one will be."""
        import time
        import torch
        from video_super_resolution_amd import _lib as L
        twin = copy.deepcopy(self.m)
        self.mutate(twin)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with L.serial_streams(), self._switched():
            for kk, v in self.switches.items():
                setattr(twin, kk, v)
            want = self.call(twin, k)
        torch.cuda.synchronize()
        return want, (time.perf_counter() - t0) * 1e3


class _StreamingCase(_VsrCase):
    """E.  temporal_cache = True: three consecutive windows of one clip tensor, the whole sequence is the lagged call; want is the
    per-window serial evaluation without the cache.  Every window forks and joins as in C (cached frames shrink the batches, not the
    forks): 3 x 14 = 42 hooked waits."""

    def __init__(self):
        super().__init__(own="streaming")
        self.min_waits = 42
        self.data = {k: _frames(s, 5, 66, 70) for k, s in SEEDS.items()}

    def _sequence(self, k, cache):
        m, clip = self.m, self.data[k]
        m.temporal_cache = cache
        m.reset_temporal_cache()
        try:
            est, res = None, OrderedDict()
            for t in range(3):
                m.plane_taps = {}
                est, _ = m(clip[t:t + 3], None, None, est, train=False)
                for tap in TAPS:
                    res[f"window{t}.{tap}"] = m.plane_taps[tap]
                res[f"window{t}.output"] = est.clone()
            return res
        finally:
            m.temporal_cache, m.plane_taps = False, None
            m.reset_temporal_cache()

    def forked(self, k):
        return self._sequence(k, True)

    def serial(self, k):
        from video_super_resolution_amd import _lib as L
        with L.serial_streams():
            return self._sequence(k, False)


# ================================================================================================ G. ClipRunner
CLIP_T, CLIP_HW, CLIP_S, CLIP_FMT = 7, 256, 4, "nv12"   # LR 64 x 64 -> 256 x 256 (tests/test_gpu_metric.py, tests/test_gpu_msssim.py), nv12
CLIP_CONFIGS = {
    "plain": {},
    "msssim": dict(score="y", multiscale=True, baseline="bicubic", decimate="bicubic"),
    "warp-scene": dict(score="rgb", temporal="warp", scene="sad"),
}


def _light_model():
    """A stand-in for VSR with the interface ClipRunner uses, whose forward is a dozen plain torch launches on the current stream: the
    window's three frames and the fed-back estimate all reach every output pixel (a stale ring slot or a stale estimate shows), and the
    same launches in the same order give the same bits forked and serial.  It forks nothing itself, so every hooked wait of a run is
    one of the runner's own (or of `truth_flows`, which uses the real FlowNet2 of the fp16 model through `FlowModule`)."""
    import torch

    class Light(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.FlowModule = _model(4, "fp16").FlowModule
            self.model = torch.nn.Module()
            self.model.upscale_factor = self.upscale_factor = CLIP_S
            self.precision = "fp16"

        def _fast(self):
            return True

        def forward(self, x, target, high_frames, est, train=False):
            S = self.upscale_factor
            lr = 0.25 * x[0] + 0.5 * x[1] + 0.25 * x[2]
            if est is not None:
                e = est.detach().float()
                e = e[0] if e.dim() == 4 else e
                if e.shape[0] != lr.shape[0]:
                    e = e[::S, ::S]                  # (the nearest resize VSR.forward makes)
                lr = 0.75 * lr + 0.25 * e
            out = lr.repeat_interleave(S, 0).repeat_interleave(S, 1)
            return out.unsqueeze(0).contiguous(), None
    return Light().cuda().eval()


class _ClipCase:
    """G.  ClipRunner(overlap=True) over T = 7 frames, twice on the same object: every input, output and ring slot and both truth buffers
    are reused at least twice.  A two-scene clip (4 + 3 frames): scene="sad" finds one cut.  Compared with the `overlap=False` runner:
    output bytes, `metrics`, `cuts`.  Hooked waits of one run, from clip_runner.py: `_upload` waits on `uploaded` for every frame (7) and
    on `converted` from the third frame on (5); `_write_out` waits on `ready` for every window (5) and on `copied` from the third window
    on (3): 20 of the runner's own.

    Which model the runner drives decides whether `waiter` and `waited` can run at all.  With the float32 VSR a warm serial run takes
    258-312 ms of host time (measured on an MI355X), the lag is 516-624 ms, and one run has 70 hooked waits (20 + 5 windows x 10 of the
    model's): 36-44 s of lags against the 2 s a call may spend -- the rule for the lag and the rule for the budget exclude each other.
    Neither rule is bent.  What G is about is the RUNNER's order (s_in, main, s_out, the slots, the ring, the truth buffers, the four
    events); the model's own forks are C to F under every policy.  So:
      `light=True`   the runner drives `_light_model()` under every policy: 20 hooked waits (28 with temporal="warp": four `truth_flows` calls
                     fork and join FlowNetSD inside the real FlowNet2Exec), a run of a few milliseconds, lags that fit.
                     Pool: main, s_in, s_out (and the truth-flow executor's FlowNetSD stream with temporal="warp").
      `light=False`  the runner drives the float32 VSR under every `pre:<k>` turn (one lag of 0.5-0.6 s on each stream): 70 hooked
                     waits.  Pool: main, s_in, s_out and the model's two side streams.  `waiter` and `waited` are not parametrised
                     here: by the arithmetic above they can only answer "lag budget"."""

    def __init__(self, config, light):
        import torch
        import _scene_ref as R
        from video_super_resolution_amd import driver
        self.kw, self.light = CLIP_CONFIGS[config], light
        self.warp = self.kw.get("temporal") is not None
        self.m = _light_model() if light else _model(4, "fp32", own="clip-" + config)
        self.n_pool = (3 + self.warp) if light else 5
        self.min_waits = (20 + 8 * self.warp) if light else 70
        H = W = CLIP_HW
        self.clip = {}
        for k, s in SEEDS.items():
            video = np.concatenate([R.scene_video(4, H, W, s), R.scene_video(3, H, W, s + 10, invert=True)])
            self.clip[k] = driver.frames_to_yuv(torch.from_numpy(video).cuda().float(), CLIP_FMT).cpu().numpy()
        mk = lambda overlap: driver.ClipRunner(self.m, (H, W), CLIP_FMT, CLIP_FMT, scale_down=CLIP_S, overlap=overlap, **self.kw)   # noqa: E731
        self.over, self.plain = mk(True), mk(False)

    def pool(self):
        import torch
        p = [torch.cuda.current_stream(), self.over._s_in, self.over._s_out]
        if not self.light:
            return p + list(self.m._side_streams(self.over.device))
        if self.warp:
            from video_super_resolution_amd import frames
            p.append(frames._truth_flow_exec[self.m].get()._sd_stream(self.over.device))
        return p

    @staticmethod
    def _result(r, out):
        res = OrderedDict(bytes=out.copy())
        for k, v in sorted((r.metrics or {}).items()):
            res["metrics." + k] = np.array(v)
        if r.cuts is not None:
            res["cuts"] = np.array(r.cuts)
        return res

    def forked(self, k):
        return self._result(self.over, self.over.run(self.clip[k]))

    def serial(self, k):
        from video_super_resolution_amd import _lib as L
        with L.serial_streams():
            return self._result(self.plain, self.plain.run(self.clip[k]))


# ================================================================================================ the cases
def _cases():
    """id -> (factory, streams in the pool, side streams the case may take from torch's pool when it is built and first runs forked)."""
    c = OrderedDict()
    for v in ("correct", "nojoin", "nofork", "norecord"):
        c["toy-" + v] = (lambda v=v: _ToyCase(v), 3, 2)
    c["A-4x64x128"] = (lambda: _FlowCase(4, 64, 128), 2, 1)
    c["A-2x64x64"] = (lambda: _FlowCase(2, 64, 64), 2, 1)
    for front in (True, False):
        for n, h, w in ((2, 70, 90), (1, 64, 96)):
            c[f"B-{'front' if front else 'nofront'}-{n}x{h}x{w}"] = (lambda front=front, n=n, h=h, w=w: _HourglassCase(front, n, h, w), 4 if front else 5, 3 if front else 4)
    for rec in (False, True):
        call = "recurrent" if rec else "first"
        for early in (0, 1, 2, 3):
            c[f"C-x4-early{early}-{call}"] = (lambda rec=rec, early=early: _VsrCase(4, "fp16", rec, early_planes=early), 4, 3)
        for scale in (2, 3):
            c[f"C-x{scale}-{call}"] = (lambda rec=rec, scale=scale: _VsrCase(scale, "fp16", rec), 4, 3)
        c[f"C-x4-notail-{call}"] = (lambda rec=rec: _VsrCase(4, "fp16", rec, share_tail=False), 4, 3)
        for early in (1, 3):
            c[f"D-x4-early{early}-{call}"] = (lambda rec=rec, early=early: _ColdVsrCase(scale=4, precision="fp16", recurrent=rec, early_planes=early), 3, 3)
        c[f"F-fp32-{call}"] = (lambda rec=rec: _VsrCase(4, "fp32", rec, f32_streams=True), 3, 2)
    c["E-streaming"] = (lambda: _StreamingCase(), 4, 3)
    for cfg in CLIP_CONFIGS:
        warp = CLIP_CONFIGS[cfg].get("temporal") is not None
        c["G-" + cfg] = (lambda cfg=cfg: _ClipCase(cfg, light=True), 3 + warp, 2 + warp)
        c["Gvsr-" + cfg] = (lambda cfg=cfg: _ClipCase(cfg, light=False), 5, 4)
    return c


CASES = _cases()
TOY_BROKEN = ("toy-nojoin", "toy-nofork", "toy-norecord")
PARAMS = [(cid, pol) for cid, (_, n_pool, _) in CASES.items() if cid not in TOY_BROKEN for pol in G.policies(n_pool)
          if not (cid.startswith("Gvsr-") and not pol.startswith("pre:"))]   # (see _ClipCase)
PARAMS += [(cid, "any") for cid in TOY_BROKEN]


# ================================================================================================ the driver
_STATE, _PROBES = {}, {}


def _same(a, b):
    import torch
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _first_difference(got, want):
    for name in want:
        if name not in got:
            return f"{name}: missing"
        if not _same(got[name], want[name]):
            a, b = got[name], want[name]
            if a.shape != b.shape:
                return f"{name}: shape {tuple(a.shape)} != {tuple(b.shape)}"
            a, b = (np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64) for t in (a, b))
            return f"{name}: {int((a != b).sum())} of {a.size} values differ, max |diff| {np.nanmax(np.abs(a - b)):.6g}"
    return None


def _align(n):
    """torch hands out side streams round-robin from a pool of 32 per device, and the runtime spreads them over the process's hardware
    queues in a way the test cannot choose: of two streams a case is given, one may share a queue with the other or with main.  So before
    a case takes its `n` streams, the next n of the pool are tried (`probe_independence`, main included); a clean set is put back by taking
    the pool's other 32 - n, so that the case is handed exactly those; an unclean one is left behind and the next n are tried.  This only
    arranges WHICH pool streams the package gets; whether they are independent is still decided by the probe in `_prepare`."""
    import torch
    main = torch.cuda.current_stream()
    for _ in range(12):
        cands = [torch.cuda.Stream() for _ in range(n)]
        if all(G.probe_independence([main] + cands, lag_ms=10.0).values()):
            for _ in range(32 - n):
                torch.cuda.Stream()
            return True
    return False


def _prepare(cid):
    """Steps 1 and the bookkeeping every policy of a case shares: want, the warm host time, the hooks of an unlagged forked run, the probe."""
    import torch
    if cid in _STATE:
        return _STATE[cid]
    _align(CASES[cid][2])
    case = CASES[cid][0]()
    sync = torch.cuda.synchronize
    case.serial("B")                                  # warm: packs, constant maps, the allocator
    want = case.serial("B")
    sync()
    host_ms = G.warm_host_ms(lambda: case.serial("B"), sync)
    case.forked("A")                                  # warm the forked order too: its streams exist from here on
    sync()
    pool = case.pool()
    assert len(pool) == case.n_pool == CASES[cid][1], (len(pool), case.n_pool)
    assert len({G.handle(s) for s in pool}) == len(pool), "two streams of the pool are one"
    with G.Lagger("none", 0.0, pool=pool, exempt=_exempt(cid)) as count:
        got = case.forked("B")
    sync()
    key = tuple(G.handle(s) for s in pool)
    if key not in _PROBES:
        _PROBES[key] = G.probe_independence(pool)
    st = dict(case=case, want=want, host_ms=host_ms, pool=pool, hooks=count.waits, forked=count.pairs(),
              unlagged=_first_difference(got, want), serialised=G.serialised_pairs(_PROBES[key], pool, count.pairs()),
              probe={f"{i}>{j}": ok for (i, j), ok in _PROBES[key].items()})
    _STATE[cid] = st
    return st


def _lagged(st, cid, policy):
    """Steps 2 to 4 under one policy -> (message or None, info)."""
    import torch
    case, want = st["case"], st["want"]
    host_ms = st["host_ms"]
    cold = getattr(case, "cold", False)
    if cold:   # (before step 2, so that what lies in freed memory at step 3 is still A's)
        want, host_ms = case.cold_want("B")
    case.forked("A")
    torch.cuda.synchronize()
    if cold:
        case.mutate()
    lag_ms = G.lag_for(host_ms)
    runs, msgs = [], []
    if not policy.startswith("pre:") and st["hooks"] * lag_ms > G.BUDGET_MS:   # (every hooked wait gets a lag: known before the run)
        return (f"lag budget: {st['hooks']} hooked waits x {lag_ms:.1f} ms = {st['hooks'] * lag_ms:.0f} ms of lags in one call, over "
                f"{G.BUDGET_MS:.0f} ms"), dict(host_ms=round(host_ms, 2), lag_ms=round(lag_ms, 2), hooks=st["hooks"], runs=[])
    for again in range(2 if cid.startswith("G") else 1):   # (the runner: a second run of the same object)
        lg = G.Lagger(policy, lag_ms, pool=st["pool"], exempt=_exempt(cid))
        try:
            with lg:
                got = case.forked("B")
            torch.cuda.synchronize()
        except G.LagBudget as e:
            torch.cuda.synchronize()
            msgs.append(str(e))
            runs.append(dict(lags=len(lg.lags), spent_ms=lg.spent_ms, held=None, waits=lg.waits))
            break
        diff = _first_difference(got, want)
        runs.append(dict(lags=len(lg.lags), spent_ms=lg.spent_ms, held=all(r["held"] for r in lg.lags), waits=lg.waits))
        if diff is not None:
            msgs.append(f"forked under {policy} differs from serial at {diff}\n{lg.report()}")
        msgs += lg.failures
        if lg.waits < case.min_waits:
            msgs.append(f"{lg.waits} hooked forks and joins, the code has {case.min_waits}: the configuration ran serial?\n{lg.report()}")
    info = dict(host_ms=round(host_ms, 2), lag_ms=round(lag_ms, 2), hooks=st["hooks"], runs=runs)
    return ("\n".join(msgs) if msgs else None), info


def run_case(cid, policy):
    """-> dict(ok, message, info): one (case, policy) of PARAMS."""
    try:
        st = _prepare(cid)
        info = dict(host_ms=round(st["host_ms"], 2), hooks=st["hooks"], serialised=st["serialised"], unlagged_equal=st["unlagged"] is None)
        if st["serialised"]:
            return dict(ok=False, info=info, message=f"streams {st['serialised']} of the pool are forked or joined by the package but share a "
                        f"hardware queue (probe: {st['probe']}): a lag on one holds the other back")
        if cid in TOY_BROKEN:
            caught = []
            for pol in G.policies(CASES[cid][1]):
                msg, run_info = _lagged(st, cid, pol)
                if msg is not None and "differs from serial" in msg:
                    caught.append(pol)
                info[pol] = run_info["runs"]
            info["caught_under"] = caught
            msgs = []
            if not caught:
                msgs.append("the broken variant equals the serial result under every policy: the harness cannot see what it is for")
            if st["unlagged"] is not None:
                msgs.append(f"the broken variant already differs unlagged ({st['unlagged']}): it does not show that the harness is needed")
            return dict(ok=not msgs, info=info, message="\n".join(msgs))
        if st["unlagged"] is not None:
            return dict(ok=False, info=info, message=f"forked and UNLAGGED differs from serial at {st['unlagged']}")
        msg, run_info = _lagged(st, cid, policy)
        info.update(run_info)
        return dict(ok=msg is None, info=info, message=msg or "")
    except Exception:
        return dict(ok=False, info={}, message=traceback.format_exc())


# ================================================================================================ the child
def _child_main(argv):
    out, ids = argv[0], argv[1:]
    import torch
    be = G.TorchBackend()
    results = {"_calibration": dict(cycles_per_ms=be.cycles_per_ms(), queues=os.environ.get("GPU_MAX_HW_QUEUES"), device=torch.cuda.get_device_name(0))}
    last = None
    for item in ids:
        cid, policy = item.split("|")
        if last is not None and last != cid:
            _STATE.pop(last, None)        # (a case's tensors are not needed once its policies are through, nor is a model of its own)
            for key in [k for k in _MODELS if k[2] is not None]:
                del _MODELS[key]
        last = cid
        t0 = time.perf_counter()
        results[item] = run_case(cid, policy)
        results[item]["info"]["seconds"] = round(time.perf_counter() - t0, 2)   # (a case's first policy pays for its build, warm-up and probe)
        print(f"{item:<36} {'ok' if results[item]['ok'] else 'FAILED'} {json.dumps(results[item]['info'])}", flush=True)
        with open(out + ".tmp", "w") as f:
            json.dump(results, f)
        os.replace(out + ".tmp", out)
    return 0


_RESULTS = {}


def _child_results(wanted):
    """The per-case results of ONE child process for every selected case of this file (started with subprocess; nothing is exec'd)."""
    if "done" not in _RESULTS:
        d = tempfile.mkdtemp(prefix="vsr_lag_")
        out = os.path.join(d, "results.json")
        env = dict(os.environ, GPU_MAX_HW_QUEUES=CHILD_QUEUES)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), out] + wanted, env=env, cwd=ROOT, timeout=CHILD_TIMEOUT_S,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            _RESULTS["log"], _RESULTS["rc"] = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:
            _RESULTS["log"], _RESULTS["rc"] = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), "timeout"
        _RESULTS["res"] = json.load(open(out)) if os.path.exists(out) else {}
        _RESULTS["done"] = True
        print(_RESULTS["log"][-20000:])
    return _RESULTS


@pytest.fixture(scope="module")
def selected(request):
    ids = []
    for it in request.session.items:
        if getattr(getattr(it, "module", None), "__name__", None) == __name__ and hasattr(it, "callspec") and "cid" in it.callspec.params:
            ids.append(f"{it.callspec.params['cid']}|{it.callspec.params['policy']}")
    return ids


@pytest.mark.parametrize("cid,policy", PARAMS, ids=[f"{c}-{p}" for c, p in PARAMS])
def test_forked_equals_serial_when_a_stream_lags(selected, cid, policy):
    """One case under one policy (module docstring).  The toy's broken variants run under `any`: each differs from the serial result under
    at least one policy and equals it unlagged -- which is what makes the harness necessary."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if MODE == "child":
        r = _child_results(selected)
        res = r["res"].get(f"{cid}|{policy}")
        assert res is not None, f"the child process (exit {r['rc']}) left no result for this case; the end of its output:\n{r['log'][-3000:]}"
    else:
        res = run_case(cid, policy)
    print(f"[{cid} {policy}] {json.dumps(res['info'])}")
    assert res["ok"], res["message"]


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1:]))
