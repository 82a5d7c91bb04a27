"""Timing as an input of a stream-order test: `Lagger` holds one stream back with a bounded spin kernel at the ordering points of a
forked call, so that a consumer that lacks its wait, or a buffer that lacks its `record_stream`, reads old data from valid memory and
the result differs from the serial evaluation -- deterministically, not "now and then".

Inside `with Lagger(policy, lag_ms, pool=...)` four methods are wrapped (class attributes, restored on exit, also after an exception):

    Stream.wait_stream(other)   waiter = the stream, waited = `other`
    Stream.wait_event(event)    waiter = the stream, waited = the stream the event was last recorded on (if that record was seen)
    Event.record(stream=None)   an ordering point (remembers the event's stream); never lagged
    Event.synchronize()         an ordering point (a host wait the code makes itself); never lagged

Only the OUTERMOST wrapped call counts: `wait_stream` is `wait_event(record_event())` inside, and the harness's own events and sleeps
run under the same guard.  Streams are told apart by their `.cuda_stream` handle (`torch.cuda.current_stream()` builds a new object per call).

Policies, each one whole-call run:
    "none"     nothing is lagged: the hooks are only counted and listed
    "waiter"   after every hooked wait has been enqueued, a lag on the stream that waits
    "waited"   after every hooked wait, a lag on the stream that was waited on
    "pre:<k>"  before the call starts, one lag on stream k of `pool`

A lag is `backend.sleep(stream, ms)` (torch.cuda._sleep with measured cycles per millisecond).  Its length is the caller's: `lag_for(host_ms)`
= max(5 ms, twice the warm serial call's host time); the sum of the lags of one Lagger may not pass 2 s: the one that would raises
`LagBudget` ("lag budget"), nothing is shortened.  After each sleep an event is recorded on the lagged stream; on entry to the next hooked
call (and on a clean exit) `query()` must still be False -- True means the lag had ended before the host reached the next ordering point and
tested nothing: `failures` gets "lag did not hold at <file:line>" unless the site that placed the lag is in `exempt` (an interval with a
host wait the code makes by design).

Everything the GPU does goes through `backend`; tests/test_lag_helper.py drives the same code with fake streams, events and a fake sleep.
"""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_MS = 5.0
BUDGET_MS = 2000.0
POLICIES = ("none", "waiter", "waited")
_HERE = os.path.abspath(__file__)


class LagBudget(AssertionError):
    pass


def lag_for(host_ms: float) -> float:
    """The lag of a case whose warm serial call takes `host_ms` of host time: twice that, at least the floor."""
    return max(FLOOR_MS, 2.0 * float(host_ms))


def policies(n_pool: int):
    """Every policy a case with a pool of `n_pool` streams runs under: each stream takes one `pre:<k>` turn, main (k = 0) included."""
    return ["waiter", "waited"] + [f"pre:{k}" for k in range(n_pool)]


def parse_policy(policy: str, n_pool: int):
    """-> (kind, k): kind in none / waiter / waited / pre; k the pool index of a pre:<k>, else None."""
    if policy in POLICIES:
        return policy, None
    if isinstance(policy, str) and policy.startswith("pre:"):
        try:
            k = int(policy[4:])
        except ValueError:
            k = -1
        if 0 <= k < n_pool:
            return "pre", k
        raise ValueError(f"policy {policy!r}: the pool has streams 0..{n_pool - 1}")
    raise ValueError(f"unknown policy {policy!r}")


def handle(stream):
    return int(stream.cuda_stream)


def _site(skip_prefixes):
    """file:line of the nearest caller outside this file and outside `skip_prefixes` (the framework), relative to the repository."""
    f = sys._getframe(1)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE and not fn.startswith(skip_prefixes):
            rel = os.path.relpath(fn, ROOT) if fn.startswith(ROOT + os.sep) else fn
            return f"{rel}:{f.f_lineno}"
        f = f.f_back
    return "?"


class TorchBackend:
    """The real thing: torch.cuda streams and events, torch.cuda._sleep with cycles per millisecond measured once per process."""
    _cycles_per_ms = None

    def __init__(self):
        import torch
        assert hasattr(torch.cuda, "_sleep"), "torch.cuda._sleep is missing from this torch: the lag tests need it"
        self.torch = torch
        self.Stream, self.Event = torch.cuda.Stream, torch.cuda.Event
        self.skip = (os.path.dirname(os.path.abspath(torch.__file__)),)

    def current_stream(self):
        return self.torch.cuda.current_stream()

    def new_event(self):
        return self.torch.cuda.Event()

    def cycles_per_ms(self) -> float:
        """Two timed events around a short sleep; the second of two measurements (the first pays the kernel's load)."""
        if TorchBackend._cycles_per_ms is None:
            t = self.torch
            cycles, rate = 2_000_000, None
            for _ in range(2):
                a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                t.cuda.synchronize()
                a.record()
                t.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                rate = cycles / a.elapsed_time(b)
            assert rate > 0
            TorchBackend._cycles_per_ms = rate
        return TorchBackend._cycles_per_ms

    def sleep(self, stream, ms: float) -> None:
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(int(ms * self.cycles_per_ms()))


class Lagger:
    def __init__(self, policy: str, lag_ms: float, pool=(), backend=None, only=None, exempt=(), budget_ms: float = BUDGET_MS):
        self.backend = backend if backend is not None else TorchBackend()
        self.pool = list(pool)
        self.kind, self.pre_k = parse_policy(policy, len(self.pool))
        self.policy = policy
        if self.kind != "none" and lag_ms < FLOOR_MS:
            raise ValueError(f"a lag of {lag_ms} ms is below the floor of {FLOOR_MS} ms")
        self.lag_ms, self.only, self.exempt, self.budget_ms = float(lag_ms), only, set(exempt), float(budget_ms)
        self.calls = []      # every outermost hooked call: dict(k, op, site, waiter, waited, lagged)
        self.lags = []       # every lag placed: dict(site, stream, ms, held)
        self.failures = []   # "lag did not hold at <site>" ...
        self.spent_ms = 0.0
        self._depth = 0
        self._pending = []   # (event, lag record) of the lags placed since the last ordering point
        self._ev_stream = {}   # id(event) -> (event, stream): where an event was last recorded (the event is held: its id stays taken)
        self._saved = None
        self._names = {handle(s): f"pool[{i}]" for i, s in enumerate(self.pool)}

    # ---- what a test reads
    @property
    def waits(self) -> int:
        """Hooked forks and joins: the outermost wait_stream / wait_event calls."""
        return sum(1 for c in self.calls if c["op"] in ("wait_stream", "wait_event"))

    def pairs(self):
        """(waiter handle, waited handle) of every hooked wait whose two streams are known and differ."""
        return sorted({(c["waiter_h"], c["waited_h"]) for c in self.calls
                       if c.get("waiter_h") is not None and c.get("waited_h") is not None and c["waiter_h"] != c["waited_h"]})

    def streams_seen(self):
        return sorted({h for c in self.calls for h in (c.get("waiter_h"), c.get("waited_h")) if h is not None})

    def name(self, h):
        return "-" if h is None else self._names.get(h, f"stream {h:#x}")

    def report(self) -> str:
        lines = [f"policy {self.policy}, lag {self.lag_ms:.1f} ms, {len(self.lags)} lags ({self.spent_ms:.0f} ms), {self.waits} hooked waits"]
        for c in self.calls:
            lines.append(f"  #{c['k']:<3} {c['op']:<12} {c['site']:<48} waiter {self.name(c.get('waiter_h')):<10} "
                         f"waited {self.name(c.get('waited_h')):<10} lagged {self.name(c.get('lagged'))}")
        return "\n".join(lines + self.failures)

    # ---- the lag
    def _lag(self, stream, site):
        if self.spent_ms + self.lag_ms > self.budget_ms:
            raise LagBudget(f"lag budget: lag {len(self.lags) + 1} of {self.lag_ms:.1f} ms at {site} would bring the call's lags to "
                            f"{self.spent_ms + self.lag_ms:.0f} ms, over {self.budget_ms:.0f} ms")
        self.spent_ms += self.lag_ms
        self.backend.sleep(stream, self.lag_ms)
        ev = self.backend.new_event()
        ev.record(stream)
        rec = dict(site=site, stream=handle(stream), ms=self.lag_ms, held=None)
        self.lags.append(rec)
        self._pending.append((ev, rec))

    def _check_held(self, at):
        for ev, rec in self._pending:
            rec["held"] = not ev.query()
            if not rec["held"] and rec["site"] not in self.exempt:
                self.failures.append(f"lag did not hold at {at} (placed on {self.name(rec['stream'])} at {rec['site']})")
        self._pending = []

    # ---- the hooks
    def _hooked(self, op, orig, obj, args, kwargs):
        if self._depth:
            return orig(obj, *args, **kwargs)
        self._depth += 1
        try:
            site = _site(self.backend.skip)
            self._check_held(site)
            waiter = waited = None
            if op == "wait_stream":
                waiter, waited = obj, (args[0] if args else kwargs["stream"])
            elif op == "wait_event":
                ev = args[0] if args else kwargs["event"]
                waiter, waited = obj, self._ev_stream.get(id(ev), (None, None))[1]
            elif op == "record":
                st = args[0] if args else kwargs.get("stream")
                self._ev_stream[id(obj)] = (obj, st if st is not None else self.backend.current_stream())
            out = orig(obj, *args, **kwargs)
            k = len(self.calls)
            call = dict(k=k, op=op, site=site, waiter_h=handle(waiter) if waiter is not None else None,
                        waited_h=handle(waited) if waited is not None else None, lagged=None)
            self.calls.append(call)
            target = {"waiter": waiter, "waited": waited}.get(self.kind)
            if target is not None and (self.only is None or self.only == k):
                self._lag(target, site)
                call["lagged"] = handle(target)
            return out
        finally:
            self._depth -= 1

    def _wrap(self, op, orig):
        lagger = self

        def hook(obj, *args, **kwargs):
            return lagger._hooked(op, orig, obj, args, kwargs)
        hook.__name__ = getattr(orig, "__name__", op)
        return hook

    def __enter__(self):
        S, E = self.backend.Stream, self.backend.Event
        targets = [(S, "wait_stream"), (S, "wait_event"), (E, "record"), (E, "synchronize")]
        self._saved = [(cls, name, name in cls.__dict__, cls.__dict__.get(name)) for cls, name in targets]
        for cls, name in targets:
            setattr(cls, name, self._wrap(name, getattr(cls, name)))
        try:
            if self.kind == "pre" and (self.only is None or self.only == 0):
                self._depth += 1
                try:
                    self._lag(self.pool[self.pre_k], "before the call")
                finally:
                    self._depth -= 1
        except BaseException:
            self._restore()
            raise
        return self

    def _restore(self):
        for cls, name, own, old in self._saved or ():
            if own:
                setattr(cls, name, old)
            else:
                delattr(cls, name)
        self._saved = None

    def __exit__(self, exc_type, exc, tb):
        self._restore()
        if exc_type is None:
            self._depth += 1
            try:
                self._check_held("the end of the call")
            finally:
                self._depth -= 1
        self._pending, self._ev_stream = [], {}
        return False


# ---------------------------------------------------------------------------------------------------------------- independence
def probe_independence(pool, backend=None, lag_ms: float = 20.0, clock=time.perf_counter):
    """Two streams of a process may share a hardware queue; a lag on one then holds the other back too and hides the race it is there to
    show.  For every ordered pair (a, b) of `pool`: a lag on a, an event behind it, an event on b; b's event must complete while a's has
    not (polled with `query()` for at most the lag's length).  -> {(i, j): True (independent) | False (serialised)} by pool index."""
    backend = backend if backend is not None else TorchBackend()
    out = {}
    for i, a in enumerate(pool):
        for j, b in enumerate(pool):
            if i == j or handle(a) == handle(b):
                continue
            backend.sleep(a, lag_ms)
            ea, eb = backend.new_event(), backend.new_event()
            ea.record(a)
            eb.record(b)
            t0, free = clock(), False
            while True:
                done_b, done_a = eb.query(), ea.query()
                if done_b and not done_a:
                    free = True
                    break
                if done_a or (clock() - t0) * 1e3 > 4 * lag_ms:
                    break
            ea.synchronize()
            eb.synchronize()
            out[(i, j)] = free
    return out


def serialised_pairs(indep, pool, forked):
    """The pairs of `forked` ((waiter handle, waited handle), as `Lagger.pairs()` lists what the package forks or joins) that the probe
    found serialised in either order, by pool index."""
    idx = {}
    for i, s in enumerate(pool):
        idx.setdefault(handle(s), i)
    bad = set()
    for wa, wd in forked:
        if wa in idx and wd in idx and idx[wa] != idx[wd]:
            i, j = idx[wa], idx[wd]
            if not (indep.get((i, j), True) and indep.get((j, i), True)):
                bad.add((min(i, j), max(i, j)))
    return sorted(bad)


def warm_host_ms(call, sync, repeats: int = 3, clock=time.perf_counter) -> float:
    """Host wall time of `call()` plus `sync()`, best of `repeats` (the caller has warmed the call up)."""
    best = None
    for _ in range(repeats):
        t0 = clock()
        call()
        sync()
        dt = (clock() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best
