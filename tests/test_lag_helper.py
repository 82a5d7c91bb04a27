"""tests/_lag.py on fake streams, fake events and a fake sleep: what the GPU cases of tests/test_gpu_stream_order.py rely on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lag as G  # noqa: E402


def make_backend():
    """A backend with classes of its own (the patches go onto class attributes: every test gets fresh ones)."""
    class Event:
        complete = False   # what query() answers: False = the work in front of the event is still running (a lag holds)

        def __init__(self):
            self.stream, self.synced = None, 0

        def record(self, stream=None):
            self.stream = stream if stream is not None else be.cur

        def synchronize(self):
            self.synced += 1

        def query(self):
            return type(self).complete

        def wait(self, stream):
            stream.waited_for.append(self)

    class Stream:
        def __init__(self, h):
            self.cuda_stream, self.waited_for = h, []

        def record_event(self):
            e = Event()
            e.record(self)
            return e

        def wait_event(self, event):
            event.wait(self)

        def wait_stream(self, stream):   # as torch's: a wait_event and a record inside, which must not count
            self.wait_event(stream.record_event())

    class Backend:
        skip = ()

        def __init__(self):
            self.Stream, self.Event, self.slept = Stream, Event, []
            self.cur = Stream(0)

        def current_stream(self):
            return Stream(self.cur.cuda_stream)   # (a new object per call, like torch.cuda.current_stream)

        def new_event(self):
            return Event()

        def sleep(self, stream, ms):
            self.slept.append((stream.cuda_stream, ms))
    be = Backend()
    return be


def pool_of(be, n):
    return [be.cur] + [be.Stream(16 * k) for k in range(1, n)]


def fork_join(main, side):
    side.wait_stream(main)
    main.wait_stream(side)


def test_only_outermost_calls_are_counted_and_listed_with_their_site():
    be = make_backend()
    main, side = pool_of(be, 2)
    with G.Lagger("none", 0.0, pool=[main, side], backend=be) as lg:
        fork_join(main, side)
        e = be.Event()
        e.record(side)
        main.wait_event(e)
        e.synchronize()
    assert [c["op"] for c in lg.calls] == ["wait_stream", "wait_stream", "record", "wait_event", "synchronize"]
    assert lg.waits == 3 and be.slept == [] and lg.failures == []
    assert all(c["site"].startswith("tests/test_lag_helper.py:") for c in lg.calls), lg.calls
    assert lg.calls[0]["site"] != lg.calls[1]["site"]
    # the event's stream is remembered from the hooked record: wait_event knows whom it waits on
    assert (lg.calls[3]["waiter_h"], lg.calls[3]["waited_h"]) == (0, 16)
    assert lg.pairs() == [(0, 16), (16, 0)] and lg.streams_seen() == [0, 16]


@pytest.mark.parametrize("policy,want", [("waiter", [16, 0, 0]), ("waited", [0, 16, 32]), ("pre:0", [0]), ("pre:2", [32]), ("none", [])])
def test_each_policy_lags_the_right_stream(policy, want):
    be = make_backend()
    main, side, other = pool = pool_of(be, 3)
    with G.Lagger(policy, 7.0, pool=pool, backend=be) as lg:
        fork_join(main, side)
        e = be.Event()
        with_stream = other
        e.record(with_stream)
        main.wait_event(e)
    assert be.slept == [(h, 7.0) for h in want]
    assert [r["stream"] for r in lg.lags] == want and all(r["held"] for r in lg.lags) and lg.failures == []
    assert lg.spent_ms == 7.0 * len(want)
    # the harness's own record behind each sleep is not a hooked call
    assert [c["op"] for c in lg.calls] == ["wait_stream", "wait_stream", "record", "wait_event"]


def test_an_event_recorded_on_the_current_stream_and_an_unseen_record():
    be = make_backend()
    main, side = pool = pool_of(be, 2)
    old = be.Event()
    old.record(side)          # (recorded before the Lagger was entered: its stream is not known)
    with G.Lagger("waited", 5.0, pool=pool, backend=be) as lg:
        e = be.Event()
        e.record()            # the current stream
        side.wait_event(e)
        main.wait_event(old)
    assert be.slept == [(0, 5.0)]
    assert lg.calls[1]["waited_h"] == 0 and lg.calls[2]["waited_h"] is None and lg.calls[2]["lagged"] is None


def test_only_lags_at_one_ordinal():
    be = make_backend()
    main, side = pool = pool_of(be, 2)
    with G.Lagger("waiter", 5.0, pool=pool, backend=be, only=1) as lg:
        fork_join(main, side)
        fork_join(main, side)
    assert be.slept == [(0, 5.0)] and [c["lagged"] for c in lg.calls] == [None, 0, None, None]


def test_a_lag_that_has_ended_at_the_next_ordering_point_fails_the_case():
    be = make_backend()
    main, side = pool = pool_of(be, 2)
    be.Event.complete = True
    with G.Lagger("waiter", 5.0, pool=pool, backend=be) as lg:
        fork_join(main, side)
    assert [r["held"] for r in lg.lags] == [False, False]
    assert len(lg.failures) == 2 and all(f.startswith("lag did not hold at ") for f in lg.failures)
    assert "tests/test_lag_helper.py:" in lg.failures[0] and lg.failures[1].startswith("lag did not hold at the end of the call")
    assert "lag did not hold" in lg.report()
    # an interval listed as exempt (by the site that placed the lag) is not a failure, but is still reported as not held
    site = lg.lags[0]["site"]
    be2 = make_backend()
    main, side = pool = pool_of(be2, 2)
    be2.Event.complete = True
    with G.Lagger("pre:1", 5.0, pool=pool, backend=be2, exempt={"before the call"}) as lg2:
        fork_join(main, side)
    assert lg2.failures == [] and [r["held"] for r in lg2.lags] == [False] and site != "before the call"


def test_floor_and_budget():
    assert G.lag_for(0.3) == 5.0 and G.lag_for(2.5) == 5.0 and G.lag_for(40.0) == 80.0
    be = make_backend()
    main, side = pool = pool_of(be, 2)
    with pytest.raises(ValueError, match="floor"):
        G.Lagger("waiter", 4.9, pool=pool, backend=be)
    # 2 s in all: three lags of 800 ms do not fit; the third raises, nothing is shortened, and the patches are gone
    with pytest.raises(G.LagBudget, match="lag budget"):
        with G.Lagger("waiter", 800.0, pool=pool, backend=be) as lg:
            fork_join(main, side)
            fork_join(main, side)
    assert be.slept == [(16, 800.0), (0, 800.0)] and lg.spent_ms == 1600.0
    assert "hook" not in be.Stream.wait_stream.__qualname__
    with G.Lagger("waiter", 1000.0, pool=pool, backend=be) as lg:   # exactly 2 s is allowed
        fork_join(main, side)
    assert lg.spent_ms == 2000.0
    with pytest.raises(G.LagBudget):
        with G.Lagger("pre:0", 2000.5, pool=pool, backend=be):
            pass
    assert "hook" not in be.Stream.wait_stream.__qualname__


def test_patches_are_restored_after_an_exception():
    be = make_backend()
    main, side = pool = pool_of(be, 2)
    before = {(cls, n): cls.__dict__[n] for cls, n in ((be.Stream, "wait_stream"), (be.Stream, "wait_event"), (be.Event, "record"),
                                                       (be.Event, "synchronize"))}
    with pytest.raises(RuntimeError, match="boom"):
        with G.Lagger("waiter", 5.0, pool=pool, backend=be):
            assert be.Stream.__dict__["wait_stream"] is not before[(be.Stream, "wait_stream")]
            side.wait_stream(main)
            raise RuntimeError("boom")
    for (cls, n), fn in before.items():
        assert cls.__dict__[n] is fn
    with G.Lagger("none", 0.0, backend=be):
        pass
    for (cls, n), fn in before.items():
        assert cls.__dict__[n] is fn
    side.wait_stream(main)   # and they still work
    assert len(side.waited_for) == 2


def test_pre_turns():
    assert G.policies(1) == ["waiter", "waited", "pre:0"]
    assert G.policies(4) == ["waiter", "waited", "pre:0", "pre:1", "pre:2", "pre:3"]
    assert G.parse_policy("pre:3", 4) == ("pre", 3) and G.parse_policy("waited", 0) == ("waited", None)
    for bad in ("pre:4", "pre:-1", "pre:x", "both"):
        with pytest.raises(ValueError):
            G.parse_policy(bad, 4)


def test_independence_probe_and_the_pairs_that_matter():
    be = make_backend()
    pool = pool_of(be, 3)
    shared = {(0, 32), (32, 0)}   # streams 0 and 32 share a queue: an event on one is done only when the other's lag is

    class Ev(be.Event):
        def query(self):
            return self.done()

    state = {"lagged": None, "polls": 0}

    def new_event():
        e = Ev()

        def done():
            state["polls"] += 1
            h = e.stream.cuda_stream
            blocked = h == state["lagged"] or (state["lagged"], h) in shared
            return not blocked or state["polls"] > 6   # (the lag ends after a few polls)
        e.done = done
        return e

    def sleep(stream, ms):
        state["lagged"], state["polls"] = stream.cuda_stream, 0
    be.new_event, be.sleep = new_event, sleep
    indep = G.probe_independence(pool, backend=be, lag_ms=5.0)
    assert indep == {(0, 1): True, (1, 0): True, (1, 2): True, (2, 1): True, (0, 2): False, (2, 0): False}
    assert G.serialised_pairs(indep, pool, [(16, 0), (0, 16)]) == []
    assert G.serialised_pairs(indep, pool, [(32, 0), (16, 32)]) == [(0, 2)]
    assert G.serialised_pairs(indep, pool, [(48, 0)]) == []   # (a stream outside the pool: nothing the probe can say)


def test_warm_host_ms_is_the_best_of_three():
    ticks = iter([0.0, 0.030, 1.0, 1.010, 2.0, 2.020])
    calls = []
    assert G.warm_host_ms(lambda: calls.append("c"), lambda: calls.append("s"), clock=lambda: next(ticks)) == pytest.approx(10.0)
    assert calls == ["c", "s"] * 3
