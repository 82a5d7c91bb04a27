"""tests/_poison.py tested on its own, without a GPU: a fake "kernel" written with torch indexing that leaves an element
unwritten, writes one element past the end, writes one element before the start, or behaves.  The helper must flag the first
three with the allocation site and the offset and pass the fourth; this is what makes a green run of
tests/test_gpu_poisoned_buffers.py mean something."""
import inspect
import os
import re

import pytest
import torch

from _poison import DEFAULT_BAND, PoisonError, poisoned

HERE = os.path.basename(__file__)


def _lineno():
    return inspect.currentframe().f_back.f_lineno


def _raw(t, arena):
    """The whole block (bands included) behind an arena tensor, viewed in the tensor's dtype: what a kernel holding the raw
    pointer can reach."""
    r = arena.find(t)
    return r.block.view(t.dtype), r.band // t.element_size()


def _kernel(out, arena, mode):
    """Writes out[i] = i.  mode 'skip': element 5 is left out; 'over': one element past the end too; 'under': one before the start."""
    n = out.numel()
    raw, first = _raw(out, arena)
    vals = torch.arange(n, dtype=out.dtype)
    if mode == "skip":
        keep = torch.ones(n, dtype=torch.bool)
        keep[5] = False
        out.view(-1)[keep] = vals[keep]
    else:
        out.view(-1).copy_(vals)
    if mode == "over":
        raw[first + n] = 1.0
    if mode == "under":
        raw[first - 1] = 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64, torch.bfloat16])
def test_an_unwritten_element_is_found_with_its_site(dtype):
    with poisoned(devices=("cpu",)) as arena:
        line = _lineno() + 1
        out = torch.empty((3, 7), dtype=dtype, device="cpu")
        assert out.shape == (3, 7) and out.dtype == dtype and out.is_contiguous()
        assert out.data_ptr() % 64 == 0
        assert torch.isnan(out.float()).all()                   # the poison is a NaN in every floating format
        assert arena.unwritten(out).shape[0] == 21
        _kernel(out, arena, "skip")
        idx = arena.unwritten(out)
        assert idx.tolist() == [[0, 5]]
        assert torch.isnan(out.float()).sum() == 1
        with pytest.raises(PoisonError, match=rf"1 of 21 elements were never written.*\(0, 5\).*{re.escape(HERE)}:{line}"):
            arena.assert_written(out, "out")
        lines = arena.unwritten_sites()
        assert len(lines) == 1 and f"{HERE}:{line}" in lines[0] and "first flat index 5" in lines[0]
        arena.check()                                           # nothing outside the payload was touched


def test_a_write_past_the_end_is_found_with_site_and_offset():
    with poisoned(devices=("cpu",)) as arena:
        other = torch.empty(100, dtype=torch.float32)          # (default device: the CPU)
        line = _lineno() + 1
        out = torch.empty(21, dtype=torch.float32, device="cpu")
        _kernel(other, arena, "ok")
        _kernel(out, arena, "over")
        assert arena.unwritten(out).shape[0] == 0               # the payload itself is complete
        with pytest.raises(PoisonError) as e:
            arena.check()
        msg = str(e.value)
        assert "PAST the end" in msg and "BEFORE" not in msg
        assert "first at byte offset 84 " in msg and "element 21" in msg          # 21 float32 elements: bytes 0..83 are the caller's
        assert f"{HERE}:{line}" in msg and f"{HERE}:{line - 2}" not in msg       # the damaged allocation only


def test_a_write_into_the_far_band_is_found():
    """Not only the round-up slack: a store hundreds of bytes beyond the payload (another row, another tile)."""
    with poisoned(devices=("cpu",)) as arena:
        out = torch.empty(128, dtype=torch.float32, device="cpu")   # exactly 512 B: no slack
        _kernel(out, arena, "ok")
        raw, first = _raw(out, arena)
        raw[first + 128 + 1000] = 0.0
        with pytest.raises(PoisonError, match=r"PAST the end.*first at byte offset 4512 "):
            arena.check()


def test_a_write_before_the_start_is_found_with_site_and_offset():
    with poisoned(devices=("cpu",)) as arena:
        line = _lineno() + 1
        out = torch.empty((2, 8), dtype=torch.float16, device="cpu")
        _kernel(out, arena, "under")
        with pytest.raises(PoisonError) as e:
            arena.check()
        msg = str(e.value)
        assert "BEFORE the start" in msg and "PAST" not in msg
        assert "nearest at byte offset -1 " in msg and "(first at -2)" in msg      # one float16 just below the payload
        assert f"{HERE}:{line}" in msg


def test_a_well_behaved_kernel_passes_and_blocks_can_be_released_in_stages():
    with poisoned(devices=("cpu",)) as arena:
        a = torch.empty((4, 5), dtype=torch.float32, device="cpu")
        b = torch.empty_like(a)
        c = a.new_empty((7,))
        d = torch.empty_strided((2, 3), (1, 2), dtype=torch.float32, device="cpu")
        e = torch.empty(9, dtype=torch.uint8, device="cpu")
        assert d.stride() == (1, 2) and int(e[0]) == 255
        assert b.shape == a.shape and c.shape == (7,) and c.dtype == a.dtype
        for t in (a, b, c):
            assert torch.isnan(t).all()
            _kernel(t, arena, "ok")
            assert arena.unwritten(t).shape[0] == 0
        assert arena.check(release=True) == 5
        assert arena.records == []
        f = torch.empty(3, dtype=torch.float32, device="cpu")
        _kernel(f, arena, "ok")
        assert arena.check() == 1
        assert arena.unwritten_sites() == []
        assert torch.equal(a.view(-1), torch.arange(20, dtype=torch.float32))     # released blocks live on through their tensors


def test_noncontiguous_empty_like_keeps_the_strides():
    with poisoned(devices=("cpu",)) as arena:
        like = torch.zeros((4, 6)).t()
        got = torch.empty_like(like)
        assert got.stride() == like.stride() and got.shape == like.shape and torch.isnan(got).all()
        assert torch.empty_like(like, memory_format=torch.contiguous_format).is_contiguous()
        arena.check()


def test_the_patched_names_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with pytest.raises(ZeroDivisionError):
        with poisoned(devices=("cpu",)):
            assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[3]
            1 / 0
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    assert after == before
    with poisoned(devices=("cpu",)):
        pass
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before[:4]
    t = torch.empty(4)
    assert t._base is None                                                     # an ordinary allocation again


def test_integer_pinned_out_and_foreign_device_allocations_pass_through():
    with poisoned(devices=("cpu",)) as arena:
        for dt in (torch.int32, torch.int64, torch.int16, torch.bool):
            t = torch.empty(8, dtype=dt, device="cpu")
            assert t._base is None and t.dtype == dt                            # untouched: may be an index
        assert torch.empty_like(torch.zeros(3, dtype=torch.int64))._base is None
        assert torch.zeros(3).new_empty(4, dtype=torch.int32)._base is None
        dst = torch.zeros(5)
        assert torch.empty(5, out=dst) is dst and float(dst.sum()) == 0.0
        assert torch.empty(0)._base is None and torch.empty((3, 0, 2)).shape == (3, 0, 2)
        try:
            p = torch.empty(16, dtype=torch.float32, pin_memory=True)
        except RuntimeError:                                                    # no accelerator runtime: pinning itself is refused
            p = None
        assert p is None or p._base is None
        assert arena.records == []
    with poisoned() as arena:                                                   # the default: CUDA allocations only
        t = torch.empty(8, dtype=torch.float32)
        assert t._base is None and arena.records == []
        assert torch.zeros(4).sum() == 0 and torch.full((2,), 3.0).sum() == 6.0


def test_package_buffers_are_emptied_inside_the_block_and_put_back():
    from video_super_resolution_amd import igemm

    class Owner:
        pass
    o = Owner()
    marker = torch.zeros(2)
    o.__dict__["_bufs"] = {("out", (1, 2), None, 0): marker}
    igemm._ws[("test", 0, 0)] = marker
    try:
        with poisoned(devices=("cpu",)):
            assert o._bufs == {} and igemm._ws == {}
            o._bufs["inside"] = torch.zeros(1)
        assert list(o._bufs.values()) == [marker] and igemm._ws[("test", 0, 0)] is marker
    finally:
        igemm._ws.pop(("test", 0, 0), None)


def test_band_is_a_multiple_of_the_allocation_granularity():
    assert DEFAULT_BAND % 512 == 0
    with pytest.raises(ValueError):
        with poisoned(band=100):
            pass
