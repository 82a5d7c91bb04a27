"""vsr_cell_stats on the device (include/vsr_hip_cell.h; `frames.cell_stats`) against the numpy restatement tests/_cell_ref.py: bit equality
of every int32 of the map, no tolerance (the values are sums of integers).  Sizes where a cell, a tile and a row end differently, both load
paths, an unaligned base, inputs with NaN / negatives / values above 255 / signed zeros, exact ties of the luma, a constant frame; the
cut sums against `scene_sums`; a poisoned `out=`; a side stream beside a lagging main stream; independence of G."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _cell_ref as R  # noqa: E402
import _lag as G  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402
from video_super_resolution_amd.driver import cell_stats  # noqa: E402

# the issue's sizes, and one more on the 16-byte path: W % 4 == 0 but no multiple of the tile, three tiles across (the halo column and the
# ragged tile under float4 loads), three tile rows
SIZES = R.SIZES + [(2, 40, 132)]


def run(frames, luma4=None, **kw):
    return cell_stats(torch.from_numpy(frames).cuda(), luma4, **kw).cpu().numpy()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_map_equals_the_restatement_bit_for_bit(size, kind):
    f = R.make_frames(kind, *size, seed=1)
    lu = R.luma_of(kind)
    got, want = run(f, lu), R.cell_stats(f, lu)
    assert got.dtype == np.int32 and got.shape == want.shape == (size[0],) + R.cells(*size[1:]) + (2,)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (got[0, :, :, 1] == 0).all() and got.min() >= 0 and got.max() <= R.MAX_VALUE
    if kind == "constant":
        assert not got.any()
    elif kind == "ties":
        y = (0.5 * f[..., 0] + 0.25 * f[..., 1] + 0.25 * f[..., 2]).astype(np.float64)
        assert (y - np.floor(y) == 0.5).any()       # the case is there: a luma exactly between two codes
    elif kind == "salted":
        assert np.isnan(f).any() and (f < 0).any() and (f > 255).any() and (np.signbit(f) & (f == 0)).any()


def test_the_default_luma_is_that_of_scene_sums():
    f = R.make_frames("bytes", 2, 33, 17)
    assert np.array_equal(run(f), R.cell_stats(f, R.LUMA_BT601))
    assert not np.array_equal(run(f), run(f, R.LUMA_TIES))


@pytest.mark.parametrize("size", [(9, 48, 64), (3, 45, 70), (2, 40, 132)], ids=lambda s: "x".join(str(v) for v in s))
def test_a_base_one_float_into_its_storage_gives_the_same_bits(size):
    """The view starts 4 bytes into an aligned allocation: element loads whatever W is; the aligned tensor of a W % 4 == 0 size takes the
    16-byte loads.  Both equal the restatement, so they equal each other."""
    f = R.make_frames("salted", *size, seed=2)
    store = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), f.reshape(-1)])).cuda()
    view = store[1:].view(*f.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    aligned = torch.from_numpy(f).cuda()
    assert aligned.data_ptr() % 16 == 0
    want = R.cell_stats(f)
    assert np.array_equal(cell_stats(view).cpu().numpy(), want) and np.array_equal(cell_stats(aligned).cpu().numpy(), want)


@pytest.mark.parametrize("size", [(9, 48, 64), (3, 45, 70), (2, 5, 7)], ids=lambda s: "x".join(str(v) for v in s))
def test_the_cut_sums_are_those_of_scene_sums_exactly(size):
    k = (size[0] + 1) // 2                                            # k dark frames, then bright ones: one cut, the pair (k - 1, k)
    frames = [R.make_frames("bytes", k, *size[1:], seed=3) * 0.25, 255.0 - R.make_frames("bytes", size[0] - k, *size[1:], seed=4) * 0.25]
    f = np.ascontiguousarray(np.concatenate(frames).astype(np.float32))
    t = torch.from_numpy(f).cuda()
    stats = cell_stats(t)
    cuts, m = driver.cell_cuts(stats, size[1:])
    sums = driver.scene_sums(t[:-1].contiguous(), t[1:].contiguous())
    wcuts, wm = driver.scene_cuts(sums)
    assert np.array_equal(m.view(np.uint64), wm.view(np.uint64)) and np.array_equal(cuts, wcuts)
    assert np.array_equal(stats.cpu().numpy()[1:, :, :, 1].astype(np.int64).sum(axis=(1, 2)), sums.cpu().numpy()[:, 0].astype(np.int64))
    assert cuts.sum() == 1 and cuts[k - 1]
    rcuts, rm = R.cell_cuts(R.cell_stats(f), size[1:])
    assert np.array_equal(cuts, rcuts) and np.array_equal(m.view(np.uint64), rm.view(np.uint64))


@pytest.mark.parametrize("size", [(3, 45, 70), (9, 48, 64), (2, 5, 7)], ids=lambda s: "x".join(str(v) for v in s))
def test_out_in_a_poisoned_larger_tensor_is_written_in_full_and_nothing_else(size):
    f = R.make_frames("bytes", *size, seed=5)
    t = torch.from_numpy(f).cuda()
    shape = (size[0],) + R.cells(*size[1:]) + (2,)
    n, before, after = int(np.prod(shape)), 37, 91
    with poisoned(extra_dtypes=(torch.int32,)) as arena:
        big = torch.empty(before + n + after, dtype=torch.int32, device="cuda")
        assert arena.n_allocated == 1 and arena.unwritten(big).shape[0] == big.numel()
        out = big[before:before + n].view(shape)
        got = cell_stats(t, out=out)
        assert got.data_ptr() == out.data_ptr() and arena.n_allocated == 1      # the call allocates nothing of its own
        arena.assert_written(out, "the map")                                   # (no value of the map is -1)
        assert arena.unwritten(big[:before]).shape[0] == before and arena.unwritten(big[before + n:]).shape[0] == after
        arena.check()
        assert np.array_equal(out.cpu().numpy(), R.cell_stats(f))
    with pytest.raises(ValueError, match="out must be int32"):
        cell_stats(t, out=torch.empty(shape[:-1] + (3,), dtype=torch.int32, device="cuda"))


def test_a_call_on_a_side_stream_with_a_lagging_main_stream_gives_the_same_bits():
    """The call is enqueued on the current stream alone (tests/_lag.py, policy pre:0: one lag on the main stream before the call)."""
    f = R.make_frames("bytes", 9, 48, 64, seed=6)
    t = torch.from_numpy(f).cuda()
    want = R.cell_stats(f)
    main = torch.cuda.current_stream()
    backend = G.TorchBackend()
    side = None
    for _ in range(4):   # a side stream on a hardware queue of its own (streams may share one: the lag would hold both)
        cand = torch.cuda.Stream()
        if all(G.probe_independence([main, cand], backend, lag_ms=10.0).values()):
            side = cand
            break
    assert side is not None, "no side stream independent of the main stream among four"
    out = torch.zeros(want.shape, dtype=torch.int32, device="cuda")

    def call():
        with torch.cuda.stream(side):
            cell_stats(t, out=out)

    torch.cuda.synchronize()
    host_ms = G.warm_host_ms(call, side.synchronize)
    out.fill_(-1)
    torch.cuda.synchronize()
    with G.Lagger("pre:0", G.lag_for(host_ms), pool=[main, side], backend=backend) as lg:
        call()
        side.synchronize()            # the side stream has finished ...
    assert lg.failures == [] and len(lg.lags) == 1 and lg.lags[0]["held"], lg.report()   # ... while the main stream still lagged
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_a_frames_activity_does_not_depend_on_the_group_it_travelled_in():
    f = R.make_frames("salted", 9, 48, 64, seed=7)
    whole = run(f)
    alone = run(np.ascontiguousarray(f[5:6]))
    assert alone.shape == (1, 3, 4, 2) and np.array_equal(alone[0, :, :, 0], whole[5, :, :, 0]) and not alone[0, :, :, 1].any()
    pair = run(np.ascontiguousarray(f[4:6]))
    assert np.array_equal(pair[1], whole[5])       # and the temporal term only on the frame before
