"""Training patches on the device (include/vsr_hip_patch.h, driver.patch_gather) against the numpy restatement of tests/_patch_ref.py,
bit for bit: the sources are random 32-bit words with NaN payloads, infinities and signed zeros planted, compared as int32 views.

csrc/train_patch.hip moves tiles of T x T = VSR_PATCH_TILE^2 output pixels (T = 32, read from the header by tests/test_abi_patch.py), the
transposed ones through LDS.  HR patch edges per scale S: 4 S (one partly filled tile: the LR patch is 4 x 4), T - T % S (one tile, full for
S = 1, 2, 4), the least multiple of S above T (one full tile and a ragged second one each way) and the least multiple of S above 2 T (two
full tiles and a ragged third): the tile loops of both grid regions run zero, one and two full times with a ragged end.  Sources: G = 4
frames of 96 x 120 and of 45 x 70 (odd sizes: the nearest LR mode only; the largest edge does not fit there and is left out)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lag as G  # noqa: E402
import _patch_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import driver  # noqa: E402
from video_super_resolution_amd.driver import patch_gather  # noqa: E402

T = R.TILE
SOURCES = {"96x120": (4, 96, 120), "45x70": (4, 45, 70), "6f": (6, 40, 52)}
PLANTED = (0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F812345, 0x00000001)


def edges(S):
    above = lambda v: (v // S + 1) * S   # noqa: E731
    return [4 * S, T - T % S, above(T), above(2 * T)]


@functools.lru_cache(maxsize=None)
def source(name, seed=0):
    """(host uint32 [G,H,W,3], the same words on the device as float32): random bits, the special patterns planted."""
    Gf, H, W = SOURCES[name]
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 2 ** 32, size=(Gf, H, W, 3), dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    at = rs.choice(flat.size, size=64 * len(PLANTED), replace=False)
    flat[at] = np.tile(np.array(PLANTED, dtype=np.uint32), 64)
    a.setflags(write=False)
    return a, on_device(a)


def on_device(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda().view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def table_all_flags(Gf, n, H, W, Ph, Pw, S, seed, flags=range(16), multiple_of_S=False):
    """One row per flag value; origins: the four corners first, then an odd x0 (where the mode allows one), then random ones."""
    rs = np.random.RandomState(seed)
    rows = []
    for b, f in enumerate(flags):
        ch, cw = R.crop(f, Ph, Pw)
        ymax, xmax = H - ch, W - cw
        if multiple_of_S:
            ymax, xmax = ymax // S * S, xmax // S * S
        corner = [(0, 0), (0, xmax), (ymax, 0), (ymax, xmax)]
        if b < 4:
            y0, x0 = corner[b]
        elif b == 4 and xmax >= 1 and not multiple_of_S:
            y0, x0 = min(1, ymax), 1
        else:
            step = S if multiple_of_S else 1
            y0, x0 = rs.randint(ymax // step + 1) * step, rs.randint(xmax // step + 1) * step
        rows.append((rs.randint(Gf - n + 1), y0, x0, f))
        assert R.row_ok(rows[-1], Gf, n, H, W, Ph, Pw, S, lr_src=multiple_of_S)
    return np.array(rows, dtype=np.int32)


def check(got_hr, got_lr, want_hr, want_lr, what):
    for name, got, want in (("hr", got_hr, want_hr), ("lr", got_lr, want_lr)):
        g = bits(got)
        assert g.shape == want.shape, (what, name, g.shape, want.shape)
        bad = np.argwhere(g != want)
        assert bad.shape[0] == 0, f"{what}: {name} differs in {bad.shape[0]} of {g.size} words, first at {tuple(bad[0])}"


CASES = [(S, name, P) for S in (1, 2, 3, 4) for name in ("96x120", "45x70") for P in edges(S) if P <= min(SOURCES[name][1:])]


# ------------------------------------------------------------------------------------------------ 1. all flags, every edge
@pytest.mark.parametrize("S, name, P", CASES)
def test_all_sixteen_flags_in_one_call_equal_the_restatement(S, name, P):
    Gf, H, W = SOURCES[name]
    words, src = source(name)
    table = table_all_flags(Gf, 3, H, W, P, P, S, seed=P)
    assert sorted(table[:, 3]) == list(range(16)) and (name != "96x120" or (table[:, 2] % 2 == 1).any())
    hr, lr = patch_gather(src, table, 3, P, S)
    check(hr, lr, R.gather_hr(words, table, 3, P, P), R.gather_lr_nearest(words, table, 3, P, P, S), (S, name, P))


def test_the_case_list_covers_what_the_docstring_says():
    assert edges(1) == [4, 32, 33, 65] and edges(2) == [8, 32, 34, 66] and edges(3) == [12, 30, 33, 66] and edges(4) == [16, 32, 36, 68]
    assert len(CASES) == 16 + 12
    for S in (1, 2, 3, 4):
        full = sorted({P // T for P in edges(S)}), sorted({(P // S) // T for P in edges(S)})
        assert full[0] == [0, 1, 2] and 0 in full[1]        # HR tile loops: zero, one and two full tiles; LR: zero at least
        assert any(P % T for P in edges(S))                 # ... with a ragged end
    assert sorted({(P // 1) // T for P in edges(1)}) == [0, 1, 2]   # (S = 1: the LR region sees all three too)


# ------------------------------------------------------------------------------------------------ 2. shapes of the call
@pytest.mark.parametrize("S", [3, 4])
def test_a_non_square_patch_without_and_with_the_transposition(S):
    Gf, H, W = SOURCES["96x120"]
    words, src = source("96x120")
    Ph, Pw = 36, 60   # multiples of 1, 2, 3 and 4; 60 x 36 when transposed
    plain = table_all_flags(Gf, 3, H, W, Ph, Pw, S, seed=1, flags=[0, 1, 2, 3, 8, 9, 10, 11])
    forced = table_all_flags(Gf, 3, H, W, Ph, Pw, S, seed=2, flags=[4, 5, 6, 7, 12, 13, 14, 15, 0, 3])
    for table in (plain, forced):
        hr, lr = patch_gather(src, table, 3, (Ph, Pw), S)
        assert tuple(hr.shape) == (len(table), 3, Ph, Pw, 3) and tuple(lr.shape) == (len(table), 3, Ph // S, Pw // S, 3)
        check(hr, lr, R.gather_hr(words, table, 3, Ph, Pw), R.gather_lr_nearest(words, table, 3, Ph, Pw, S), (S, table[:, 3]))


@pytest.mark.parametrize("n, name", [(3, "96x120"), (5, "6f")])
def test_one_sample_and_the_run_at_both_ends_of_the_group(n, name):
    Gf, H, W = SOURCES[name]
    words, src = source(name)
    P, S = 34, 2
    for t0 in (0, Gf - n):
        for flags in (0, 8, 13):
            table = np.array([[t0, 2, 5, flags]], dtype=np.int32)   # B = 1
            hr, lr = patch_gather(src, table, n, P, S)
            check(hr, lr, R.gather_hr(words, table, n, P, P), R.gather_lr_nearest(words, table, n, P, P, S), (n, t0, flags))
    with pytest.raises(driver.L.VsrHipError, match=rf"row 0 takes frames {Gf - n + 1} .. {Gf} of {Gf}"):
        patch_gather(src, np.array([[Gf - n + 1, 0, 0, 0]], dtype=np.int32), n, P, S)


@pytest.mark.parametrize("S", [1, 3])
def test_hr_only_lr_only_and_both_agree(S):
    Gf, H, W = SOURCES["96x120"]
    words, src = source("96x120")
    P = edges(S)[2]
    table = table_all_flags(Gf, 3, H, W, P, P, S, seed=9)
    want_hr, want_lr = R.gather_hr(words, table, 3, P, P), R.gather_lr_nearest(words, table, 3, P, P, S)
    hr, lr = patch_gather(src, table, 3, P, S)
    check(hr, lr, want_hr, want_lr, "both")
    hr, none = patch_gather(src, table, 3, P, S, want_lr=False)
    assert none is None and np.array_equal(bits(hr), want_hr)
    none, lr = patch_gather(src, table, 3, P, S, want_hr=False)
    assert none is None and np.array_equal(bits(lr), want_lr)
    # into buffers of the caller's
    hr_out, lr_out = torch.zeros_like(hr), torch.zeros_like(lr)
    got = patch_gather(src, table, 3, P, S, hr_out=hr_out, lr_out=lr_out)
    assert got[0] is hr_out and got[1] is lr_out
    check(hr_out, lr_out, want_hr, want_lr, "out=")
    with pytest.raises(ValueError, match="lr_out must be"):
        patch_gather(src, table, 3, P, S, lr_out=torch.zeros_like(hr)[:, :2])


# ------------------------------------------------------------------------------------------------ 3. the LR source mode
@pytest.mark.parametrize("S", [2, 3, 4])
def test_lr_src_mode_equals_the_restatement_and_nearest_mode_without_flips(S):
    Gf, H, W = SOURCES["96x120"]
    words, src = source("96x120")
    lwords = np.random.RandomState(S).randint(0, 2 ** 32, size=(Gf, H // S, W // S, 3), dtype=np.uint64).astype(np.uint32)
    lsrc = on_device(lwords)
    for P in edges(S)[1:]:
        table = table_all_flags(Gf, 3, H, W, P, P, S, seed=P, multiple_of_S=True)
        hr, lr = patch_gather(src, table, 3, P, S, lr_src=lsrc)
        check(hr, lr, R.gather_hr(words, table, 3, P, P), R.gather_lr_src(lwords, table, 3, P, P, S), ("lr_src", S, P))
        none, lr = patch_gather(src, table, 3, P, S, lr_src=lsrc, want_hr=False)
        assert none is None and np.array_equal(bits(lr), R.gather_lr_src(lwords, table, 3, P, P, S))
    # lr_src = the nearest decimation of src: without a flip bit both modes are the same copy
    dwords = np.ascontiguousarray(words[:, ::S, ::S])
    P = edges(S)[2]
    table = table_all_flags(Gf, 3, H, W, P, P, S, seed=3, flags=[0, 4, 8, 12, 0, 4, 8, 12], multiple_of_S=True)
    _, lr_a = patch_gather(src, table, 3, P, S, lr_src=on_device(dwords), want_hr=False)
    _, lr_b = patch_gather(src, table, 3, P, S, want_hr=False)
    assert np.array_equal(bits(lr_a), bits(lr_b))
    # ... and with one it is the other phase (what the header warns against), so the two differ
    flip = table.copy()
    flip[:, 3] |= 2
    _, lr_a = patch_gather(src, flip, 3, P, S, lr_src=on_device(dwords), want_hr=False)
    _, lr_b = patch_gather(src, flip, 3, P, S, want_hr=False)
    assert np.array_equal(bits(lr_a), R.gather_lr_nearest_wrong_phase(words, flip, 3, P, P, S))
    assert np.array_equal(bits(lr_b), R.gather_lr_nearest(words, flip, 3, P, P, S)) and not np.array_equal(bits(lr_a), bits(lr_b))
    with pytest.raises(driver.L.VsrHipError, match="with lr_src the origin"):
        patch_gather(src, np.array([[0, 1, 0, 0]], dtype=np.int32), 3, P, S, lr_src=lsrc)


# ------------------------------------------------------------------------------------------------ 4. against ingest_item
@pytest.mark.parametrize("S", [2, 4])
def test_the_identity_patch_reproduces_ingest_item(S):
    H, W, Tw = 64, 96, 3
    video = driver.synthetic_video(Tw + 2, H, W)
    datas = torch.from_numpy(np.stack([video[i:i + 3] for i in range(Tw)])).cuda()
    data, target, high_frames = driver.ingest_item(datas, S)
    src = torch.from_numpy(video).cuda().float()
    table = np.array([[t, 0, 0, 0] for t in range(Tw)], dtype=np.int32)
    hr, lr = patch_gather(src, table, 3, (H, W), S)
    assert torch.equal(bits_t(hr), bits_t(high_frames)) and torch.equal(bits_t(lr), bits_t(data))
    for t in range(Tw):
        d, y, hf = driver.patch_item(hr, lr, t)
        assert torch.equal(d[0], data[t]) and torch.equal(y[0], target[t]) and torch.equal(hf[0], high_frames[t])


def bits_t(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 5. every output word, none beyond
@pytest.mark.parametrize("S, P, mode", [(1, 33, "nearest"), (3, 66, "nearest"), (4, 36, "lr_src"), (2, 8, "nearest")])
def test_poisoned_outputs_are_written_in_full_and_nothing_else(S, P, mode):
    Gf, H, W = SOURCES["96x120"]
    rs = np.random.RandomState(11)
    vals = rs.uniform(-4.0, 300.0, size=(Gf, H, W, 3)).astype(np.float32)   # finite: no word is the poison pattern
    src = torch.from_numpy(vals).cuda()
    lvals = rs.uniform(-4.0, 300.0, size=(Gf, H // S, W // S, 3)).astype(np.float32)
    lsrc = torch.from_numpy(lvals).cuda() if mode == "lr_src" else None
    table = table_all_flags(Gf, 3, H, W, P, P, S, seed=P, multiple_of_S=mode == "lr_src")
    with poisoned() as arena:
        hr, lr = patch_gather(src, table, 3, P, S, lr_src=lsrc)
        assert arena.n_allocated == 2
        arena.assert_written(hr, "hr")
        arena.assert_written(lr, "lr")
        arena.check()
        want_lr = R.gather_lr_src(lvals, table, 3, P, P, S) if mode == "lr_src" else R.gather_lr_nearest(vals, table, 3, P, P, S)
        check(hr, lr, R.gather_hr(vals, table, 3, P, P), want_lr, (S, P, mode))
    with poisoned() as arena:   # one output at a time: the other region of the grid is absent
        _, lr = patch_gather(src, table, 3, P, S, lr_src=lsrc, want_hr=False)
        hr, _ = patch_gather(src, table, 3, P, S, lr_src=lsrc, want_lr=False)
        assert arena.n_allocated == 2
        arena.assert_written(hr, "hr alone")
        arena.assert_written(lr, "lr alone")
        arena.check()


# ------------------------------------------------------------------------------------------------ 6. stream order
def test_a_call_on_a_side_stream_with_a_lagging_main_stream_gives_the_same_bits():
    """The call is enqueued on the current stream alone (tests/_lag.py, policy pre:0: one lag on the main stream before the call): on a side
    stream that has the inputs it neither waits for the main stream nor needs anything from it."""
    Gf, H, W = SOURCES["96x120"]
    words, src = source("96x120")
    S, P = 2, 66
    table = table_all_flags(Gf, 3, H, W, P, P, S, seed=4)
    want_hr, want_lr = R.gather_hr(words, table, 3, P, P), R.gather_lr_nearest(words, table, 3, P, P, S)
    main = torch.cuda.current_stream()
    backend = G.TorchBackend()
    side = None
    for _ in range(4):   # a side stream on a hardware queue of its own (streams may share one: the lag would hold both)
        cand = torch.cuda.Stream()
        if all(G.probe_independence([main, cand], backend, lag_ms=10.0).values()):
            side = cand
            break
    assert side is not None, "no side stream independent of the main stream among four"
    hr_out = torch.zeros((16, 3, P, P, 3), device="cuda")
    lr_out = torch.zeros((16, 3, P // S, P // S, 3), device="cuda")

    def call():
        with torch.cuda.stream(side):
            patch_gather(src, table, 3, P, S, hr_out=hr_out, lr_out=lr_out)

    torch.cuda.synchronize()
    host_ms = G.warm_host_ms(call, side.synchronize)
    hr_out.zero_()
    lr_out.zero_()
    torch.cuda.synchronize()
    with G.Lagger("pre:0", G.lag_for(host_ms), pool=[main, side], backend=backend) as lg:
        call()
        side.synchronize()            # the side stream has finished ...
    assert lg.failures == [] and len(lg.lags) == 1 and lg.lags[0]["held"], lg.report()   # ... while the main stream still lagged
    torch.cuda.synchronize()
    assert np.array_equal(bits(hr_out), want_hr) and np.array_equal(bits(lr_out), want_lr)
