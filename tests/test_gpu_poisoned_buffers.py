"""The product's paths on poisoned, guard-banded buffers (tests/_poison.py): every byte a kernel's consumer reads has been
written by a kernel or a zero fill in the same call, and no launch stores outside the extents it was passed.

Each case runs once ordinarily on a fresh object (`want`) and once inside `poisoned()` on another fresh object (`got`):

  * `got` holds no NaN and equals `want` bit for bit (every path is deterministic; the one exception, the warp's image
    gradient -- float atomics --, keeps the bar of its own test);
  * `arena.check()`: no byte outside any payload was modified by any launch of the case;
  * documented channel padding of a returned NHWC map is exactly zero; the neighbours of a channel-slice write are untouched;
  * staleness: on the SAME poisoned object a second call at the same geometry with other inputs equals a fresh object's
    result for those inputs, bit for bit.

The launches and geometries are those of the existing value tests (their shape lists are imported); only buffer contents
differ, and nothing poisoned is ever an index."""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _conv_cases as CC  # noqa: E402
import test_gpu_conv as TC  # noqa: E402
import test_gpu_conv_f32 as TC32  # noqa: E402
import test_gpu_flow_ops as TF  # noqa: E402
import test_gpu_flow_ops_grad as TG  # noqa: E402
import test_gpu_trunk_exec as TE  # noqa: E402
from _poison import _is_poison, poisoned  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd import driver, igemm, ops, trunk_f32  # noqa: E402


def _params(fn, argname):
    """The value list of `@pytest.mark.parametrize(argname, [...])` on an existing test: its shapes are reused, not restated."""
    for mark in fn.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == argname:
            return list(mark.args[1])
    raise KeyError(argname)


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def _flat(r):
    if torch.is_tensor(r):
        return [r]
    if r is None:
        return []
    out = []
    for v in r:
        out += _flat(v)
    return out


def _snap(r):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _flat(r)]


def _same(got, want, arena, what, close=()):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i)
        bad = int(torch.isnan(g).sum()) if g.is_floating_point() else 0
        if bad or not torch.equal(g, w):
            if i in close and not bad:
                TG._close(g, w)
                continue
            diff = int((g != w).sum())
            where = tuple(int(v) for v in (g != w).nonzero()[0]) if diff else None
            sites = arena.unwritten_sites() if arena is not None else []
            raise AssertionError(f"{what}: result {i} {list(g.shape)}: {bad} NaN, {diff} elements differ from the run on ordinary "
                                 f"buffers (first at {where}); allocations with unwritten elements:\n  " + "\n  ".join(sites[:40]))


def run_poisoned(build, call, a, b, check=None, close=(), what=""):
    """build() -> a fresh object; call(obj, *inputs) -> tensor(s).  `a`, `b`: two input tuples of one geometry."""
    want_a = _snap(call(build(), *a))
    want_b = _snap(call(build(), *b))
    with poisoned() as arena:
        obj = build()
        for tag, inputs, want in (("first call", a, want_a), ("second call, other inputs", b, want_b)):
            r = call(obj, *inputs)
            got = _snap(r)
            _same(got, want, arena, f"{what} {tag}", close)
            if check is not None:
                check(r)
            arena.check()
        assert arena.n_allocated > 0, "the case allocated nothing through the patched names: it tested nothing"
    return want_a


def _rand(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.randn(*shape) * scale).astype(np.float32)).cuda()


def _frames(rs, *shape):
    return torch.from_numpy(rs.randint(0, 256, shape).astype(np.float32)).cuda()


_TUNING_DEFAULTS = (0, 2001, 4000, 5000, 6001, 7000, 8000, 9001, 1128)


@contextlib.contextmanager
def _tuned(modes):
    """Kernel-selection switches of the cross-check library for the duration of a case (tests marked `xcheck`)."""
    lib = L.load()
    try:
        for m in modes:
            lib.vsr_conv2d_tuning(m)
        yield lib
    finally:
        for m in _TUNING_DEFAULTS:
            lib.vsr_conv2d_tuning(m)


def test_the_helper_sees_device_memory():
    """The helper's own test (tests/test_poison_helper.py) runs on the CPU; the same planted errors on the device: a kernel given
    one row fewer than its buffer holds leaves that row poisoned, a stray store (torch indexing on the raw block, not a kernel)
    is found in either band, and a well-behaved launch passes."""
    from _poison import PoisonError
    x = _rand(np.random.RandomState(0), 2, 3, 5, 7)
    with poisoned() as arena:
        out = torch.empty((2, 1, 5, 7), dtype=torch.float32, device="cuda")
        assert out.data_ptr() % 512 == 0 and bool(torch.isnan(out).all())
        L.check(L.load().vsr_channelnorm_f32(L.dptr(x[:1]), L.dptr(out), 1, 3, 5, 7, L.stream()))   # image 0 only
        assert arena.unwritten(out).shape[0] == 35 and arena.unwritten(out)[0].tolist() == [1, 0, 0, 0]
        with pytest.raises(PoisonError, match="35 of 70 elements were never written"):
            arena.assert_written(out)
        L.check(L.load().vsr_channelnorm_f32(L.dptr(x), L.dptr(out), 2, 3, 5, 7, L.stream()))
        arena.assert_written(out)
        assert torch.equal(out, ops.channelnorm(x))
        assert arena.check() == 2
        rec = arena.find(out)
        raw = rec.block.view(torch.float32)
        raw[rec.band // 4 + 70] = 1.0
        with pytest.raises(PoisonError, match="PAST the end.*first at byte offset 280 "):
            arena.check()
        rec.block[rec.band + 280:rec.band + 284] = 255
        arena.check()
        raw[rec.band // 4 - 1] = 1.0
        with pytest.raises(PoisonError, match="BEFORE the start.*nearest at byte offset -1 "):
            arena.check(release=True)
    assert torch.empty(1, device="cuda")._base is None


# ---------------------------------------------------------------------------------------------------------------------
# SR net
# ---------------------------------------------------------------------------------------------------------------------
_masters = {}


def _sr_master(scale):
    from video_super_resolution_amd import SRProjectionModule
    from video_super_resolution_amd.weights import fill_module_
    if ("sr", scale) not in _masters:
        _masters["sr", scale] = fill_module_(SRProjectionModule(upscale_factor=scale).eval(), seed=0, prefix="model.")
    return _masters["sr", scale]


def _sr_build(scale, precision):
    def build():
        m = copy.deepcopy(_sr_master(scale)).cuda().eval()
        m.precision = precision
        return m
    return build


def _sr_inputs(rs, h, w):
    x = _frames(rs, 8, 3, h, w)
    x2 = x.clone()
    x2[3:] = _frames(rs, 5, 3, h, w)
    return x, x2


SR_SIZES = [(1, 7), (2, 2), (9, 40), (37, 33), (37, 95)]


@pytest.mark.parametrize("hw", SR_SIZES)
@pytest.mark.parametrize("scale", [4, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_sr_forward_full_and_decimated(precision, scale, hw):
    """All eight planes: the full frame and the decimated tail (pass 1 of VSR.forward), default builds."""
    rs = np.random.RandomState(hw[0] * 31 + hw[1] + scale)

    def call(m, x, _):
        with torch.no_grad():
            return [m(x), m(x, decimate=True)]
    run_poisoned(_sr_build(scale, precision), call, _sr_inputs(rs, *hw), _sr_inputs(rs, *hw), what=f"SR {precision} x{scale} {hw}")


@pytest.mark.parametrize("hw", [(1, 7), (9, 40), (37, 33), (37, 95)])
@pytest.mark.parametrize("scale", [4, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("ahead", [False, True])
def test_sr_shared_planes(precision, scale, hw, ahead):
    """Two calls that share their first three planes: kept by the first call (`shared`), or evaluated ahead of both by
    `precompute_shared` on three planes (fp16: into the caller's live buffers, with the pre-fusion planes where a build exists)."""
    h, w = hw
    rs = np.random.RandomState(h * 17 + w + scale)

    def call(m, x, x2):
        with torch.no_grad():
            shared = {"n": 3}
            if ahead:
                live = None
                if precision == "fp16":
                    live = {k: torch.empty((8, h * w, 32), dtype=torch.float16, device="cuda") for k in (3, 6)}
                    if scale in (4, 2):
                        live["prefc"] = torch.empty((8, 3, scale * h, scale * w), dtype=torch.float32, device="cuda")
                m.precompute_shared(x[:3].contiguous(), shared, live)
            return [m(x, decimate=True, shared=shared), m(x2, shared=shared)]
    run_poisoned(_sr_build(scale, precision), call, _sr_inputs(rs, h, w), _sr_inputs(rs, h, w),
                 what=f"SR shared planes {precision} x{scale} {hw} ahead={ahead}")


# ---------------------------------------------------------------------------------------------------------------------
# fp16 trunk convolutions
# ---------------------------------------------------------------------------------------------------------------------
def _conv_operands(case, seed):
    N, cin, H, W, cout, k = case[:6]
    rs = np.random.RandomState(seed)
    w = torch.from_numpy((rs.randn(cout, cin, k, k) / np.sqrt(cin * k * k)).astype(np.float32)).cuda().half().float()
    b = _rand(rs, cout)
    return w, b, (_rand(rs, N, cin, H, W),), (_rand(rs, N, cin, H, W),)


def _pad_is_zero(cout):
    def check(r):
        out = _flat(r)[0]
        if out.shape[3] > cout:
            assert float(out[..., cout:].abs().max()) == 0.0, "padding channels are not zero"
    return check


def _hconv_case(case, what):
    """(N, Cin, H, W, Cout, k, stride, pad, act) through igemm.HConv, input converted by to_nhwc_half inside the call."""
    N, cin, H, W, cout, k, s, p, act = case
    w, b, xa, xb = _conv_operands(case, cin * 7 + cout + k)
    run_poisoned(lambda: igemm.HConv(w, b, stride=s, pad=p, act=act), lambda conv, x: conv(igemm.to_nhwc_half(x)), xa, xb,
                 check=_pad_is_zero(cout), what=f"{what} {case}")


@pytest.mark.parametrize("case", TC.CASES + [c for c in TC.TILE_CASES if c not in TC.CASES])
def test_conv_default_route(case):
    _hconv_case(case, "HConv")


def _slice_case(case, fill):
    """The same layer reading a channel slice of a wider map and writing a channel slice of a wider map: [32, 32 + cin_pad) of an
    input with 32 channels on either side, [32, 32 + cout) of an output whose row is 32 channels longer than needed.  What lies
    outside the slices holds `fill` (ordinary run) or poison: it must be neither read into the result nor written."""
    N, cin, H, W, cout, k, s, p, act = case
    w, b, xa, xb = _conv_operands(case, cin * 5 + cout)
    cp = igemm.pad32(cin)
    ld = igemm.pad32(32 + cout) + 32

    def call(conv, x):
        Ho, Wo = conv.out_hw(H, W)
        wide = torch.empty((N, H, W, cp + 64), dtype=torch.float16, device="cuda")
        dst = torch.empty((N, Ho, Wo, ld), dtype=torch.float16, device="cuda")
        if fill is not None:
            wide.fill_(fill)
            dst.fill_(fill)
        wide[..., 32:32 + cp] = igemm.to_nhwc_half(x)
        conv(wide, out=dst, out_coff=32, in_coff=32)
        return dst
    return w, b, xa, xb, call


@pytest.mark.parametrize("case", TC.CASES)
def test_conv_channel_slices(case):
    N, cin, H, W, cout, k, s, p, act = case
    w, b, xa, xb, call = _slice_case(case, 3.0)
    build = lambda: igemm.HConv(w, b, stride=s, pad=p, act=act)   # noqa: E731
    want = call(build(), *xa)
    torch.cuda.synchronize()
    rest = torch.cat([want[..., :32], want[..., 32 + cout:]], 3)
    assert bool((rest == 3.0).all()), "channels outside the slice were written"
    _, _, _, _, pcall = _slice_case(case, None)
    with poisoned() as arena:
        for x in (xa, xb):
            got = pcall(build(), *x)
            torch.cuda.synchronize()
            rest = torch.cat([got[..., :32], got[..., 32 + cout:]], 3)
            assert bool(_is_poison(rest).all()), "channels outside the slice were written"
            live = got[..., 32:32 + cout]
            assert not bool(torch.isnan(live).any()), f"{int(torch.isnan(live).sum())} NaN: memory outside the input slice was consumed"
            assert torch.equal(live, call(build(), *x)[..., 32:32 + cout])
            arena.check()


FORCED = {   # name -> (vsr_conv2d_tuning switches, the shape list of the value test that forces the same route)
    "first_gather_build": ((8,), TC.CASES),
    "gather_128_channel_tiles": ((10,), TC.CASES),
    "gather_64_channel_tiles": ((11,), TC.CASES),
    "tile": ((2003,), TC.TILE_CASES),
    "tile_without_split_k": ((2003, 5001, 1000), TC.TILE_CASES),
    "gather_without_split_k": ((5001, 1000, 2000, 1), TC.TILE_CASES),
    "five_set_ring": ((2000, 1, 8002), _params(TC.test_gather_kernel_five_set_ring, "case")),
}
PATCH_FORCED = {   # (N, Cin, H, W, Cout, k, act) lists: stride 1, pad k // 2
    "patch": ((2,), _params(TC.test_patch_kernels_match_torch, "case")),
    "patch_without_r8": ((6,), _params(TC.test_patch_kernels_match_torch, "case")),
    "patch_plain": ((7,), _params(TC.test_patch_kernels_match_torch, "case")),
    "patch_layers_on_gather": ((1,), _params(TC.test_patch_kernels_match_torch, "case")),
    "patch_lw": ((2, 2000, 6002), _params(TC.test_patch_kernel_with_weights_in_lds, "case")),
    "patch_r8": ((2, 2000, 6000), _params(TC.test_patch_kernel_with_weights_in_lds, "case")),
    "patch_pf_64": ((2, 2000, 9002), _params(TC.test_patch_kernel_persistent_prefetching, "case")),
    "patch_pf_32": ((2, 2000, 9003), _params(TC.test_patch_kernel_persistent_prefetching, "case")),
}


@pytest.mark.xcheck
@pytest.mark.parametrize("route,case", [(r, c) for r, (_, cases) in FORCED.items() for c in cases])
def test_conv_forced_route(route, case):
    with _tuned(FORCED[route][0]):
        _hconv_case(case, route)


@pytest.mark.xcheck
@pytest.mark.parametrize("route,case", [(r, c) for r, (_, cases) in PATCH_FORCED.items() for c in cases])
def test_conv_forced_patch_route(route, case):
    N, cin, H, W, cout, k, act = case
    with _tuned(PATCH_FORCED[route][0]):
        _hconv_case((N, cin, H, W, cout, k, 1, k // 2, act), route)


def _stem_case(case):
    N, cin, H, W, cout, k, s, p, act = case
    w, b, xa, xb = _conv_operands(case, cout + k)
    run_poisoned(lambda: igemm.HConvStem(w, b, stride=s, pad=p, act=act), lambda conv, x: conv(igemm.to_nhwc_half(x, 4)), xa, xb,
                 check=_pad_is_zero(cout), what=f"HConvStem {case}")


@pytest.mark.parametrize("case", _params(TC.test_stem_conv_matches_torch, "case"))
def test_stem_conv(case):
    _stem_case(case)


def _pair_case(case):
    N, cin, H, W, cout, k, pad = case
    w, b, xa, xb = _conv_operands(case, cin + k + W)
    run_poisoned(lambda: igemm.HConvPairS2(w, b, pad=pad, act=igemm.ACT_LEAKY, slope=0.1), lambda conv, x: conv(igemm.to_nhwc_half(x, 16)),
                 xa, xb, check=_pad_is_zero(cout), what=f"HConvPairS2 {case}")


@pytest.mark.parametrize("case", _params(TC.test_pair_conv_stride2, "case"))
def test_pair_conv_stride2(case):
    _pair_case(case)


def _deconv_case(shape, what):
    N, cin, H, W, cout = shape
    rs = np.random.RandomState(cin)
    w = torch.from_numpy((rs.randn(cin, cout, 4, 4) / np.sqrt(cin * 4)).astype(np.float32)).cuda().half().float()
    b = _rand(rs, cout)
    run_poisoned(lambda: igemm.HDeconv4s2(w, b, act=igemm.ACT_LEAKY), lambda dc, x: dc(igemm.to_nhwc_half(x)),
                 (_rand(rs, N, cin, H, W),), (_rand(rs, N, cin, H, W),), check=_pad_is_zero(cout), what=f"{what} {shape}")


@pytest.mark.parametrize("shape", _params(TC.test_transposed_conv_k4s2, "shape"))
def test_transposed_conv_k4s2(shape):
    _deconv_case(shape, "HDeconv4s2")


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", _params(TC.test_transposed_conv_k4s2, "shape"))
@pytest.mark.parametrize("route", ["tile", "gather"])
def test_transposed_conv_k4s2_forced_route(shape, route):
    if route == "tile" and shape[4] <= 32:
        return   # (no tile build below 64 out-channels: the value test forces it from there too)
    with _tuned((2003,) if route == "tile" else (1,)):
        _deconv_case(shape, f"HDeconv4s2 {route}")


@pytest.mark.xcheck
@pytest.mark.parametrize("i", range(len(CC.BUILD_CASES)))
def test_conv_production_builds(i):
    """tests/_conv_cases.py BUILD_CASES: one case per kernel build that the trunks launch and no list above reaches (kept complete by
    tests/test_conv_build_census.py), through the runner of its entry; the launch takes the route the census planned for the row."""
    import test_conv_build_census as census
    kind, shape, modes, (act, _) = CC.BUILD_CASES[i]
    with _tuned(modes):
        if kind == CC.CONV:
            _hconv_case(shape + (act,), "production build")
        elif kind == CC.STEM:
            _stem_case(shape + (act,))
        elif kind == CC.PAIR:
            _pair_case(shape[:6] + (shape[7],))
        else:
            _deconv_case(shape, "production build")
        route = L.load().vsr_last_route().decode()
    kh, stride = (2, 1) if kind == CC.DECONV else shape[5:7]
    assert census.build_key(route, kh, stride) == census.case_keys([CC.BUILD_CASES[i]])[0], route


@pytest.mark.xcheck
@pytest.mark.parametrize("case", _params(TC.test_conv1x1_transposing_build, "case"))
@pytest.mark.parametrize("mode", [7001, 7000])
def test_conv1x1_builds_into_a_slice(case, mode):
    """k_conv1x1_t / k_conv1x1_stream into a channel slice of a row that is longer than the slice: the rest stays as it was."""
    N, H, W, cout, act, extra, coff = case
    rs = np.random.RandomState(H + cout)
    w = torch.from_numpy((rs.randn(cout, 128, 1, 1) / np.sqrt(128)).astype(np.float32)).cuda().half().float()
    b = _rand(rs, cout)
    ld = igemm.pad32(coff + cout) + extra

    def call(conv, x, fill):
        dst = torch.empty((N, H, W, ld), dtype=torch.float16, device="cuda")
        if fill is not None:
            dst.fill_(fill)
        conv(igemm.to_nhwc_half(x), out=dst, out_coff=coff)
        return dst
    build = lambda: igemm.HConv(w, b, stride=1, pad=0, act=act)   # noqa: E731
    with _tuned((mode,)):
        with poisoned() as arena:
            for _ in range(2):
                x = _rand(rs, N, 128, H, W)
                got = call(build(), x, None)
                torch.cuda.synchronize()
                live = got[..., coff:coff + cout]
                rest = torch.cat([got[..., :coff], got[..., coff + cout:]], 3)
                assert not bool(torch.isnan(live).any())
                assert rest.numel() == 0 or bool(_is_poison(rest).all()), "channels outside the slice were written"
                assert torch.equal(live, call(build(), x, 3.0)[..., coff:coff + cout])
                arena.check(release=True)


@pytest.mark.parametrize("case", _params(TC.test_flow_head_matches_torch, "case"))
def test_flow_head(case):
    N, cin, H, W, extra, with_up, up_bias = case
    rs = np.random.RandomState(cin + H)
    ld = igemm.pad32(cin) + extra
    wp = torch.from_numpy((rs.randn(2, cin, 3, 3) / np.sqrt(9 * cin)).astype(np.float32)).cuda().half().float()
    bp = _rand(rs, 2)
    wu = _rand(rs, 2, 2, 4, 4, scale=0.3).half().float() if with_up else None
    bu = _rand(rs, 2) if (with_up and up_bias) else None

    def operand():
        return (_rand(rs, N, H, W, cin).half(),)

    def call(head, xl):
        x = torch.empty((N, H, W, ld), dtype=torch.float16, device="cuda")   # beyond the slice: poison (must not be read)
        x[..., :igemm.pad32(cin)] = 0
        x[..., :cin] = xl
        up_out = torch.zeros((N, 2 * H, 2 * W, 32), dtype=torch.float16, device="cuda") if with_up else None
        flow = head(x, up_out=up_out, up_coff=6)
        return [flow, up_out]

    def check(r):
        assert float(r[0][..., 2:].abs().max()) == 0.0
        if with_up:
            assert float(r[1][..., :6].abs().max()) == 0.0 and float(r[1][..., 8:].abs().max()) == 0.0
    run_poisoned(lambda: igemm.HFlowHead(wp, bp, wu, bu), call, operand(), operand(), check=check, what=f"HFlowHead {case}")


@pytest.mark.parametrize("shape", _params(TE.test_hourglass_fused_front, "shape"))
def test_hourglass_front(cpu_vsr, shape):
    """igemm.HHourglassFront: stem map, pooled map and the fused 1x1s' slice, every output buffer poisoned."""
    from video_super_resolution_amd.trunk_exec import HourglassExec
    N, h, w = shape
    rs = np.random.RandomState(h + w)
    netg = copy.deepcopy(cpu_vsr.DepthModule.model.netG).cuda().eval()

    def call(ex, fr):
        inc = ex.prog[1][1][1][0][1][1][1][0][1]
        c2 = inc.first.cout
        x4 = torch.empty((N, h, w, 4), dtype=torch.float16, device="cuda")
        x4[..., :3] = fr
        x4[..., 3] = 0
        buf = torch.empty((N, h, w, inc.width), dtype=torch.float16, device="cuda")
        pooled = torch.empty((N, h // 2, w // 2, 128), dtype=torch.float16, device="cuda")
        smap = torch.empty((N, h, w, 128), dtype=torch.float16, device="cuda")
        ex.front(x4, buf, pooled, smap)
        return [buf[..., :c2], pooled, smap]
    run_poisoned(lambda: HourglassExec(netg), call, (_frames(rs, N, h, w, 3),), (_frames(rs, N, h, w, 3),), what=f"hg_front {shape}")


@pytest.mark.parametrize("shape", _params(TC.test_pool2x2, "shape") + [(2, 3, 3, 32), (1, 2, 2, 16)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pool2x2(shape, mode):
    N, H, W, C = shape
    rs = np.random.RandomState(H + W + mode)
    run_poisoned(lambda: None, lambda _, x: igemm.pool2x2(x, 0, C, mode), (_rand(rs, N, H, W, C).half(),), (_rand(rs, N, H, W, C).half(),),
                 what=f"pool2x2 {shape} mode {mode}")


RESIZE_ADD_CASES = [   # (N, Ha, Wa, H, W, c, segments of a, with b, up2, b_up2)
    (2, 17, 23, 34, 46, 64, 4, True, False, False), (1, 33, 30, 67, 61, 64, 1, True, False, False), (1, 9, 11, 18, 22, 32, 2, False, True, False),
    (2, 8, 15, 33, 60, 64, 4, True, True, False), (1, 67, 120, 134, 240, 64, 4, True, False, True), (1, 1, 7, 3, 14, 16, 1, True, False, False),
    (1, 5, 1, 10, 1, 8, 1, False, False, False)]


@pytest.mark.parametrize("case", RESIZE_ADD_CASES)
def test_resize_add(case):
    """igemm.resize_add (the hourglass's AddResized / UpsamplingNearest2d in one pass): plain slices and SegMaps, odd sizes, a
    skip arm resized onto a doubled arm, one-row and one-column maps."""
    N, Ha, Wa, H, W, c, nseg, with_b, up2, b_up2 = case
    rs = np.random.RandomState(Ha + W + c)

    def operands():
        a = [_rand(rs, N, Ha, Wa, c // nseg + 8).half() for _ in range(nseg)]
        hb, wb = (H // 2, W // 2) if b_up2 else (H, W)
        return a, (_rand(rs, N, hb, wb, c + 16).half() if with_b else None)

    def call(_, a, b):
        src = igemm.SegMap([(t, 8) for t in a]) if nseg > 1 else a[0]
        return igemm.resize_add(src, 8, c, (H, W), b, 16, up2=up2, b_up2=b_up2)
    run_poisoned(lambda: None, call, operands(), operands(), what=f"resize_add {case}")


@pytest.mark.parametrize("shape", _params(TC.test_nchw_f32_to_nhwc_f16, "shape") + [(1, 3, 1, 9, None), (1, 5, 9, 1, 16)])
def test_layout_conversion(shape):
    N, C, H, W, cp = shape
    rs = np.random.RandomState(C + H)

    def check(out):
        assert float(out[..., C:].abs().max() if out.shape[3] > C else 0.0) == 0.0
    run_poisoned(lambda: None, lambda _, x: igemm.to_nhwc_half(x, cp), (_rand(rs, N, C, H, W, scale=100),), (_rand(rs, N, C, H, W, scale=100),),
                 check=check, what=f"to_nhwc_half {shape}")


@pytest.mark.parametrize("shape", _params(TC.test_flownetc_cost_volume_mfma, "shape"))
def test_flownetc_cost_volume(shape):
    """The MFMA cost volume writes channels [32, 473) of a 480-channel row and nothing else."""
    B, H, W, C = shape
    rs = np.random.RandomState(H * W)

    def call(_, a, b, fill=None):
        out = torch.empty((B, H, W, 480), dtype=torch.float16, device="cuda")
        if fill is not None:
            out.fill_(fill)
        L.check(L.load().vsr_flownetc_corr_nhwc_f16(L.dptr(a, torch.float16), L.dptr(b, torch.float16), L.dptr(out, torch.float16), 480, 32,
                                                    B, H, W, C, L.stream()))
        return out
    with poisoned() as arena:
        for _ in range(2):
            a, b = _rand(rs, B, H, W, C).half(), _rand(rs, B, H, W, C).half()
            got = call(None, a, b)
            torch.cuda.synchronize()
            assert bool(_is_poison(got[..., :32]).all()) and bool(_is_poison(got[..., 473:]).all()), "channels outside the slice were written"
            assert not bool(torch.isnan(got[..., 32:473]).any())
            assert torch.equal(got[..., 32:473], call(None, a, b, 7.0)[..., 32:473])
            arena.check()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 trunk convolutions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(TC32.test_conv2d_f32_matches_float64, "case"))
def test_conv2d_f32(case, monkeypatch):
    monkeypatch.setattr(trunk_f32, "ROUTE", False)   # every shape through the own kernel
    N, C, H, W, Co, k, stride, pad, bias = case
    rs = np.random.RandomState(C + 7 * Co + k)
    master = trunk_f32.Conv2dF32(C, Co, k, stride, pad, bias=bias)
    with torch.no_grad():
        master.weight.copy_(torch.from_numpy((rs.randn(Co, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)))
        if bias:
            master.bias.copy_(torch.from_numpy(rs.randn(Co).astype(np.float32)))

    def call(m, x):
        with torch.no_grad():
            return m(x)
    run_poisoned(lambda: copy.deepcopy(master).cuda(), call, (_rand(rs, N, C, H, W),), (_rand(rs, N, C, H, W),), what=f"Conv2dF32 {case}")


@pytest.mark.parametrize("case", _params(TC32.test_conv_transpose_k4s2_f32_matches_float64, "case"))
def test_conv_transpose_k4s2_f32(case, monkeypatch):
    monkeypatch.setattr(trunk_f32, "ROUTE", False)
    N, C, H, W, Co, bias = case
    rs = np.random.RandomState(C + Co)
    master = trunk_f32.ConvTranspose2dF32(C, Co, 4, 2, 1, bias=bias)
    with torch.no_grad():
        master.weight.copy_(torch.from_numpy((rs.randn(C, Co, 4, 4) / np.sqrt(4 * C)).astype(np.float32)))
        if bias:
            master.bias.copy_(torch.from_numpy(rs.randn(Co).astype(np.float32)))

    def call(m, x):
        with torch.no_grad():
            return m(x)
    run_poisoned(lambda: copy.deepcopy(master).cuda(), call, (_rand(rs, N, C, H, W),), (_rand(rs, N, C, H, W),),
                 what=f"ConvTranspose2dF32 {case}")


@pytest.mark.parametrize("case", _params(TC32.test_conv2d_f32_spatial_kernels_match_float64, "case"))
@pytest.mark.parametrize("route", [2, 1])
def test_conv2d_f32_fused_epilogue_into_a_concat_slice(case, route):
    """vsr_conv2d_act_nchw_f32 with the folded BatchNorm / activation epilogue writing channels [coff, coff + Co) of a `ctot`-channel
    buffer: the other channels keep the poison."""
    N, C, H, W, Co, kh, kw, py, px, ctot, coff, bn, slope = case
    rs = np.random.RandomState(C + 7 * Co + kh)
    w = torch.from_numpy((rs.randn(Co, C, kh, kw) / np.sqrt(C * kh * kw)).astype(np.float32)).cuda()
    scale = (_rand(rs, Co).abs() + 0.5) if bn else None
    shift = _rand(rs, Co)
    Ho, Wo = H + 2 * py - kh + 1, W + 2 * px - kw + 1

    def call(x, fill):
        wp = trunk_f32._pack(w.contiguous())
        out = torch.empty((N, ctot, Ho, Wo), dtype=torch.float32, device="cuda")
        if fill is not None:
            out.fill_(fill)
        trunk_f32.conv2d_fused(x, wp, scale, shift, slope is not None, slope or 0.0, Co, kh, kw, 1, py, px, route, out=out, coff=coff)
        return out
    with poisoned() as arena:
        for _ in range(2):
            x = _rand(rs, N, C, H, W)
            got = call(x, None)
            torch.cuda.synchronize()
            live = got[:, coff:coff + Co]
            rest = torch.cat([got[:, :coff], got[:, coff + Co:]], 1)
            assert not bool(torch.isnan(live).any())
            assert rest.numel() == 0 or bool(_is_poison(rest).all()), "channels outside the slice were written"
            assert torch.equal(live, call(x, 7.0)[:, coff:coff + Co])
            arena.check()


def test_fused_sequential_and_concat_f32(monkeypatch):
    """depth.ChannelConcat / FusedSequential: branches written into the concat buffer in place (a torch.empty of the sum of widths)."""
    from video_super_resolution_amd import depth
    monkeypatch.setattr(trunk_f32, "MIN_TILES", 0)
    monkeypatch.setattr(trunk_f32, "MIN_WGS", 0)
    torch.manual_seed(3)
    blk = depth._build(depth._J).eval()
    seq = depth._build(("S", [("conv", 3, 128, 7, 3), ("bn", 128, True), "relu", depth._J, ("conv", 64, 1, 3, 1)])).eval()
    with torch.no_grad():
        for m in list(blk.modules()) + list(seq.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    rs = np.random.RandomState(3)

    def call(ms, x, img):
        with torch.no_grad():
            return [ms[0](x), ms[1](img)]
    run_poisoned(lambda: (copy.deepcopy(blk).cuda(), copy.deepcopy(seq).cuda()), call, (_rand(rs, 2, 128, 37, 45), _rand(rs, 1, 3, 40, 70)),
                 (_rand(rs, 2, 128, 37, 45), _rand(rs, 1, 3, 40, 70)), what="depth blocks fp32")


# ---------------------------------------------------------------------------------------------------------------------
# executors
# ---------------------------------------------------------------------------------------------------------------------
EXEC_SIZES = [(64, 96), (72, 88), (70, 90), (135, 240)]   # the last one is above the 8192-pixel routing threshold


def _own_kernels_at_small_sizes(monkeypatch, hw):
    """The float32 router keeps launches of a few workgroups on the stock operator (trunk_f32.MIN_TILES / MIN_WGS); below the
    8192-pixel threshold the floors are removed, as the value tests do, so that the own kernels run at the ragged small sizes
    too.  The large size runs the routing as shipped."""
    if hw[0] * hw[1] < 8192 * 2:
        monkeypatch.setattr(trunk_f32, "MIN_TILES", 0)
        monkeypatch.setattr(trunk_f32, "MIN_WGS", 0)


def _no_grad_call(f):
    def call(obj, *inputs):
        with torch.no_grad():
            return f(obj, *inputs)
    return call


@pytest.mark.parametrize("hw", EXEC_SIZES)
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_hourglass(cpu_vsr, hw, precision, monkeypatch):
    if precision == "fp32":
        _own_kernels_at_small_sizes(monkeypatch, hw)
    from video_super_resolution_amd.trunk_exec import HourglassExec
    rs = np.random.RandomState(hw[0])
    master = cpu_vsr.DepthModule.model.netG
    if precision == "fp16":
        build, call = (lambda: HourglassExec(copy.deepcopy(master).cuda().eval())), (lambda ex, fr: ex(fr))
    else:
        build, call = (lambda: copy.deepcopy(master).cuda().eval()), (lambda net, fr: net(fr.permute(0, 3, 1, 2)))
    run_poisoned(build, _no_grad_call(call), (_frames(rs, 2, *hw, 3),), (_frames(rs, 2, *hw, 3),), what=f"hourglass {precision} {hw}")


@pytest.mark.parametrize("hw", [(64, 128), (128, 192)])   # (multiples of 64: FlowNet2's own constraint; 128 x 192 is above the threshold)
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_flownet2(cpu_vsr, hw, precision, monkeypatch):
    if precision == "fp32":
        _own_kernels_at_small_sizes(monkeypatch, hw)
    from video_super_resolution_amd.trunk_exec import FlowNet2Exec
    rs = np.random.RandomState(hw[1])
    master = cpu_vsr.FlowModule.net
    if precision == "fp16":
        build = lambda: FlowNet2Exec(copy.deepcopy(master).cuda().eval())   # noqa: E731
    else:
        build = lambda: copy.deepcopy(master).cuda().eval()   # noqa: E731
    run_poisoned(build, _no_grad_call(lambda net, x: net(x)), (_frames(rs, 2, 3, 2, *hw),), (_frames(rs, 2, 3, 2, *hw),),
                 what=f"FlowNet2 {precision} {hw}")


@pytest.mark.parametrize("hw", EXEC_SIZES)
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_osvos(cpu_vsr, hw, precision, monkeypatch):
    if precision == "fp32":
        _own_kernels_at_small_sizes(monkeypatch, hw)
    from video_super_resolution_amd.trunk_exec import OSVOSExec
    rs = np.random.RandomState(hw[0] + 1)
    master = cpu_vsr.VOSModule.net
    if precision == "fp16":
        build = lambda: OSVOSExec(copy.deepcopy(master).cuda().eval())   # noqa: E731
    else:
        build = lambda: copy.deepcopy(master).cuda().eval()   # noqa: E731
    run_poisoned(build, _no_grad_call(lambda net, x: net(x)), (_frames(rs, 2, 3, *hw) - 110.0,), (_frames(rs, 2, 3, *hw) - 110.0,),
                 what=f"OSVOS {precision} {hw}")


# ---------------------------------------------------------------------------------------------------------------------
# flow operators and glue
# ---------------------------------------------------------------------------------------------------------------------
THIN = [(1, 3, 1, 9), (2, 3, 9, 1)]   # H = 1, W = 1


@pytest.mark.parametrize("shape,scale", _params(TF.test_resample2d_bit_exact, "shape,scale") + [(s, 3.0) for s in THIN])
@pytest.mark.parametrize("bilinear", [True, False])
def test_resample2d(shape, scale, bilinear):
    B, C, H, W = shape
    rs = np.random.RandomState(H + W)
    mk = lambda: (_rand(rs, B, C, H, W), _rand(rs, B, 2, H, W, scale=scale))   # noqa: E731
    run_poisoned(lambda: None, lambda _, img, flow: ops.resample2d(img, flow, 1, bilinear), mk(), mk(), what=f"resample2d {shape}")


@pytest.mark.parametrize("shape", _params(TF.test_channelnorm_bit_exact, "shape") + THIN)
def test_channelnorm(shape):
    rs = np.random.RandomState(sum(shape))
    run_poisoned(lambda: None, lambda _, x: ops.channelnorm(x), (_rand(rs, *shape),), (_rand(rs, *shape),), what=f"channelnorm {shape}")


@pytest.mark.parametrize("shape,geom", TG.GEOMS)
def test_correlation(shape, geom):
    rs = np.random.RandomState(shape[3])
    mk = lambda: (_rand(rs, *shape), _rand(rs, *shape))   # noqa: E731
    run_poisoned(lambda: None, lambda _, a, b: ops.correlation(a, b, **geom), mk(), mk(), what=f"correlation {shape}")


@pytest.mark.parametrize("shape", [(2, 33, 47), (1, 64, 128), (1, 1, 9), (2, 9, 1)])
def test_warp_concat_and_norms(shape):
    B, H, W = shape
    rs = np.random.RandomState(H + W)
    mk = lambda: (_rand(rs, B, 6, H, W), _rand(rs, B, 2, H, W, scale=6))   # noqa: E731
    run_poisoned(lambda: None, lambda _, x6, flow: [ops.warp_concat(x6, flow, 20.0), ops.warp_norms(x6, flow)], mk(), mk(),
                 what=f"warp_concat / warp_norms {shape}")


@pytest.mark.parametrize("hw", [(40, 56), (256, 384), (1, 9), (9, 1), (33, 47)])
def test_flow2img(hw):
    """Planar and NHWC-half inputs; the entries' 16-byte workspace (two unsigned words the entry zeroes, not an address) is
    poisoned too."""
    h, w = hw
    rs = np.random.RandomState(h + w)

    def mk():
        m = torch.zeros((h, w, 32), dtype=torch.float16, device="cuda")
        m[..., :2] = _rand(rs, h, w, 2, scale=5).half()
        return (m,)

    def call(_, m):
        return [ops.flow2img(m[..., :2].permute(2, 0, 1).float()), ops.flow2img_nhwc(m)]
    a, b = mk(), mk()
    want = [_snap(call(None, *a)), _snap(call(None, *b))]
    with poisoned(extra_dtypes=(torch.int32,)) as arena:
        for inputs, wnt in zip((a, b), want):
            got = _snap(call(None, *inputs))
            _same(got, wnt, arena, f"flow2img {hw}")
            assert torch.equal(got[0], got[1])
            arena.check()
        assert any(r.dtype is torch.int32 and r.nbytes == 16 for r in arena.records)


def test_prepare_pairs():
    rs = np.random.RandomState(11)
    y0, x0, H, W = 3, 3, 64, 128
    B = 2

    def call(_, frames):
        x = torch.empty((B, 6, H, W), device="cuda")
        x6 = torch.empty((B, H, W, 32), dtype=torch.float16, device="cuda")
        both = torch.empty((2 * B, H, W, 4), dtype=torch.float16, device="cuda")
        ws = torch.empty(B * 128 * 3, device="cuda")
        L.check(L.load().vsr_flownet_prepare_pairs(L.dptr(frames), 3, 70, 134, (ctypes.c_int * B)(0, 1), (ctypes.c_int * B)(1, 2), B, y0, x0,
                                                   H, W, L.dptr(ws), L.dptr(x), L.dptr(x6, torch.float16), L.dptr(both, torch.float16),
                                                   L.stream()))
        return [x, x6, both]

    def check(r):
        assert not r[1][..., 6:].any() and not r[2][..., 3].any(), "padding channels are not zero"
    run_poisoned(lambda: None, call, (_frames(rs, 3, 70, 134, 3),), (_frames(rs, 3, 70, 134, 3),), check=check, what="prepare_pairs")


def _flow_maps(rs, B, H, W):
    x = _rand(rs, B, 6, H, W, scale=0.3)
    f2 = torch.zeros((B, H // 4, W // 4, 32), dtype=torch.float16, device="cuda")
    f2[..., :2] = _rand(rs, B, H // 4, W // 4, 2, scale=8.0).half()
    g2 = torch.zeros_like(f2)
    g2[..., :2] = _rand(rs, B, H // 4, W // 4, 2, scale=30).half()
    return x, f2, g2


@pytest.mark.xcheck
@pytest.mark.parametrize("shape", [(2, 64, 128), (1, 36, 200), (2, 132, 76), (1, 4, 8)])
@pytest.mark.parametrize("bilinear", [1, 0])
@pytest.mark.parametrize("variant", [1, 0])
def test_up_warp_concat16(shape, bilinear, variant):
    """Both builds of the warp (gather, the default; LDS-staged): 12 live channels of 16, the other four zero."""
    B, H, W = shape
    rs = np.random.RandomState(H + W + bilinear)
    lib = L.load()

    def call(_, x, f2, g2):
        out16 = torch.empty((B, H, W, 16), dtype=torch.float16, device="cuda")
        L.check(lib.vsr_flownet_up_warp_concat16_f16(L.dptr(x), L.dptr(f2, torch.float16), 32, bilinear, L.cf(20.0), L.cf(1 / 20.0),
                                                     L.dptr(out16, torch.float16), B, H, W, L.stream()))
        return out16

    def check(out16):
        assert not out16[..., 12:].any(), "padding channels are not zero"
    try:
        L.check(lib.vsr_flownet_warp_variant(variant))
        run_poisoned(lambda: None, call, _flow_maps(rs, B, H, W), _flow_maps(rs, B, H, W), check=check, what=f"up_warp_concat16 {shape}")
    finally:
        lib.vsr_flownet_warp_variant(1)


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 36, 200), (1, 4, 8)])
def test_fusion_input(shape):
    B, H, W = shape
    rs = np.random.RandomState(H + W)

    def call(_, x, f2, g2):
        out32 = torch.empty((B, H, W, 32), dtype=torch.float16, device="cuda")
        L.check(L.load().vsr_flownet_fusion_input_f16(L.dptr(x), L.dptr(g2, torch.float16), 32, L.dptr(f2, torch.float16), 32, L.cf(20.0),
                                                      L.dptr(out32, torch.float16), B, H, W, L.stream()))
        return out32

    def check(out32):
        assert not out32[..., 11:].any(), "padding channels are not zero"
    run_poisoned(lambda: None, call, _flow_maps(rs, B, H, W), _flow_maps(rs, B, H, W), check=check, what=f"fusion_input {shape}")


@pytest.mark.parametrize("hw", [(66, 70), (33, 47), (1, 9), (9, 1)])
@pytest.mark.parametrize("first_call", [True, False])
def test_assemble_planes_and_resize_estimate(hw, first_call):
    from video_super_resolution_amd.vsr import VSR
    h, w = hw
    rs = np.random.RandomState(14 + h)

    def mk():
        d = _frames(rs, 3, h, w, 3)
        pics = _frames(rs, 2, 64, 64, 3)
        z = [_rand(rs, 1, 1, h, w) for _ in range(3)]
        prev = _frames(rs, 1, 4 * h, 4 * w, 3)
        mask = (torch.from_numpy(rs.rand(h, w).astype(np.float32)).cuda() > 0.5).float()
        return d, pics, z, prev, mask

    def call(_, d, pics, z, prev, mask):
        if first_call:
            return VSR._assemble(d, pics, z)
        est = torch.empty((3, h, w), device="cuda")
        est_hw3 = torch.empty((h, w, 3), device="cuda")
        L.check(L.load().vsr_resize_estimate_f32(L.dptr(prev), 4 * h, 4 * w, L.dptr(est), L.dptr(est_hw3), h, w, L.stream()))
        return [est, est_hw3, VSR._assemble(d, pics, z, est, mask)]
    run_poisoned(lambda: None, call, mk(), mk(), what=f"assemble_planes {hw}")


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def _grads(out, leaves, gout):
    return list(torch.autograd.grad(out, leaves, gout))


@pytest.mark.parametrize("shape", _params(TG.test_resample2d_gradients, "shape") + THIN)
@pytest.mark.parametrize("bilinear", [True, False])
@pytest.mark.parametrize("which", ["img", "flow", "both"])
def test_grad_resample2d(shape, bilinear, which):
    B, C, H, W = shape
    rs = np.random.RandomState(H * W)
    mk = lambda: (_rand(rs, B, C, H, W), _rand(rs, B, 2, H, W, scale=4.0), _rand(rs, B, C, H, W))   # noqa: E731

    def call(_, img, flow, gout):
        img, flow = TG._leaf(img), TG._leaf(flow)
        out = ops.resample2d(img, flow, 1, bilinear)
        return [out] + _grads(out, {"img": [img], "flow": [flow], "both": [img, flow]}[which], gout)
    # the image gradient is a scatter of float atomic adds: order-dependent in its last bits (the bar of its own test)
    run_poisoned(lambda: None, call, mk(), mk(), close=(1,) if which != "flow" else (), what=f"grad_resample2d {shape} {which}")


@pytest.mark.parametrize("shape", _params(TG.test_channelnorm_gradient, "shape") + THIN)
def test_grad_channelnorm(shape):
    rs = np.random.RandomState(sum(shape))
    mk = lambda: (_rand(rs, *shape), _rand(rs, shape[0], 1, *shape[2:]))   # noqa: E731

    def call(_, x, gout):
        x = TG._leaf(x)
        out = ops.channelnorm(x)
        return [out] + _grads(out, [x], gout)
    run_poisoned(lambda: None, call, mk(), mk(), what=f"grad_channelnorm {shape}")


@pytest.mark.parametrize("shape,geom", TG.GEOMS)
@pytest.mark.parametrize("which", ["f1", "f2", "both"])
def test_grad_correlation(shape, geom, which):
    rs = np.random.RandomState(shape[3] + 1)
    oc, oh, ow = ops.correlation_out_shape(shape[2], shape[3], geom["pad_size"], geom["kernel_size"], geom["max_displacement"],
                                           geom["stride1"], geom["stride2"])
    mk = lambda: (_rand(rs, *shape), _rand(rs, *shape), _rand(rs, shape[0], oc, oh, ow))   # noqa: E731

    def call(_, f1, f2, gout):
        f1, f2 = TG._leaf(f1), TG._leaf(f2)
        out = ops.correlation(f1, f2, **geom)
        return [out] + _grads(out, {"f1": [f1], "f2": [f2], "both": [f1, f2]}[which], gout)
    run_poisoned(lambda: None, call, mk(), mk(), what=f"grad_correlation {shape} {which}")


@pytest.mark.parametrize("hw", [(10, 12), (7, 9)])
@pytest.mark.parametrize("scale", [4, 2])
def test_sr_train_step(hw, scale):
    """sr_train.forward_train + backward on the full SR net: every output, saved map, gradient and workspace (`*_ws_floats`) of
    csrc/sr_train.hip is a torch.empty."""
    rs = np.random.RandomState(hw[0] + scale)

    def build():
        m = copy.deepcopy(_sr_master(scale)).cuda()
        m.precision = "fp32"
        return m.train()

    def call(m, x):
        import warnings
        m.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = m(x)
        assert out.requires_grad
        (out ** 2).mean().backward()
        grads = [p.grad for _, p in sorted(m.named_parameters()) if p.grad is not None]
        assert len(grads) >= 60
        return [out.detach()] + grads
    run_poisoned(build, call, (_frames(rs, 8, 3, *hw),), (_frames(rs, 8, 3, *hw),), what=f"SR train step x{scale} {hw}")


# ---------------------------------------------------------------------------------------------------------------------
# whole frame
# ---------------------------------------------------------------------------------------------------------------------
def _vsr_master(cpu_vsr, scale):
    from video_super_resolution_amd import VSR
    from video_super_resolution_amd.weights import fill_module_
    if scale == 4:
        return cpu_vsr
    if ("vsr", scale) not in _masters:
        m = VSR(upscale_factor=scale).eval()
        m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
        fill_module_(m.model, seed=0, prefix="model.")
        _masters["vsr", scale] = m
    return _masters["vsr", scale]


def _vsr_build(cpu_vsr, scale, precision, **attrs):
    def build():
        m = copy.deepcopy(_vsr_master(cpu_vsr, scale)).cuda().eval()
        m.precision = m.model.precision = precision
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    return build


# VSR.forward refuses frames below 64 x 64 (FlowNet2's centre crop to multiples of 64), so the second, ragged size is 71 x 93
@pytest.mark.parametrize("hw", [(66, 70), (71, 93)])
@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_vsr_forward_first_and_recurrent_call(cpu_vsr, precision, scale, hw):
    """estimated_image = None, then the output fed back; the frame written into high_frames[1] and its uint8 write-out."""
    h, w = hw
    rs = np.random.RandomState(h + scale)

    def call(m, data):
        hf = torch.zeros(3, h * scale, w * scale, 3, device="cuda")
        out0, loss = m(data, None, hf, None, train=False)
        out0 = out0.clone()
        out1, _ = m(data, None, hf, out0, train=False)
        assert loss is None and torch.equal(hf[1], out1[0])
        return [out0, out1, driver.frames_to_u8(out1)]
    run_poisoned(_vsr_build(cpu_vsr, scale, precision), call, (_frames(rs, 3, h, w, 3),), (_frames(rs, 3, h, w, 3),),
                 what=f"VSR.forward {precision} x{scale} {hw}")


def test_vsr_streaming_mode_with_the_driver(cpu_vsr):
    """temporal_cache on: three sliding windows of one uint8 clip through driver.ingest_item, the estimate fed back, the frames
    written out as uint8 (the kept depth predictions and flow pictures of shared frames are arena tensors of an earlier call)."""
    rs = np.random.RandomState(5)

    def clip():
        video = rs.randint(0, 256, (5, 264, 280, 3)).astype(np.uint8)
        return (torch.from_numpy(np.stack([video[i:i + 3] for i in range(3)])).cuda(),)

    def call(m, datas):
        m.reset_temporal_cache()
        data, target, hf = driver.ingest_item(datas, 4)
        # the five LR frames once, the windows as views of them: consecutive windows share storage, which is what the cache keys on
        lr = torch.cat([data[0], data[1, 2:], data[2, 2:]])
        est, outs = None, []
        with torch.no_grad():
            for t in range(3):
                est, _ = m(lr[t:t + 3], None, hf[t], est, train=False)
                outs.append(est[0].clone())
        assert len(m._tcache["depth"]) == 3 and len(m._tcache["flow"]) == 2
        outs = torch.stack(outs)
        return [data, target, hf, outs, driver.frames_to_u8(outs)]
    run_poisoned(_vsr_build(cpu_vsr, 4, "fp16", temporal_cache=True), call, clip(), clip(), what="streaming VSR through the driver")


@pytest.mark.parametrize("shape,scale", _params(__import__("test_gpu_driver").test_ingest_matches_main_py_tensor_preparation, "shape,scale")[:3])
def test_driver_ingest_and_write_out(shape, scale):
    rs = np.random.RandomState(shape[2])
    mk = lambda: (torch.from_numpy(rs.randint(0, 256, shape).astype(np.uint8)).cuda(),)   # noqa: E731

    def call(_, d):
        lr, target, hf = driver.ingest_item(d, scale)
        lr_only, _, _ = driver.ingest_item(d, scale, want_hr=False)
        return [lr, target, hf, lr_only, driver.frames_to_u8(hf * 1.1 - 10.0)]
    run_poisoned(lambda: None, call, mk(), mk(), what=f"driver ingest / write-out {shape}")
