"""The one-launch inception block (csrc/conv_hg_inception.hip, libvsr_hip_hgi.so; trunk_exec._Inception.fused) on the GPU:

  1. exact arithmetic (tests/_exact.py): integer operands, sparse integer weights, non-zero biases on every convolution, against a
     float64 reference chained from `conv_ref` (1x1, ReLU, k x k, ReLU, concat), bit for bit, for every block signature _A to _G;
  2. Gaussian operands against a float64 evaluation with the same fp16-rounded weights and the same fp16 rounding of the mid maps:
     the fused launch's maximum error at most 2 x the four-launch path's on the same case;
  3. batch invariance: image i of an N = 4 call equals the N = 1 call on image i;
  4. poisoned buffers (tests/_poison.py): all of the output is written and nothing else, the pad channels of x are never read;
  5. the whole hourglass with the switch on against the float32 master on stock operators.

The reference of a (signature, size) pair is computed once, for N = 3, and shared by the N = 1 runs (its first image), both input
offsets and both paths.  The cases and their references: tests/_hgi_cases.py (checked on the CPU by tests/test_hgi_cases_helper.py)."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import _exact as X  # noqa: E402
import _hgi_cases as C  # noqa: E402
from _hgi_cases import BIG_SIZES, NREF, SIGS, SIZES  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd import trunk_f32  # noqa: E402
from video_super_resolution_amd.trunk_exec import HourglassExec, _Inception  # noqa: E402


def _conv(w, b):
    k = w.shape[-1]
    c = nn.Conv2d(w.shape[1], w.shape[0], k, 1, (k - 1) // 2)
    c.weight.data = w.to(torch.float32)
    c.bias.data = b.to(torch.float32)
    return c.cuda()


def _block(wts):
    """_Inception from float64 weights: lists stand in for the Sequentials (conv, no BatchNorm, ReLU)."""
    (w0, b0), branches = wts
    mod = [[_conv(w0, b0), None, None]] + [[_conv(w1, b1), None, None, _conv(wk, bk), None, None] for (w1, b1, wk, bk) in branches]
    return _Inception(mod)


def _run(inc, x, in_coff, fused):
    """-> ([N,ctot,H,W] fp16 on the CPU, route histogram)."""
    inc.fused_small = fused
    L.ROUTES.calls, L.ROUTES.enabled = [], True
    try:
        buf, coff, c = inc(x, in_coff)
        torch.cuda.synchronize()
    finally:
        L.ROUTES.enabled = False
    hist = L.ROUTES.histogram()
    assert any(k.startswith("hg_inception<") for k in hist) == fused, hist
    assert len(hist) == 1 or not fused, hist
    return buf[..., coff:coff + c].permute(0, 3, 1, 2).contiguous().cpu(), hist


_exact_routes_seen = []   # the route of every fused launch of test_fused_block_is_exact


def _wide(x64, in_coff, fill):
    """[N,cin,H,W] float64 -> device [N,H,W,in_coff + cin + 32] fp16 with the live slice at in_coff and `fill` in every other channel."""
    N, C, H, W = x64.shape
    buf = torch.full((N, H, W, in_coff + C + 32), fill, dtype=torch.float16)
    buf[..., in_coff:in_coff + C] = x64.permute(0, 2, 3, 1).to(torch.float16)
    return buf.cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SIGS))
def test_fused_block_is_exact(name, hw):
    wts = C.exact_weights(name)
    inc = _block(wts)
    x = C.exact_input(name, hw)
    ref = C.exact_ref(wts, x)
    for n in (1, NREF):
        for in_coff in (0, 32):
            got, hist = _run(inc, _wide(x[:n], in_coff, 1000.0), in_coff, fused=True)
            _exact_routes_seen.extend(hist)
            X.assert_exact(got, ref[:n], f"block {name} {hw[0]}x{hw[1]} N={n} in_coff={in_coff} (fused)")
    four, _ = _run(inc, _wide(x, 32, 1000.0), 32, fused=False)
    X.assert_exact(four, ref, f"block {name} {hw[0]}x{hw[1]} (four launches)")


def test_exact_cases_ran_every_inception_route_the_trunks_launch():
    """(runs after the cases above) `hg_inception<..>` has no plan function: every such route the trunks launch at the BASELINE sizes
    (tests/golden/g14_trunk_layers.json, `self_named`) was the route of an exact case."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_trunk_layers.json")) as f:
        want = {r for r in json.load(f)["self_named"] if r.startswith("hg_inception<")}
    assert len(want) >= 2
    if len(_exact_routes_seen) >= 4 * len(SIZES) * len(SIGS):   # (the whole list ran, not a selection of its cases)
        assert want <= set(_exact_routes_seen), sorted(want - set(_exact_routes_seen))


# ---------------------------------------------------------------------------------------------------------------- 2. Gaussian
@pytest.mark.parametrize("hw", SIZES + BIG_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SIGS))
def test_fused_block_error_is_within_twice_the_four_launch_paths(name, hw):
    """Both paths against the float64 evaluation of the same operands.  The 2 x margin covers the different float32 summation order
    over up to 64 * 121 terms; the rounding points are the same."""
    cin = C.parts(SIGS[name])[0]
    wts = C.gauss_weights(name)
    inc = _block(wts)
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    x = torch.randn((NREF, cin) + hw, generator=g, dtype=torch.float64).to(torch.float16).double()
    ref = C.gauss_ref(wts, x)
    for n in (1, NREF):
        for in_coff in (0, 32):
            xd = _wide(x[:n], in_coff, float("nan"))
            fused, _ = _run(inc, xd, in_coff, fused=True)
            four, _ = _run(inc, xd, in_coff, fused=False)
            e_fused = float((fused.double() - ref[:n]).abs().max())
            e_four = float((four.double() - ref[:n]).abs().max())
            print(f"[hg_inception gauss] {name} {hw[0]}x{hw[1]} N={n} in_coff={in_coff}: fused {e_fused:.3e} four-launch {e_four:.3e} "
                  f"(range {float(ref.abs().max()):.2f})")
            assert torch.isfinite(fused).all() and torch.isfinite(four).all()
            assert e_fused <= 2.0 * e_four, (name, hw, n, in_coff, e_fused, e_four)


# ---------------------------------------------------------------------------------------------------------------- 3. batch invariance
@pytest.mark.parametrize("hw", [(17, 33), (33, 60)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SIGS))
def test_a_pixel_does_not_depend_on_the_batch(name, hw):
    cin = C.parts(SIGS[name])[0]
    inc = _block(C.gauss_weights(name))
    g = torch.Generator().manual_seed(hw[0] + hw[1])
    x = torch.randn((4, cin) + hw, generator=g, dtype=torch.float64)
    all4, _ = _run(inc, _wide(x, 32, float("nan")), 32, fused=True)
    for i in range(4):
        one, _ = _run(inc, _wide(x[i:i + 1], 32, float("nan")), 32, fused=True)
        assert torch.equal(one[0], all4[i]), (name, hw, i)
    with L.route_batch(1, 2):   # the route batch of the streaming mode changes nothing either
        half, _ = _run(inc, _wide(x[:2], 32, float("nan")), 32, fused=True)
    assert torch.equal(half, all4[:2])


# ---------------------------------------------------------------------------------------------------------------- 4. poisoned buffers
@pytest.mark.parametrize("hw", [(7, 9), (17, 33)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SIGS))
def test_fused_block_writes_all_of_its_output_and_nothing_else(name, hw):
    cin = C.parts(SIGS[name])[0]
    inc = _block(C.gauss_weights(name))
    g = torch.Generator().manual_seed(hw[0] * 7 + hw[1])
    x = torch.randn((2, cin) + hw, generator=g, dtype=torch.float64)
    clean, _ = _run(inc, _wide(x, 32, 0.0), 32, fused=True)
    xd = _wide(x, 32, float("nan"))   # the pad channels of x on both sides of the slice are NaN
    with poisoned() as arena:
        inc.fused_small = True
        buf, coff, c = inc(xd, 32)
        assert arena.n_allocated == 1 and (coff, c) == (0, buf.shape[3])      # the dense result is the launch's only allocation
        arena.assert_written(buf, f"block {name} result")
        arena.check()
        got = buf.permute(0, 3, 1, 2).contiguous().cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got, clean)


# ---------------------------------------------------------------------------------------------------------------- 5. the trunk
@contextlib.contextmanager
def _stock_trunks():
    old = trunk_f32.ENABLED
    trunk_f32.ENABLED = False
    try:
        yield
    finally:
        trunk_f32.ENABLED = old


@pytest.mark.parametrize("hw", [(48, 80), (50, 70)], ids=lambda s: "%dx%d" % s)
def test_hourglass_with_the_fused_blocks(gpu_vsr, hw):
    netg = gpu_vsr.DepthModule.model.netG
    fr = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (2,) + hw + (3,)).astype(np.float32)).cuda()
    old = _Inception.fused_small
    try:
        with torch.no_grad():
            ex = HourglassExec(netg)
            with _stock_trunks():
                ref = netg(fr.permute(0, 3, 1, 2).contiguous())
            _Inception.fused_small = False
            off = ex(fr).clone()
            _Inception.fused_small = True
            L.ROUTES.calls, L.ROUTES.enabled = [], True
            try:
                on = ex(fr).clone()
            finally:
                L.ROUTES.enabled = False
    finally:
        _Inception.fused_small = old
    hist = L.ROUTES.histogram()
    scale = ref.abs().max().item()
    e_on, e_off = (on - ref).abs().max().item() / scale, (off - ref).abs().max().item() / scale
    print(f"[hourglass 2x{hw[0]}x{hw[1]} vs fp32 master] fused blocks {e_on:.3e}, four launches {e_off:.3e} of range; routes {hist}")
    assert on.shape == ref.shape
    assert e_on < 1e-2
    assert hist.get("hg_inception<3,5,7>", 0) >= 1 and hist.get("hg_inception<3,7,11>", 0) >= 1, hist
