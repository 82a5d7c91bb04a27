"""Gradients of Resample2d / ChannelNorm / Correlation (csrc/flow_ops_bwd.hip through include/vsr_hip_grad.h and the
autograd Functions of ops.py) against stock PyTorch autograd on float64 restatements of the three forwards (tests/_flow_ref.py).
Bit-level claims about these kernels (exact operands, every build, the grid-stride second pass) are tests/test_gpu_exact_flow.py's;
this file keeps what that one cannot see: Gaussian operands, rounding behaviour, composition through autograd.

Tolerance: float32 kernels against a float64 master, 1e-5 of the gradient's largest magnitude.  The restatement of Resample2d
forms its sampling coordinate `x + flow` in float32 like the kernel (then continues in float64), so that both pick the same
cell at a coordinate that rounds onto an integer: the flow gradient is discontinuous there.  Finite differences
(`gradcheck`) are not usable in float32 and are not attempted.
"""
import copy

import pytest
import torch
import torch.nn as nn

from _flow_ref import GEOMS, ref_channelnorm, ref_correlation, ref_resample2d   # the restatements, moved there unchanged

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd import ops  # noqa: E402

DEV = "cuda"


def _leaf(t, dtype=None):
    return t.detach().to(dtype or t.dtype).clone().requires_grad_(True)


def _close(got, want, bar=1e-5):
    assert got is not None and got.shape == want.shape and got.dtype == torch.float32
    scale = want.abs().max().item()
    assert scale > 0
    err = (got.double() - want).abs().max().item() / scale
    assert err <= bar, err


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# Resample2d
# ----------------------------------------------------------------------------------------------------------------------
def _resample_case(img, flow, bilinear=True):
    gout = _rand(*img.shape, seed=99)
    i32, f32 = _leaf(img), _leaf(flow)
    out = ops.Resample2d(bilinear=bilinear)(i32, f32)
    assert out.requires_grad and out.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(out, ops.resample2d(img, flow, bilinear=bilinear))   # the Function's forward IS the forward entry
    out.backward(gout)
    i64, f64 = _leaf(img, torch.float64), _leaf(flow, torch.float64)
    ref = ref_resample2d(i64, f64, bilinear)
    torch.testing.assert_close(out.detach().double(), ref.detach(), rtol=0, atol=1e-5 * ref.abs().max().item())
    ref.backward(gout.double())
    return i32.grad, f32.grad, i64.grad, f64.grad


@pytest.mark.parametrize("shape", [(1, 3, 33, 47), (2, 5, 20, 70)])
@pytest.mark.parametrize("sigma", [0.5, 4.0, 40.0])
def test_resample2d_gradients(shape, sigma):
    B, C, H, W = shape
    img, flow = _rand(*shape, seed=1), _rand(B, 2, H, W, seed=2, scale=sigma)
    d_img, d_flow, r_img, r_flow = _resample_case(img, flow)
    _close(d_img, r_img)
    _close(d_flow, r_flow)


def test_resample2d_integer_flows_and_negative_coordinates():
    """Integer flows (alpha = beta = 0: all weight on one pixel) and coordinates left of / above the image, where floor and
    truncation differ: the image gradient is the adjoint of the forward there too."""
    B, C, H, W = 2, 3, 17, 29
    img = _rand(B, C, H, W, seed=3)
    flow = torch.randint(-6, 7, (B, 2, H, W), generator=torch.Generator().manual_seed(4)).float().to(DEV)
    d_img, d_flow, r_img, r_flow = _resample_case(img, flow)
    _close(d_img, r_img)
    _close(d_flow, r_flow)
    # every sample at x + flow in (-1, 0): floor gives xL = -1 -> clamped to 0, alpha = xf + 1; truncation would give alpha = xf < 0
    flow = torch.zeros(B, 2, H, W, device=DEV)
    flow[:, 0] = -torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, W) - 0.25
    flow[:, 1] = -torch.arange(H, device=DEV, dtype=torch.float32).view(1, H, 1) - 0.75
    d_img, d_flow, r_img, r_flow = _resample_case(img, flow)
    _close(d_img, r_img)
    # adjoint identity on the forward itself: <out(img), g> == <img, d_img> (out is linear in img)
    gout = _rand(B, C, H, W, seed=99)
    lhs = (ops.resample2d(img, flow).double() * gout.double()).sum()
    rhs = (img.double() * d_img.double()).sum()
    assert abs(lhs.item() - rhs.item()) <= 1e-5 * (img.double() * d_img.double()).abs().sum().item()
    assert torch.count_nonzero(d_img[:, :, 1:, 1:]) == 0        # everything lands on pixel (0, 0) ...
    bar = 1e-6 * gout.double().abs().sum((2, 3)).max().item()   # H*W float32 adds into one address
    torch.testing.assert_close(d_img[:, :, 0, 0].double(), gout.double().sum((2, 3)), rtol=0, atol=bar)  # ... with weight 1


def test_resample2d_nearest_has_zero_flow_gradient_and_a_one_pixel_scatter():
    B, C, H, W = 2, 3, 21, 38
    img, flow = _rand(B, C, H, W, seed=5), _rand(B, 2, H, W, seed=6, scale=3.0)
    d_img, d_flow, r_img, r_flow = _resample_case(img, flow, bilinear=False)
    _close(d_img, r_img)
    assert r_flow is None and d_flow is not None and torch.count_nonzero(d_flow) == 0


def test_resample2d_computes_only_the_gradients_asked_for():
    B, C, H, W = 1, 3, 33, 47
    img, flow = _rand(B, C, H, W, seed=7), _rand(B, 2, H, W, seed=8, scale=2.0)
    gout = _rand(B, C, H, W, seed=99)
    both_i, both_f, _, _ = _resample_case(img, flow)
    i32, f32 = _leaf(img), flow.clone()
    ops.resample2d(i32, f32).backward(gout)
    assert f32.grad is None
    _close(i32.grad, both_i.double(), 1e-6)          # atomics: equal up to the order of the adds
    i32, f32 = img.clone(), _leaf(flow)
    ops.resample2d(i32, f32).backward(gout)
    assert i32.grad is None and torch.equal(f32.grad, both_f)   # the flow gradient is a gather: bit-identical


# ----------------------------------------------------------------------------------------------------------------------
# ChannelNorm
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 33, 47), (2, 5, 20, 70), (3, 7, 5, 1)])
def test_channelnorm_gradient(shape):
    """H*W a multiple of 4 (16-byte accesses) and not (the one-pixel build); one pixel with all channels zero."""
    x = _rand(*shape, seed=9)
    x[0, :, shape[2] // 2, shape[3] // 2] = 0.0
    gout = _rand(shape[0], 1, shape[2], shape[3], seed=10)
    x32 = _leaf(x)
    out = ops.ChannelNorm()(x32)
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, ops.channelnorm(x))
    out.backward(gout)
    x64 = _leaf(x, torch.float64)
    ref_channelnorm(x64).backward(gout.double())
    assert torch.isfinite(x32.grad).all()
    assert torch.count_nonzero(x32.grad[0, :, shape[2] // 2, shape[3] // 2]) == 0    # 0, where stock autograd has 0/0
    want = torch.nan_to_num(x64.grad, nan=0.0)
    assert torch.isnan(x64.grad).sum() == shape[1]
    _close(x32.grad, want)


# ----------------------------------------------------------------------------------------------------------------------
# Correlation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,geom", GEOMS)
def test_correlation_gradients(shape, geom):
    f1, f2 = _rand(*shape, seed=11), _rand(*shape, seed=12)
    a32, b32 = _leaf(f1), _leaf(f2)
    out = ops.Correlation(**geom)(a32, b32)
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, ops.correlation(f1, f2, **geom))
    gout = _rand(*out.shape, seed=13)
    out.backward(gout)
    a64, b64 = _leaf(f1, torch.float64), _leaf(f2, torch.float64)
    ref = ref_correlation(a64, b64, geom["pad_size"], geom["max_displacement"], geom["stride1"], geom["stride2"])
    assert ref.shape == out.shape
    torch.testing.assert_close(out.detach().double(), ref.detach(), rtol=0, atol=1e-5 * ref.abs().max().item())
    ref.backward(gout.double())
    _close(a32.grad, a64.grad)
    _close(b32.grad, b64.grad)
    # each gradient alone (the other pointer null), and a second run: gathers in a fixed order, bit-identical
    x = _leaf(f1)
    (only_a,) = torch.autograd.grad(ops.correlation(x, f2, **geom), [x], gout)
    y = _leaf(f2)
    (only_b,) = torch.autograd.grad(ops.correlation(f1, y, **geom), [y], gout)
    assert torch.equal(only_a, a32.grad) and torch.equal(only_b, b32.grad)
    x, y = _leaf(f1), _leaf(f2)
    again_a, again_b = torch.autograd.grad(ops.correlation(x, y, **geom), [x, y], gout)
    assert torch.equal(again_a, a32.grad) and torch.equal(again_b, b32.grad)


# ----------------------------------------------------------------------------------------------------------------------
# composition, dtypes, unchanged behaviour
# ----------------------------------------------------------------------------------------------------------------------
class _Head(nn.Module):
    """A small FlowNetC-like head: conv -> correlation -> conv -> flow -> warp of the second image -> norm of the difference."""

    def __init__(self, corr, warp, norm):
        super().__init__()
        self.feat = nn.Conv2d(3, 16, 3, padding=1)
        self.pred = nn.Conv2d(25, 2, 3, padding=1)
        self.corr, self.warp, self.norm = corr, warp, norm

    def forward(self, im1, im2):
        c = self.corr(torch.tanh(self.feat(im1)), torch.tanh(self.feat(im2)))
        flow = 3.0 * self.pred(c)
        return self.norm(im1 - self.warp(im2, flow)).mean()


def test_a_flownetc_like_head_trains_through_the_three_operators():
    torch.manual_seed(0)
    geom = dict(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=2)
    head = _Head(ops.Correlation(**geom), ops.Resample2d(), ops.ChannelNorm()).to(DEV)
    master = _Head(lambda a, b: ref_correlation(a, b, 4, 4, 1, 2), ref_resample2d, ref_channelnorm).to(DEV)
    master.load_state_dict(copy.deepcopy(head.state_dict()))
    master = master.double()
    im1, im2 = _rand(2, 3, 24, 36, seed=20), _rand(2, 3, 24, 36, seed=21)
    a32, b32, a64, b64 = _leaf(im1), _leaf(im2), _leaf(im1, torch.float64), _leaf(im2, torch.float64)
    loss = head(a32, b32)
    loss.backward()
    ref = master(a64, b64)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    _close(a32.grad, a64.grad, 1e-4)
    _close(b32.grad, b64.grad, 1e-4)
    for (name, p), q in zip(head.named_parameters(), master.parameters()):
        _close(p.grad, q.grad, 1e-4)


def test_half_inputs_get_half_gradients():
    img = _rand(1, 3, 16, 24, seed=30).half().requires_grad_(True)
    flow = _rand(1, 2, 16, 24, seed=31).half().requires_grad_(True)
    out = ops.channelnorm(ops.resample2d(img, flow))
    assert out.dtype == torch.float32 and out.requires_grad
    out.sum().backward()
    assert img.grad.dtype == torch.float16 and flow.grad.dtype == torch.float16 and img.grad.abs().sum() > 0
    f = _rand(1, 8, 10, 12, seed=32).bfloat16().requires_grad_(True)
    ops.correlation(f, f.detach(), 2, 1, 2, 1, 1).sum().backward()
    assert f.grad.dtype == torch.bfloat16 and f.grad.abs().sum() > 0


def test_no_grad_calls_are_the_plain_forward_entries():
    img, flow = _leaf(_rand(2, 3, 20, 31, seed=40)), _leaf(_rand(2, 2, 20, 31, seed=41, scale=3.0))
    f1, f2 = _leaf(_rand(2, 8, 20, 31, seed=42)), _leaf(_rand(2, 8, 20, 31, seed=43))
    lib = L.load()

    def direct(entry, shape, *args):
        out = torch.empty(shape, dtype=torch.float32, device=DEV)
        L.check(entry(*args[:-1], L.dptr(out), *args[-1], L.stream()))
        return out

    with torch.no_grad():
        w = ops.resample2d(img, flow)
        n = ops.channelnorm(img)
        c = ops.correlation(f1, f2, 4, 1, 4, 1, 2)
        for t in (w, n, c):
            assert not t.requires_grad and t.grad_fn is None
        d = lambda t: L.dptr(t.detach())  # noqa: E731
        assert torch.equal(w, direct(lib.vsr_resample2d_f32, w.shape, d(img), d(flow), (2, 3, 20, 31, 1, 1)))
        assert torch.equal(n, direct(lib.vsr_channelnorm_f32, n.shape, d(img), (2, 3, 20, 31)))
        assert torch.equal(c, direct(lib.vsr_correlation_f32, c.shape, d(f1), d(f2), (2, 8, 20, 31, 4, 1, 4, 1, 2)))
    # inputs that do not require grad: the plain path with gradients enabled, too
    assert not ops.resample2d(img.detach(), flow.detach()).requires_grad
    assert ops.resample2d(img, flow).requires_grad and ops.correlation(f1, f2.detach(), 4, 1, 4, 1, 2).requires_grad


def test_refusals():
    with pytest.raises(L.VsrHipError):
        ops.resample2d(torch.zeros(1, 3, 4, 4, requires_grad=True), torch.zeros(1, 2, 4, 4))
    with pytest.raises(L.VsrHipError):
        ops.channelnorm(torch.zeros(1, 3, 4, 4, requires_grad=True))
    with pytest.raises(L.VsrHipError):
        ops.correlation(torch.zeros(1, 3, 4, 4, requires_grad=True), torch.zeros(1, 3, 4, 4))
    # kernel_size 3: the forward refuses first through the public call; the backward entries refuse on their own
    G = L.load_grad()
    img, flow = _rand(1, 3, 8, 8), _rand(1, 2, 8, 8)
    d_img = torch.full_like(img, 7.0)
    rc = G.vsr_grad_resample2d_f32(L.dptr(img), L.dptr(flow), L.dptr(img), L.dptr(d_img), None, 1, 3, 8, 8, 3, 1, L.stream())
    with pytest.raises(L.VsrHipError, match="grad_resample2d: kernel_size 3"):
        L.check(rc, "grad_resample2d", lib=G)
    rc = G.vsr_grad_correlation_f32(L.dptr(img), L.dptr(img), L.dptr(img), L.dptr(d_img), None, 1, 3, 8, 8, 1, 3, 1, 1, 1, L.stream())
    with pytest.raises(L.VsrHipError, match="grad_correlation: kernel_size 3"):
        L.check(rc, "grad_correlation", lib=G)
    torch.cuda.synchronize()
    assert torch.all(d_img == 7.0)      # nothing was launched, nothing was zeroed
    with pytest.raises(L.VsrHipError):
        ops.resample2d(_leaf(img), flow, kernel_size=3)
    # no double backward
    x = _leaf(_rand(1, 3, 8, 8, seed=50))
    (g,) = torch.autograd.grad(ops.channelnorm(x).sum(), [x], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
