"""FlowNet2's native operators and the flow colour coding on gfx950 (HIP, through the C ABI).

Module names, constructor arguments and call signatures mirror the reference's wrappers so the
FlowNet2 graph reads the same: `Resample2d` (resample2d_package/resample2d.py:42-51), `ChannelNorm`
(channelnorm_package/channelnorm.py:32-39), `Correlation` (correlation_package/correlation.py:50-64).

Differentiable: when gradients are enabled and an input requires grad, `resample2d`, `channelnorm` and `correlation` (and the
three modules) go through a `torch.autograd.Function` whose forward is the same entry of libvsr_hip.so and whose backward is
a kernel of libvsr_hip_grad.so (include/vsr_hip_grad.h, csrc/flow_ops_bwd.hip) -- the counterpart of the reference's
`*_cuda.backward` bindings; there is no stock-operator fallback.  float32 kernels: a half / bfloat16 input is converted inside
the graph, so its gradient comes back in its own dtype.  Every gradient is bit-reproducible except Resample2d's image
gradient (a scatter of float atomic adds: order-dependent in the last bits).  No double backward.
Otherwise -- the whole flow branch of `VSR.forward` runs under `torch.no_grad()` (network/video_super_resolution.py:24) --
the call is the plain forward launch: nothing is saved, nothing else runs.  The fused forms (`warp_concat`, `warp_norms`) and
the fp16 NHWC correlation of the FlowNetC executor are forward-only.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib as L


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


@L.on_device
def resample2d(img: torch.Tensor, flow: torch.Tensor, kernel_size: int = 1, bilinear: bool = True) -> torch.Tensor:
    """out[b,c,y,x] = bilinear(img[b,c], x + flow[b,0,y,x], y + flow[b,1,y,x]); indices clamped independently."""
    if _wants_grad(img, flow):
        return Resample2dFn.apply(img.to(torch.float32), flow.to(torch.float32), int(kernel_size), bool(bilinear))
    return _resample2d_fwd(_f32c(img), _f32c(flow), kernel_size, bilinear)


def _resample2d_fwd(img, flow, kernel_size, bilinear):
    B, C, Hi, Wi = img.shape
    Bf, two, H, W = flow.shape
    if two != 2 or Bf != B or (Hi, Wi) != (H, W):
        raise ValueError(f"resample2d: img {tuple(img.shape)} vs flow {tuple(flow.shape)}")
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=img.device)
    L.check(L.load().vsr_resample2d_f32(L.dptr(img), L.dptr(flow), L.dptr(out), B, C, H, W, int(kernel_size),
                                        int(bool(bilinear)), L.stream()), "resample2d")
    return out


@L.on_device
def channelnorm(x: torch.Tensor) -> torch.Tensor:
    if _wants_grad(x):
        return ChannelNormFn.apply(x.to(torch.float32))
    return _channelnorm_fwd(_f32c(x))


def _channelnorm_fwd(x):
    B, C, H, W = x.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    L.check(L.load().vsr_channelnorm_f32(L.dptr(x), L.dptr(out), B, C, H, W, L.stream()), "channelnorm")
    return out


def correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2):
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.check(L.load().vsr_correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2,
                                               ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)), "correlation_out_shape")
    return oc.value, oh.value, ow.value


@L.on_device
def correlation(f1: torch.Tensor, f2: torch.Tensor, pad_size=20, kernel_size=1, max_displacement=20, stride1=1,
                stride2=2, corr_multiply=1) -> torch.Tensor:
    if _wants_grad(f1, f2):
        return CorrelationFn.apply(f1.to(torch.float32), f2.to(torch.float32), pad_size, kernel_size, max_displacement, stride1,
                                   stride2)
    return _correlation_fwd(_f32c(f1), _f32c(f2), pad_size, kernel_size, max_displacement, stride1, stride2)


def _correlation_fwd(f1, f2, pad_size, kernel_size, max_displacement, stride1, stride2):
    if f1.shape != f2.shape:
        raise ValueError("correlation: inputs differ in shape")
    B, C, H, W = f1.shape
    oc, oh, ow = correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    out = torch.empty((B, oc, oh, ow), dtype=torch.float32, device=f1.device)
    L.check(L.load().vsr_correlation_f32(L.dptr(f1), L.dptr(f2), L.dptr(out), B, C, H, W, pad_size, kernel_size,
                                         max_displacement, stride1, stride2, L.stream()), "correlation")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The differentiable form of the three operators: forward = the entry above, backward = libvsr_hip_grad.so.  `backward`
# launches on the device of the gradient it is handed (`on_device`), on that device's current stream -- the autograd engine
# has made the forward's stream current.  A gradient that is not needed is not computed (null pointer) and returned as None.
# ---------------------------------------------------------------------------------------------------------------------
@L.on_device
def _resample2d_bwd(gout, img, flow, kernel_size, bilinear, need_img, need_flow):
    B, C, H, W = img.shape
    d_img = torch.empty_like(img) if need_img else None      # zeroed by the entry (it scatters)
    d_flow = torch.empty_like(flow) if need_flow else None
    G = L.load_grad()
    L.check(G.vsr_grad_resample2d_f32(L.dptr(img), L.dptr(flow), L.dptr(gout), L.optr(d_img), L.optr(d_flow), B, C, H, W,
                                      int(kernel_size), int(bool(bilinear)), L.stream()), "grad_resample2d", lib=G)
    return d_img, d_flow


@L.on_device
def _channelnorm_bwd(gout, x, out):
    B, C, H, W = x.shape
    d_x = torch.empty_like(x)
    G = L.load_grad()
    L.check(G.vsr_grad_channelnorm_f32(L.dptr(x), L.dptr(out), L.dptr(gout), L.dptr(d_x), B, C, H, W, L.stream()),
            "grad_channelnorm", lib=G)
    return d_x


@L.on_device
def _correlation_bwd(gout, f1, f2, geom, need_f1, need_f2):
    B, C, H, W = f1.shape
    d_f1 = torch.empty_like(f1) if need_f1 else None
    d_f2 = torch.empty_like(f2) if need_f2 else None
    G = L.load_grad()
    L.check(G.vsr_grad_correlation_f32(L.dptr(f1), L.dptr(f2), L.dptr(gout), L.optr(d_f1), L.optr(d_f2), B, C, H, W, *geom,
                                       L.stream()), "grad_correlation", lib=G)
    return d_f1, d_f2


class Resample2dFn(torch.autograd.Function):
    """resample2d_package/resample2d.py:6-39 (Resample2dFunction) on the HIP entries."""

    @staticmethod
    def forward(ctx, img, flow, kernel_size, bilinear):
        img, flow = _f32c(img), _f32c(flow)
        ctx.save_for_backward(img, flow)
        ctx.kernel_size, ctx.bilinear = kernel_size, bilinear
        return _resample2d_fwd(img, flow, kernel_size, bilinear)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        img, flow = ctx.saved_tensors
        need_img, need_flow = ctx.needs_input_grad[:2]
        if not (need_img or need_flow):
            return None, None, None, None
        d_img, d_flow = _resample2d_bwd(_f32c(gout), img, flow, ctx.kernel_size, ctx.bilinear, need_img, need_flow)
        return d_img, d_flow, None, None


class ChannelNormFn(torch.autograd.Function):
    """channelnorm_package/channelnorm.py:6-29 (ChannelNormFunction) on the HIP entries."""

    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        out = _channelnorm_fwd(x)
        ctx.save_for_backward(x, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, out = ctx.saved_tensors
        return _channelnorm_bwd(_f32c(gout), x, out)


class CorrelationFn(torch.autograd.Function):
    """correlation_package/correlation.py:7-47 (CorrelationFunction) on the HIP entries; no rbot1 / rbot2 scratch copies."""

    @staticmethod
    def forward(ctx, f1, f2, pad_size, kernel_size, max_displacement, stride1, stride2):
        f1, f2 = _f32c(f1), _f32c(f2)
        ctx.save_for_backward(f1, f2)
        ctx.geom = tuple(int(v) for v in (pad_size, kernel_size, max_displacement, stride1, stride2))
        return _correlation_fwd(f1, f2, *ctx.geom)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        f1, f2 = ctx.saved_tensors
        need_f1, need_f2 = ctx.needs_input_grad[:2]
        if not (need_f1 or need_f2):
            return (None,) * 7
        d_f1, d_f2 = _correlation_bwd(_f32c(gout), f1, f2, ctx.geom, need_f1, need_f2)
        return (d_f1, d_f2) + (None,) * 5


@L.on_device
def warp_concat(x6: torch.Tensor, flow: torch.Tensor, div_flow: float) -> torch.Tensor:
    """cat(x6, warp(x6[:,3:], flow), flow/div_flow, |x6[:,:3]-warp|) in one kernel (models.py:86-91,98-103)."""
    x6, flow = _f32c(x6), _f32c(flow)
    B, six, H, W = x6.shape
    if six != 6 or tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("warp_concat: bad shapes")
    out = torch.empty((B, 12, H, W), dtype=torch.float32, device=x6.device)
    L.check(L.load().vsr_flownet_warp_concat_f32(L.dptr(x6), L.dptr(flow), L.cf(1.0 / div_flow), L.dptr(out), B, H, W,
                                                 L.stream()), "warp_concat")
    return out


@L.on_device
def warp_norms(x6: torch.Tensor, flow: torch.Tensor):
    """(|flow|, |x6[:,:3] - warp(x6[:,3:], flow)|) without materialising the warp (models.py:107-112,116-121)."""
    x6, flow = _f32c(x6), _f32c(flow)
    B, six, H, W = x6.shape
    if six != 6 or tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("warp_norms: bad shapes")
    nf = torch.empty((B, 1, H, W), dtype=torch.float32, device=x6.device)
    nd = torch.empty_like(nf)
    L.check(L.load().vsr_flownet_warp_norms_f32(L.dptr(x6), L.dptr(flow), L.dptr(nf), L.dptr(nd), B, H, W, L.stream()),
            "warp_norms")
    return nf, nd


@L.on_device
def flow2img(flow_2hw: torch.Tensor) -> torch.Tensor:
    """[2,h,w] float32 flow -> [h,w,3] float32 picture of uint8 values (utils/flow_utils.py:4-62), no host trip."""
    flow = _f32c(flow_2hw)
    two, H, W = flow.shape
    if two != 2:
        raise ValueError("flow2img expects [2,h,w]")
    out = torch.empty((H, W, 3), dtype=torch.float32, device=flow.device)
    ws = torch.empty(4, dtype=torch.int32, device=flow.device)
    L.check(L.load().vsr_flow2img_f32(L.dptr(flow), L.dptr(out), L.dptr(ws, torch.int32), H, W, L.stream()), "flow2img")
    return out


@L.on_device
def flow2img_nhwc(flow_hwc_half: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """[h,w,ld] float16 map whose channels 0,1 are the flow (the fusion network's output as the MFMA convolution leaves it)
    -> [h,w,3] float32 picture; same arithmetic as flow2img (half -> float is exact)."""
    H, W, ld = flow_hwc_half.shape
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.float32, device=flow_hwc_half.device)
    ws = torch.empty(4, dtype=torch.int32, device=flow_hwc_half.device)
    L.check(L.load().vsr_flow2img_nhwc_f16(L.dptr(flow_hwc_half, torch.float16), ld, L.dptr(out), L.dptr(ws, torch.int32), H, W,
                                           L.stream()), "flow2img_nhwc")
    return out


class Resample2d(nn.Module):
    def __init__(self, kernel_size=1, bilinear=True):
        super().__init__()
        self.kernel_size = kernel_size
        self.bilinear = bilinear

    def forward(self, input1, input2):
        return resample2d(input1, input2, self.kernel_size, self.bilinear)


class ChannelNorm(nn.Module):
    def __init__(self, norm_deg=2):
        super().__init__()
        self.norm_deg = norm_deg  # accepted and ignored, like the reference kernel (channelnorm_kernel.cu:26)

    def forward(self, input1):
        return channelnorm(input1)


class Correlation(nn.Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super().__init__()
        self.pad_size, self.kernel_size, self.max_displacement = pad_size, kernel_size, max_displacement
        self.stride1, self.stride2, self.corr_multiply = stride1, stride2, corr_multiply

    def forward(self, input1, input2):
        return correlation(input1, input2, self.pad_size, self.kernel_size, self.max_displacement, self.stride1,
                           self.stride2, self.corr_multiply)
