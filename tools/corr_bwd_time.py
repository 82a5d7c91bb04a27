"""Time of the correlation backward (vsr_grad_correlation_f32: d_f1 + d_f2, two launches) at FlowNetC's geometry
(C 256, pad 20, max_displacement 20, stride2 2: 441 displacements) beside the forward launch and beside stock autograd on
the shift / multiply / mean restatement in float32; device events, rounds interleaved, best of the rounds.  Also the two byte
movers (Resample2d and ChannelNorm backward) at a pair of 512x960 frames, the warp on a smooth and on a white-noise flow.  Prints the algorithmic FLOP rate of the correlation gradients."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from video_super_resolution_amd import _lib as L, ops

assert torch.cuda.is_available(), "needs the GPU (no fallback)"
G = L.load_grad()
PAD, K, MD, S1, S2 = 20, 1, 20, 1, 2


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def restated(f1, f2):
    R = MD // S2
    p2 = F.pad(f2, (PAD,) * 4)
    H, W = f1.shape[2:]
    return torch.stack([(f1 * p2[:, :, MD + tj * S2:MD + tj * S2 + H, MD + ti * S2:MD + ti * S2 + W]).mean(1)
                        for tj in range(-R, R + 1) for ti in range(-R, R + 1)], 1)


for B, H, W in ((1, 48, 64), (1, 64, 120), (2, 64, 120)):     # 1/8 of 384x512, of the 512x960 benchmark frame, a pair of them
    f1, f2 = torch.randn(B, 256, H, W, device="cuda"), torch.randn(B, 256, H, W, device="cuda")
    out = ops.correlation(f1, f2, PAD, K, MD, S1, S2)
    g = torch.randn_like(out)
    d1, d2 = torch.empty_like(f1), torch.empty_like(f2)

    def fwd():
        ops.correlation(f1, f2, PAD, K, MD, S1, S2)

    def bwd():
        L.check(G.vsr_grad_correlation_f32(L.dptr(f1), L.dptr(f2), L.dptr(g), L.dptr(d1), L.dptr(d2), B, 256, H, W, PAD, K, MD, S1, S2,
                                           L.stream()), lib=G)

    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)

    def stock():
        torch.autograd.grad(restated(a, b), [a, b], g)

    t = {"fwd": [], "bwd": [], "stock": []}
    for rnd in range(4):
        for name, fn, reps in (("fwd", fwd, 50), ("bwd", bwd, 50), ("stock", stock, 2)):
            fn(); t[name].append(events(fn, reps))
    flop = 2 * 2.0 * 441 * 256 * B * H * W     # both gradients
    best = {k: min(v) for k, v in t.items()}
    print(f"B {B} C 256 {H}x{W}: forward {best['fwd']:8.1f} us | backward (d_f1 + d_f2) {best['bwd']:8.1f} us = "
          f"{flop / best['bwd'] * 1e-6:6.2f} TFLOP/s algorithmic | stock autograd fwd+bwd of the restatement {best['stock']:10.1f} us")

B, C, H, W = 2, 3, 512, 960
img, gout = torch.randn(B, C, H, W, device="cuda"), torch.randn(B, C, H, W, device="cuda")
d_img, d_flow = torch.empty_like(img), torch.empty(B, 2, H, W, device="cuda")
nrm = ops.channelnorm(img)
gn = torch.randn_like(nrm)
# a smooth field (what a flow network predicts: neighbouring lanes add into runs of consecutive addresses) and white noise of 4 px
# (every lane its own row and column: the atomics' worst access shape)
smooth = F.interpolate(torch.randn(B, 2, H // 32, W // 32, device="cuda") * 4, size=(H, W), mode="bilinear", align_corners=False).contiguous()
rough = torch.randn(B, 2, H, W, device="cuda") * 4


def warp_bwd(flow, want_img=True, want_flow=True):
    L.check(G.vsr_grad_resample2d_f32(L.dptr(img), L.dptr(flow), L.dptr(gout), L.optr(d_img if want_img else None),
                                      L.optr(d_flow if want_flow else None), B, C, H, W, 1, 1, L.stream()), lib=G)


def norm_bwd():
    L.check(G.vsr_grad_channelnorm_f32(L.dptr(img), L.dptr(nrm), L.dptr(gn), L.dptr(d_img), B, C, H, W, L.stream()), lib=G)


def best_of(fn):
    fn()
    return min(events(fn, 50) for _ in range(4))


for name, flow in (("smooth flow", smooth), ("white-noise flow, sigma 4 px", rough)):
    both, only_img, only_flow = (best_of(lambda: warp_bwd(flow)), best_of(lambda: warp_bwd(flow, want_flow=False)),
                                 best_of(lambda: warp_bwd(flow, want_img=False)))
    print(f"resample2d backward at {B}x{C}x{H}x{W}, {name}: both gradients {both:7.1f} us | d_img alone (memset + scatter) {only_img:7.1f} us = "
          f"{4.0 * B * C * H * W * 4 / only_img * 1e-6:5.2f} TB/s of atomic bytes | d_flow alone (gather) {only_flow:7.1f} us")
t = best_of(norm_bwd)
print(f"channelnorm backward at {B}x{C}x{H}x{W}: {t:7.1f} us = {4.0 * B * H * W * (2 * C + 2) / t * 1e-6:5.2f} TB/s of algorithmic bytes")
