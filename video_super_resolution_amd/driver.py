"""A `main.py`-like driver around `VSR.forward`: the callers and data formats either side of the path.

What the reference's train/validate loop does per dataset item (main.py:154-203) and what utils/video_utils.py:7-33
feeds it, on the GPU path and without OpenCV:

    VideoDataset            sliding 3-frame windows over a decoded RGB clip, cut into `splitvideonum` = 20 chunks per video,
                            handed out chunk by chunk (video_utils.py:7-33; same indexing, including the 21st "truth" slot)
    ingest_item             uint8 [T,3,H,W,3] -> data [T,3,H/s,W/s,3] (nearest), target [T,1,H,W,3], high_frames [T,3,H,W,3]
                            as float32, ON THE DEVICE in one kernel (main.py:155-167, MakeData/Target/HFDatasetToTensor)
    run_item                `for x, y, high_frame in zip(data, target, high_frames): output, loss = model(x, y, high_frame,
                            estimated_image); estimated_image = output` (main.py:196-203) -> HR frames (+ losses)
    frames_to_u8            HR write-out, float32 -> uint8 NHWC on the device (the step after the path; the reference never
                            writes its frames)
    frame_metrics / psnr_ssim   HR frames scored against ground truth on the device: the float64 sums behind PSNR and SSIM per frame
                            (include/vsr_hip_metric.h), and the host step that forms the two numbers from them
    read_clip_yuv / ingest_item_yuv / frames_to_yuv     the same three steps for what decoders emit: packed Y'CbCr 4:2:0 frames
                            (yuv420p, nv12, yuv420p10le, p010le), converted on the device (include/vsr_hip_yuv.h); the matrix
                            coefficients come from `yuv_coefficients` alone
    resize_tables / FrameResizer   float32 RGB frames resampled on the device by a separable filter given as tables
                            (include/vsr_hip_resize.h): antialiased bicubic (Keys, a = -0.5, Pillow's convention) or bilinear; the tables
                            come from `resize_tables` alone
    ClipRunner              a clip streamed through the model: every source frame uploaded once from pinned memory on a copy stream,
                            converted once into a three-slot LR ring, the window formed on the device, the HR frame written out as
                            4:2:0 and copied back on a second copy stream; `score=`: every output frame scored against the source
                            frame it restores, from the upload already on the device; `decimate="bicubic"`: LR frames that are the
                            antialiased bicubic reduction of the source stored as 8-bit; `baseline="bicubic"`: the bicubic enlargement
                            of the middle LR frame scored beside the estimate; `temporal="warp"`: the flow-warped error between
                            consecutive output frames beside the per-frame scores
    truth_flows / warp_error / ewarp   the temporal warping error on the device (include/vsr_hip_warp.h): forward and backward FlowNet2
                            flows between ground-truth frames, frame t + 1 warped back onto frame t and the squared difference summed
                            over the pixels that are not occluded, in float64, and the host step that forms E_warp from the sums
    save_checkpoint / load_checkpoint   utils/tools.py:68-73 and main.py:108-122,233-237: {'arch','epoch','state_dict':
                            SRmodel.model.state_dict(),'optimizer'} -- files interchange with the reference's

`python -m video_super_resolution_amd.driver` is BASELINE.json's config C1 (3-frame 128x128 LR synthetic clip through the
main-like plumbing) on the GPU path (`tools/c1_check.py` runs the CPU checker beside it and reports the PSNR between the two:
the package itself never touches the checker).
Decoding compressed video (cv2.VideoCapture, video_utils.py:17-23) is out of scope: a clip enters as a uint8 RGB array
(`.npy`, raw rgb24, or synthetic) or as raw 4:2:0 frames (`ffmpeg -f rawvideo`; transfer functions, 4:2:2 / 4:4:4 stay out too).
"""
from __future__ import annotations

import os
import shutil
from glob import glob
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


# ------------------------------------------------------------------------------------------------ dataset
def read_clip(path: str, shape: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """A clip as uint8 RGB [T,H,W,3]: `.npy`, or headerless rgb24 (`shape` = (H, W) required)."""
    if path.endswith(".npy"):
        a = np.load(path)
    else:
        if shape is None:
            raise ValueError("raw rgb24 clips need shape=(H, W)")
        a = np.fromfile(path, dtype=np.uint8)
        a = a.reshape(-1, shape[0], shape[1], 3)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"{path}: expected uint8 [T,H,W,3], got {a.dtype} {a.shape}")
    return a


def sliding_windows(imgs: Sequence[np.ndarray], splitvideonum: int = 20) -> List[List[Sequence[np.ndarray]]]:
    """video_utils.py:24-27: 3-frame windows `imgs[i:i+3]`, cut into chunks of `length // splitvideonum` windows starting
    at every multiple of that step below `length` (length = FRAME count, so the last chunks are short or empty -- kept)."""
    length = len(imgs)
    data = [imgs[i:i + 3] for i in range(len(imgs) - 2)]
    step = int(length / splitvideonum)
    if step <= 0:
        raise ValueError(f"a clip needs at least {splitvideonum} frames (video_utils.py:26 steps by int(length / {splitvideonum}))")
    return [data[i:i + step] for i in range(0, length, step)]


class VideoDataset(torch.utils.data.Dataset):
    """utils/video_utils.py:7-33 without OpenCV: `videos` are paths (`.npy` / rgb24 + `raw_shape`), arrays [T,H,W,3] uint8,
    or a directory (globbed like the reference).  `__len__` = videos x 21, item `idx` with idx % 21 == 0 (re)reads video
    idx // 21, every item pops the next chunk: a list of 3-frame windows ([3,H,W,3] uint8 each)."""

    def __init__(self, videos, raw_shape: Optional[Tuple[int, int]] = None, splitvideonum: int = 20):
        if isinstance(videos, str):
            videos = sorted(glob(os.path.join(videos, "*")))
        elif isinstance(videos, np.ndarray):   # ONE clip [T,H,W,3], not a list of clips (list() would split it into frames)
            videos = [videos]
        self.video_paths = list(videos)
        self.raw_shape = raw_shape
        self.data: list = []
        self.splitvideonum = splitvideonum
        self.truthsplitvideonum = splitvideonum + 1

    def __len__(self):
        return len(self.video_paths) * self.truthsplitvideonum

    def read_video(self, v):
        imgs = read_clip(v, self.raw_shape) if isinstance(v, str) else np.asarray(v)
        self.data.extend(sliding_windows(list(imgs), self.splitvideonum))

    def __getitem__(self, idx):
        if idx % self.truthsplitvideonum == 0:
            self.read_video(self.video_paths[idx // self.truthsplitvideonum])
        data = self.data[0]
        self.data = self.data[1:]
        return data


# ------------------------------------------------------------------------------------------------ ingest / write-out
@L.on_device
def ingest_item(datas_u8: torch.Tensor, scale: int = 4, want_hr: bool = True):
    """uint8 [T,3,H,W,3] on the device -> (data [T,3,H//s,W//s,3], target [T,1,H,W,3] | None, high_frames [T,3,H,W,3] | None),
    float32 (main.py:155-167; `scale` is 4 there: `int(d.shape[1] / 4)`)."""
    if datas_u8.dtype != torch.uint8 or datas_u8.dim() != 5 or datas_u8.shape[1] != 3 or datas_u8.shape[4] != 3:
        raise ValueError(f"expected uint8 [T,3,H,W,3], got {datas_u8.dtype} {tuple(datas_u8.shape)}")
    T, _, H, W, _ = datas_u8.shape
    h, w = int(H / scale), int(W / scale)
    d = datas_u8.contiguous()
    lr = torch.empty((T, 3, h, w, 3), dtype=torch.float32, device=d.device)
    hr = torch.empty((T, 3, H, W, 3), dtype=torch.float32, device=d.device) if want_hr else None
    L.check(L.load().vsr_clip_ingest_u8(L.dptr(d, torch.uint8), L.dptr(lr), L.optr(hr), T * 3, H, W, h, w, L.stream()), "clip_ingest")
    if hr is None:
        return lr, None, None
    # target = datas[:, 1:2].float() (main.py:161-163): its own tensor -- VSR.forward overwrites high_frames[1] in place (:66)
    return lr, hr[:, 1:2].clone(), hr


@L.on_device
def frames_to_u8(frames: torch.Tensor) -> torch.Tensor:
    """float32 HR frames (any shape) -> uint8, round half to even, clamped to 0..255."""
    f = frames.detach().to(torch.float32).contiguous()
    out = torch.empty(f.shape, dtype=torch.uint8, device=f.device)
    import ctypes
    L.check(L.load().vsr_frame_to_u8(L.dptr(f), L.dptr(out, torch.uint8), ctypes.c_size_t(f.numel()), L.stream()), "frame_to_u8")
    return out


# ------------------------------------------------------------------------------------------------ PSNR / SSIM
METRIC_CHANNELS = {"rgb": 0, "y": 1}     # the `channels` codes of include/vsr_hip_metric.h
METRIC_WHAT = {"psnr": 1, "ssim": 2}     # the bits of `what`: PSNR needs the SSE


def ssim_window() -> np.ndarray:
    """The normalised 1-D window of SSIM (Wang et al. 2004): 11 taps of exp(-(i - 5)^2 / (2 * 1.5^2)) over their sum, float64; the 2-D
    window is its outer product."""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


@L.on_device
def frame_metrics(a: torch.Tensor, b: torch.Tensor, channels: str = "rgb", quantise: bool = True, shave: int = 0, what=("psnr", "ssim"),
                  matrix: str = "bt601", full_range: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 RGB frames `a`, `b` ([H,W,3], [1,H,W,3] or [F,H,W,3], 0..255) -> the device tensor [F,4] float64 of
    {sse, n_sse, ssim_sum, n_ssim} per frame (vsr_metric_frames); nothing is synchronised, `psnr_ssim` is the host step.
    `quantise`: score what write-out stores (clamp to 0..255, round half to even); `shave`: pixels dropped on every side;
    `channels="y"`: on the luma of `matrix` / `full_range` (row 0 of `yuv_coefficients`; the default is BT.601 limited range, the
    literature's "Y"); `what`: "psnr" and / or "ssim" (the slots of the other are 0); `out`: write the sums there ([F,4] float64)."""
    import ctypes
    if channels not in METRIC_CHANNELS:
        raise ValueError(f"unknown channels {channels!r} (known: {', '.join(METRIC_CHANNELS)})")
    names = (what,) if isinstance(what, str) else tuple(what)
    if not names or any(n not in METRIC_WHAT for n in names):
        raise ValueError(f"what must name 'psnr' and / or 'ssim', got {what!r}")
    bits = 0
    for n in names:
        bits |= METRIC_WHAT[n]
    if tuple(a.shape) != tuple(b.shape) or a.dim() not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"expected two float32 tensors of one shape [H,W,3] or [F,H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    shave = int(shave)
    H, W = int(a.shape[-3]), int(a.shape[-2])
    F = int(a.shape[0]) if a.dim() == 4 else 1
    if shave < 0 or 2 * shave >= min(H, W):
        raise ValueError(f"shave {shave} leaves nothing of {H} x {W}")
    if bits & 2 and min(H, W) - 2 * shave < 11:
        raise ValueError(f"SSIM needs 11 pixels each way after the shave, got {min(H, W) - 2 * shave}")
    luma4 = None
    if channels == "y":
        c = yuv_coefficients("yuv420p", matrix, full_range)
        luma4 = np.ascontiguousarray(np.array([c[0], c[1], c[2], c[9]], dtype=np.float32))
    win = ssim_window()
    fa, fb = a.detach().contiguous(), b.detach().contiguous()
    M = L.load_metric()
    pa, pb = L.dptr(fa), L.dptr(fb)   # (raises on CPU tensors and on anything but float32)
    if fb.device != fa.device:
        raise ValueError("the two tensors live on different devices")
    if out is None:
        out = torch.empty((F, 4), dtype=torch.float64, device=fa.device)
    elif tuple(out.shape) != (F, 4) or out.device != fa.device:
        raise ValueError(f"out must be float64 {(F, 4)} on {fa.device}, got {tuple(out.shape)} on {out.device}")
    ws = torch.empty(int(M.vsr_metric_ws_bytes(F, H, W, shave, bits)), dtype=torch.uint8, device=fa.device)
    L.check(M.vsr_metric_frames(pa, pb, F, H, W, bits, METRIC_CHANNELS[channels], 1 if quantise else 0, shave,
                                None if luma4 is None else luma4.ctypes.data_as(ctypes.c_void_p), win.ctypes.data_as(ctypes.c_void_p),
                                L.dptr(out, torch.float64), L.dptr(ws, torch.uint8), L.stream()), "metric_frames", lib=M)
    return out


def psnr_ssim(sums) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `frame_metrics`: sums [F,4] (a tensor, copied to the host here, or an array) -> (PSNR [F] in dB,
    SSIM [F]).  PSNR = 10 log10(255^2 n_sse / sse), `inf` where sse == 0; SSIM = ssim_sum / n_ssim.  A metric that was not asked for
    (its count is 0) comes back as NaN."""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    s = np.asarray(s, dtype=np.float64).reshape(-1, 4)
    sse, n_sse, ssim_sum, n_ssim = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    psnr = np.full(s.shape[0], np.nan)
    ssim = np.full(s.shape[0], np.nan)
    on = n_sse > 0
    psnr[on & (sse == 0)] = np.inf
    pos = on & (sse > 0)
    psnr[pos] = 10.0 * np.log10(255.0 ** 2 * n_sse[pos] / sse[pos])
    on = n_ssim > 0
    ssim[on] = ssim_sum[on] / n_ssim[on]
    return psnr, ssim


# ------------------------------------------------------------------------------------------------ temporal warping error
WARP_OCC = (0.01, 0.5, 0.01, 0.002)   # {c1, c2, g1, g2} of the occlusion rule (Ruder, Dosovitskiy, Brox 2016)
_truth_flow_exec = None               # model -> its FlowNet2 executor for `truth_flows` (made on first use)


def truth_flows(model, frames_t: torch.Tensor, frames_t1: torch.Tensor):
    """The optical flow between ground-truth frames, the guide of `warp_error`: float32 RGB frames [P,H,W,3] (or [H,W,3]) at time t and
    at time t + 1 -> (forward flows t -> t + 1, backward flows t + 1 -> t, crop (y0, x0, h, w)), all 2 P flows as one FlowNet2 batch over
    the centre crop to multiples of 64, in the precision `model.precision` selects: "fp32" planar float32 [P,2,h,w]; "fp16" the executor's
    NHWC half map [P,h,w,ld] with the flow in channels 0 and 1.  The executor is one of this function's own per model: its buffers hold
    the geometry of the truth frames, and `model._flow_exec`, whose buffers hold the LR geometry of the windows, is left alone."""
    global _truth_flow_exec
    if frames_t.dim() == 3:
        frames_t, frames_t1 = frames_t[None], frames_t1[None]
    if tuple(frames_t.shape) != tuple(frames_t1.shape) or frames_t.dim() != 4 or frames_t.shape[-1] != 3:
        raise ValueError(f"expected two float32 tensors of one shape [H,W,3] or [P,H,W,3], got {tuple(frames_t.shape)} and {tuple(frames_t1.shape)}")
    P = int(frames_t.shape[0])
    net = None
    if model._fast():
        import weakref
        from .trunk_exec import FlowNet2Exec, TrunkExecCache
        if _truth_flow_exec is None:
            _truth_flow_exec = weakref.WeakKeyDictionary()
        if model not in _truth_flow_exec:
            _truth_flow_exec[model] = TrunkExecCache(model.FlowModule.net, FlowNet2Exec)
        net = _truth_flow_exec[model].get()
    pairs = [(frames_t[p], frames_t1[p]) for p in range(P)] + [(frames_t1[p], frames_t[p]) for p in range(P)]
    flows, crop = model.FlowModule.flow_pairs(pairs, net)
    return flows[:P], flows[P:], crop


@L.on_device
def warp_error(a: torch.Tensor, b: torch.Tensor, flows, channels: str = "rgb", quantise: bool = True, shave: int = 0, occ=None,
               out: Optional[torch.Tensor] = None, matrix: str = "bt601", full_range: bool = False, luma4=None) -> torch.Tensor:
    """float32 RGB frames `a` (time t) and `b` (time t + 1) ([H,W,3] or [P,H,W,3], 0..255) and `flows` = (forward, backward, crop) as
    `truth_flows` returns them -> the device tensor [P,4] float64 of {sse, n_terms, n_valid, n_pixels} per pair (vsr_warp_error,
    include/vsr_hip_warp.h): frame b warped back onto frame a along the forward flow, the squared difference summed over the pixels of
    the crop that are in frame, forward-backward consistent and off a motion boundary.  Nothing is synchronised, `ewarp` is the host
    step.  `quantise`, `shave` (counted inside the crop), `channels`, `matrix`, `full_range`: as `frame_metrics`; `luma4`: four float32
    {a0, a1, a2, o} in place of the matrix's luma row; `occ`: {c1, c2, g1, g2}, default `WARP_OCC`; `out`: write the sums there ([P,4]
    float64, rows of a larger tensor will do)."""
    import ctypes
    if channels not in METRIC_CHANNELS:
        raise ValueError(f"unknown channels {channels!r} (known: {', '.join(METRIC_CHANNELS)})")
    fwd, bwd, crop = flows
    if a.dim() == 3:
        a, b = a[None], b[None]
    if tuple(a.shape) != tuple(b.shape) or a.dim() != 4 or a.shape[-1] != 3:
        raise ValueError(f"expected two float32 tensors of one shape [H,W,3] or [P,H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    P, H, W = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    y0, x0, h, w = (int(v) for v in crop)
    shave = int(shave)
    if h <= 0 or w <= 0 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"the crop {(y0, x0, h, w)} leaves the frame of {H} x {W}")
    if shave < 0 or 2 * shave >= min(h, w):
        raise ValueError(f"shave {shave} leaves nothing of the crop of {h} x {w}")
    if fwd.dtype != bwd.dtype or tuple(fwd.shape) != tuple(bwd.shape) or fwd.stride() != bwd.stride():
        raise ValueError("the forward and the backward flows must have one dtype, shape and layout")
    if fwd.dtype == torch.float32 and tuple(fwd.shape) == (P, 2, h, w):
        ftype, strides = 0, (2 * h * w, h * w, 1)                                # VSR_WARP_FLOW_F32, planar
    elif fwd.dtype == torch.float16 and fwd.dim() == 4 and tuple(fwd.shape[:3]) == (P, h, w) and fwd.shape[3] >= 2:
        ftype, strides = 1, (h * w * int(fwd.shape[3]), 1, int(fwd.shape[3]))    # VSR_WARP_FLOW_F16, NHWC with the flow in channels 0, 1
    else:
        raise ValueError(f"flows must be float32 {(P, 2, h, w)} or float16 {(P, h, w)} + (ld,), got {fwd.dtype} {tuple(fwd.shape)}")
    if luma4 is not None:
        luma4 = np.ascontiguousarray(np.asarray(luma4, dtype=np.float32).reshape(4))
    elif channels == "y":
        c = yuv_coefficients("yuv420p", matrix, full_range)
        luma4 = np.ascontiguousarray(np.array([c[0], c[1], c[2], c[9]], dtype=np.float32))
    occ4 = np.ascontiguousarray(np.asarray(WARP_OCC if occ is None else occ, dtype=np.float64).reshape(4))
    fa, fb = a.detach().contiguous(), b.detach().contiguous()
    M = L.load_warp()
    pa, pb = L.dptr(fa), L.dptr(fb)   # (raises on CPU tensors and on anything but float32)
    pf, pg = L.dptr(fwd, fwd.dtype), L.dptr(bwd, bwd.dtype)
    if any(t.device != fa.device for t in (fb, fwd, bwd)):
        raise ValueError("the frames and the flows live on different devices")
    if out is None:
        out = torch.empty((P, 4), dtype=torch.float64, device=fa.device)
    elif tuple(out.shape) != (P, 4) or out.device != fa.device:
        raise ValueError(f"out must be float64 {(P, 4)} on {fa.device}, got {tuple(out.shape)} on {out.device}")
    ws = torch.empty(int(M.vsr_warp_ws_bytes(P, h, w, shave)), dtype=torch.uint8, device=fa.device)
    L.check(M.vsr_warp_error(pa, pb, P, H, W, y0, x0, h, w, pf, pg, ftype, strides[0], strides[1], strides[2], METRIC_CHANNELS[channels],
                             1 if quantise else 0, shave, None if luma4 is None else luma4.ctypes.data_as(ctypes.c_void_p),
                             occ4.ctypes.data_as(ctypes.c_void_p), L.dptr(out, torch.float64), L.dptr(ws, torch.uint8), L.stream()),
            "warp_error", lib=M)
    return out


def ewarp(sums) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `warp_error`: sums [P,4] (a tensor, copied to the host here, or an array) -> (E_warp [P] = sse / n_terms /
    255^2, the mean squared warping error over the valid pixels in the 0..1 range of Lai et al. 2018; valid share [P] = n_valid /
    n_pixels).  E_warp is NaN where no pixel is valid."""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    s = np.asarray(s, dtype=np.float64).reshape(-1, 4)
    e = np.full(s.shape[0], np.nan)
    on = s[:, 2] > 0
    e[on] = s[on, 0] / s[on, 1] / 255.0 ** 2
    return e, s[:, 2] / s[:, 3]


# ------------------------------------------------------------------------------------------------ resampling
RESIZE_KERNELS = {"bicubic": 2.0, "bilinear": 1.0}   # the support of the filter at scale 1
RESIZE_MAX_TAPS = 33                                 # VSR_RESIZE_MAX_TAPS of include/vsr_hip_resize.h


def _resize_filter(kernel: str, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    if kernel == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5   # Keys' cubic
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


def resize_tables(n_in: int, n_out: int, kernel: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """One axis of an antialiased resize from `n_in` to `n_out` samples as the two tables vsr_resize_frames takes:
    (first int32 [n_out], weight float32 [n_out, K]); output i is sum_k weight[i, k] * in[clamp(first[i] + k)].  Pillow's convention,
    which is also that of torch's `interpolate(antialias=True, align_corners=False)`: scale = n_in / n_out, fs = max(scale, 1), support =
    2 fs ("bicubic": Keys' cubic with a = -0.5) or fs ("bilinear": the triangle), K = 2 ceil(support) + 1; for output i, c = scale (i + 0.5),
    lo = max(int(c - support + 0.5), 0), hi = min(int(c + support + 0.5), n_in), w_j = filter((j + lo - c + 0.5) / fs) for j < hi - lo over
    their sum, first = lo; the taps from hi - lo to K - 1 carry weight 0.  Computed in float64, the weights rounded once to float32;
    this is the single source of the coefficients (the C side computes none)."""
    if kernel not in RESIZE_KERNELS:
        raise ValueError(f"unknown kernel {kernel!r} (known: {', '.join(RESIZE_KERNELS)})")
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = RESIZE_KERNELS[kernel] * fs
    K = 2 * int(np.ceil(support)) + 1
    if K > RESIZE_MAX_TAPS:
        raise ValueError(f"{kernel} from {n_in} to {n_out} needs {K} taps, beyond the {RESIZE_MAX_TAPS} of the library")
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum((c - support + 0.5).astype(np.int64), 0)       # (int(): truncation; the arguments of the ones that matter are >= 0)
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    j = np.arange(K, dtype=np.float64)[None, :]
    wt = _resize_filter(kernel, (j + lo[:, None] - c[:, None] + 0.5) / fs)
    wt = np.where(j < (hi - lo)[:, None], wt, 0.0)
    wt = wt / wt.sum(axis=1, keepdims=True)
    return lo.astype(np.int32), np.ascontiguousarray(wt.astype(np.float32))


@L.on_device
def resize_frames(src: torch.Tensor, out_shape: Tuple[int, int], x_first: torch.Tensor, x_weight: torch.Tensor, y_first: torch.Tensor,
                  y_weight: torch.Tensor, quantise: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The low-level call (vsr_resize_frames) with any tables on the device: src float32 [F,H,W,3] (or [H,W,3]) -> [F,h,w,3] ([h,w,3]);
    x_first int32 [w], x_weight float32 [w,KX], y_first int32 [h], y_weight float32 [h,KY]."""
    if src.dim() not in (3, 4) or src.shape[-1] != 3:
        raise ValueError(f"expected float32 [F,H,W,3] or [H,W,3], got {tuple(src.shape)}")
    h, w = int(out_shape[0]), int(out_shape[1])
    H, W = int(src.shape[-3]), int(src.shape[-2])
    lead = tuple(src.shape[:-3])
    F = int(src.shape[0]) if src.dim() == 4 else 1
    if tuple(x_first.shape) != (w,) or x_weight.dim() != 2 or x_weight.shape[0] != w or tuple(y_first.shape) != (h,) or y_weight.dim() != 2 \
            or y_weight.shape[0] != h:
        raise ValueError(f"tables do not fit {h} x {w}: x {tuple(x_first.shape)} / {tuple(x_weight.shape)}, y {tuple(y_first.shape)} / "
                         f"{tuple(y_weight.shape)}")
    R = L.load_resize()
    ps = L.dptr(src)   # (raises on CPU tensors, on anything but float32 and on strided views)
    if out is None:
        out = torch.empty(lead + (h, w, 3), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != lead + (h, w, 3) or out.device != src.device:
        raise ValueError(f"out must be float32 {lead + (h, w, 3)} on {src.device}, got {tuple(out.shape)} on {out.device}")
    L.check(R.vsr_resize_frames(ps, L.dptr(out), F, H, W, h, w, L.dptr(x_first, torch.int32), L.dptr(x_weight), int(x_weight.shape[1]),
                                L.dptr(y_first, torch.int32), L.dptr(y_weight), int(y_weight.shape[1]), 1 if quantise else 0, L.stream()),
            "resize_frames", lib=R)
    return out


class FrameResizer:
    """Frames of `in_shape` = (H, W) resampled to `out_shape` = (h, w) by `kernel` ("bicubic" | "bilinear", antialiased: `resize_tables`):
    the four tables are built and uploaded once; `resizer(src [F,H,W,3] or [H,W,3] float32 on the device, quantise=False, out=None)`
    enqueues one launch on the current stream.  `quantise`: the result as an 8-bit file would hold it (clamped to 0..255, rounded half to
    even); without it a bicubic result may leave 0..255."""

    def __init__(self, in_shape: Tuple[int, int], out_shape: Tuple[int, int], kernel: str = "bicubic", device="cuda"):
        self.in_shape = (int(in_shape[0]), int(in_shape[1]))
        self.out_shape = (int(out_shape[0]), int(out_shape[1]))
        self.kernel = kernel
        yf, yw = resize_tables(self.in_shape[0], self.out_shape[0], kernel)
        xf, xw = resize_tables(self.in_shape[1], self.out_shape[1], kernel)
        self.device = torch.device(device)
        self.y_first, self.y_weight, self.x_first, self.x_weight = (torch.from_numpy(a).to(self.device) for a in (yf, yw, xf, xw))

    def __call__(self, src: torch.Tensor, quantise: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not src.is_cuda:
            raise L.VsrHipError("device path called with a CPU tensor (no CPU fallback exists)")
        if src.dim() not in (3, 4) or tuple(src.shape[-3:]) != self.in_shape + (3,):
            raise ValueError(f"expected float32 [F,{self.in_shape[0]},{self.in_shape[1]},3], got {tuple(src.shape)}")
        if src.device != self.x_first.device:
            raise ValueError(f"the tables live on {self.x_first.device}, the frames on {src.device}")
        return resize_frames(src, self.out_shape, self.x_first, self.x_weight, self.y_first, self.y_weight, quantise, out)


# ------------------------------------------------------------------------------------------------ Y'CbCr 4:2:0 in and out
YUV_FORMATS = {"yuv420p": 0, "nv12": 1, "yuv420p10le": 2, "p010le": 3}      # the `fmt` codes of include/vsr_hip_yuv.h
YUV_SITINGS = {"left": 0, "center": 1}
_YUV_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}   # bt2020: non-constant luminance


def _yuv_depth(fmt: str) -> int:
    if fmt not in YUV_FORMATS:
        raise ValueError(f"unknown pixel format {fmt!r} (known: {', '.join(YUV_FORMATS)})")
    return 10 if fmt in ("yuv420p10le", "p010le") else 8


def yuv_frame_bytes(fmt: str, H: int, W: int) -> int:
    """Bytes of one packed 4:2:0 frame: 3/2 samples per pixel, 1 byte (8-bit formats) or 2 bytes (10-bit formats) per sample."""
    d = _yuv_depth(fmt)
    if H <= 0 or W <= 0 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 needs positive even H and W, got {H} x {W}")
    return H * W * 3 // 2 * (2 if d == 10 else 1)


def yuv_coefficients(fmt: str, matrix: str = "bt709", full_range: bool = False, inverse: bool = False, dtype=np.float32) -> np.ndarray:
    """The 12 values the device entries take: a row-major 3x3 matrix, then 3 offsets.  Forward (`inverse=False`): the model's R'G'B'
    in 0..255 -> the code values (Y, Cb, Cr) of `fmt`, what `frames_to_yuv` applies; `inverse=True`: code values -> R'G'B' in 0..255,
    what `ingest_item_yuv` applies.  With (Kr, Kb) of `matrix`, Kg = 1 - Kr - Kb, E'Y = Kr R + Kg G + Kb B, E'Cb = (B - E'Y) / (2 (1 - Kb)),
    E'Cr = (R - E'Y) / (2 (1 - Kr)) on R'G'B' in 0..1 and d the bit depth: limited range Y = (16 + 219 E'Y) 2^(d-8),
    C = (128 + 224 E'C) 2^(d-8); full range Y = (2^d - 1) E'Y, C = 2^(d-1) + (2^d - 1) E'C.  Computed in float64 and rounded once to
    `dtype`; this is the single source of the coefficients (the C side computes none)."""
    d = _yuv_depth(fmt)
    if matrix not in _YUV_KR_KB:
        raise ValueError(f"unknown matrix {matrix!r} (known: {', '.join(_YUV_KR_KB)})")
    kr, kb = _YUV_KR_KB[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        sy = sc = float(2 ** d - 1)
        oy, oc = 0.0, float(2 ** (d - 1))
    else:
        m = float(2 ** (d - 8))
        sy, sc, oy, oc = 219.0 * m, 224.0 * m, 16.0 * m, 128.0 * m
    gy, gc = sy / 255.0, sc / 255.0
    if not inverse:
        A = np.array([[gy * kr, gy * kg, gy * kb],
                      [-gc * kr / (2 * (1 - kb)), -gc * kg / (2 * (1 - kb)), gc * 0.5],
                      [gc * 0.5, -gc * kg / (2 * (1 - kr)), -gc * kb / (2 * (1 - kr))]], dtype=np.float64)
        o = np.array([oy, oc, oc], dtype=np.float64)
    else:
        A = np.array([[1 / gy, 0.0, 2 * (1 - kr) / gc],
                      [1 / gy, -2 * (1 - kb) * kb / kg / gc, -2 * (1 - kr) * kr / kg / gc],
                      [1 / gy, 2 * (1 - kb) / gc, 0.0]], dtype=np.float64)
        o = -A @ np.array([oy, oc, oc], dtype=np.float64)
    return np.concatenate([A.reshape(-1), o]).astype(dtype)


def read_clip_yuv(path: str, shape: Tuple[int, int], fmt: str) -> np.ndarray:
    """A headerless 4:2:0 clip (`ffmpeg -f rawvideo -pix_fmt <fmt>`) as uint8 [T, frame_bytes]; `shape` = (H, W)."""
    fb = yuv_frame_bytes(fmt, shape[0], shape[1])
    a = np.fromfile(path, dtype=np.uint8)
    if a.size == 0 or a.size % fb:
        raise ValueError(f"{path}: {a.size} bytes is not a whole number of {fmt} frames of {shape[0]}x{shape[1]} ({fb} bytes each)")
    return a.reshape(-1, fb)


def _coef12(coef12) -> np.ndarray:
    c = np.ascontiguousarray(np.asarray(coef12, dtype=np.float32).reshape(-1))
    if c.size != 12:
        raise ValueError(f"expected 12 coefficients (3x3 matrix, 3 offsets), got {c.size}")
    return c


@L.on_device
def yuv_ingest(frames: torch.Tensor, shape: Tuple[int, int], fmt: str, coef12, siting: str = "left", lr_shape: Optional[Tuple[int, int]] = None,
               want_hr: bool = False, lr_out: Optional[torch.Tensor] = None):
    """The low-level call (vsr_yuv_ingest) with any 12 coefficients: uint8 [..., frame_bytes] on the device -> float32 RGB
    (lr [..., h, w, 3], hr [..., H, W, 3] | None); `lr_shape` = (h, w), default the full size; `lr_out`: write lr there."""
    import ctypes
    H, W = int(shape[0]), int(shape[1])
    fb = yuv_frame_bytes(fmt, H, W)
    if frames.dtype != torch.uint8 or frames.dim() < 1 or frames.shape[-1] != fb:
        raise ValueError(f"expected uint8 [..., {fb}] ({fmt} {H}x{W}), got {frames.dtype} {tuple(frames.shape)}")
    h, w = (H, W) if lr_shape is None else (int(lr_shape[0]), int(lr_shape[1]))
    lead = tuple(frames.shape[:-1])
    F = int(np.prod(lead)) if lead else 1
    c = _coef12(coef12)
    lr = torch.empty(lead + (h, w, 3), dtype=torch.float32, device=frames.device) if lr_out is None else lr_out
    if tuple(lr.shape) != lead + (h, w, 3):
        raise ValueError(f"lr_out must be {lead + (h, w, 3)}, got {tuple(lr.shape)}")
    hr = torch.empty(lead + (H, W, 3), dtype=torch.float32, device=frames.device) if want_hr else None
    Y = L.load_yuv()
    L.check(Y.vsr_yuv_ingest(L.dptr(frames, torch.uint8), YUV_FORMATS[fmt], c.ctypes.data_as(ctypes.c_void_p), YUV_SITINGS[siting], L.dptr(lr),
                             L.optr(hr), F, H, W, h, w, L.stream()), "yuv_ingest", lib=Y)
    return lr, hr


@L.on_device
def yuv_write(frames: torch.Tensor, fmt: str, coef12, siting: str = "left", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The low-level call (vsr_yuv_write) with any 12 coefficients: float32 [..., H, W, 3] -> uint8 [..., frame_bytes]."""
    import ctypes
    if frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError(f"expected float32 [..., H, W, 3], got {tuple(frames.shape)}")
    f = frames.detach().to(torch.float32).contiguous()
    H, W = int(f.shape[-3]), int(f.shape[-2])
    fb = yuv_frame_bytes(fmt, H, W)
    lead = tuple(f.shape[:-3])
    F = int(np.prod(lead)) if lead else 1
    c = _coef12(coef12)
    if out is None:
        out = torch.empty(lead + (fb,), dtype=torch.uint8, device=f.device)
    elif tuple(out.shape) != lead + (fb,):
        raise ValueError(f"out must be {lead + (fb,)}, got {tuple(out.shape)}")
    Y = L.load_yuv()
    L.check(Y.vsr_yuv_write(L.dptr(f), L.dptr(out, torch.uint8), YUV_FORMATS[fmt], c.ctypes.data_as(ctypes.c_void_p), YUV_SITINGS[siting],
                            F, H, W, L.stream()), "yuv_write", lib=Y)
    return out


def ingest_item_yuv(frames: torch.Tensor, shape: Tuple[int, int], fmt: str, scale: int = 4, want_hr: bool = True, matrix: str = "bt709",
                    full_range: bool = False, siting: str = "left"):
    """`ingest_item` for 4:2:0 frames: uint8 [T,3,frame_bytes] on the device -> (data [T,3,H//s,W//s,3], target [T,1,H,W,3] | None,
    high_frames [T,3,H,W,3] | None), float32 R'G'B' in 0..255."""
    if frames.dim() != 3 or frames.shape[1] != 3:
        raise ValueError(f"expected uint8 [T,3,frame_bytes], got {frames.dtype} {tuple(frames.shape)}")
    H, W = shape
    lr, hr = yuv_ingest(frames.contiguous(), shape, fmt, yuv_coefficients(fmt, matrix, full_range, inverse=True), siting,
                        (int(H / scale), int(W / scale)), want_hr)
    if hr is None:
        return lr, None, None
    return lr, hr[:, 1:2].clone(), hr   # (the clone: as in ingest_item)


def frames_to_yuv(frames: torch.Tensor, fmt: str, matrix: str = "bt709", full_range: bool = False, siting: str = "left") -> torch.Tensor:
    """float32 HR frames [...,H,W,3] (R'G'B' in 0..255) -> packed 4:2:0 frames uint8 [...,frame_bytes]: values clamped to 0..255, chroma
    from the filtered R'G'B', round half to even, clamped to the code range."""
    return yuv_write(frames, fmt, yuv_coefficients(fmt, matrix, full_range), siting)


# ------------------------------------------------------------------------------------------------ the per-item loop
def run_item(model, data, target, high_frames, train: bool = False, estimated_image=None):
    """main.py:196-203 for one dataset item: windows in order, the output of one fed back as the next `estimated_image`.
    -> (outputs [T,H,W,3] float32, losses list, last estimate)."""
    outs, losses = [], []
    T = data.shape[0]
    with torch.no_grad():
        for t in range(T):
            x = data[t]
            y = target[t] if target is not None else None
            hf = high_frames[t] if high_frames is not None else None
            output, loss = model(x, y, hf, estimated_image, train=train)
            estimated_image = output
            outs.append(output[0])
            if loss is not None:
                losses.append(loss.data)
    return torch.stack(outs), losses, estimated_image


def train_step(model, optimizer, x, y, high_frame, estimated_image, loss_value=None):
    """main.py:206-210 for one window, without the host round trip of :207: the differentiable call (the SR net through
    sr_train.forward_train), the fake MSE against `y` on the device, `loss.data` overwritten by `loss_value` when given (:208, the mean
    of the no-grad windows' losses), backward, `optimizer.step()`.  `optimizer`: optim.Adam (update and clip on the device path) or
    any torch optimizer.  The caller zeroes the gradients (:197).  -> (output detached, loss)."""
    import torch.nn.functional as F
    output, _ = model(x, y, high_frame, estimated_image)
    loss = F.mse_loss(output, y.detach().float())
    if loss_value is not None:
        loss.data = torch.as_tensor(loss_value, dtype=loss.dtype, device=loss.device).reshape(())
    loss.backward()
    optimizer.step()
    return output.detach(), loss


class ClipRunner:
    """A 4:2:0 clip streamed through `model` frame by frame.  `shape` = (H, W) of the source frames in `fmt_in`; the model sees them
    decimated by `scale_down` (1: as they are) and returns frames of (S * (H // scale_down), S * (W // scale_down)), written out as
    `fmt_out`.  `run(frames)`: host array [T, frame_bytes] -> host array [T-2, out_frame_bytes] (one frame per 3-frame window).

    Per source frame: one upload from one of two pinned slots on the copy-in stream, one conversion into a slot of a three-slot LR
    ring; per window: the ring's slots stacked on the device, `model(x, None, None, est, train=False)` on the current stream with the
    estimate fed back (as `run_item`), `frames_to_yuv`'s kernel into one of two device slots, the copy back into one of two pinned
    slots on the copy-out stream.  Events order every reuse of a slot; the host waits on events only, never on the device.
    `overlap=False`: both copy streams ARE the current stream -- the same work in one stream's order (the cross-check).
    `h2d_bytes`, `d2h_bytes`, `frames_in`, `frames_out` count what the last `run()` moved (reset when a run starts).

    `score="rgb" | "y"` (only where the output frame has the source's shape, `scale_down == S`): output frame j is scored against source
    frame j + 1, the middle frame of its window (`target = datas[:, 1:2]` in the reference's loop), which is still resident in its
    upload slot when the window runs: one more conversion at full size into a reused HR buffer and `frame_metrics` of the float
    estimate (quantised as write-out does, `shave` pixels dropped on every side, default S; "y" is `frame_metrics`' BT.601 luma whatever
    `matrix` the frames are coded with) into row j of one [T-2,4] tensor; nothing
    extra is uploaded, and one copy at the end gives `metrics = {"psnr": [T-2], "ssim": [T-2]}`.

    `decimate="nearest"` (default): the LR frame is the conversion's own nearest-neighbour decimation (the reference's `interpolate` at
    main.py:157).  `decimate="bicubic"`: every uploaded frame is converted at full size into a reused HR buffer of its own (not the one the
    scored window's truth lives in) and reduced into its ring slot by `FrameResizer(quantise=True)`: the antialiased bicubic LR frame as an
    8-bit file would hold it, the evaluation protocol of the literature.  `baseline="bicubic"` (needs `score`): per window the middle LR
    frame of the ring is enlarged to the output shape into a reused buffer and scored against the same truth with the same quantise,
    shave and channels as the estimate, into a second [T-2,4] tensor copied with the first: `metrics` gains `psnr_baseline` and
    `ssim_baseline`.  Neither uploads or downloads a byte more; with both at their defaults the launches are the ones described above.

    `temporal="warp"` (needs `score`): the temporal warping error of the output (`warp_error`, Lai et al. 2018).  For every output frame
    j >= 1 the pair (j - 1, j) is scored along the flows between the source frames j and j + 1 (`truth_flows`, both directions in one
    FlowNet2 batch, in the model's precision): the previous estimate and the previous truth frame are kept (`_truth` is then two
    alternating buffers), and the pair of truth frames is scored along the same flows: the floor any method sits above.  With
    `baseline="bicubic"` the baseline pair is scored too (`_base` is then two alternating buffers).  Same channels, quantise and shave
    (counted inside the flow's centre crop) as the per-frame scores, `occ` as `warp_error`'s (default: the published constants), into [T-3,4] tensors that travel in the one copy at the end:
    `metrics` gains `ewarp`, `ewarp_truth`, `valid_share` (the occlusion mask depends on the flows alone: one share for all) and, with a
    baseline, `ewarp_baseline`, each [T-3] (empty for T = 3).  No upload, download or host wait is added; with `temporal=None` the
    launches are the ones described above."""

    DECIMATE = ("nearest", "bicubic")
    BASELINE = (None, "bicubic")
    TEMPORAL = (None, "warp")

    def __init__(self, model, shape: Tuple[int, int], fmt_in: str, fmt_out: str, scale_down: int = 1, overlap: bool = True,
                 matrix: str = "bt709", full_range: bool = False, siting: str = "left", score: Optional[str] = None,
                 shave: Optional[int] = None, decimate: str = "nearest", baseline: Optional[str] = None, temporal: Optional[str] = None,
                 occ=None):
        if decimate not in self.DECIMATE:
            raise ValueError(f"decimate must be 'nearest' or 'bicubic', got {decimate!r}")
        if baseline not in self.BASELINE:
            raise ValueError(f"baseline must be None or 'bicubic', got {baseline!r}")
        if baseline is not None and score is None:
            raise ValueError(f"baseline={baseline!r} is scored beside the estimate: it needs score='rgb' or 'y'")
        if temporal not in self.TEMPORAL:
            raise ValueError(f"temporal must be None or 'warp', got {temporal!r}")
        if temporal is not None and score is None:
            raise ValueError(f"temporal={temporal!r} is scored beside the estimate: it needs score='rgb' or 'y'")
        if occ is not None and temporal is None:
            raise ValueError("occ is given but no temporal score is asked for (temporal=None)")
        self.decimate, self.baseline, self.temporal, self.occ = decimate, baseline, temporal, occ
        self.model, self.fmt_in, self.fmt_out, self.overlap, self.siting = model, fmt_in, fmt_out, bool(overlap), siting
        H, W = int(shape[0]), int(shape[1])
        self.shape = (H, W)
        self.lr_shape = (int(H / scale_down), int(W / scale_down))
        S = int(model.model.upscale_factor)
        self.out_shape = (S * self.lr_shape[0], S * self.lr_shape[1])
        if score is not None and score not in METRIC_CHANNELS:
            raise ValueError(f"score must be None, 'rgb' or 'y', got {score!r}")
        if score is None and shave is not None:
            raise ValueError("shave is given but nothing is scored (score=None)")
        if score is not None and self.out_shape != self.shape:
            raise ValueError(f"score={score!r} needs output frames of the source's shape: {self.shape} in, {self.out_shape} out "
                             f"(scale_down {scale_down}, x{S})")
        self.score, self.shave = score, (S if shave is None else int(shave))
        if score is not None and (self.shave < 0 or min(self.shape) - 2 * self.shave < 11):
            raise ValueError(f"shave {self.shave} leaves less than SSIM's 11 pixels of {self.shape}")
        self.metrics = None   # of the last run(): {"psnr": [T-2], "ssim": [T-2]} when scoring
        self.in_bytes = yuv_frame_bytes(fmt_in, H, W)
        self.out_bytes = yuv_frame_bytes(fmt_out, *self.out_shape)
        self.coef_in = yuv_coefficients(fmt_in, matrix, full_range, inverse=True)
        self.coef_out = yuv_coefficients(fmt_out, matrix, full_range)
        self.device = next(model.parameters()).device
        dev = self.device
        self._pin_in = [torch.empty(self.in_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._pin_out = [torch.empty(self.out_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._dev_in = [torch.empty(self.in_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._dev_out = [torch.empty(self.out_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._ring = [torch.empty(self.lr_shape + (3,), dtype=torch.float32, device=dev) for _ in range(3)]
        self._truth = torch.empty(self.shape + (3,), dtype=torch.float32, device=dev) if score is not None else None
        if temporal is not None:   # the truth frame of the previous window stays: two alternating buffers
            self._truth = [self._truth, torch.empty(self.shape + (3,), dtype=torch.float32, device=dev)]
        self._full = self._down = self._up = self._base = None
        if decimate == "bicubic":
            self._full = torch.empty(self.shape + (3,), dtype=torch.float32, device=dev)   # the frame being reduced; `_truth` is the window's
            self._down = FrameResizer(self.shape, self.lr_shape, "bicubic", dev)
        if baseline is not None:
            self._base = torch.empty(self.out_shape + (3,), dtype=torch.float32, device=dev)
            self._up = FrameResizer(self.lr_shape, self.out_shape, baseline, dev)
            if temporal is not None:
                self._base = [self._base, torch.empty(self.out_shape + (3,), dtype=torch.float32, device=dev)]
        self._s_in = torch.cuda.Stream(dev) if self.overlap else None
        self._s_out = torch.cuda.Stream(dev) if self.overlap else None
        self.h2d_bytes = self.d2h_bytes = self.frames_in = self.frames_out = 0   # of the last run()

    @property
    def h2d_bytes_per_frame(self) -> float:
        return self.h2d_bytes / max(self.frames_in, 1)

    def run(self, frames: np.ndarray) -> np.ndarray:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != self.in_bytes or frames.shape[0] < 3:
            raise ValueError(f"expected uint8 [T >= 3, {self.in_bytes}], got {frames.dtype} {frames.shape}")
        T = frames.shape[0]
        out = np.empty((T - 2, self.out_bytes), dtype=np.uint8)
        self.h2d_bytes = self.d2h_bytes = self.frames_in = self.frames_out = 0
        self.metrics = None
        with torch.cuda.device(self.device), torch.no_grad():
            sums = torch.empty((T - 2, 4), dtype=torch.float64, device=self.device) if self.score is not None else None
            sums_base = torch.empty((T - 2, 4), dtype=torch.float64, device=self.device) if self.baseline is not None else None
            warp = self.temporal is not None
            sums_warp = [torch.empty((T - 3, 4), dtype=torch.float64, device=self.device)
                         for _ in range((2 + (self.baseline is not None)) if warp else 0)]   # the estimate's pairs, the truth's, the baseline's
            prev_est = None
            main = torch.cuda.current_stream(self.device)
            s_in, s_out = (self._s_in, self._s_out) if self.overlap else (main, main)
            uploaded = [None, None]    # per input slot: the upload from its pinned buffer has finished (event on s_in)
            converted = [None, None]   # per input slot: the conversion has read its device buffer (event on main)
            copied = [None, None]      # per output slot: (frame index, event on s_out: the copy into its pinned buffer has finished)
            est = None
            for i in range(T):
                a = i % 2
                if uploaded[a] is not None:
                    uploaded[a].synchronize()   # the pinned slot is free again (host wait on one event)
                self._pin_in[a].numpy()[:] = frames[i]
                if converted[a] is not None:
                    s_in.wait_event(converted[a])
                with torch.cuda.stream(s_in):
                    self._dev_in[a].copy_(self._pin_in[a], non_blocking=True)
                    uploaded[a] = torch.cuda.Event()
                    uploaded[a].record(s_in)
                self.h2d_bytes += self.in_bytes
                self.frames_in += 1
                main.wait_event(uploaded[a])
                # (ring slot i % 3 was last read by the window of frames i-3 .. i-1, stacked on this stream)
                if self._down is None:
                    yuv_ingest(self._dev_in[a], self.shape, self.fmt_in, self.coef_in, self.siting, self.lr_shape, lr_out=self._ring[i % 3])
                else:   # (the HR buffer was last read by the previous frame's reduction, on this stream)
                    yuv_ingest(self._dev_in[a], self.shape, self.fmt_in, self.coef_in, self.siting, lr_out=self._full)
                    self._down(self._full, quantise=True, out=self._ring[i % 3])
                converted[a] = torch.cuda.Event()
                converted[a].record(main)
                if i < 2:
                    continue
                j = i - 2          # the output frame
                b = j % 2
                x = torch.stack([self._ring[(i - 2) % 3], self._ring[(i - 1) % 3], self._ring[i % 3]])
                est, _ = self.model(x, None, None, est, train=False)
                if sums is not None:
                    # source frame j + 1 = i - 1 is still in its upload slot (the other one of the pair): converted at full size into the
                    # reused HR buffer, then scored; the slot's next upload waits for this read as it does for the LR conversion
                    c = (i - 1) % 2
                    truth = self._truth[j % 2] if warp else self._truth
                    base = self._base[j % 2] if warp and sums_base is not None else self._base
                    yuv_ingest(self._dev_in[c], self.shape, self.fmt_in, self.coef_in, self.siting, lr_out=truth)
                    frame_metrics(est[0], truth, self.score, True, self.shave, out=sums[j:j + 1])
                    if sums_base is not None:
                        self._up(self._ring[(i - 1) % 3], quantise=False, out=base)
                        frame_metrics(base, truth, self.score, True, self.shave, out=sums_base[j:j + 1])
                    if warp and j >= 1:
                        # the pair (j - 1, j) along the flows between source frames j and j + 1: the other truth buffer still holds
                        # source frame j, `prev_est` the estimate of the window before
                        truth_prev = self._truth[(j - 1) % 2]
                        flows = truth_flows(self.model, truth_prev, truth)
                        warp_error(prev_est, est[0], flows, self.score, True, self.shave, self.occ, out=sums_warp[0][j - 1:j])
                        warp_error(truth_prev, truth, flows, self.score, True, self.shave, self.occ, out=sums_warp[1][j - 1:j])
                        if sums_base is not None:
                            warp_error(self._base[(j - 1) % 2], base, flows, self.score, True, self.shave, self.occ, out=sums_warp[2][j - 1:j])
                    prev_est = est[0]
                    converted[c] = torch.cuda.Event()
                    converted[c].record(main)
                if copied[b] is not None:   # frame j-2 leaves the slot pair: wait for its copy, take it from the pinned buffer
                    jj, ev = copied[b]
                    ev.synchronize()
                    out[jj] = self._pin_out[b].numpy()
                    main.wait_event(ev)
                yuv_write(est[0], self.fmt_out, self.coef_out, self.siting, out=self._dev_out[b])
                ready = torch.cuda.Event()
                ready.record(main)
                s_out.wait_event(ready)
                with torch.cuda.stream(s_out):
                    self._pin_out[b].copy_(self._dev_out[b], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(s_out)
                copied[b] = (j, ev)
                self.d2h_bytes += self.out_bytes
                self.frames_out += 1
            for b in range(2):
                if copied[b] is not None:
                    jj, ev = copied[b]
                    ev.synchronize()
                    out[jj] = self._pin_out[b].numpy()
            for ev in uploaded + converted:   # the slots are idle when run() returns
                if ev is not None:
                    ev.synchronize()
            if warp:
                rows = torch.cat([sums] + ([sums_base] if sums_base is not None else []) + sums_warp).cpu().numpy()   # the one copy
                psnr, ssim = psnr_ssim(rows[:T - 2])
                self.metrics = {"psnr": psnr, "ssim": ssim}
                at = T - 2
                if sums_base is not None:
                    self.metrics["psnr_baseline"], self.metrics["ssim_baseline"] = psnr_ssim(rows[at:at + T - 2])
                    at += T - 2
                self.metrics["ewarp"], self.metrics["valid_share"] = ewarp(rows[at:at + T - 3])
                self.metrics["ewarp_truth"], _ = ewarp(rows[at + T - 3:at + 2 * (T - 3)])
                if sums_base is not None:
                    self.metrics["ewarp_baseline"], _ = ewarp(rows[at + 2 * (T - 3):at + 3 * (T - 3)])
            elif sums is not None:
                if sums_base is None:
                    psnr, ssim = psnr_ssim(sums)   # the one copy (it waits for the current stream)
                    self.metrics = {"psnr": psnr, "ssim": ssim}
                else:
                    both = torch.stack([sums, sums_base]).cpu().numpy()   # still one copy
                    psnr, ssim = psnr_ssim(both[0])
                    psnr_b, ssim_b = psnr_ssim(both[1])
                    self.metrics = {"psnr": psnr, "ssim": ssim, "psnr_baseline": psnr_b, "ssim_baseline": ssim_b}
        return out


# ------------------------------------------------------------------------------------------------ checkpoints
def save_checkpoint(state, is_best, path, prefix, filename="checkpoint.pth.tar"):
    """utils/tools.py:68-73, same file naming."""
    prefix_save = os.path.join(path, prefix)
    name = prefix_save + "_" + filename
    torch.save(state, name)
    if is_best:
        shutil.copyfile(name, prefix_save + "_model_best.pth.tar")
    return name


def checkpoint_state(model, epoch: int, optimizer=None, arch: str = "VSR") -> dict:
    """The dict main.py:233-237 / :248-252 saves: only the SR net's state_dict is checkpointed."""
    return {"arch": arch, "epoch": epoch, "state_dict": model.model.state_dict(), "optimizer": optimizer}


def load_checkpoint(model, path: str, map_location=None, trusted: bool = False) -> dict:
    """main.py:108-122: `SRmodel.model.load_state_dict(checkpoint['state_dict'])` (strict).
    The file is first read with `weights_only=True` (tensors and plain containers only).  The reference's checkpoints hold
    the pickled Adam OBJECT under 'optimizer' (main.py:236), which that mode refuses: such a file is unpickled in full only
    when the caller says it is `trusted` (unpickling runs arbitrary code from the file)."""
    import pickle
    try:
        ckpt = torch.load(path, map_location=map_location, weights_only=True)
    except pickle.UnpicklingError as e:   # ONLY the weights-only refusal (an object beyond tensors / containers); a missing or
        #                                   corrupt file, a bad map_location etc. propagate as what they are
        if not trusted:
            raise RuntimeError(f"{path} holds pickled objects beyond tensors (the reference saves its optimizer object, "
                               f"main.py:236); pass trusted=True to unpickle it in full -- only for files you trust") from e
        ckpt = torch.load(path, map_location=map_location, weights_only=False)
    model.model.load_state_dict(ckpt["state_dict"])
    return ckpt


# ------------------------------------------------------------------------------------------------ config C1
def synthetic_video(n_frames: int, H: int, W: int, seed: int = 1234) -> np.ndarray:
    """uint8 RGB [T,H,W,3]: blurred-noise scene translated by (2k, k) px per frame (distribution S)."""
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(seed)
    pad = 4 * n_frames
    base = gaussian_filter(rs.uniform(0, 255, size=(H + pad, W + 2 * pad, 3)).astype(np.float32), sigma=(3, 3, 0))
    base = (base - base.min()) / (base.max() - base.min()) * 255.0
    return np.stack([np.floor(base[k:k + H, 2 * k:2 * k + W]) for k in range(n_frames)]).astype(np.uint8)


def run_c1(lr: int = 128, frames: int = 3, scale: int = 4, precision: str = "fp32"):
    """Config C1: a synthetic clip through ingest_item / run_item on the GPU path.
    -> (result line, model, datas uint8 [T,3,H,W,3] on the device, outputs [T,H,W,3])."""
    import time
    from . import VSR
    from .weights import fill_module_
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S = scale
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = precision
    video = synthetic_video(frames, S * lr, S * lr)
    windows = [video[i:i + 3] for i in range(frames - 2)]                 # one dataset item (video_utils.py:25)
    datas = torch.from_numpy(np.stack(windows)).to(dev)                   # main.py:186 `torch.tensor(dataset[batch_idx])`
    data, target, high_frames = ingest_item(datas, S)
    run_item(model, data, target, high_frames)                            # warm-up (packing, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs, _, _ = run_item(model, data, target, high_frames)
    u8 = frames_to_u8(outs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    line = dict(config=f"C1: {frames}-frame {lr}x{lr} LR synthetic clip, x{S}, main-like driver, GPU path",
                precision=precision, windows=len(windows), frames_per_s=round(len(windows) / dt, 3), out_shape=list(u8.shape))
    return line, model, datas, outs


def run_c1_yuv(pix_fmt: str, lr: int = 128, frames: int = 3, scale: int = 4, precision: str = "fp32", score: Optional[str] = None,
               decimate: str = "nearest", baseline: Optional[str] = None, temporal: Optional[str] = None):
    """Config C1 with a 4:2:0 boundary: the synthetic clip as `pix_fmt` frames on the host, streamed through `ClipRunner`
    (decimated by `scale`, super-resolved by `scale`).  -> (result line, output frames uint8 [T-2, frame_bytes] on the host).
    `score`: "rgb" | "y": the line also carries the per-frame PSNR / SSIM against the synthetic HR clip.  `decimate` / `baseline`: as
    `ClipRunner`'s; with a baseline the line carries its mean PSNR / SSIM beside the estimate's and `psnr_gain`, their difference in dB; with
    `temporal` the clip means of E_warp of the estimate, of the truth frames (and of the baseline) and of the valid share (E_warp over the
    pairs that have valid pixels; null where there is none, or no pair: a clip of three frames)."""
    import time
    from . import VSR
    from .weights import fill_module_
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S = scale
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = precision
    video = synthetic_video(frames, S * lr, S * lr)
    clip = frames_to_yuv(torch.from_numpy(video).to(dev).float(), pix_fmt).cpu().numpy()
    runner = ClipRunner(model, (S * lr, S * lr), pix_fmt, pix_fmt, scale_down=S, score=score, decimate=decimate, baseline=baseline,
                        temporal=temporal)
    runner.run(clip)                                                      # warm-up (packing, allocator)
    t0 = time.perf_counter()
    out = runner.run(clip)
    dt = time.perf_counter() - t0
    line = dict(config=f"C1: {frames}-frame {lr}x{lr} LR synthetic clip, x{S}, {pix_fmt} in and out, streamed clip runner, GPU path",
                precision=precision, windows=frames - 2, frames_per_s=round((frames - 2) / dt, 3), out_shape=list(out.shape),
                h2d_bytes_per_frame=runner.in_bytes, d2h_bytes_per_frame=runner.out_bytes)
    if score is not None:
        line.update(score=score, shave=runner.shave, psnr_db=[round(float(v), 4) for v in runner.metrics["psnr"]],
                    ssim=[round(float(v), 6) for v in runner.metrics["ssim"]])
    if decimate != "nearest":
        line.update(decimate=decimate)
    if baseline is not None:
        m = runner.metrics
        line.update(baseline=baseline, psnr_mean_db=round(float(np.mean(m["psnr"])), 4), ssim_mean=round(float(np.mean(m["ssim"])), 6),
                    psnr_baseline_mean_db=round(float(np.mean(m["psnr_baseline"])), 4),
                    ssim_baseline_mean=round(float(np.mean(m["ssim_baseline"])), 6),
                    psnr_gain=round(float(np.mean(m["psnr"]) - np.mean(m["psnr_baseline"])), 4))
    if temporal is not None:
        m = runner.metrics
        mean = lambda v: float(np.mean(v[np.isfinite(v)])) if np.isfinite(v).any() else None   # (no pair, or no valid pixel in any: null)
        line.update(temporal=temporal, ewarp=mean(m["ewarp"]), ewarp_truth=mean(m["ewarp_truth"]), valid_share=mean(m["valid_share"]))
        if baseline is not None:
            line.update(ewarp_baseline=mean(m["ewarp_baseline"]))
    return line, out


def run_c1_train(steps: int, lr: int = 128, frames: int = 3, scale: int = 4, precision: str = "fp32", max_grad_norm: Optional[float] = None,
                 learning_rate: float = 1e-3, loss_path: str = "reference"):
    """Config C1's clip, then `steps` train steps on its last window (main.py:196-210 with optim.Adam): the no-grad windows give the
    loss value and the estimate, each step is `train_step`.  -> result line with the loss per step and, with `max_grad_norm`, the
    gradient norm per step (read back once, after the last step).  `loss_path` is VSR.loss_path: with "fused" the windows' losses and their
    mean stay on the device."""
    from . import optim
    line, model, datas, _ = run_c1(lr, frames, scale, precision)
    model.loss_path = loss_path
    data, target, high_frames = ingest_item(datas, scale)
    model.train()
    optimizer = optim.Adam(model.parameters(), lr=learning_rate, max_grad_norm=max_grad_norm)
    losses, norms_sq = [], []
    for _ in range(steps):
        optimizer.zero_grad()
        _, window_losses, est = run_item(model, data, target, high_frames, train=True)                 # main.py:199-203
        _, loss = train_step(model, optimizer, data[-1], target[-1], high_frames[-1], est, sum(window_losses) / len(window_losses))
        losses.append(loss.detach())
        if optimizer.last_grad_norm_sq is not None:
            norms_sq.append(optimizer.last_grad_norm_sq.clone())
    line.update(train_steps=steps, learning_rate=learning_rate, max_grad_norm=max_grad_norm, loss_path=loss_path,
                loss=[round(float(v), 6) for v in torch.stack(losses).cpu()] if losses else [],
                grad_norm=[round(float(v) ** 0.5, 6) for v in torch.stack(norms_sq).cpu()] if norms_sq else None)
    return line, model


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="config C1: a synthetic clip through the main.py-like plumbing on the GPU path")
    ap.add_argument("--lr", type=int, default=128, help="LR frame size (BASELINE.json C1: 128)")
    ap.add_argument("--frames", type=int, default=3, help="frames of the clip (3 = one window)")
    ap.add_argument("--scale", type=int, default=4, choices=[2, 3, 4], help="4 = the reference's geometry; 2 = C1's label")
    ap.add_argument("--precision", default="fp32", choices=["fp16", "fp32"])
    ap.add_argument("--pix-fmt", default=None, choices=sorted(YUV_FORMATS),
                    help="the clip enters and leaves as 4:2:0 frames of this format through ClipRunner (default: the RGB path)")
    ap.add_argument("--score", default=None, choices=sorted(METRIC_CHANNELS),
                    help="with --pix-fmt: per-frame PSNR / SSIM of the output against the synthetic HR clip, on RGB or on luma (BT.601 Y)")
    ap.add_argument("--decimate", default="nearest", choices=list(ClipRunner.DECIMATE),
                    help="with --pix-fmt: how the LR frames are made (nearest: the reference's decimation; bicubic: antialiased, stored as 8-bit)")
    ap.add_argument("--baseline", default=None, choices=["bicubic"],
                    help="with --score: also score the bicubic enlargement of the LR frame; the line carries both means and psnr_gain")
    ap.add_argument("--temporal", default=None, choices=["warp"],
                    help="with --score: also the flow-warped error between consecutive output frames (E_warp); the line carries the clip means")
    ap.add_argument("--train-steps", type=int, default=None, metavar="K",
                    help="after the no-grad windows: K train steps on the last window (optim.Adam); the line carries the loss per step")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="with --train-steps: clip the global gradient norm at X on the device; the line carries the norm per step")
    ap.add_argument("--loss-path", default=None, choices=["reference", "fused"],
                    help="with --train-steps: VSR.loss_path (default reference; fused: the loss stays on the device)")
    args = ap.parse_args(argv)
    if args.loss_path is not None and args.train_steps is None:
        ap.error("--loss-path needs --train-steps")
    if args.score is not None and args.pix_fmt is None:
        ap.error("--score needs --pix-fmt (the streamed clip runner scores its frames)")
    if args.decimate != "nearest" and args.pix_fmt is None:
        ap.error("--decimate needs --pix-fmt (the streamed clip runner makes the LR frames)")
    if args.baseline is not None and args.score is None:
        ap.error("--baseline needs --score (it is scored beside the estimate)")
    if args.temporal is not None and args.score is None:
        ap.error("--temporal needs --score (it is scored beside the estimate)")
    if args.max_grad_norm is not None and args.train_steps is None:
        ap.error("--max-grad-norm needs --train-steps")
    if args.train_steps is not None:
        if args.pix_fmt is not None or args.train_steps < 0:
            ap.error("--train-steps takes a non-negative count and runs on the RGB path (no --pix-fmt)")
        line, _ = run_c1_train(args.train_steps, args.lr, args.frames, args.scale, args.precision, args.max_grad_norm,
                               loss_path=args.loss_path or "reference")
    elif args.pix_fmt is not None:
        line, _ = run_c1_yuv(args.pix_fmt, args.lr, args.frames, args.scale, args.precision, args.score, args.decimate, args.baseline,
                             args.temporal)
    else:
        line, _, _, _ = run_c1(args.lr, args.frames, args.scale, args.precision)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
