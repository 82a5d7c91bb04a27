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
    train_step / train_item the train step of one window (main.py:206-210) and the whole loop body of one dataset item (:196-210): what
                            `run_c1_train` runs per step on the synthetic clip and `ClipTrainer` per sample of a real one
    save_checkpoint / load_checkpoint   utils/tools.py:68-73 and main.py:108-122,233-237: {'arch','epoch','state_dict':
                            SRmodel.model.state_dict(),'optimizer'} -- files interchange with the reference's
    run_file_train          `--input clip.y4m --train-steps K`: `ClipTrainer` over a streamed file (patches cut and augmented on the
                            device: `patch_table` / `patch_gather` / `patch_item` of `frames`), `--save DIR` writes a checkpoint of
                            tensors and plain containers that `--input ... --checkpoint` takes back; `--avoid-cuts` / `--act-min X`
                            keep the samples off scene cuts and prefer patches with detail (`cell_stats` / `cell_cuts` /
                            `patch_table_select` of `frames`)

The device bindings for frames in, out, resampled and scored (4:2:0 I/O, the resampler, PSNR / SSIM, MS-SSIM, the warping error) live in
`frames`, the streamed `ClipRunner` on top of them in `clip_runner`, `ClipTrainer` in `clip_trainer`; their public names are imported here,
so `driver.frame_metrics`, `driver.ClipRunner`, `driver.ClipTrainer` and the rest resolve.

`python -m video_super_resolution_amd.driver` is BASELINE.json's config C1 (3-frame 128x128 LR synthetic clip through the
main-like plumbing) on the GPU path (`tools/c1_check.py` runs the CPU checker beside it and reports the PSNR between the two:
the package itself never touches the checker).
Decoding compressed video (cv2.VideoCapture, video_utils.py:17-23) is out of scope: a clip enters as a uint8 RGB array
(`.npy`, raw rgb24, or synthetic) or as planar Y'CbCr frames, 4:2:0, 4:2:2 or 4:4:4, in a `.y4m` file or headerless (`ffmpeg -f rawvideo`):
`--input` streams such a file through `ClipRunner.run_stream` (`run_file`), an interlaced one made progressive on the device first
(`--deinterlace frame|field`, `frames.deinterlace`); transfer functions stay out.
"""
from __future__ import annotations

import os
import shutil
from glob import glob
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .clip_runner import ArraySource, ClipRunner, sums_layout  # noqa: F401
from .clip_trainer import ClipTrainer  # noqa: F401
from .frames import (DEINTERLACE, METRIC_CHANNELS, METRIC_WHAT, MSSSIM_BETA, MSSSIM_MIN_SIZE, PIX_FORMATS, RESIZE_KERNELS, RESIZE_MAX_TAPS,  # noqa: F401
                     CELL, PATCH_FLAGS, SCENE_THRESHOLDS, WARP_OCC, YUV_FORMATS, YUV_SITINGS, FrameResizer, ewarp, frame_metrics, frame_msssim, frames_to_pix,
                     frames_to_yuv, ingest_item_pix, ingest_item_yuv, msssim, msssim_levels, patch_gather, patch_item, patch_table,
                     cell_cuts, cell_shape, cell_stats, patch_score, patch_table_select,
                     deint_planes, deint_schedule, deinterlace, deinterlace_clip, deinterlace_planes,
                     pix_coefficients, pix_frame_bytes, pix_ingest, pix_write, psnr_ssim, read_clip_yuv, resize_frames, resize_tables, scene_cuts, scene_flags, scene_sums, scene_window, ssim_window, truth_flows, warp_error,
                     yuv_coefficients, yuv_frame_bytes, yuv_ingest, yuv_write)
from .y4m import RawReader, RawWriter, Y4MReader, Y4MWriter  # noqa: F401


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


def train_item(model, optimizer, data, target, high_frames):
    """main.py:196-210 for one dataset item: the gradients zeroed, the item's windows without gradient (`run_item`: their losses and the
    estimate), then `train_step` on the last window with the mean of the windows' losses as the loss value.  What `run_c1_train` does
    per step on the synthetic clip and `ClipTrainer` per sample of a real one.  -> the step's loss (a 0-d tensor where the loss path left it)."""
    optimizer.zero_grad()
    _, window_losses, est = run_item(model, data, target, high_frames, train=True)                 # main.py:199-203
    _, loss = train_step(model, optimizer, data[-1], target[-1], high_frames[-1], est, sum(window_losses) / len(window_losses))
    return loss.detach()


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
               decimate: str = "nearest", baseline: Optional[str] = None, temporal: Optional[str] = None, scene: Optional[str] = None,
               scene_thresholds=None, cut_at: Optional[int] = None, multiscale: bool = False):
    """Config C1 with a Y'CbCr boundary (`pix_fmt`: any name of `PIX_FORMATS`): the synthetic clip as `pix_fmt` frames on the host, streamed through `ClipRunner`
    (decimated by `scale`, super-resolved by `scale`).  -> (result line, output frames uint8 [T-2, frame_bytes] on the host).
    `score`: "rgb" | "y": the line also carries the per-frame PSNR / SSIM against the synthetic HR clip.  `decimate` / `baseline`: as
    `ClipRunner`'s; with a baseline the line carries its mean PSNR / SSIM beside the estimate's and `psnr_gain`, their difference in dB; with
    `temporal` the clip means of E_warp of the estimate, of the truth frames (and of the baseline) and of the valid share (E_warp over the
    pairs that have valid pixels; null where there is none, or no pair: a clip of three frames).  `cut_at` = K: the clip's frames from K
    on come from a second seed, a scene cut between the frames K - 1 and K.  `scene` / `scene_thresholds`: as `ClipRunner`'s; the line
    then carries `cuts`, the indices i of the pairs (i, i + 1) found to be cuts, and `scene_m`, the mean absolute luma difference per pair.
    `multiscale` (needs `score`): the line also carries the per-frame MS-SSIM as `msssim` (and its baseline mean with a baseline)."""
    import time
    from . import VSR
    from .weights import fill_module_
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S = scale
    model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
    model.precision = model.model.precision = precision
    video = synthetic_video(frames, S * lr, S * lr)
    if cut_at is not None:
        if not 0 < cut_at < frames:
            raise ValueError(f"cut_at must lie inside the clip of {frames} frames, got {cut_at}")
        video[cut_at:] = synthetic_video(frames, S * lr, S * lr, seed=4321)[cut_at:]
    clip = frames_to_pix(torch.from_numpy(video).to(dev).float(), pix_fmt).cpu().numpy()
    runner = ClipRunner(model, (S * lr, S * lr), pix_fmt, pix_fmt, scale_down=S, score=score, decimate=decimate, baseline=baseline,
                        temporal=temporal, scene=scene, scene_thresholds=scene_thresholds, multiscale=multiscale)
    runner.run(clip)                                                      # warm-up (packing, allocator)
    t0 = time.perf_counter()
    out = runner.run(clip)
    dt = time.perf_counter() - t0
    line = dict(config=f"C1: {frames}-frame {lr}x{lr} LR synthetic clip, x{S}, {pix_fmt} in and out, streamed clip runner, GPU path",
                precision=precision, windows=frames - 2, frames_per_s=round((frames - 2) / dt, 3), out_shape=list(out.shape),
                h2d_bytes_per_frame=runner.in_bytes, d2h_bytes_per_frame=runner.out_bytes)
    _score_fields(line, runner, score, baseline, temporal, scene, multiscale, decimate)
    if cut_at is not None:
        line.update(cut_at=cut_at)
    if scene is not None:
        line.update(scene=scene, scene_thresholds=list(runner.scene_thresholds), cuts=[int(i) for i in np.flatnonzero(runner.cuts)],
                    scene_m=[round(float(v), 4) for v in runner.scene_m])
    return line, out


def _score_fields(line: dict, runner, score, baseline, temporal, scene, multiscale, decimate) -> None:
    """The fields a scored / watched `ClipRunner` run adds to a result line (what `run_c1_yuv` and `run_file` report alike)."""
    if score is not None:
        line.update(score=score, shave=runner.shave, psnr_db=[round(float(v), 4) for v in runner.metrics["psnr"]],
                    ssim=[round(float(v), 6) for v in runner.metrics["ssim"]])
    if multiscale:
        line.update(msssim=[round(float(v), 6) for v in runner.metrics["msssim"]])
        if baseline is not None:
            line.update(msssim_baseline_mean=round(float(np.mean(runner.metrics["msssim_baseline"])), 6))
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


def run_file(path: str, output: Optional[str] = None, size: Optional[Tuple[int, int]] = None, pix_fmt: Optional[str] = None,
             out_pix_fmt: Optional[str] = None, matrix: str = "bt709", siting: Optional[str] = None, checkpoint: Optional[str] = None,
             scale_down: Optional[int] = None, frames: Optional[int] = None, scale: int = 4, precision: str = "fp32",
             score: Optional[str] = None, decimate: str = "nearest", baseline: Optional[str] = None, temporal: Optional[str] = None,
             scene: Optional[str] = None, scene_thresholds=None, multiscale: bool = False, model=None,
             deinterlace: Optional[str] = None, field_order: Optional[str] = None) -> dict:
    """A clip file streamed through `ClipRunner.run_stream`: `path` a `.y4m` file (size, rate, format, siting and range from its header)
    or a headerless one (`size` = (H, W) and `pix_fmt` required); `output`: the output frames as `out_pix_fmt` (default: the input's),
    with a header when it ends in `.y4m` (S x the LR size, the input's F and A), raw otherwise, or None: the frames are dropped.  The file
    is decimated by `scale_down` (default 1; with `score`: `scale`, the file is the ground truth) and super-resolved by `scale`.  `siting`
    overrides the file's; `checkpoint`: `load_checkpoint` into the seeded model (`model`: use this one instead).  Host memory does not
    depend on the clip's length.  `deinterlace` ("frame" | "field"): the file is interlaced and is made progressive on the device first
    (`ClipRunner(deinterlace=...)`); the field order is the header's (It / Ib) unless `field_order` ("tff" | "bff") names it, which a
    headerless file and a header without a field order need; an interlaced header without `deinterlace` is refused.  The output is
    progressive; with "field" it has twice the input's frame rate.  -> the result line."""
    import time
    from . import VSR
    from .weights import fill_module_
    S = scale
    if field_order not in (None, "tff", "bff"):
        raise ValueError(f"field_order must be None, 'tff' or 'bff', got {field_order!r}")
    if field_order is not None and deinterlace is None:
        raise ValueError("field_order is given but the clip is not deinterlaced (deinterlace=None)")
    if path.endswith(".y4m"):
        src = Y4MReader(path, siting=siting, interlaced=True)
    else:
        if size is None or pix_fmt is None:
            raise ValueError("a headerless clip needs size=(H, W) and pix_fmt")
        src = RawReader(path, size, pix_fmt, siting or "left")
    tff = None
    if deinterlace is None:
        if src.tff is not None:
            src.close()
            raise ValueError(f"{path}: the header says the clip is interlaced (I{'t' if src.tff else 'b'}): pass --deinterlace frame|field "
                             f"(deinterlace=) to make it progressive on the device")
    else:
        tff = src.tff if field_order is None else field_order == "tff"
        if tff is None:
            src.close()
            raise ValueError(f"{path}: nothing says which field comes first (a headerless file, or a header without It / Ib): "
                             f"--deinterlace needs --field-order tff|bff (field_order=)")
    dev = torch.device("cuda", 0)   # (after the refusals above: they need no device)
    torch.cuda.set_device(dev)
    fmt_in, fmt_out = src.fmt, (out_pix_fmt or src.fmt)
    weights = "seeded"
    if model is None:
        model = fill_module_(VSR(upscale_factor=S).eval(), seed=0).to(dev)
        model.precision = model.model.precision = precision
    else:
        weights = "given"
    if checkpoint is not None:
        load_checkpoint(model, checkpoint, map_location=dev)
        weights = checkpoint
    if scale_down is None:
        scale_down = S if score is not None else 1
    runner = ClipRunner(model, src.shape, fmt_in, fmt_out, scale_down=scale_down, matrix=matrix, full_range=src.full_range,
                        siting=src.siting, score=score, decimate=decimate, baseline=baseline, temporal=temporal, scene=scene,
                        scene_thresholds=scene_thresholds, multiscale=multiscale, deinterlace=deinterlace, tff=tff)
    T = len(src) if frames is None else int(frames)
    fps = src.fps or (25, 1)   # (a headerless input has no rate: 25:1, and A0:0 = unknown)
    if deinterlace == "field":   # a frame per field: twice the rate
        fps = (2 * fps[0], fps[1])
    if output is None:
        sink = lambda j, frame: None   # noqa: E731
    elif output.endswith(".y4m"):
        sink = Y4MWriter(output, runner.out_shape, fmt_out, fps, src.siting, src.full_range, src.aspect)
    else:
        sink = RawWriter(output, runner.out_bytes)
    t0 = time.perf_counter()
    try:
        n = runner.run_stream(src, sink, frames=T)
    finally:
        src.close()
        if output is not None:
            sink.close()
    dt = time.perf_counter() - t0
    line = dict(config=f"{T}-frame {src.shape[0]}x{src.shape[1]} clip from a file, /{scale_down} x{S}, streamed clip runner, GPU path",
                input=path, output=output, frames=T, precision=precision, windows=n, frames_per_s=round(n / dt, 3),
                out_shape=[n, runner.out_bytes], out_size=list(runner.out_shape), pix_fmt_in=fmt_in, pix_fmt_out=fmt_out, matrix=matrix,
                siting=src.siting, full_range=bool(src.full_range), weights=weights, fps=list(src.fps) if src.fps else None,
                h2d_bytes_per_frame=runner.in_bytes, d2h_bytes_per_frame=runner.out_bytes)
    _score_fields(line, runner, score, baseline, temporal, scene, multiscale, decimate)
    if deinterlace is not None:
        line.update(deinterlace=deinterlace, tff=bool(tff), frames_out=n)
    if scene is not None:
        line.update(scene=scene, scene_thresholds=list(runner.scene_thresholds), cuts=[int(i) for i in np.flatnonzero(runner.cuts)],
                    scene_m=[round(float(v), 4) for v in runner.scene_m])
    return line


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
        losses.append(train_item(model, optimizer, data, target, high_frames))
        if optimizer.last_grad_norm_sq is not None:
            norms_sq.append(optimizer.last_grad_norm_sq.clone())
    line.update(train_steps=steps, learning_rate=learning_rate, max_grad_norm=max_grad_norm, loss_path=loss_path,
                loss=[round(float(v), 6) for v in torch.stack(losses).cpu()] if losses else [],
                grad_norm=[round(float(v) ** 0.5, 6) for v in torch.stack(norms_sq).cpu()] if norms_sq else None)
    return line, model


def run_file_train(path: str, steps: int, size: Optional[Tuple[int, int]] = None, pix_fmt: Optional[str] = None, matrix: str = "bt709",
                   siting: Optional[str] = None, checkpoint: Optional[str] = None, scale: int = 4, precision: str = "fp32", patch: int = 64,
                   frames_per_sample: int = 3, group: int = 8, seed: int = 0, decimate: str = "nearest",
                   max_grad_norm: Optional[float] = None, learning_rate: float = 1e-3, loss_path: str = "reference",
                   save: Optional[str] = None, model=None, avoid_cuts: bool = False, cut_thresholds=None, act_min: Optional[float] = None,
                   tries: Optional[int] = None):
    """`steps` train steps on patches of a clip file through `ClipTrainer.run_stream`: `path`, `size`, `pix_fmt`, `siting`, `model` as
    `run_file`'s; `checkpoint`: resume (loaded into the model before the first step).  The file is read once, or until `steps` are done.
    `save`: a directory; the trained SR net goes to `<save>/VSR_train-checkpoint.pth.tar` as `checkpoint_state` with the optimizer's
    `state_dict()` under "optimizer_state" and None under "optimizer": tensors and plain containers only, so `load_checkpoint` takes it
    untrusted (the reference pickles the optimizer OBJECT; files written here do not).  `avoid_cuts`, `cut_thresholds`, `act_min`, `tries`:
    `ClipTrainer`'s; when one of them is given the line gains `avoid_cuts`, `cut_thresholds`, `act_min`, `tries`, `cuts` (the source-frame
    indices i whose pair (i, i + 1) was flagged), `samples_skipped` and `act_mean` (the mean `patch_score` of the steps' samples; None
    without `act_min`), and without them it has exactly the keys it had.  -> (result line, model)."""
    from . import VSR, optim
    from .weights import fill_module_
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if path.endswith(".y4m"):
        src = Y4MReader(path, siting=siting)
    else:
        if size is None or pix_fmt is None:
            raise ValueError("a headerless clip needs size=(H, W) and pix_fmt")
        src = RawReader(path, size, pix_fmt, siting or "left")
    weights = "seeded"
    if model is None:
        model = fill_module_(VSR(upscale_factor=scale).eval(), seed=0).to(dev)
        model.precision = model.model.precision = precision
    else:
        weights = "given"
    if checkpoint is not None:
        load_checkpoint(model, checkpoint, map_location=dev)
        weights = checkpoint
    optimizer = optim.Adam(model.parameters(), lr=learning_rate, max_grad_norm=max_grad_norm)
    try:
        trainer = ClipTrainer(model, optimizer, src.shape, src.fmt, patch=patch, frames_per_sample=frames_per_sample, group=group,
                              seed=seed, decimate=decimate, matrix=matrix, full_range=src.full_range, siting=src.siting, loss_path=loss_path,
                              avoid_cuts=avoid_cuts, cut_thresholds=cut_thresholds, act_min=act_min, **({} if tries is None else {"tries": tries}))
        trainer.run_stream(src, max_steps=steps)
    finally:
        src.close()
    written = None
    if save is not None:
        os.makedirs(save, exist_ok=True)
        state = checkpoint_state(model, epoch=1, optimizer=None)
        state["optimizer_state"] = optimizer.state_dict()
        written = save_checkpoint(state, False, save, "VSR", filename="train-checkpoint.pth.tar")
    line = dict(config=f"train steps on {patch}x{patch} LR patches of a {src.shape[0]}x{src.shape[1]} clip from a file, x{scale}, streamed clip "
                       f"trainer, GPU path",
                input=path, frames=trainer.frames_in, pix_fmt_in=src.fmt, precision=precision, weights=weights, train_steps=trainer.steps,
                patch=patch, frames_per_sample=frames_per_sample, group=group, seed=seed, decimate=decimate, loss_path=loss_path,
                learning_rate=learning_rate, max_grad_norm=max_grad_norm, frames_skipped=trainer.frames_skipped,
                loss=[round(float(v), 6) for v in trainer.losses],
                grad_norm=[round(float(v), 6) for v in trainer.grad_norms] if trainer.grad_norms is not None else None, checkpoint=written)
    if avoid_cuts or cut_thresholds is not None or act_min is not None or tries is not None:
        line.update(avoid_cuts=trainer.avoid_cuts, cut_thresholds=list(trainer.cut_thresholds) if trainer.avoid_cuts else None,
                    act_min=trainer.act_min, tries=trainer.tries, cuts=[int(i) for i in trainer.cuts],
                    samples_skipped=trainer.samples_skipped,
                    act_mean=round(float(np.mean(trainer.scores)), 6) if trainer.act_min is not None and len(trainer.scores) else None)
    return line, model


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="config C1: a synthetic clip through the main.py-like plumbing on the GPU path")
    ap.add_argument("--lr", type=int, default=128, help="LR frame size (BASELINE.json C1: 128)")
    ap.add_argument("--frames", type=int, default=3, help="frames of the clip (3 = one window)")
    ap.add_argument("--scale", type=int, default=4, choices=[2, 3, 4], help="4 = the reference's geometry; 2 = C1's label")
    ap.add_argument("--precision", default="fp32", choices=["fp16", "fp32"])
    ap.add_argument("--pix-fmt", default=None, choices=sorted(PIX_FORMATS),
                    help="the clip enters and leaves as Y'CbCr frames of this format through ClipRunner (default: the RGB path); with a "
                         "headerless --input: the file's format")
    ap.add_argument("--input", default=None, metavar="PATH",
                    help="stream this clip through ClipRunner instead of the synthetic one: a .y4m file, or a headerless file with --size and --pix-fmt")
    ap.add_argument("--size", default=None, metavar="HxW", help="with a headerless --input: the frame size")
    ap.add_argument("--output", default=None, metavar="PATH", help="with --input: write the output frames there (.y4m gets a header, anything else is raw)")
    ap.add_argument("--out-pix-fmt", default=None, choices=sorted(PIX_FORMATS), help="with --input: the output format (default: the input's)")
    ap.add_argument("--matrix", default="bt709", choices=["bt601", "bt709", "bt2020"], help="with --input: the Y'CbCr matrix of the file")
    ap.add_argument("--siting", default=None, choices=sorted(YUV_SITINGS), help="with --input: the chroma siting (overrides the file's)")
    ap.add_argument("--checkpoint", default=None, metavar="PATH", help="with --input: load the SR net from this checkpoint (default: the seeded weights)")
    ap.add_argument("--scale-down", type=int, default=None, metavar="N",
                    help="with --input: decimate the file's frames by N before the model (default 1: the file is upscaled by --scale; with "
                         "--score the default is --scale: the file is the ground truth)")
    ap.add_argument("--score", default=None, choices=sorted(METRIC_CHANNELS),
                    help="with --pix-fmt: per-frame PSNR / SSIM of the output against the synthetic HR clip, on RGB or on luma (BT.601 Y)")
    ap.add_argument("--decimate", default="nearest", choices=list(ClipRunner.DECIMATE),
                    help="with --pix-fmt: how the LR frames are made (nearest: the reference's decimation; bicubic: antialiased, stored as 8-bit)")
    ap.add_argument("--multiscale", action="store_true",
                    help="with --score: also the per-frame multi-scale SSIM (five levels; needs 161 pixels each way after the shave)")
    ap.add_argument("--baseline", default=None, choices=["bicubic"],
                    help="with --score: also score the bicubic enlargement of the LR frame; the line carries both means and psnr_gain")
    ap.add_argument("--temporal", default=None, choices=["warp"],
                    help="with --score: also the flow-warped error between consecutive output frames (E_warp); the line carries the clip means")
    ap.add_argument("--scene", default=None, choices=["sad"],
                    help="with --pix-fmt: find scene cuts on the device (mean absolute luma difference of consecutive LR frames) and keep the "
                         "other scene out of the window and of the fed-back estimate; the line carries the cuts found")
    ap.add_argument("--scene-thresholds", type=float, nargs=2, default=None, metavar=("T_ABS", "RATIO"),
                    help="with --scene: a pair is a cut where its mean difference reaches T_ABS (0..255 luma scale) and RATIO times the "
                         "previous pair's (default 15 2; not validated on real video)")
    ap.add_argument("--deinterlace", default=None, choices=["frame", "field"],
                    help="with --input: the file is interlaced; make it progressive on the device before anything else (frame: one frame "
                         "per interlaced frame, its first field kept; field: one per field, twice the rate); not validated on real video")
    ap.add_argument("--field-order", default=None, choices=["tff", "bff"],
                    help="with --deinterlace: which field comes first in time (overrides the .y4m header's It / Ib; required for a "
                         "headerless file)")
    ap.add_argument("--cut-at", type=int, default=None, metavar="K",
                    help="with --pix-fmt: the synthetic clip's frames from K on come from a second seed (a scene cut before frame K)")
    ap.add_argument("--train-steps", type=int, default=None, metavar="K",
                    help="after the no-grad windows: K train steps on the last window (optim.Adam); the line carries the loss per step; "
                         "with --input: K train steps on patches of the file (ClipTrainer), read once or until K steps are done")
    ap.add_argument("--patch", type=int, default=None, metavar="P",
                    help="with --input and --train-steps: the LR patch edge (default 64; the HR patch is --scale times that)")
    ap.add_argument("--frames-per-sample", type=int, default=None, metavar="N",
                    help="with --input and --train-steps: consecutive frames per training sample (default 3: one window)")
    ap.add_argument("--group", type=int, default=None, metavar="G",
                    help="with --input and --train-steps: frames resident on the device at a time (default 8)")
    ap.add_argument("--seed", type=int, default=None, help="with --input and --train-steps: the seed of the patch draws (default 0)")
    ap.add_argument("--save", default=None, metavar="DIR",
                    help="with --input and --train-steps: write DIR/VSR_train-checkpoint.pth.tar (tensors and plain containers only)")
    ap.add_argument("--avoid-cuts", action="store_true", default=None,
                    help="with --input and --train-steps: find scene cuts in every resident group on the device and draw no sample across "
                         "one; the line carries the cuts found")
    ap.add_argument("--cut-thresholds", type=float, nargs=2, default=None, metavar=("T_ABS", "RATIO"),
                    help="with --avoid-cuts: as --scene-thresholds, on the full-size frames (default 15 2; not validated on real video)")
    ap.add_argument("--act-min", type=float, default=None, metavar="X",
                    help="with --input and --train-steps: prefer patches whose mean |dx| + |dy| of the luma code per pixel reaches X (no "
                         "default: any value is the caller's choice and unvalidated)")
    ap.add_argument("--tries", type=int, default=None, metavar="N",
                    help="with --act-min: candidates drawn per sample before the most active one is taken (default 8)")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="with --train-steps: clip the global gradient norm at X on the device; the line carries the norm per step")
    ap.add_argument("--loss-path", default=None, choices=["reference", "fused"],
                    help="with --train-steps: VSR.loss_path (default reference; fused: the loss stays on the device)")
    args = ap.parse_args(argv)
    if args.loss_path is not None and args.train_steps is None:
        ap.error("--loss-path needs --train-steps")
    if args.input is None or args.train_steps is None:
        for name in ("patch", "frames_per_sample", "group", "seed", "save", "avoid_cuts", "cut_thresholds", "act_min", "tries"):
            if getattr(args, name) is not None:
                ap.error(f"--{name.replace('_', '-')} needs --input and --train-steps (the streamed clip trainer)")
    if args.field_order is not None and args.deinterlace is None:
        ap.error("--field-order needs --deinterlace")
    if args.input is None:
        for name in ("size", "output", "out_pix_fmt", "siting", "checkpoint", "scale_down", "deinterlace"):
            if getattr(args, name) is not None:
                ap.error(f"--{name.replace('_', '-')} needs --input")
    else:
        if args.cut_at is not None:
            ap.error("--input takes no --cut-at (the cut is made in the synthetic clip)")
        if args.input.endswith(".y4m") == (args.size is not None or args.pix_fmt is not None):
            ap.error("--input: a .y4m file carries its size and format (no --size / --pix-fmt); a headerless file needs both")
        if args.size is not None:
            try:
                args.size = tuple(int(v) for v in args.size.lower().split("x"))
                assert len(args.size) == 2
            except (ValueError, AssertionError):
                ap.error("--size is HxW, two integers")
        if args.deinterlace is not None and not args.input.endswith(".y4m") and args.field_order is None:
            ap.error("--deinterlace on a headerless file needs --field-order tff|bff")
        if args.train_steps is not None:
            if args.deinterlace is not None:
                ap.error("--input with --train-steps takes no --deinterlace (the streamed clip trainer reads progressive frames)")
            for name in ("output", "out_pix_fmt", "scale_down", "score", "baseline", "temporal", "scene", "scene_thresholds"):
                if getattr(args, name) is not None:
                    ap.error(f"--input with --train-steps trains on the file and writes no frames: it takes no --{name.replace('_', '-')}")
            if args.multiscale:
                ap.error("--input with --train-steps trains on the file and writes no frames: it takes no --multiscale")
            if args.train_steps <= 0:
                ap.error("--input with --train-steps takes a positive count")
            patch, n, group = (64 if args.patch is None else args.patch, 3 if args.frames_per_sample is None else args.frames_per_sample,
                               8 if args.group is None else args.group)
            if patch <= 0:
                ap.error("--patch is a positive LR patch edge")
            if n < 3:
                ap.error("--frames-per-sample is at least 3 (one window)")
            if group < n:
                ap.error("--group must hold a sample: at least --frames-per-sample frames")
            if args.cut_thresholds is not None and not args.avoid_cuts:
                ap.error("--cut-thresholds needs --avoid-cuts")
            if args.tries is not None and args.act_min is None:
                ap.error("--tries needs --act-min")
            if args.tries is not None and args.tries < 1:
                ap.error("--tries is at least 1")
            line, _ = run_file_train(args.input, args.train_steps, size=args.size, pix_fmt=args.pix_fmt, matrix=args.matrix, siting=args.siting,
                                     checkpoint=args.checkpoint, scale=args.scale, precision=args.precision, patch=patch,
                                     frames_per_sample=n, group=group, seed=args.seed or 0, decimate=args.decimate,
                                     max_grad_norm=args.max_grad_norm, loss_path=args.loss_path or "reference", save=args.save,
                                     avoid_cuts=bool(args.avoid_cuts), cut_thresholds=args.cut_thresholds, act_min=args.act_min, tries=args.tries)
            print(json.dumps(line))
            return
        if args.multiscale and args.score is None:
            ap.error("--multiscale needs --score (it is scored beside the estimate)")
        if (args.baseline is not None or args.temporal is not None) and args.score is None:
            ap.error("--baseline and --temporal need --score (they are scored beside the estimate)")
        if args.scene_thresholds is not None and args.scene is None:
            ap.error("--scene-thresholds needs --scene")
        line = run_file(args.input, args.output, size=args.size, pix_fmt=args.pix_fmt, out_pix_fmt=args.out_pix_fmt, matrix=args.matrix,
                        siting=args.siting, checkpoint=args.checkpoint, scale_down=args.scale_down, frames=None, scale=args.scale,
                        precision=args.precision, score=args.score, decimate=args.decimate, baseline=args.baseline, temporal=args.temporal,
                        scene=args.scene, scene_thresholds=args.scene_thresholds, multiscale=args.multiscale,
                        deinterlace=args.deinterlace, field_order=args.field_order)
        print(json.dumps(line))
        return
    if args.score is not None and args.pix_fmt is None:
        ap.error("--score needs --pix-fmt (the streamed clip runner scores its frames)")
    if args.decimate != "nearest" and args.pix_fmt is None:
        ap.error("--decimate needs --pix-fmt (the streamed clip runner makes the LR frames)")
    if args.multiscale and args.score is None:
        ap.error("--multiscale needs --score (it is scored beside the estimate)")
    if args.baseline is not None and args.score is None:
        ap.error("--baseline needs --score (it is scored beside the estimate)")
    if args.temporal is not None and args.score is None:
        ap.error("--temporal needs --score (it is scored beside the estimate)")
    if args.scene is not None and args.pix_fmt is None:
        ap.error("--scene needs --pix-fmt (the streamed clip runner watches its frames)")
    if args.scene_thresholds is not None and args.scene is None:
        ap.error("--scene-thresholds needs --scene")
    if args.cut_at is not None and (args.pix_fmt is None or not 0 < args.cut_at < args.frames):
        ap.error("--cut-at needs --pix-fmt and a frame index inside the clip (0 < K < --frames)")
    if args.max_grad_norm is not None and args.train_steps is None:
        ap.error("--max-grad-norm needs --train-steps")
    if args.train_steps is not None:
        if args.pix_fmt is not None or args.train_steps < 0:
            ap.error("--train-steps takes a non-negative count and runs on the RGB path (no --pix-fmt)")
        line, _ = run_c1_train(args.train_steps, args.lr, args.frames, args.scale, args.precision, args.max_grad_norm,
                               loss_path=args.loss_path or "reference")
    elif args.pix_fmt is not None:
        line, _ = run_c1_yuv(args.pix_fmt, args.lr, args.frames, args.scale, args.precision, args.score, args.decimate, args.baseline,
                             args.temporal, args.scene, args.scene_thresholds, args.cut_at, args.multiscale)
    else:
        line, _, _, _ = run_c1(args.lr, args.frames, args.scale, args.precision)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
