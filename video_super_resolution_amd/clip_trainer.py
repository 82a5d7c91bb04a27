"""`ClipTrainer`: train steps on patches of a real clip.  Frames of planar Y'CbCr (any name of `frames.PIX_FORMATS`) are streamed to the
device group by group, converted at full size, and every training sample is cut from the resident group and augmented there
(`frames.patch_table` / `patch_gather` / `patch_item`, include/vsr_hip_patch.h); each sample is one `driver.train_item`.  `driver` imports
`ClipTrainer`, so `driver.ClipTrainer` resolves like `driver.ClipRunner`.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .clip_runner import ArraySource
from .frames import (FrameResizer, _scene_thresholds, cell_cuts, cell_stats, patch_gather, patch_item, patch_table, patch_table_select,
                     pix_coefficients, pix_frame_bytes, pix_ingest)


class ClipTrainer:
    """Train steps of `model` under `optimizer` (optim.Adam, or any torch optimizer) on a clip of `shape` = (H, W) frames in `fmt_in`.
    `patch` is the LR patch edge: the HR patch is S * patch each way, S the model's scale (FlowNet2 needs an LR edge of at least 64).  A
    sample is `frames_per_sample` = n consecutive frames, that is n - 2 overlapping windows; `group` frames are resident at a time and
    `samples_per_group` samples are drawn from each group.

    `run_stream(source, frames=None, max_steps=None) -> steps`: `source.read_into(buf) -> bool` as `ClipRunner`'s (a `y4m.Y4MReader`, an
    `ArraySource`); `run(array)` is the array form.  Per source frame: one upload from one of two pinned slots, then `pix_ingest` at full
    size into row g of a [group,H,W,3] buffer; with `decimate="bicubic"` also `FrameResizer(quantise=True)` of that frame into row g of a
    [group,H/S,W/S,3] buffer (the antialiased LR frame as an 8-bit file would hold it; H and W must then be multiples of S).  When a
    group is full: one `patch_table` drawn from `self.rng` (`np.random.RandomState(seed)`), one `patch_gather` for all its samples, and per
    sample `patch_item` and `driver.train_item` (the gradients zeroed, the sample's windows without gradient, the train step on the last
    window with the windows' mean loss).  With `decimate="nearest"` the LR patch is the decimation of the AUGMENTED HR patch: the pixel
    phase the model sees at inference (include/vsr_hip_patch.h).  Groups do not overlap; the clip's last group may be short, and one
    shorter than a sample is dropped and counted in `frames_skipped`.  `max_steps`: stop reading when that many steps are done.

    Everything runs on the current stream: a group's upload is milliseconds against seconds of training, so there is no copy stream and
    no overlap machinery here.  The loop adds no host wait of its own but the one that frees a pinned slot (the event of the upload two
    frames back, long complete); with `loss_path="fused"` the losses stay on the device and come back, with the gradient norms, in one
    copy when the run ends.  (`loss_path=None` leaves `model.loss_path` as it is; "reference" forms every loss on the host, as the
    reference does.)

    After a run: `steps`, `losses` (float64 [steps]), `grad_norms` (float64 [steps] when the optimizer clips, else None), `tables` (every
    table drawn, in order), `frames_in`, `frames_skipped`, `h2d_bytes`.

    Where the samples are cut (both off by default: then no launch, copy or wait is added, `patch_table` is called as before and tables,
    losses and weights are bit for bit what they were):
        avoid_cuts=True   no sample spans a scene cut.  `cut_thresholds`: (t_abs, ratio), default `frames.SCENE_THRESHOLDS`, applied here
                          to FULL-SIZE frames where `ClipRunner` applies it to LR frames; the measure is a mean per pixel, so the scale is
                          the same.  The rule and its defaults are NOT validated on real video.  A group's first pair has no pair before
                          it (`frames.cell_cuts`), and the pair between two groups is not scored: samples never span groups.
        act_min=X         patches with detail are preferred: up to `tries` candidates are drawn per sample, the first whose
                          `frames.patch_score` (mean |dx| + |dy| of the 8-bit luma code per pixel) reaches X is taken, else the most
                          active one.  There is no default: any value is the caller's choice and unvalidated (`driver.synthetic_video`
                          has 3.4 to 10.7 per cell; a constant region has 0).
    With either, per full group: one `frames.cell_stats` over the resident frames (one launch, every frame read once), one device-to-host
    copy of the small map and its wait (2 MB for eight 2160 x 3840 frames, against seconds of training), then `frames.cell_cuts` and
    `frames.patch_table_select` on the host.  A group in which no run of n frames is free of cuts trains nothing; its samples are counted
    in `samples_skipped`.  `cut_thresholds` without `avoid_cuts`, a `tries` other than the default without `act_min` and `tries` < 1
    are refused.  After a run also: `cuts` (the source-frame indices i whose pair (i, i + 1) was flagged), `cut_m` (float64, the mean
    absolute luma difference of those pairs), `scores` (float64 [steps], NaN without `act_min`), `tried` (int32 [steps]) and
    `samples_skipped`.

    Known limit: a cut is looked for between frames of one group only, and only by the mean absolute luma difference: a dissolve or a
    fade is not a cut to this rule, and a sample may run through one."""

    DECIMATE = ("nearest", "bicubic")
    TRIES = 8

    def __init__(self, model, optimizer, shape: Tuple[int, int], fmt_in: str, patch: int = 64, frames_per_sample: int = 3, group: int = 8,
                 samples_per_group: int = 4, seed: int = 0, augment: bool = True, decimate: str = "nearest", matrix: str = "bt709",
                 full_range: bool = False, siting: str = "left", loss_path: Optional[str] = None, avoid_cuts: bool = False, cut_thresholds=None,
                 act_min: Optional[float] = None, tries: int = 8):
        H, W = int(shape[0]), int(shape[1])
        S = int(model.model.upscale_factor)
        self.model, self.optimizer, self.shape, self.fmt_in, self.siting, self.S = model, optimizer, (H, W), fmt_in, siting, S
        self.patch, self.hr_patch = int(patch), S * int(patch)
        self.n, self.group, self.samples_per_group = int(frames_per_sample), int(group), int(samples_per_group)
        if decimate not in self.DECIMATE:
            raise ValueError(f"decimate must be 'nearest' or 'bicubic', got {decimate!r}")
        if self.patch <= 0 or self.hr_patch > min(H, W):
            raise ValueError(f"the frames of {H} x {W} are smaller than the HR patch of {self.hr_patch} x {self.hr_patch} (x{S} of the LR "
                             f"patch {self.patch})")
        if self.n < 3:
            raise ValueError(f"frames_per_sample must be at least 3 (one window), got {self.n}")
        if self.group < self.n:
            raise ValueError(f"group = {self.group} frames cannot hold a sample of frames_per_sample = {self.n}")
        if self.samples_per_group <= 0:
            raise ValueError(f"samples_per_group must be positive, got {self.samples_per_group}")
        if decimate == "bicubic" and (H % S or W % S):
            raise ValueError(f"decimate='bicubic' needs frames that are a multiple of S = {S}, got {H} x {W}")
        if cut_thresholds is not None and not avoid_cuts:
            raise ValueError("cut_thresholds is given but cuts are not avoided (avoid_cuts=False)")
        if int(tries) < 1:
            raise ValueError(f"tries must be at least 1, got {tries}")
        if int(tries) != self.TRIES and act_min is None:
            raise ValueError(f"tries = {tries} is given but no activity bar is set (act_min=None)")
        if act_min is not None and (not np.isfinite(act_min) or self.hr_patch < 31):
            raise ValueError(f"act_min must be finite, and the HR patch of {self.hr_patch} at least 31 (one whole cell inside any crop)")
        self.avoid_cuts, self.cut_thresholds = bool(avoid_cuts), (_scene_thresholds(cut_thresholds) if avoid_cuts else None)
        self.act_min, self.tries = (None if act_min is None else float(act_min)), int(tries)
        if loss_path is not None:
            model.loss_path = loss_path
        self.decimate, self.augment, self.seed = decimate, bool(augment), int(seed)
        self.rng = np.random.RandomState(self.seed)
        self.in_bytes = pix_frame_bytes(fmt_in, H, W)
        self.coef_in = pix_coefficients(fmt_in, matrix, full_range, inverse=True)
        self.device = dev = next(model.parameters()).device
        self._pin_in = [torch.empty(self.in_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._dev_in = [torch.empty(self.in_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._frames = torch.empty((self.group, H, W, 3), dtype=torch.float32, device=dev)
        self._frames_lr = self._down = None
        if decimate == "bicubic":
            self._frames_lr = torch.empty((self.group, H // S, W // S, 3), dtype=torch.float32, device=dev)
            self._down = FrameResizer(self.shape, (H // S, W // S), "bicubic", dev)
        self.gather_events = None   # a list: (start, end) timed events around every `patch_gather` (tools/patch_time.py)
        self._reset()

    def _reset(self) -> None:
        self.steps = self.frames_in = self.frames_skipped = self.h2d_bytes = 0
        self.losses = self.grad_norms = None
        self.tables = []
        self.samples_skipped = 0
        self.cuts, self.cut_m, self.scores, self.tried = [], [], [], []

    def run(self, frames: np.ndarray, max_steps: Optional[int] = None) -> int:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != self.in_bytes:
            raise ValueError(f"expected uint8 [T, {self.in_bytes}], got {frames.dtype} {frames.shape}")
        return self.run_stream(ArraySource(frames), max_steps=max_steps)

    def run_stream(self, source, frames: Optional[int] = None, max_steps: Optional[int] = None) -> int:
        """`source` group by group (the class docstring); returns the number of train steps taken."""
        T = len(source) if frames is None else int(frames)
        self._reset()
        losses, norms_sq, uploaded = [], [], [None, None]
        done = lambda: max_steps is not None and self.steps >= max_steps   # noqa: E731
        self.model.train()
        with torch.cuda.device(self.device):
            g = 0
            for i in range(T):
                if done():
                    break
                self._upload(i, g, source, uploaded, T)
                g += 1
                if g == self.group:
                    self._train_group(g, losses, norms_sq, max_steps)
                    g = 0
            if g >= self.n and not done():
                self._train_group(g, losses, norms_sq, max_steps)
            elif not done():
                self.frames_skipped += g
            # the one copy of the run: the losses, and the squared gradient norms where the optimizer clips
            dev = [torch.as_tensor(v, dtype=torch.float64, device=self.device).reshape(()) for v in losses + norms_sq]
            host = torch.stack(dev).cpu().numpy() if dev else np.zeros(0)
            self.losses = host[:len(losses)]
            self.grad_norms = np.sqrt(host[len(losses):]) if norms_sq else None
        self.cut_m, self.scores = np.asarray(self.cut_m, dtype=np.float64), np.asarray(self.scores, dtype=np.float64)
        self.tried = np.asarray(self.tried, dtype=np.int32)
        return self.steps

    def _upload(self, i: int, g: int, source, uploaded, T: int) -> None:
        """Source frame `i` into row `g` of the group: pinned slot i % 2, the device slot, the conversion at full size (and its reduction)."""
        a = i % 2
        if uploaded[a] is not None:
            uploaded[a].synchronize()   # the pinned slot is free again (host wait on one event)
        if not source.read_into(self._pin_in[a].numpy()):
            raise ValueError(f"the source ended before frame {i} of the {T} asked for")
        self._dev_in[a].copy_(self._pin_in[a], non_blocking=True)
        uploaded[a] = torch.cuda.Event()
        uploaded[a].record()
        self.h2d_bytes += self.in_bytes
        self.frames_in += 1
        pix_ingest(self._dev_in[a], self.shape, self.fmt_in, self.coef_in, self.siting, lr_out=self._frames[g])
        if self._down is not None:
            self._down(self._frames[g], quantise=True, out=self._frames_lr[g])

    def _train_group(self, G: int, losses, norms_sq, max_steps) -> None:
        """The samples of a group of `G` resident frames: one table, one gather, a `train_item` per sample."""
        from .driver import train_item
        scores = tried = None
        if self.avoid_cuts or self.act_min is not None:
            table, scores, tried = self._select(G)
        else:
            table = patch_table(self.rng, self.samples_per_group, G, self.n, self.shape, self.hr_patch, self.S, self.augment)
        self.tables.append(table)
        if table.shape[0] == 0:
            self.samples_skipped += self.samples_per_group
            return
        if self.gather_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        hr, lr = patch_gather(self._frames[:G], table, self.n, self.hr_patch, self.S,
                              None if self._frames_lr is None else self._frames_lr[:G])
        if self.gather_events is not None:
            ev[1].record()
            self.gather_events.append(ev)
        for b in range(table.shape[0]):
            if max_steps is not None and self.steps >= max_steps:
                break
            data, target, high_frames = patch_item(hr, lr, b)
            losses.append(train_item(self.model, self.optimizer, data, target, high_frames))
            norm_sq = getattr(self.optimizer, "last_grad_norm_sq", None)
            if norm_sq is not None:
                norms_sq.append(norm_sq.clone())
            self.steps += 1
            if scores is not None:
                self.scores.append(scores[b])
                self.tried.append(tried[b])

    def _select(self, G: int):
        """The table of a group of `G` resident frames under `avoid_cuts` / `act_min`: the map, its one copy to the host, the two host steps."""
        stats = cell_stats(self._frames[:G]).cpu().numpy()   # the one copy and its wait
        cuts = None
        if self.avoid_cuts:
            cuts, m = cell_cuts(stats, self.shape, self.cut_thresholds)
            first = self.frames_in - G   # the source index of the group's first frame
            self.cuts.extend(first + int(p) for p in np.flatnonzero(cuts))
            self.cut_m.extend(float(v) for v in m[cuts])
        return patch_table_select(self.rng, self.samples_per_group, G, self.n, self.shape, self.hr_patch, self.S, self.augment, cuts=cuts,
                                  stats=stats if self.act_min is not None else None, act_min=self.act_min, tries=self.tries)
