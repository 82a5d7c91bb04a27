"""`ClipRunner`: a clip of planar Y'CbCr frames (any name of `frames.PIX_FORMATS`: 4:2:0, 4:2:2, 4:4:4) streamed through the model on top of
`frames`: every source frame read straight into pinned memory and uploaded once on a copy stream, converted once into a three-slot LR
ring, the window formed on the device, the HR frame written out in the output format, copied back on a second copy stream and handed
to a sink from its pinned slot: no host array of the clip's length exists on either side (`run_stream`; `run` is the array form).  What a run scores (`score=`, `baseline=`, `temporal=`) is a list of series, each a range of rows of one
float64 tensor of sums (`sums_layout`); with `multiscale=True` the frames' multi-scale SSIM sums go into a tensor of their own; with
`scene="sad"` scene cuts are found and the window composed under them on the device, in
tensors of their own; with `deinterlace="frame" | "field"` the frames of an interlaced clip are made progressive on the device before
anything else sees them; `driver` imports `ClipRunner`, so `driver.ClipRunner` resolves as before.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .frames import (DEINTERLACE, METRIC_CHANNELS, MSSSIM_BETA, MSSSIM_MIN_SIZE, FrameResizer, _scene_thresholds, deint_planes,
                     deint_schedule, deinterlace, ewarp, frame_metrics, frame_msssim,
                     msssim, pix_coefficients, pix_frame_bytes, pix_ingest, pix_write, psnr_ssim, scene_flags, scene_sums, scene_window,
                     truth_flows, warp_error)

# series of `sums_layout` -> the keys of `ClipRunner.metrics` its host step (`psnr_ssim` for a frame series, `ewarp` for a pair series)
# fills; the occlusion mask depends on the flows alone, so the estimate's pairs give the one `valid_share`
METRIC_KEYS = {"estimate": ("psnr", "ssim"), "baseline": ("psnr_baseline", "ssim_baseline"), "ewarp": ("ewarp", "valid_share"),
               "ewarp_truth": ("ewarp_truth", None), "ewarp_baseline": ("ewarp_baseline", None)}


def sums_layout(T: int, score: Optional[str], baseline: Optional[str] = None,
                temporal: Optional[str] = None) -> Optional[Dict[str, Tuple[int, int, str]]]:
    """What a scored run of `T` source frames sums up, as rows of ONE [rows,4] float64 tensor: series name -> (row0, rows, kind), in
    row order.  A "frame" series has a row per output frame (T - 2: `frame_metrics`' sums), a "pair" series a row per pair of consecutive
    output frames (T - 3, none for T = 3: `warp_error`'s sums).  `estimate` always; `baseline` with a baseline; `ewarp` (the estimate's
    pairs) and `ewarp_truth` with `temporal`, `ewarp_baseline` with both.  None when nothing is scored (`score` is None)."""
    if score is None:
        return None
    series = [("estimate", "frame")]
    if baseline is not None:
        series.append(("baseline", "frame"))
    if temporal is not None:
        series += [("ewarp", "pair"), ("ewarp_truth", "pair")]
        if baseline is not None:
            series.append(("ewarp_baseline", "pair"))
    layout, row0 = {}, 0
    for name, kind in series:
        rows = T - 2 if kind == "frame" else T - 3
        layout[name] = (row0, rows, kind)
        row0 += rows
    return layout


class ArraySource:
    """A host array [T, frame_bytes] as a frame source: `read_into(buf)` copies the next row, False after the last (`len`: the rows)."""

    def __init__(self, frames: np.ndarray):
        self.frames, self._i = frames, 0

    def __len__(self) -> int:
        return self.frames.shape[0]

    def read_into(self, buf: np.ndarray) -> bool:
        if self._i >= self.frames.shape[0]:
            return False
        buf[:] = self.frames[self._i]
        self._i += 1
        return True


class ClipRunner:
    """A clip streamed through `model` frame by frame.  `shape` = (H, W) of the source frames in `fmt_in`; the model sees them
    decimated by `scale_down` (1: as they are) and returns frames of (S * (H // scale_down), S * (W // scale_down)), written out as
    `fmt_out`; both formats are names of `frames.PIX_FORMATS`, and an output shape `fmt_out` cannot hold (an odd width for 4:2:2, an odd
    size for 4:2:0) is refused here.  `run_stream(source, sink, frames=T)`: `source.read_into(buf) -> bool` fills a uint8 array of
    `in_bytes` elements with the next frame (a `y4m.Y4MReader`, an `ArraySource`); the runner hands it the pinned upload slot itself, so
    a frame goes from the file to pinned memory in one read.  `sink(j, frame)` is called once per output frame j = 0 .. T-3, in order,
    with a uint8 view of the pinned output slot that is valid during the call only (a `y4m.Y4MWriter`).  `frames`: how many source frames
    to take, default `len(source)`; the sums of a scored run are sized by it, nothing else is.  `run(frames)`: host array
    [T, frame_bytes] -> host array [T-2, out_frame_bytes] (one frame per 3-frame window): `run_stream` over an `ArraySource` with a
    collecting sink.

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
    `matrix` the frames are coded with) into row j of its series in the run's one tensor of sums (`sums_layout`); nothing
    extra is uploaded, and one copy at the end gives `metrics = {"psnr": [T-2], "ssim": [T-2]}`.

    `decimate="nearest"` (default): the LR frame is the conversion's own nearest-neighbour decimation (the reference's `interpolate` at
    main.py:157).  `decimate="bicubic"`: every uploaded frame is converted at full size into a reused HR buffer of its own (not the one the
    scored window's truth lives in) and reduced into its ring slot by `FrameResizer(quantise=True)`: the antialiased bicubic LR frame as an
    8-bit file would hold it, the evaluation protocol of the literature.  `baseline="bicubic"` (needs `score`): per window the middle LR
    frame of the ring is enlarged to the output shape into a reused buffer and scored against the same truth with the same quantise,
    shave and channels as the estimate, into a second series of T - 2 rows of the same tensor: `metrics` gains `psnr_baseline` and
    `ssim_baseline`.  Neither uploads or downloads a byte more; with both at their defaults the launches are the ones described above.

    `temporal="warp"` (needs `score`): the temporal warping error of the output (`warp_error`, Lai et al. 2018).  For every output frame
    j >= 1 the pair (j - 1, j) is scored along the flows between the source frames j and j + 1 (`truth_flows`, both directions in one
    FlowNet2 batch, in the model's precision): the previous estimate and the previous truth frame are kept (`_truth` is then two
    alternating buffers), and the pair of truth frames is scored along the same flows: the floor any method sits above.  With
    `baseline="bicubic"` the baseline pair is scored too (`_base` is then two alternating buffers).  Same channels, quantise and shave
    (counted inside the flow's centre crop) as the per-frame scores, `occ` as `warp_error`'s (default: the published constants), into series of
    T - 3 rows each that travel in the one copy at the end:
    `metrics` gains `ewarp`, `ewarp_truth`, `valid_share` (the occlusion mask depends on the flows alone: one share for all) and, with a
    baseline, `ewarp_baseline`, each [T-3] (empty for T = 3).  No upload, download or host wait is added; with `temporal=None` the
    launches are the ones described above.

    `multiscale=True` (needs `score`, and 161 pixels each way after the shave): multi-scale SSIM of every output frame (`frame_msssim`,
    Wang et al. 2003), one more scoring call per window on the buffers the per-frame scores already hold, with the same channels,
    quantise and shave, into row j of a [T-2,P,5,2] float64 tensor of its own; with `baseline="bicubic"` the baseline frame gets one too,
    into a second such tensor (both are views of one buffer).  One small copy at the end brings them back: `metrics` gains `msssim` and,
    with a baseline, `msssim_baseline`, each [T-2] (`msssim`, the host step).  `sums_layout` and the [rows,4] tensor are untouched; no
    upload, download or host wait is added; with `multiscale=False` the launches are the ones described above.

    `scene="sad"`: scene cuts found and handled on the device (include/vsr_hip_scene.h).  After source frame i >= 1 has been converted
    into its ring slot, `scene_sums` of the ring's frames i - 1 and i goes into row i - 1 of a [T-1,2] float64 tensor and `scene_flags`
    of that row, with the row above as the pair before, into element i - 1 of a [T-1] int32 tensor.  The window of frames i - 2 .. i
    = (a, b, c) is then `scene_window`'s under the flags of the pairs (a, b) and (b, c): a cut between a and b gives (b, b, c) and
    restarts the recurrence from b, a cut between b and c gives (a, b, b): for a clip A ++ B with one cut the outputs are those of a run
    over A ++ [A[-1]] followed by those of a fresh run over [B[0]] ++ B.  The host never reads a flag: no host wait is added, no byte
    more is uploaded, and the two small tensors (views of one buffer) come back in one copy at the end of `run()`: `cuts` (bool [T-1],
    entry i - 1 is the pair (i - 1, i)) and `scene_m` (float64 [T-1], the mean absolute luma difference).  `scene_thresholds`:
    (t_abs, ratio), default `frames.SCENE_THRESHOLDS`: this project's choice, not validated on real video.  With `temporal="warp"` the
    rows of `ewarp`, `ewarp_truth` and `ewarp_baseline` whose flows cross a cut (row r where `cuts[r + 1]`) are NaN: a warping error
    across a cut measures nothing; `valid_share` stays as computed.  With `scene=None` the launches are the ones described above and
    `cuts` and `scene_m` are None.

    `deinterlace="frame" | "field"` (`tff`: the top field is the first in time, default True): the source frames are interlaced and are
    made progressive on the device by the rule of include/vsr_hip_deint.h before the conversion.  Every uploaded frame goes into a ring of
    three raw device buffers; progressive frame k is produced into the two buffers the conversion reads (what an uploaded frame is
    without this option) once its later neighbour i = k + 1 has arrived, the last one at the end of the source, with the neighbours and
    parities of `frames.deint_schedule` (reflection at both ends).  "frame" keeps the first field in time of every frame: T' = T
    progressive frames; "field" rebuilds a frame around each field: T' = 2 T, at twice the rate.  From there everything above holds with
    "source frame" read as "progressive frame": the windows, `scene`, `score` (the truth of output frame j is the DEINTERLACED frame
    j + 1, not a progressive original, which the runner never sees), `baseline`, `temporal`, `multiscale`, `sums_layout(T')`;
    `run_stream` gives T' - 2 outputs and returns that number, `run` takes T >= 3 ("frame") or T >= 2 ("field") frames: the output equals
    `ClipRunner(...).run(frames.deinterlace_clip(frames, shape, fmt_in, mode, tff))` byte for byte.  One launch per progressive frame on
    the current stream; no upload, download or host wait is added (`h2d_bytes` stays T * in_bytes, `frames_in` T), an event orders every
    reuse of a raw slot by the upload stream against the launches that read it.  Interlaced 4:2:0 chroma is deinterlaced per plane and
    then read with the progressive siting: the field-dependent vertical chroma siting is ignored.  The rule is not validated on real
    video.  `tff` without `deinterlace`, and a layout with a plane of fewer than 2 rows, are refused.  With `deinterlace=None` the
    launches are the ones described above."""

    DECIMATE = ("nearest", "bicubic")
    BASELINE = (None, "bicubic")
    TEMPORAL = (None, "warp")
    SCENE = (None, "sad")
    DEINTERLACE = DEINTERLACE

    def __init__(self, model, shape: Tuple[int, int], fmt_in: str, fmt_out: str, scale_down: int = 1, overlap: bool = True,
                 matrix: str = "bt709", full_range: bool = False, siting: str = "left", score: Optional[str] = None,
                 shave: Optional[int] = None, decimate: str = "nearest", baseline: Optional[str] = None, temporal: Optional[str] = None,
                 occ=None, scene: Optional[str] = None, scene_thresholds=None, multiscale: bool = False,
                 deinterlace: Optional[str] = None, tff: Optional[bool] = None):
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
        if scene not in self.SCENE:
            raise ValueError(f"scene must be None or 'sad', got {scene!r}")
        if scene_thresholds is not None and scene is None:
            raise ValueError("scene_thresholds is given but no scene detection is asked for (scene=None)")
        if deinterlace not in self.DEINTERLACE:
            raise ValueError(f"deinterlace must be None, 'frame' or 'field', got {deinterlace!r}")
        if tff is not None and deinterlace is None:
            raise ValueError("tff is given but the frames are not deinterlaced (deinterlace=None)")
        self.deinterlace, self.tff = deinterlace, (None if deinterlace is None else True if tff is None else bool(tff))
        self.decimate, self.baseline, self.temporal, self.occ = decimate, baseline, temporal, occ
        self.scene, self.scene_thresholds = scene, (_scene_thresholds(scene_thresholds) if scene is not None else None)
        self.cuts = self.scene_m = None   # of the last run(): bool [T-1], float64 [T-1] with scene="sad"
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
        self.multiscale = bool(multiscale)
        if self.multiscale and score is None:
            raise ValueError("multiscale=True is scored beside the estimate: it needs score='rgb' or 'y'")
        if self.multiscale and min(self.shape) - 2 * self.shave < MSSSIM_MIN_SIZE:
            raise ValueError(f"multiscale=True needs {MSSSIM_MIN_SIZE} pixels each way after the shave: shave {self.shave} leaves "
                             f"{min(self.shape) - 2 * self.shave} of {self.shape}")
        self.metrics = None   # of the last run(): {"psnr": [T-2], "ssim": [T-2]} when scoring
        self.in_bytes = pix_frame_bytes(fmt_in, H, W)
        try:
            self.out_bytes = pix_frame_bytes(fmt_out, *self.out_shape)
        except ValueError as e:
            raise ValueError(f"the output frames of {self.out_shape[0]} x {self.out_shape[1]} do not fit {fmt_out}: {e}") from None
        self.coef_in = pix_coefficients(fmt_in, matrix, full_range, inverse=True)
        self.coef_out = pix_coefficients(fmt_out, matrix, full_range)
        self.device = next(model.parameters()).device
        dev = self.device
        self._pin_in = [torch.empty(self.in_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._pin_out = [torch.empty(self.out_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._dev_in = [torch.empty(self.in_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._dev_out = [torch.empty(self.out_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._raw = None
        if deinterlace is not None:   # the interlaced frames as uploaded: frame i in slot i % 3, its neighbours in the other two
            rows = min(p[1] for p in deint_planes(fmt_in, H, W)[0])
            if rows < 2:
                raise ValueError(f"deinterlace={deinterlace!r}: {fmt_in} {H}x{W} has a plane of {rows} row(s), which holds no two fields")
            self._raw = [torch.empty(self.in_bytes, dtype=torch.uint8, device=dev) for _ in range(3)]
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

    @staticmethod
    def _slot(buf, j: int):
        """Buffer of window `j`: `_truth` and `_base` are one tensor, or two alternating ones when the previous window's is kept."""
        return buf[j % 2] if isinstance(buf, list) else buf

    def run(self, frames: np.ndarray) -> np.ndarray:
        frames = np.asarray(frames)
        least = 2 if self.deinterlace == "field" else 3
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != self.in_bytes or frames.shape[0] < least:
            raise ValueError(f"expected uint8 [T >= {least}, {self.in_bytes}], got {frames.dtype} {frames.shape}")
        out = np.empty((self.progressive_frames(frames.shape[0]) - 2, self.out_bytes), dtype=np.uint8)

        def collect(j, frame):
            out[j] = frame

        self.run_stream(ArraySource(frames), collect)
        return out

    def progressive_frames(self, T: int) -> int:
        """T': the frames the windows are formed over for `T` source frames (2 T with deinterlace="field", else T)."""
        return 2 * T if self.deinterlace == "field" else T

    def run_stream(self, source, sink, frames: Optional[int] = None) -> int:
        """`source` -> `sink`, frame by frame (the class docstring); returns the number of output frames, T' - 2 (T' = T without
        `deinterlace`)."""
        T = len(source) if frames is None else int(frames)
        Tp = self.progressive_frames(T)
        if Tp < 3:
            raise ValueError(f"a run needs at least 3 {'progressive' if self.deinterlace else 'source'} frames (one window), got {Tp}")
        self.h2d_bytes = self.d2h_bytes = self.frames_in = self.frames_out = 0
        self.metrics = self.cuts = self.scene_m = None
        with torch.cuda.device(self.device), torch.no_grad():
            st = self._begin(Tp)
            st.sink, st.T = sink, T
            if self.deinterlace is None:
                for i in range(T):
                    self._upload(st, i, source)
                    self._window(st, i)
            else:
                self._run_interlaced(st, T, source)
            self._drain(st)
            if st.scene_buf is not None:
                self._collect_scene(st, Tp)
            if st.layout is not None:
                self.metrics = self._collect(st)
        return Tp - 2

    def _window(self, st, i: int) -> None:
        """Once frame `i` >= 2 is in the ring: the window of frames i - 2 .. i, its scores and its output frame i - 2."""
        if i < 2:
            return
        self._forward(st, i)
        if st.layout is not None:
            self._score(st, i - 2)
        self._write_out(st, i - 2)

    def _run_interlaced(self, st, T: int, source) -> None:
        """`deinterlace`: raw frame i uploaded into slot i % 3 of the raw ring; the entries of `deint_schedule` whose three frames have
        arrived (those of frame k when frame k + 1 is in; the last frame's with the last frame itself, the end of the source: its later
        neighbour is the earlier one) produced into `_dev_in[q % 2]` on the current stream, progressive frame q then converted and its
        window run as an uploaded frame's is."""
        sched = deint_schedule(T, self.deinterlace, self.tff)
        q = 0
        for i in range(T):
            self._fetch(st, i, source, self._raw[i % 3], st.deinterlaced)
            while q < len(sched) and max(sched[q][:3]) <= i:
                p, c, n, keep, kept_first = sched[q]
                # (`_dev_in[q % 2]` was last read by progressive frame q - 2's conversion and by the truth of window q - 3, on this stream)
                deinterlace(self._raw[p % 3], self._raw[c % 3], self._raw[n % 3], self.shape, self.fmt_in, keep, kept_first, out=self._dev_in[q % 2])
                st.deinterlaced = torch.cuda.Event()   # the raw slots are free once this launch has read them
                st.deinterlaced.record(st.main)
                self._convert(st, q)
                self._window(st, q)
                q += 1

    def _begin(self, T: int):
        """The state of one run: the sink, the one tensor of sums, the streams and the events that order every reuse of a slot."""
        layout = sums_layout(T, self.score, self.baseline, self.temporal)
        rows = sum(n for _, n, _ in layout.values()) if layout is not None else 0
        main = torch.cuda.current_stream(self.device)
        s_in, s_out = (self._s_in, self._s_out) if self.overlap else (main, main)
        # scene="sad": the sums [T-1,2] float64 and the flags [T-1] int32, views of one buffer so that one copy brings both back
        scene_buf = scene_rows = scene_flag = None
        if self.scene is not None:
            scene_buf = torch.empty(20 * (T - 1), dtype=torch.uint8, device=self.device)
            scene_rows = scene_buf[:16 * (T - 1)].view(torch.float64).view(T - 1, 2)
            scene_flag = scene_buf[16 * (T - 1):].view(torch.int32)
        # multiscale: the sums [series, T-2, P, 5, 2] float64 of `frame_msssim`, series 0 the estimate's and 1 the baseline's
        ms = None
        if self.multiscale:
            ms = torch.empty((2 if self.baseline is not None else 1, T - 2, 3 if self.score == "rgb" else 1, len(MSSSIM_BETA), 2),
                             dtype=torch.float64, device=self.device)
        return SimpleNamespace(
            ms=ms, scene_buf=scene_buf, scene_sums=scene_rows, scene_flags=scene_flag,
            sink=None, layout=layout,
            sums=None if layout is None else torch.empty((rows, 4), dtype=torch.float64, device=self.device),
            main=main, s_in=s_in, s_out=s_out, est=None, prev_est=None,
            deinterlaced=None,        # deinterlace: the last launch that read the raw ring has finished (event on main)
            uploaded=[None, None],    # per input slot: the upload from its pinned buffer has finished (event on s_in)
            converted=[None, None],   # per input slot: the conversion has read its device buffer (event on main)
            copied=[None, None])      # per output slot: (frame index, event on s_out: the copy into its pinned buffer has finished)

    def _upload(self, st, i: int, source) -> None:
        """Source frame `i`: read into its pinned slot, from there to the device on the copy-in stream, converted into ring slot i % 3 on
        the current one."""
        self._fetch(st, i, source, self._dev_in[i % 2], st.converted[i % 2])
        self._convert(st, i)

    def _fetch(self, st, i: int, source, dst: torch.Tensor, free) -> None:
        """Source frame `i`: read into pinned slot i % 2, from there into the device buffer `dst` on the copy-in stream once `free` (an
        event on the current stream, or None: what last read `dst` has finished); the current stream then waits for the upload."""
        a = i % 2
        if st.uploaded[a] is not None:
            st.uploaded[a].synchronize()   # the pinned slot is free again (host wait on one event)
        if not source.read_into(self._pin_in[a].numpy()):   # (straight into the pinned slot: no temporary in between)
            raise ValueError(f"the source ended before frame {i} of the {st.T} asked for")
        if free is not None:
            st.s_in.wait_event(free)
        with torch.cuda.stream(st.s_in):
            dst.copy_(self._pin_in[a], non_blocking=True)
            st.uploaded[a] = torch.cuda.Event()
            st.uploaded[a].record(st.s_in)
        self.h2d_bytes += self.in_bytes
        self.frames_in += 1
        st.main.wait_event(st.uploaded[a])

    def _convert(self, st, i: int) -> None:
        """The frame in `_dev_in[i % 2]` (source frame `i`, or progressive frame `i` with `deinterlace`) converted into ring slot i % 3
        on the current stream, and with `scene` the pair (i - 1, i) summed and flagged."""
        a = i % 2
        # (ring slot i % 3 was last read by the window of frames i-3 .. i-1, stacked on this stream)
        if self._down is None:
            pix_ingest(self._dev_in[a], self.shape, self.fmt_in, self.coef_in, self.siting, self.lr_shape, lr_out=self._ring[i % 3])
        else:   # (the HR buffer was last read by the previous frame's reduction, on this stream)
            pix_ingest(self._dev_in[a], self.shape, self.fmt_in, self.coef_in, self.siting, lr_out=self._full)
            self._down(self._full, quantise=True, out=self._ring[i % 3])
        st.converted[a] = torch.cuda.Event()
        st.converted[a].record(st.main)
        if st.scene_buf is not None and i >= 1:   # the pair (i - 1, i): its sums, then its flag against the pair before
            row = st.scene_sums[i - 1:i]
            scene_sums(self._ring[(i - 1) % 3], self._ring[i % 3], out=row)
            scene_flags(row, st.scene_sums[i - 2] if i >= 2 else None, self.scene_thresholds, out=st.scene_flags[i - 1:i])

    def _forward(self, st, i: int) -> None:
        """The window of source frames i - 2 .. i through the model, the estimate fed back (as `run_item`)."""
        if st.scene_buf is None:
            x = torch.stack([self._ring[(i - 2) % 3], self._ring[(i - 1) % 3], self._ring[i % 3]])
            st.est, _ = self.model(x, None, None, st.est, train=False)
            return
        # the window and the fed-back estimate under the flags of the pairs (i - 2, i - 1) and (i - 1, i), chosen on the device; the
        # first window passes no estimate, as above: if its first pair is a cut, the model's "plane 7 = frame 0" picks the middle frame
        x, est = scene_window(self._ring[(i - 2) % 3], self._ring[(i - 1) % 3], self._ring[i % 3], st.est,
                              st.scene_flags[i - 2:i - 1], st.scene_flags[i - 1:i])
        st.est, _ = self.model(x, None, None, est, train=False)

    def _score(self, st, j: int) -> None:
        """Output frame `j` against source frame j + 1, and the pair (j - 1, j); every launch writes its row of `st.sums`."""
        def row(name, k):
            row0 = st.layout[name][0]
            return st.sums[row0 + k:row0 + k + 1]
        # source frame j + 1 is still in its upload slot (the other one of the pair): converted at full size into the reused HR buffer,
        # then scored; the slot's next upload waits for this read as it does for the LR conversion
        c = (j + 1) % 2
        est, truth, base = st.est[0], self._slot(self._truth, j), self._slot(self._base, j)
        pix_ingest(self._dev_in[c], self.shape, self.fmt_in, self.coef_in, self.siting, lr_out=truth)
        frame_metrics(est, truth, self.score, True, self.shave, out=row("estimate", j))
        if st.ms is not None:
            frame_msssim(est, truth, self.score, True, self.shave, out=st.ms[0, j:j + 1])
        if base is not None:
            self._up(self._ring[(j + 1) % 3], quantise=False, out=base)
            frame_metrics(base, truth, self.score, True, self.shave, out=row("baseline", j))
            if st.ms is not None:
                frame_msssim(base, truth, self.score, True, self.shave, out=st.ms[1, j:j + 1])
        if self.temporal is not None and j >= 1:
            # the pair (j - 1, j) along the flows between source frames j and j + 1: the other truth buffer still holds source frame j,
            # `prev_est` the estimate of the window before
            truth_prev = self._slot(self._truth, j - 1)
            flows = truth_flows(self.model, truth_prev, truth)
            pairs = [("ewarp", st.prev_est, est), ("ewarp_truth", truth_prev, truth)]
            if base is not None:
                pairs.append(("ewarp_baseline", self._slot(self._base, j - 1), base))
            for name, before, after in pairs:
                warp_error(before, after, flows, self.score, True, self.shave, self.occ, out=row(name, j - 1))
        st.prev_est = est
        st.converted[c] = torch.cuda.Event()
        st.converted[c].record(st.main)

    def _write_out(self, st, j: int) -> None:
        """Output frame `j`: written as `fmt_out` into device slot j % 2 on the current stream, copied back on the copy-out stream."""
        b = j % 2
        if st.copied[b] is not None:   # frame j-2 leaves the slot pair: wait for its copy, take it from the pinned buffer
            self._take(st, b)
            st.main.wait_event(st.copied[b][1])
        pix_write(st.est[0], self.fmt_out, self.coef_out, self.siting, out=self._dev_out[b])
        ready = torch.cuda.Event()
        ready.record(st.main)
        st.s_out.wait_event(ready)
        with torch.cuda.stream(st.s_out):
            self._pin_out[b].copy_(self._dev_out[b], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st.s_out)
        st.copied[b] = (j, ev)
        self.d2h_bytes += self.out_bytes
        self.frames_out += 1

    def _take(self, st, b: int) -> None:
        """The frame in pinned output slot `b` to the sink, once its copy has finished (host wait on one event); the view is valid during
        the call: the slot's next copy is enqueued after it returns."""
        jj, ev = st.copied[b]
        ev.synchronize()
        st.sink(jj, self._pin_out[b].numpy())

    def _drain(self, st) -> None:
        """The last two output frames, and every slot idle when run() returns."""
        for b in sorted((b for b in range(2) if st.copied[b] is not None), key=lambda b: st.copied[b][0]):   # (the sink sees them in order)
            self._take(st, b)
        for ev in st.uploaded + st.converted:
            if ev is not None:
                ev.synchronize()

    def _collect(self, st) -> dict:
        """`metrics` from the sums: one copy of the whole tensor (it waits for the current stream), then the host step of each series."""
        host = st.sums.cpu().numpy()
        metrics = {}
        for name, (row0, rows, kind) in st.layout.items():
            values = (psnr_ssim if kind == "frame" else ewarp)(host[row0:row0 + rows])
            if kind == "pair" and self.cuts is not None:   # row r is scored along the flows between source frames r + 1 and r + 2
                values[0][self.cuts[1:1 + rows]] = np.nan
            metrics.update((k, v) for k, v in zip(METRIC_KEYS[name], values) if k is not None)
        if st.ms is not None:   # one more small copy, after the wait above
            host = st.ms.cpu().numpy()
            h, w = self.shape[0] - 2 * self.shave, self.shape[1] - 2 * self.shave
            for k, name in enumerate(("msssim", "msssim_baseline")[:host.shape[0]]):
                metrics[name] = msssim(host[k], h, w)
        return metrics

    def _collect_scene(self, st, T: int) -> None:
        """`cuts` and `scene_m` from the run's scene buffer: one copy (it waits for the current stream)."""
        host = st.scene_buf.cpu().numpy()
        sums = host[:16 * (T - 1)].view(np.float64).reshape(T - 1, 2)
        self.cuts = host[16 * (T - 1):].view(np.int32) != 0
        self.scene_m = sums[:, 0] / sums[:, 1]
