"""Frames in, out, resampled, scored, watched for scene cuts and cut into training samples on the device: the Python side of the side
libraries for frames, one section each.

    read_clip_yuv / ingest_item_yuv / frames_to_yuv     ingest, and write-out for what decoders emit: packed Y'CbCr 4:2:0 frames
                            (yuv420p, nv12, yuv420p10le, p010le), converted on the device (include/vsr_hip_yuv.h); the matrix
                            coefficients come from `yuv_coefficients` alone
    resize_tables / FrameResizer   float32 RGB frames resampled on the device by a separable filter given as tables
                            (include/vsr_hip_resize.h): antialiased bicubic (Keys, a = -0.5, Pillow's convention) or bilinear; the tables
                            come from `resize_tables` alone
    frame_metrics / psnr_ssim   HR frames scored against ground truth on the device: the float64 sums behind PSNR and SSIM per frame
                            (include/vsr_hip_metric.h), and the host step that forms the two numbers from them
    frame_msssim / msssim_levels / msssim   multi-scale SSIM on the device (include/vsr_hip_msssim.h): the float64 sums of the contrast-
                            structure and SSIM maps per frame, plane and level, five levels pooled 2 x 2 on the device, and the host step
                            that forms the means, the powers and their product
    truth_flows / warp_error / ewarp   the temporal warping error on the device (include/vsr_hip_warp.h): forward and backward FlowNet2
                            flows between ground-truth frames, frame t + 1 warped back onto frame t and the squared difference summed
                            over the pixels that are not occluded, in float64, and the host step that forms E_warp from the sums
    scene_sums / scene_flags / scene_window / scene_cuts   scene cuts on the device (include/vsr_hip_scene.h): the absolute luma difference
                            of consecutive LR frames summed per pair, the cut rule on the sums as device flags, the 3-frame window and
                            the fed-back estimate composed under two flags, and the host step that applies the same rule to the sums

    pix_ingest / pix_write / ingest_item_pix / frames_to_pix   the same two steps for every planar layout: the four 4:2:0 names through
                            the library above, yuv422p, yuv444p, yuv422p10le and yuv444p10le through include/vsr_hip_pix.h
    deint_planes / deinterlace / deint_schedule / deinterlace_clip   interlaced frames made progressive on the packed bytes, before the
                            conversion (include/vsr_hip_deint.h): the planes of every layout, one frame rebuilt from itself and its two
                            neighbours in one launch, the neighbours and field parities of a whole clip, and the clip deinterlaced frame
                            by frame (what `ClipRunner(deinterlace=...)` must equal)
    patch_table / patch_gather / patch_item   training samples (include/vsr_hip_patch.h): random crops, the eight symmetries of the
                            square and time reversal drawn on the host as a table, all samples of a step cut from the resident frames
                            in one launch with their LR patches, and a sample as the (data, target, high_frames) of the train loop
    cell_stats / cell_cuts / patch_score / patch_table_select   where to cut them (include/vsr_hip_cell.h): the spatial activity and the
                            temporal difference of every 16 x 16 cell of every resident frame in one launch, the cut rule of `scene_cuts`
                            on the map's sums, the activity of a table row's crop, and a table whose rows straddle no cut and prefer
                            patches with detail

`clip_runner.ClipRunner` streams a clip through the first six, `clip_trainer.ClipTrainer` trains on patches of one; `driver` imports every public name here, so `driver.frame_metrics` and the
rest resolve as before.  `y4m` reads and writes the YUV4MPEG2 files a clip arrives in.  Transfer functions stay out.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L


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


def _ingest(side: str, code: int, fb: int, frames: torch.Tensor, shape, fmt: str, coef12, siting: str, lr_shape, want_hr: bool, lr_out):
    """What `yuv_ingest` and `pix_ingest` do alike around vsr_<side>_ingest: `code` is the format's code in that library, `fb` its frame bytes."""
    import ctypes
    H, W = int(shape[0]), int(shape[1])
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
    Y = getattr(L, "load_" + side)()
    L.check(getattr(Y, f"vsr_{side}_ingest")(L.dptr(frames, torch.uint8), code, c.ctypes.data_as(ctypes.c_void_p), YUV_SITINGS[siting], L.dptr(lr),
                                             L.optr(hr), F, H, W, h, w, L.stream()), side + "_ingest", lib=Y)
    return lr, hr


def _write(side: str, codes: dict, frame_bytes, frames: torch.Tensor, fmt: str, coef12, siting: str, out) -> torch.Tensor:
    """What `yuv_write` and `pix_write` do alike around vsr_<side>_write: `codes` the library's formats, `frame_bytes` their sizes."""
    import ctypes
    if frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError(f"expected float32 [..., H, W, 3], got {tuple(frames.shape)}")
    f = frames.detach().to(torch.float32).contiguous()
    H, W = int(f.shape[-3]), int(f.shape[-2])
    fb = frame_bytes(fmt, H, W)
    lead = tuple(f.shape[:-3])
    F = int(np.prod(lead)) if lead else 1
    c = _coef12(coef12)
    if out is None:
        out = torch.empty(lead + (fb,), dtype=torch.uint8, device=f.device)
    elif tuple(out.shape) != lead + (fb,):
        raise ValueError(f"out must be {lead + (fb,)}, got {tuple(out.shape)}")
    Y = getattr(L, "load_" + side)()
    L.check(getattr(Y, f"vsr_{side}_write")(L.dptr(f), L.dptr(out, torch.uint8), codes[fmt], c.ctypes.data_as(ctypes.c_void_p), YUV_SITINGS[siting],
                                            F, H, W, L.stream()), side + "_write", lib=Y)
    return out


@L.on_device
def yuv_ingest(frames: torch.Tensor, shape: Tuple[int, int], fmt: str, coef12, siting: str = "left", lr_shape: Optional[Tuple[int, int]] = None,
               want_hr: bool = False, lr_out: Optional[torch.Tensor] = None):
    """The low-level call (vsr_yuv_ingest) with any 12 coefficients: uint8 [..., frame_bytes] on the device -> float32 RGB
    (lr [..., h, w, 3], hr [..., H, W, 3] | None); `lr_shape` = (h, w), default the full size; `lr_out`: write lr there."""
    fb = yuv_frame_bytes(fmt, int(shape[0]), int(shape[1]))
    return _ingest("yuv", YUV_FORMATS[fmt], fb, frames, shape, fmt, coef12, siting, lr_shape, want_hr, lr_out)


@L.on_device
def yuv_write(frames: torch.Tensor, fmt: str, coef12, siting: str = "left", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The low-level call (vsr_yuv_write) with any 12 coefficients: float32 [..., H, W, 3] -> uint8 [..., frame_bytes]."""
    return _write("yuv", YUV_FORMATS, yuv_frame_bytes, frames, fmt, coef12, siting, out)


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


# ------------------------------------------------------------------------------------------------ every planar layout: 4:2:0, 4:2:2, 4:4:4
_PIX_NEW = {"yuv422p": 0, "yuv444p": 1, "yuv422p10le": 2, "yuv444p10le": 3}   # the `fmt` codes of include/vsr_hip_pix.h
PIX_FORMATS = {**YUV_FORMATS, **_PIX_NEW}   # name -> the code in its own library: the four of YUV_FORMATS (libvsr_hip_yuv.so) + libvsr_hip_pix.so's


def _pix_depth(fmt: str) -> int:
    if fmt not in PIX_FORMATS:
        raise ValueError(f"unknown pixel format {fmt!r} (known: {', '.join(PIX_FORMATS)})")
    return 10 if fmt.endswith("10le") else 8


def pix_chroma(fmt: str) -> str:
    """"420" | "422" | "444": which axes of `fmt` carry half the chroma samples."""
    _pix_depth(fmt)
    return "422" if "422" in fmt else "444" if "444" in fmt else "420"


def pix_frame_bytes(fmt: str, H: int, W: int) -> int:
    """Bytes of one packed frame of any name of `PIX_FORMATS`: 3/2 (4:2:0), 2 (4:2:2) or 3 (4:4:4) samples per pixel, 1 or 2 bytes per
    sample.  4:2:0 needs even H and W (`yuv_frame_bytes`), 4:2:2 an even W, 4:4:4 nothing but positive sizes."""
    d = _pix_depth(fmt)
    if fmt in YUV_FORMATS:
        return yuv_frame_bytes(fmt, H, W)
    ss = pix_chroma(fmt)
    if H <= 0 or W <= 0 or (ss == "422" and W % 2):
        raise ValueError(f"4:{ss[1:2]}:{ss[2:]} needs positive H and W{' and an even W' if ss == '422' else ''}, got {H} x {W}")
    return H * W * (2 if ss == "422" else 3) * (2 if d == 10 else 1)


def pix_coefficients(fmt: str, matrix: str = "bt709", full_range: bool = False, inverse: bool = False, dtype=np.float32) -> np.ndarray:
    """`yuv_coefficients` for any name of `PIX_FORMATS`: the 12 values depend on the bit depth alone, not on the chroma layout."""
    return yuv_coefficients("yuv420p10le" if _pix_depth(fmt) == 10 else "yuv420p", matrix, full_range, inverse, dtype)


@L.on_device
def pix_ingest(frames: torch.Tensor, shape: Tuple[int, int], fmt: str, coef12, siting: str = "left", lr_shape: Optional[Tuple[int, int]] = None,
               want_hr: bool = False, lr_out: Optional[torch.Tensor] = None):
    """`yuv_ingest` for any name of `PIX_FORMATS`: a 4:2:0 name goes to vsr_yuv_ingest, a 4:2:2 / 4:4:4 name to vsr_pix_ingest."""
    fb = pix_frame_bytes(fmt, int(shape[0]), int(shape[1]))
    side = "yuv" if fmt in YUV_FORMATS else "pix"
    return _ingest(side, PIX_FORMATS[fmt], fb, frames, shape, fmt, coef12, siting, lr_shape, want_hr, lr_out)


@L.on_device
def pix_write(frames: torch.Tensor, fmt: str, coef12, siting: str = "left", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`yuv_write` for any name of `PIX_FORMATS`: a 4:2:0 name goes to vsr_yuv_write, a 4:2:2 / 4:4:4 name to vsr_pix_write."""
    _pix_depth(fmt)
    return _write("yuv" if fmt in YUV_FORMATS else "pix", PIX_FORMATS, pix_frame_bytes, frames, fmt, coef12, siting, out)


def ingest_item_pix(frames: torch.Tensor, shape: Tuple[int, int], fmt: str, scale: int = 4, want_hr: bool = True, matrix: str = "bt709",
                    full_range: bool = False, siting: str = "left"):
    """`ingest_item_yuv` for any name of `PIX_FORMATS`."""
    if frames.dim() != 3 or frames.shape[1] != 3:
        raise ValueError(f"expected uint8 [T,3,frame_bytes], got {frames.dtype} {tuple(frames.shape)}")
    H, W = shape
    lr, hr = pix_ingest(frames.contiguous(), shape, fmt, pix_coefficients(fmt, matrix, full_range, inverse=True), siting,
                        (int(H / scale), int(W / scale)), want_hr)
    if hr is None:
        return lr, None, None
    return lr, hr[:, 1:2].clone(), hr   # (the clone: as in ingest_item)


def frames_to_pix(frames: torch.Tensor, fmt: str, matrix: str = "bt709", full_range: bool = False, siting: str = "left") -> torch.Tensor:
    """`frames_to_yuv` for any name of `PIX_FORMATS`."""
    return pix_write(frames, fmt, pix_coefficients(fmt, matrix, full_range), siting)


# ------------------------------------------------------------------------------------------------ deinterlacing
DEINTERLACE = (None, "frame", "field")   # "frame": one progressive frame per interlaced frame; "field": one per field (twice the rate)


def deint_planes(fmt: str, H: int, W: int):
    """The planes of one packed frame of any name of `PIX_FORMATS` as vsr_deint_frame takes them -> (planes, sample_bytes, shift):
    `planes` a list of (offset in bytes, rows, cols, comps) that tiles the `pix_frame_bytes(fmt, H, W)` bytes with no gap, in the file's
    order; nv12 / p010le carry Cb and Cr as ONE plane of comps = 2; `shift` is 6 for p010le (the value in the high 10 bits), else 0."""
    fb = pix_frame_bytes(fmt, H, W)   # (raises on an unknown name and on a shape the layout cannot hold)
    sb = 2 if _pix_depth(fmt) == 10 else 1
    ss = pix_chroma(fmt)
    ch, cw = (H // 2 if ss == "420" else H), (W if ss == "444" else W // 2)
    luma = H * W * sb
    if fmt in ("nv12", "p010le"):
        planes = [(0, H, W, 1), (luma, ch, cw, 2)]
    else:
        planes = [(0, H, W, 1), (luma, ch, cw, 1), (luma + ch * cw * sb, ch, cw, 1)]
    assert planes[-1][0] + planes[-1][1] * planes[-1][2] * planes[-1][3] * sb == fb
    return planes, sb, (6 if fmt == "p010le" else 0)


def _deint_mode(mode) -> str:
    if mode not in DEINTERLACE or mode is None:
        raise ValueError(f"deinterlace mode must be 'frame' or 'field', got {mode!r}")
    return mode


@L.on_device
def deinterlace_planes(prev: torch.Tensor, cur: torch.Tensor, next: torch.Tensor, planes, sample_bytes: int, shift: int, keep: int,
                       kept_first: int, out: torch.Tensor) -> torch.Tensor:
    """The low-level call (vsr_deint_frame) with any planes: four dense uint8 tensors on the device (`prev`, `cur` and `next` may be one
    another; `out` none of them), `planes` a list of (offset, rows, cols, comps) inside them.  The caller answers for the planes lying
    inside all four tensors.  Nothing is synchronised."""
    planes = [tuple(int(v) for v in p) for p in planes]
    arr = (L.DeintPlane * max(len(planes), 1))(*[L.DeintPlane(*p) for p in planes])
    D = L.load_deint()
    L.check(D.vsr_deint_frame(L.dptr(prev, torch.uint8), L.dptr(cur, torch.uint8), L.dptr(next, torch.uint8), L.dptr(out, torch.uint8), arr,
                              len(planes), int(sample_bytes), int(shift), int(keep), int(kept_first), L.stream()), "deint_frame", lib=D)
    return out


def deinterlace(prev: torch.Tensor, cur: torch.Tensor, next: torch.Tensor, shape: Tuple[int, int], fmt: str, keep: int, kept_first: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One interlaced frame `cur` of `fmt` (any name of `PIX_FORMATS`) and `shape` = (H, W) made progressive by the rule of
    include/vsr_hip_deint.h: uint8 device tensors of `pix_frame_bytes` bytes each -> a uint8 tensor of as many (`out`: write there).
    The rows of parity `keep` are copies of `cur`'s, the others rebuilt from `cur` and the neighbouring frames `prev` and `next`
    (at a clip end pass the other neighbour, `deint_schedule`); `kept_first`: the kept field is the first of `cur`'s two in time.  One
    launch, nothing is synchronised."""
    H, W = int(shape[0]), int(shape[1])
    planes, sb, shift = deint_planes(fmt, H, W)
    fb = pix_frame_bytes(fmt, H, W)
    for name, t in (("prev", prev), ("cur", cur), ("next", next)) + ((("out", out),) if out is not None else ()):
        if t.dtype != torch.uint8 or t.numel() != fb or t.device != cur.device:
            raise ValueError(f"{name} must be uint8 of {fb} bytes ({fmt} {H}x{W}) on {cur.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if min(p[1] for p in planes) < 2:
        raise ValueError(f"{fmt} {H}x{W}: a plane of {min(p[1] for p in planes)} row(s) holds no two fields")
    if out is None:
        out = torch.empty(fb, dtype=torch.uint8, device=cur.device)
    return deinterlace_planes(prev, cur, next, planes, sb, shift, keep, kept_first, out)


def deint_schedule(T: int, mode: str, tff: bool = True) -> list:
    """The progressive frames of a clip of `T` interlaced frames, in time order, as (prev, cur, next, keep, kept_first): the indices of
    the three frames `deinterlace` takes and its two flags.  Pure host code.  The neighbours of frame i are i - 1 and i + 1; at a clip
    end the missing neighbour is the OTHER neighbour (reflection: the frame itself there would blind td0 and td1 of the rule), and for
    T = 1 both are the frame itself.  "frame": per interlaced frame one entry that keeps its first field in time (keep = 0 if `tff` else
    1, kept_first = 1); "field": that entry, then the second field's (keep flipped, kept_first = 0): 2 T entries."""
    _deint_mode(mode)
    T = int(T)
    if T <= 0:
        raise ValueError(f"a clip has at least one frame, got {T}")
    first = 0 if tff else 1
    out = []
    for i in range(T):
        p, n = i - 1, i + 1
        if p < 0:
            p = n if n < T else i
        if n >= T:
            n = p
        out.append((p, i, n, first, 1))
        if mode == "field":
            out.append((p, i, n, 1 - first, 0))
    return out


def deinterlace_clip(frames_u8, shape: Tuple[int, int], fmt: str, mode: str, tff: bool = True, device="cuda") -> np.ndarray:
    """A whole clip deinterlaced on the device, frame by frame: uint8 [T, frame_bytes] (a host array or a tensor) -> a host array
    [T, frame_bytes] ("frame") or [2 T, frame_bytes] ("field"), the entries of `deint_schedule` in order.  The definition of what
    `ClipRunner(deinterlace=mode, tff=tff)` feeds its windows; a clip's length of device memory, so a tool for tests and short clips."""
    t = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames_u8)))
    fb = pix_frame_bytes(fmt, int(shape[0]), int(shape[1]))
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != fb or t.shape[0] < 1:
        raise ValueError(f"expected uint8 [T >= 1, {fb}] ({fmt} {shape[0]}x{shape[1]}), got {t.dtype} {tuple(t.shape)}")
    sched = deint_schedule(int(t.shape[0]), mode, tff)
    src = t.to(device).contiguous()
    out = torch.empty((len(sched), fb), dtype=torch.uint8, device=src.device)
    for q, (p, i, n, keep, kept_first) in enumerate(sched):
        deinterlace(src[p], src[i], src[n], shape, fmt, keep, kept_first, out=out[q])
    return out.cpu().numpy()


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


# ------------------------------------------------------------------------------------------------ PSNR / SSIM
METRIC_CHANNELS = {"rgb": 0, "y": 1}     # the `channels` codes of include/vsr_hip_metric.h
METRIC_WHAT = {"psnr": 1, "ssim": 2}     # the bits of `what`: PSNR needs the SSE


def ssim_window() -> np.ndarray:
    """The normalised 1-D window of SSIM (Wang et al. 2004): 11 taps of exp(-(i - 5)^2 / (2 * 1.5^2)) over their sum, float64; the 2-D
    window is its outer product."""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


# the arguments and the sums `frame_metrics` and `warp_error` have in common
def _channel_code(channels: str) -> int:
    if channels not in METRIC_CHANNELS:
        raise ValueError(f"unknown channels {channels!r} (known: {', '.join(METRIC_CHANNELS)})")
    return METRIC_CHANNELS[channels]


def _frame_pair(a: torch.Tensor, b: torch.Tensor, many: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two frame sets of one shape, [H,W,3] (one frame) or [`many`,H,W,3] -> both as contiguous [N,H,W,3]."""
    if tuple(a.shape) != tuple(b.shape) or a.dim() not in (3, 4) or a.shape[-1] != 3:
        raise ValueError(f"expected two float32 tensors of one shape [H,W,3] or [{many},H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dim() == 3:
        a, b = a[None], b[None]
    return a.detach().contiguous(), b.detach().contiguous()


def _luma4(channels: str, matrix: str, full_range: bool) -> Optional[np.ndarray]:
    """{a0, a1, a2, o} of the luma the kernels form in "y" mode: row 0 of `yuv_coefficients` and its offset, float32."""
    if channels != "y":
        return None
    c = yuv_coefficients("yuv420p", matrix, full_range)
    return np.ascontiguousarray(np.array([c[0], c[1], c[2], c[9]], dtype=np.float32))


def _sums_out(out: Optional[torch.Tensor], shape: tuple, device) -> torch.Tensor:
    """The float64 tensor of `shape` the sums go to: `out` if it fits (rows of a larger tensor will do), else a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if tuple(out.shape) != shape or out.device != device:
        raise ValueError(f"out must be float64 {shape} on {device}, got {tuple(out.shape)} on {out.device}")
    return out


def _sums_array(sums) -> np.ndarray:
    """Sums [n,4] (a tensor, copied to the host here, or an array) as a float64 array [n,4]."""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    return np.asarray(s, dtype=np.float64).reshape(-1, 4)


def _score_frames(name: str, a, b, quantise, shave, refuse, luma4, out, out_shape: tuple, head: tuple) -> torch.Tensor:
    """What `frame_metrics` (name "metric") and `frame_msssim` ("msssim") do alike around vsr_<name>_frames: the frame pair, the shave
    and the size (`refuse(H, W, shave)` raises what the entry would refuse), the window, the device pointers, the sums [F] + `out_shape`
    and the workspace.  `head`: the entry's arguments between W and quantise; the first of them is also vsr_<name>_ws_bytes' last."""
    import ctypes
    fa, fb = _frame_pair(a, b, "F")
    shave = int(shave)
    F, H, W = int(fa.shape[0]), int(fa.shape[1]), int(fa.shape[2])
    refuse(H, W, shave)
    win = ssim_window()
    M = getattr(L, "load_" + name)()
    pa, pb = L.dptr(fa), L.dptr(fb)   # (raises on CPU tensors and on anything but float32)
    if fb.device != fa.device:
        raise ValueError("the two tensors live on different devices")
    out = _sums_out(out, (F,) + out_shape, fa.device)
    ws = torch.empty(int(getattr(M, f"vsr_{name}_ws_bytes")(F, H, W, shave, head[0])), dtype=torch.uint8, device=fa.device)
    L.check(getattr(M, f"vsr_{name}_frames")(pa, pb, F, H, W, *head, 1 if quantise else 0, shave,
                                             None if luma4 is None else luma4.ctypes.data_as(ctypes.c_void_p),
                                             win.ctypes.data_as(ctypes.c_void_p), L.dptr(out, torch.float64), L.dptr(ws, torch.uint8),
                                             L.stream()), name + "_frames", lib=M)
    return out


@L.on_device
def frame_metrics(a: torch.Tensor, b: torch.Tensor, channels: str = "rgb", quantise: bool = True, shave: int = 0, what=("psnr", "ssim"),
                  matrix: str = "bt601", full_range: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 RGB frames `a`, `b` ([H,W,3], [1,H,W,3] or [F,H,W,3], 0..255) -> the device tensor [F,4] float64 of
    {sse, n_sse, ssim_sum, n_ssim} per frame (vsr_metric_frames); nothing is synchronised, `psnr_ssim` is the host step.
    `quantise`: score what write-out stores (clamp to 0..255, round half to even); `shave`: pixels dropped on every side;
    `channels="y"`: on the luma of `matrix` / `full_range` (row 0 of `yuv_coefficients`; the default is BT.601 limited range, the
    literature's "Y"); `what`: "psnr" and / or "ssim" (the slots of the other are 0); `out`: write the sums there ([F,4] float64)."""
    code = _channel_code(channels)
    names = (what,) if isinstance(what, str) else tuple(what)
    if not names or any(n not in METRIC_WHAT for n in names):
        raise ValueError(f"what must name 'psnr' and / or 'ssim', got {what!r}")
    bits = 0
    for n in names:
        bits |= METRIC_WHAT[n]

    def refuse(H, W, shave):
        if shave < 0 or 2 * shave >= min(H, W):
            raise ValueError(f"shave {shave} leaves nothing of {H} x {W}")
        if bits & 2 and min(H, W) - 2 * shave < 11:
            raise ValueError(f"SSIM needs 11 pixels each way after the shave, got {min(H, W) - 2 * shave}")

    return _score_frames("metric", a, b, quantise, shave, refuse, _luma4(channels, matrix, full_range), out, (4,), (bits, code))


def psnr_ssim(sums) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `frame_metrics`: sums [F,4] (a tensor, copied to the host here, or an array) -> (PSNR [F] in dB,
    SSIM [F]).  PSNR = 10 log10(255^2 n_sse / sse), `inf` where sse == 0; SSIM = ssim_sum / n_ssim.  A metric that was not asked for
    (its count is 0) comes back as NaN."""
    s = _sums_array(sums)
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


# ------------------------------------------------------------------------------------------------ multi-scale SSIM
MSSSIM_BETA = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # the exponents of levels 1 to 5 (Wang, Simoncelli, Bovik 2003)
MSSSIM_MIN_SIZE = 161                                    # VSR_MSSSIM_MIN_SIZE of include/vsr_hip_msssim.h: 161, 81, 41, 21, 11


def msssim_levels(h: int, w: int) -> list:
    """The five (h_j, w_j) of a plane of h x w (after the shave): every level half the one before, rounded up."""
    out = []
    for _ in range(len(MSSSIM_BETA)):
        out.append((int(h), int(w)))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


@L.on_device
def frame_msssim(a: torch.Tensor, b: torch.Tensor, channels: str = "rgb", quantise: bool = True, shave: int = 0, luma4=None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 RGB frames `a`, `b` ([H,W,3], [1,H,W,3] or [F,H,W,3], 0..255) -> the device tensor [F,P,5,2] float64 of
    {cs_sum, ssim_sum} per frame, plane (P = 3 for "rgb", 1 for "y") and level (vsr_msssim_frames); nothing is synchronised, `msssim`
    is the host step.  `quantise`, `shave`, `channels`: as `frame_metrics`; `luma4`: four float32 {a0, a1, a2, o} of the luma of "y"
    mode, default the BT.601 limited-range luma of `frame_metrics`; `out`: write the sums there ([F,P,5,2] float64)."""
    code = _channel_code(channels)

    def refuse(H, W, shave):
        if shave < 0 or min(H, W) - 2 * shave < MSSSIM_MIN_SIZE:
            raise ValueError(f"MS-SSIM needs {MSSSIM_MIN_SIZE} pixels each way after the shave, got {min(H, W) - 2 * shave} "
                             f"(shave {shave} of {H} x {W})")

    if channels == "y":
        luma4 = _luma4("y", "bt601", False) if luma4 is None else np.ascontiguousarray(np.asarray(luma4, dtype=np.float32).reshape(4))
    else:
        luma4 = None
    return _score_frames("msssim", a, b, quantise, shave, refuse, luma4, out, (1 if channels == "y" else 3, len(MSSSIM_BETA), 2), (code,))


def msssim(sums, h: int, w: int) -> np.ndarray:
    """The host step after `frame_msssim`: sums [F,P,5,2] (a tensor, copied to the host here, or an array) of planes of h x w (after the
    shave) -> MS-SSIM [F].  Per plane prod_{j<5} max(mcs_j, 0)^beta_j * max(mssim_5, 0)^beta_5, the means being the sums over
    (h_j - 10)(w_j - 10) and beta `MSSSIM_BETA`; the result is the mean over the planes (the per-channel rule of
    tf.image.ssim_multiscale and pytorch-msssim)."""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    s = np.asarray(s, dtype=np.float64)
    if s.ndim != 4 or s.shape[2:] != (len(MSSSIM_BETA), 2):
        raise ValueError(f"expected sums [F,P,5,2], got {s.shape}")
    n = np.array([(hj - 10) * (wj - 10) for hj, wj in msssim_levels(h, w)], dtype=np.float64)
    if n[-1] <= 0:
        raise ValueError(f"MS-SSIM needs {MSSSIM_MIN_SIZE} pixels each way, got {h} x {w}")
    means = s / n[None, None, :, None]
    terms = np.concatenate([means[:, :, :-1, 0], means[:, :, -1:, 1]], axis=2)   # mcs_1 .. mcs_4, mssim_5
    per_plane = np.prod(np.maximum(terms, 0.0) ** np.array(MSSSIM_BETA), axis=2)
    return per_plane.mean(axis=1)


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
    code = _channel_code(channels)
    fwd, bwd, crop = flows
    fa, fb = _frame_pair(a, b, "P")
    P, H, W = int(fa.shape[0]), int(fa.shape[1]), int(fa.shape[2])
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
    else:
        luma4 = _luma4(channels, matrix, full_range)
    occ4 = np.ascontiguousarray(np.asarray(WARP_OCC if occ is None else occ, dtype=np.float64).reshape(4))
    M = L.load_warp()
    pa, pb = L.dptr(fa), L.dptr(fb)   # (raises on CPU tensors and on anything but float32)
    pf, pg = L.dptr(fwd, fwd.dtype), L.dptr(bwd, bwd.dtype)
    if any(t.device != fa.device for t in (fb, fwd, bwd)):
        raise ValueError("the frames and the flows live on different devices")
    out = _sums_out(out, (P, 4), fa.device)
    ws = torch.empty(int(M.vsr_warp_ws_bytes(P, h, w, shave)), dtype=torch.uint8, device=fa.device)
    L.check(M.vsr_warp_error(pa, pb, P, H, W, y0, x0, h, w, pf, pg, ftype, strides[0], strides[1], strides[2], code,
                             1 if quantise else 0, shave, None if luma4 is None else luma4.ctypes.data_as(ctypes.c_void_p),
                             occ4.ctypes.data_as(ctypes.c_void_p), L.dptr(out, torch.float64), L.dptr(ws, torch.uint8), L.stream()),
            "warp_error", lib=M)
    return out


def ewarp(sums) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `warp_error`: sums [P,4] (a tensor, copied to the host here, or an array) -> (E_warp [P] = sse / n_terms /
    255^2, the mean squared warping error over the valid pixels in the 0..1 range of Lai et al. 2018; valid share [P] = n_valid /
    n_pixels).  E_warp is NaN where no pixel is valid."""
    s = _sums_array(sums)
    e = np.full(s.shape[0], np.nan)
    on = s[:, 2] > 0
    e[on] = s[on, 0] / s[on, 1] / 255.0 ** 2
    return e, s[:, 2] / s[:, 3]


# ------------------------------------------------------------------------------------------------ scene cuts
SCENE_THRESHOLDS = (15.0, 2.0)   # {t_abs on the 0..255 luma scale, ratio against the pair before}: this project's choice, not validated on real video


def _scene_thresholds(thresholds) -> Tuple[float, float]:
    """(t_abs, ratio) as two floats, default `SCENE_THRESHOLDS`; both finite and not negative (what vsr_scene_decide accepts)."""
    t = np.asarray(SCENE_THRESHOLDS if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
    if t.size != 2 or not np.isfinite(t).all() or (t < 0).any():
        raise ValueError(f"scene thresholds are (t_abs, ratio), both finite and not negative, got {thresholds!r}")
    return float(t[0]), float(t[1])


@L.on_device
def scene_sums(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, luma4=None) -> torch.Tensor:
    """float32 RGB frames `a`, `b` ([h,w,3] or [P,h,w,3], 0..255) -> the device tensor [P,2] float64 of {sad, n} per pair
    (vsr_scene_pair_sums, include/vsr_hip_scene.h): the absolute difference of the two frames' 8-bit luma codes summed over the pixels,
    and their count.  Nothing is synchronised; `scene_flags` is the device step on the sums, `scene_cuts` the host step.  `luma4`: four
    float32 {a0, a1, a2, o}, default the BT.601 luma of `frame_metrics`; `out`: write the sums there ([P,2] float64, rows of a larger
    tensor will do)."""
    import ctypes
    fa, fb = _frame_pair(a, b, "P")
    P, h, w = int(fa.shape[0]), int(fa.shape[1]), int(fa.shape[2])
    luma4 = _luma4("y", "bt601", False) if luma4 is None else np.ascontiguousarray(np.asarray(luma4, dtype=np.float32).reshape(4))
    M = L.load_scene()
    pa, pb = L.dptr(fa), L.dptr(fb)   # (raises on CPU tensors and on anything but float32)
    if fb.device != fa.device:
        raise ValueError("the two tensors live on different devices")
    if out is None:
        out = torch.empty((P, 2), dtype=torch.float64, device=fa.device)
    elif tuple(out.shape) != (P, 2) or out.device != fa.device:
        raise ValueError(f"out must be float64 {(P, 2)} on {fa.device}, got {tuple(out.shape)} on {out.device}")
    ws = torch.empty(int(M.vsr_scene_ws_bytes(P, h, w)), dtype=torch.uint8, device=fa.device)
    L.check(M.vsr_scene_pair_sums(pa, pb, P, h, w, luma4.ctypes.data_as(ctypes.c_void_p), L.dptr(out, torch.float64), L.dptr(ws, torch.uint8),
                                  L.stream()), "scene_pair_sums", lib=M)
    return out


@L.on_device
def scene_flags(sums: torch.Tensor, prev: Optional[torch.Tensor] = None, thresholds=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The cut rule on the device (vsr_scene_decide): `sums` [P,2] float64 as `scene_sums` writes them -> int32 [P], 1 where pair p is a
    cut: m_p = sad_p / n_p, flag_p = m_p >= t_abs and m_p >= ratio * m_{p-1}; for p = 0 the pair before is `prev` (two float64 {sad, n} on
    the device, e.g. the row above in a larger tensor), m = 0 without it.  `thresholds`: (t_abs, ratio), default `SCENE_THRESHOLDS`; `out`:
    write the flags there (int32 [P], elements of a larger tensor will do).  Nothing is synchronised."""
    if sums.dim() != 2 or sums.shape[1] != 2:
        raise ValueError(f"expected float64 sums [P,2], got {tuple(sums.shape)}")
    P = int(sums.shape[0])
    t_abs, ratio = _scene_thresholds(thresholds)
    if prev is not None and (prev.numel() != 2 or prev.device != sums.device):
        raise ValueError(f"prev must be two float64 values on {sums.device}, got {tuple(prev.shape)} on {prev.device}")
    M = L.load_scene()
    ps = L.dptr(sums, torch.float64)
    if out is None:
        out = torch.empty((P,), dtype=torch.int32, device=sums.device)
    elif tuple(out.shape) != (P,) or out.device != sums.device:
        raise ValueError(f"out must be int32 {(P,)} on {sums.device}, got {tuple(out.shape)} on {out.device}")
    L.check(M.vsr_scene_decide(ps, P, L.optr(prev, torch.float64), t_abs, ratio, L.dptr(out, torch.int32), L.stream()), "scene_decide", lib=M)
    return out


@L.on_device
def scene_window(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, prev_est: Optional[torch.Tensor] = None,
                 flag_ab: Optional[torch.Tensor] = None, flag_bc: Optional[torch.Tensor] = None):
    """The window of three consecutive LR frames `a`, `b`, `c` (float32 [h,w,3]) and the fed-back estimate under two device flags
    (vsr_scene_window; one int32 element each, None: not set) -> (x [3,h,w,3], est [1,h,w,3] | None): x = (flag_ab ? b : a, b,
    flag_bc ? b : c); est = b where flag_ab is set, else `prev_est` ([1,H,W,3] or [H,W,3], H = S h, W = S w) at its pixels (y S, x S):
    the nearest resize VSR.forward performs; None without `prev_est` (the first window of a run).  Bit copies throughout.  Both results are
    freshly allocated on every call: `VSR.temporal_cache` keys on storage identity and version, which a raw-pointer write into reused
    storage would not change.  Nothing is synchronised."""
    if a.dim() != 3 or a.shape[-1] != 3 or tuple(b.shape) != tuple(a.shape) or tuple(c.shape) != tuple(a.shape):
        raise ValueError(f"expected three float32 frames of one shape [h,w,3], got {tuple(a.shape)}, {tuple(b.shape)} and {tuple(c.shape)}")
    h, w = int(a.shape[0]), int(a.shape[1])
    H = W = 0
    if prev_est is not None:
        if prev_est.dim() not in (3, 4) or prev_est.shape[-1] != 3 or (prev_est.dim() == 4 and prev_est.shape[0] != 1):
            raise ValueError(f"prev_est must be float32 [1,H,W,3] or [H,W,3], got {tuple(prev_est.shape)}")
        prev_est = prev_est.detach().to(torch.float32).contiguous()   # (the model's output is a permuted view: the copy VSR.forward makes)
        H, W = int(prev_est.shape[-3]), int(prev_est.shape[-2])
        if H % h or W % w or H // h != W // w:
            raise ValueError(f"prev_est of {H} x {W} is no integer multiple (one factor both ways) of the frames of {h} x {w}")
    for name, f in (("flag_ab", flag_ab), ("flag_bc", flag_bc)):
        if f is not None and f.numel() != 1:
            raise ValueError(f"{name} must be one int32 element on the device, got {tuple(f.shape)}")
    M = L.load_scene()
    pa, pb, pc = L.dptr(a.detach()), L.dptr(b.detach()), L.dptr(c.detach())   # (raises on CPU tensors, other dtypes and strided views)
    if any(t is not None and t.device != a.device for t in (b, c, prev_est, flag_ab, flag_bc)):
        raise ValueError("the frames, the estimate and the flags live on different devices")
    x = torch.empty((3, h, w, 3), dtype=torch.float32, device=a.device)
    est = torch.empty((1, h, w, 3), dtype=torch.float32, device=a.device) if prev_est is not None else None
    L.check(M.vsr_scene_window(pa, pb, pc, L.optr(prev_est), H, W, L.optr(flag_ab, torch.int32), L.optr(flag_bc, torch.int32), L.dptr(x),
                               L.optr(est), h, w, L.stream()), "scene_window", lib=M)
    return x, est


def scene_cuts(sums, thresholds=None) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `scene_sums`: sums [P,2] of CONSECUTIVE pairs (a tensor, copied to the host here, or an array) -> (cuts bool
    [P], m float64 [P]), the rule of `scene_flags` with no pair before the first: m = sad / n, cut_p = m_p >= t_abs and
    m_p >= ratio * m_{p-1} (m_{-1} = 0)."""
    t_abs, ratio = _scene_thresholds(thresholds)
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    s = np.asarray(s, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s[:, 0] / s[:, 1]
        m_prev = np.concatenate([[0.0], m[:-1]])
        cuts = (m >= t_abs) & (m >= ratio * m_prev)
    return cuts, m


# ------------------------------------------------------------------------------------------------ training patches
PATCH_FLAGS = {"flip_x": 1, "flip_y": 2, "transpose": 4, "reverse": 8}   # the `flags` bits of include/vsr_hip_patch.h
PATCH_MAX_B = 64                                                          # VSR_PATCH_MAX_B


def _patch_shape(patch) -> Tuple[int, int]:
    """`patch` as (Ph, Pw): one edge for a square patch, or the pair."""
    if isinstance(patch, (int, np.integer)):
        return int(patch), int(patch)
    Ph, Pw = patch
    return int(Ph), int(Pw)


def patch_table(rng, B: int, G: int, n: int, shape: Tuple[int, int], patch, S: int, augment: bool = True,
                transpose: Optional[bool] = None) -> np.ndarray:
    """B training samples drawn from `G` resident frames of `shape` = (H, W) as the table vsr_patch_gather takes: int32 [B,4] of
    {t0, y0, x0, flags}; `patch` = the HR patch (one edge or (Ph, Pw)), `n` the frames per sample, `S` the scale.  Pure host code; `rng`
    is an `np.random.RandomState`.  The draw order is part of the contract (same seed, same table).  Per row, in this order:
        1. flags = rng.randint(16)     (not drawn, 0, when `augment` is false; bit 4, the transposition, masked off AFTER the draw when
                                        Ph != Pw, unless the caller passes transpose=True; transpose=False masks it off always)
        2. t0 = rng.randint(G - n + 1)
        3. y0 = rng.randint((H - ch) // S + 1) * S      (ch, cw) = (Pw, Ph) where bit 4 is set, else (Ph, Pw)
        4. x0 = rng.randint((W - cw) // S + 1) * S
    Origins are multiples of S, so both LR modes of `patch_gather` accept every row."""
    Ph, Pw = _patch_shape(patch)
    H, W = int(shape[0]), int(shape[1])
    B, G, n, S = int(B), int(G), int(n), int(S)
    if B <= 0 or n <= 0 or G < n:
        raise ValueError(f"need B > 0 and 0 < n <= G, got B {B}, n {n}, G {G}")
    if S <= 0 or Ph <= 0 or Pw <= 0 or Ph % S or Pw % S:
        raise ValueError(f"the patch of {Ph} x {Pw} must be a positive multiple of S = {S}")
    may_transpose = (Ph == Pw) if transpose is None else bool(transpose)
    if Ph > H or Pw > W or (may_transpose and (Pw > H or Ph > W)):
        raise ValueError(f"the patch of {Ph} x {Pw} does not fit the frames of {H} x {W}")
    table = np.empty((B, 4), dtype=np.int32)
    for b in range(B):
        flags = int(rng.randint(16)) if augment else 0
        if not may_transpose:
            flags &= ~PATCH_FLAGS["transpose"]
        ch, cw = (Pw, Ph) if flags & PATCH_FLAGS["transpose"] else (Ph, Pw)
        t0 = int(rng.randint(G - n + 1))
        y0 = int(rng.randint((H - ch) // S + 1)) * S
        x0 = int(rng.randint((W - cw) // S + 1)) * S
        table[b] = (t0, y0, x0, flags)
    return table


@L.on_device
def patch_gather(src: torch.Tensor, table, n: int, patch, S: int, lr_src: Optional[torch.Tensor] = None, want_hr: bool = True,
                 hr_out: Optional[torch.Tensor] = None, lr_out: Optional[torch.Tensor] = None, want_lr: bool = True):
    """The samples of `table` (int32 [B,4] on the HOST, as `patch_table` draws them) cut from `src`, float32 RGB [G,H,W,3] on the device,
    in one launch (vsr_patch_gather, include/vsr_hip_patch.h) -> (hr [B,n,Ph,Pw,3] | None, lr [B,n,Ph/S,Pw/S,3]).  `lr_src` None: lr is
    the nearest decimation of the augmented patch, lr[i][j] = hr[i S][j S]; `lr_src` [G,H/S,W/S,3]: the frames reduced beforehand, cut and
    augmented the same way.  `want_hr=False`: only lr; `want_lr=False`: only hr (the other is None).  `hr_out` / `lr_out`: write there.
    Nothing is synchronised."""
    import ctypes
    Ph, Pw = _patch_shape(patch)
    S, n = int(S), int(n)
    if src.dim() != 4 or src.shape[-1] != 3:
        raise ValueError(f"expected float32 [G,H,W,3], got {tuple(src.shape)}")
    G, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] == 0:
        raise ValueError(f"expected a table int32 [B,4] of {{t0, y0, x0, flags}}, got {t.shape}")
    B = int(t.shape[0])
    if S <= 0 or Ph % S or Pw % S:
        raise ValueError(f"the patch of {Ph} x {Pw} must be a multiple of S = {S}")
    if lr_src is not None and (tuple(lr_src.shape) != (G, H // S, W // S, 3) or H % S or W % S or lr_src.device != src.device):
        raise ValueError(f"lr_src must be float32 {(G, H // S, W // S, 3)} on {src.device} (frames a multiple of S = {S}), got "
                         f"{tuple(lr_src.shape)} on {lr_src.device}")
    M = L.load_patch()
    ps, pl = L.dptr(src), L.optr(lr_src)   # (raises on CPU tensors, on anything but float32 and on strided views)

    def out(given, shape, name):
        if given is None:
            return torch.empty(shape, dtype=torch.float32, device=src.device)
        if tuple(given.shape) != shape or given.device != src.device:
            raise ValueError(f"{name} must be float32 {shape} on {src.device}, got {tuple(given.shape)} on {given.device}")
        return given

    hr = out(hr_out, (B, n, Ph, Pw, 3), "hr_out") if want_hr or hr_out is not None else None
    lr = out(lr_out, (B, n, Ph // S, Pw // S, 3), "lr_out") if want_lr or lr_out is not None else None
    if hr is None and lr is None:
        raise ValueError("nothing is asked for (want_hr and want_lr are both false)")
    L.check(M.vsr_patch_gather(ps, G, H, W, pl, S, t.ctypes.data_as(ctypes.c_void_p), B, n, Ph, Pw, L.optr(hr), L.optr(lr), L.stream()),
            "patch_gather", lib=M)
    return hr, lr


def patch_item(hr: torch.Tensor, lr: torch.Tensor, b: int):
    """Sample `b` of `patch_gather`'s (hr [B,n,Hp,Wp,3], lr [B,n,h,w,3]) as one item of the train loop -> (data [n-2,3,h,w,3], target
    [n-2,1,Hp,Wp,3], high_frames [n-2,3,Hp,Wp,3]): the overlapping 3-frame windows lr[b, t:t+3] and hr[b, t:t+3], target the middle frame
    (as `ingest_item`).  `data` is a view; `high_frames` and `target` are their own storage: VSR.forward overwrites high_frames[t][1] in
    place, and views of one run would hand the next window a frame the previous one has overwritten."""
    n = int(hr.shape[1])
    if hr.dim() != 5 or lr.dim() != 5 or n < 3 or lr.shape[1] != n or lr.shape[0] != hr.shape[0]:
        raise ValueError(f"expected hr [B,n >= 3,Hp,Wp,3] and lr [B,n,h,w,3], got {tuple(hr.shape)} and {tuple(lr.shape)}")
    data = lr[b].unfold(0, 3, 1).permute(0, 4, 1, 2, 3)            # [n-2,3,h,w,3]: window t is lr[b, t:t+3]
    high_frames = hr[b].unfold(0, 3, 1).permute(0, 4, 1, 2, 3).contiguous()
    return data, high_frames[:, 1:2].clone(), high_frames


# ------------------------------------------------------------------------------------------------ where to cut training patches
CELL = 16   # VSR_CELL of include/vsr_hip_cell.h


def cell_shape(shape: Tuple[int, int]) -> Tuple[int, int]:
    """(Ch, Cw) = (ceil(H / CELL), ceil(W / CELL)): the cells of a frame of `shape` = (H, W)."""
    return -(-int(shape[0]) // CELL), -(-int(shape[1]) // CELL)


@L.on_device
def cell_stats(frames: torch.Tensor, luma4=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 RGB `frames` [G,H,W,3] (0..255) on the device -> the device tensor int32 [G,Ch,Cw,2] of vsr_cell_stats
    (include/vsr_hip_cell.h), (Ch, Cw) = `cell_shape`: per frame and cell of CELL x CELL pixels, channel 0 the sum of |dx| + |dy| of the
    8-bit luma code over the cell's pixels (neighbours inside the frame only), channel 1 the sum of its absolute difference against the
    frame before (0 for the first frame).  One launch; every frame is read once.  Nothing is synchronised; `cell_cuts`, `patch_score` and
    `patch_table_select` are the host steps on the map.  `luma4`: four float32 {a0, a1, a2, o}, default the BT.601 luma of `scene_sums`;
    `out`: write the map there (int32 of that shape, part of a larger tensor will do)."""
    import ctypes
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"expected float32 [G,H,W,3], got {tuple(frames.shape)}")
    G, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    luma4 = _luma4("y", "bt601", False) if luma4 is None else np.ascontiguousarray(np.asarray(luma4, dtype=np.float32).reshape(4))
    M = L.load_cell()
    pf = L.dptr(frames)   # (raises on CPU tensors, on anything but float32 and on strided views)
    shape = (G,) + cell_shape((H, W)) + (2,)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=frames.device)
    elif tuple(out.shape) != shape or out.device != frames.device:
        raise ValueError(f"out must be int32 {shape} on {frames.device}, got {tuple(out.shape)} on {out.device}")
    L.check(M.vsr_cell_stats(pf, G, H, W, luma4.ctypes.data_as(ctypes.c_void_p), L.dptr(out, torch.int32), L.stream()), "cell_stats", lib=M)
    return out


def _stats_array(stats) -> np.ndarray:
    """The map [G,Ch,Cw,2] (a tensor, copied to the host here, or an array) as an int64 array."""
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    if s.ndim != 4 or s.shape[-1] != 2:
        raise ValueError(f"expected the map int32 [G,Ch,Cw,2] of cell_stats, got {s.shape}")
    return s.astype(np.int64)


def cell_cuts(stats, shape: Tuple[int, int], thresholds=None) -> Tuple[np.ndarray, np.ndarray]:
    """The host step after `cell_stats`: the map of ONE group of G frames of `shape` = (H, W) -> (cuts bool [G-1], m float64 [G-1]).
    Pair p = (p, p + 1) has sad = stats[p+1, :, :, 1].sum() in int64 and n = H * W; the rest is `scene_cuts` on those rows, unchanged:
    m = sad / n, cut_p = m_p >= t_abs and m_p >= ratio * m_{p-1}, with m_{-1} = 0 AT THE START OF EVERY GROUP: the pair between two groups
    is not scored, because samples never span groups, so a group's first pair is judged on t_abs alone.  The m are, bit for bit, those of
    `scene_sums` / `scene_cuts` on the same consecutive frames.  `thresholds`: (t_abs, ratio), default `SCENE_THRESHOLDS`."""
    s = _stats_array(stats)
    H, W = int(shape[0]), int(shape[1])
    if tuple(s.shape[1:3]) != cell_shape((H, W)):
        raise ValueError(f"the map of {s.shape[1]} x {s.shape[2]} cells is not that of frames of {H} x {W}")
    _scene_thresholds(thresholds)
    if s.shape[0] < 2:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.float64)
    sums = np.empty((s.shape[0] - 1, 2), dtype=np.float64)
    sums[:, 0] = s[1:, :, :, 1].sum(axis=(1, 2))
    sums[:, 1] = float(H * W)
    return scene_cuts(sums, thresholds)


def _crop_cells(row, patch) -> Tuple[int, int, int, int]:
    """(i0, i1, j0, j1): the cells wholly inside the crop of table row `row`, i in [i0, i1), j in [j0, j1)."""
    Ph, Pw = _patch_shape(patch)
    _, y0, x0, flags = (int(v) for v in row)
    ch, cw = (Pw, Ph) if flags & PATCH_FLAGS["transpose"] else (Ph, Pw)
    return -(-y0 // CELL), (y0 + ch) // CELL, -(-x0 // CELL), (x0 + cw) // CELL


def patch_score(stats, row, n: int, patch) -> float:
    """The activity of the sample of table row `row` = {t0, y0, x0, flags} (`patch_table`) on the map `stats` [G,Ch,Cw,2] of `cell_stats`:
    the mean |dx| + |dy| in luma codes per pixel, float64.  (ch, cw) is the crop of the row, (Pw, Ph) under the transposition bit; the
    counted cells are those wholly inside the crop, i in [ceil(y0 / CELL), floor((y0 + ch) / CELL)), j likewise (so a ragged cell of the
    frame's edge is never counted); the score is the sum of stats[t, i, j, 0] over them and t in [t0, t0 + n), divided once in double by
    n * cells * CELL * CELL.  A crop with no whole cell inside is refused (every crop of at least 2 * CELL - 1 each way has one)."""
    s = stats if isinstance(stats, np.ndarray) and stats.dtype == np.int64 and stats.ndim == 4 else _stats_array(stats)
    i0, i1, j0, j1 = _crop_cells(row, patch)
    t0, n = int(row[0]), int(n)
    if i1 <= i0 or j1 <= j0:
        raise ValueError(f"the crop of row {tuple(int(v) for v in row)} holds no whole cell of {CELL} x {CELL}")
    if t0 < 0 or n <= 0 or t0 + n > s.shape[0] or i0 < 0 or j0 < 0 or i1 > s.shape[1] or j1 > s.shape[2]:
        raise ValueError(f"row {tuple(int(v) for v in row)} with n = {n} leaves the map of {tuple(s.shape[:3])}")
    total = int(s[t0:t0 + n, i0:i1, j0:j1, 0].sum())
    return float(np.float64(total) / np.float64(n * (i1 - i0) * (j1 - j0) * CELL * CELL))


def patch_table_select(rng, B: int, G: int, n: int, shape: Tuple[int, int], patch, S: int, augment: bool = True,
                       transpose: Optional[bool] = None, cuts=None, stats=None, act_min: Optional[float] = None, tries: int = 8):
    """`patch_table` with two rules on top -> (table int32 [B',4], scores float64 [B'], tried int32 [B']).  Pure host code.
        cuts     bool [G-1] (`cell_cuts`): pair p set means frames p and p + 1 belong to two shots.  valid = the t0 of range(G - n + 1) with
                 no set pair among cuts[t0 : t0 + n - 1]; all of them without `cuts`.  No valid t0: B' = 0 and NOTHING is drawn from `rng`.
        act_min  with `stats` (the map of `cell_stats`, on the host): a candidate qualifies where `patch_score` >= act_min.
    A candidate is drawn exactly as a row of `patch_table`, in its order: flags (if `augment`), t0 = valid[rng.randint(len(valid))], y0,
    x0.  Without `act_min` the first candidate is the row (score NaN, tried 1).  With it, up to `tries` candidates are drawn: the first
    that qualifies is the row (tried = its number, from 1); if none does, the one with the largest score, the first among equals
    (tried = tries).  The draw order is part of the contract: with no cut set and no `act_min`, the table AND the state of `rng`
    afterwards are `patch_table`'s for the same seed.  B' is B or 0."""
    Ph, Pw = _patch_shape(patch)
    H, W = int(shape[0]), int(shape[1])
    B, G, n, S, tries = int(B), int(G), int(n), int(S), int(tries)
    if B <= 0 or n <= 0 or G < n:
        raise ValueError(f"need B > 0 and 0 < n <= G, got B {B}, n {n}, G {G}")
    if S <= 0 or Ph <= 0 or Pw <= 0 or Ph % S or Pw % S:
        raise ValueError(f"the patch of {Ph} x {Pw} must be a positive multiple of S = {S}")
    may_transpose = (Ph == Pw) if transpose is None else bool(transpose)
    if Ph > H or Pw > W or (may_transpose and (Pw > H or Ph > W)):
        raise ValueError(f"the patch of {Ph} x {Pw} does not fit the frames of {H} x {W}")
    if tries < 1:
        raise ValueError(f"tries must be at least 1, got {tries}")
    if act_min is not None:
        if stats is None:
            raise ValueError("act_min needs stats (the map of cell_stats)")
        stats = _stats_array(stats)
        if stats.shape[0] != G or tuple(stats.shape[1:3]) != cell_shape((H, W)):
            raise ValueError(f"the map {tuple(stats.shape)} is not that of {G} frames of {H} x {W}")
        act_min = float(act_min)
    valid = list(range(G - n + 1))
    if cuts is not None:
        c = np.asarray(cuts, dtype=bool).reshape(-1)
        if c.size != G - 1:
            raise ValueError(f"cuts must hold the G - 1 = {G - 1} pairs of the group, got {c.size}")
        valid = [t0 for t0 in valid if not c[t0:t0 + n - 1].any()]
    if not valid:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32)

    def draw():
        flags = int(rng.randint(16)) if augment else 0
        if not may_transpose:
            flags &= ~PATCH_FLAGS["transpose"]
        ch, cw = (Pw, Ph) if flags & PATCH_FLAGS["transpose"] else (Ph, Pw)
        t0 = valid[int(rng.randint(len(valid)))]
        y0 = int(rng.randint((H - ch) // S + 1)) * S
        x0 = int(rng.randint((W - cw) // S + 1)) * S
        return (t0, y0, x0, flags)

    table = np.empty((B, 4), dtype=np.int32)
    scores, tried = np.full(B, np.nan, dtype=np.float64), np.ones(B, dtype=np.int32)
    for b in range(B):
        if act_min is None:
            table[b] = draw()
            continue
        best = None
        for k in range(1, tries + 1):
            row = draw()
            score = patch_score(stats, row, n, (Ph, Pw))
            if best is None or score > best[1]:
                best = (row, score)
            if score >= act_min:
                best = (row, score)
                break
        table[b], scores[b], tried[b] = best[0], best[1], k
    return table, scores, tried
