"""ctypes binding of libvsr_hip.so (the C ABI declared in include/vsr_hip.h), of libvsr_hip_grad.so (include/vsr_hip_grad.h:
the backward of the three native flow operators), of libvsr_hip_s3.so (include/vsr_hip_s3.h: the fused x3 stage of the SR net), of
libvsr_hip_s3t.so (include/vsr_hip_s3t.h: the one-launch x3 tail), of libvsr_hip_s3p.so (include/vsr_hip_s3p.h: the x3 stage with
the next group's uptran slice inside the launch), of libvsr_hip_s3f.so (include/vsr_hip_s3f.h: the x3 stage with the step-opening
1x1 chain in its LR load path), of libvsr_hip_yuv.so (include/vsr_hip_yuv.h: Y'CbCr 4:2:0 frames in and out), of
libvsr_hip_metric.so (include/vsr_hip_metric.h: the float64 sums behind PSNR and SSIM of HR frames), of libvsr_hip_opt.so
(include/vsr_hip_opt.h: the Adam step and the gradient-norm clip of the train step), of libvsr_hip_loss.so (include/vsr_hip_loss.h:
the pixel terms of the training loss), of libvsr_hip_resize.so (include/vsr_hip_resize.h: frames resampled by a separable,
table-driven filter), of libvsr_hip_warp.so (include/vsr_hip_warp.h: the float64 sums behind the temporal warping error of
consecutive HR frames), of libvsr_hip_scene.so (include/vsr_hip_scene.h: scene cuts in a streamed clip, found and handled on the
device), of libvsr_hip_hgi.so (include/vsr_hip_hgi.h: an inception block of the hourglass's inner levels in one launch), of
libvsr_hip_msssim.so (include/vsr_hip_msssim.h: the float64 sums behind multi-scale SSIM of HR frames), of libvsr_hip_pix.so
(include/vsr_hip_pix.h: planar Y'CbCr 4:2:2 and 4:4:4 frames in and out), of libvsr_hip_patch.so (include/vsr_hip_patch.h: training
samples cut and augmented from frames on the device), of libvsr_hip_deint.so (include/vsr_hip_deint.h: motion-adaptive deinterlacing
of packed frames) and of libvsr_hip_cell.so (include/vsr_hip_cell.h: a resident group of frames measured per cell and frame).

There is deliberately no CPU or eager-PyTorch fallback behind these entry points: if the
shared library is missing, or an operator is handed a non-CUDA tensor, the call raises.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "libvsr_hip.so")
XLIB_PATH = os.path.join(_PKG, "libvsr_hip_xcheck.so")
HEADER_PATH = os.path.join(_ROOT, "include", "vsr_hip.h")
XHEADER_PATH = os.path.join(_ROOT, "include", "vsr_hip_xcheck.h")
_lib = None
_xlib = None


def _side(name: str, prefix: str, abi: int, has_query: bool) -> tuple:
    return (os.path.join(_PKG, f"libvsr_hip_{name}.so"), os.path.join(_ROOT, "include", f"vsr_hip_{name}.h"), prefix, abi, has_query)


# the side libraries, each with a version entry and an error buffer of its own: (library, header, symbol prefix, ABI version, has a
# `<prefix>_query`).  grad: the backward kernels of Resample2d, ChannelNorm and Correlation; s3: the fused FeedbackBlock stage of the x3
# geometry (csrc/sr_utd_s3.hip); s3t: the one-launch x3 tail (csrc/sr_tail_s3.hip); s3p: the x3 stage with the next group's uptran slice
# inside the launch (csrc/sr_utd_s3p.hip); s3f: the x3 stage with the step-opening 1x1 chain in its LR load path (csrc/sr_utd_s3f.hip);
# yuv: Y'CbCr 4:2:0 frames to the model's float32 RGB and back (csrc/clip_yuv.hip); metric: the float64 sums behind PSNR and SSIM of HR
# frames against ground truth (csrc/frame_metric.hip); opt: Adam over a plan of tensors in one launch, the gradient norm and its clip
# coefficient in two (csrc/train_update.hip); loss: object masking, image SSEs, TV sums and the NHWC-4 half VGG inputs of the training loss
# in one launch and a finish (csrc/loss_terms.hip); resize: float32 RGB frames resampled by a separable filter given as tables, both passes
# in one launch (csrc/frame_resize.hip); warp: frame t + 1 warped back onto frame t along a flow, the squared difference summed over the
# pixels that are not occluded (csrc/frame_warp_error.hip); scene: the absolute luma difference of consecutive LR frames summed per pair,
# the cut rule on the sums, and the window and fed-back estimate composed under the rule's flags (csrc/clip_scene.hip); hgi: an inception
# block of the depth hourglass's inner levels (four 1x1s, three k x k) in one launch, the mid maps in LDS (csrc/conv_hg_inception.hip);
# msssim: the float64 sums behind multi-scale SSIM of HR frames against ground truth, five levels in three launches (csrc/frame_msssim.hip);
# pix: planar Y'CbCr 4:2:2 and 4:4:4 frames to the model's float32 RGB and back (csrc/clip_pix.hip); patch: runs of HR frames cropped,
# flipped, transposed and reversed in time into training samples, with their LR patches, in one launch (csrc/train_patch.hip); deint: the
# rows of one field of a packed interlaced frame kept, the rows of the other rebuilt from the fields either side in time, all planes in one
# launch (csrc/clip_deint.hip); cell: the spatial activity of every 16 x 16 cell of every frame of a resident group and its absolute luma
# difference against the frame before, in one launch that reads each frame once (csrc/clip_cell_stats.hip)
_SIDE = {"grad": _side("grad", "vsr_grad", 1, False), "s3": _side("s3", "vsr_s3", 1, True), "s3t": _side("s3t", "vsr_s3t", 1, True),
         "s3p": _side("s3p", "vsr_s3p", 1, True), "s3f": _side("s3f", "vsr_s3f", 1, True), "yuv": _side("yuv", "vsr_yuv", 1, False),
         "metric": _side("metric", "vsr_metric", 1, False), "opt": _side("opt", "vsr_opt", 1, False), "loss": _side("loss", "vsr_loss", 1, False),
         "resize": _side("resize", "vsr_resize", 1, False), "warp": _side("warp", "vsr_warp", 1, False),
         "scene": _side("scene", "vsr_scene", 1, False), "hgi": _side("hgi", "vsr_hgi", 1, False),
         "msssim": _side("msssim", "vsr_msssim", 1, False), "pix": _side("pix", "vsr_pix", 1, False),
         "patch": _side("patch", "vsr_patch", 1, False), "deint": _side("deint", "vsr_deint", 1, False),
         "cell": _side("cell", "vsr_cell", 1, False)}
(GLIB_PATH, GHEADER_PATH), (S3LIB_PATH, S3HEADER_PATH), (S3TLIB_PATH, S3THEADER_PATH), (S3PLIB_PATH, S3PHEADER_PATH), \
    (S3FLIB_PATH, S3FHEADER_PATH), (YUVLIB_PATH, YUVHEADER_PATH), (METRICLIB_PATH, METRICHEADER_PATH), (OPTLIB_PATH, OPTHEADER_PATH), \
    (LOSSLIB_PATH, LOSSHEADER_PATH), (RESIZELIB_PATH, RESIZEHEADER_PATH), (WARPLIB_PATH, WARPHEADER_PATH), (SCENELIB_PATH, SCENEHEADER_PATH), \
    (HGILIB_PATH, HGIHEADER_PATH), (MSSSIMLIB_PATH, MSSSIMHEADER_PATH), (PIXLIB_PATH, PIXHEADER_PATH), (PATCHLIB_PATH, PATCHHEADER_PATH), \
    (DEINTLIB_PATH, DEINTHEADER_PATH), (CELLLIB_PATH, CELLHEADER_PATH) = (row[:2] for row in _SIDE.values())
_gradlib = _s3lib = _s3tlib = _s3plib = _s3flib = _yuvlib = _metriclib = _optlib = _losslib = _resizelib = _warplib = _scenelib = _hgilib = _msssimlib = _pixlib = _patchlib = _deintlib = _celllib = None   # `_<name>lib`: the loaded side library (None: this process has not asked for it)
# the cross-check library instead of the shipping one for every call (set by `xcheck()`; the environment switch serves the
# measurement tools, whose VSR_TUNING codes only that library understands)
_use_x = os.environ.get("VSR_USE_XCHECK", "0") == "1" or bool(os.environ.get("VSR_TUNING", "").strip())


class VsrHipError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into the in-tree libvsr_hip.so, libvsr_hip_xcheck.so, libvsr_hip_grad.so,
    libvsr_hip_s3.so, libvsr_hip_s3t.so, libvsr_hip_s3p.so, libvsr_hip_s3f.so, libvsr_hip_yuv.so, libvsr_hip_metric.so,
    libvsr_hip_opt.so, libvsr_hip_loss.so, libvsr_hip_resize.so, libvsr_hip_warp.so, libvsr_hip_scene.so, libvsr_hip_hgi.so,
    libvsr_hip_msssim.so, libvsr_hip_pix.so, libvsr_hip_patch.so, libvsr_hip_deint.so and libvsr_hip_cell.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-j4", "-C", os.path.join(_PKG, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def declared_symbols(xcheck: bool = False, grad: bool = False, s3: bool = False, s3t: bool = False, s3p: bool = False, s3f: bool = False,
                     yuv: bool = False, metric: bool = False, opt: bool = False, loss: bool = False, resize: bool = False,
                     warp: bool = False, scene: bool = False, hgi: bool = False, msssim: bool = False, pix: bool = False,
                     patch: bool = False, deint: bool = False, cell: bool = False) -> list:
    """Entry points include/vsr_hip.h declares (xcheck: the ones include/vsr_hip_xcheck.h adds; grad / s3 / s3t / s3p / s3f / yuv / metric /
    opt / loss / resize / warp / scene / hgi / msssim / pix / patch / deint / cell: the ones of include/vsr_hip_grad.h / include/vsr_hip_s3.h / include/vsr_hip_s3t.h / include/vsr_hip_s3p.h / include/vsr_hip_s3f.h /
    include/vsr_hip_yuv.h / include/vsr_hip_metric.h / include/vsr_hip_opt.h / include/vsr_hip_loss.h / include/vsr_hip_resize.h /
    include/vsr_hip_warp.h / include/vsr_hip_scene.h / include/vsr_hip_hgi.h / include/vsr_hip_msssim.h / include/vsr_hip_pix.h / include/vsr_hip_patch.h /
    include/vsr_hip_deint.h / include/vsr_hip_cell.h, libraries of their own)."""
    side = [name for name, on in (("grad", grad), ("s3", s3), ("s3t", s3t), ("s3p", s3p), ("s3f", s3f), ("yuv", yuv), ("metric", metric),
                                  ("opt", opt), ("loss", loss), ("resize", resize), ("warp", warp), ("scene", scene), ("hgi", hgi),
                                  ("msssim", msssim), ("pix", pix), ("patch", patch), ("deint", deint), ("cell", cell)) if on]
    with open(_SIDE[side[-1]][1] if side else XHEADER_PATH if xcheck else HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", text)))


def _dlopen(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise VsrHipError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the device path)")
    return ctypes.CDLL(path)


def _open(path: str) -> ctypes.CDLL:
    lib = _dlopen(path)
    lib.vsr_last_error.restype = ctypes.c_char_p
    lib.vsr_last_route.restype = ctypes.c_char_p
    for fn in ("vsr_sr_query", "vsr_train_corr_dw_ws_floats", "vsr_train_prelu_bwd_ws_floats"):
        getattr(lib, fn).restype = ctypes.c_size_t
    if lib.vsr_abi_version() != 3:
        raise VsrHipError(f"{os.path.basename(path)}: ABI version mismatch")
    return lib


def load_xcheck() -> ctypes.CDLL:
    """libvsr_hip_xcheck.so (include/vsr_hip_xcheck.h): the shipping entry points + the superseded builds, switches and stamped
    diagnostics.  For tests and tools; the package calls it only from code paths that exist for the tests."""
    global _xlib
    if _xlib is None:
        lib = _open(XLIB_PATH)
        for t in os.environ.get("VSR_TUNING", "").split(","):   # measurement hook: kernel-selection switches (vsr_conv2d_tuning codes)
            if t.strip():
                lib.vsr_conv2d_tuning(int(t))
        _xlib = lib
    return _xlib


def _load_side(name: str) -> ctypes.CDLL:
    """The side library `name` of `_SIDE`, opened once.  Its own error buffer: `check(rc, what, lib=load_<name>())`."""
    cache = f"_{name}lib"
    if globals()[cache] is None:
        path, _, prefix, abi, has_query = _SIDE[name]
        lib = _dlopen(path)
        getattr(lib, prefix + "_last_error").restype = ctypes.c_char_p
        lib.vsr_last_error = getattr(lib, prefix + "_last_error")   # the name `check` reads a library's message under
        if has_query:
            getattr(lib, prefix + "_query").restype = ctypes.c_size_t
        if getattr(lib, prefix + "_abi_version")() != abi:
            raise VsrHipError(f"{os.path.basename(path)}: ABI version mismatch")
        globals()[cache] = lib
    return globals()[cache]


def load_grad() -> ctypes.CDLL:
    """libvsr_hip_grad.so (include/vsr_hip_grad.h)."""
    return _load_side("grad")


def load_s3() -> ctypes.CDLL:
    """libvsr_hip_s3.so (include/vsr_hip_s3.h)."""
    return _load_side("s3")


def load_s3t() -> ctypes.CDLL:
    """libvsr_hip_s3t.so (include/vsr_hip_s3t.h)."""
    return _load_side("s3t")


def load_s3p() -> ctypes.CDLL:
    """libvsr_hip_s3p.so (include/vsr_hip_s3p.h)."""
    return _load_side("s3p")


def load_s3f() -> ctypes.CDLL:
    """libvsr_hip_s3f.so (include/vsr_hip_s3f.h)."""
    return _load_side("s3f")


def load_yuv() -> ctypes.CDLL:
    """libvsr_hip_yuv.so (include/vsr_hip_yuv.h)."""
    return _load_side("yuv")


def load_metric() -> ctypes.CDLL:
    """libvsr_hip_metric.so (include/vsr_hip_metric.h)."""
    lib = _load_side("metric")
    lib.vsr_metric_ws_bytes.restype = ctypes.c_size_t
    return lib


class OptTensor(ctypes.Structure):
    """vsr_opt_tensor_t of include/vsr_hip_opt.h (all pointers as integers)."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_ulonglong)]


def load_opt() -> ctypes.CDLL:
    """libvsr_hip_opt.so (include/vsr_hip_opt.h)."""
    lib = _load_side("opt")
    lib.vsr_opt_plan_bytes.restype = lib.vsr_opt_norm_ws_bytes.restype = ctypes.c_size_t
    lib.vsr_opt_plan_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.vsr_opt_plan_fill.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(OptTensor)]
    lib.vsr_opt_norm_ws_bytes.argtypes = [ctypes.c_void_p]
    lib.vsr_opt_adam_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_float] * 7 + [ctypes.c_void_p]
    lib.vsr_opt_grad_norm.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def load_loss() -> ctypes.CDLL:
    """libvsr_hip_loss.so (include/vsr_hip_loss.h)."""
    lib = _load_side("loss")
    lib.vsr_loss_ws_bytes.restype = ctypes.c_size_t
    lib.vsr_loss_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.vsr_loss_pixel_terms.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6
    return lib


def load_resize() -> ctypes.CDLL:
    """libvsr_hip_resize.so (include/vsr_hip_resize.h)."""
    lib = _load_side("resize")
    lib.vsr_resize_frames.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] * 2 + \
        [ctypes.c_int, ctypes.c_void_p]
    return lib


def load_warp() -> ctypes.CDLL:
    """libvsr_hip_warp.so (include/vsr_hip_warp.h)."""
    lib = _load_side("warp")
    lib.vsr_warp_ws_bytes.restype = ctypes.c_size_t
    lib.vsr_warp_ws_bytes.argtypes = [ctypes.c_int] * 4
    lib.vsr_warp_error.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_longlong] * 3 + \
        [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    return lib


def load_scene() -> ctypes.CDLL:
    """libvsr_hip_scene.so (include/vsr_hip_scene.h)."""
    lib = _load_side("scene")
    lib.vsr_scene_ws_bytes.restype = ctypes.c_size_t
    lib.vsr_scene_ws_bytes.argtypes = [ctypes.c_int] * 3
    lib.vsr_scene_pair_sums.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    lib.vsr_scene_decide.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.vsr_scene_window.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    return lib


def load_hgi() -> ctypes.CDLL:
    """libvsr_hip_hgi.so (include/vsr_hip_hgi.h)."""
    lib = _load_side("hgi")
    lib.vsr_hgi_workgroups.restype = ctypes.c_longlong
    lib.vsr_hgi_inception_f16.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] * 3 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return lib


def load_msssim() -> ctypes.CDLL:
    """libvsr_hip_msssim.so (include/vsr_hip_msssim.h)."""
    lib = _load_side("msssim")
    lib.vsr_msssim_ws_bytes.restype = ctypes.c_size_t
    lib.vsr_msssim_ws_bytes.argtypes = [ctypes.c_int] * 5
    lib.vsr_msssim_frames.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 5
    return lib


def load_pix() -> ctypes.CDLL:
    """libvsr_hip_pix.so (include/vsr_hip_pix.h)."""
    return _load_side("pix")


def load_patch() -> ctypes.CDLL:
    """libvsr_hip_patch.so (include/vsr_hip_patch.h)."""
    lib = _load_side("patch")
    lib.vsr_patch_gather.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + \
        [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    return lib


class DeintPlane(ctypes.Structure):
    """vsr_deint_plane of include/vsr_hip_deint.h."""
    _fields_ = [("offset", ctypes.c_size_t), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("comps", ctypes.c_int)]


def load_deint() -> ctypes.CDLL:
    """libvsr_hip_deint.so (include/vsr_hip_deint.h)."""
    lib = _load_side("deint")
    lib.vsr_deint_frame.argtypes = [ctypes.c_void_p] * 4 + [ctypes.POINTER(DeintPlane)] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def load_cell() -> ctypes.CDLL:
    """libvsr_hip_cell.so (include/vsr_hip_cell.h)."""
    lib = _load_side("cell")
    lib.vsr_cell_stats.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    return lib


def load() -> ctypes.CDLL:
    """The library every product call goes through: libvsr_hip.so, unless a test / tool asked for the cross-check library."""
    global _lib
    if _use_x:
        return load_xcheck()
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


class xcheck:
    """`with _lib.xcheck():` -- every `load()` inside returns the cross-check library (so a switch set through it reaches the
    kernels the package's classes launch)."""

    def __enter__(self):
        global _use_x
        self._old, _use_x = _use_x, True
        return load_xcheck()

    def __exit__(self, *exc):
        global _use_x
        _use_x = self._old
        return False


# vsr_sr_query codes (include/vsr_hip.h)
Q_UTD_BLOB_BYTES, Q_UTD_STRIP_WIDTH, Q_UTD_S2_BLOB_BYTES, Q_UTD_S2_STRIP_WIDTH, Q_TAIL_S2_BLOB_BYTES = range(5)
# vsr_s3_query codes (include/vsr_hip_s3.h)
Q_S3_BLOB_BYTES, Q_S3_STRIP_WIDTH = range(2)
# vsr_s3t_query codes (include/vsr_hip_s3t.h)
Q_S3T_BLOB_BYTES, Q_S3T_BLOB_FOLD_BYTES, Q_S3T_STRIP_WIDTH = range(3)
# vsr_s3p_query codes (include/vsr_hip_s3p.h)
Q_S3P_BLOB_BYTES, Q_S3P_STRIP_WIDTH = range(2)
# vsr_s3f_query codes (include/vsr_hip_s3f.h)
Q_S3F_BLOB_BYTES, Q_S3F_STRIP_WIDTH = range(2)


def check(rc: int, what: str = "", lib=None) -> None:
    """`lib`: the library that made the call (each has its own error buffer); by default the text of every loaded library is
    shown, the one `load()` returns first (a call site that went through `load_xcheck()` directly is then still reported)."""
    if rc != 0:
        libs = [lib] if lib is not None else [l for l in (load(), _lib, _xlib) if l is not None]
        msgs = []
        for l in libs:
            m = l.vsr_last_error().decode("utf-8", "replace")
            if m and m not in msgs:
                msgs.append(m)
        raise VsrHipError(f"{what or 'vsr'} failed ({rc}): {' | '.join(msgs)}")


def dptr(t: torch.Tensor, dtype=torch.float32) -> ctypes.c_void_p:
    """Device pointer of a dense tensor; refuses anything the kernels' indexing does not assume."""
    if not t.is_cuda:
        raise VsrHipError("device path called with a CPU tensor (no CPU fallback exists)")
    if t.dtype != dtype:
        raise VsrHipError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise VsrHipError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def optr(t, dtype=torch.float32):
    return ctypes.c_void_p(0) if t is None else dptr(t, dtype)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def raw_stream(index=None) -> int:
    """Handle of the current stream of device `index` (default: the current device) as an integer.  A forward issues ~900 launches and
    as many buffer look-ups keyed by the stream: `torch.cuda.current_stream()` builds a Stream object per call (~6 us of host time each),
    the raw accessor does not."""
    if _raw_stream is not None:
        return _raw_stream(torch._C._cuda_getDevice() if index is None else index)
    return torch.cuda.current_stream(index).cuda_stream


def stream() -> ctypes.c_void_p:
    """The current stream of the CURRENT device: entry points make the tensors' device current first (`on_device`)."""
    return ctypes.c_void_p(raw_stream())


def _first_cuda_tensor(objs):
    for o in objs:
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                return o
        elif isinstance(o, (list, tuple)):
            t = _first_cuda_tensor(o)
            if t is not None:
                return t
    return None


def on_device(fn):
    """Run `fn` with the device of its first CUDA tensor argument made current: kernels are launched on the current
    device's current stream and the >64 KB LDS attribute is kept per device, so a module living on cuda:1 must not launch
    while cuda:0 is current.  No-op (no context switch) when that device is current already."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        t = _first_cuda_tensor(args)
        if t is None:
            t = _first_cuda_tensor(tuple(kwargs.values()))
        if t is None or t.device.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return wrapped


def cf(v: float) -> ctypes.c_float:
    return ctypes.c_float(float(v))


class _ChainStage(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p * 2), ("w", ctypes.c_void_p * 2), ("ldw", ctypes.c_int * 2), ("w_prev", ctypes.c_void_p),
                ("ldw_prev", ctypes.c_int), ("bias", ctypes.c_void_p), ("cmap", ctypes.c_void_p), ("slope", ctypes.c_float),
                ("out", ctypes.c_void_p)]


class Chain1x1(ctypes.Structure):
    """vsr_chain1x1_t of include/vsr_hip.h (all pointers as integers)."""
    _fields_ = [("nstages", ctypes.c_int), ("stage", _ChainStage * 3)]


_ROUTE_BATCH = os.environ.get("VSR_ROUTE_BATCH", "1") != "0"   # (A/B switch: 0 = every launcher follows the batch it is handed, as before round 5)


class route_batch:
    """`with _lib.route_batch(num, den):` -- the convolution launchers inside choose kernel / tile width / split-K as if their batch N
    were N * num / den (vsr_conv2d_route_batch): a trunk evaluated on a part of its usual batch runs the usual kernels.  num == den or
    den <= 0: no-op."""

    def __init__(self, num: int, den: int):
        self.num, self.den = int(num), int(den)
        self.on = self.den > 0 and self.num > 0 and self.num != self.den and _ROUTE_BATCH

    def __enter__(self):
        if self.on:
            check(load().vsr_conv2d_route_batch(self.num, self.den), "conv2d_route_batch")
        return self

    def __exit__(self, *exc):
        if self.on:
            load().vsr_conv2d_route_batch(0, 0)
        return False


class serial_streams:
    """`with _lib.serial_streams():` -- inside, the side streams the forward forks work onto (VSR._side_streams, the hourglass levels',
    FlowNetSD's) ARE the current stream: the same launches with the same values in one stream's order.  GraphedVSR captures a
    single-branch graph this way where the process may not open a hardware queue per branch (graph.py)."""
    on = False

    def __init__(self, enable: bool = True):
        self.enable = bool(enable)

    def __enter__(self):
        self._old, serial_streams.on = serial_streams.on, serial_streams.on or self.enable
        return self

    def __exit__(self, *exc):
        serial_streams.on = self._old
        return False


class EventTimer:
    """HIP-event timing of selected kernel launches on the current stream (used by bench.py for the roofline
    leg).  Disabled (no events, no overhead) unless `enabled` is set."""

    def __init__(self):
        self.enabled = False
        self.only = None   # optional set of names: everything else stays untimed (bench.py times the dominant kernel only)
        self._pairs = {}

    def reset(self):
        self._pairs = {}

    def start(self, name: str):
        if not self.enabled or (self.only is not None and name not in self.only):
            return None
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        self._pairs.setdefault(name, []).append((a, b))
        return b

    @staticmethod
    def stop(tok):
        if tok is not None:
            tok.record()

    def summary(self):
        """{name: (launches, mean milliseconds)} -- call after a device synchronise."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self._pairs.items()}


TIMER = EventTimer()


class RouteLog:
    """Which kernel every convolution launch was routed to (`vsr_last_route`), recorded while `enabled`: the launchers
    pick by layer size, so the full-size parity tests log what actually ran (label -> route -> count)."""

    def __init__(self):
        self.enabled = False
        self.calls = []

    def note(self, label: str):
        if self.enabled:
            self.calls.append((label, load().vsr_last_route().decode()))

    def note_as(self, label: str, route: str):
        """A launch whose route the caller names itself (the stock operator; a suffix on `vsr_last_route`)."""
        if self.enabled:
            self.calls.append((label, route))

    def last(self) -> str:
        return load().vsr_last_route().decode()

    def histogram(self):
        h = {}
        for _, r in self.calls:
            h[r] = h.get(r, 0) + 1
        return h


ROUTES = RouteLog()
