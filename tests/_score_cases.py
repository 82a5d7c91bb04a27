"""The inputs the device scoring tests share (tests/test_gpu_metric.py, tests/test_gpu_msssim.py, tests/test_gpu_score_bits.py) and the
cases whose float64 bits tests/golden/g13_score_bits.json pins (recorded by tools/record_score_bits.py).

A shape is (F, H, W, shave, offset flag); an image pair is made once per (kind, shape), seeded by the shape and the kind alone."""
import functools
import hashlib

import numpy as np
import torch

import _metric_ref as R
from video_super_resolution_amd import driver

IMAGES = {"textured": R.textured, "near_flat": R.near_flat, "gaussian": R.gaussian, "awkward": R.awkward,
          "awkward_no_nan": functools.partial(R.awkward, nan=False)}
MODES = [(ch, q) for ch in ("rgb", "y") for q in (0, 1)]


def _ids(v):
    return "x".join(str(int(i)) for i in v) if isinstance(v, tuple) else str(v)   # (a shape; other parameters are plain values)


def _luma4():
    c = driver.yuv_coefficients("yuv420p", "bt601", False)
    return np.array([c[0], c[1], c[2], c[9]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def images(kind, shape):
    """A pair of float32 [F,H,W,3] arrays, made once per (kind, shape) and never modified."""
    F, H, W, shave, _ = shape
    a, b = IMAGES[kind](np.random.RandomState(H * 131 + W + len(kind)), F, H, W)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def to_device(x, offset):
    """The array on the device; `offset`: inside a flat buffer at a storage offset of one float (4 bytes past a 16-byte boundary)."""
    if not offset:
        return torch.tensor(x).cuda()   # (a copy: the cached arrays are read-only)
    buf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    buf[1:1 + x.size] = torch.tensor(x).reshape(-1).cuda()
    view = buf[1:1 + x.size].view(x.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ------------------------------------------------------------------------------------------------ the pinned bits
# the smallest shapes that reach each branch of the march (the docstrings of the two test files say which)
BIT_SHAPES = {"frame_metrics": [(2, 12, 75, 0, False), (1, 23, 140, 3, False), (1, 75, 64, 0, False), (3, 16, 64, 2, False),
                                (2, 16, 64, 2, True)],
              "frame_msssim": [(1, 161, 161, 0, False), (2, 176, 208, 0, False), (1, 189, 211, 4, False)]}
BIT_CASES = [(entry, shape, what, ch, q) for entry, shapes in BIT_SHAPES.items() for shape in shapes
             for what in ((("psnr", "ssim"), "psnr") if entry == "frame_metrics" else (None,)) for ch, q in MODES]


def bit_case_key(entry, shape, what, channels, quant):
    w = "" if what is None else " what=" + ("+".join(what) if isinstance(what, tuple) else what)
    return f"{entry} {_ids(shape[:4])}{' offset' if shape[4] else ''}{w} {channels} q{quant}"


def bit_case(entry, shape, what, channels, quant):
    """One pinned case on the device -> (SHA-256 of the input bytes, the float64 bits of the result as hex strings)."""
    a, b = images("textured" if quant else "gaussian", shape)
    ta, tb = to_device(a, shape[4]), to_device(b, shape[4])
    if entry == "frame_metrics":
        got = driver.frame_metrics(ta, tb, channels, bool(quant), shape[3], what)
    else:
        got = driver.frame_msssim(ta, tb, channels, bool(quant), shape[3])
    bits = np.ascontiguousarray(got.cpu().numpy(), dtype=np.float64).reshape(-1).view(np.uint64)
    return hashlib.sha256(a.tobytes() + b.tobytes()).hexdigest(), [f"{v:016x}" for v in bits.tolist()]
