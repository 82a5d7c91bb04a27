"""CPU-side checks of libvsr_hip_resize.so (include/vsr_hip_resize.h): the resampler is a library of its own, built for gfx950 by the
same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry validates its
arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_resize_abi_version", "vsr_resize_frames", "vsr_resize_last_error"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def _define(name):
    with open(_lib.RESIZEHEADER_PATH) as f:
        return int(re.search(rf"#define {name} (\d+)", f.read()).group(1))


def test_resize_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.RESIZELIB_PATH) and os.path.exists(_lib.RESIZEHEADER_PATH)
    assert _lib._SIDE["resize"][:2] == (_lib.RESIZELIB_PATH, _lib.RESIZEHEADER_PATH)
    declared = _lib.declared_symbols(resize=True)
    assert declared == ENTRIES
    assert _exported(_lib.RESIZELIB_PATH) == declared
    rlib = _lib.load_resize()
    assert rlib.vsr_resize_abi_version() == 1 and _lib.load_resize() is rlib
    assert "gfx950" in subprocess.run(["strings", _lib.RESIZELIB_PATH], capture_output=True, text=True).stdout
    assert (_define("VSR_RESIZE_MAX_TAPS"), _define("VSR_RESIZE_ABI_VERSION")) == (33, 1)
    assert _define("VSR_RESIZE_TILE_W") % 4 == 0 and _define("VSR_RESIZE_TILE_H") > 0


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, rdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(resize=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(yuv=True) == ["vsr_yuv_abi_version", "vsr_yuv_ingest", "vsr_yuv_last_error", "vsr_yuv_write"]
    assert _lib.declared_symbols(metric=True) == ["vsr_metric_abi_version", "vsr_metric_frames", "vsr_metric_last_error", "vsr_metric_ws_bytes"]
    assert not set(rdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "resize"]
    for path in others:
        # (libvsr_hip.so has vsr_resize_add_segs_nhwc_f16 and vsr_resize_estimate_f32 of its own, nearest resizers: the names, not the prefix)
        assert not set(_exported(path)) & set(ENTRIES), path
    assert not set(_exported(_lib.RESIZELIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "resize":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.RESIZELIB_PATH)) & set(_exported(row[0])), name


def test_resize_entry_validates_before_any_launch():
    R = _lib.load_resize()
    null, off2 = ctypes.c_void_p(0), ctypes.c_void_p(0x100002)
    src, dst, tab = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000), ctypes.c_void_p(0x1000)
    TH = _define("VSR_RESIZE_TILE_H")

    def msg():
        return R.vsr_resize_last_error()

    def call(src=src, dst=dst, F=1, H=32, W=32, h=8, w=8, xf=tab, xw=tab, KX=17, yf=tab, yw=tab, KY=17, quantise=1):
        return R.vsr_resize_frames(src, dst, F, H, W, h, w, xf, xw, KX, yf, yw, KY, quantise, null)

    for kw in ({"src": null}, {"dst": null}):
        assert call(**kw) == -1 and b"resize_frames: null frame pointer" in msg(), kw
    for kw in ({"xf": null}, {"xw": null}, {"yf": null}, {"yw": null}):
        assert call(**kw) == -1 and b"resize_frames: null table pointer" in msg(), kw
    for kw in ({"F": 0}, {"H": 0}, {"W": -3}, {"h": 0}, {"w": -1}, {"F": -1}):
        assert call(**kw) == -1 and b"bad shape" in msg(), kw
    assert call(W=2147483584) == -1 and b"beyond 2^31 - 65" in msg()
    assert call(H=2147483647) == -1 and b"beyond 2^31 - 65" in msg()
    for k in (0, 34, -1):
        assert call(KX=k) == -1 and b"KX %d outside 1..33" % k in msg()
        assert call(KY=k) == -1 and b"KY %d outside 1..33" % k in msg()
    for q in (2, -1):
        assert call(quantise=q) == -1 and b"quantise must be 0 or 1, got %d" % q in msg()
    # the limits of the launch geometry, each naming its dimension
    assert call(F=65536) == -1 and b"grid overflow (F 65536 beyond 65535: grid dimension z)" in msg()
    assert call(h=65535 * TH + 1, dst=ctypes.c_void_p(1 << 40)) == -1 and b"grid overflow (65536 tiles" in msg() and b"grid dimension y" in msg()
    assert call(F=65535, H=1 << 30, W=1 << 30) == -1 and b"2^62 bytes or more" in msg()
    # alignment: 4 bytes for the frames and for every table
    assert call(src=off2) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(dst=ctypes.c_void_p(0x900001)) == -1 and b"frames must be 4-byte aligned" in msg()
    for name in ("xf", "xw", "yf", "yw"):
        assert call(**{name: ctypes.c_void_p(0x1002)}) == -1 and b"tables must be 4-byte aligned" in msg(), name
    # overlap of the two byte ranges: src is 32 x 32 x 3 floats = 12288 bytes, dst 8 x 8 x 3 floats = 768 bytes
    assert call(dst=src) == -1 and b"src and dst overlap" in msg()
    assert call(dst=ctypes.c_void_p(0x100000 + 12288 - 4)) == -1 and b"src and dst overlap" in msg()
    assert call(dst=ctypes.c_void_p(0x100000 - 768 + 4)) == -1 and b"src and dst overlap" in msg()
    # the order of the checks: a bad shape is reported before alignment
    assert call(src=off2, F=0) == -1 and b"bad shape" in msg()


def test_check_reports_from_the_resize_librarys_own_buffer():
    R = _lib.load_resize()
    fake = ctypes.c_void_p(0x1000)
    rc = R.vsr_resize_frames(fake, fake, 1, 8, 8, 4, 4, fake, fake, 40, fake, fake, 5, 0, None)
    with pytest.raises(_lib.VsrHipError, match=r"resize_frames failed \(-1\): resize_frames: KX 40 outside 1\.\.33"):
        _lib.check(rc, "resize_frames", lib=R)
