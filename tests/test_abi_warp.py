"""CPU-side checks of libvsr_hip_warp.so (include/vsr_hip_warp.h): the temporal warping error is a library of its own, built for gfx950 by
the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry
validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

import _warp_ref as R
from video_super_resolution_amd import _lib

ENTRIES = ["vsr_warp_abi_version", "vsr_warp_error", "vsr_warp_last_error", "vsr_warp_ws_bytes"]
RGB, Y = 0, 1
F32, F16 = 0, 1


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_warp_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.WARPLIB_PATH) and os.path.exists(_lib.WARPHEADER_PATH)
    assert _lib._SIDE["warp"][:2] == (_lib.WARPLIB_PATH, _lib.WARPHEADER_PATH)
    declared = _lib.declared_symbols(warp=True)
    assert declared == ENTRIES
    assert _exported(_lib.WARPLIB_PATH) == declared
    wlib = _lib.load_warp()
    assert wlib.vsr_warp_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.WARPLIB_PATH], capture_output=True, text=True).stdout
    # the constants the tests are written in are the header's
    with open(_lib.WARPHEADER_PATH) as f:
        defs = dict(re.findall(r"#define (VSR_WARP_[A-Z_0-9]+) (\d+)", f.read()))
    assert (int(defs["VSR_WARP_TILE_W"]), int(defs["VSR_WARP_TILE_H"]), int(defs["VSR_WARP_FINISH_THREADS"])) == \
        (R.TILE_W, R.TILE_H, R.FINISH_THREADS)
    assert (int(defs["VSR_WARP_RGB"]), int(defs["VSR_WARP_Y"]), int(defs["VSR_WARP_FLOW_F32"]), int(defs["VSR_WARP_FLOW_F16"])) == (RGB, Y, F32, F16)


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, wdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(warp=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(metric=True) == ["vsr_metric_abi_version", "vsr_metric_frames", "vsr_metric_last_error", "vsr_metric_ws_bytes"]
    assert not set(wdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "warp"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_warp_")], path
    assert not set(_exported(_lib.WARPLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "warp":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.WARPLIB_PATH)) & set(_exported(row[0])), name


def test_warp_entry_validates_before_any_launch():
    M = _lib.load_warp()
    null, fake, off4, off2, off1 = (ctypes.c_void_p(v) for v in (0, 0x1000, 0x1004, 0x1002, 0x1001))
    luma = (ctypes.c_float * 4)(0.25, 0.5, 0.25, 0.0)     # the two pointers the entry reads on the host
    occ = (ctypes.c_double * 4)(*R.OCC)

    def msg():
        return M.vsr_warp_last_error()

    def call(a=fake, b=fake, P=1, H=70, W=75, y0=3, x0=5, h=64, w=64, fwd=fake, bwd=fake, flow_type=F32, pair=2 * 64 * 64, chan=64 * 64, pix=1,
             channels=RGB, quantise=1, shave=0, luma4=luma, occ=occ, sums=fake, ws=fake):
        return M.vsr_warp_error(a, b, P, H, W, y0, x0, h, w, fwd, bwd, flow_type, pair, chan, pix, channels, quantise, shave, luma4, occ,
                                sums, ws, null)

    # null pointers, each kind with its message
    for kw in ({"a": null}, {"b": null}, {"fwd": null}, {"bwd": null}, {"sums": null}, {"ws": null}):
        assert call(**kw) == -1 and b"warp_error: null pointer" in msg(), kw
    assert call(occ=null) == -1 and b"warp_error: null occ" in msg()
    assert call(luma4=null, channels=Y) == -1 and b"null luma4 in Y mode" in msg()
    assert call(luma4=null, shave=32) == -1 and b"bad shave" in msg()        # RGB needs no luma4: refused only further on
    # enums
    for ft in (2, -1):
        assert call(flow_type=ft) == -1 and b"unknown flow_type %d" % ft in msg()
    for ch in (2, -1):
        assert call(channels=ch) == -1 and b"unknown channels %d" % ch in msg()
    assert call(quantise=2) == -1 and b"quantise must be 0 or 1, got 2" in msg()
    # shapes, the crop and the shave
    for kw in ({"P": 0}, {"h": 0}, {"w": -3}, {"P": -1}, {"H": 0}, {"W": -1}):
        assert call(**kw) == -1 and b"bad shape" in msg(), kw
    for kw in ({"y0": -1}, {"x0": -1}, {"y0": 7}, {"x0": 12}, {"h": 68}, {"w": 71}):
        assert call(**kw) == -1 and b"leaves the frame of 70 x 75" in msg(), kw
    assert call(shave=-1) == -1 and b"bad shave -1" in msg()
    assert call(shave=32) == -1 and b"bad shave 32 for a crop of 64 x 64" in msg()           # 2 * shave == min(h, w)
    assert call(h=40, w=20, shave=10) == -1 and b"bad shave 10 for a crop of 40 x 20" in msg()
    # the limits of the launch geometry
    for kw in ({"P": 65536}, {"H": 65536}, {"W": 65536}, {"H": 70000, "h": 65536}, {"W": 70000, "w": 65536}):
        assert call(**kw) == -1 and b"grid overflow" in msg() and b"beyond 65535" in msg(), kw
    # flow strides
    for kw in ({"pair": -1}, {"chan": 0}, {"pix": 0}, {"pix": -32}):
        assert call(**kw) == -1 and b"bad flow strides" in msg(), kw
    # alignment: 4 bytes for the frames, the element for the flows, 8 for the sums and the workspace
    assert call(a=off2) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(b=off1) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(fwd=off2) == -1 and b"flows must be aligned to their element (4 bytes)" in msg()
    assert call(bwd=off1, flow_type=F16) == -1 and b"flows must be aligned to their element (2 bytes)" in msg()
    assert call(sums=off4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    assert call(ws=off4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()

    # the workspace: two doubles per tile of TILE_W x TILE_H scored pixels and pair; 0 for what the call would refuse
    ws = M.vsr_warp_ws_bytes
    assert ws(1, 1, 1, 0) == 16 and ws(3, 16, 64, 0) == 3 * 16 and ws(1, 17, 65, 0) == 4 * 16 and ws(1, 18, 66, 1) == 16
    assert ws(2, 2160, 3840, 4) == 2 * 135 * 60 * 16
    for c in R.CASES:
        assert ws(c.P, c.crop[2], c.crop[3], c.shave) == c.P * R.n_tiles(c) * 16, c.name
    assert ws(0, 64, 64, 0) == 0 and ws(1, 64, 64, 32) == 0 and ws(1, 0, 64, 0) == 0 and ws(1, 64, 64, -1) == 0 and ws(65536, 64, 64, 0) == 0


def test_check_reports_from_the_warp_librarys_own_buffer():
    M = _lib.load_warp()
    fake = ctypes.c_void_p(0x1000)
    occ = (ctypes.c_double * 4)(*R.OCC)
    rc = M.vsr_warp_error(fake, fake, 1, 64, 64, 0, 0, 64, 64, fake, fake, 7, 8192, 4096, 1, 0, 1, 0, None, occ, fake, fake, None)
    with pytest.raises(_lib.VsrHipError, match=r"warp_error failed \(-1\): warp_error: unknown flow_type 7"):
        _lib.check(rc, "warp_error", lib=M)
