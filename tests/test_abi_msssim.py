"""CPU-side checks of libvsr_hip_msssim.so (include/vsr_hip_msssim.h): multi-scale SSIM is a library of its own, built for gfx950 by
the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it (the single-scale
metric library least of all), and the entry validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_msssim_abi_version", "vsr_msssim_frames", "vsr_msssim_last_error", "vsr_msssim_ws_bytes"]
RGB, Y = 0, 1


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_msssim_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.MSSSIMLIB_PATH) and os.path.exists(_lib.MSSSIMHEADER_PATH)
    assert _lib._SIDE["msssim"][:2] == (_lib.MSSSIMLIB_PATH, _lib.MSSSIMHEADER_PATH)
    declared = _lib.declared_symbols(msssim=True)
    assert declared == ENTRIES
    assert _exported(_lib.MSSSIMLIB_PATH) == declared
    mlib = _lib.load_msssim()
    assert mlib.vsr_msssim_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.MSSSIMLIB_PATH], capture_output=True, text=True).stdout


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, mdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(msssim=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(metric=True) == ["vsr_metric_abi_version", "vsr_metric_frames", "vsr_metric_last_error", "vsr_metric_ws_bytes"]
    assert not set(mdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "msssim"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_msssim_")], path
    # ... and the new library defines none of theirs (its own version / error entries, no second vsr_last_error)
    assert not set(_exported(_lib.MSSSIMLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "msssim":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.MSSSIMLIB_PATH)) & set(_exported(row[0])), name


def test_msssim_entry_validates_before_any_launch():
    M = _lib.load_msssim()
    null, fake, off4, off2 = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1002)
    luma = (ctypes.c_float * 4)(0.25, 0.5, 0.25, 0.0)     # the two pointers the entry reads on the host
    win = (ctypes.c_double * 11)(*([1.0 / 11] * 11))

    def msg():
        return M.vsr_msssim_last_error()

    def call(a=fake, b=fake, F=1, H=192, W=256, channels=RGB, quantise=1, shave=0, luma4=luma, win11=win, sums=fake, ws=fake):
        return M.vsr_msssim_frames(a, b, F, H, W, channels, quantise, shave, luma4, win11, sums, ws, null)

    # null pointers, each kind with its message
    for kw in ({"a": null}, {"b": null}, {"sums": null}, {"ws": null}):
        assert call(**kw) == -1 and b"msssim_frames: null pointer" in msg(), kw
    assert call(win11=null) == -1 and b"null win11" in msg()
    assert call(luma4=null, channels=Y) == -1 and b"null luma4 in Y mode" in msg()
    # channels, quantise
    for ch in (2, -1):
        assert call(channels=ch) == -1 and b"unknown channels %d" % ch in msg()
    for q in (2, -1):
        assert call(quantise=q) == -1 and b"quantise must be 0 or 1, got %d" % q in msg()
    # shapes, the shave and the five levels
    for kw in ({"F": 0}, {"H": 0}, {"W": -3}, {"F": -1}):
        assert call(**kw) == -1 and b"bad shape" in msg(), kw
    assert call(shave=-1) == -1 and b"bad shave -1" in msg()
    assert call(H=160, W=400) == -1 and b"five levels need 161 pixels each way after the shave, got 160" in msg()
    assert call(H=400, W=168, shave=4) == -1 and b"five levels need 161 pixels each way after the shave, got 160" in msg()
    assert call(H=192, W=256, shave=200) == -1 and b"five levels need 161 pixels each way after the shave, got -208" in msg()
    # the limits of the launch geometry: grid.z (F), grid.y (from H); W with them
    for kw in ({"F": 65536}, {"H": 65536}, {"W": 65536}):
        assert call(**kw) == -1 and b"grid overflow" in msg() and b"beyond 65535" in msg(), kw
    # alignment: 4 bytes for the frames, 8 for the sums and the workspace
    assert call(a=off2) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(b=ctypes.c_void_p(0x1001)) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(sums=off4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    assert call(ws=off4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    # RGB needs no luma: refused only further on (here: for the size)
    assert call(luma4=null, H=100) == -1 and b"five levels need" in msg()

    # the workspace: per frame and plane, both frames' pooled planes of levels 2 to 5 as doubles and two doubles per scoring tile of
    # 64 x 64 map positions (the tiles of all five levels); 0 for what the call would refuse
    def want(F, h, w, P):
        pooled = tiles = 0
        for j in range(5):
            if j:
                pooled += h * w
            tiles += -(-(h - 10) // 64) * -(-(w - 10) // 64)
            h, w = (h + 1) // 2, (w + 1) // 2
        return F * P * (2 * pooled + 2 * tiles) * 8

    ws = M.vsr_msssim_ws_bytes
    assert ws(1, 161, 161, 0, Y) == want(1, 161, 161, 1) == (2 * (81 * 81 + 41 * 41 + 21 * 21 + 11 * 11) + 2 * (9 + 4 + 1 + 1 + 1)) * 8
    assert ws(2, 176, 208, 0, RGB) == want(2, 176, 208, 3) and ws(1, 189, 211, 4, RGB) == want(1, 181, 203, 3)
    assert ws(3, 2160, 3840, 4, RGB) == want(3, 2152, 3832, 3) and ws(3, 2160, 3840, 4, Y) == want(3, 2152, 3832, 1)
    assert ws(1, 160, 400, 0, RGB) == 0 and ws(0, 192, 256, 0, RGB) == 0 and ws(1, 192, 256, 16, Y) == 0 and ws(1, 192, 256, 0, 2) == 0
    assert ws(1, 192, 256, -1, Y) == 0 and ws(65536, 192, 256, 0, Y) == 0


def test_check_reports_from_the_msssim_librarys_own_buffer():
    M = _lib.load_msssim()
    fake = ctypes.c_void_p(0x1000)
    rc = M.vsr_msssim_frames(fake, fake, 1, 192, 256, 7, 1, 0, None, fake, fake, fake, None)
    with pytest.raises(_lib.VsrHipError, match=r"msssim_frames failed \(-1\): msssim_frames: unknown channels 7"):
        _lib.check(rc, "msssim_frames", lib=M)
