"""CPU-side checks of libvsr_hip_scene.so (include/vsr_hip_scene.h): scene-cut detection is a library of its own, built for gfx950 by the
same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and every entry validates
its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

import _scene_ref as R
from video_super_resolution_amd import _lib

ENTRIES = ["vsr_scene_abi_version", "vsr_scene_decide", "vsr_scene_last_error", "vsr_scene_pair_sums", "vsr_scene_window",
           "vsr_scene_ws_bytes"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_scene_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.SCENELIB_PATH) and os.path.exists(_lib.SCENEHEADER_PATH)
    assert _lib._SIDE["scene"][:2] == (_lib.SCENELIB_PATH, _lib.SCENEHEADER_PATH)
    declared = _lib.declared_symbols(scene=True)
    assert declared == ENTRIES
    assert _exported(_lib.SCENELIB_PATH) == declared
    slib = _lib.load_scene()
    assert slib.vsr_scene_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.SCENELIB_PATH], capture_output=True, text=True).stdout
    # the constants the tests are written in are the header's
    with open(_lib.SCENEHEADER_PATH) as f:
        text = f.read()
    defs = dict(re.findall(r"#define (VSR_SCENE_[A-Z_0-9]+) (\d+)", text))
    assert (int(defs["VSR_SCENE_WG_PIXELS"]), int(defs["VSR_SCENE_FINISH_THREADS"])) == (R.WG_PIXELS, R.FINISH_THREADS)
    # the header states the rule's two known limits and that the defaults are not validated
    assert "ONSET of fast motion" in text and "second of two cuts one frame apart is missed" in text and "not been validated" in text


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, sdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(scene=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(warp=True) == ["vsr_warp_abi_version", "vsr_warp_error", "vsr_warp_last_error", "vsr_warp_ws_bytes"]
    assert not set(sdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "scene"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_scene_")], path
    assert not set(_exported(_lib.SCENELIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "scene":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.SCENELIB_PATH)) & set(_exported(row[0])), name


NULL, FAKE, FAKE2, OFF8, OFF4, OFF2, OFF1 = (ctypes.c_void_p(v) for v in (0, 0x1000, 0x2000, 0x1008, 0x1004, 0x1002, 0x1001))


def test_pair_sums_validates_before_any_launch():
    M = _lib.load_scene()
    luma = (ctypes.c_float * 4)(0.25, 0.5, 0.25, 16.0)     # the pointer the entry reads on the host

    def msg():
        return M.vsr_scene_last_error()

    def call(a=FAKE, b=FAKE, P=1, h=64, w=64, luma4=luma, sums=FAKE, ws=FAKE):
        return M.vsr_scene_pair_sums(a, b, P, h, w, luma4, sums, ws, NULL)

    for kw in ({"a": NULL}, {"b": NULL}, {"sums": NULL}, {"ws": NULL}):
        assert call(**kw) == -1 and b"scene_pair_sums: null pointer" in msg(), kw
    assert call(luma4=NULL) == -1 and b"scene_pair_sums: null luma4" in msg()
    for kw in ({"P": 0}, {"h": 0}, {"w": -3}, {"P": -1}):
        assert call(**kw) == -1 and b"scene_pair_sums: bad shape" in msg(), kw
    for kw in ({"P": 65536}, {"h": 65536}, {"w": 70000}):
        assert call(**kw) == -1 and b"scene_pair_sums: grid overflow" in msg() and b"beyond 65535" in msg(), kw
    assert call(a=OFF2) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(b=OFF1) == -1 and b"frames must be 4-byte aligned" in msg()
    assert call(sums=OFF4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    assert call(ws=OFF4) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()

    # the workspace: one double per workgroup of WG_PIXELS pixels and pair; 0 for what the call would refuse
    ws = M.vsr_scene_ws_bytes
    assert ws(1, 1, 1) == 8 and ws(3, 32, 32) == 3 * 8 and ws(1, 1, 1025) == 16 and ws(2, 540, 960) == 2 * 507 * 8
    for h, w in R.SIZES:
        for P in (1, 3):
            assert ws(P, h, w) == P * R.n_workgroups(h, w) * 8, (P, h, w)
    assert ws(1, *R.FINISH_SIZE) == (R.FINISH_THREADS + 1) * 8
    assert ws(0, 64, 64) == 0 and ws(1, 0, 64) == 0 and ws(1, 64, -1) == 0 and ws(65536, 64, 64) == 0 and ws(1, 65536, 1) == 0


def test_decide_validates_before_any_launch():
    M = _lib.load_scene()

    def msg():
        return M.vsr_scene_last_error()

    def call(sums=FAKE, P=1, prev=NULL, t_abs=15.0, ratio=2.0, flags=FAKE2):
        return M.vsr_scene_decide(sums, P, prev, t_abs, ratio, flags, NULL)

    for kw in ({"sums": NULL}, {"flags": NULL}):
        assert call(**kw) == -1 and b"scene_decide: null pointer" in msg(), kw
    for P in (0, -2):
        assert call(P=P) == -1 and b"scene_decide: bad count (P %d)" % P in msg()
    for v in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(t_abs=v) == -1 and b"scene_decide: t_abs must be finite and not negative" in msg(), v
        assert call(ratio=v) == -1 and b"scene_decide: ratio must be finite and not negative" in msg(), v
    assert call(sums=OFF4) == -1 and b"sums and prev must be 8-byte aligned" in msg()
    assert call(prev=OFF4) == -1 and b"sums and prev must be 8-byte aligned" in msg()
    assert call(flags=OFF2) == -1 and b"flags must be 4-byte aligned" in msg()


def test_window_validates_before_any_launch():
    M = _lib.load_scene()

    def msg():
        return M.vsr_scene_last_error()

    def call(a=FAKE, b=FAKE, c=FAKE, prev=FAKE, H=128, W=192, fab=NULL, fbc=NULL, x3=FAKE2, est=FAKE2, h=64, w=96):
        return M.vsr_scene_window(a, b, c, prev, H, W, fab, fbc, x3, est, h, w, NULL)

    for kw in ({"a": NULL}, {"b": NULL}, {"c": NULL}, {"x3": NULL}):
        assert call(**kw) == -1 and b"scene_window: null pointer" in msg(), kw
    assert call(prev=NULL) == -1 and b"both given or both null (got est given, prev_est null)" in msg()
    assert call(est=NULL) == -1 and b"both given or both null (got est null, prev_est given)" in msg()
    for kw in ({"h": 0}, {"w": -1}):
        assert call(**kw) == -1 and b"scene_window: bad shape (frames of" in msg(), kw
    for kw in ({"h": 65536, "H": 65536}, {"w": 65536, "W": 65536}):
        assert call(**kw) == -1 and b"scene_window: grid overflow" in msg(), kw
    for kw in ({"H": 0}, {"W": -192}):
        assert call(**kw) == -1 and b"scene_window: bad shape (estimate of" in msg(), kw
    assert call(H=129) == -1 and b"the estimate of 129 x 192 is no integer multiple of 64 x 96" in msg()
    assert call(W=200) == -1 and b"the estimate of 128 x 200 is no integer multiple of 64 x 96" in msg()
    assert call(H=192) == -1 and b"unequal factors (3 down, 2 across)" in msg()
    for kw in ({"a": OFF2}, {"b": OFF1}, {"c": OFF2}, {"prev": OFF1}, {"x3": OFF2}, {"est": OFF2}):
        assert call(**kw) == -1 and b"scene_window: the frames must be 4-byte aligned" in msg(), kw
    for kw in ({"fab": OFF2}, {"fbc": OFF1}):
        assert call(**kw) == -1 and b"scene_window: the flags must be 4-byte aligned" in msg(), kw
    # without an estimate H and W are not looked at: the shape checks that remain still refuse
    assert call(prev=NULL, est=NULL, H=-5, W=7, h=0) == -1 and b"scene_window: bad shape (frames of" in msg()


def test_check_reports_from_the_scene_librarys_own_buffer():
    M = _lib.load_scene()
    rc = M.vsr_scene_decide(FAKE, 1, None, -1.0, 2.0, FAKE2, None)
    with pytest.raises(_lib.VsrHipError, match=r"scene_decide failed \(-1\): scene_decide: t_abs must be finite and not negative, got -1"):
        _lib.check(rc, "scene_decide", lib=M)
