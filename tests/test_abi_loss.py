"""CPU-side checks of libvsr_hip_loss.so (include/vsr_hip_loss.h): the loss's pixel terms are a library of their own, built for gfx950
by the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry
validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_loss_abi_version", "vsr_loss_last_error", "vsr_loss_pixel_terms", "vsr_loss_ws_bytes"]
SF, SR, NS = 768, 32, 14


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_loss_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.LOSSLIB_PATH) and os.path.exists(_lib.LOSSHEADER_PATH)
    assert _lib._SIDE["loss"][:2] == (_lib.LOSSLIB_PATH, _lib.LOSSHEADER_PATH)
    declared = _lib.declared_symbols(loss=True)
    assert declared == ENTRIES
    assert _exported(_lib.LOSSLIB_PATH) == declared
    lib = _lib.load_loss()
    assert lib.vsr_loss_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.LOSSLIB_PATH], capture_output=True, text=True).stdout
    with open(_lib.LOSSHEADER_PATH) as f:
        text = f.read()
    for name, value in (("VSR_LOSS_STRIP_FLOATS", SF), ("VSR_LOSS_SEGMENT_ROWS", SR), ("VSR_LOSS_NSUMS", NS)):
        assert f"#define {name} {value}\n" in text


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, ldeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(loss=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(metric=True) == ["vsr_metric_abi_version", "vsr_metric_frames", "vsr_metric_last_error", "vsr_metric_ws_bytes"]
    assert not set(ldeclared) & (set(declared) | set(xdeclared))
    for path in [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "loss"]:
        assert not [s for s in _exported(path) if s.startswith("vsr_loss_")], path
    assert not set(_exported(_lib.LOSSLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "loss":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.LOSSLIB_PATH)) & set(_exported(row[0])), name


def test_loss_entry_validates_before_any_launch():
    M = _lib.load_loss()
    null = ctypes.c_void_p(0)
    H, W = 8, 12
    N = 3 * H * W
    # fake device addresses, far apart: every range of the call fits between two of them
    outputs, target, mask, masked, nhwc4, sums, terms, ws = (ctypes.c_void_p(0x100000 * (i + 1)) for i in range(8))

    def off(p, n):
        return ctypes.c_void_p(p.value + n)

    def msg():
        return M.vsr_loss_last_error()

    def call(**kw):
        a = dict(outputs=outputs, target=target, mask=mask, H=H, W=W, masked=masked, nhwc4=nhwc4, sums=sums, terms=terms, ws=ws)
        a.update(kw)
        return M.vsr_loss_pixel_terms(a["outputs"], a["target"], a["mask"], a["H"], a["W"], a["masked"], a["nhwc4"], a["sums"], a["terms"],
                                      a["ws"], null)

    # null pointers: the six required ones; masked and nhwc4 may be null (such a call is refused only further on, here for its size)
    for name in ("outputs", "target", "mask", "sums", "terms", "ws"):
        assert call(**{name: null}) == -1 and b"loss_pixel_terms: null pointer" in msg(), name
    assert call(masked=null, nhwc4=null, H=1) == -1 and b"must be at least 2" in msg()
    # sizes: below 2 the reference divides by zero; beyond the grid
    for kw in ({"H": 1}, {"W": 1}, {"H": 0}, {"W": -4}):
        assert call(**kw) == -1 and b"H and W must be at least 2" in msg(), kw
    assert call(H=1, W=7) == -1 and b"got 1 x 7" in msg()
    for kw in ({"H": 65536}, {"W": 65536}):
        assert call(**kw) == -1 and b"grid overflow" in msg() and b"beyond 65535" in msg(), kw
    # alignment: 4 bytes for the floats, 2 for nhwc4, 8 for sums and ws
    for name in ("outputs", "target", "masked", "terms"):
        assert call(**{name: off(locals()[name], 2)}) == -1 and b"float buffers must be 4-byte aligned" in msg(), name
    assert call(nhwc4=off(nhwc4, 1)) == -1 and b"nhwc4 must be 2-byte aligned" in msg()
    assert call(sums=off(sums, 4)) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    assert call(ws=off(ws, 4)) == -1 and b"sums and the workspace must be 8-byte aligned" in msg()
    # an output range that overlaps an input range: first and last byte of each, and the byte past the end is allowed ... up to the
    # next check (a fake address cannot be launched on: the accepted forms are exercised on the device, tests/test_gpu_loss.py)
    ws_bytes = M.vsr_loss_ws_bytes(H, W)
    in_bytes = {"outputs": 3 * N * 4, "target": N * 4, "mask": N}
    out_bytes = {"masked": 4 * N * 4, "nhwc4": 8 * H * W * 8, "sums": NS * 8, "terms": 48, "ws": ws_bytes}
    base = dict(outputs=outputs, target=target, mask=mask)
    for iname, ibytes in in_bytes.items():
        for oname, obytes in out_bytes.items():
            need = b"the output %s overlaps the input %s" % (oname.encode(), iname.encode())
            last = (ibytes - 1) // 8 * 8                       # an aligned address inside the input's last bytes
            first = base[iname].value - (obytes - 1) // 8 * 8  # ... whose range ends inside the input's first bytes
            for addr in (base[iname].value, base[iname].value + last, first):
                assert call(**{oname: ctypes.c_void_p(addr)}) == -1 and need in msg(), (oname, iname, hex(addr))

    # the workspace: 14 doubles per workgroup of 768 floats of a row by 32 rows; 0 for what the call would refuse
    wsb = M.vsr_loss_ws_bytes
    assert wsb(2, 2) == NS * 8 and wsb(32, 256) == NS * 8 and wsb(33, 256) == 2 * NS * 8 and wsb(32, 257) == 2 * NS * 8
    assert wsb(65, 513) == 3 * 3 * NS * 8 and wsb(2160, 3840) == 15 * 68 * NS * 8 and wsb(264, 280) == 2 * 9 * NS * 8
    assert wsb(1, 64) == 0 and wsb(64, 1) == 0 and wsb(0, 0) == 0 and wsb(65536, 64) == 0 and wsb(64, 65536) == 0


def test_check_reports_from_the_loss_librarys_own_buffer():
    M = _lib.load_loss()
    fake = ctypes.c_void_p(0x1000)
    rc = M.vsr_loss_pixel_terms(fake, fake, fake, 1, 1, None, None, fake, fake, fake, None)
    with pytest.raises(_lib.VsrHipError, match=r"loss_pixel_terms failed \(-1\): loss_pixel_terms: H and W must be at least 2"):
        _lib.check(rc, "loss_pixel_terms", lib=M)
