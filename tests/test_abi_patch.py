"""CPU-side checks of libvsr_hip_patch.so (include/vsr_hip_patch.h): the training-patch gather is a library of its own, built for gfx950 by
the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry validates
its arguments and every row of its host table before any launch (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

import _patch_ref as R
from video_super_resolution_amd import _lib

ENTRIES = ["vsr_patch_abi_version", "vsr_patch_gather", "vsr_patch_last_error"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_patch_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.PATCHLIB_PATH) and os.path.exists(_lib.PATCHHEADER_PATH)
    assert _lib._SIDE["patch"][:2] == (_lib.PATCHLIB_PATH, _lib.PATCHHEADER_PATH)
    declared = _lib.declared_symbols(patch=True)
    assert declared == ENTRIES
    assert _exported(_lib.PATCHLIB_PATH) == declared
    plib = _lib.load_patch()
    assert plib.vsr_patch_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.PATCHLIB_PATH], capture_output=True, text=True).stdout
    # the constants the tests are written in are the header's, and so are the flag bits of the Python side
    with open(_lib.PATCHHEADER_PATH) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"#define (VSR_PATCH_[A-Z_0-9]+) (\d+)", text)}
    assert (defs["VSR_PATCH_MAX_B"], defs["VSR_PATCH_TILE"]) == (R.MAX_B, R.TILE)
    assert (defs["VSR_PATCH_FLIP_X"], defs["VSR_PATCH_FLIP_Y"], defs["VSR_PATCH_TRANSPOSE"], defs["VSR_PATCH_REVERSE_TIME"]) == \
        (R.FLIP_X, R.FLIP_Y, R.TRANSPOSE, R.REVERSE_TIME)
    from video_super_resolution_amd import frames
    assert frames.PATCH_FLAGS == {"flip_x": R.FLIP_X, "flip_y": R.FLIP_Y, "transpose": R.TRANSPOSE, "reverse": R.REVERSE_TIME}
    assert frames.PATCH_MAX_B == R.MAX_B
    # the header says why the nearest LR patch is decimated after the augmentation
    assert "decimation of the AUGMENTED patch" in text and "HR[iS+S-1][jS]" in text


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, pdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(patch=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert not set(pdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "patch"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_patch_")], path
    assert not set(_exported(_lib.PATCHLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "patch":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.PATCHLIB_PATH)) & set(_exported(row[0])), name


# fake device pointers, far enough apart that no extent of the calls below reaches the next
NULL, SRC, LSRC, HR, LR = (ctypes.c_void_p(v) for v in (0, 0x10000000, 0x20000000, 0x30000000, 0x40000000))


def _table(*rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int * len(flat))(*flat)


def test_gather_validates_before_any_launch():
    M = _lib.load_patch()

    def msg():
        return M.vsr_patch_last_error()

    def call(src=SRC, G=4, H=96, W=120, lr_src=NULL, S=2, table=_table((0, 0, 0, 0)), B=1, n=3, Ph=64, Pw=64, hr=HR, lr=LR):
        return M.vsr_patch_gather(src, G, H, W, lr_src, S, table, B, n, Ph, Pw, hr, lr, NULL)

    assert call(src=NULL) == -1 and b"patch_gather: null src" in msg()
    assert call(table=NULL) == -1 and b"patch_gather: null table" in msg()
    assert call(hr=NULL, lr=NULL) == -1 and b"patch_gather: both outputs are null" in msg()
    for kw in ({"G": 0}, {"H": 0}, {"W": -3}):
        assert call(**kw) == -1 and b"patch_gather: bad source shape" in msg(), kw
    for kw in ({"B": 0}, {"n": 0}, {"Ph": 0}, {"Pw": -2}, {"B": -1}):
        assert call(**kw) == -1 and b"patch_gather: bad sample shape" in msg(), kw
    for S in (0, 9, -1):
        assert call(S=S) == -1 and b"patch_gather: S must lie in 1..8, got %d" % S in msg()
    assert call(Ph=63) == -1 and b"the patch of 63 x 64 is no multiple of S = 2" in msg()
    assert call(Pw=33) == -1 and b"the patch of 64 x 33 is no multiple of S = 2" in msg()
    big = _table(*[(0, 0, 0, 0)] * (R.MAX_B + 1))
    assert call(B=R.MAX_B + 1, table=big) == -1 and b"B = 65 is beyond VSR_PATCH_MAX_B = 64" in msg()
    for kw in ({"G": 65536}, {"H": 65536}, {"W": 70000}, {"n": 65536, "G": 65535}, {"Ph": 65536, "H": 65535}, {"Pw": 65536, "W": 65535}):
        assert call(**kw) == -1 and b"patch_gather: grid overflow" in msg() and b"beyond 65535" in msg(), kw
    assert call(lr_src=LSRC, H=97) == -1 and b"with lr_src the frames of 97 x 120 must be a multiple of S = 2" in msg()
    assert call(lr_src=LSRC, W=121) == -1 and b"with lr_src the frames of 96 x 121 must be a multiple of S = 2" in msg()

    # per row; the message names the row
    ok = (0, 0, 0, 0)
    assert call(B=2, table=_table(ok, (0, 0, 0, 16))) == -1 and b"row 1 has unknown flag bits (flags 16" in msg()
    assert call(B=2, table=_table(ok, (0, 0, 0, -1))) == -1 and b"row 1 has unknown flag bits" in msg()
    assert call(table=_table((-1, 0, 0, 0))) == -1 and b"row 0 takes frames -1 .. 1 of 4" in msg()
    assert call(table=_table((2, 0, 0, 0))) == -1 and b"row 0 takes frames 2 .. 4 of 4" in msg()
    assert call(n=5) == -1 and b"row 0 takes frames 0 .. 4 of 4" in msg()
    assert call(table=_table((0, -2, 0, 0))) == -1 and b"row 0: the crop of 64 x 64 at (-2, 0) leaves the frame of 96 x 120" in msg()
    assert call(table=_table((0, 0, -2, 0))) == -1 and b"at (0, -2) leaves the frame" in msg()
    assert call(table=_table((0, 34, 0, 0))) == -1 and b"row 0: the crop of 64 x 64 at (34, 0) leaves the frame of 96 x 120" in msg()
    assert call(B=3, table=_table(ok, ok, (0, 0, 58, 3))) == -1 and b"row 2: the crop of 64 x 64 at (0, 58) leaves the frame of 96 x 120" in msg()
    assert call(Ph=128) == -1 and b"row 0: the crop of 128 x 64 at (0, 0) leaves the frame" in msg()
    # a 64 x 112 patch fits the 96 x 120 frame as it is (`R.row_ok`, below; not called here: it would launch on fake pointers); transposed
    # it takes 112 rows and leaves it
    assert call(Pw=112, table=_table((0, 0, 0, 4))) == -1 and b"row 0: the crop of 112 x 64 at (0, 0) leaves the frame of 96 x 120" in msg()
    assert call(Pw=112, B=2, table=_table((0, 32, 8, 3), (1, 0, 56, 7))) == -1 and b"row 1: the crop of 112 x 64 at (0, 56)" in msg()
    # with lr_src the origins are multiples of S
    assert call(lr_src=LSRC, table=_table((0, 3, 0, 0))) == -1 and b"row 0: with lr_src the origin (3, 0) must be a multiple of S = 2" in msg()
    assert call(lr_src=LSRC, table=_table((0, 0, 7, 0))) == -1 and b"with lr_src the origin (0, 7) must be a multiple of S = 2" in msg()

    for kw in ({"src": 0x10000002}, {"lr_src": 0x20000001}, {"hr": 0x30000002}, {"lr": 0x40000003}):
        kw = {k: ctypes.c_void_p(v) for k, v in kw.items()}
        assert call(**kw) == -1 and b"patch_gather: the frames and the patches must be 4-byte aligned" in msg(), kw
    # extents: src is 4 * 96 * 120 * 12 bytes, hr 3 * 64 * 64 * 12, lr a quarter of that
    src_bytes, hr_bytes, lr_bytes = 4 * 96 * 120 * 12, 3 * 64 * 64 * 12, 3 * 32 * 32 * 12
    assert call(hr=ctypes.c_void_p(0x10000000 + src_bytes - 4)) == -1 and b"patch_gather: hr overlaps src" in msg()
    assert call(hr=ctypes.c_void_p(0x10000000 - hr_bytes + 4)) == -1 and b"patch_gather: hr overlaps src" in msg()
    assert call(lr=SRC) == -1 and b"patch_gather: lr overlaps src" in msg()
    assert call(lr_src=LSRC, hr=LSRC) == -1 and b"patch_gather: hr overlaps lr_src" in msg()
    assert call(lr_src=LSRC, lr=ctypes.c_void_p(0x20000000 - lr_bytes + 4)) == -1 and b"patch_gather: lr overlaps lr_src" in msg()
    assert call(lr=ctypes.c_void_p(0x30000000 + hr_bytes - 4)) == -1 and b"patch_gather: hr overlaps lr" in msg()


def test_the_bounds_rule_of_the_reference_module_is_the_librarys():
    """Every refusal of a row above is one `R.row_ok` refuses too, and the rows it accepts are in frame."""
    for row, kw in (((0, 34, 0, 0), {}), ((0, 0, 58, 3), {}), ((2, 0, 0, 0), {}), ((0, 0, 0, 16), {}), ((0, 3, 0, 0), {"S": 2, "lr_src": True})):
        assert not R.row_ok(row, 4, 3, 96, 120, 64, 64, **kw), row
    assert not R.row_ok((0, 0, 0, 4), 4, 3, 96, 120, 64, 112) and R.row_ok((0, 32, 8, 3), 4, 3, 96, 120, 64, 112)
    assert R.row_ok((1, 32, 56, 15), 4, 3, 96, 120, 64, 64, S=2, lr_src=True)


def test_check_reports_from_the_patch_librarys_own_buffer():
    M = _lib.load_patch()
    rc = M.vsr_patch_gather(SRC, 4, 96, 120, NULL, 9, _table((0, 0, 0, 0)), 1, 3, 64, 64, HR, LR, NULL)
    with pytest.raises(_lib.VsrHipError, match=r"patch_gather failed \(-1\): patch_gather: S must lie in 1\.\.8, got 9"):
        _lib.check(rc, "patch_gather", lib=M)
