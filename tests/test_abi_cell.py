"""CPU-side checks of libvsr_hip_cell.so (include/vsr_hip_cell.h): the per-cell measure of a resident group is a library of its own, built
for gfx950 by the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry
validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cell_ref as R
from video_super_resolution_amd import _lib

ENTRIES = ["vsr_cell_abi_version", "vsr_cell_last_error", "vsr_cell_stats"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_cell_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.CELLLIB_PATH) and os.path.exists(_lib.CELLHEADER_PATH)
    assert _lib._SIDE["cell"][:2] == (_lib.CELLLIB_PATH, _lib.CELLHEADER_PATH)
    declared = _lib.declared_symbols(cell=True)
    assert declared == ENTRIES
    assert _exported(_lib.CELLLIB_PATH) == declared
    clib = _lib.load_cell()
    assert clib.vsr_cell_abi_version() == 1 and _lib.load_cell() is clib
    assert "gfx950" in subprocess.run(["strings", _lib.CELLLIB_PATH], capture_output=True, text=True).stdout
    # the constants the tests are written in are the header's, and so is the Python side's cell
    with open(_lib.CELLHEADER_PATH) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"#define (VSR_CELL[A-Z_0-9]*) (\d+)", text)}
    assert (defs["VSR_CELL"], defs["VSR_CELL_TILE_H"], defs["VSR_CELL_TILE_W"], defs["VSR_CELL_MAX_G"]) == (R.CELL, *R.TILE, R.MAX_G)
    assert R.TILE[0] % R.CELL == 0 and R.TILE[1] % R.CELL == 0      # a workgroup owns whole cells
    from video_super_resolution_amd import frames
    assert frames.CELL == R.CELL and frames.cell_shape((33, 17)) == R.cells(33, 17) == (3, 2)
    # the header states the arithmetic, the bound and that both load paths agree
    assert "y = ((o + a0 * R) + a1 * G) + a2 * B" in text and "130560" in text and "both give the same bits" in text
    assert R.MAX_VALUE == 130560


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, cdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(cell=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert not set(cdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "cell"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_cell_")], path
    assert not set(_exported(_lib.CELLLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "cell":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.CELLLIB_PATH)) & set(_exported(row[0])), name


# fake device pointers
NULL, FRAMES, STATS = (ctypes.c_void_p(v) for v in (0, 0x10000000, 0x30000000))
LUMA = (ctypes.c_float * 4)(*[float(v) for v in R.LUMA_BT601])


def test_cell_stats_validates_before_any_launch():
    M = _lib.load_cell()

    def msg():
        return M.vsr_cell_last_error()

    def call(frames=FRAMES, G=3, H=48, W=64, luma4=LUMA, stats=STATS):
        return M.vsr_cell_stats(frames, G, H, W, luma4, stats, NULL)

    assert call(frames=NULL) == -1 and b"cell_stats: null pointer" in msg()
    assert call(stats=NULL) == -1 and b"cell_stats: null pointer" in msg()
    assert call(luma4=NULL) == -1 and b"cell_stats: null luma4 (the four values of the luma row)" in msg()
    for kw in ({"G": 0}, {"H": 0}, {"W": -3}, {"G": -1}):
        assert call(**kw) == -1 and b"cell_stats: bad shape (G %d, frames of %d x %d)" % tuple({"G": 3, "H": 48, "W": 64, **kw}.values()) in msg(), kw
    for kw in ({"H": 65536}, {"W": 70000}):
        assert call(**kw) == -1 and b"cell_stats: grid overflow" in msg() and b"beyond 65535" in msg(), kw
    assert call(G=R.MAX_G + 1) == -1 and b"cell_stats: G = 65536 is beyond VSR_CELL_MAX_G = 65535" in msg()
    for kw in ({"frames": 0x10000002}, {"stats": 0x30000001}, {"frames": 0x10000003, "stats": 0x30000002}):
        kw = {k: ctypes.c_void_p(v) for k, v in kw.items()}
        assert call(**kw) == -1 and b"cell_stats: frames and stats must be 4-byte aligned" in msg(), kw


def test_check_reports_from_the_cell_librarys_own_buffer():
    M = _lib.load_cell()
    rc = M.vsr_cell_stats(FRAMES, 3, 48, 70000, LUMA, STATS, NULL)
    with pytest.raises(_lib.VsrHipError, match=r"cell_stats failed \(-1\): cell_stats: grid overflow \(frames of 48 x 70000 beyond 65535\)"):
        _lib.check(rc, "cell_stats", lib=M)


def test_the_restatement_on_hand_made_frames():
    """Two 2 x 3 frames whose luma code is the red value (luma4 = {1, 0, 0, 0}): every term by hand."""
    lu = np.array([1, 0, 0, 0], dtype=np.float32)
    f = np.zeros((2, 2, 3, 3), dtype=np.float32)
    f[0, :, :, 0] = [[10, 13, 13], [20, 10, 300]]     # codes 10 13 13 / 20 10 255
    f[1, :, :, 0] = [[10, 3, -7], [20.5, 11.5, np.nan]]   # codes 10 3 0 / 20 12 0 (ties to even; negatives and NaN to 0)
    s = R.cell_stats(f, lu)
    assert s.shape == (2, 1, 1, 2) and s.dtype == np.int32
    # frame 0: dx 3 + 0 + 10 + 245, dy 10 + 3 + 242
    assert s[0, 0, 0].tolist() == [3 + 0 + 10 + 245 + 10 + 3 + 242, 0]
    # frame 1: dx 7 + 3 + 8 + 12, dy 10 + 9 + 0; against frame 0: 0 + 10 + 13 + 0 + 2 + 255
    assert s[1, 0, 0].tolist() == [7 + 3 + 8 + 12 + 10 + 9 + 0, 0 + 10 + 13 + 0 + 2 + 255]
    cuts, m = R.cell_cuts(s, (2, 3), (15.0, 2.0))
    assert m.tolist() == [280.0 / 6.0] and cuts.tolist() == [True]
