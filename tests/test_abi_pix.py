"""CPU-side checks of libvsr_hip_pix.so (include/vsr_hip_pix.h): planar 4:2:2 / 4:4:4 frames in and out are a library of their own,
built for gfx950 by the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and
both entries validate their arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_pix_abi_version", "vsr_pix_ingest", "vsr_pix_last_error", "vsr_pix_write"]
P422, P444, P422_10, P444_10 = range(4)
LEFT, CENTER = range(2)


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_pix_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.PIXLIB_PATH) and _lib.PIXLIB_PATH.endswith("libvsr_hip_pix.so")
    assert _lib.PIXHEADER_PATH.endswith(os.path.join("include", "vsr_hip_pix.h"))
    assert _lib._SIDE["pix"][2:] == ("vsr_pix", 1, False)
    declared = _lib.declared_symbols(pix=True)
    assert declared == ENTRIES
    assert _exported(_lib.PIXLIB_PATH) == declared
    plib = _lib.load_pix()
    assert plib.vsr_pix_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.PIXLIB_PATH], capture_output=True, text=True).stdout


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, pdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(pix=True)
    assert _lib.declared_symbols(yuv=True) == ["vsr_yuv_abi_version", "vsr_yuv_ingest", "vsr_yuv_last_error", "vsr_yuv_write"]
    assert _lib.load_yuv().vsr_yuv_abi_version() == 1
    assert not set(pdeclared) & (set(declared) | set(xdeclared))
    mine = set(_exported(_lib.PIXLIB_PATH))
    for path in [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "pix"]:
        theirs = _exported(path)
        assert not [s for s in theirs if s.startswith("vsr_pix_")], path
        assert not mine & set(theirs), path   # (its own version / error entries, no second vsr_last_error, none of the yuv entries)


def test_pix_entries_validate_before_any_launch():
    P = _lib.load_pix()
    null, fake, odd, off8 = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001), ctypes.c_void_p(0x1008)
    coef = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)   # the only pointer an entry reads on the host

    def msg():
        return P.vsr_pix_last_error()

    ing, wr = P.vsr_pix_ingest, P.vsr_pix_write
    # ingest(frames, fmt, coef12, siting, lr, hr_or_null, F, H, W, h, w, stream)
    assert ing(null, P422, coef, LEFT, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"pix_ingest: null pointer" in msg()
    assert ing(fake, P422, null, LEFT, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"pix_ingest: null pointer" in msg()
    assert ing(fake, P422, coef, LEFT, null, fake, 1, 8, 8, 2, 2, null) == -1 and b"pix_ingest: null pointer" in msg()
    assert ing(fake, 4, coef, LEFT, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"unknown pixel format 4" in msg()
    assert ing(fake, -1, coef, LEFT, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"unknown pixel format -1" in msg()
    for fmt in (P422, P444):   # 4:4:4 ignores the siting but still wants a known one
        assert ing(fake, fmt, coef, 2, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"unknown chroma siting 2" in msg()
    for fmt in (P422, P422_10):   # 4:2:2: an even W; H may be odd
        assert ing(fake, fmt, coef, LEFT, fake, null, 1, 8, 9, 2, 2, null) == -1 and b"bad shape" in msg() and b"even W" in msg()
    for fmt in range(4):
        assert ing(fake, fmt, coef, LEFT, fake, null, 1, 0, 8, 2, 2, null) == -1 and b"bad shape" in msg()
        assert ing(fake, fmt, coef, LEFT, fake, null, 1, 8, -8, 2, 2, null) == -1 and b"bad shape" in msg()
        assert ing(fake, fmt, coef, LEFT, fake, null, 0, 8, 8, 2, 2, null) == -1 and b"bad shape" in msg()
    assert ing(fake, P422, coef, LEFT, fake, null, 1, 8, 8, 10, 2, null) == -1 and b"bad shape (lr 10 x 2 from 8 x 8)" in msg()
    assert ing(fake, P444, coef, LEFT, fake, null, 1, 7, 9, 2, 10, null) == -1 and b"bad shape (lr 2 x 10 from 7 x 9)" in msg()
    assert ing(fake, P422, coef, LEFT, fake, null, 1, 8, 8, 0, 2, null) == -1 and b"bad shape" in msg()
    assert ing(fake, P422, coef, LEFT, fake, null, 1, 8, 8, 2, 0, null) == -1 and b"bad shape" in msg()
    # the limits of the launch geometry: grid.z (F), grid.y (h <= H), 32-bit indices inside a frame (W), the flat grid (F * H * W)
    assert ing(fake, P422, coef, LEFT, fake, null, 65536, 8, 8, 2, 2, null) == -1 and b"grid overflow" in msg()
    assert ing(fake, P422, coef, LEFT, fake, null, 1, 65536, 8, 2, 2, null) == -1 and b"grid overflow" in msg()
    assert ing(fake, P422, coef, LEFT, fake, null, 1, 8, 65536, 2, 2, null) == -1 and b"grid overflow (F 1, H 8, W 65536 beyond" in msg()
    assert ing(fake, P444, coef, LEFT, fake, null, 65535, 65534, 65534, 2, 2, null) == -1
    assert b"grid overflow (F * H * W = %d)" % (65535 * 65534 * 65534) in msg()
    # float buffers: 16-byte aligned; 16-bit samples: an even address (8-bit frames may start anywhere)
    assert ing(fake, P422, coef, LEFT, off8, null, 1, 8, 8, 2, 2, null) == -1 and b"16-byte aligned" in msg()
    assert ing(fake, P422, coef, LEFT, fake, off8, 1, 8, 8, 2, 2, null) == -1 and b"16-byte aligned" in msg()
    for fmt in (P422_10, P444_10):
        assert ing(odd, fmt, coef, LEFT, fake, null, 1, 8, 8, 2, 2, null) == -1 and b"16-bit pixel format at an odd byte address" in msg()

    # write(rgb, frames_out, fmt, coef12, siting, F, H, W, stream)
    assert wr(null, fake, P444, coef, LEFT, 1, 8, 8, null) == -1 and b"pix_write: null pointer" in msg()
    assert wr(fake, null, P444, coef, LEFT, 1, 8, 8, null) == -1 and b"pix_write: null pointer" in msg()
    assert wr(fake, fake, P444, null, LEFT, 1, 8, 8, null) == -1 and b"pix_write: null pointer" in msg()
    assert wr(fake, fake, 7, coef, LEFT, 1, 8, 8, null) == -1 and b"unknown pixel format 7" in msg()
    for fmt in (P422, P444):
        assert wr(fake, fake, fmt, coef, -1, 1, 8, 8, null) == -1 and b"unknown chroma siting -1" in msg()
    assert wr(fake, fake, P422, coef, LEFT, 1, 8, 7, null) == -1 and b"bad shape" in msg()
    assert wr(fake, fake, P444, coef, LEFT, 1, -2, 8, null) == -1 and b"bad shape" in msg()
    assert wr(fake, fake, P444, coef, LEFT, 0, 8, 8, null) == -1 and b"bad shape" in msg()
    assert wr(fake, fake, P422, coef, LEFT, 65536, 8, 8, null) == -1 and b"grid overflow" in msg()
    assert wr(fake, fake, P422, coef, LEFT, 1, 65536, 8, null) == -1 and b"grid overflow" in msg()
    assert wr(fake, fake, P422, coef, LEFT, 1, 8, 65536, null) == -1 and b"grid overflow" in msg()
    assert wr(fake, fake, P444, coef, LEFT, 65535, 65534, 65534, null) == -1 and b"grid overflow (F * H * W" in msg()
    assert wr(off8, fake, P422, coef, LEFT, 1, 8, 8, null) == -1 and b"16-byte aligned" in msg()
    for fmt in (P422_10, P444_10):
        assert wr(fake, odd, fmt, coef, LEFT, 1, 8, 8, null) == -1 and b"16-bit pixel format at an odd byte address" in msg()


def test_check_reports_from_the_pix_librarys_own_buffer():
    P = _lib.load_pix()
    fake = ctypes.c_void_p(0x1000)
    coef = (ctypes.c_float * 12)()
    rc = P.vsr_pix_write(fake, fake, 9, coef, 0, 1, 8, 8, None)
    with pytest.raises(_lib.VsrHipError, match=r"pix_write failed \(-1\): pix_write: unknown pixel format 9"):
        _lib.check(rc, "pix_write", lib=P)
