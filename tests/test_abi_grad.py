"""CPU-side checks of libvsr_hip_grad.so (include/vsr_hip_grad.h): the backward of Resample2d / ChannelNorm / Correlation is a
library of its own, built for gfx950 by the same `make`; it exports exactly what its header declares, the shipping library
gains nothing from it, and every entry validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import os
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_grad_abi_version", "vsr_grad_channelnorm_f32", "vsr_grad_correlation_f32", "vsr_grad_last_error",
           "vsr_grad_resample2d_f32"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_grad_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.GLIB_PATH)
    declared = _lib.declared_symbols(grad=True)
    assert declared == ENTRIES
    assert _exported(_lib.GLIB_PATH) == declared
    glib = _lib.load_grad()
    assert glib.vsr_grad_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.GLIB_PATH], capture_output=True, text=True).stdout


def test_the_other_two_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    # the two existing call forms of declared_symbols keep their results; the three headers share no entry
    declared, xdeclared, gdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(grad=True)
    assert len(declared) == 66 and "vsr_resample2d_f32" in declared and "vsr_conv2d_tuning" in xdeclared
    assert not set(gdeclared) & (set(declared) | set(xdeclared))
    for path in (_lib.LIB_PATH, _lib.XLIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("vsr_grad_")], path
    # ... and the grad library defines none of theirs (its own version / error entries, no second vsr_last_error)
    assert not set(_exported(_lib.GLIB_PATH)) & (set(declared) | set(xdeclared))


def test_grad_entries_validate_before_any_launch():
    G = _lib.load_grad()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)   # never dereferenced on the host: every call fails before a launch

    def msg():
        return G.vsr_grad_last_error()

    assert G.vsr_grad_resample2d_f32(null, fake, fake, fake, fake, 1, 3, 8, 8, 1, 1, null) == -1 and b"null" in msg()
    assert G.vsr_grad_resample2d_f32(fake, fake, fake, null, null, 1, 3, 8, 8, 1, 1, null) == -1 and b"both gradients" in msg()
    assert G.vsr_grad_resample2d_f32(fake, fake, fake, fake, null, 1, 0, 8, 8, 1, 1, null) == -1 and b"bad shape" in msg()
    assert G.vsr_grad_resample2d_f32(fake, fake, fake, fake, fake, 1, 3, 8, 8, 3, 1, null) == -3 and b"kernel_size 3" in msg()

    assert G.vsr_grad_channelnorm_f32(fake, fake, fake, null, 1, 3, 8, 8, null) == -1 and b"null" in msg()
    assert G.vsr_grad_channelnorm_f32(fake, fake, fake, fake, 1, 3, -8, 8, null) == -1 and b"bad shape" in msg()

    corr = G.vsr_grad_correlation_f32
    assert corr(fake, null, fake, fake, fake, 1, 8, 8, 8, 4, 1, 4, 1, 2, null) == -1 and b"null" in msg()
    assert corr(fake, fake, fake, null, null, 1, 8, 8, 8, 4, 1, 4, 1, 2, null) == -1 and b"both gradients" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 0, 8, 4, 1, 4, 1, 2, null) == -1 and b"bad shape" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 8, 8, 4, 3, 4, 1, 2, null) == -3 and b"kernel_size 3" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 8, 8, 4, 1, 4, 0, 2, null) == -1 and b"strides" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 8, 8, 0, 1, 20, 1, 2, null) == -1 and b"empty output" in msg()
    # the limits of the launch geometry: displacement range, LDS window, grid.z, grid.y
    assert corr(fake, fake, fake, fake, fake, 1, 8, 64, 2048, 600, 1, 600, 1, 1, null) == -1 and b"displacement range 1201" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 64, 2048, 240, 1, 240, 1, 16, null) == -1 and b"LDS" in msg()   # 32 + 480 columns
    assert corr(fake, fake, fake, fake, fake, 4096, 1024, 8, 8, 4, 1, 4, 1, 2, null) == -1 and b"grid overflow" in msg()
    assert corr(fake, fake, fake, fake, fake, 1, 8, 70000, 8, 4, 1, 4, 1, 2, null) == -1 and b"grid overflow" in msg()


def test_check_reports_from_the_grad_librarys_own_buffer():
    G = _lib.load_grad()
    fake = ctypes.c_void_p(0x1000)
    rc = G.vsr_grad_correlation_f32(fake, fake, fake, fake, fake, 1, 8, 8, 8, 4, 3, 4, 1, 2, None)
    with pytest.raises(_lib.VsrHipError, match=r"grad_correlation failed \(-3\): grad_correlation: kernel_size 3"):
        _lib.check(rc, "grad_correlation", lib=G)
