"""CPU-side checks of libvsr_hip_deint.so (include/vsr_hip_deint.h): the deinterlacer is a library of its own, built for gfx950 by the
same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry validates
its arguments before any launch, each refusal with its own message (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_deint_abi_version", "vsr_deint_frame", "vsr_deint_last_error"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def _planes(*rows):
    return (_lib.DeintPlane * len(rows))(*[_lib.DeintPlane(*r) for r in rows])


def test_deint_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.DEINTLIB_PATH) and _lib.DEINTLIB_PATH.endswith("libvsr_hip_deint.so")
    assert _lib.DEINTHEADER_PATH.endswith(os.path.join("include", "vsr_hip_deint.h"))
    assert _lib._SIDE["deint"][:2] == (_lib.DEINTLIB_PATH, _lib.DEINTHEADER_PATH)
    assert _lib._SIDE["deint"][2:] == ("vsr_deint", 1, False)
    declared = _lib.declared_symbols(deint=True)
    assert declared == ENTRIES
    assert _exported(_lib.DEINTLIB_PATH) == declared
    lib = _lib.load_deint()
    assert _lib.load_deint() is lib and lib.vsr_deint_abi_version() == 1
    assert lib.vsr_last_error() == lib.vsr_deint_last_error()
    assert "gfx950" in subprocess.run(["strings", _lib.DEINTLIB_PATH], capture_output=True, text=True).stdout


def test_the_makefile_builds_it_from_its_source_alone():
    with open(os.path.join(os.path.dirname(_lib.DEINTLIB_PATH), "csrc", "Makefile")) as f:
        text = f.read()
    names = re.search(r"^NAMES := (.*)$", text, re.M).group(1).split()
    assert "clip_deint" not in names                                       # neither main library links it
    assert re.search(r"^\$\(DEINTOUT\): build/clip_deint\.o\n\t\$\(HIPCC\) .* -o \$@ build/clip_deint\.o$", text, re.M)


def test_the_header_states_the_constants_the_tests_derive_their_sizes_from():
    with open(_lib.DEINTHEADER_PATH) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (VSR_DEINT_[A-Z_]+) (\d+)", text, re.M)}
    assert defs == {"VSR_DEINT_ABI_VERSION": 1, "VSR_DEINT_MAX_PLANES": 3, "VSR_DEINT_TILE_ROWS": 8, "VSR_DEINT_TILE_BYTES": 1024}
    assert ctypes.sizeof(_lib.DeintPlane) == 24   # size_t, three ints, padded to the size_t


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, ddeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(deint=True)
    assert not set(ddeclared) & (set(declared) | set(xdeclared))
    mine = set(_exported(_lib.DEINTLIB_PATH))
    for path in [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "deint"]:
        theirs = _exported(path)
        assert not [s for s in theirs if s.startswith("vsr_deint_")], path
        assert not mine & set(theirs), path
    for name, row in _lib._SIDE.items():   # every side library still exports exactly what its header declares
        assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name


def test_deint_frame_validates_before_any_launch():
    D = _lib.load_deint()
    null, fake, fake2, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x1001)
    out = ctypes.c_void_p(0x9000)
    one = _planes((0, 4, 6, 1))

    def call(prev=fake, cur=fake, nxt=fake2, o=out, planes=one, n=1, sb=1, shift=0, keep=0, kf=1):
        return D.vsr_deint_frame(prev, cur, nxt, o, planes, n, sb, shift, keep, kf, null)

    def msg():
        return D.vsr_deint_last_error()

    for kw in ("prev", "cur", "nxt", "o"):
        assert call(**{kw: null}) == -1 and b"deint_frame: null pointer" in msg()
    assert call(planes=ctypes.cast(null, ctypes.POINTER(_lib.DeintPlane))) == -1 and b"null pointer" in msg()
    for n in (0, 4, -1):
        assert call(n=n) == -1 and b"n_planes %d outside 1..3" % n in msg()
    for rows in (1, 0, -3):
        assert call(planes=_planes((0, rows, 6, 1))) == -1 and b"plane 0 has %d rows" % rows in msg()
    assert call(planes=_planes((0, 4, 6, 1), (24, 1, 3, 1)), n=2) == -1 and b"plane 1 has 1 rows" in msg()
    assert call(planes=_planes((0, 4, 0, 1))) == -1 and b"cols 0 and comps 1 must be positive" in msg()
    assert call(planes=_planes((0, 4, -6, 1))) == -1 and b"must be positive" in msg()
    assert call(planes=_planes((0, 4, 6, 0))) == -1 and b"cols 6 and comps 0 must be positive" in msg()
    assert call(planes=_planes((0, 4, 6, 3))) == -1 and b"comps 3 beyond 2" in msg()
    for sb in (0, 3, 4):
        assert call(sb=sb) == -1 and b"sample_bytes %d is not 1 or 2" % sb in msg()
    for shift in (1, 2, 8, -6):
        assert call(sb=2, shift=shift) == -1 and b"shift %d is not 0 or 6" % shift in msg()
    assert call(sb=1, shift=6) == -1 and b"shift 6 needs 16-bit samples" in msg()
    assert call(keep=2) == -1 and b"keep 2 and kept_first 1 must each be 0 or 1" in msg()
    assert call(kf=-1) == -1 and b"keep 0 and kept_first -1 must each be 0 or 1" in msg()
    # 16-bit samples: every base and every plane offset even; 8-bit frames may start and lie anywhere
    for kw in ("prev", "cur", "nxt", "o"):
        assert call(**{kw: odd}, sb=2) == -1 and b"16-bit samples at an odd byte address" in msg()
    assert call(planes=_planes((0, 4, 6, 1), (49, 2, 3, 2)), n=2, sb=2) == -1 and b"plane 1: 16-bit samples at an odd byte offset 49" in msg()
    # the grid: rows in grid.y (65535 workgroups of 8 rows), a row of at most 2^30 samples
    assert call(planes=_planes((0, 65535 * 8 + 1, 6, 1))) == -1 and b"grid overflow (plane 0: 524281 rows" in msg()
    assert call(planes=_planes((0, 4, 2 ** 30, 2))) == -1 and b"grid overflow" in msg() and b"%d samples" % 2 ** 31 in msg()
    # out must be none of the inputs; the inputs may be one another
    for kw in ("prev", "cur", "nxt"):
        assert call(**{kw: out}) == -1 and b"out is one of the inputs" in msg()
    # the last message stays until the next failure, and a refused call is the only kind a machine without a GPU can make
    assert b"out is one of the inputs" in msg()


def test_check_reports_from_the_deint_librarys_own_buffer():
    D = _lib.load_deint()
    fake = ctypes.c_void_p(0x1000)
    rc = D.vsr_deint_frame(fake, fake, fake, ctypes.c_void_p(0x2000), _planes((0, 4, 6, 1)), 1, 5, 0, 0, 1, None)
    with pytest.raises(_lib.VsrHipError, match=r"deint_frame failed \(-1\): deint_frame: sample_bytes 5 is not 1 or 2"):
        _lib.check(rc, "deint_frame", lib=D)
