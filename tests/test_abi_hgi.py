"""CPU-side checks of libvsr_hip_hgi.so (include/vsr_hip_hgi.h): the one-launch inception block is a library of its own, built for
gfx950 by the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, and the entry
validates its arguments before any launch (no compute without a GPU; no pointer is dereferenced on the host)."""
import ctypes
import os
import re
import subprocess

import pytest

from video_super_resolution_amd import _lib
from video_super_resolution_amd.depth import _A, _B, _C, _D, _E, _F, _G, _H, _J
from video_super_resolution_amd.trunk_exec import _Inception

ENTRIES = ["vsr_hgi_abi_version", "vsr_hgi_inception_f16", "vsr_hgi_last_error", "vsr_hgi_supported", "vsr_hgi_workgroups"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_hgi_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.HGILIB_PATH) and os.path.exists(_lib.HGIHEADER_PATH)
    assert _lib._SIDE["hgi"][:2] == (_lib.HGILIB_PATH, _lib.HGIHEADER_PATH)
    declared = _lib.declared_symbols(hgi=True)
    assert declared == ENTRIES
    assert _exported(_lib.HGILIB_PATH) == declared
    lib = _lib.load_hgi()
    assert lib.vsr_hgi_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.HGILIB_PATH], capture_output=True, text=True).stdout
    with open(_lib.HGIHEADER_PATH) as f:
        defs = dict(re.findall(r"#define (VSR_HGI_[A-Z_0-9]+) (\d+)", f.read()))
    assert (int(defs["VSR_HGI_TILE_H"]), int(defs["VSR_HGI_TILE_W"])) == (8, 16)


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, hdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(hgi=True)
    assert len(declared) == 66 and "vsr_hg_front_f16" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _exported(_lib.LIB_PATH) == declared and len(_exported(_lib.LIB_PATH)) == 66
    assert _lib.load().vsr_abi_version() == 3
    assert not set(hdeclared) & (set(declared) | set(xdeclared))
    others = [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "hgi"]
    for path in others:
        assert not [s for s in _exported(path) if s.startswith("vsr_hgi_")], path
    assert not set(_exported(_lib.HGILIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "hgi":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.HGILIB_PATH)) & set(_exported(row[0])), name


def _sig(node):
    _, cin, o0, *rest = node
    return cin, rest[0][0], tuple(k for _, k, _ in rest), rest[0][2], o0


def test_supported_signatures_are_the_blocks_a_to_g_and_the_rule_is_capped():
    lib = _lib.load_hgi()
    for node in (_A, _B, _C, _D, _E, _F, _G):
        cin, mid, ks, cout, o0 = _sig(node)
        assert lib.vsr_hgi_supported(*ks, mid, cout, o0) == 1, node
        assert all(_Inception.fused_rule(_sig(node), h, w) for h, w in ((1, 1), (33, 60), (66, 120), (67, 120))), node
        # above 67 x 120 the measured verdict keeps the four launches for every block but _B
        assert all(_Inception.fused_rule(_sig(node), h, w) == (node is _B) for h, w in ((67, 121), (132, 240), (135, 240))), node
        assert not _Inception.fused_rule(_sig(node), 135, 241) and not _Inception.fused_rule(_sig(node), 270, 480), node
        assert not _Inception.fused_rule(_sig(node), 0, 60) and not _Inception.fused_rule(_sig(node), 33, -1), node
    for node in (_H, _J):   # 16-wide outputs: the dense_thin path keeps them
        cin, mid, ks, cout, o0 = _sig(node)
        assert lib.vsr_hgi_supported(*ks, mid, cout, o0) == 0, node
        assert not _Inception.fused_rule(_sig(node), 33, 60), node
    assert lib.vsr_hgi_supported(3, 5, 9, 32, 32, 32) == 0 and lib.vsr_hgi_supported(3, 5, 7, 48, 32, 32) == 0
    assert _Inception.FUSED_MAX_PIXELS <= 135 * 240
    # what the host rule lets through, the library has a kernel for
    for cin in (128, 256):
        for mid in (32, 64):
            for ks in ((3, 5, 7), (3, 7, 11)):
                for cout in (32, 64):
                    for o0 in (32, 64):
                        if _Inception.fused_rule((cin, mid, ks, cout, o0), 33, 60):
                            assert lib.vsr_hgi_supported(*ks, mid, cout, o0) == 1, (cin, mid, ks, cout, o0)
    # workgroups: 4 per 8 x 16 tile and image
    wg = lib.vsr_hgi_workgroups
    assert wg(1, 33, 60) == 80 and wg(1, 67, 120) == 4 * 9 * 8 and wg(4, 135, 240) == 4 * 17 * 15 * 4 and wg(1, 1, 1) == 4
    assert wg(0, 8, 8) == 0 and wg(1, 0, 8) == 0 and wg(1, 8, -1) == 0 and wg(65536, 8, 8) == 0


NULL, X, OUT, W1, WK, B = (ctypes.c_void_p(v) for v in (0, 0x10000000, 0x20000000, 0x1000, 0x2000, 0x3000))


def _call(lib, x=X, in_ld=128, in_coff=0, cin=128, w1=W1, b1=B, c1_pad=128, mid=32, o0=32, wk1=WK, bk1=B, k1=3, wk2=WK, bk2=B, k2=5,
          wk3=WK, bk3=B, k3=7, cout=32, out=OUT, out_ld=128, N=1, H=33, W=60):
    return lib.vsr_hgi_inception_f16(x, in_ld, in_coff, cin, w1, b1, c1_pad, mid, o0, wk1, bk1, k1, wk2, bk2, k2, wk3, bk3, k3, cout, out,
                                     out_ld, N, H, W, NULL)


def test_inception_validates_before_any_launch():
    """Every refusal with pointers that are never dereferenced (none of them is a mapping of this process)."""
    lib = _lib.load_hgi()

    def refused(text, **kw):
        assert _call(lib, **kw) == -1, kw
        assert text in lib.vsr_hgi_last_error(), (kw, lib.vsr_hgi_last_error())

    for name in ("x", "w1", "b1", "wk1", "bk1", "wk2", "bk2", "wk3", "bk3", "out"):
        refused(b"hgi_inception: null pointer", **{name: NULL})
    for kw in ({"N": 0}, {"H": 0}, {"W": -4}, {"N": -1}):
        refused(b"hgi_inception: bad shape", **kw)
    refused(b"grid overflow (N 65536 beyond 65535)", N=65536, H=1, W=1)
    for kw in ({"k3": 9}, {"k1": 5}, {"mid": 16}, {"mid": 48}, {"cout": 16}, {"o0": 16}, {"o0": 128}, {"k2": 7, "k3": 11}):
        refused(b"hgi_inception: no kernel for k", **kw)       # (mid 32 with k 3,7,11 is no block of the hourglass)
    for kw in ({"cin": 64}, {"cin": 96}, {"cin": 512, "in_ld": 512}, {"cin": 0}):
        refused(b"hgi_inception: cin", **kw)
    for kw in ({"in_ld": 136}, {"in_coff": 8, "in_ld": 160}, {"out_ld": 144}, {"c1_pad": 144}, {"in_ld": 0}, {"in_coff": -32}, {"out_ld": -128}):
        refused(b"must be multiples of 32", **kw)
    refused(b"the input slice [32, 160) leaves its row of 128", in_coff=32)
    refused(b"the result of 128 channels leaves its row of 96", out_ld=96)
    refused(b"c1_pad 96 below the fused 1x1's 128 rows", c1_pad=96)
    for name in ("x", "out", "w1", "wk1", "wk2", "wk3"):
        refused(b"x, out and the weight slabs must be 16-byte aligned", **{name: ctypes.c_void_p(0x10000008)})
    for name in ("b1", "bk1", "bk2", "bk3"):
        refused(b"the biases must be 16-byte aligned", **{name: ctypes.c_void_p(0x3004)})
    # 4 GiB: 65535 images of 135 x 240 pixels x 128 channels of fp16
    refused(b"reaches 4 GiB", N=65535, H=135, W=240)
    refused(b"reaches 4 GiB", N=1, H=4096, W=4096)
    # overlap: out inside x, x inside out, equal bases; adjacent buffers are fine for this check (the next refusal is none: it would launch,
    # so the adjacent case is not called here)
    nbytes = 33 * 60 * 128 * 2
    refused(b"x and out overlap", out=X)
    refused(b"x and out overlap", out=ctypes.c_void_p(X.value + nbytes - 16))
    refused(b"x and out overlap", out=ctypes.c_void_p(X.value - nbytes + 16))


def test_check_reports_from_the_hgi_librarys_own_buffer():
    lib = _lib.load_hgi()
    main = _lib.load()
    before = main.vsr_last_error()
    rc = _call(lib, k3=9)
    assert main.vsr_last_error() == before          # the main library's buffer is another one
    with pytest.raises(_lib.VsrHipError, match=r"hgi_inception failed \(-1\): hgi_inception: no kernel for k \(3,5,9\) mid 32 cout 32 o0 32"):
        _lib.check(rc, "hgi_inception", lib=lib)
