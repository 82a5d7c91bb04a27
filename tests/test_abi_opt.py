"""CPU-side checks of libvsr_hip_opt.so (include/vsr_hip_opt.h): the train step's update is a library of its own, built for gfx950 by
the same `make`; it exports exactly what its header declares, the other libraries gain and lose nothing by it, the planner (pure host
code) sizes and fills the plan image, and every entry validates its arguments before any launch (no compute without a GPU)."""
import ctypes
import struct
import subprocess

import os

import pytest

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_opt_abi_version", "vsr_opt_adam_f32", "vsr_opt_grad_norm", "vsr_opt_last_error", "vsr_opt_norm_ws_bytes",
           "vsr_opt_plan_bytes", "vsr_opt_plan_fill"]
MAGIC, CHUNK = 0x3154504F, 4096
HDR, TEN, CHK = 32, 40, 8          # bytes of the image's header, of a tensor entry, of a chunk entry
MAX_CHUNKS = 2 ** 31 - 1


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def _sizes(sizes):
    return (ctypes.c_ulonglong * len(sizes))(*sizes)


def _table(sizes, base=0x100000, step=0):
    """Fake (never dereferenced) 16-byte aligned pointers, distinct per tensor and array."""
    rows, at = [], base
    for n in sizes:
        ptrs = []
        for _ in range(4):
            ptrs.append(at + step)
            at += (4 * n + 255) // 256 * 256 + 256
        rows.append(_lib.OptTensor(*ptrs, n))
    return (_lib.OptTensor * len(rows))(*rows)


def _image(L, sizes):
    nbytes = L.vsr_opt_plan_bytes(len(sizes), _sizes(sizes))
    assert nbytes > 0, L.vsr_opt_last_error()
    img = ctypes.create_string_buffer(nbytes)
    table = _table(sizes)
    assert L.vsr_opt_plan_fill(img, nbytes, len(sizes), table) == 0, L.vsr_opt_last_error()
    return img, nbytes, table


def _parse(img, nbytes):
    magic, nt, nc, reserved, total, ne = struct.unpack_from("<IiIIQQ", img.raw, 0)
    tensors = [struct.unpack_from("<QQQQQ", img.raw, HDR + TEN * i) for i in range(nt)]
    chunks = [struct.unpack_from("<II", img.raw, HDR + TEN * nt + CHK * j) for j in range(nc)]
    assert HDR + TEN * nt + CHK * nc == nbytes == total and reserved == 0
    return magic, nt, nc, ne, tensors, chunks


def test_opt_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.OPTLIB_PATH) and os.path.exists(_lib.OPTHEADER_PATH)
    assert _lib._SIDE["opt"][:2] == (_lib.OPTLIB_PATH, _lib.OPTHEADER_PATH)
    declared = _lib.declared_symbols(opt=True)
    assert declared == ENTRIES
    assert _exported(_lib.OPTLIB_PATH) == declared
    assert _lib.load_opt().vsr_opt_abi_version() == 1
    assert "gfx950" in subprocess.run(["strings", _lib.OPTLIB_PATH], capture_output=True, text=True).stdout


def test_the_other_libraries_and_headers_are_untouched_by_it():
    _lib.build()
    declared, xdeclared, odeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(opt=True)
    assert len(declared) == 66 and "vsr_frame_to_u8" in declared and "vsr_conv2d_tuning" in xdeclared
    assert _lib.declared_symbols(metric=True) == ["vsr_metric_abi_version", "vsr_metric_frames", "vsr_metric_last_error", "vsr_metric_ws_bytes"]
    assert _lib.declared_symbols(yuv=True) == ["vsr_yuv_abi_version", "vsr_yuv_ingest", "vsr_yuv_last_error", "vsr_yuv_write"]
    assert _lib.declared_symbols(grad=True) == ["vsr_grad_abi_version", "vsr_grad_channelnorm_f32", "vsr_grad_correlation_f32",
                                                "vsr_grad_last_error", "vsr_grad_resample2d_f32"]
    assert not set(odeclared) & (set(declared) | set(xdeclared))
    for path in [_lib.LIB_PATH, _lib.XLIB_PATH] + [row[0] for name, row in _lib._SIDE.items() if name != "opt"]:
        assert not [s for s in _exported(path) if s.startswith("vsr_opt_")], path
    assert not set(_exported(_lib.OPTLIB_PATH)) & (set(declared) | set(xdeclared))
    for name, row in _lib._SIDE.items():
        if name != "opt":
            assert _exported(row[0]) == _lib.declared_symbols(**{name: True}), name   # each still exports exactly its own header
            assert not set(_exported(_lib.OPTLIB_PATH)) & set(_exported(row[0])), name


def test_planner_chunks_and_entries():
    L = _lib.load_opt()
    sizes = [1, 4095, 4096, 4097, 8195, 1]
    img, nbytes, table = _image(L, sizes)
    magic, nt, nc, ne, tensors, chunks = _parse(img, nbytes)
    assert magic == MAGIC and nt == 6 and nc == 1 + 1 + 1 + 2 + 3 + 1 and ne == sum(sizes)
    assert chunks == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (5, 0)]
    assert tensors == [(r.p, r.g, r.m, r.v, r.n) for r in table]
    assert L.vsr_opt_norm_ws_bytes(img) == 8 * nc


def test_planner_round_trips_the_sr_nets_tensors():
    from video_super_resolution_amd import SRProjectionModule
    L = _lib.load_opt()
    sizes = [p.numel() for p in SRProjectionModule().parameters() if p.requires_grad]
    assert len(sizes) == 87 and sum(sizes) == 910847                    # the x4 SR net
    img, nbytes, table = _image(L, sizes)
    magic, nt, nc, ne, tensors, chunks = _parse(img, nbytes)
    assert (magic, nt, ne) == (MAGIC, 87, 910847) and nc == sum(-(-n // CHUNK) for n in sizes)
    assert tensors == [(r.p, r.g, r.m, r.v, r.n) for r in table]
    assert chunks == [(i, j) for i, n in enumerate(sizes) for j in range(-(-n // CHUNK))]
    # every element of every tensor is in exactly one chunk
    for i, n in enumerate(sizes):
        mine = [j for t, j in chunks if t == i]
        assert mine == list(range(len(mine))) and (len(mine) - 1) * CHUNK < n <= len(mine) * CHUNK


def test_every_refusal_comes_before_any_launch():
    L = _lib.load_opt()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)

    def msg():
        return L.vsr_opt_last_error()

    # ---- the planner
    one = _sizes([5])
    assert L.vsr_opt_plan_bytes(1, None) == 0 and b"opt_plan_bytes: null pointer" in msg()
    for n in (0, -2):
        assert L.vsr_opt_plan_bytes(n, one) == 0 and b"n_tensors must be positive, got %d" % n in msg()
    assert L.vsr_opt_plan_bytes(3, _sizes([4, 0, 4])) == 0 and b"tensor 1 has no elements" in msg()
    assert L.vsr_opt_plan_bytes(1, _sizes([MAX_CHUNKS * CHUNK + 1])) == 0 and b"too many chunks for one grid" in msg()
    assert L.vsr_opt_plan_bytes(2, _sizes([MAX_CHUNKS * CHUNK, 1])) == 0 and b"too many chunks for one grid" in msg()
    assert L.vsr_opt_plan_bytes(1, _sizes([2 ** 64 - 1])) == 0 and b"too many chunks for one grid" in msg()
    assert L.vsr_opt_plan_bytes(2, _sizes([2 ** 33 + 1, 7])) == HDR + 2 * TEN + CHK * (2 ** 21 + 2)      # 64-bit sizes are fine

    sizes = [5, 4097]
    nbytes = L.vsr_opt_plan_bytes(2, _sizes(sizes))
    assert nbytes == HDR + 2 * TEN + 3 * CHK
    img = ctypes.create_string_buffer(nbytes)
    good = _table(sizes)
    assert L.vsr_opt_plan_fill(None, nbytes, 2, good) == -1 and b"opt_plan_fill: null pointer" in msg()
    assert L.vsr_opt_plan_fill(img, nbytes, 2, None) == -1 and b"opt_plan_fill: null pointer" in msg()
    for n in (0, -1):
        assert L.vsr_opt_plan_fill(img, nbytes, n, good) == -1 and b"n_tensors must be positive" in msg()
    for field in ("p", "g", "m", "v"):
        bad = _table(sizes)
        setattr(bad[1], field, 0)
        assert L.vsr_opt_plan_fill(img, nbytes, 2, bad) == -1 and b"tensor 1 has a null pointer" in msg(), field
        for off in (1, 2, 3):
            bad = _table(sizes)
            setattr(bad[0], field, getattr(bad[0], field) + off)
            assert L.vsr_opt_plan_fill(img, nbytes, 2, bad) == -1 and b"tensor 0: every pointer must be 4-byte aligned" in msg(), (field, off)
    bad = _table(sizes)
    bad[0].n = 0
    assert L.vsr_opt_plan_fill(img, nbytes, 2, bad) == -1 and b"tensor 0 has no elements" in msg()
    bad = _table(sizes)
    bad[1].n = MAX_CHUNKS * CHUNK
    assert L.vsr_opt_plan_fill(img, nbytes, 2, bad) == -1 and b"too many chunks for one grid" in msg()
    for wrong in (nbytes - 8, nbytes + 8, 0):
        assert L.vsr_opt_plan_fill(img, wrong, 2, good) == -1 and b"image of the wrong size" in msg(), wrong
    assert img.raw == b"\0" * nbytes                                    # a refused fill writes nothing
    assert L.vsr_opt_plan_fill(img, nbytes, 2, _table(sizes, step=4)) == 0   # 4-byte alignment is enough
    assert L.vsr_opt_plan_fill(img, nbytes, 2, good) == 0

    # ---- the launch entries (a null stream and fake device pointers: nothing may be launched)
    sc = [0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8, 0.0]

    def adam(host=img, dev=fake, ctl=null):
        return L.vsr_opt_adam_f32(host, dev, ctl, *sc, null)

    def norm(host=img, dev=fake, max_norm=1.0, ctl=fake, ws=fake):
        return L.vsr_opt_grad_norm(host, dev, max_norm, ctl, ws, null)

    def damaged(offset, fmt, value):
        b = ctypes.create_string_buffer(img.raw, nbytes)
        struct.pack_into(fmt, b, offset, value)
        return b

    for call, name in ((adam, b"opt_adam_f32"), (norm, b"opt_grad_norm")):
        assert call(host=null) == -1 and name + b": null plan" in msg()
        assert call(dev=null) == -1 and name + b": null plan" in msg()
        assert call(host=damaged(0, "<I", MAGIC ^ 1)) == -1 and name + b": not a plan image (magic 0x3154504e)" in msg()
        assert call(host=ctypes.create_string_buffer(nbytes)) == -1 and name + b": not a plan image" in msg()
        for off, fmt, val in ((4, "<i", 3), (4, "<i", 0), (8, "<I", 4), (8, "<I", 0), (12, "<I", 1), (16, "<Q", nbytes + 8)):
            assert call(host=damaged(off, fmt, val)) == -1 and name + b": plan image of the wrong size" in msg(), (off, val)
        assert call(dev=ctypes.c_void_p(0x1004)) == -1 and name + b": the device plan must be 8-byte aligned" in msg()
    assert adam(ctl=ctypes.c_void_p(0x1002)) == -1 and b"opt_adam_f32: ctl must be 4-byte aligned" in msg()
    assert norm(ctl=null) == -1 and b"opt_grad_norm: null pointer" in msg()
    assert norm(ws=null) == -1 and b"opt_grad_norm: null pointer" in msg()
    assert norm(ctl=ctypes.c_void_p(0x1004)) == -1 and b"ctl and the workspace must be 8-byte aligned" in msg()
    assert norm(ws=ctypes.c_void_p(0x1004)) == -1 and b"ctl and the workspace must be 8-byte aligned" in msg()
    for bad_norm in (0.0, -1.0, float("nan")):
        assert norm(max_norm=bad_norm) == -1 and b"max_norm must be positive" in msg(), bad_norm
    # the workspace: one double per chunk; 0 for an image the launch would refuse
    assert L.vsr_opt_norm_ws_bytes(img) == 3 * 8
    assert L.vsr_opt_norm_ws_bytes(damaged(0, "<I", 0)) == 0 and L.vsr_opt_norm_ws_bytes(None) == 0


def test_check_reports_from_the_opt_librarys_own_buffer():
    L = _lib.load_opt()
    rc = L.vsr_opt_plan_fill(None, 0, 1, None)
    with pytest.raises(_lib.VsrHipError, match=r"opt_plan_fill failed \(-1\): opt_plan_fill: null pointer"):
        _lib.check(rc, "opt_plan_fill", lib=L)
    _lib.load_metric().vsr_metric_ws_bytes(0, 0, 0, 0, 0)                 # another library's message does not leak into this one's
    assert b"opt_plan_fill" in L.vsr_opt_last_error()
