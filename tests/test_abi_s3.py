"""CPU-side checks of libvsr_hip_s3.so (include/vsr_hip_s3.h): the fused x3 stage is a library of its own, built for gfx950 by
the same `make`; it exports exactly what its header declares, the three other libraries export what their headers declare and
nothing of it, the entry validates its arguments before any launch (no compute without a GPU), and the host-side packer
produces a blob of the size the library reports."""
import ctypes
import os
import subprocess

import pytest
import torch

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_s3_abi_version", "vsr_s3_last_error", "vsr_s3_query", "vsr_s3_sr_utd_f16"]


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_s3_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.S3LIB_PATH)
    declared = _lib.declared_symbols(s3=True)
    assert declared == ENTRIES
    assert _exported(_lib.S3LIB_PATH) == declared
    lib = _lib.load_s3()
    assert lib.vsr_s3_abi_version() == 1
    assert lib.vsr_s3_query(_lib.Q_S3_STRIP_WIDTH) == 30 and lib.vsr_s3_query(_lib.Q_S3_BLOB_BYTES) % 16 == 0
    assert lib.vsr_s3_query(99) == 0
    assert "gfx950" in subprocess.run(["strings", _lib.S3LIB_PATH], capture_output=True, text=True).stdout


def test_the_other_three_libraries_export_what_they_exported_before():
    _lib.build()
    declared, xdeclared, gdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(grad=True)
    s3declared = _lib.declared_symbols(s3=True)
    assert len(declared) == 66 and len(gdeclared) == 5
    assert not set(s3declared) & (set(declared) | set(xdeclared) | set(gdeclared))
    # count and names read from the headers: the shipping library exports its header, the cross-check library both headers,
    # the grad library its own -- and none of them anything of the x3 stage
    assert _exported(_lib.LIB_PATH) == declared
    assert _exported(_lib.XLIB_PATH) == sorted(set(declared) | set(xdeclared))
    assert _exported(_lib.GLIB_PATH) == gdeclared
    for path in (_lib.LIB_PATH, _lib.XLIB_PATH, _lib.GLIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("vsr_s3_")], path
    assert not set(_exported(_lib.S3LIB_PATH)) & (set(declared) | set(xdeclared) | set(gdeclared))


def test_s3_entry_validates_before_any_launch():
    S = _lib.load_s3()
    null, fake, fake2 = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)   # never dereferenced on the host
    fn = S.vsr_s3_sr_utd_f16

    def msg():
        return S.vsr_s3_last_error()

    assert fn(null, fake, fake2, 1, 4, 4, 4, 1, null) == -1 and b"null" in msg()
    assert fn(fake, null, fake2, 1, 4, 4, 4, 1, null) == -1 and b"null" in msg()
    assert fn(fake, fake, null, 1, 4, 4, 4, 1, null) == -1 and b"null" in msg()
    for N, h, w, rps in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, -3, 4), (1, 4, 4, -1), (70000, 4, 4, 4)):
        assert fn(fake, fake, fake2, N, h, w, rps, 1, null) == -1 and b"bad shape" in msg(), (N, h, w, rps)
    assert fn(ctypes.c_void_p(0x1008), fake, fake2, 1, 4, 4, 4, 1, null) == -1 and b"aligned" in msg()
    assert fn(fake, fake, fake, 1, 4, 4, 4, 1, null) == -1 and b"overlap" in msg()
    assert fn(fake, fake, fake2, 8, 3000, 3000, 16, 1, null) == -3 and b"4 GiB" in msg()
    assert fn(fake, fake, fake2, 1, 70000, 8, 1, 1, null) == -1 and b"row segments" in msg()


def test_s3_entry_refuses_overlapping_byte_ranges_for_every_pair():
    """in, blob, out as RANGES (1 x 4 x 4 x 64 B = 1024 B per tensor): the same address, one starting inside another, one ending inside
    another -- for every pair; far apart they pass every check up to the launch, which a host without a GPU refuses with another code."""
    S = _lib.load_s3()
    fn = S.vsr_s3_sr_utd_f16
    null = ctypes.c_void_p(0)
    bufs = [ctypes.c_void_p(0x100000000000 * (i + 1)) for i in range(3)]   # never dereferenced on the host
    inside = lambda p: ctypes.c_void_p(p.value + 1008)
    before = lambda p: ctypes.c_void_p(p.value - 16)
    for i in range(3):
        for j in range(i + 1, 3):
            for shift in (lambda p: p, inside, before):
                args = list(bufs)
                args[j] = shift(bufs[i])
                assert fn(*args, 1, 4, 4, 4, 1, null) == -1 and b"overlap" in S.vsr_s3_last_error(), (i, j)


def test_check_reports_from_the_s3_librarys_own_buffer():
    S = _lib.load_s3()
    fake = ctypes.c_void_p(0x1000)
    rc = S.vsr_s3_sr_utd_f16(fake, fake, ctypes.c_void_p(0x2000), 1, 4, 0, 4, 1, None)
    with pytest.raises(_lib.VsrHipError, match=r"sr_utd_s3_f16 failed \(-1\): s3_sr_utd: bad shape \(N 1, h 4, w 0, rows_per_seg 4\)"):
        _lib.check(rc, "sr_utd_s3_f16", lib=S)


def test_pack_utd_s3_blob_on_cpu_tensors_has_the_size_the_library_reports():
    from video_super_resolution_amd.sr_pack import _S3_PHASES, _s3_taps, pack_utd_s3_blob
    g = torch.Generator().manual_seed(0)
    up_w, dn_w = torch.randn(32, 32, 7, 7, generator=g), torch.randn(32, 32, 7, 7, generator=g)
    tr_w = torch.randn(32, 96, generator=g)
    b = [torch.randn(32, generator=g) for _ in range(3)]
    blob = pack_utd_s3_blob(up_w, b[0], 0.25, tr_w, 32, b[1], 0.5, dn_w, b[2], -0.75)
    assert blob.dtype == torch.uint8 and blob.numel() == _lib.load_s3().vsr_s3_query(_lib.Q_S3_BLOB_BYTES)
    # the nine phases are covered once, 49 taps in all, split 13 / 12 / 12 / 12 over the waves
    phases = [p for wave in _S3_PHASES for p in wave]
    assert sorted(phases) == [(r, c) for r in range(3) for c in range(3)]
    assert [sum(len(_s3_taps(r)) * len(_s3_taps(c)) for r, c in wave) for wave in _S3_PHASES] == [13, 12, 12, 12]
    assert sorted(k for x in range(3) for k in _s3_taps(x)) == list(range(7))
    # wave 0, slot 0 = phase (1, 1), kernel element (0, 0): the deconvolution's fragment holds W_up[ci = 8 (lane / 16) + j][co = lane % 16]
    frag = blob[:1024].view(torch.float16).view(64, 8)
    lane, j = 37, 5
    assert frag[lane, j] == up_w[8 * (lane >> 4) + j, lane & 15, 0, 0].half()
    # the parameters close the blob: three biases, three slopes
    fpar = blob[-512:].view(torch.float32)
    assert torch.equal(fpar[:32], b[0]) and torch.equal(fpar[64:96], b[2]) and fpar[96:99].tolist() == [0.25, 0.5, -0.75]
    with pytest.raises(NotImplementedError):
        pack_utd_s3_blob(up_w, b[0], 0.25, tr_w, 32, b[1], 0.5, dn_w, b[2], -0.75, post=(tr_w, 0, b[0], 0.5))
