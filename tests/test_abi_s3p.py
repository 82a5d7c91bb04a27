"""CPU-side checks of libvsr_hip_s3p.so (include/vsr_hip_s3p.h): the x3 stage with the next group's uptran slice inside the launch is
a library of its own, built for gfx950 by the same `make`; it exports exactly what its header declares, the five other libraries
export what their headers declare and nothing of it, its entry validates its arguments before any launch (no compute without a GPU),
the host-side packer produces a blob of the size the library reports whose stage part IS the plain stage's blob, and a float64
restatement of the kernel's four quadrant products on the DECODED blob equals conv2d 1x1 + PReLU (fragment order, channel order and
parameter block are right before the first GPU run)."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from video_super_resolution_amd import _lib

ENTRIES = ["vsr_s3p_abi_version", "vsr_s3p_last_error", "vsr_s3p_query", "vsr_s3p_sr_utd_post_f16"]
POST_BYTES = 2048 + 256


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_s3p_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.S3PLIB_PATH)
    declared = _lib.declared_symbols(s3p=True)
    assert declared == ENTRIES
    assert _exported(_lib.S3PLIB_PATH) == declared
    lib = _lib.load_s3p()
    assert lib.vsr_s3p_abi_version() == 1
    assert lib.vsr_s3p_query(_lib.Q_S3P_STRIP_WIDTH) == 30 == _lib.load_s3().vsr_s3_query(_lib.Q_S3_STRIP_WIDTH)
    assert lib.vsr_s3p_query(_lib.Q_S3P_BLOB_BYTES) == _lib.load_s3().vsr_s3_query(_lib.Q_S3_BLOB_BYTES) + POST_BYTES
    assert lib.vsr_s3p_query(99) == 0
    assert "gfx950" in subprocess.run(["strings", _lib.S3PLIB_PATH], capture_output=True, text=True).stdout


def test_the_other_five_libraries_export_what_their_headers_declare():
    _lib.build()
    declared, xdeclared, gdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True), _lib.declared_symbols(grad=True)
    s3declared, s3tdeclared, s3pdeclared = _lib.declared_symbols(s3=True), _lib.declared_symbols(s3t=True), _lib.declared_symbols(s3p=True)
    assert len(declared) == 66 and len(gdeclared) == 5 and len(s3declared) == 4 and len(s3tdeclared) == 5
    assert not set(s3pdeclared) & (set(declared) | set(xdeclared) | set(gdeclared) | set(s3declared) | set(s3tdeclared))
    assert _exported(_lib.LIB_PATH) == declared
    assert _exported(_lib.XLIB_PATH) == sorted(set(declared) | set(xdeclared))
    assert _exported(_lib.GLIB_PATH) == gdeclared
    assert _exported(_lib.S3LIB_PATH) == s3declared
    assert _exported(_lib.S3TLIB_PATH) == s3tdeclared
    for path in (_lib.LIB_PATH, _lib.XLIB_PATH, _lib.GLIB_PATH, _lib.S3LIB_PATH, _lib.S3TLIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("vsr_s3p_")], path
    assert not [s for s in _exported(_lib.S3PLIB_PATH) if not s.startswith("vsr_s3p_")]


def _kernel_names(path):
    out = subprocess.run(["strings", path], capture_output=True, text=True, check=True).stdout
    return set(ln for ln in out.splitlines() if "k_utd_s3" in ln)


def test_the_plain_library_holds_no_post_kernel_and_the_post_library_no_plain_one():
    """One kernel text (csrc/sr_utd_s3.h), two libraries: each holds only its own instantiations."""
    _lib.build()
    assert not [s for s in _kernel_names(_lib.S3LIB_PATH) if "k_utd_s3_post" in s]
    post = _kernel_names(_lib.S3PLIB_PATH)
    assert post and all("k_utd_s3_post" in s for s in post)


# never dereferenced on the host: far apart, so that no range of a refused shape reaches from one into another
_NULL = ctypes.c_void_p(0)
_IN, _BLOB, _OUT, _POST = (ctypes.c_void_p(0x100000000000 * (i + 1)) for i in range(4))


def test_s3p_entry_validates_before_any_launch():
    S = _lib.load_s3p()
    fn = S.vsr_s3p_sr_utd_post_f16

    def msg():
        return S.vsr_s3p_last_error()

    for args in ((_NULL, _BLOB, _OUT, _POST), (_IN, _NULL, _OUT, _POST), (_IN, _BLOB, _NULL, _POST), (_IN, _BLOB, _OUT, _NULL)):
        assert fn(*args, 1, 4, 4, 4, 1, _NULL) == -1 and b"null" in msg()
    for N, h, w, rps in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, -3, 4), (1, 4, 4, -1), (70000, 4, 4, 4)):
        assert fn(_IN, _BLOB, _OUT, _POST, N, h, w, rps, 1, _NULL) == -1 and b"bad shape" in msg(), (N, h, w, rps)
    off8 = lambda p: ctypes.c_void_p(p.value + 8)
    for args in ((off8(_IN), _BLOB, _OUT, _POST), (_IN, off8(_BLOB), _OUT, _POST), (_IN, _BLOB, off8(_OUT), _POST), (_IN, _BLOB, _OUT, off8(_POST))):
        assert fn(*args, 1, 4, 4, 4, 1, _NULL) == -1 and b"aligned" in msg()
    # overlap as a RANGE check on the three tensors (1 x 4 x 4 x 64 B = 1024 B each): the same address, one starting inside another,
    # one ending inside another -- for every pair
    inside = lambda p: ctypes.c_void_p(p.value + 1008)
    before = lambda p: ctypes.c_void_p(p.value - 16)
    for shift in (lambda p: p, inside, before):
        assert fn(_IN, _BLOB, shift(_IN), _POST, 1, 4, 4, 4, 1, _NULL) == -1 and b"overlap" in msg()
        assert fn(_IN, _BLOB, _OUT, shift(_IN), 1, 4, 4, 4, 1, _NULL) == -1 and b"overlap" in msg()
        assert fn(_IN, _BLOB, _OUT, shift(_OUT), 1, 4, 4, 4, 1, _NULL) == -1 and b"overlap" in msg()
    assert fn(_IN, _BLOB, _BLOB, _POST, 1, 4, 4, 4, 1, _NULL) == -1 and b"overlap" in msg()       # an output over the weights
    # ... and every pair of the four, the blob among them, with the same three shifts
    bufs = (_IN, _BLOB, _OUT, _POST)
    for i in range(4):
        for j in range(i + 1, 4):
            for shift in (lambda p: p, inside, before):
                args = list(bufs)
                args[j] = shift(bufs[i])
                assert fn(*args, 1, 4, 4, 4, 1, _NULL) == -1 and b"overlap" in msg(), (i, j)
    assert fn(_IN, _BLOB, _OUT, _POST, 8, 3000, 3000, 16, 1, _NULL) == -3 and b"4 GiB" in msg() and b"split the planes" in msg()
    assert fn(_IN, _BLOB, _OUT, _POST, 1, 70000, 8, 1, 1, _NULL) == -1 and b"row segments" in msg()


def test_check_reports_from_the_s3p_librarys_own_buffer():
    S = _lib.load_s3p()
    rc = S.vsr_s3p_sr_utd_post_f16(_IN, _BLOB, _OUT, _POST, 1, 4, 0, 4, 1, None)
    with pytest.raises(_lib.VsrHipError, match=r"sr_utd_s3_post_f16 failed \(-1\): s3p_sr_utd_post: bad shape \(N 1, h 4, w 0, rows_per_seg 4\)"):
        _lib.check(rc, "sr_utd_s3_post_f16", lib=S)
    # ... and the plain stage's library keeps its own message
    P = _lib.load_s3()
    P.vsr_s3_sr_utd_f16(_IN, _BLOB, _OUT, 1, 0, 4, 4, 1, None)
    assert b"s3_sr_utd:" in P.vsr_s3_last_error() and b"s3p_sr_utd_post" in S.vsr_s3p_last_error()


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    up_w, dn_w = torch.randn(32, 32, 7, 7, generator=g), torch.randn(32, 32, 7, 7, generator=g)
    tr_w, ut_w = torch.randn(32, 96, generator=g), torch.randn(32, 192, generator=g)
    b = [torch.randn(32, generator=g) for _ in range(4)]
    return up_w, dn_w, tr_w, ut_w, b


def test_pack_utd_s3_post_blob_has_the_queried_size_the_plain_stage_part_and_the_headers_post_section():
    from video_super_resolution_amd.sr_pack import pack_utd_s3_blob, pack_utd_s3_post_blob
    up_w, dn_w, tr_w, ut_w, b = _operands()
    args = (up_w, b[0], 0.25, tr_w, 32, b[1], 0.5, dn_w, b[2], -0.75)
    blob = pack_utd_s3_post_blob(*args, post=(ut_w, 128, b[3], 1.5))
    plain = pack_utd_s3_blob(*args)
    assert blob.dtype == torch.uint8 and blob.numel() == _lib.load_s3p().vsr_s3p_query(_lib.Q_S3P_BLOB_BYTES)
    assert plain.numel() == _lib.load_s3().vsr_s3_query(_lib.Q_S3_BLOB_BYTES) and blob.numel() == plain.numel() + POST_BYTES
    assert torch.equal(blob[:plain.numel()], plain)
    frag = blob[plain.numel():plain.numel() + 2048].view(torch.float16).view(2, 64, 8)
    for mt, lane, j in ((0, 0, 0), (1, 37, 5), (0, 63, 7), (1, 16, 0)):     # natural channel order: ci = col0 + 8 (lane / 16) + j
        assert frag[mt, lane, j] == ut_w[16 * mt + (lane & 15), 128 + 8 * (lane >> 4) + j].half(), (mt, lane, j)
    ppar = blob[plain.numel() + 2048:].view(torch.float32)
    assert ppar.numel() == 64 and torch.equal(ppar[:32], b[3]) and ppar[32] == 1.5 and not ppar[33:].any()
    # the plain packer keeps refusing `post=`
    with pytest.raises(NotImplementedError):
        pack_utd_s3_blob(*args, post=(ut_w, 128, b[3], 1.5))


@pytest.mark.parametrize("slope", [0.25, -0.5, 1.5])
def test_float64_restatement_of_the_quadrant_products_on_the_decoded_blob(slope):
    """Wave wv multiplies out-channel tile pmt = wv / 2 with pixel tile wv % 2: A[row = lane % 16][k = 8 (lane / 16) + j] from the blob's
    POST section, B[k][col = lane % 16] = the output row's pixel 16 (wv % 2) + col, channels 8 (lane / 16) .. + 7 as they lie in memory,
    C = the bias of channels 16 pmt + 4 (lane / 16) .. + 3; lane (col, g) then holds channels 16 pmt + 4 g + e of its pixel."""
    from video_super_resolution_amd.sr_pack import pack_utd_s3_post_blob
    up_w, dn_w, tr_w, ut_w, b = _operands(1)
    # operands of the 1x1 as multiples of 2^-10 below 2: fp16 values whose products are multiples of 2^-20, so every 32-term sum (< 2^8) is
    # exact in float64 in ANY order, while it has more bits than fp16 keeps: the two roundings are exercised and the comparison is an equality
    q = lambda t: (t.clamp(-1.99, 1.99) * 1024).round() / 1024
    ut_w, b[3] = q(ut_w * 0.5), q(b[3])
    blob = pack_utd_s3_post_blob(up_w, b[0], 0.25, tr_w, 32, b[1], 0.5, dn_w, b[2], 0.5, post=(ut_w, 128, b[3], slope))
    o_p = blob.numel() - POST_BYTES
    frag = blob[o_p:o_p + 2048].view(torch.float16).view(2, 64, 8).double()
    ppar = blob[o_p + 2048:].view(torch.float32).double()
    g = torch.Generator().manual_seed(2)
    row = q(torch.randn(32, 32, generator=g)).double()              # [pixel 32][channel 32]: one finished output row of a strip
    assert torch.equal(row.half().double(), row) and torch.equal(ut_w.half().float(), ut_w)
    got = torch.full((32, 32), float("nan"), dtype=torch.float64)   # [pixel][out channel]
    for wv in range(4):
        pmt, pt = wv >> 1, wv & 1
        A = torch.zeros(16, 32, dtype=torch.float64)
        Bm = torch.zeros(32, 16, dtype=torch.float64)
        for lane in range(64):
            l15, gg = lane & 15, lane >> 4
            A[l15, 8 * gg:8 * gg + 8] = frag[pmt, lane]
            Bm[8 * gg:8 * gg + 8, l15] = row[16 * pt + l15, 8 * gg:8 * gg + 8]
        D = A @ Bm                                                   # D[row i][col]: lane (col, g) holds rows 4 g .. 4 g + 3
        for lane in range(64):
            l15, gg = lane & 15, lane >> 4
            for e in range(4):
                got[16 * pt + l15, 16 * pmt + 4 * gg + e] = D[4 * gg + e, l15] + ppar[16 * pmt + 4 * gg + e]
    assert not torch.isnan(got).any()
    prelu16 = lambda v, a: (lambda q: torch.where(q >= 0, q, (q * a).half().double()))(v.half().double())
    got = prelu16(got, float(ppar[32]))
    x = row.t().reshape(1, 32, 1, 32)
    want = prelu16(F.conv2d(x, ut_w[:, 128:160].half().double().view(32, 32, 1, 1), b[3].double()), slope)[0, :, 0].t()
    assert want.unique().numel() > 500          # (a live case: a thousand outputs, hardly two alike)
    assert torch.equal(got, want)
