"""CPU-side checks of libvsr_hip_s3f.so (include/vsr_hip_s3f.h): the x3 stage with the step-opening 1x1 chain folded into its LR load
path is a library of its own, built for gfx950 by the same `make`; it exports exactly what its header declares, the six other libraries
export what their headers declare and nothing of it, each of the three stage libraries holds only its own instantiations of the one
kernel text, the entry validates its arguments before any launch (no compute without a GPU), the host-side packer produces a blob of
the size the library reports whose first part IS the POST build's blob, and a float64 restatement of the folded chain on the DECODED
PRE section -- the MFMA operand lanes of csrc/sr_utd_s3.h, both modes -- equals conv2d 1x1 + PReLU chains."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from video_super_resolution_amd import _lib
from video_super_resolution_amd._lib import load_s3f  # (absent without the feature: the module fails at import)

ENTRIES = ["vsr_s3f_abi_version", "vsr_s3f_last_error", "vsr_s3f_query", "vsr_s3f_sr_utd_pre_f16"]
PRE_BYTES = 12 * 1024 + 512


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


def test_s3f_library_builds_and_exports_exactly_what_its_header_declares():
    _lib.build()
    assert os.path.exists(_lib.S3FLIB_PATH)
    declared = _lib.declared_symbols(s3f=True)
    assert declared == ENTRIES
    assert _exported(_lib.S3FLIB_PATH) == declared
    lib = load_s3f()
    assert lib.vsr_s3f_abi_version() == 1
    assert lib.vsr_s3f_query(_lib.Q_S3F_STRIP_WIDTH) == 30 == _lib.load_s3().vsr_s3_query(_lib.Q_S3_STRIP_WIDTH)
    assert lib.vsr_s3f_query(_lib.Q_S3F_BLOB_BYTES) == _lib.load_s3p().vsr_s3p_query(_lib.Q_S3P_BLOB_BYTES) + PRE_BYTES
    assert lib.vsr_s3f_query(99) == 0
    assert "gfx950" in subprocess.run(["strings", _lib.S3FLIB_PATH], capture_output=True, text=True).stdout


def test_all_seven_libraries_export_what_their_headers_declare():
    _lib.build()
    D = _lib.declared_symbols
    declared, xdeclared = D(), D(xcheck=True)
    own = {_lib.GLIB_PATH: D(grad=True), _lib.S3LIB_PATH: D(s3=True), _lib.S3TLIB_PATH: D(s3t=True), _lib.S3PLIB_PATH: D(s3p=True),
           _lib.S3FLIB_PATH: D(s3f=True)}
    assert len(declared) == 66 and [len(v) for v in own.values()] == [5, 4, 5, 4, 4]
    assert _exported(_lib.LIB_PATH) == declared
    assert _exported(_lib.XLIB_PATH) == sorted(set(declared) | set(xdeclared))
    for path, syms in own.items():
        assert _exported(path) == syms, path
    s3f = set(own[_lib.S3FLIB_PATH])
    assert not s3f & (set(declared) | set(xdeclared))
    for path, syms in own.items():
        if path != _lib.S3FLIB_PATH:
            assert not s3f & set(syms)
            assert not [s for s in _exported(path) if s.startswith("vsr_s3f_")], path
    for path in (_lib.LIB_PATH, _lib.XLIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("vsr_s3f_")], path
    assert not [s for s in _exported(_lib.S3FLIB_PATH) if not s.startswith("vsr_s3f_")]


def _kernel_names(path):
    out = subprocess.run(["strings", path], capture_output=True, text=True, check=True).stdout
    return set(ln for ln in out.splitlines() if "k_utd_s3" in ln)


def test_each_stage_library_holds_only_its_own_instantiations():
    """One kernel text (csrc/sr_utd_s3.h), three libraries: plain, POST, PRE (with and without POST)."""
    _lib.build()
    plain, post, pre = (_kernel_names(p) for p in (_lib.S3LIB_PATH, _lib.S3PLIB_PATH, _lib.S3FLIB_PATH))
    assert plain and not [s for s in plain if "k_utd_s3_post" in s or "k_utd_s3_pre" in s]
    assert post and all("k_utd_s3_post" in s for s in post)
    assert pre and all("k_utd_s3_pre" in s for s in pre)
    # max / select build x with / without POST
    for inst in ("k_utd_s3_preILb1ELb1EE", "k_utd_s3_preILb0ELb1EE", "k_utd_s3_preILb1ELb0EE", "k_utd_s3_preILb0ELb0EE"):
        assert [s for s in pre if inst in s], inst
    for path in (_lib.LIB_PATH, _lib.XLIB_PATH, _lib.GLIB_PATH, _lib.S3TLIB_PATH):
        assert not [s for s in _kernel_names(path) if "k_utd_s3_pre" in s], path


# never dereferenced on the host: far apart, so that no range of a refused shape reaches from one into another
_NULL = ctypes.c_void_p(0)
_FEAT, _A, _B, _CMAP, _BLOB, _OUT, _POST = (ctypes.c_void_p(0x100000000000 * (i + 1)) for i in range(7))
_ALL = (_FEAT, _A, _B, _CMAP, _BLOB, _OUT, _POST)
_NAMES = ("feat", "a", "b", "cmap", "blob", "out", "out_post")


def _with(**kw):
    return tuple(kw.get(n, p) for n, p in zip(_NAMES, _ALL))


def test_s3f_entry_validates_before_any_launch():
    S = load_s3f()
    fn = S.vsr_s3f_sr_utd_pre_f16
    msg = S.vsr_s3f_last_error
    tail = (1, 4, 4, 4, 1, _NULL)
    for name in ("feat", "blob", "out"):
        assert fn(*_with(**{name: _NULL}), *tail) == -1 and b"null" in msg(), name
    # a, b, cmap: all three (PRE3) or none (PRE2)
    for missing in (("a",), ("b",), ("cmap",), ("a", "b"), ("a", "cmap"), ("b", "cmap")):
        assert fn(*_with(**{n: _NULL for n in missing}), *tail) == -1 and b"given together" in msg(), missing
    for N, h, w, rps in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, -3, 4), (1, 4, 4, -1), (70000, 4, 4, 4)):
        for args in (_ALL, _with(a=_NULL, b=_NULL, cmap=_NULL), _with(out_post=_NULL)):
            assert fn(*args, N, h, w, rps, 1, _NULL) == -1 and b"bad shape" in msg(), (N, h, w, rps)
    off8 = lambda p: ctypes.c_void_p(p.value + 8)
    for name, p in zip(_NAMES, _ALL):
        assert fn(*_with(**{name: off8(p)}), *tail) == -1 and b"aligned" in msg(), name
    # overlap as a RANGE check (1 x 4 x 4 x 64 B = 1024 B per tensor, 2048 B of constant map): the same address, one starting inside
    # another, one ending inside another -- for every pair of the seven
    inside = lambda p: ctypes.c_void_p(p.value + 1008)
    before = lambda p: ctypes.c_void_p(p.value - 16)
    for i, (ni, pi) in enumerate(zip(_NAMES, _ALL)):
        for nj, pj in list(zip(_NAMES, _ALL))[i + 1:]:
            for shift in (lambda p: p, inside, before):
                assert fn(*_with(**{nj: shift(pi)}), *tail) == -1 and b"overlap" in msg(), (ni, nj)
    assert fn(*_with(out=ctypes.c_void_p(_CMAP.value + 2032)), *tail) == -1 and b"overlap" in msg()     # the map is 2048 bytes long
    # ... PRE2 and the build without POST check what they are given
    assert fn(*_with(a=_NULL, b=_NULL, cmap=_NULL, out=_FEAT), *tail) == -1 and b"overlap" in msg()
    assert fn(*_with(out_post=_NULL, out=inside(_B)), *tail) == -1 and b"overlap" in msg()
    for args in (_ALL, _with(a=_NULL, b=_NULL, cmap=_NULL), _with(out_post=_NULL)):
        assert fn(*args, 8, 3000, 3000, 16, 1, _NULL) == -3 and b"4 GiB" in msg() and b"split the planes" in msg()
        assert fn(*args, 1, 70000, 8, 1, 1, _NULL) == -1 and b"row segments" in msg()


def test_check_reports_from_the_s3f_librarys_own_buffer():
    S = load_s3f()
    rc = S.vsr_s3f_sr_utd_pre_f16(*_ALL, 1, 4, 0, 4, 1, None)
    with pytest.raises(_lib.VsrHipError, match=r"sr_utd_s3_pre_f16 failed \(-1\): s3f_sr_utd_pre: bad shape \(N 1, h 4, w 0, rows_per_seg 4\)"):
        _lib.check(rc, "sr_utd_s3_pre_f16", lib=S)
    # ... and the POST library keeps its own message
    P = _lib.load_s3p()
    P.vsr_s3p_sr_utd_post_f16(_FEAT, _BLOB, _OUT, _POST, 1, 0, 4, 4, 1, None)
    assert b"s3p_sr_utd_post:" in P.vsr_s3p_last_error() and b"s3f_sr_utd_pre" in S.vsr_s3f_last_error()


# operands as multiples of 2^-10 below 2: fp16 values whose products are multiples of 2^-20 or, after a rounding to fp16, of 2^-34 at the
# least; every sum of the chain (< 2^9) is then exact in float64 in ANY order, while it has more bits than fp16 keeps
_q = lambda t: (t.clamp(-1.99, 1.99) * 1024).round() / 1024


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    up_w, dn_w = torch.randn(32, 32, 7, 7, generator=g), torch.randn(32, 32, 7, 7, generator=g)
    tr_w, post_w = torch.randn(32, 96, generator=g), torch.randn(32, 192, generator=g)
    b = [torch.randn(32, generator=g) for _ in range(4)]
    co_w, ci_w, ut_w = _q(torch.randn(32, 192, generator=g) * 0.4), _q(torch.randn(32, 64, generator=g) * 0.4), _q(torch.randn(32, 64, generator=g) * 0.5)
    pb = [_q(torch.randn(32, generator=g)) for _ in range(3)]
    return (up_w, b[0], 0.25, tr_w, 32, b[1], 0.5, dn_w, b[2], -0.75), (post_w, 128, b[3], 1.5), (co_w, ci_w, ut_w, pb)


def _pack(slopes, seed=0):
    from video_super_resolution_amd.sr_pack import pack_utd_s3_post_blob, pack_utd_s3_pre_blob
    stage, post, (co_w, ci_w, ut_w, pb) = _operands(seed)
    post_blob = pack_utd_s3_post_blob(*stage, post=post)
    blob = pack_utd_s3_pre_blob(post_blob, (co_w, (64, 160), pb[0], slopes[0]), (ci_w, pb[1], slopes[1]), (ut_w, 32, pb[2], slopes[2]))
    return post_blob, blob, (co_w, ci_w, ut_w, pb)


def test_pack_utd_s3_pre_blob_has_the_queried_size_the_post_blob_and_the_headers_pre_section():
    post_blob, blob, (co_w, ci_w, ut_w, pb) = _pack((0.25, -0.5, 1.5))
    assert blob.dtype == torch.uint8 and blob.numel() == load_s3f().vsr_s3f_query(_lib.Q_S3F_BLOB_BYTES) == post_blob.numel() + PRE_BYTES
    assert post_blob.numel() == _lib.load_s3p().vsr_s3p_query(_lib.Q_S3P_BLOB_BYTES)
    assert torch.equal(blob[:post_blob.numel()], post_blob)
    o = post_blob.numel()
    frag = blob[o:o + 12 * 1024].view(torch.float16).view(6, 2, 64, 8)
    acc = lambda g, j: 4 * g + j if j < 4 else 16 + 4 * g + j - 4
    for mt, lane, j in ((0, 0, 0), (1, 37, 5), (0, 63, 7), (1, 16, 0), (0, 21, 4)):
        r, g = 16 * mt + (lane & 15), lane >> 4
        assert frag[0, mt, lane, j] == co_w[r, 64 + 8 * g + j].half()
        assert frag[1, mt, lane, j] == co_w[r, 160 + 8 * g + j].half()
        assert frag[2, mt, lane, j] == ci_w[r, 8 * g + j].half()
        assert frag[3, mt, lane, j] == ci_w[r, 32 + acc(g, j)].half()
        assert frag[4, mt, lane, j] == ut_w[r, 32 + acc(g, j)].half()
        assert frag[5, mt, lane, j] == ci_w[r, 32 + 8 * g + j].half()
    par = blob[o + 12 * 1024:].view(torch.float32)
    assert par.numel() == 128 and all(torch.equal(par[32 * i:32 * i + 32], pb[i]) for i in range(3))
    assert par[96:99].tolist() == [0.25, -0.5, 1.5] and not par[99:].any()


def _mfma(A_frag, B_lanes, C_lanes):
    """One 16x16x32 MFMA in float64 on operands as the 64 lanes hold them: A_frag [64][8] (row lane % 16, k = 8 (lane / 16) + j),
    B_lanes [64][8] (col lane % 16, same k), C_lanes [64][4] (col lane % 16, rows 4 (lane / 16) + e) -> D in C's layout."""
    A = torch.zeros(16, 32, dtype=torch.float64)
    Bm = torch.zeros(32, 16, dtype=torch.float64)
    for lane in range(64):
        l15, g = lane & 15, lane >> 4
        A[l15, 8 * g:8 * g + 8] = A_frag[lane]
        Bm[8 * g:8 * g + 8, l15] = B_lanes[lane]
    D = A @ Bm
    out = C_lanes.clone()
    for lane in range(64):
        l15, g = lane & 15, lane >> 4
        out[lane] += D[4 * g:4 * g + 4, l15]
    return out


_prelu16 = lambda v, a: (lambda q: torch.where(q >= 0, q, (q * a).half().double()))(v.half().double())


@pytest.mark.parametrize("slopes", [(0.25, 0.25, 0.25), (-0.5, 1.5, 0.25), (1.5, 0.5, -0.75)])
@pytest.mark.parametrize("mode", ["PRE3", "PRE2"])
def test_float64_restatement_of_the_folded_chain_on_the_decoded_blob(mode, slopes):
    """The kernel's pre_row (csrc/sr_utd_s3.h) on one 16-pixel tile, lane by lane: lane (l15, g) holds chunk g of pixel l15 of every
    memory input; an accumulator pair (c0, c1) holds channels 4 g + e and 16 + 4 g + e; act_pack makes of it the lane's B operand of the
    next 1x1 (k index (g, j) <-> the accumulator's channel order).  PRE2 reads the blob's sixth matrix where PRE3 reads its fourth."""
    post_blob, blob, (co_w, ci_w, ut_w, pb) = _pack(slopes, seed=3)
    o = post_blob.numel()
    frag = blob[o:o + 12 * 1024].view(torch.float16).view(12, 64, 8).double()
    par = blob[o + 12 * 1024:].view(torch.float32).double()
    g_ = torch.Generator().manual_seed(7)
    feat, a, b = (_q(torch.randn(16, 32, generator=g_)).double() for _ in range(3))       # [pixel][channel]
    cmap = _q(torch.randn(16, 32, generator=g_)).double()
    for t in (feat, a, b):
        assert torch.equal(t.half().double(), t)
    lanes = torch.arange(64)
    l15, g = lanes & 15, lanes >> 4
    chunk = lambda t: torch.stack([t[l15[i], 8 * g[i]:8 * g[i] + 8] for i in range(64)])                                 # B operand from memory
    accl = lambda v, mt: torch.stack([v[16 * mt + 4 * g[i]:16 * mt + 4 * g[i] + 4] for i in range(64)])                    # per-channel vector -> C
    accpx = lambda t, mt: torch.stack([t[l15[i], 16 * mt + 4 * g[i]:16 * mt + 4 * g[i] + 4] for i in range(64)])           # per-pixel map -> C
    bias = lambda s, mt: accl(par[32 * s:32 * s + 32], mt)
    pack = lambda c0, c1, slope: torch.cat((_prelu16(c0, slope), _prelu16(c1, slope)), dim=1)                              # act_pack
    f = chunk(feat)
    fr = list(range(10))
    if mode == "PRE3":
        c = [bias(0, mt) + accpx(cmap, mt) for mt in range(2)]
        c = [_mfma(frag[0 + mt], chunk(a), c[mt]) for mt in range(2)]
        c = [_mfma(frag[2 + mt], chunk(b), c[mt]) for mt in range(2)]
        prev = pack(c[0], c[1], float(par[96]))
    else:
        prev = f
        fr[6], fr[7] = 10, 11
    c = [_mfma(frag[fr[4 + mt]], f, bias(1, mt)) for mt in range(2)]
    c = [_mfma(frag[fr[6 + mt]], prev, c[mt]) for mt in range(2)]
    prev = pack(c[0], c[1], float(par[97]))
    c = [_mfma(frag[fr[8 + mt]], prev, bias(2, mt)) for mt in range(2)]
    prev = pack(c[0], c[1], float(par[98]))
    got = torch.full((16, 32), float("nan"), dtype=torch.float64)       # the two 8-byte ring pieces of every lane
    for i in range(64):
        got[l15[i], 4 * g[i]:4 * g[i] + 4] = prev[i, :4]
        got[l15[i], 16 + 4 * g[i]:16 + 4 * g[i] + 4] = prev[i, 4:]
    assert not torch.isnan(got).any()
    # ---- conv2d 1x1 + PReLU chains on the module's matrices
    img = lambda t: t.t().reshape(1, 32, 1, 16)
    c1 = lambda x, wm, bb: F.conv2d(x, wm.half().double().view(32, -1, 1, 1), bb)
    if mode == "PRE3":
        hid = c1(torch.cat((img(a), img(b)), 1), torch.cat((co_w[:, 64:96], co_w[:, 160:192]), 1), pb[0].double()) + img(cmap)
        hid = _prelu16(hid, slopes[0])
    else:
        hid = img(feat)
    lr0 = _prelu16(c1(torch.cat((img(feat), hid), 1), ci_w, pb[1].double()), slopes[1])
    want = _prelu16(c1(lr0, ut_w[:, 32:64], pb[2].double()), slopes[2])[0, :, 0].t()
    assert want.unique().numel() > 250          # (a live case: five hundred outputs, hardly two alike)
    assert torch.equal(got, want)
