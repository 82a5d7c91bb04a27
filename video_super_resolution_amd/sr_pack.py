"""Weight blobs of the fused SR kernels: every packer of sr.py's fp16 path (and `pack_dt_frags` of the fp32 path), written from one
vocabulary.  A blob's byte layout is a contract with a hand-scheduled kernel that reads its fragments from fixed offsets;
tests/test_sr_blob_layout.py pins every blob byte for byte.

Vocabulary.  An MFMA A fragment is [lane 64][8] fp16: lane l holds 8 consecutive K positions of one row of A (= one output channel).
  16x16x32 (k_utd, k_utd_s2, k_utd_s3, the tails): two row tiles mt; row = 16 mt + l % 16, K position (g = l / 16, j).
  32x32x16 (k_utd4, k_utd_s2w): two K blocks kb; row = l % 32, K position (kb, kh = l / 32, e).
Which input channel a K position means is one of four tables (`_k16_natural`, `_k16_acc`, `_k32_natural`, `_k32_acc`): "natural" where the
B operand comes from memory as it lies there, "acc" where it is the accumulator of the previous product used as-is.  A fragment pair is
always [2][lane 64][8]: `_rows(k)` and a table k broadcast to it whichever MFMA shape k belongs to.  All inputs are read with
`.detach().float()` and rounded to fp16 once (to nearest even, as the kernels round at load)."""
from __future__ import annotations

import torch

from . import _lib as L

_NF = 32  # the kernels are specialised for the reference's num_features


# ---------------------------------------------------------------------- K-index tables: the channel of MFMA K position (lane, j)
def _chunk_channel_order(device):
    """Channel held at position j of 16-byte chunk g in the HR ring / the MFMA k index (g, j): the accumulator of a
    16x16 MFMA gives lane group g the output rows {4g..4g+3} of tile 0 and {16+4g..16+4g+3} of tile 1, and that
    register block is used as-is as the next product's operand (csrc/sr_f16.hip)."""
    g = torch.arange(4, device=device).view(4, 1)
    j = torch.arange(8, device=device).view(1, 8)
    return torch.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))  # [4,8]


def _lane_j(device):
    return torch.arange(64, device=device).view(64, 1), torch.arange(8, device=device).view(1, 8)


def _k16_natural(device):
    """[64, 8]: channel 8 g + j."""
    lane, j = _lane_j(device)
    return 8 * (lane >> 4) + j


def _k16_acc(device):
    """[64, 8]: the 16x16 accumulator's order (_chunk_channel_order)."""
    return _chunk_channel_order(device)[torch.arange(64, device=device) >> 4]


def _k32_natural(device):
    """[kb 2, 64, 8]: channel 16 kb + 8 kh + e."""
    lane, e = _lane_j(device)
    return 16 * torch.arange(2, device=device).view(2, 1, 1) + 8 * (lane >> 5) + e


def _k32_acc(device):
    """[kb 2, 64, 8]: the 32x32 accumulator's order, channel 16 kb + 8 (e / 4) + 4 kh + e % 4."""
    lane, e = _lane_j(device)
    return 16 * torch.arange(2, device=device).view(2, 1, 1) + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3)


def _rows(k):
    """The row of A (output channel) each lane holds, shaped to broadcast with its K table k to [2][64][8]:
    16x16 [mt 2, 64, 1] = 16 mt + lane % 16; 32x32 [64, 1] = lane % 32."""
    lane = torch.arange(64, device=k.device).view(64, 1)
    return 16 * torch.arange(2, device=k.device).view(2, 1, 1) + (lane & 15) if k.dim() == 2 else lane & 31


# ---------------------------------------------------------------------- fragments, parameter blocks, placement
def _f32(t):
    return t.detach().float()


def _frags(w, transposed, row, k, ky, kx):
    """fp16 A fragments W[out = row][in = k] at kernel element (ky, kx) of a float32 Conv2d weight [out,in,K,K] (transposed: of a
    ConvTranspose2d weight [in,out,K,K]); the four indices broadcast to the fragments' shape [..., 2, 64, 8]."""
    return (w[k, row, ky, kx] if transposed else w[row, k, ky, kx]).to(torch.float16)


def _frag_1x1(w, col0, order):
    """The two fp16 A fragments [2][lane 64][8] of the 32 columns from col0 of a 1x1 weight matrix w [32, ld], K index in `order`."""
    k = order(w.device)
    return _f32(w)[_rows(k), col0 + k].to(torch.float16)


def _param_block(biases, slopes, n, device):
    """n float32 as bytes: bias i (any length up to 32; None: zeros) from float 32 i, the PReLU slopes from float n - 32 on."""
    par = torch.zeros(n, dtype=torch.float32, device=device)
    for i, b in enumerate(biases):
        if b is not None:
            par[32 * i:32 * i + b.numel()] = _f32(b)
    for i, a in enumerate(slopes):
        par[n - 32 + i] = float(a)
    return par.view(torch.uint8)


def _put(blob, off, t, nbytes):
    """t's bytes to blob[off : off + nbytes], which they fill exactly -> off + nbytes."""
    raw = t.contiguous().view(torch.uint8).reshape(-1)
    assert raw.numel() == nbytes, (raw.numel(), nbytes)
    blob[off:off + nbytes] = raw
    return off + nbytes


def _lead3(device, a, b, c):
    """arange(a), arange(b), arange(c) along the three leading axes of a fragment array [a][b][c][2][lane 64][8]."""
    return (torch.arange(a, device=device).view(a, 1, 1, 1, 1, 1), torch.arange(b, device=device).view(b, 1, 1, 1, 1),
            torch.arange(c, device=device).view(c, 1, 1, 1))


def _conv_out_frags9(cv_w):
    """conv_out [3,32,3,3] as the nine fp16 A fragments [dy 3][dx 3][lane 64][8] of the fused x2 / x3 tails: rows 0-2 are its output
    channels, K index in the 16x16 accumulator's order (the HR ring's)."""
    dev = cv_w.device
    k = _k16_acc(dev)
    row = torch.arange(64, device=dev) & 15
    live = row < 3
    cv = torch.zeros((3, 3, 64, 8), dtype=torch.float32, device=dev)
    cv[:, :, live] = _f32(cv_w)[row[live].unsqueeze(1), k[live]].permute(2, 3, 0, 1)
    return cv.to(torch.float16)


def _fold_co_section(blob, off, fold_co):
    """fold_co = (w [32,ld], (col_a, col_b), b [32], a) at `off`: compress_out's slices for the two live maps as 2 x 2 fragments in natural
    order (the 1x1 reads the raw maps), then b[32] and the slope -> the offset behind them."""
    co_w, cols, co_b, co_a = fold_co
    off = _put(blob, off, torch.stack([_frag_1x1(co_w, c, _k16_natural) for c in cols]), 4096)
    return _put(blob, off, _param_block([co_b], [co_a], 64, blob.device), 256)


def _post_section(blob, off, post, gap=0):
    """post = (w [32,ld], col0, b [32], a) at `off`: two fragments in natural order (the B operand is the stage's output row as it lies in
    memory), `gap` unused bytes, then b[32] and the slope -> the offset behind them."""
    pw, pcol, pb, pa = post
    off = _put(blob, off, _frag_1x1(pw, pcol, _k16_natural), 2048)
    return _put(blob, off + gap, _param_block([pb], [pa], 64, blob.device), 256)


# ---------------------------------------------------------------------- fp32 path
def pack_dt_frags(dt_w: torch.Tensor, col: int) -> torch.Tensor:
    """The 32 x 32 slice [:, col:col+32] of a downtran weight matrix [32(out), ld(in)] as the 16 A-operand fragments of the fused tail of
    csrc/sr_f32_mfma.hip:k_deconv_mfma_sh<.., DT>: fragment r, lane l = W[out = l % 32][in = 8 (r // 4) + 4 (l // 32) + r % 4]."""
    w = _f32(dt_w[:, col:col + _NF])
    r = torch.arange(16).view(16, 1)
    l = torch.arange(64).view(1, 64)
    ci = 8 * (r // 4) + 4 * (l // 32) + r % 4
    co = (l % 32).expand(16, 64)
    return w[co.to(w.device), ci.to(w.device)].contiguous()


# ---------------------------------------------------------------------- x4
def pack_utd_blob(up_w, up_b, up_a, tr_w, tr_col0, tr_b, tr_a, dn_w, dn_b, dn_a, layout: int = 1, fold_co=None, post=None) -> torch.Tensor:
    """Weights of one fused up->tran->down stage in the per-wave MFMA fragment order of csrc/sr_f16.hip (layout 1: k_utd, every wave both
    phases; 2: k_utd2, producer / consumer waves) or csrc/sr_utd4.hip (layout 4: k_utd4, v_mfma_f32_32x32x16_f16, same regions and sizes).

    up_w [32(in),32(out),8,8] ConvTranspose2d weight; tr_w [32,ld] 1x1 weight whose live slice starts at column
    tr_col0; dn_w [32(out),32(in),8,8] Conv2d weight.  tr_w/dn_w None -> deconv-only blob (tail).
    fold_co = (co_w [32,ld], (col0_a, col0_b), co_b [32], co_a): the 1x1 + PReLU over two LR maps (+ constant map) that
    produces the deconv's input, applied by k_tail3<.., FOLD> on the rows' way into LDS; the deconv fragments then take
    their K index in the accumulator's channel order (vsr_sr_tail3_fold_f16).
    post = (w [32,ld], col0, b [32], a): the 1x1 + PReLU that vsr_sr_utd_post_f16 applies to every finished output row (the next
    group's uptran slice); its two fragments, bias and slope take the first half of the compress_out region (natural channel order).

    Regions: deconv fragments 128 KiB, down fragments 128 KiB, 1x1 fragments 2 KiB, parameters 512 B, compress_out region.
    deconv (natural order, the B operand comes straight from the LR rows): layout 1 [w 8][c 2][t 4], tap t of phase (py, px);
    2 [producer p 4][phase c 4][tap 4], HR row phase p, column phase c; 4 [wave 4][column phase 4][tap (dy, dx) 4], ky = wave + 4 dy,
    kx = phase + 4 dx.  down (accumulator order): 1 [w 8][lo/hi 2][kx 8], wave w owns kernel rows w & 3 (lo) and (w & 3) + 4 (hi) of
    out-channel half w >> 2 -- one fragment per slot; 2 [consumer q 4][lo/hi 2][kx 8], rows q and q + 4, both halves; 4 [wave 4][0: kernel
    row wave (next output row), 1: wave + 4 (current)][kx 8]."""
    dev = up_w.device
    nbytes = int(L.load().vsr_sr_query(L.Q_UTD_BLOB_BYTES))
    if layout == 4:
        k_up, k_acc = _k32_natural(dev), _k32_acc(dev)
    else:
        k_up, k_acc = (_k16_natural if fold_co is None else _k16_acc)(dev), _k16_acc(dev)
    if layout == 1:
        W, C, T = _lead3(dev, 8, 2, 4)
        ky, kx = (W >> 1) + 4 * (T >> 1), 2 * (W & 1) + C + 4 * (T & 1)
    else:
        P, C, T = _lead3(dev, 4, 4, 4)
        ky, kx = P + 4 * (T >> 1), C + 4 * (T & 1)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    off = _put(blob, 0, _frags(_f32(up_w), True, _rows(k_up), k_up, ky, kx), 128 * 1024)
    if dn_w is None:
        off += 128 * 1024 + 2048   # the down fragments and the 1x1 fragments: left zero, the tail deconvolution has neither
        off = _put(blob, off, _param_block([up_b], [up_a], 128, dev), 512)
    else:
        Q, HL, KX = _lead3(dev, 4, 2, 8)
        dn_frag = _frags(_f32(dn_w), False, _rows(k_acc), k_acc, Q + 4 * HL, KX)   # [q 4][lo/hi 2][kx 8][2][lane 64][8]
        if layout == 1:   # wave w = 4 mt + q holds one row tile per slot: the tile index leads
            dn_frag = dn_frag.permute(3, 0, 1, 2, 4, 5)
        off = _put(blob, off, dn_frag, 128 * 1024)
        off = _put(blob, off, _frag_1x1(tr_w, tr_col0, _k32_acc if layout == 4 else _k16_acc), 2048)
        off = _put(blob, off, _param_block([up_b, tr_b, dn_b], [up_a, tr_a, dn_a], 128, dev), 512)
    if fold_co is not None:
        _fold_co_section(blob, off, fold_co)
    if post is not None:
        assert fold_co is None
        _post_section(blob, off, post, gap=2048)   # the parameters sit where fold_co's do, at + 4096
    return blob


def pack_conv_out_frags3(weight) -> torch.Tensor:
    """conv_out weight [3,32,3,3] -> the 3 MFMA A-fragments (one per dx) of csrc/sr_tail3.hip:k_tail3, [dx][lane 64][8]
    fp16: accumulator row m = 4 dy + co holds the contribution of an HR row to output row (HR row + 1 - dy), channel co;
    k index (g, j) follows the operand tiles' channel order."""
    dev = weight.device
    w = _f32(weight)
    m = torch.arange(64, device=dev) & 15
    dy, co = m >> 2, m & 3
    live = (dy < 3) & (co < 3)
    ci = _k16_acc(dev)[live]  # [n_live, 8]
    frags = torch.zeros((3, 64, 8), dtype=torch.float32, device=dev)
    for dx in range(3):
        frags[dx, live] = w[co[live].unsqueeze(1), ci, dy[live].unsqueeze(1), dx]
    return frags.to(torch.float16).contiguous()


def pack_conv_out_frags(weight) -> torch.Tensor:
    """conv_out weight [3,32,3,3] -> the 9 MFMA A-fragments of csrc/sr_f16.hip:k_tail, [tap][lane 64][8] fp16:
    accumulator row m = lane & 15 carries output channel c iff m == 4c; k index (g, j) follows the ring's channel order."""
    dev = weight.device
    w = _f32(weight)
    m = torch.arange(64, device=dev) & 15
    k = _k16_acc(dev)
    frags = torch.zeros((9, 64, 8), dtype=torch.float32, device=dev)
    for c in range(3):
        sel = m == 4 * c
        ci = k[sel]  # [n_sel, 8]
        for t in range(9):
            frags[t, sel] = w[c, ci, t // 3, t % 3]
    return frags.to(torch.float16).contiguous()


# ---------------------------------------------------------------------- x2
def _s2_taps(device):
    """Kernel element (ky, kx) of wave (r, c) = (HR row parity, HR column parity), tap (dy, dx) of the k6 s2 geometry, along the leading
    axes [wave 4][dy 3][dx 3] of a fragment array: (r + 2 dy, c + 2 dx)."""
    W, A, B = _lead3(device, 4, 3, 3)
    return (W >> 1) + 2 * A, (W & 1) + 2 * B


def pack_utd_s2_blob(up_w, up_b, up_a, tr_w, tr_col0, tr_b, tr_a, dn_w, dn_b, dn_a, layout: int = 1, post=None) -> torch.Tensor:
    """Weights of one fused x2 stage in the per-wave MFMA fragment order of csrc/sr_utd_s2.hip (layout 4: csrc/sr_utd_s2w.hip, k_utd_s2w,
    v_mfma_f32_32x32x16_f16 -- same regions and size).  Wave (r, c) = (HR row parity, HR column parity): deconv tap (dy, dx) is kernel
    element (r + 2 dy, c + 2 dx) of the ConvTranspose2d weight [32(in),32(out),6,6] (natural order: the B operand comes straight from
    the LR rows); conv slot (k, s) is kernel element (r + 2 k, c + 2 s) of the Conv2d weight [32(out),32(in),6,6] (accumulator order,
    as the 1x1).  Regions: deconv 72 KiB, conv 72 KiB, 1x1 2 KiB, parameters 512 B.
    post = (w [32,ld], col0, b [32], a): the 1x1 + PReLU that vsr_sr_utd_s2_post_f16 applies to every finished output row (the next
    group's uptran slice), behind the stage's parameters."""
    dev = up_w.device
    nbytes = int(L.load().vsr_sr_query(L.Q_UTD_S2_BLOB_BYTES))
    nat, acc = (_k32_natural, _k32_acc) if layout == 4 else (_k16_natural, _k16_acc)
    k_nat, k_acc = nat(dev), acc(dev)
    ky, kx = _s2_taps(dev)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    off = _put(blob, 0, _frags(_f32(up_w), True, _rows(k_nat), k_nat, ky, kx), 72 * 1024)
    off = _put(blob, off, _frags(_f32(dn_w), False, _rows(k_acc), k_acc, ky, kx), 72 * 1024)
    off = _put(blob, off, _frag_1x1(tr_w, tr_col0, acc), 2048)
    off = _put(blob, off, _param_block([up_b, tr_b, dn_b], [up_a, tr_a, dn_a], 128, dev), 512)
    if post is not None:
        _post_section(blob, off, post)
    return blob


def pack_tail_s2_blob(out_w, out_b, out_a, cv_w, cv_b, fold_co=None) -> torch.Tensor:
    """Weights of the fused x2 tail (csrc/sr_tail_s2.hip): the `out` ConvTranspose2d [32,32,6,6] in k_utd_s2's per-wave
    fragment order, conv_out [3,32,3,3] as nine A fragments whose rows 0-2 are its output channels (k index in the
    accumulator-derived channel order of the ring), then b_out[32], b_cv[3] and the PReLU slope.
    fold_co = (w [32,ld], (col_a, col_b), b [32], a): compress_out over two live maps, for vsr_sr_tail_s2_fold_f16."""
    dev = out_w.device
    nbytes = int(L.load().vsr_sr_query(L.Q_TAIL_S2_BLOB_BYTES))
    k = _k16_natural(dev)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    off = _put(blob, 0, _frags(_f32(out_w), True, _rows(k), k, *_s2_taps(dev)), 72 * 1024)
    off = _put(blob, off, _conv_out_frags9(cv_w), 9 * 1024)
    off = _put(blob, off, _param_block([out_b, cv_b], [out_a], 128, dev), 512)
    if fold_co is not None:
        _fold_co_section(blob, off, fold_co)
    return blob


# ---------------------------------------------------------------------- x3
# the x3 stage's waves own phase SETS of equal tap count (csrc/sr_utd_s3.hip): (HR row phase, HR column phase) per wave, in slot order
_S3_PHASES = (((1, 1), (0, 0)), ((0, 1), (2, 1)), ((1, 0), (1, 2)), ((0, 2), (2, 0), (2, 2)))
_S3_SLOTS = 13                             # per wave; the unused ones stay zero
_S3_FRAG_BYTES = 4 * _S3_SLOTS * 2 * 1024  # one [wave 4][slot 13][mt 2][lane 64][8] fp16 array


def _s3_taps(x):
    """Kernel indices of phase x of the (7, 3, 2) geometry in slot order: k = x + 2 - 3 d for d = +1, 0, -1 where 0 <= k <= 6."""
    return [x + 2 - 3 * d for d in (1, 0, -1) if 0 <= x + 2 - 3 * d <= 6]


def _s3_slots():
    """(wave, slot, ky, kx): a wave's slots run over its phases (r, c) of _S3_PHASES, then the kernel rows ky of r, then the kernel
    columns kx of c (_s3_taps)."""
    for wv, phases in enumerate(_S3_PHASES):
        taps = [(ky, kx) for r, c in phases for ky in _s3_taps(r) for kx in _s3_taps(c)]
        assert len(taps) <= _S3_SLOTS
        for t, (ky, kx) in enumerate(taps):
            yield wv, t, ky, kx


def _s3_frags(w, transposed, k):
    """[wave 4][slot 13][mt 2][lane 64][8] fp16: slot t holds kernel element (ky, kx) of _s3_slots, K index k."""
    w, row = _f32(w), _rows(k)
    out = torch.zeros((4, _S3_SLOTS, 2, 64, 8), dtype=torch.float16, device=w.device)
    for wv, t, ky, kx in _s3_slots():
        out[wv, t] = _frags(w, transposed, row, k, ky, kx)
    return out


def pack_utd_s3_blob(up_w, up_b, up_a, tr_w, tr_col0, tr_b, tr_a, dn_w, dn_b, dn_a, layout: int = 1, post=None) -> torch.Tensor:
    """Weights of one fused x3 stage in the per-wave MFMA fragment order of csrc/sr_utd_s3.hip (include/vsr_hip_s3.h).  Slot t
    (_s3_slots) of the deconvolution is element (ky, kx) of the ConvTranspose2d weight [32(in),32(out),7,7] (natural order: the B operand
    comes straight from the LR rows) and slot t of the convolution the SAME element of the Conv2d weight [32(out),32(in),7,7]
    (accumulator order, as the 1x1; the down-convolution mirrors the tap algebra).  `layout` and `post` exist for the argument list of
    pack_utd_s2_blob: one layout, no POST build."""
    if layout != 1 or post is not None:
        raise NotImplementedError("k_utd_s3 has one fragment layout and no in-launch uptran slice")
    dev = up_w.device
    nbytes = int(L.load_s3().vsr_s3_query(L.Q_S3_BLOB_BYTES))
    assert nbytes == 2 * _S3_FRAG_BYTES + 2048 + 512
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    off = _put(blob, 0, _s3_frags(up_w, True, _k16_natural(dev)), _S3_FRAG_BYTES)
    off = _put(blob, off, _s3_frags(dn_w, False, _k16_acc(dev)), _S3_FRAG_BYTES)
    off = _put(blob, off, _frag_1x1(tr_w, tr_col0, _k16_acc), 2048)
    _put(blob, off, _param_block([up_b, tr_b, dn_b], [up_a, tr_a, dn_a], 128, dev), 512)
    return blob


def pack_tail_s3_blob(out_w, out_b, out_a, cv_w, cv_b, fold_co=None) -> torch.Tensor:
    """Weights of the fused x3 tail (csrc/sr_tail_s3.hip, include/vsr_hip_s3t.h): the `out` ConvTranspose2d [32,32,7,7] in k_utd_s3's
    per-wave slot order (the `up` half of pack_utd_s3_blob), conv_out [3,32,3,3] as nine A fragments whose rows 0-2 are its output
    channels (k index in the accumulator-derived channel order of the HR ring), then b_out[32], b_cv[3] and the PReLU slope.
    fold_co = (w [32,ld], (col_a, col_b), b [32], a): compress_out over two live maps, for vsr_s3t_sr_tail_fold_f16
    (the blob is then VSR_S3T_Q_BLOB_FOLD_BYTES long; the plain entry reads its first VSR_S3T_Q_BLOB_BYTES)."""
    dev = out_w.device
    lib = L.load_s3t()
    nplain = int(lib.vsr_s3t_query(L.Q_S3T_BLOB_BYTES))
    nbytes = nplain if fold_co is None else int(lib.vsr_s3t_query(L.Q_S3T_BLOB_FOLD_BYTES))
    assert nplain == _S3_FRAG_BYTES + 9 * 1024 + 512
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    off = _put(blob, 0, _s3_frags(out_w, True, _k16_natural(dev)), _S3_FRAG_BYTES)
    off = _put(blob, off, _conv_out_frags9(cv_w), 9 * 1024)
    off = _put(blob, off, _param_block([out_b, cv_b], [out_a], 128, dev), 512)
    if fold_co is not None:
        off = _fold_co_section(blob, off, fold_co)
        assert off == nbytes
    return blob


def _append_post_s3(stage_blob, post) -> torch.Tensor:
    """stage_blob (pack_utd_s3_blob's bytes) + the POST section of include/vsr_hip_s3p.h: post = (w [32,ld], col0, b [32], a) as two A
    fragments in NATURAL channel order (the B operand is the stage's output row as it lies in memory), then b_post[32], slope_post."""
    nbytes = int(L.load_s3p().vsr_s3p_query(L.Q_S3P_BLOB_BYTES))
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=stage_blob.device)
    off = _put(blob, 0, stage_blob, stage_blob.numel())
    off = _post_section(blob, off, post)
    assert off == nbytes
    return blob


def pack_utd_s3_post_blob(up_w, up_b, up_a, tr_w, tr_col0, tr_b, tr_a, dn_w, dn_b, dn_a, post) -> torch.Tensor:
    """The blob of vsr_s3p_sr_utd_post_f16 (include/vsr_hip_s3p.h): pack_utd_s3_blob's bytes, then post = (w [32,ld], col0, b [32], a), the
    1x1 + PReLU applied to every finished output row (the next group's uptran slice)."""
    return _append_post_s3(pack_utd_s3_blob(up_w, up_b, up_a, tr_w, tr_col0, tr_b, tr_a, dn_w, dn_b, dn_a), post)


PRE_SECTION_BYTES = 12 * 1024 + 512


def pack_utd_s3_pre_blob(post_blob, co, ci, ut0) -> torch.Tensor:
    """The blob of vsr_s3f_sr_utd_pre_f16 (include/vsr_hip_s3f.h): post_blob (pack_utd_s3_post_blob's bytes, byte for byte), then the PRE
    section -- the step-opening 1x1 chain as twelve A fragments [lane 64][8] fp16 (fragment 2 i + mt: rows 16 mt + lane % 16 of matrix i)
    and a parameter block.  co = (w [32,ld], (col_a, col_b), b [32], a): compress_out over the two live maps; ci = (w [32,64], b, a):
    compress_in (columns 0:32 multiply `feat`, 32:64 the previous 1x1's tile); ut0 = (w [32,ld], col0, b, a): the first uptran slice.
    Memory inputs in natural channel order, chained inputs in the accumulator's; the second half of ci a second time in natural order
    (step 0, where it multiplies `feat`)."""
    nbytes = int(L.load_s3f().vsr_s3f_query(L.Q_S3F_BLOB_BYTES))
    assert nbytes == post_blob.numel() + PRE_SECTION_BYTES
    co_w, (col_a, col_b), co_b, co_a = co
    ci_w, ci_b, ci_a = ci
    ut_w, ut_col, ut_b, ut_a = ut0
    frags = torch.stack((_frag_1x1(co_w, col_a, _k16_natural), _frag_1x1(co_w, col_b, _k16_natural), _frag_1x1(ci_w, 0, _k16_natural),
                         _frag_1x1(ci_w, _NF, _k16_acc), _frag_1x1(ut_w, ut_col, _k16_acc), _frag_1x1(ci_w, _NF, _k16_natural)))
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=post_blob.device)
    off = _put(blob, 0, post_blob, post_blob.numel())
    off = _put(blob, off, frags, 12 * 1024)
    _put(blob, off, _param_block([co_b, ci_b, ut_b], [co_a, ci_a, ut_a], 128, blob.device), 512)
    return blob
