// conv_kwalk.h -- the K walk of the gather kernels (conv_igemm.hip: k_conv_igemm_d, k_conv_igemm) and of the tile kernel
// (conv_tile.hip: k_conv_tile), stated once: the split-K range and phase of a workgroup, the two buffer resources, the (tap, chunk)
// table in LDS and its size, and the per-row pixel origin.
// The first part is plain C++ (no HIP type): the launchers and a host-only test program read it.
#pragma once

namespace vsrc {

// K steps of a layer: (tap, 32-channel chunk) pairs, two per step (the odd tail pair is zero-filled), `splits` contiguous ranges of
// ks_per steps.  stem: one chunk per kernel ROW (conv_igemm.hip, STEM).
struct KSteps {
    int nchunk, npair, nk_all, ks_per;
};
constexpr KSteps k_steps(bool stem, int kh, int kw, int cin, int splits) {
    const int nchunk = stem ? 1 : cin >> 5;
    const int npair = stem ? kh : kh * kw * nchunk;
    const int nk_all = (npair + 1) >> 1;
    return KSteps{nchunk, npair, nk_all, (nk_all + splits - 1) / splits};
}

// Entries (16 bytes each) of a workgroup's K-walk table: the two pairs of each of its ks_per steps and of `lookahead` steps past them,
// which the kernel requests like any other (dead entries: zeros, no traffic).  What each kernel looks ahead:
//   gather, D register sets: the loop runs whole groups of D steps (up to D - 1 past the range), D - 1 steps are in flight ahead of
//                            the step being multiplied, and the entries of the next request are read one step early;
//   first gather build:      as D = 3 (it needs 3: groups of two, two steps ahead, one of read-ahead);
//   tile:                    one step staged ahead + one of read-ahead.
constexpr int kwalk_gather_lookahead(int D) { return 2 * D - 1; }
constexpr int KWALK_FIRST_LOOKAHEAD = 5, KWALK_TILE_LOOKAHEAD = 2;
constexpr int kwalk_entries(int ks_per, int lookahead) { return 2 * (ks_per + lookahead); }

}  // namespace vsrc

#ifdef __HIP__
#include "conv_common.h"

namespace vsrc {

// ---- the range of K steps and the phase of one workgroup.  bz = blockIdx.z (gather) / the decoded z (tile) = split * 4 + phase
//      for the four phases of a k4 s2 transposed convolution in one launch, else the split.
// split-K (small pixel counts with long K, e.g. the 1/32 and 1/64-resolution FlowNet layers): a workgroup owns a contiguous range of
// K steps [ks0, nk) and writes an fp32 partial tile; k_splitk_finish sums them in a fixed order
struct KRange {
    int ph, zsplit;
    const _Float16* wpk;
    int pad_y, pad_x, oy_off, ox_off;
    int ks_per, ks0, nk;
};
template <class Z>
__device__ __forceinline__ KRange k_range(const ConvP& p, Z bz, int nk_all) {
    KRange r;
    r.ph = p.nphase > 1 ? (int)(bz & 3) : 0;
    r.zsplit = p.nphase > 1 ? (int)(bz >> 2) : (int)bz;
    r.wpk = p.nphase > 1 ? p.wpk_ph[r.ph] : p.wpk;
    r.pad_y = p.nphase > 1 ? p.pad_y_ph[r.ph] : p.pad_y; r.pad_x = p.nphase > 1 ? p.pad_x_ph[r.ph] : p.pad_x;
    r.oy_off = p.nphase > 1 ? p.oy_off_ph[r.ph] : p.oy_off; r.ox_off = p.nphase > 1 ? p.ox_off_ph[r.ph] : p.ox_off;
    r.ks_per = (nk_all + p.splits - 1) / p.splits;
    r.ks0 = r.zsplit * r.ks_per;
    r.nk = min(nk_all, r.ks0 + r.ks_per);
    return r;
}

// the two operands' buffer resources: the packed weight slabs [pair][cout_pad][32] of this phase, the whole input batch
__device__ __forceinline__ __amdgpu_buffer_rsrc_t kwalk_w_rsrc(const ConvP& p, const _Float16* wpk, int npair) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(wpk), 0, (int)((size_t)npair * p.cout_pad * 64), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t kwalk_in_rsrc(const ConvP& p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.in), 0, (int)((size_t)p.N * p.H * p.W * p.in_ld * 2), 0x00020000);
}

// ---- the K walk as a table in LDS, built once per workgroup: entry i = pair 2 ks0 + i = (tap (ky, kx), chunk ch) as
//      {input byte offset of the tap and chunk relative to tap (0,0) chunk 0, ky, kx, byte offset of the pair's weight slab};
//      a pair past the kernel or past this split's range has ky = 2^29 (fails every row test) and a weight offset past the
//      slabs, so the loop requests it like any other and the hardware returns zeros.  The loop itself then holds no integer
//      division, no tap walk and no range logic: per piece one add and two unsigned compares on broadcast table values.
//      (Measured, tools/gather_steps.py: with the addresses computed per step from (pair / nchunk, tap / kw, ...) a K step of
//      an otherwise EMPTY loop -- loads and MFMAs switched off -- cost 500-620 cycles per workgroup, half of the step.)
//      STEM: a pair is a whole kernel row (ky = pair, kx = 0).  ntab = kwalk_entries(ks_per, the kernel's lookahead): the launcher
//      reserves the same count.
//      (The layer's fields come in as scalars through the wrapper below: with `p` read inside the loop's function the STEM builds
//      of k_conv_igemm_d gained 7-9 prologue instructions.)
template <bool STEM>
__device__ __forceinline__ void build_kwalk_s(int cout_pad, int W, int in_ld, int pkw, u4* tab, int tid, int ks0, int nk, int npair, int nchunk, int ntab) {
    const int pr0 = 2 * ks0;
    const unsigned wstep = (unsigned)cout_pad * 64u;
    const int kw = STEM ? 1 : pkw;   // (STEM: nchunk = 1 too, so ky = pair, kx = 0)
    for (int i = tid; i < ntab; i += 256) {
        const int pr = pr0 + i;
        const bool live = pr < npair && pr < 2 * nk;
        const int prc = live ? pr : 0;
        const int tap = prc / nchunk, ch = prc - tap * nchunk;
        const int ky = tap / kw, kx = tap - ky * kw;
        const unsigned delta = ((unsigned)(ky * W + kx) * (unsigned)in_ld + (unsigned)ch * 32u) * 2u;
        tab[i] = live ? u4{delta, (unsigned)ky, (unsigned)kx, (unsigned)pr * wstep} : u4{0u, 1u << 29, 0u, 0x80000000u};
    }
}
template <bool STEM>
__device__ __forceinline__ void build_kwalk(const ConvP& p, u4* tab, int tid, int ks0, int nk, int npair, int nchunk, int ntab) {
    build_kwalk_s<STEM>(p.cout_pad, p.W, p.in_ld, p.kw, tab, tid, ks0, nk, npair, nchunk, ntab);
}

// ---- the origin of output pixel m (row m - m0 of the workgroup's 128) for a lane that fetches 16-byte channel piece `piece` of it:
//      a 32-bit byte offset of (pixel, tap (0,0), chunk 0, piece) -- wrapped modulo 2^32 where the padding makes it negative; adding
//      the table's tap offset wraps it back -- plus the pixel's first input row / column for the bounds tests.  A pixel past M fails
//      every row test.  STEM: the piece is two 8-byte pixels, taps 2 piece and 2 piece + 1 of a kernel row (columns fixed per lane).
struct PixOrigin {
    int piy0, pix0;
    unsigned pbase;
};
template <bool STEM>
__device__ __forceinline__ PixOrigin pixel_origin(const ConvP& p, long long m, long long M, int pad_y, int pad_x, int piece) {
    PixOrigin o;
    const bool ok = m < M;
    const unsigned mm = ok ? (unsigned)m : 0u, HoWo = (unsigned)(p.Ho * p.Wo);   // (M < 2^31: checked by the launchers; 32-bit divisions)
    const int n = (int)(mm / HoWo);
    const int rem = (int)(mm - (unsigned)n * HoWo);
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    o.piy0 = ok ? oy * p.stride - pad_y : -(1 << 28);
    o.pix0 = ox * p.stride_x - pad_x + (STEM ? 2 * piece : 0);
    o.pbase = (unsigned)(((((long long)n * p.H + o.piy0) * p.W + o.pix0) * p.in_ld + (STEM ? 0 : p.in_coff + piece * 8)) * 2);
    return o;
}

}  // namespace vsrc
#endif  // __HIP__
