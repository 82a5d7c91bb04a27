// conv_patch.h -- the vocabulary of the LDS-patch convolution kernels (conv_igemm.hip, conv_patch_pf.hip), each item once: the
// epilogue (bias + activation + fp16, out through wave-local LDS as whole 16-byte pieces), the patch staging (global -> registers
// -> LDS, 64-byte pixels, 16-byte pieces XOR-swizzled by pixel-column bits 1-2), the 16 x 32 tile family's LDS geometry, the
// workgroup's tile, the tap-column walk and the wave's output addressing.  The helpers are shaped so that every kernel compiles to
// the parent's instructions (register names aside); what did not is said where it stays duplicated.
#pragma once
#include "conv_common.h"

namespace vsrc {

// Epilogue of the convolution kernels: bias + activation + fp16, then out through LDS so that a pixel's 16 MT channels leave
// as whole 16-byte pieces from adjacent lanes (a full 128-byte line per pixel at MT = 4).  Straight from the MFMA
// layout a store instruction writes 8 bytes per lane, 32 bytes per pixel per out-channel tile; measured on the 3x3
// FlowNet layers those partial-line writes cost a third of the kernel (3x3 32->64 at 2x512x960: 121 -> 88 us).  Wave-local: each
// wave transposes its own NT x 16 pixels in its own LDS slice (the caller has synchronised after the last patch read).
// acc(ti, mt) -> f4 of pixel-tile ti; pixoff(ti, li) -> element offset of pixel li of tile ti in the output tensor (its
// channel 0), or -1 when the pixel does not exist.
template <int MT, int NT, int ACT, class GetAcc, class PixOf>
__device__ __forceinline__ void patch_epilogue_act(const ConvP& p, unsigned char* wave_lds, int co0, int lane, GetAcc acc, PixOf pixoff) {
    constexpr int RB = 32 * MT, LPP = 2 * MT, PPI = 64 / LPP;
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int c = co0 + 16 * mt + 4 * g;
        float bz[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bz[e] = (p.bias && c + e < p.cout) ? p.bias[c + e] : 0.0f;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const f4 a = acc(ti, mt);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float tt = a[e] + bz[e];
                if (ACT == 1) tt = fmaxf(tt, 0.0f);
                else if (ACT == 2) tt = tt >= 0.0f ? tt : tt * p.slope;
                v[e] = tt;
            }
            *reinterpret_cast<h4*>(wave_lds + (ti * 16 + l15) * RB + (((2 * mt + (g >> 1)) ^ (l15 & (LPP - 1))) << 4) + ((g & 1) << 3)) =
                h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        }
    }
    asm volatile("" ::: "memory");   // (same wave, in-order LDS: the reads below see the writes above)
    const bool vec_ok = ((p.out_coff + co0) & 7) == 0 && (p.out_ld & 7) == 0;
    const int k = lane % LPP;
    const int c = co0 + 8 * k;
#pragma unroll
    for (int it = 0; it < NT * 16 / PPI; ++it) {
        const int pl = it * PPI + lane / LPP;
        const int ti = pl >> 4, li = pl & 15;
        const long long po = pixoff(ti, li);
        const h8 v = *reinterpret_cast<const h8*>(wave_lds + pl * RB + ((k ^ (li & (LPP - 1))) << 4));
        if (po < 0 || c >= p.cout) continue;
        _Float16* dst = p.out + po + p.out_coff + c;
        if (vec_ok && c + 8 <= p.cout) {
            *reinterpret_cast<h8*>(dst) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c + e < p.cout) dst[e] = v[e];
        }
    }
}

// (the activation is a template constant: tested per value at run time it compiled to two scalar branches per output value --
//  128 branches per wave in the 3x3 build, whose epilogue and patch addressing together issued 9 vector instructions per MFMA;
//  PMC on the 32 -> 64 layer at 2 x 512 x 960: 1340 VALU / 586 SALU / 144 MFMA per wave, VALU pipe 51 % busy, MFMA pipe 22 %)
template <int MT, int NT, class GetAcc, class PixOf>
__device__ __forceinline__ void patch_epilogue(const ConvP& p, unsigned char* wave_lds, int co0, int lane, GetAcc acc, PixOf pixoff) {
    if (p.act == 0) patch_epilogue_act<MT, NT, 0>(p, wave_lds, co0, lane, acc, pixoff);
    else if (p.act == 1) patch_epilogue_act<MT, NT, 1>(p, wave_lds, co0, lane, acc, pixoff);
    else patch_epilogue_act<MT, NT, 2>(p, wave_lds, co0, lane, acc, pixoff);
}

__device__ __forceinline__ long long patch_pixoff(const ConvP& p, int n, int oy, int ox) {
    if (oy >= p.Ho || ox >= p.Wo) return -1;
    return (long long)((((size_t)n * p.outH + oy * p.oy_mul + p.oy_off) * p.outW + ox * p.ox_mul + p.ox_off) * p.out_ld);
}

constexpr int PT_H = 8, PT_W = 32;
constexpr int P8_H = 16, P8_W = 32, P8_R = 8;   // 16 x 32 output tile, 8 rows x 16 columns per wave (k_conv_patch_r8 / _lw / _pf)

// The input of one patch as a buffer resource.  It starts at the patch's first image row: offsets then span PH rows only, whatever
// the size of the image (a 2160 x 3840 x 224-channel map is 3.7 GB; with the resource at the image base the 32-bit offsets capped an
// image at 2 GiB and such layers fell back to the gather kernel: 127 ms of a 437 ms frame at 4K -> 8K)
// (by: the patch's first image row, max(iy0, 0); k_conv_patch_pf keeps it per work item)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t patch_rsrc_at(const ConvP& p, int n, int by) {
    const size_t rem_bytes = (size_t)(p.H - by) * p.W * p.in_ld * 2;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.in) + ((size_t)n * p.H + by) * p.W * p.in_ld, 0,
                                             (int)(rem_bytes < 0x7FFFFFF0ull ? rem_bytes : 0x7FFFFFF0ull), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t patch_rsrc(const ConvP& p, int n, int iy0) { return patch_rsrc_at(p, n, iy0 > 0 ? iy0 : 0); }

// Stages the [PH][PW] x 32-channel input patch of image n, chunk ch into LDS (pixel = 64 B, 16-byte pieces XOR-swizzled
// by pixel-column bits 1-2).  Six pieces per thread are requested back to back with no branch in between (buffer loads:
// positions outside the image or past the patch carry an out-of-range offset and read zeros) and only then written to
// LDS -- a conditional load per piece serialises one memory latency per piece, which was most of the 3x3 layers' time.
__device__ __forceinline__ void stage_patch(const ConvP& p, unsigned char* patch, int n, int ch, int iy0, int ix0, int PH, int PW, int tid) {
    constexpr int U = 6;
    typedef u4 u4v;
    const int by = iy0 > 0 ? iy0 : 0;   // (offsets count from the resource's first row)
    const __amdgpu_buffer_rsrc_t rsrc = patch_rsrc(p, n, iy0);
    const int total = PH * PW * 4;
    const unsigned coff = (unsigned)(p.in_coff + ch * 32) * 2;
    // piece q = tid + 256 k of the patch = pixel q >> 2 (row py, column px), 16-byte piece q & 3.  One division per call; from slot
    // to slot the pixel index grows by 64 = dpy rows + dpx columns (a division per piece was half of this function's instructions)
    const int c4 = tid & 3;
    int pix = tid >> 2, py = pix / PW, px = pix - py * PW;
    const int dpy = 64 / PW, dpx = 64 - dpy * PW;
    const unsigned ld2 = (unsigned)p.in_ld * 2, row2 = (unsigned)p.W * ld2;
    for (int q0 = 0; q0 < total; q0 += 256 * U) {
        u4v v[U];
        int dst[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int iy = iy0 + py, ix = ix0 + px;
            const bool in = pix * 4 < total;   // (all four pieces of a pixel exist or none: total is a multiple of 4)
            const bool ok = in && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const unsigned off = ok ? ((unsigned)(iy - by) * row2 + (unsigned)ix * ld2 + coff + c4 * 16) : 0xFFFFFFFFu;
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
            dst[u] = in ? pix * 64 + ((c4 ^ ((px >> 1) & 3)) << 4) : -1;
            pix += 64; py += dpy; px += dpx;
            if (px >= PW) { px -= PW; ++py; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (dst[u] >= 0) *reinterpret_cast<u4v*>(patch + dst[u]) = v[u];
    }
}

// (The piece walk below is written out in stage_patch and again in patch_pieces: as one routine, member or free function, the
//  address arithmetic of every caller was selected differently -- LAB_NOTES.md, "Trunk conv kernels".)
// The same staging with the pieces' descriptors kept in registers across the 32-channel chunks of a layer: a thread's NP
// pieces are the same pixels for every chunk -- only the channel offset moves, 64 bytes per chunk -- so the (row, column) walk,
// the bounds tests and the LDS addresses are computed once per workgroup (`patch_pieces`) and a chunk's staging is one add per
// piece (`stage_patch_cached`; `cached_piece_off` for k_conv_patch_pf, which issues the loads itself).  A 256 -> 256 3x3 layer spent 330 of its 465 vector instructions per chunk on this walk.
template <int NP>
__device__ __forceinline__ void patch_pieces(const ConvP& p, int iy0, int ix0, int PH, int PW, int tid, unsigned (&poff)[NP], int (&pdst)[NP]) {
    const int by = iy0 > 0 ? iy0 : 0;
    const int total = PH * PW * 4;
    const int c4 = tid & 3;
    int pix = tid >> 2, py = pix / PW, px = pix - py * PW;
    const int dpy = 64 / PW, dpx = 64 - dpy * PW;
    const unsigned ld2 = (unsigned)p.in_ld * 2, row2 = (unsigned)p.W * ld2;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int iy = iy0 + py, ix = ix0 + px;
        const bool in = pix * 4 < total;
        const bool ok = in && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        poff[k] = ok ? ((unsigned)(iy - by) * row2 + (unsigned)ix * ld2 + (unsigned)p.in_coff * 2 + c4 * 16) : 0xFFFFFFFFu;
        pdst[k] = in ? pix * 64 + ((c4 ^ ((px >> 1) & 3)) << 4) : -1;
        pix += 64; py += dpy; px += dpx;
        if (px >= PW) { px -= PW; ++py; }
    }
}
// a cached piece's offset at chunk ch (64 bytes per chunk)
__device__ __forceinline__ unsigned cached_piece_off(unsigned poff, int ch) { return poff == 0xFFFFFFFFu ? 0xFFFFFFFFu : poff + (unsigned)ch * 64u; }
template <int NP>
__device__ __forceinline__ void stage_patch_cached(const ConvP& p, unsigned char* patch, int n, int ch, int iy0, const unsigned (&poff)[NP],
                                                   const int (&pdst)[NP]) {
    constexpr int U = 6;
    typedef u4 u4v;
    const __amdgpu_buffer_rsrc_t rsrc = patch_rsrc(p, n, iy0);
#pragma unroll
    for (int k0 = 0; k0 < NP; k0 += U) {
        u4v v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + u < NP) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, cached_piece_off(poff[k0 + u], ch), 0, 0);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + u < NP && pdst[k0 + u] >= 0) *reinterpret_cast<u4v*>(patch + pdst[k0 + u]) = v[u];
    }
}

// ---- the 16 x 32 tile family's LDS geometry (k_conv_patch_lw in conv_igemm.hip, k_conv_patch_pf): the patch, the chunk's weight
//      block [KH*KH][16 MT] rows of 64 B (sw_off per tap) and the epilogue's four wave slices.  lw puts the weight block right
//      behind the patch and the output tile over both; pf keeps the weight block (prefetched during the epilogue) behind the
//      larger of patch and output tile.
template <int KH, int MT>
struct P8Geom {
    static constexpr int PH = P8_H + KH - 1, PW = P8_W + KH - 1;
    static constexpr int PATCH_BYTES = PH * PW * 64;
    static constexpr int WROWS = 16 * MT, WTAP = WROWS * 64, WBYTES = KH * KH * WTAP;
    static constexpr int NPC = (PH * PW * 4 + 255) / 256;      // 16-byte patch pieces per thread
    static constexpr int NWC = (WBYTES / 16 + 255) / 256;      // 16-byte weight pieces per thread
    static constexpr int OUT_BYTES = 4 * P8_R * 16 * 32 * MT;  // epilogue: 4 wave slices
    static constexpr int LW_LDS = PATCH_BYTES + WBYTES > OUT_BYTES ? PATCH_BYTES + WBYTES : OUT_BYTES;
    static constexpr int LDS = (PATCH_BYTES > OUT_BYTES ? PATCH_BYTES : OUT_BYTES) + WBYTES;   // pf
    static constexpr int WOFF = LDS - WBYTES;                  // pf: weight block behind the patch / epilogue region
};

// ---- a workgroup's output tile (TH x TW, blockIdx.x walks the tiles row-major, blockIdx.y the images) and the origin of its patch
struct PatchTile {
    int n, oy0, ox0, iy0, ix0;
};
template <int TH, int TW>
__device__ __forceinline__ PatchTile patch_tile(const ConvP& p, int wo) {   // wo: columns of the tiled map
    const int tiles_x = (wo + TW - 1) / TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    PatchTile t;
    t.n = blockIdx.y;
    t.oy0 = ty * TH; t.ox0 = tx * TW;
    t.iy0 = t.oy0 - p.pad_y; t.ix0 = t.ox0 - p.pad_x;
    return t;
}

// ---- one tap COLUMN of a wave's R rows x 16 columns: each of the KH + R - 1 patch rows is read once and feeds the up-to-R output
//      rows it belongs to (row r, tap row ky = pr - r), MT out-channel tiles each.  src: this lane's piece of the column's first patch
//      row (computed by the kernel: inside this function its address arithmetic compiled to other instructions), A[ky][mt]: the
//      column's weight fragments; after(pr): invoked once row pr has been fed.  Used by k_conv_patch_lw and k_conv_patch_rows.
//      k_conv_patch_r8 (it replaces a tap row's fragments inside the walk, which fits `after`) and k_conv_patch_pf keep this loop
//      nest as their own text: through this function their builds changed register counts / scratch (LAB_NOTES.md, "Trunk conv
//      kernels").  Every kernel of the family walks chunk-major, then tap-column-major, through this nest: bit-identical accumulators.
template <int KH, int R, int MT, class After>
__device__ __forceinline__ void walk_tap_column(const unsigned char* src, int PW, const h8 (&A)[KH][MT], f4 (&acc)[R][MT], After after) {
#pragma unroll
    for (int pr = 0; pr < KH + R - 1; ++pr) {
        const h8 bf = *reinterpret_cast<const h8*>(src + pr * PW * 64);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int ky = pr - r;
            if (ky < 0 || ky >= KH) continue;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[ky][mt], bf, acc[r][mt], 0, 0, 0);
        }
        after(pr);
    }
}

// ---- where a wave's rows x 16 columns leave: the wave's first pixel once (64-bit, scalar), then row / column strides; (r, li) ->
//      element offset of pixel (row r, column li) in the output tensor, -1 past the map:
//          r < rows_ok && li < cols_ok ? wbase + r * rstride + li * cstride : -1ll
//      which each kernel hands to patch_epilogue as its own lambda (as a member of this struct the epilogue compiled to other,
//      shorter code: not the parent's).  oy, ox: the wave's first output pixel; output pixel (y, x) is written at
//      (y oy_mul + oy_off, x ox_mul + ox_off) of [outH][outW]; rows x cols: the map the wave's pixels must lie in.
struct WaveOut {
    long long wbase;
    int rstride, cstride, rows_ok, cols_ok;
};
__device__ __forceinline__ WaveOut wave_out(int outH, int outW, int out_ld, int n, int oy, int ox, int oy_mul, int oy_off, int ox_mul, int ox_off, int rows,
                                            int cols) {
    WaveOut w;
    w.wbase = (((long long)n * outH + oy * oy_mul + oy_off) * outW + ox * ox_mul + ox_off) * out_ld;
    w.rstride = oy_mul * outW * out_ld; w.cstride = ox_mul * out_ld;
    w.rows_ok = rows - oy; w.cols_ok = cols - ox;
    return w;
}
__device__ __forceinline__ WaveOut wave_out(const ConvP& p, int n, int oy, int ox) {
    return wave_out(p.outH, p.outW, p.out_ld, n, oy, ox, p.oy_mul, p.oy_off, p.ox_mul, p.ox_off, p.Ho, p.Wo);
}

}  // namespace vsrc
