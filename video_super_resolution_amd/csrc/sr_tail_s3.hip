// sr_tail_s3.hip -- k_tail_s3: the tail of the SR net for the scale-3 extension in one launch:
//   `out` DeconvBlock (ConvTranspose2d 32->32 k7 s3 p2 + PReLU) -> conv_out 3x3 (32 -> 3, bias, no activation)
// (SRProjectionModule.py:118-123,142 with SRFBN's (7, 3, 2) geometry) -> raw planes [N,3,3h,3w] fp32; the bilinear skip,
// add_mean and the fusion MLP ride on the read of these planes (csrc/sr_scale.hip k_fc_planes_skip_s).  The x3 map goes from the
// deconvolution to the 3x3 through an 8-row LDS ring and never reaches HBM (the unfused route -- sr.py:_PhaseDeconv, nine phase
// convolutions, + k_convout_planes, kept as the cross-check -- writes and re-reads 576 B per LR pixel and plane).  Built into a
// library of its own (libvsr_hip_s3t.so, include/vsr_hip_s3t.h: this file alone).
//
// Design = k_tail_s2's (sr_tail_s2.hip) with k_utd_s3's tap algebra (sr_utd_s3.hip):
//   * a workgroup of 4 waves marches down a strip of 30 LR columns; step m deconvolves the HR row TRIPLE 3m .. 3m+2 at the 32
//     positions q = x0-1 .. x0+30 (2 MFMA pixel tiles = HR columns 3(x0-1) .. 3(x0+30)+2: the 90 of the strip, one halo column
//     each side for the 3x3, two more that only discarded outputs read).  LR rows m-1, m, m+1 sit in a 4-row LDS ring.
//   * the waves own the stage's phase sets -- (1,1)(0,0) | (0,1)(2,1) | (1,0)(1,2) | (0,2)(2,0)(2,2): 13 / 12 / 12 / 12 taps, 2 x 2
//     MFMA 16x16x32 each -- with the weights in registers (26 fragments per wave); bias-seeded accumulators, PReLU, rounding to
//     fp16 (the rounding point of the unfused HR map), zeros outside the image (conv_out's padding is on the HR map), 16-byte
//     stores into the HR ring: 8 rows x 96 columns x 64 B, chunk index swizzled by the column (hr_off: the deconvolution writes
//     columns 3n + c from 16 lanes, the 3x3 reads 16 consecutive ones; both conflict-free on the lane groups of ds_write_b128 /
//     ds_read_b128).  Rows 3m-2 .. 3m+2 are read while 3m+3 .. 3m+5 may be written: 8 consecutive rows, 8 slots.
//   * one barrier; then conv_out on the three rows that became complete (3m-1, 3m, 3m+1): a unit = (row, 16-column tile) = 3 x 3
//     MFMAs whose A fragment holds conv_out's three output channels in rows 0-2 (M is 3/16 used) and whose B operand is the ring
//     row shifted by the tap; lanes 0-15 store the three channels.  The 18 units of a step go 4 / 5 / 5 / 4 to the waves:
//         wave      deconvolution + conv_out MFMAs
//         0         52 + 36 = 88
//         1         48 + 45 = 93
//         2         48 + 45 = 93
//         3         48 + 36 = 84
//     358 MFMAs per step against 372 if every wave ran at the critical waves' 93 (96 %).  `dec` (only the pixels (3i, 3j) leave,
//     what the nearest x1/3 resize of pass 1 reads): row 3m alone, 6 units, 1 / 2 / 2 / 1.
//   * every output pixel is one accumulation chain of a fixed order (the phase's taps, then the nine taps of the 3x3), whatever
//     strip, row segment or plane it falls in: rows_per_seg, N and the strip change no bit, and `dec` returns the full frame's values.
//   * FOLD: the FeedbackBlock's last compress_out (1x1 over the two live LR maps + constant map + PReLU) applied in the LR load
//     path exactly as k_tail_s2<.., FOLD> does: loader lanes are MFMA operand lanes (pixel 16 wv + l15 of waves 0-2, chunk g), bias +
//     map, then the two products (k_chain1x1's order), PReLU, natural channel order into the ring: bit-identical to the chain
//     launch followed by the plain build.
//     Its four fragments and bias sit in LDS behind the rings (in registers the build spilled), and the FOLD builds walk the conv units in
//     a loop where the plain builds unroll them (the unrolled max build spilled 8 bytes): same order of every sum.
// Two workgroups per CU (__launch_bounds__(256, 2): 256 registers per lane; 58,112 B of dynamic LDS each, 62,336 B with FOLD: 116 / 125 KB
// of the CU's 160).  As compiled by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage; max / select build): 252 / 239 VGPRs, FOLD
// 230 / 237, no AGPRs, scratch 0 bytes per lane, occupancy 2 waves per SIMD.
// Measured on an MI355X (tools/tail_s3_time.py): 8 x 720 x 1280 in 2.36 ms = 362 TFLOP/s at 115,904 FLOP per pixel and plane, against
// 7.21 ms of the unfused launches; decimated 1.48 against 4.07 ms; FOLD 2.65 ms against 2.74 ms for chain launch + plain build.
#include "sr_s3_taps.h"
#include "sr_strip30.h"

#include "../../include/vsr_hip_s3t.h"

namespace {

constexpr int T3_HR_COLS = 96;                // HR columns 3 (x0-1) .. 3 (x0+30) + 2
constexpr int T3_HR_ROW = T3_HR_COLS * 64;    // x 32 channels fp16
constexpr int T3_HR_ROWS = 8;                 // rows 3m-2 .. 3m+2 are read while 3m+3 .. 3m+5 may already be written
constexpr int T3_HR_BYTES = T3_HR_ROWS * T3_HR_ROW;
constexpr int T3_BIAS_BYTES = 256;
constexpr int T3_LDS = S30_LR_BYTES + T3_HR_BYTES + T3_BIAS_BYTES;
constexpr int T3_CO_BYTES = 4096 + 128;       // FOLD: compress_out's four fragments + b_co[32] (read at use: the register budget)
static_assert(T3_LDS + T3_CO_BYTES <= 64 * 1024, "dynamic LDS without the large-LDS attribute");
static_assert(2 * (T3_LDS + T3_CO_BYTES) <= 160 * 1024, "two workgroups per CU");

constexpr int T3_SLOTS = 13;                                  // tap fragments per wave (waves 1-3 use 12)
constexpr int T3_BLOB_UP = 0;                                 // [wave 4][slot 13][mt 2][lane 64][8] fp16 (as k_utd_s3)
constexpr int T3_BLOB_CV = 4 * T3_SLOTS * 2 * 1024;           // [dy 3][dx 3][lane 64][8] fp16: rows 0-2 = conv_out's channels
constexpr int T3_BLOB_F32 = T3_BLOB_CV + 9 * 1024;            // b_out[32], b_cv[3], pad, slope_out at [96]
constexpr int T3_BLOB_BYTES = T3_BLOB_F32 + 512;
constexpr int T3_BLOB_CO = T3_BLOB_BYTES;                     // FOLD: [map 2][mt 2][lane 64][8] fp16 (natural channel order), then b_co[32], slope_co (64 floats)
constexpr int T3_BLOB_FOLD_BYTES = T3_BLOB_CO + 4096 + 256;

typedef unsigned int u4t __attribute__((ext_vector_type(4)));

template <bool ALLMAX, bool FOLD>
__global__ void __launch_bounds__(256, 2)
k_tail_s3(const _Float16* __restrict__ in, const unsigned char* __restrict__ blob, float* __restrict__ raw, int h, int w,
          int rows_per_seg, int dec, const _Float16* __restrict__ in2, const float* __restrict__ cmap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const lrr = smem;
    unsigned char* const hrr = smem + S30_LR_BYTES;
    float* const bias_s = reinterpret_cast<float*>(smem + S30_LR_BYTES + T3_HR_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * S30_TX;
    const int n = blockIdx.z;
    const int r0 = blockIdx.y * rows_per_seg;
    const int r1 = min(h, r0 + rows_per_seg);
    if (r0 >= r1) return;   // uniform per workgroup

    // ---- weights -> registers, once per workgroup (slot 12 of waves 1-3 is zero padding that no step reads)
    h8 Aup[T3_SLOTS][2], Acv[3][3];
#pragma unroll
    for (int t = 0; t < T3_SLOTS; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            Aup[t][mt] = *reinterpret_cast<const h8*>(blob + T3_BLOB_UP + (((wv * T3_SLOTS + t) * 2 + mt) * 64 + lane) * 16);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) Acv[dy][dx] = *reinterpret_cast<const h8*>(blob + T3_BLOB_CV + ((dy * 3 + dx) * 64 + lane) * 16);
    const float* fpar = reinterpret_cast<const float*>(blob + T3_BLOB_F32);
    if (tid < 64) bias_s[tid] = fpar[tid];   // b_out[0..31], b_cv at [32..34] (visible after the prologue's barrier)
    // this lane's accumulator rows are channels {4g..4g+3} of tile mt
    auto bup = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(bias_s + 16 * mt + 4 * g); };
    const float a_up = fpar[96];
    const h2 a_up2 = {(_Float16)a_up, (_Float16)a_up};
    const bool up_max = ALLMAX || a_up <= 1.0f;
    // conv_out accumulator rows 4g + e: channels 0-2 live in lane group 0 only
    const f4 bcv = g == 0 ? f4{fpar[32], fpar[33], fpar[34], 0.0f} : f4{0.0f, 0.0f, 0.0f, 0.0f};

    // ---- LR loader: 34 columns x 4 chunks of 16 bytes per row; out-of-image pieces read zeros (out-of-range buffer offset)
    const __amdgpu_buffer_rsrc_t in_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(in), 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t in2_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(FOLD ? in2 : in), 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t cm_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(FOLD ? cmap : fpar), 0, FOLD ? (int)((size_t)h * w * NF * 4) : 0, 0x00020000);
    // FOLD: loader lanes are MFMA operand lanes -- pixel 16 wv + l15 (waves 0-2: 48 >= 34 columns), channel chunk g
    const int lr_px = FOLD ? 16 * wv + l15 : tid >> 2, lr_ch = FOLD ? g : tid & 3, lr_col = x0 - 2 + lr_px;
    const bool lr_loader = FOLD ? (wv < 3 && lr_px < S30_LRC) : tid < S30_LRC * 4;
    const bool lr_col_ok = lr_loader && lr_col >= 0 && lr_col < w;
    const int lr_st = lr_off(lr_px, lr_ch);
    // FOLD: where the two halves of a lane's activated tile pair (channels 4g..4g+3 and 16+4g..16+4g+3) lie in natural order
    const int lr_st_lo = lr_off(lr_px, g >> 1) + (g & 1) * 8, lr_st_hi = lr_off(lr_px, 2 + (g >> 1)) + (g & 1) * 8;
    struct RawRow {
        u4t a, b, c0, c1;
    };
    // FOLD: compress_out's fragments and bias live in LDS behind the rings (in registers the build spilled 24 of them)
    unsigned char* const co_s = smem + T3_LDS;
    float a_co = 1.0f;
    if (FOLD) {
        *reinterpret_cast<u4t*>(co_s + tid * 16) = *reinterpret_cast<const u4t*>(blob + T3_BLOB_CO + tid * 16);
        if (tid < 8) *reinterpret_cast<u4t*>(co_s + 4096 + tid * 16) = *reinterpret_cast<const u4t*>(blob + T3_BLOB_CO + 4096 + tid * 16);
        a_co = reinterpret_cast<const float*>(blob + T3_BLOB_CO + 4096)[32];
        __syncthreads();   // (the prologue's LR rows go through these)
    }
    auto aco = [&](int t, int mt) __attribute__((always_inline)) { return *reinterpret_cast<const h8*>(co_s + ((t * 2 + mt) * 64 + lane) * 16); };
    auto bco = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(co_s + 4096 + (16 * mt + 4 * g) * 4); };
    const h2 a_co2 = {(_Float16)a_co, (_Float16)a_co};
    const bool co_max = a_co <= 1.0f;
    auto fetch_lr = [&](int row) __attribute__((always_inline)) -> RawRow {
        const bool ok = lr_col_ok && row >= 0 && row < h;
        const unsigned off = ok ? (unsigned)(((((size_t)n * h + row) * w + lr_col) * NF + lr_ch * 8) * 2) : 0xFFFFFFFFu;
        RawRow v;
        v.a = __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off, 0, 0);
        if (FOLD) {
            v.b = __builtin_amdgcn_raw_buffer_load_b128(in2_rsrc, off, 0, 0);
            const unsigned coff = ok ? (unsigned)((((size_t)row * w + lr_col) * NF + 4 * g) * 4) : 0xFFFFFFFFu;
            v.c0 = __builtin_amdgcn_raw_buffer_load_b128(cm_rsrc, coff, 0, 0);
            v.c1 = __builtin_amdgcn_raw_buffer_load_b128(cm_rsrc, ok ? coff + 64 : 0xFFFFFFFFu, 0, 0);
        }
        return v;
    };
    // LR row -> ring: the fetched piece, or (FOLD) PReLU(W_co [a; b] + b_co + cmap) of the lane's pixel -- bias + map, then the two
    // products: k_chain1x1's order -- and zero outside the image (the deconvolution's padding applies to the 1x1's OUTPUT).  The MFMAs
    // run on whole waves (wave-uniform guard), the stores on the loader lanes.
    auto store_lr = [&](const RawRow& v, int row) __attribute__((always_inline)) {
        unsigned char* const slot = lrr + ((row + 4) & 3) * S30_LR_SLOT;
        if (!FOLD) {
            if (lr_loader) *reinterpret_cast<u4t*>(slot + lr_st) = v.a;
            return;
        }
        if (wv < 3) {
            f4 acc[2] = {bco(0) + __builtin_bit_cast(f4, v.c0), bco(1) + __builtin_bit_cast(f4, v.c1)};
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                acc[mt] = mfma16(aco(0, mt), __builtin_bit_cast(h8, v.a), acc[mt]);
                acc[mt] = mfma16(aco(1, mt), __builtin_bit_cast(h8, v.b), acc[mt]);
            }
            const u4t o = __builtin_bit_cast(u4t, act_pack(acc[0], acc[1], a_co2, co_max));
            const bool ok = lr_col_ok && row >= 0 && row < h;
            typedef unsigned int u2t __attribute__((ext_vector_type(2)));
            if (lr_loader) {
                *reinterpret_cast<u2t*>(slot + lr_st_lo) = u2t{ok ? o[0] : 0u, ok ? o[1] : 0u};
                *reinterpret_cast<u2t*>(slot + lr_st_hi) = u2t{ok ? o[2] : 0u, ok ? o[3] : 0u};
            }
        }
    };
    auto lr_slot = [&](int row) __attribute__((always_inline)) { return ((row + 4) & 3) * S30_LR_SLOT; };   // (row >= -4)
    auto hr_slot = [&](int Y) __attribute__((always_inline)) { return (Y & (T3_HR_ROWS - 1)) * T3_HR_ROW; };  // (two's complement: Y may be negative)

    // ---- prologue: LR rows r0-2, r0-1, r0 (the first triple, m = r0-1, reads them)
    store_lr(fetch_lr(r0 - 2), r0 - 2);
    store_lr(fetch_lr(r0 - 1), r0 - 1);
    store_lr(fetch_lr(r0), r0);
    __syncthreads();

    // lanes whose deconv position q lies outside the image (HR columns 3q .. 3q+2) hold conv_out's zero padding
    bool col_ok[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int q = x0 - 1 + 16 * nt + l15;
        col_ok[nt] = q >= 0 && q < w;
    }

    // ---- deconvolution role WV: its phases of the HR row triple m -> PReLU -> fp16 -> HR ring (zero rows outside the image)
    auto deconv = [&](auto role, int m, bool live) __attribute__((always_inline)) {
        constexpr int WV = decltype(role)::value;
#pragma unroll
        for (int p = 0; p < ph_cnt(WV); ++p) {
            const int r = ph_r(WV, p), c = ph_c(WV, p);
            h8 T[2];
            if (live) {
                f4 d[2][2];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) d[mt][nt] = bup(mt);
#pragma unroll
                for (int di = 1; di >= -1; --di) {
                    if (!tap_ok(r, di)) continue;
                    const unsigned char* rowp = lrr + lr_slot(m + di);
#pragma unroll
                    for (int dj = 1; dj >= -1; --dj) {
                        if (!tap_ok(c, dj)) continue;
                        const int slot = tap_slot(WV, p, di, dj);
                        h8 B[2];
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) B[nt] = *reinterpret_cast<const h8*>(rowp + lr_off(16 * nt + l15 + 1 + dj, g));
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt) d[mt][nt] = mfma16(Aup[slot][mt], B[nt], d[mt][nt]);
                    }
                }
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    h8 t = act_pack(d[0][nt], d[1][nt], a_up2, up_max);
                    if (!col_ok[nt]) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) t[e] = (_Float16)0.0f;
                    }
                    T[nt] = t;
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int e = 0; e < 8; ++e) T[nt][e] = (_Float16)0.0f;
            }
            // HR ring: row 3m + r, columns 3 n + c
            unsigned char* const rowp = hrr + hr_slot(3 * m + r);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) *reinterpret_cast<h8*>(rowp + hr_off(3 * (16 * nt + l15) + c, g)) = T[nt];
        }
    };

    // ---- conv role: units [ubeg, uend) of the step's (row, tile) list -- full: 18 = rows 3m-1, 3m, 3m+1 x 6 tiles, 4 / 5 / 5 / 4;
    // dec: row 3m alone, 1 / 2 / 2 / 1
    const int ubeg = dec ? (wv == 0 ? 0 : 2 * wv - 1) : (wv == 0 ? 0 : 5 * wv - 1);
    const int uend = dec ? (wv == 3 ? 6 : 2 * wv + 1) : (wv == 3 ? 18 : 5 * wv + 4);
    const int Ho = dec ? h : 3 * h, Wo = dec ? w : 3 * w;
    const size_t plane = (size_t)Ho * Wo;
    float* const raw_n = raw + (size_t)n * 3 * plane;

    for (int m = r0 - 1; m <= r1; ++m) {
        const RawRow nxt = fetch_lr(m + 2);
        const bool live = m >= 0 && m < h;   // (uniform) triples outside the image are conv_out's zero padding
        switch (wv) {
            case 0: deconv(IntC<0>{}, m, live); break;
            case 1: deconv(IntC<1>{}, m, live); break;
            case 2: deconv(IntC<2>{}, m, live); break;
            default: deconv(IntC<3>{}, m, live); break;
        }
        store_lr(nxt, m + 2);   // over row m-2 (last read in step m-1)
        __syncthreads();
        // ---- conv_out for the output rows 3m-1, 3m, 3m+1 (HR rows 3m-2 .. 3m+2 are in the ring)
        auto conv_unit = [&](int u) __attribute__((always_inline)) {
            const int k = dec ? 1 : (u >= 12 ? 2 : u >= 6 ? 1 : 0), t = dec ? u : u - 6 * k;
            const int Y = 3 * m - 1 + k;
            if (Y < 3 * r0 || Y >= 3 * r1) return;                // (uniform) rows of the neighbouring segments / outside the image
            if (3 * (x0 - 1) + 16 * t >= 3 * w) return;           // (uniform) tiles right of the image
            const int xr = 16 * t + l15;                          // ring column 0..95  <->  X = 3 (x0 - 1) + xr
            f4 acc = bcv;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const unsigned char* rowp = hrr + hr_slot(Y + dy - 1);
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int xs = xr + dx - 1;
                    h8 B;
                    if (xs >= 0 && xs < T3_HR_COLS) B = *reinterpret_cast<const h8*>(rowp + hr_off(xs, g));
                    else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) B[e] = (_Float16)0.0f;   // (window edge: only discarded outputs read it)
                    }
                    acc = mfma16(Acv[dy][dx], B, acc);
                }
            }
            // live output columns of the strip: X in [3 x0, 3 x0 + 90) and inside the image
            const int X = 3 * (x0 - 1) + xr;
            int Xd = X, Yd = Y;
            bool ok = (g == 0) && xr >= 3 && xr < 3 + 3 * S30_TX && X < 3 * w;
            if (dec) {
                Xd = (int)((unsigned)X / 3u);
                Yd = m;
                ok = ok && Xd * 3 == X;
            }
            if (ok) {
                const size_t o = (size_t)Yd * Wo + Xd;
                raw_n[o] = acc[0];
                raw_n[plane + o] = acc[1];
                raw_n[2 * plane + o] = acc[2];
            }
        };
        // (the plain builds unroll the units -- the reads of one beside the MFMA chain of another; with the fold's four loads in
        // flight that costs a spill, so the FOLD builds walk them one by one: same order of every sum, same bits)
        if (FOLD) {
#pragma unroll 1
            for (int u = ubeg; u < uend; ++u) conv_unit(u);
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i)
                if (ubeg + i < uend) conv_unit(ubeg + i);   // (uniform)
        }
    }
}

typedef void (*kern_t)(const _Float16*, const unsigned char*, float*, int, int, int, int, const _Float16*, const float*);

int launch_tail_s3(const void* in, const void* in2, const float* cmap, const void* blob, float* raw, int N, int h, int w, int rows_per_seg,
                   int slopes_le_one, int decimate, vsr_stream_t stream, const char* what) {
    VSR_REQUIRE(in && blob && raw, "%s: null pointer", what);
    VSR_REQUIRE(N > 0 && h > 0 && w > 0 && rows_per_seg >= 0 && N <= 65535, "%s: bad shape (N %d, h %d, w %d, rows_per_seg %d)", what, N, h, w,
                rows_per_seg);
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(in2) & 15) == 0 && (reinterpret_cast<uintptr_t>(blob) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(cmap) & 15) == 0 && (reinterpret_cast<uintptr_t>(raw) & 3) == 0,
                "%s: inputs must be 16-byte aligned, the planes 4-byte aligned", what);
    const size_t in_bytes = (size_t)N * h * w * NF * 2, cm_bytes = (size_t)h * w * NF * 4;
    const size_t raw_bytes = (size_t)N * 3 * (decimate ? (size_t)h * w : (size_t)9 * h * w) * 4;
    VSR_REQUIRE(!ranges_overlap(in, in_bytes, raw, raw_bytes) && !(in2 && ranges_overlap(in2, in_bytes, raw, raw_bytes)) &&
                    !(cmap && ranges_overlap(cmap, cm_bytes, raw, raw_bytes)) &&
                    !ranges_overlap(blob, in2 ? T3_BLOB_FOLD_BYTES : T3_BLOB_BYTES, raw, raw_bytes),
                "%s: the planes must not overlap an input", what);
    if (in_bytes >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "%s: input beyond 4 GiB (split the planes)", what);
    if (in2 && cm_bytes >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "%s: constant map beyond 4 GiB", what);
    if (rows_per_seg == 0) rows_per_seg = h;   // one march per strip
    const unsigned strips = vsr::cdiv(w, S30_TX), segs = vsr::cdiv(h, rows_per_seg);
    VSR_REQUIRE(segs <= 65535, "%s: too many row segments", what);
    const kern_t k = in2 ? (slopes_le_one ? k_tail_s3<true, true> : k_tail_s3<false, true>) : (slopes_le_one ? k_tail_s3<true, false> : k_tail_s3<false, false>);
    hipLaunchKernelGGL(k, dim3(strips, segs, N), dim3(256), T3_LDS + (in2 ? T3_CO_BYTES : 0), vsr::S(stream), (const _Float16*)in, (const unsigned char*)blob, raw, h, w,
                       rows_per_seg, decimate, (const _Float16*)in2, cmap);
    return vsr::launched(what);
}

}  // namespace

extern "C" {

int vsr_s3t_abi_version(void) { return VSR_S3T_ABI_VERSION; }
const char* vsr_s3t_last_error(void) { return vsr::err_buf(); }

size_t vsr_s3t_query(int what) {
    switch (what) {
        case VSR_S3T_Q_BLOB_BYTES: return T3_BLOB_BYTES;
        case VSR_S3T_Q_BLOB_FOLD_BYTES: return T3_BLOB_FOLD_BYTES;
        case VSR_S3T_Q_STRIP_WIDTH: return S30_TX;
        default: return 0;
    }
}

int vsr_s3t_sr_tail_f16(const void* in, const void* blob, float* raw, int N, int h, int w, int rows_per_seg, int slopes_le_one, int decimate,
                        vsr_stream_t stream) {
    return launch_tail_s3(in, nullptr, nullptr, blob, raw, N, h, w, rows_per_seg, slopes_le_one, decimate, stream, "s3t_sr_tail");
}

int vsr_s3t_sr_tail_fold_f16(const void* lr3, const void* lr6, const float* cmap, const void* blob, float* raw, int N, int h, int w,
                             int rows_per_seg, int slopes_le_one, int decimate, vsr_stream_t stream) {
    VSR_REQUIRE(lr3 && lr6 && cmap, "s3t_sr_tail_fold: null pointer");
    return launch_tail_s3(lr3, lr6, cmap, blob, raw, N, h, w, rows_per_seg, slopes_le_one, decimate, stream, "s3t_sr_tail_fold");
}

}  // extern "C"
