// frame_ssim.h -- the SSIM window march, written once for k_metric (frame_metric.hip) and k_score (frame_msssim.hip), and the host
// pieces their two entries share.
//
// One workgroup (NW = 4 waves) scores a tile of SW = 64 map columns x SR = 64 map rows of one plane; it reads (SW + 10) x (SR + 10) values.
// The tile marches down its rows four at a time: in step t wave v takes input row 4 t + v.
//   load    : stage_row: the row's 74 x 3 floats of a and of b into LDS as they lie in memory (WIDE: one aligned 16-byte load per lane;
//             otherwise four element loads per lane)
//   convert : lane l takes pixels l and l + 64: level1 (quantise, luma or channel p, to double) into the converted row of XS doubles;
//             k_metric takes its SSE here, k_score reads the rows of its higher levels as doubles instead
//   rows    : row_pass: lane c = map column c: the five 11-tap sums along the row into slot (row % RING) of an LDS ring of NW + 10 = 14 rows
//   columns : column_pass: wave v takes map row 4 t + v - 10, whose eleven ring rows are complete once row 4 t + 3 is: the five 11-tap
//             sums down the column and the four terms of the formula; the kernel forms its quotients from them
// with a barrier after each of load, convert and rows; the next step's ring stores come after its first barriers, when every read of
// the column pass has been issued.  RGB runs the march once per plane with one ring (36 KB; three would leave one workgroup per
// compute unit).
//
// For frame_metric.hip and frame_msssim.hip ONLY, under the rules of frame_sums.h: sources compiled with -ffp-contract=off (Makefile)
// that state the pragma themselves, whose results tests/test_gpu_score_bits.py pins bit for bit.  Every operation below rounds once, in
// the order written; the window sums ask for their fmas by name.
#pragma once
#include <type_traits>

#include "frame_sums.h"
#include "vsr_common.h"

#pragma clang fp contract(off)

namespace vsr {
namespace ssim {

using sums::Luma;
using sums::quant;

constexpr int SW = 64, SR = 64;    // the tile: map columns (a strip) x map rows (a row segment)
constexpr int NW = 4;              // waves per workgroup = input rows per step
constexpr int K = 11;              // window taps
constexpr int RING = NW + K - 1;   // ring rows: the 11 rows of the oldest map row of a step up to the newest input row
constexpr int RAW = 256;           // floats of one staged row: 74 x 3 = 222, + 3 before an aligned start, rounded up to 64 lanes x 4
constexpr int XS = 80;             // doubles of one converted row (74 used)
constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);

struct Win {
    double w[K];
};
inline Win win_of(const double* win11) {
    Win win;
    for (int i = 0; i < K; ++i) win.w[i] = win11[i];
    return win;
}

// a row's `nfl` floats starting at float `s` of the frames fa and fb into raw[0] and raw[1]; returns where the row starts in both.
// The two frames go together: an element load of a and of b under one condition keeps both in flight and pairs their LDS stores;
// a's four loads, then b's four, measured 733 us against 538 (k_metric, RGB, 2160 x 3840, unaligned bases).
template <bool WIDE>
__device__ inline int stage_row(float (*raw)[RAW], const float* __restrict__ fa, const float* __restrict__ fb, size_t s, int nfl, int lane) {
    if (WIDE) {
        const size_t s4 = s & ~(size_t)3;   // H * W * 3 is a multiple of 4: an aligned group ends inside the frame
        const int o = (int)(s - s4);
        if (4 * lane < o + nfl) {
            *reinterpret_cast<float4*>(&raw[0][4 * lane]) = *reinterpret_cast<const float4*>(fa + s4 + 4 * lane);
            *reinterpret_cast<float4*>(&raw[1][4 * lane]) = *reinterpret_cast<const float4*>(fb + s4 + 4 * lane);
        }
        return o;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        if (i < nfl) {
            raw[0][i] = fa[s + i];
            raw[1][i] = fb[s + i];
        }
    }
    return 0;
}

// plane `p` of the pixel at q[0..2] as the double of level 1 (Y: the luma; RGB: channel p)
template <bool YMODE, bool QUANT>
__device__ inline double level1(const float* q, int p, const Luma& lu) {
    if (YMODE) {
        const float r = QUANT ? quant(q[0]) : q[0], g = QUANT ? quant(q[1]) : q[1], b = QUANT ? quant(q[2]) : q[2];
        return sums::luma(lu, r, g, b);
    }
    return (double)(QUANT ? quant(q[p]) : q[p]);
}

// rows: the five 11-tap sums of a converted row from this lane's column on (xa, xb: the two frames' doubles there) into a ring slot
__device__ inline void row_pass(const Win& win, const double* xa, const double* xb, double (*slot)[SW], int lane) {
    double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double va = xa[k], vb = xb[k];
        const double paa = va * va, pbb = vb * vb, pab = va * vb;
        sa = __builtin_fma(win.w[k], va, sa);
        sb = __builtin_fma(win.w[k], vb, sb);
        saa = __builtin_fma(win.w[k], paa, saa);
        sbb = __builtin_fma(win.w[k], pbb, sbb);
        sab = __builtin_fma(win.w[k], pab, sab);
    }
    slot[0][lane] = sa;
    slot[1][lane] = sb;
    slot[2][lane] = saa;
    slot[3][lane] = sbb;
    slot[4][lane] = sab;
}

// SSIM = (num_l * num_cs) / (den_l * den_cs), its contrast-structure part num_cs / den_cs
struct Terms {
    double num_l, den_l, num_cs, den_cs;   // {2 mab + C1, (maa + mbb) + C1, 2 s_ab + C2, (s_aa + s_bb) + C2}
};

// columns: map row q needs input rows q .. q + 10 of the ring: the five 11-tap sums down this lane's column, then the terms
__device__ inline Terms column_pass(const Win& win, const double (*ring)[5][SW], int q, int lane) {
    double ma = 0.0, mb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
    int slot = q % RING;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        ma = __builtin_fma(win.w[k], ring[slot][0][lane], ma);
        mb = __builtin_fma(win.w[k], ring[slot][1][lane], mb);
        eaa = __builtin_fma(win.w[k], ring[slot][2][lane], eaa);
        ebb = __builtin_fma(win.w[k], ring[slot][3][lane], ebb);
        eab = __builtin_fma(win.w[k], ring[slot][4][lane], eab);
        slot = slot + 1 == RING ? 0 : slot + 1;
    }
    const double maa = ma * ma, mbb = mb * mb, mab = ma * mb;
    const double s_aa = eaa - maa, s_bb = ebb - mbb, s_ab = eab - mab;
    return {2.0 * mab + C1, (maa + mbb) + C1, 2.0 * s_ab + C2, (s_aa + s_bb) + C2};
}

// ---- host: what the two entries check and decide alike; `who` is the entry's own prefix of the message
inline int check_pointers(const char* who, const void* a, const void* b, const void* sums, const void* ws) {
    VSR_REQUIRE(a && b && sums && ws, "%s: null pointer", who);
    return VSR_OK;
}
inline int check_quantise(const char* who, int quantise) {
    VSR_REQUIRE(quantise == 0 || quantise == 1, "%s: quantise must be 0 or 1, got %d", who, quantise);
    return VSR_OK;
}
// the luma of Y mode and the alignment of the four device pointers; *wide: 16-byte loads, for both bases aligned and a row pitch (so a
// frame) of a whole number of 16-byte groups
inline int check_frames(const char* who, bool ymode, const float* luma4, const float* a, const float* b, int W, const double* sums,
                        const void* ws, bool* wide) {
    VSR_REQUIRE(!ymode || luma4, "%s: null luma4 in Y mode", who);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    VSR_REQUIRE(((pa | pb) & 3) == 0, "%s: the frames must be 4-byte aligned", who);
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "%s: sums and the workspace must be 8-byte aligned", who);
    *wide = ((pa | pb) & 15) == 0 && W % 4 == 0;
    return VSR_OK;
}

// f(X, Y) with the two run-time switches as std::bool_constant types: the (quant, wide) pair of a launch -> template arguments
template <class F>
inline void dispatch(bool x, bool y, F&& f) {
    if (x && y) f(std::true_type{}, std::true_type{});
    else if (x) f(std::true_type{}, std::false_type{});
    else if (y) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

}  // namespace ssim
}  // namespace vsr
