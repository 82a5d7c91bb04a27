// sr_mfma32.h -- the operand vocabulary of the fused stages on v_mfma_f32_32x32x16_f16 (sr_utd4.hip: k_utd4;  sr_utd_s2w.hip: k_utd_s2w).
// A lane holds 16 channels of ONE pixel / deconv position: its accumulator, PReLU'd and packed to fp16 pairs, IS the B operand of the
// next product (channel order ch(kb, kh, e) = 16 kb + 8 (e / 4) + 4 kh + e % 4, sr_pack.py: layout=4), and a one-pixel shift of the
// tile is one whole-wave DPP move per register.
#pragma once
#include "sr_f16_common.h"

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f2v4 __attribute__((ext_vector_type(2)));
typedef unsigned int u4w __attribute__((ext_vector_type(4)));
typedef unsigned int u2w __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f16v mfma32(h8 a, h8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// One column phase's operand of the next product: the lane's 16 channels of one pixel as 8 packed fp16 pairs; dwords 4 kb .. 4 kb + 3 are
// the B operand of K block kb.  (Kept as dwords: the hand-placed activation stages finish them one at a time, in place.)
struct Ob {
    h2 d[8];
};
__device__ __forceinline__ h8 opk(const Ob& o, int kb) {
    return h8{o.d[4 * kb][0], o.d[4 * kb][1], o.d[4 * kb + 1][0], o.d[4 * kb + 1][1], o.d[4 * kb + 2][0], o.d[4 * kb + 2][1], o.d[4 * kb + 3][0], o.d[4 * kb + 3][1]};
}
// 16 accumulator values of a lane -> PReLU -> 8 packed fp16 pairs (plain form: cold rows)
__device__ __forceinline__ Ob act16(const f16v& a, h2 slope, bool use_max) {
    Ob o;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const h2 c = __builtin_convertvector(f2v4{a[2 * d], a[2 * d + 1]}, h2);
        const h2 m = c * slope;
        o.d[d] = use_max ? __builtin_elementwise_max(c, m) : __builtin_elementwise_min(c, m);
    }
    return o;
}
// The same as 24 single instructions the step schedule places one by one ("program positions" 0..23): convert 0, convert 1, then per
// dword pair p = 0..2: multiply 2p, multiply 2p+1, convert 2p+2, max 2p, max 2p+1, convert 2p+3; then multiply 6, 7, max 6, 7.
// Chunks of the program that end behind a convert -- [0,2) [2,5) [5,8) [8,11) [11,14) [14,17) [17,20) [20,24): chunk c begins at
// act_chunk_begin(c) -- keep a packed-math instruction (v_pk_mul / v_pk_max) from being the last one in front of the next MFMA: that
// costs an s_nop every time (seen in the ISA: none behind v_cvt_pk_f16_f32, v_add_f32, DPP moves).  Each result is pinned to the gap it
// is written in.  ZERO: the result is zeroed where `keep` is false (columns outside the image: the conv's zero padding).
struct ActT {
    h2 c[8], m[8];
};
__device__ __forceinline__ constexpr int act_chunk_begin(int c) { return c == 0 ? 0 : (c >= 8 ? 24 : 3 * c - 1); }
template <bool ZERO>
__device__ __forceinline__ void act_st(int j, const f16v& a, ActT& t, Ob& o, h2 slope, bool use_max, bool keep) {
    // position -> (operation 0 convert / 1 multiply / 2 max, dword)
    int op, d;
    if (j < 2) { op = 0; d = j; }
    else if (j < 20) {
        const int p = (j - 2) / 6, k = (j - 2) % 6;
        op = (k == 2 || k == 5) ? 0 : (k < 2 ? 1 : 2);
        d = k == 2 ? 2 * p + 2 : k == 5 ? 2 * p + 3 : ((k == 0 || k == 3) ? 2 * p : 2 * p + 1);
    } else { op = j < 22 ? 1 : 2; d = 6 + (j & 1); }
    if (op == 0) {
        t.c[d] = __builtin_convertvector(f2v4{a[2 * d], a[2 * d + 1]}, h2);
        asm volatile("" : : "v"(t.c[d]));
    } else if (op == 1) {
        t.m[d] = t.c[d] * slope;
        asm volatile("" : : "v"(t.m[d]));
    } else {
        h2 r = use_max ? __builtin_elementwise_max(t.c[d], t.m[d]) : __builtin_elementwise_min(t.c[d], t.m[d]);
        if (ZERO) r = keep ? r : h2{(_Float16)0.0f, (_Float16)0.0f};
        o.d[d] = r;
        asm volatile("" : : "v"(o.d[d]));
    }
}

// the tile moved down one pixel: lane j takes lane j + 1 (whole-wave shift; lane 31 / 63 -- position 32, which only the discarded
// outputs read -- take whatever the neighbour holds)
__device__ __forceinline__ h2 shift1d(h2 v) {
    return __builtin_bit_cast(h2, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));   // wave_shl:1
}
__device__ __forceinline__ Ob shift1(const Ob& v) {
    Ob o;
#pragma unroll
    for (int d = 0; d < 8; ++d) o.d[d] = shift1d(v.d[d]);
    return o;
}

// byte offset of (pixel p, 16-byte piece) inside an LR row slot for THESE kernels' operand reads -- 32 consecutive pixels, one piece per
// half wave: the piece XOR pixel bits 2-3.  (lr_off's XOR of bits 1-2 serves 16-pixel x 4-piece reads; on this pattern it gives two-way
// bank conflicts, 8 cycles per ds_read_b128 instead of 4: tools/lds_bank_sim.py; PMC on k_utd_s2w: 41 % of the LDS-active cycles were
// conflicts.)
__device__ __forceinline__ int lr_off32(int p, int chunk) { return p * 64 + ((chunk ^ ((p >> 2) & 3)) << 4); }

}  // namespace
