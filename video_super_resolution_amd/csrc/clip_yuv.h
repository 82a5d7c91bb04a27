// clip_yuv.h -- what the planar Y'CbCr sources share (clip_yuv.hip: 4:2:0, include/vsr_hip_yuv.h; clip_pix.hip: 4:2:2 and 4:4:4,
// include/vsr_hip_pix.h): the coefficient block, the per-axis siting rules, the two fma nests and the run store.  Each source is a
// library of its own; everything here is in an unnamed namespace or inline, so neither exports a symbol from it.
#pragma once
#include "vsr_common.h"

namespace {

struct Coef {
    float a[9];
    float o[3];
};

// midway siting along one axis: luma index i between chroma samples i0 (weight w0) and i1 (weight 1 - w0), clamped to 0..n-1
__device__ inline void midway(int i, int n, int& i0, int& i1, float& w0) {
    const int k = i >> 1;
    if (i & 1) {
        i0 = k, i1 = k + 1 < n ? k + 1 : n - 1, w0 = 0.75f;
    } else {
        i0 = k > 0 ? k - 1 : 0, i1 = k, w0 = 0.25f;
    }
}

// co-sited along one axis: even luma index = the sample, odd = the mean of its neighbours
__device__ inline void cosited(int i, int n, int& i0, int& i1, float& w0) {
    const int k = i >> 1;
    i0 = k;
    if (i & 1) {
        i1 = k + 1 < n ? k + 1 : n - 1, w0 = 0.5f;
    } else {
        i1 = k, w0 = 1.0f;
    }
}

__device__ inline void to_rgb(const Coef& k, float yc, float cb, float cr, float* out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = __builtin_fmaf(k.a[3 * c + 2], cr, __builtin_fmaf(k.a[3 * c + 1], cb, __builtin_fmaf(k.a[3 * c], yc, k.o[c])));
        out[c] = fminf(fmaxf(v, 0.0f), 255.0f);
    }
}

__device__ inline float clamp255(float v) {
    v = v >= 0.0f ? v : 0.0f;   // negatives and NaN
    return v > 255.0f ? 255.0f : v;
}

__device__ inline float dot_row(const Coef& k, int c, float r, float g, float b) {
    return __builtin_fmaf(k.a[3 * c + 2], b, __builtin_fmaf(k.a[3 * c + 1], g, __builtin_fmaf(k.a[3 * c], r, k.o[c])));
}

// N samples (codes already positioned in their words) to consecutive addresses: one store when WIDE, element stores otherwise
template <typename T, int N, bool WIDE>
__device__ inline void store_run(T* q, const unsigned* c) {
    if constexpr (WIDE) {
        constexpr int per = 4 / (int)sizeof(T);   // samples per 32-bit word
        constexpr int NW = N / per;
        static_assert(NW == 1 || NW == 2 || NW == 4, "a run is one 4-, 8- or 16-byte store");
        unsigned w[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if constexpr (sizeof(T) == 1) w[i] = c[4 * i] | (c[4 * i + 1] << 8) | (c[4 * i + 2] << 16) | (c[4 * i + 3] << 24);
            else w[i] = c[2 * i] | (c[2 * i + 1] << 16);
        }
        if constexpr (NW == 1) *reinterpret_cast<unsigned*>(q) = w[0];
        else if constexpr (NW == 2) *reinterpret_cast<uint2*>(q) = make_uint2(w[0], w[1]);
        else *reinterpret_cast<uint4*>(q) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = (T)c[i];
    }
}

inline Coef read_coef(const float* coef12) {
    Coef k;
    for (int i = 0; i < 9; ++i) k.a[i] = coef12[i];
    for (int i = 0; i < 3; ++i) k.o[i] = coef12[9 + i];
    return k;
}

}  // namespace
