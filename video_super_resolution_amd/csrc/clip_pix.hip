// clip_pix.hip -- planar Y'CbCr 4:2:2 and 4:4:4 frames either side of the path (include/vsr_hip_pix.h; libvsr_hip_pix.so is built
// from this source alone): yuv422p, yuv444p, yuv422p10le, yuv444p10le -> the model's float32 RGB, and float32 RGB -> a packed frame.
// The arithmetic is clip_yuv.hip's on the axes that are subsampled (clip_yuv.h holds what the two sources share).
//
//   k_pix_lr       : one thread = one LR pixel, nearest neighbour with ATen's index rule (k_yuv_lr), chroma taken at the source pixel
//                    (4:4:4: the sample; 4:2:2: 2 samples of the pixel's own chroma row per component), matrix, clamp.
//   k_pix_full     : the conversion at full size (hr, and lr when h == H): one thread = 4 consecutive pixels of the flat [F*H*W] index
//                    = 48 output bytes = three 16-byte stores.  F*H*W need not be a multiple of 4 (5 x 7 4:4:4), and with
//                    H*W % 4 == 2 a group straddles two frames (3 x 6 4:2:2): unless WIDE every pixel of a group finds its own frame,
//                    and the ragged last group stores its 1..3 pixels element by element (no 16-byte store passes the end).
//                    WIDE (checked by the entry): 4:2:2 with W % 4 == 0 and an aligned base -- the group lies in one row, its 4 luma
//                    samples are one load and it shares its 3 or 4 chroma columns (element loads: the Cr plane starts at an odd
//                    multiple of H*W/2); 4:4:4 with H*W % 4 == 0 and an aligned base -- every plane of every frame starts on a
//                    multiple of 4 samples, so the group's Y, Cb and Cr are one load each.
//   k_pix_write422 : one thread = 1 row x 2*NC pixels = NC chroma columns of that row.  NC = 4 (W % 8 == 0 and a 16-byte aligned
//                    base, checked by the entry): 6 16-byte loads, luma as 8 samples in one store, each chroma plane 4 samples in one
//                    store; NC = 1: 8-byte loads, element stores.
//   k_pix_write444 : one thread = 4 consecutive pixels of the flat index: three 16-byte loads (element loads in the ragged last
//                    group); WIDE (H*W % 4 == 0 and an aligned base): 4 samples per plane in one store each, else element stores with
//                    every pixel finding its own frame.
// In both write kernels every sample of the frames belongs to exactly one thread, so every byte is written once and nothing else is.
// All are HBM-bound byte passes.  The up-sampling weights are dyadic (1, 1/2, 1/4, 3/4) and the code values below 2^10, so the
// up-sampled chroma is exact in float32 in any order; the matrix is three nested fmas spelled out (a restatement can follow them).
#include "clip_yuv.h"

#include <type_traits>

#include "../../include/vsr_hip_pix.h"

namespace {

template <int FMT>
struct Fmt {
    static constexpr bool k16 = FMT == VSR_PIX_422P10LE || FMT == VSR_PIX_444P10LE;
    static constexpr bool k422 = FMT == VSR_PIX_422P || FMT == VSR_PIX_422P10LE;
    static constexpr float kMax = k16 ? 1023.0f : 255.0f;
    using T = typename std::conditional<k16, unsigned short, unsigned char>::type;
    __device__ static inline float dec(T v) { return k16 ? (float)(v & 0x3FF) : (float)v; }
    __device__ static inline unsigned enc(float v) {   // rint (ties to even), clamp
        v = rintf(v);
        if (!(v >= 0.0f)) v = 0.0f;
        if (v > kMax) v = kMax;
        return (unsigned)v;
    }
    // samples of one chroma plane / of one frame
    __host__ __device__ static inline size_t plane(size_t hw) { return k422 ? hw / 2 : hw; }
    __host__ __device__ static inline size_t frame(size_t hw) { return k422 ? 2 * hw : 3 * hw; }
};

// (Cb', Cr') at luma position (y, x) of the frame at `fr`: the sample (4:4:4) or 2 samples of chroma row y per component (4:2:2)
template <int FMT, int SIT>
__device__ inline void chroma_at(const typename Fmt<FMT>::T* __restrict__ fr, int H, int W, int y, int x, float& cb, float& cr) {
    using P = Fmt<FMT>;
    const size_t hw = (size_t)H * W, d = P::plane(hw);
    if (!P::k422) {
        const size_t i = hw + (size_t)y * W + x;
        cb = P::dec(fr[i]);
        cr = P::dec(fr[i + d]);
        return;
    }
    const int Wc = W >> 1;
    int c0, c1;
    float wx;
    if (SIT == VSR_YUV_SITING_LEFT) cosited(x, Wc, c0, c1, wx);
    else midway(x, Wc, c0, c1, wx);
    const size_t i0 = hw + (size_t)y * Wc + c0, i1 = hw + (size_t)y * Wc + c1;
    const float vx = 1.0f - wx;
    cb = wx * P::dec(fr[i0]) + vx * P::dec(fr[i1]);
    cr = wx * P::dec(fr[i0 + d]) + vx * P::dec(fr[i1 + d]);
}

template <int FMT, int SIT>
__global__ void __launch_bounds__(256)
k_pix_lr(const typename Fmt<FMT>::T* __restrict__ in, float* __restrict__ lr, int H, int W, int h, int w, float sy, float sx, Coef k) {
    using P = Fmt<FMT>;
    const int f = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    int yy = (int)floorf((float)y * sy), xx = (int)floorf((float)x * sx);   // ATen nearest_neighbor_compute_source_index
    yy = yy < H - 1 ? yy : H - 1;
    xx = xx < W - 1 ? xx : W - 1;
    const size_t hw = (size_t)H * W;
    const typename P::T* fr = in + (size_t)f * P::frame(hw);
    float cb, cr, o[3];
    chroma_at<FMT, SIT>(fr, H, W, yy, xx, cb, cr);
    to_rgb(k, P::dec(fr[(size_t)yy * W + xx]), cb, cr, o);
    float* q = lr + (((size_t)f * h + y) * w + x) * 3;
    q[0] = o[0];
    q[1] = o[1];
    q[2] = o[2];
}

// 4 samples at `p` (a multiple of 4 samples from an aligned base) as floats
template <int FMT>
__device__ inline void load4(const typename Fmt<FMT>::T* __restrict__ p, float* v) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    if (P::k16) {
        const ushort4 u = *reinterpret_cast<const ushort4*>(p);
        v[0] = P::dec((T)u.x), v[1] = P::dec((T)u.y), v[2] = P::dec((T)u.z), v[3] = P::dec((T)u.w);
    } else {
        const uchar4 u = *reinterpret_cast<const uchar4*>(p);
        v[0] = P::dec((T)u.x), v[1] = P::dec((T)u.y), v[2] = P::dec((T)u.z), v[3] = P::dec((T)u.w);
    }
}

__device__ inline void store12(float* out, const float* o) {
    float4* q = reinterpret_cast<float4*>(out);
    q[0] = make_float4(o[0], o[1], o[2], o[3]);
    q[1] = make_float4(o[4], o[5], o[6], o[7]);
    q[2] = make_float4(o[8], o[9], o[10], o[11]);
}

template <int FMT, int SIT, bool WIDE>
__global__ void __launch_bounds__(256)
k_pix_full(const typename Fmt<FMT>::T* __restrict__ in, float* __restrict__ out1, float* __restrict__ out2, int H, int W, size_t total,
           Coef k) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= total) return;
    const size_t hw = (size_t)H * W;
    const int n = total - p < 4 ? (int)(total - p) : 4;   // pixels of this group: 4, or 1..3 in the ragged last one
    float o[12];
    if (WIDE) {   // H * W % 4 == 0: n == 4 and the group lies in one frame
        const size_t f = p / hw;
        const unsigned r = (unsigned)(p - f * hw);   // H, W <= 65535: below 2^32
        const T* fr = in + f * P::frame(hw);
        float yc[4], cb[4], cr[4];
        load4<FMT>(fr + r, yc);
        if (!P::k422) {
            load4<FMT>(fr + hw + r, cb);
            load4<FMT>(fr + 2 * hw + r, cr);
        } else {   // W % 4 == 0: x is a multiple of 4 and the group lies in one row
            const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * (unsigned)W);
            const int Wc = W >> 1, k0 = x >> 1;
            // chroma columns k0-1 (CENTER only), k0, k0+1 (< Wc: x + 3 < W), k0+2 of row y
            const int col[4] = {k0 > 0 ? k0 - 1 : 0, k0, k0 + 1, k0 + 2 < Wc ? k0 + 2 : Wc - 1};
            const T* cbrow = fr + hw + (size_t)y * Wc;
            const size_t d = P::plane(hw);
            float vb[4], vr[4];
#pragma unroll
            for (int j = (SIT == VSR_YUV_SITING_LEFT ? 1 : 0); j < 4; ++j) {
                vb[j] = P::dec(cbrow[col[j]]);
                vr[j] = P::dec(cbrow[col[j] + d]);
            }
            if (SIT == VSR_YUV_SITING_LEFT) {
                cb[0] = vb[1], cb[1] = 0.5f * vb[1] + 0.5f * vb[2], cb[2] = vb[2], cb[3] = 0.5f * vb[2] + 0.5f * vb[3];
                cr[0] = vr[1], cr[1] = 0.5f * vr[1] + 0.5f * vr[2], cr[2] = vr[2], cr[3] = 0.5f * vr[2] + 0.5f * vr[3];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // pixel i: even = 1/4 of the column before + 3/4 of its own, odd = 3/4 of its own + 1/4 of the next
                    const int a = (i + 1) >> 1;   // vb index of the first of the two columns: 0, 1, 1, 2
                    const float wx = (i & 1) ? 0.75f : 0.25f;
                    cb[i] = wx * vb[a] + (1.0f - wx) * vb[a + 1];
                    cr[i] = wx * vr[a] + (1.0f - wx) * vr[a + 1];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) to_rgb(k, yc[i], cb[i], cr[i], o + 3 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {   // every pixel finds its own frame: a group may straddle two
                const size_t pi = p + i, f = pi / hw;
                const unsigned ri = (unsigned)(pi - f * hw);
                const T* fr = in + f * P::frame(hw);
                const int y = (int)(ri / (unsigned)W), x = (int)(ri - (unsigned)y * (unsigned)W);
                float cb, cr;
                chroma_at<FMT, SIT>(fr, H, W, y, x, cb, cr);
                to_rgb(k, P::dec(fr[ri]), cb, cr, o + 3 * i);
            } else {
                o[3 * i] = o[3 * i + 1] = o[3 * i + 2] = 0.0f;   // (never stored)
            }
        }
    }
    if (n == 4) {   // 48 bytes at a multiple of 48 from a 16-byte aligned base
        store12(out1 + p * 3, o);
        if (out2) store12(out2 + p * 3, o);
    } else {   // n <= 3: at most 9 floats, none past the end
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (i < 3 * n) {
                out1[p * 3 + i] = o[i];
                if (out2) out2[p * 3 + i] = o[i];
            }
        }
    }
}

template <int FMT, int SIT, int NC>
__global__ void __launch_bounds__(256)
k_pix_write422(const float* __restrict__ rgb, typename Fmt<FMT>::T* __restrict__ out, int H, int W, Coef k) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    constexpr bool WIDE = NC == 4;
    constexpr int NP = 2 * NC;   // pixels of the row
    const int Wc = W >> 1;
    const int cx0 = (blockIdx.x * 256 + threadIdx.x) * NC;
    if (cx0 >= Wc) return;   // (NC == 4: Wc is a multiple of 4, so a thread's columns are all inside)
    const int y = blockIdx.y, f = blockIdx.z;
    const float* row = rgb + (((size_t)f * H + y) * W + 2 * cx0) * 3;
    float a[NP * 3];
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < NP * 3 / 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(row)[i];
            a[4 * i] = v.x, a[4 * i + 1] = v.y, a[4 * i + 2] = v.z, a[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NP * 3 / 2; ++i) {
            const float2 v = reinterpret_cast<const float2*>(row)[i];
            a[2 * i] = v.x, a[2 * i + 1] = v.y;
        }
    }
#pragma unroll
    for (int i = 0; i < NP * 3; ++i) a[i] = clamp255(a[i]);
    float l[3];   // LEFT: the pixel before the thread's first column (the column clamped at 0)
    if (SIT == VSR_YUV_SITING_LEFT) {
        const int back = cx0 > 0 ? 3 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) l[c] = clamp255(*(row - back + c));
    }
    const size_t hw = (size_t)H * W;
    T* fr = out + (size_t)f * P::frame(hw);
    unsigned cy[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) cy[i] = P::enc(dot_row(k, 0, a[3 * i], a[3 * i + 1], a[3 * i + 2]));
    store_run<T, NP, WIDE>(fr + (size_t)y * W + 2 * cx0, cy);
    // chroma from the row's filtered R'G'B'
    unsigned cb[NC], cr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (SIT == VSR_YUV_SITING_LEFT) {
                const float left = j == 0 ? l[c] : a[3 * (2 * j - 1) + c];
                m[c] = ((left + a[3 * (2 * j + 1) + c]) + 2.0f * a[3 * (2 * j) + c]) * 0.25f;
            } else {
                m[c] = (a[3 * (2 * j) + c] + a[3 * (2 * j + 1) + c]) * 0.5f;
            }
        }
        cb[j] = P::enc(dot_row(k, 1, m[0], m[1], m[2]));
        cr[j] = P::enc(dot_row(k, 2, m[0], m[1], m[2]));
    }
    T* q = fr + hw + (size_t)y * Wc + cx0;
    store_run<T, NC, WIDE>(q, cb);
    store_run<T, NC, WIDE>(q + P::plane(hw), cr);
}

template <int FMT, bool WIDE>
__global__ void __launch_bounds__(256)
k_pix_write444(const float* __restrict__ rgb, typename Fmt<FMT>::T* __restrict__ out, size_t hw, size_t total, Coef k) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= total) return;
    const int n = total - p < 4 ? (int)(total - p) : 4;   // pixels of this group: 4, or 1..3 in the ragged last one
    float a[12];
    if (n == 4) {   // 48 bytes at a multiple of 48 from a 16-byte aligned base
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float4 v = reinterpret_cast<const float4*>(rgb + p * 3)[i];
            a[4 * i] = v.x, a[4 * i + 1] = v.y, a[4 * i + 2] = v.z, a[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) a[i] = i < 3 * n ? rgb[p * 3 + i] : 0.0f;
    }
    unsigned c[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float r = clamp255(a[3 * i]), g = clamp255(a[3 * i + 1]), b = clamp255(a[3 * i + 2]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][i] = P::enc(dot_row(k, ch, r, g, b));
    }
    if constexpr (WIDE) {   // H * W % 4 == 0: n == 4, the group lies in one frame and every plane starts on a multiple of 4 samples
        const size_t f = p / hw, r = p - f * hw;
        T* fr = out + f * 3 * hw;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) store_run<T, 4, true>(fr + ch * hw + r, c[ch]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {   // every pixel finds its own frame: a group may straddle two
                const size_t pi = p + i, f = pi / hw, r = pi - f * hw;
                T* fr = out + f * 3 * hw;
                fr[r] = (T)c[0][i];
                fr[hw + r] = (T)c[1][i];
                fr[2 * hw + r] = (T)c[2][i];
            }
        }
    }
}

inline bool is16(int fmt) { return fmt == VSR_PIX_422P10LE || fmt == VSR_PIX_444P10LE; }
inline bool is422(int fmt) { return fmt == VSR_PIX_422P || fmt == VSR_PIX_422P10LE; }

// the checks the two entries share; `what` names the entry in the message
int check_frames(const char* what, const void* frames, int fmt, const float* coef12, int siting, int F, int H, int W) {
    if (!frames || !coef12) return vsr::fail(VSR_E_ARG, "%s: null pointer", what);
    if (fmt < VSR_PIX_422P || fmt > VSR_PIX_444P10LE) return vsr::fail(VSR_E_ARG, "%s: unknown pixel format %d", what, fmt);
    if (siting != VSR_YUV_SITING_LEFT && siting != VSR_YUV_SITING_CENTER) return vsr::fail(VSR_E_ARG, "%s: unknown chroma siting %d", what, siting);
    if (F <= 0 || H <= 0 || W <= 0 || (is422(fmt) && (W & 1)))
        return vsr::fail(VSR_E_ARG, "%s: bad shape (F %d, H %d, W %d: all positive, and 4:2:2 needs an even W)", what, F, H, W);
    if (F > 65535 || H > 65535 || W > 65535) return vsr::fail(VSR_E_ARG, "%s: grid overflow (F %d, H %d, W %d beyond 65535)", what, F, H, W);
    if ((unsigned long long)F * H * W / 1024 >= (1ull << 31))
        return vsr::fail(VSR_E_ARG, "%s: grid overflow (F * H * W = %llu)", what, (unsigned long long)F * H * W);
    if (is16(fmt) && (reinterpret_cast<uintptr_t>(frames) & 1))
        return vsr::fail(VSR_E_ARG, "%s: a 16-bit pixel format at an odd byte address", what);
    return VSR_OK;
}

// one case per (fmt, siting): BODY sees the compile-time FMT and SIT (4:4:4 has one siting: the entries pass LEFT)
#define VSR_PIX_DISPATCH(fmt, siting, BODY)                                                          \
    do {                                                                                             \
        const int code_ = (fmt) * 2 + (siting);                                                      \
        switch (code_) {                                                                             \
            case 0: { constexpr int FMT = 0, SIT = 0; BODY; } break;                                 \
            case 1: { constexpr int FMT = 0, SIT = 1; BODY; } break;                                 \
            case 2: { constexpr int FMT = 1, SIT = 0; BODY; } break;                                 \
            case 4: { constexpr int FMT = 2, SIT = 0; BODY; } break;                                 \
            case 5: { constexpr int FMT = 2, SIT = 1; BODY; } break;                                 \
            default: { constexpr int FMT = 3, SIT = 0; BODY; } break;                                \
        }                                                                                            \
    } while (0)

template <int FMT>
bool aligned4(const void* frames) {   // a run of 4 samples from the base is one access
    return (reinterpret_cast<uintptr_t>(frames) & (4 * sizeof(typename Fmt<FMT>::T) - 1)) == 0;
}

template <int FMT, int SIT>
void launch_full(const void* frames, float* out1, float* out2, int F, int H, int W, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    const size_t hw = (size_t)H * W, total = (size_t)F * hw;
    // 4:2:2: W % 4 == 0 keeps every row and frame start (2 H W samples a frame) on a multiple of 4 samples: the luma load; 4:4:4:
    // H W % 4 == 0 does the same for every plane of every frame (3 H W samples a frame)
    const bool wide = aligned4<FMT>(frames) && (Fmt<FMT>::k422 ? W % 4 == 0 : hw % 4 == 0);
    const dim3 grid(vsr::cdiv((long long)((total + 3) / 4), 256));
    if (wide) hipLaunchKernelGGL((k_pix_full<FMT, SIT, true>), grid, dim3(256), 0, s, (const T*)frames, out1, out2, H, W, total, k);
    else hipLaunchKernelGGL((k_pix_full<FMT, SIT, false>), grid, dim3(256), 0, s, (const T*)frames, out1, out2, H, W, total, k);
}

template <int FMT, int SIT>
void launch_lr(const void* frames, float* lr, int F, int H, int W, int h, int w, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    // scale as ATen forms it when only the output size is given (compute_scales_value): (float)input / output
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;
    hipLaunchKernelGGL((k_pix_lr<FMT, SIT>), dim3(vsr::cdiv(w, 256), h, F), dim3(256), 0, s, (const T*)frames, lr, H, W, h, w, sy, sx, k);
}

template <int FMT, int SIT>
void launch_write(const float* rgb, void* frames_out, int F, int H, int W, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    const size_t hw = (size_t)H * W, total = (size_t)F * hw;
    if constexpr (Fmt<FMT>::k422) {
        // 16-byte loads of rgb (the entry checked its base; a row is W * 12 bytes) and one store per run of samples.  With W % 8 == 0 a
        // frame holds a multiple of 16 samples, its luma plane a multiple of 8 and each chroma row a multiple of 4, so from a 16-byte
        // aligned base each store falls on a multiple of its own width: 8 luma samples = 8 bytes at 8 bit, 16 at 16 bit; 4 chroma
        // samples = 4 or 8 bytes.  (The Cr plane need NOT start on a multiple of 16: H W / 2 = 12 samples at 3 x 8.)
        const bool wide = W % 8 == 0 && (reinterpret_cast<uintptr_t>(frames_out) & 15) == 0;
        const int Wc = W / 2;
        if (wide) hipLaunchKernelGGL((k_pix_write422<FMT, SIT, 4>), dim3(vsr::cdiv(Wc / 4, 256), H, F), dim3(256), 0, s, rgb, (T*)frames_out, H, W, k);
        else hipLaunchKernelGGL((k_pix_write422<FMT, SIT, 1>), dim3(vsr::cdiv(Wc, 256), H, F), dim3(256), 0, s, rgb, (T*)frames_out, H, W, k);
    } else {
        const bool wide = aligned4<FMT>(frames_out) && hw % 4 == 0;
        const dim3 grid(vsr::cdiv((long long)((total + 3) / 4), 256));
        if (wide) hipLaunchKernelGGL((k_pix_write444<FMT, true>), grid, dim3(256), 0, s, rgb, (T*)frames_out, hw, total, k);
        else hipLaunchKernelGGL((k_pix_write444<FMT, false>), grid, dim3(256), 0, s, rgb, (T*)frames_out, hw, total, k);
    }
}

}  // namespace

extern "C" {

int vsr_pix_abi_version(void) { return VSR_PIX_ABI_VERSION; }
const char* vsr_pix_last_error(void) { return vsr::err_buf(); }

int vsr_pix_ingest(const void* frames, int fmt, const float* coef12, int siting, float* lr, float* hr_or_null, int F, int H, int W,
                   int h, int w, vsr_stream_t stream) {
    if (!lr) return vsr::fail(VSR_E_ARG, "pix_ingest: null pointer");
    const int rc0 = check_frames("pix_ingest", frames, fmt, coef12, siting, F, H, W);
    if (rc0) return rc0;
    VSR_REQUIRE(h > 0 && w > 0 && h <= H && w <= W, "pix_ingest: bad shape (lr %d x %d from %d x %d)", h, w, H, W);
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(lr) & 15) == 0 && (reinterpret_cast<uintptr_t>(hr_or_null) & 15) == 0,
                "pix_ingest: the float buffers must be 16-byte aligned");
    const Coef k = read_coef(coef12);
    hipStream_t s = vsr::S(stream);
    if (!is422(fmt)) siting = VSR_YUV_SITING_LEFT;   // (no effect on 4:4:4: one build)
    if (h == H && w == W) {   // the plain conversion: one pass writes both
        VSR_PIX_DISPATCH(fmt, siting, (launch_full<FMT, SIT>(frames, lr, hr_or_null, F, H, W, k, s)));
        return vsr::launched("pix_ingest/full");
    }
    VSR_PIX_DISPATCH(fmt, siting, (launch_lr<FMT, SIT>(frames, lr, F, H, W, h, w, k, s)));
    const int rc = vsr::launched("pix_ingest/lr");
    if (rc || !hr_or_null) return rc;
    VSR_PIX_DISPATCH(fmt, siting, (launch_full<FMT, SIT>(frames, hr_or_null, nullptr, F, H, W, k, s)));
    return vsr::launched("pix_ingest/hr");
}

int vsr_pix_write(const float* rgb, void* frames_out, int fmt, const float* coef12, int siting, int F, int H, int W,
                  vsr_stream_t stream) {
    if (!rgb) return vsr::fail(VSR_E_ARG, "pix_write: null pointer");
    const int rc0 = check_frames("pix_write", frames_out, fmt, coef12, siting, F, H, W);
    if (rc0) return rc0;
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(rgb) & 15) == 0, "pix_write: the float buffer must be 16-byte aligned");
    const Coef k = read_coef(coef12);
    hipStream_t s = vsr::S(stream);
    if (!is422(fmt)) siting = VSR_YUV_SITING_LEFT;   // (no effect on 4:4:4: one build)
    VSR_PIX_DISPATCH(fmt, siting, (launch_write<FMT, SIT>(rgb, frames_out, F, H, W, k, s)));
    return vsr::launched("pix_write");
}

}  // extern "C"
