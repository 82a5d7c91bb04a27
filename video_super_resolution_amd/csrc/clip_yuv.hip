// clip_yuv.hip -- Y'CbCr 4:2:0 frames either side of the path (include/vsr_hip_yuv.h; libvsr_hip_yuv.so is built from this source
// alone): what decoders emit (yuv420p, nv12, yuv420p10le, p010le) -> the model's float32 RGB, and float32 RGB -> a packed 4:2:0 frame.
//
//   k_yuv_lr    : the YUV counterpart of k_ingest_lr (clip_io.hip): one thread = one LR pixel, nearest neighbour with ATen's index
//                 rule, chroma up-sampled at the source pixel (4 samples per component), matrix, clamp.
//   k_yuv_full  : the conversion at full size (hr, and lr when h == H): one thread = 4 consecutive pixels of the flat [F*H*W] index
//                 = 48 output bytes = three 16-byte stores (F*H*W is a multiple of 4 and the group never leaves its frame).  WIDE
//                 (W % 4 == 0 and an aligned base, checked by the entry): the 4 luma samples are one load and the group shares its
//                 vertically interpolated chroma columns; otherwise every pixel fetches its own samples element by element.
//   k_yuv_write : one thread = 2 rows x 2*NC pixels = NC chroma columns of one chroma row.  NC = 4 (W % 8 == 0 and 16-byte
//                 aligned frames, checked by the entry): 6 16-byte loads per row, luma stored as 8 samples per row in one store, the
//                 planar chroma as 4 samples per store; NC = 1: 8-byte loads, element stores.  Every sample of the frame belongs to
//                 exactly one thread, so every byte is written once and nothing else is.
// All three are HBM-bound byte passes.  The up-sampling weights are dyadic (1, 1/2, 1/4, 3/4) and the code values below 2^10, so the
// up-sampled chroma is exact in float32 in any order; the matrix is three nested fmas spelled out (a restatement can follow them).
#include "clip_yuv.h"   // Coef, midway, cosited, to_rgb, clamp255, dot_row, store_run, read_coef: shared with clip_pix.hip

#include <type_traits>

#include "../../include/vsr_hip_yuv.h"

namespace {

template <int FMT>
struct Fmt {
    static constexpr bool k16 = FMT == VSR_YUV_420P10LE || FMT == VSR_YUV_P010LE;
    static constexpr bool kSemi = FMT == VSR_YUV_NV12 || FMT == VSR_YUV_P010LE;   // one plane of interleaved (Cb, Cr)
    static constexpr float kMax = k16 ? 1023.0f : 255.0f;
    using T = typename std::conditional<k16, unsigned short, unsigned char>::type;
    __device__ static inline float dec(T v) {
        if (FMT == VSR_YUV_420P10LE) return (float)(v & 0x3FF);
        if (FMT == VSR_YUV_P010LE) return (float)(v >> 6);
        return (float)v;
    }
    __device__ static inline unsigned enc(float v) {   // rint (ties to even), clamp, position in the word
        v = rintf(v);
        if (!(v >= 0.0f)) v = 0.0f;
        if (v > kMax) v = kMax;
        const unsigned c = (unsigned)v;
        return FMT == VSR_YUV_P010LE ? c << 6 : c;
    }
    // sample index of chroma (cy, cx) inside a frame: Cb; Cr is kCr further
    __device__ static inline size_t cidx(int H, int W, int cy, int cx) {
        return (size_t)H * W + (kSemi ? ((size_t)cy * (W >> 1) + cx) * 2 : (size_t)cy * (W >> 1) + cx);
    }
    __device__ static inline size_t cr_step(int H, int W) { return kSemi ? 1 : (size_t)(H >> 1) * (W >> 1); }
};

// the up-sampled (Cb', Cr') at luma position (y, x) of the frame at `fr`: 4 samples per component
template <int FMT, int SIT>
__device__ inline void chroma_up(const typename Fmt<FMT>::T* __restrict__ fr, int H, int W, int y, int x, float& cb, float& cr) {
    using P = Fmt<FMT>;
    int r0, r1, c0, c1;
    float wy, wx;
    midway(y, H >> 1, r0, r1, wy);
    if (SIT == VSR_YUV_SITING_LEFT) cosited(x, W >> 1, c0, c1, wx);
    else midway(x, W >> 1, c0, c1, wx);
    const size_t i00 = P::cidx(H, W, r0, c0), i01 = P::cidx(H, W, r0, c1), i10 = P::cidx(H, W, r1, c0), i11 = P::cidx(H, W, r1, c1);
    const size_t d = P::cr_step(H, W);
    const float vy = 1.0f - wy, vx = 1.0f - wx;
    cb = wy * (wx * P::dec(fr[i00]) + vx * P::dec(fr[i01])) + vy * (wx * P::dec(fr[i10]) + vx * P::dec(fr[i11]));
    cr = wy * (wx * P::dec(fr[i00 + d]) + vx * P::dec(fr[i01 + d])) + vy * (wx * P::dec(fr[i10 + d]) + vx * P::dec(fr[i11 + d]));
}

template <int FMT, int SIT>
__global__ void __launch_bounds__(256)
k_yuv_lr(const typename Fmt<FMT>::T* __restrict__ in, float* __restrict__ lr, int H, int W, int h, int w, float sy, float sx, Coef k) {
    using P = Fmt<FMT>;
    const int f = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    int yy = (int)floorf((float)y * sy), xx = (int)floorf((float)x * sx);   // ATen nearest_neighbor_compute_source_index
    yy = yy < H - 1 ? yy : H - 1;
    xx = xx < W - 1 ? xx : W - 1;
    const size_t hw = (size_t)H * W;
    const typename P::T* fr = in + (size_t)f * (hw + hw / 2);
    float cb, cr, o[3];
    chroma_up<FMT, SIT>(fr, H, W, yy, xx, cb, cr);
    to_rgb(k, P::dec(fr[(size_t)yy * W + xx]), cb, cr, o);
    float* q = lr + (((size_t)f * h + y) * w + x) * 3;
    q[0] = o[0];
    q[1] = o[1];
    q[2] = o[2];
}

template <int FMT, int SIT, bool WIDE>
__global__ void __launch_bounds__(256)
k_yuv_full(const typename Fmt<FMT>::T* __restrict__ in, float* __restrict__ out1, float* __restrict__ out2, int H, int W, size_t ngroups,
           Coef k) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const size_t p = g * 4, hw = (size_t)H * W;
    const size_t f = p / hw;
    const unsigned r = (unsigned)(p - f * hw);   // H, W <= 65535: below 2^32; hw is a multiple of 4, so r + 3 stays in the frame
    const T* fr = in + f * (hw + hw / 2);
    float o[12];
    if (WIDE) {   // W % 4 == 0: x is a multiple of 4 and the group lies in one row
        const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * (unsigned)W);
        float yc[4];
        if (P::k16) {
            const ushort4 v = *reinterpret_cast<const ushort4*>(fr + (size_t)y * W + x);
            yc[0] = P::dec((T)v.x), yc[1] = P::dec((T)v.y), yc[2] = P::dec((T)v.z), yc[3] = P::dec((T)v.w);
        } else {
            const uchar4 v = *reinterpret_cast<const uchar4*>(fr + (size_t)y * W + x);
            yc[0] = P::dec((T)v.x), yc[1] = P::dec((T)v.y), yc[2] = P::dec((T)v.z), yc[3] = P::dec((T)v.w);
        }
        const int Wc = W >> 1, k0 = x >> 1;
        int r0, r1;
        float wy;
        midway(y, H >> 1, r0, r1, wy);
        const float vy = 1.0f - wy;
        // chroma columns k0-1 (CENTER only), k0, k0+1 (< Wc: x + 3 < W), k0+2, interpolated between the two chroma rows
        const int col[4] = {k0 > 0 ? k0 - 1 : 0, k0, k0 + 1, k0 + 2 < Wc ? k0 + 2 : Wc - 1};
        const size_t d = P::cr_step(H, W);
        float vb[4], vr[4];
#pragma unroll
        for (int j = (SIT == VSR_YUV_SITING_LEFT ? 1 : 0); j < 4; ++j) {
            const size_t i0 = P::cidx(H, W, r0, col[j]), i1 = P::cidx(H, W, r1, col[j]);
            vb[j] = wy * P::dec(fr[i0]) + vy * P::dec(fr[i1]);
            vr[j] = wy * P::dec(fr[i0 + d]) + vy * P::dec(fr[i1 + d]);
        }
        float cb[4], cr[4];
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
#pragma unroll
        for (int i = 0; i < 4; ++i) to_rgb(k, yc[i], cb[i], cr[i], o + 3 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned ri = r + i;
            const int y = (int)(ri / (unsigned)W), x = (int)(ri - (unsigned)y * (unsigned)W);
            float cb, cr;
            chroma_up<FMT, SIT>(fr, H, W, y, x, cb, cr);
            to_rgb(k, P::dec(fr[ri]), cb, cr, o + 3 * i);
        }
    }
    float4* q = reinterpret_cast<float4*>(out1 + p * 3);
    q[0] = make_float4(o[0], o[1], o[2], o[3]);
    q[1] = make_float4(o[4], o[5], o[6], o[7]);
    q[2] = make_float4(o[8], o[9], o[10], o[11]);
    if (out2) {
        q = reinterpret_cast<float4*>(out2 + p * 3);
        q[0] = make_float4(o[0], o[1], o[2], o[3]);
        q[1] = make_float4(o[4], o[5], o[6], o[7]);
        q[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
}

template <int FMT, int SIT, int NC>
__global__ void __launch_bounds__(256)
k_yuv_write(const float* __restrict__ rgb, typename Fmt<FMT>::T* __restrict__ out, int H, int W, Coef k) {
    using P = Fmt<FMT>;
    using T = typename P::T;
    constexpr bool WIDE = NC == 4;
    constexpr int NP = 2 * NC;   // pixels per row
    const int Wc = W >> 1;
    const int cx0 = (blockIdx.x * 256 + threadIdx.x) * NC;
    if (cx0 >= Wc) return;   // (NC == 4: Wc is a multiple of 4, so a thread's columns are all inside)
    const int cy = blockIdx.y, f = blockIdx.z;
    const float* row = rgb + (((size_t)f * H + 2 * cy) * W + 2 * cx0) * 3;
    float a[2][NP * 3];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const float* p = row + (size_t)rr * W * 3;
        if constexpr (WIDE) {
#pragma unroll
            for (int i = 0; i < NP * 3 / 4; ++i) {
                const float4 v = reinterpret_cast<const float4*>(p)[i];
                a[rr][4 * i] = v.x, a[rr][4 * i + 1] = v.y, a[rr][4 * i + 2] = v.z, a[rr][4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NP * 3 / 2; ++i) {
                const float2 v = reinterpret_cast<const float2*>(p)[i];
                a[rr][2 * i] = v.x, a[rr][2 * i + 1] = v.y;
            }
        }
#pragma unroll
        for (int i = 0; i < NP * 3; ++i) a[rr][i] = clamp255(a[rr][i]);
    }
    float l[2][3];   // LEFT: the pixel before the thread's first column (the column clamped at 0)
    if (SIT == VSR_YUV_SITING_LEFT) {
        const int back = cx0 > 0 ? 3 : 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int c = 0; c < 3; ++c) l[rr][c] = clamp255(*(row + (size_t)rr * W * 3 - back + c));
    }
    const size_t hw = (size_t)H * W;
    T* fr = out + (size_t)f * (hw + hw / 2);
    // luma
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        unsigned c[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) c[i] = P::enc(dot_row(k, 0, a[rr][3 * i], a[rr][3 * i + 1], a[rr][3 * i + 2]));
        store_run<T, NP, WIDE>(fr + (size_t)(2 * cy + rr) * W + 2 * cx0, c);
    }
    // chroma from the filtered R'G'B'
    unsigned cb[NC], cr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (SIT == VSR_YUV_SITING_LEFT) {
                float hrow[2];
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const float left = j == 0 ? l[rr][c] : a[rr][3 * (2 * j - 1) + c];
                    hrow[rr] = ((left + a[rr][3 * (2 * j + 1) + c]) + 2.0f * a[rr][3 * (2 * j) + c]) * 0.25f;
                }
                m[c] = (hrow[0] + hrow[1]) * 0.5f;
            } else {
                m[c] = ((a[0][3 * (2 * j) + c] + a[0][3 * (2 * j + 1) + c]) + (a[1][3 * (2 * j) + c] + a[1][3 * (2 * j + 1) + c])) * 0.25f;
            }
        }
        cb[j] = P::enc(dot_row(k, 1, m[0], m[1], m[2]));
        cr[j] = P::enc(dot_row(k, 2, m[0], m[1], m[2]));
    }
    if (P::kSemi) {
        unsigned c[2 * NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) c[2 * j] = cb[j], c[2 * j + 1] = cr[j];
        store_run<T, 2 * NC, WIDE>(fr + P::cidx(H, W, cy, cx0), c);
    } else {
        store_run<T, NC, WIDE>(fr + P::cidx(H, W, cy, cx0), cb);
        store_run<T, NC, WIDE>(fr + P::cidx(H, W, cy, cx0) + P::cr_step(H, W), cr);
    }
}

inline bool is16(int fmt) { return fmt == VSR_YUV_420P10LE || fmt == VSR_YUV_P010LE; }

// the checks the two entries share; `what` names the entry in the message
int check_frames(const char* what, const void* frames, int fmt, const float* coef12, int siting, int F, int H, int W) {
    if (!frames || !coef12) return vsr::fail(VSR_E_ARG, "%s: null pointer", what);
    if (fmt < VSR_YUV_420P || fmt > VSR_YUV_P010LE) return vsr::fail(VSR_E_ARG, "%s: unknown pixel format %d", what, fmt);
    if (siting != VSR_YUV_SITING_LEFT && siting != VSR_YUV_SITING_CENTER) return vsr::fail(VSR_E_ARG, "%s: unknown chroma siting %d", what, siting);
    if (F <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1))
        return vsr::fail(VSR_E_ARG, "%s: bad shape (F %d, H %d, W %d: 4:2:0 needs positive even H and W)", what, F, H, W);
    if (F > 65535 || H > 65535 || W > 65535) return vsr::fail(VSR_E_ARG, "%s: grid overflow (F %d, H %d, W %d beyond 65535)", what, F, H, W);
    if (is16(fmt) && (reinterpret_cast<uintptr_t>(frames) & 1))
        return vsr::fail(VSR_E_ARG, "%s: a 16-bit pixel format at an odd byte address", what);
    return VSR_OK;
}

// one case per (fmt, siting): BODY sees the compile-time FMT and SIT
#define VSR_YUV_DISPATCH(fmt, siting, BODY)                                                          \
    do {                                                                                             \
        const int code_ = (fmt) * 2 + (siting);                                                      \
        switch (code_) {                                                                             \
            case 0: { constexpr int FMT = 0, SIT = 0; BODY; } break;                                 \
            case 1: { constexpr int FMT = 0, SIT = 1; BODY; } break;                                 \
            case 2: { constexpr int FMT = 1, SIT = 0; BODY; } break;                                 \
            case 3: { constexpr int FMT = 1, SIT = 1; BODY; } break;                                 \
            case 4: { constexpr int FMT = 2, SIT = 0; BODY; } break;                                 \
            case 5: { constexpr int FMT = 2, SIT = 1; BODY; } break;                                 \
            case 6: { constexpr int FMT = 3, SIT = 0; BODY; } break;                                 \
            default: { constexpr int FMT = 3, SIT = 1; BODY; } break;                                \
        }                                                                                            \
    } while (0)

template <int FMT, int SIT>
void launch_full(const void* frames, float* out1, float* out2, int F, int H, int W, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    const size_t ngroups = (size_t)F * H * W / 4;
    // one load of 4 luma samples: the row starts and the frame starts keep the base's alignment when W % 4 == 0
    const bool wide = W % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & (4 * sizeof(T) - 1)) == 0;
    const dim3 grid(vsr::cdiv((long long)ngroups, 256));
    if (wide) hipLaunchKernelGGL((k_yuv_full<FMT, SIT, true>), grid, dim3(256), 0, s, (const T*)frames, out1, out2, H, W, ngroups, k);
    else hipLaunchKernelGGL((k_yuv_full<FMT, SIT, false>), grid, dim3(256), 0, s, (const T*)frames, out1, out2, H, W, ngroups, k);
}

template <int FMT, int SIT>
void launch_lr(const void* frames, float* lr, int F, int H, int W, int h, int w, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    // scale as ATen forms it when only the output size is given (compute_scales_value): (float)input / output
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;
    hipLaunchKernelGGL((k_yuv_lr<FMT, SIT>), dim3(vsr::cdiv(w, 256), h, F), dim3(256), 0, s, (const T*)frames, lr, H, W, h, w, sy, sx, k);
}

template <int FMT, int SIT>
void launch_write(const float* rgb, void* frames_out, int F, int H, int W, const Coef& k, hipStream_t s) {
    using T = typename Fmt<FMT>::T;
    // 16-byte loads of rgb (the entry checked its base; a row is W * 12 bytes) and one store per run of samples.  With W % 8 == 0 a
    // frame holds a multiple of 8 luma samples and every plane a multiple of 4, so from a 16-byte aligned base each store falls on a
    // multiple of its own width: 8 luma samples or 4 (Cb, Cr) pairs = 8 bytes at 8 bit, 16 at 16 bit; 4 planar chroma samples = 4 or 8
    // bytes.  (Frames and planes need NOT start on a multiple of 16: 2 frames of 6 x 8 yuv420p are 72 bytes each.)
    const bool wide = W % 8 == 0 && (reinterpret_cast<uintptr_t>(frames_out) & 15) == 0;
    const int Wc = W / 2;
    if (wide) hipLaunchKernelGGL((k_yuv_write<FMT, SIT, 4>), dim3(vsr::cdiv(Wc / 4, 256), H / 2, F), dim3(256), 0, s, rgb, (T*)frames_out, H, W, k);
    else hipLaunchKernelGGL((k_yuv_write<FMT, SIT, 1>), dim3(vsr::cdiv(Wc, 256), H / 2, F), dim3(256), 0, s, rgb, (T*)frames_out, H, W, k);
}

}  // namespace

extern "C" {

int vsr_yuv_abi_version(void) { return VSR_YUV_ABI_VERSION; }
const char* vsr_yuv_last_error(void) { return vsr::err_buf(); }

int vsr_yuv_ingest(const void* frames, int fmt, const float* coef12, int siting, float* lr, float* hr_or_null, int F, int H, int W,
                   int h, int w, vsr_stream_t stream) {
    if (!lr) return vsr::fail(VSR_E_ARG, "yuv_ingest: null pointer");
    const int rc0 = check_frames("yuv_ingest", frames, fmt, coef12, siting, F, H, W);
    if (rc0) return rc0;
    VSR_REQUIRE(h > 0 && w > 0 && h <= H && w <= W, "yuv_ingest: bad shape (lr %d x %d from %d x %d)", h, w, H, W);
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(lr) & 15) == 0 && (reinterpret_cast<uintptr_t>(hr_or_null) & 15) == 0,
                "yuv_ingest: the float buffers must be 16-byte aligned");
    VSR_REQUIRE((unsigned long long)F * H * W / 1024 < (1ull << 31), "yuv_ingest: grid overflow (F * H * W = %llu)",
                (unsigned long long)F * H * W);
    const Coef k = read_coef(coef12);
    hipStream_t s = vsr::S(stream);
    if (h == H && w == W) {   // the plain conversion: one pass writes both
        VSR_YUV_DISPATCH(fmt, siting, (launch_full<FMT, SIT>(frames, lr, hr_or_null, F, H, W, k, s)));
        return vsr::launched("yuv_ingest/full");
    }
    VSR_YUV_DISPATCH(fmt, siting, (launch_lr<FMT, SIT>(frames, lr, F, H, W, h, w, k, s)));
    const int rc = vsr::launched("yuv_ingest/lr");
    if (rc || !hr_or_null) return rc;
    VSR_YUV_DISPATCH(fmt, siting, (launch_full<FMT, SIT>(frames, hr_or_null, nullptr, F, H, W, k, s)));
    return vsr::launched("yuv_ingest/hr");
}

int vsr_yuv_write(const float* rgb, void* frames_out, int fmt, const float* coef12, int siting, int F, int H, int W,
                  vsr_stream_t stream) {
    if (!rgb) return vsr::fail(VSR_E_ARG, "yuv_write: null pointer");
    const int rc0 = check_frames("yuv_write", frames_out, fmt, coef12, siting, F, H, W);
    if (rc0) return rc0;
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(rgb) & 15) == 0, "yuv_write: the float buffer must be 16-byte aligned");
    const Coef k = read_coef(coef12);
    hipStream_t s = vsr::S(stream);
    VSR_YUV_DISPATCH(fmt, siting, (launch_write<FMT, SIT>(rgb, frames_out, F, H, W, k, s)));
    return vsr::launched("yuv_write");
}

}  // extern "C"
