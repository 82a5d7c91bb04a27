// flow_ops_bwd.hip -- gfx950 kernels for the gradients of FlowNet2's three native operators (include/vsr_hip_grad.h).
//
// The adjoints of flow_ops.hip's k_resample2d, k_channelnorm and k_correlation, built into a library of their own
// (libvsr_hip_grad.so: this file alone).  Resample2d and ChannelNorm are byte movers: one thread per pixel handling every
// channel, consecutive lanes on consecutive x.  The correlation gradients are the arithmetic ones (2 * D^2 * C FLOP per pixel
// each) and are built like the forward: a row segment x a channel chunk per workgroup, operands staged through LDS.
//
// Determinism: everything here is a gather with a fixed summation order, except the image gradient of Resample2d, which
// scatters with float atomic adds (one global_atomic_add_f32 each, no compare-and-swap loop) and so depends on arrival
// order in its last bits.  Sized by atomic bytes: C * 4 adds * 4 B per pixel = 48 B at C = 3, 24 MB for a 512 x 960 frame,
// against a chip-wide atomic rate of about 1.3 TB/s for wave-instructions of 256 contiguous bytes -- tens of microseconds.
// Measured on a pair of such frames: 0.33 TB/s of added bytes on a smooth flow (a wave's 64 adds already fall on several
// rows), 0.12 on white noise of 4 px (a row per lane): 142 / 396 us, small beside a training step (LAB_NOTES.md).
#include "vsr_common.h"

#include "../../include/vsr_hip_grad.h"

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(size_t n) {
    size_t g = (n + kBlock - 1) / kBlock;
    return (unsigned)(g < 2048 ? (g ? g : 1) : 2048);  // cap + grid-stride
}

// ---------------------------------------------------------------------------------------------
// Resample2d.  The forward's coordinates (flow_ops.hip bilerp_setup: float adds, floorf, the four indices clamped
// independently); alpha and beta are exact in float (x - floor(x)).  The clamps come after the float -> int conversion, so
// every index is inside the image whatever the flow holds: the scatter cannot leave d_img.
// ---------------------------------------------------------------------------------------------
template <bool kImg, bool kFlow>
__global__ void __launch_bounds__(kBlock) k_resample2d_bwd(const float* __restrict__ img, const float* __restrict__ flow,
                                                           const float* __restrict__ gout, float* __restrict__ d_img,
                                                           float* __restrict__ d_flow, int C, int H, int W, int bilinear) {
    const int b = blockIdx.y;
    const size_t hw = (size_t)H * W;
    for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < hw; p += (size_t)gridDim.x * kBlock) {
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        const float xf = (float)x + flow[((size_t)b * 2 + 0) * hw + p];
        const float yf = (float)y + flow[((size_t)b * 2 + 1) * hw + p];
        if (bilinear) {
            const float fx = floorf(xf), fy = floorf(yf);
            const float alpha = xf - fx, beta = yf - fy;
            const int xL = max(min((int)fx, W - 1), 0), xR = max(min((int)(fx + 1.0f), W - 1), 0);
            const int yT = max(min((int)fy, H - 1), 0), yB = max(min((int)(fy + 1.0f), H - 1), 0);
            const size_t o00 = (size_t)yT * W + xL, o01 = (size_t)yT * W + xR;
            const size_t o10 = (size_t)yB * W + xL, o11 = (size_t)yB * W + xR;
            const float w00 = (1.0f - alpha) * (1.0f - beta), w01 = alpha * (1.0f - beta);
            const float w10 = (1.0f - alpha) * beta, w11 = alpha * beta;
            float gx = 0.0f, gy = 0.0f;
            for (int c = 0; c < C; ++c) {
                const size_t pl = ((size_t)b * C + c) * hw;
                const float gv = gout[pl + p];
                if (kImg) {
                    atomicAdd(d_img + pl + o00, gv * w00);
                    atomicAdd(d_img + pl + o01, gv * w01);
                    atomicAdd(d_img + pl + o10, gv * w10);
                    atomicAdd(d_img + pl + o11, gv * w11);
                }
                if (kFlow) {
                    const float i00 = img[pl + o00], i01 = img[pl + o01], i10 = img[pl + o10], i11 = img[pl + o11];
                    gx += gv * ((1.0f - beta) * (i01 - i00) + beta * (i11 - i10));
                    gy += gv * ((1.0f - alpha) * (i10 - i00) + alpha * (i11 - i01));
                }
            }
            if (kFlow) {
                d_flow[((size_t)b * 2 + 0) * hw + p] = gx;
                d_flow[((size_t)b * 2 + 1) * hw + p] = gy;
            }
        } else {  // nearest: the forward's one rounded pixel; the output does not depend on the flow
            const int xN = max(min((int)floorf(xf + 0.5f), W - 1), 0);
            const int yN = max(min((int)floorf(yf + 0.5f), H - 1), 0);
            if (kImg)
                for (int c = 0; c < C; ++c) {
                    const size_t pl = ((size_t)b * C + c) * hw;
                    atomicAdd(d_img + pl + (size_t)yN * W + xN, gout[pl + p]);
                }
            if (kFlow) {
                d_flow[((size_t)b * 2 + 0) * hw + p] = 0.0f;
                d_flow[((size_t)b * 2 + 1) * hw + p] = 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ChannelNorm: d_in = gout * in / (out + 1e-9), elementwise.  V pixels per thread: 4 (16-byte accesses; needs H*W % 4 == 0 and
// 16-byte aligned pointers, so that every plane starts aligned) or 1.  (gout * in) * (1 / (out + 1e-9)): at a pixel whose
// channels are all zero the product is 0 and the reciprocal 1e9 -- the gradient is 0.
// ---------------------------------------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));
template <int V>
struct VecOf;
template <>
struct VecOf<1> { typedef float type; };
template <>
struct VecOf<4> { typedef f4 type; };

template <int V>
__global__ void __launch_bounds__(kBlock) k_channelnorm_bwd(const float* __restrict__ in, const float* __restrict__ out,
                                                            const float* __restrict__ gout, float* __restrict__ d_in, int C,
                                                            size_t hw) {
    typedef typename VecOf<V>::type vec;
    const int b = blockIdx.y;
    const size_t n = hw / V;
    const vec* g_v = reinterpret_cast<const vec*>(gout + (size_t)b * hw);
    const vec* o_v = reinterpret_cast<const vec*>(out + (size_t)b * hw);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const vec g = g_v[i];
        const vec r = 1.0f / (o_v[i] + 1e-9f);
        for (int c = 0; c < C; ++c) {
            const size_t pl = ((size_t)b * C + c) * hw;
            reinterpret_cast<vec*>(d_in + pl)[i] = (g * reinterpret_cast<const vec*>(in + pl)[i]) * r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Correlation, kernel_size 1.  One kernel for both gradients (kSecond: d_f2, else d_f1), each a GATHER over the pixels of the
// gradient's own map, so every element is written exactly once (positions that feed no output pixel get 0; no memset, no
// atomics) and the sum runs in one fixed order: tj outer, ti inner.
//   One workgroup = a row segment of kTX pixels (y, x0 .. x0+kTX) of the gradient x a chunk of kCH channels.  Per vertical
// displacement tj it stages through LDS, once, the D gout values of every pixel of the segment ([D][kTX]: the tj-slice of the
// segment's [D*D][kTX] column) and the row window of the OTHER feature map the segment reaches, [kCH][kTX + 2*R*s2] (rows padded
// to NP * 32 columns); both are then reused by all kCH channels.  A thread owns one pixel and kKC channels: per (tj, ti) one
// gout read serves kKC FMAs.  NCHW is read directly (no padded copies).
//   Staging: every thread's global loads of a step (4 * NP of the window, 4 of the gout slice) are issued together
// into registers -- one memory latency per step, not one per element -- and the NEXT step's are issued before the current
// step's arithmetic, so they are in flight behind it (one LDS image, two barriers per step).
//   LDS reads: lanes of a 32-lane half share the channel and take consecutive columns (conflict-free); the gout read is the
// same for the 8 thread rows (broadcast).
//   d_f1 at f1 pixel (y, x):  its output pixel (oy, ox) = ((y, x) - off) / s1 if on the stride1 grid and inside the output;
//                             other = f2 at (y + tj*s2, x + ti*s2).
//   d_f2 at f2 pixel (y, x):  other = f1 at (y1, x1) = (y - tj*s2, x - ti*s2), and (oy, ox) is THAT position's output pixel.
// off = max_displacement - pad_size (f1 coordinate of output pixel 0).
// ---------------------------------------------------------------------------------------------
constexpr int kTX = 32;
constexpr int kCH = 32;
constexpr int kKC = 4;       // kCH = (256 / kTX) thread rows x kKC
constexpr int kMaxNP = 15;   // builds exist for windows of up to kMaxNP * 32 = 480 columns (everything the forward's LDS window admits)
static_assert(kTX == 32 && kCH == (256 / kTX) * kKC, "thread rows x channels per thread");

// index of the output pixel whose f1 coordinate is r + off, or -1 (off the stride1 grid / outside the output)
__device__ __forceinline__ int out_index(int r, int s1, int n) {
    if (r < 0) return -1;
    const int q = r / s1;
    return (q * s1 == r && q < n) ? q : -1;
}

template <bool kSecond, int NP>   // NP: 32-column pieces of a window row, ceil((kTX + 2*R*s2) / 32)
__global__ void __launch_bounds__(256) k_correlation_bwd(const float* __restrict__ other, const float* __restrict__ gout,
                                                         float* __restrict__ d, int C, int H, int W, int OH, int OW, int off,
                                                         int s1, int s2, int R, int nchunk) {
    extern __shared__ float lds[];
    const int D = 2 * R + 1, OC = D * D;
    constexpr int wpad = NP * 32;       // LDS row of the window (>= kTX + 2*R*s2 columns)
    float* g_s = lds;                   // [D][kTX], D <= 32
    float* o_s = lds + D * kTX;         // [kCH][wpad]
    const int b = blockIdx.z / nchunk, c0 = (blockIdx.z % nchunk) * kCH;
    const int y = blockIdx.y, x0 = blockIdx.x * kTX;
    const int px = threadIdx.x % kTX, cg = threadIdx.x / kTX;
    const size_t hw = (size_t)H * W;
    const int xw0 = x0 - R * s2;        // first column of the window
    const int oy_self = out_index(y - off, s1, OH);

    // the steps that add something: the other map's row inside the image and an output row behind it (uniform over the workgroup)
    auto other_row = [&](int tjI) { return kSecond ? y - (tjI - R) * s2 : y + (tjI - R) * s2; };
    auto out_row = [&](int tjI) { return kSecond ? out_index(other_row(tjI) - off, s1, OH) : oy_self; };
    auto next_step = [&](int tjI) {
        for (; tjI < D; ++tjI)
            if (other_row(tjI) >= 0 && other_row(tjI) < H && out_row(tjI) >= 0) break;
        return tjI;
    };

    // This thread's part of a step: window elements (channel cg + 8*jc, column px + 32*jp) and gout elements i = j*256 + tid
    // (D <= 32, the forward's limit: 4 x 256 cover the slice).  Which of them exist does not depend on the step: the loads are
    // unconditional from clamped (always in-bounds) addresses and the zeros are put in when the registers go to LDS -- a
    // select on the loaded value at load time would wait for the load and undo the prefetch.
    float ov[4 * NP], gv4[4];
    unsigned long long omask = 0;
#pragma unroll
    for (int jc = 0; jc < 4; ++jc)
#pragma unroll
        for (int jp = 0; jp < NP; ++jp) {
            const int c = c0 + cg + 8 * jc, xx = xw0 + px + 32 * jp;
            if (c < C && xx >= 0 && xx < W) omask |= 1ull << (jc * NP + jp);
        }
    auto g_ox = [&](int i) {   // output column behind gout element i of a slice, or -1
        const int tiI = i / kTX;
        if (tiI >= D || x0 + px >= W) return -1;
        return out_index((kSecond ? x0 + px - (tiI - R) * s2 : x0 + px) - off, s1, OW);   // the f1 column of this (pixel, ti)
    };
    int gox[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gox[j] = g_ox(j * 256 + threadIdx.x);

    auto load_g = [&](int tjI) {
        const float* slice = gout + (((size_t)b * OC + (size_t)tjI * D) * OH + out_row(tjI)) * OW;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int tiI = min((j * 256 + (int)threadIdx.x) / kTX, D - 1);
            gv4[j] = slice[(size_t)tiI * OH * OW + max(gox[j], 0)];
        }
    };
    auto store_g = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = j * 256 + threadIdx.x;
            if (i < D * kTX) g_s[i] = gox[j] >= 0 ? gv4[j] : 0.0f;
        }
    };
    auto load_o = [&](int tjI) {
        const float* row = other + (size_t)b * C * hw + (size_t)other_row(tjI) * W;
#pragma unroll
        for (int jc = 0; jc < 4; ++jc) {
            const float* crow = row + (size_t)min(c0 + cg + 8 * jc, C - 1) * hw;
#pragma unroll
            for (int jp = 0; jp < NP; ++jp) ov[jc * NP + jp] = crow[min(max(xw0 + px + 32 * jp, 0), W - 1)];
        }
    };
    auto store_o = [&]() {
#pragma unroll
        for (int jc = 0; jc < 4; ++jc)
#pragma unroll
            for (int jp = 0; jp < NP; ++jp)
                o_s[(cg + 8 * jc) * wpad + px + 32 * jp] = ((omask >> (jc * NP + jp)) & 1ull) ? ov[jc * NP + jp] : 0.0f;
    };

    float acc[kKC];
#pragma unroll
    for (int k = 0; k < kKC; ++k) acc[k] = 0.0f;
    int tjI = next_step(0);
    if (tjI < D) {
        load_o(tjI);
        load_g(tjI);
    }
    while (tjI < D) {
        __syncthreads();   // the previous step's reads are done
        store_o();
        store_g();
        __syncthreads();
        const int nxt = next_step(tjI + 1);
        if (nxt < D) {     // in flight behind the arithmetic below
            load_o(nxt);
            load_g(nxt);
        }
        const float* o_t = o_s + cg * kKC * wpad + px;
        for (int tiI = 0; tiI < D; ++tiI) {
            const float gv = g_s[tiI * kTX + px];
            const int col = (kSecond ? D - 1 - tiI : tiI) * s2;
#pragma unroll
            for (int k = 0; k < kKC; ++k) acc[k] += gv * o_t[k * wpad + col];
        }
        tjI = nxt;
    }
    const float inv = 1.0f / (float)C;   // the forward's 1 / (kernel_size^2 * C)
    const int x = x0 + px;
    if (x < W) {
#pragma unroll
        for (int k = 0; k < kKC; ++k) {
            const int c = c0 + cg * kKC + k;
            if (c < C) d[((size_t)b * C + c) * hw + (size_t)y * W + x] = acc[k] * inv;
        }
    }
}

template <bool kSecond, int NP>
int launch_correlation_bwd_np(const float* other, const float* gout, float* d, int B, int C, int H, int W, int OH, int OW, int off,
                              int s1, int s2, int R, hipStream_t st) {
    const int nchunk = (C + kCH - 1) / kCH;
    const size_t lds = sizeof(float) * ((size_t)(2 * R + 1) * kTX + (size_t)kCH * NP * 32);
    hipLaunchKernelGGL((k_correlation_bwd<kSecond, NP>), dim3(vsr::cdiv(W, kTX), H, B * nchunk), dim3(256), lds, st, other, gout,
                       d, C, H, W, OH, OW, off, s1, s2, R, nchunk);
    return vsr::launched(kSecond ? "grad_correlation/d_f2" : "grad_correlation/d_f1");
}

template <bool kSecond>
int launch_correlation_bwd(const float* other, const float* gout, float* d, int B, int C, int H, int W, int OH, int OW, int off,
                           int s1, int s2, int R, hipStream_t st) {
#define VSR_CORR_BWD_NP(n) \
    case n: return launch_correlation_bwd_np<kSecond, n>(other, gout, d, B, C, H, W, OH, OW, off, s1, s2, R, st)
    switch ((kTX + 2 * R * s2 + 31) / 32) {
        VSR_CORR_BWD_NP(1);
        VSR_CORR_BWD_NP(2);
        VSR_CORR_BWD_NP(3);
        VSR_CORR_BWD_NP(4);
        VSR_CORR_BWD_NP(5);
        VSR_CORR_BWD_NP(6);
        VSR_CORR_BWD_NP(7);
        VSR_CORR_BWD_NP(8);
        VSR_CORR_BWD_NP(9);
        VSR_CORR_BWD_NP(10);
        VSR_CORR_BWD_NP(11);
        VSR_CORR_BWD_NP(12);
        VSR_CORR_BWD_NP(13);
        VSR_CORR_BWD_NP(14);
        VSR_CORR_BWD_NP(15);
    }
#undef VSR_CORR_BWD_NP
    return vsr::fail(VSR_E_ARG, "grad_correlation: no build for this window");   // (refused by the entry before)
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int vsr_grad_abi_version(void) { return VSR_GRAD_ABI_VERSION; }
const char* vsr_grad_last_error(void) { return vsr::err_buf(); }

int vsr_grad_resample2d_f32(const float* img, const float* flow, const float* gout, float* d_img, float* d_flow, int B, int C,
                            int H, int W, int kernel_size, int bilinear, vsr_stream_t stream) {
    VSR_REQUIRE(img && flow && gout, "grad_resample2d: null pointer");
    VSR_REQUIRE(d_img || d_flow, "grad_resample2d: null pointer for both gradients (nothing to compute)");
    VSR_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "grad_resample2d: bad shape %dx%dx%dx%d", B, C, H, W);
    VSR_REQUIRE(B <= 65535, "grad_resample2d: batch %d beyond the grid limit", B);
    if (kernel_size != 1) return vsr::fail(VSR_E_UNSUPPORTED, "grad_resample2d: kernel_size %d (the path uses 1)", kernel_size);
    const hipStream_t st = vsr::S(stream);
    if (d_img && hipMemsetAsync(d_img, 0, sizeof(float) * (size_t)B * C * H * W, st) != hipSuccess)
        return vsr::fail(VSR_E_LAUNCH, "grad_resample2d: memset");
    const dim3 grid(grid_for((size_t)H * W), B), block(kBlock);
    if (d_img && d_flow)
        hipLaunchKernelGGL((k_resample2d_bwd<true, true>), grid, block, 0, st, img, flow, gout, d_img, d_flow, C, H, W, bilinear);
    else if (d_img)
        hipLaunchKernelGGL((k_resample2d_bwd<true, false>), grid, block, 0, st, img, flow, gout, d_img, d_flow, C, H, W, bilinear);
    else
        hipLaunchKernelGGL((k_resample2d_bwd<false, true>), grid, block, 0, st, img, flow, gout, d_img, d_flow, C, H, W, bilinear);
    return vsr::launched("grad_resample2d");
}

int vsr_grad_channelnorm_f32(const float* in, const float* out, const float* gout, float* d_in, int B, int C, int H, int W,
                             vsr_stream_t stream) {
    VSR_REQUIRE(in && out && gout && d_in, "grad_channelnorm: null pointer");
    VSR_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "grad_channelnorm: bad shape %dx%dx%dx%d", B, C, H, W);
    VSR_REQUIRE(B <= 65535, "grad_channelnorm: batch %d beyond the grid limit", B);
    const size_t hw = (size_t)H * W;
    if (hw % 4 == 0 && aligned16(in) && aligned16(out) && aligned16(gout) && aligned16(d_in))
        hipLaunchKernelGGL(k_channelnorm_bwd<4>, dim3(grid_for(hw / 4), B), dim3(kBlock), 0, vsr::S(stream), in, out, gout, d_in,
                           C, hw);
    else
        hipLaunchKernelGGL(k_channelnorm_bwd<1>, dim3(grid_for(hw), B), dim3(kBlock), 0, vsr::S(stream), in, out, gout, d_in, C,
                           hw);
    return vsr::launched("grad_channelnorm");
}

int vsr_grad_correlation_f32(const float* f1, const float* f2, const float* gout, float* d_f1, float* d_f2, int B, int C, int H,
                             int W, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                             vsr_stream_t stream) {
    VSR_REQUIRE(f1 && f2 && gout, "grad_correlation: null pointer");
    VSR_REQUIRE(d_f1 || d_f2, "grad_correlation: null pointer for both gradients (nothing to compute)");
    VSR_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "grad_correlation: bad shape %dx%dx%dx%d", B, C, H, W);
    if (kernel_size != 1)
        return vsr::fail(VSR_E_UNSUPPORTED, "grad_correlation: kernel_size %d (FlowNetC uses 1)", kernel_size);
    VSR_REQUIRE(stride1 > 0 && stride2 > 0 && pad_size >= 0 && max_displacement >= 0, "grad_correlation: bad strides / pad");
    // the forward's output geometry (vsr_correlation_out_shape; correlation_cuda.cc:26-34 with kernel_size 1)
    const int OH = (H + 2 * pad_size - 2 * max_displacement + stride1 - 1) / stride1;
    const int OW = (W + 2 * pad_size - 2 * max_displacement + stride1 - 1) / stride1;
    VSR_REQUIRE(OH > 0 && OW > 0, "grad_correlation: empty output");
    const int R = max_displacement / stride2, D = 2 * R + 1;
    const long long win = kTX + 2ll * R * stride2;   // columns of the other map a 32-pixel segment reaches
    // the forward's limits (vsr_correlation_f32: 32 * D pairs over 4 x 256 threads, its LDS window) hold here too
    VSR_REQUIRE(D <= 32, "grad_correlation: displacement range %d too large", D);
    const long long np = (win + 31) / 32;
    VSR_REQUIRE(np <= kMaxNP, "grad_correlation: window too wide for LDS (%lld columns)", win);
    const int nchunk = (C + kCH - 1) / kCH;
    VSR_REQUIRE((long long)B * nchunk <= 65535 && H <= 65535, "grad_correlation: grid overflow (B * ceil(C/%d) = %lld, H = %d)",
                kCH, (long long)B * nchunk, H);
    const int off = max_displacement - pad_size;
    const hipStream_t st = vsr::S(stream);
    if (d_f1) {
        const int rc = launch_correlation_bwd<false>(f2, gout, d_f1, B, C, H, W, OH, OW, off, stride1, stride2, R, st);
        if (rc) return rc;
    }
    if (d_f2) return launch_correlation_bwd<true>(f1, gout, d_f2, B, C, H, W, OH, OW, off, stride1, stride2, R, st);
    return VSR_OK;
}

}  // extern "C"
