// conv_glue.hip -- the NHWC fp16 glue kernels of the guidance trunks, none of them a convolution: 2x2 pooling, the NCHW fp32 -> NHWC
// fp16 entry conversion, nearest-resize + add over channel segments (the hourglass), the folded OSVOS head and the FlowNetC cost volume
// on MFMA, each with its entry point.
#include "conv_common.h"

namespace {

using vsrc::h8;
using vsrc::h4;
using vsrc::f4;

}  // namespace

// ---- NHWC fp16 glue of the hourglass (pytorch_DIW_scratch.py: MaxPool2d / AvgPool2d 2x2, UpsamplingNearest2d(2),
//      coolAddTensors = nearest-resize + add): 16 bytes (8 channels) per thread, channel-slice aware on the input side.
typedef _Float16 h8v __attribute__((ext_vector_type(8)));

// mode 0: 2x2 max pool, 1: 2x2 average pool (both floor: out H/2 x W/2), 2: 2x2 max pool with ceil_mode (out ceil(H/2) x
// ceil(W/2); the last window of an odd side holds one row / column).  in [N,H,W,in_ld] slice [in_coff, +C) -> out [N,Ho,Wo,C]
__global__ void __launch_bounds__(256) k_pool2(const _Float16* __restrict__ in, int in_ld, int in_coff, _Float16* __restrict__ out,
                                               int N, int H, int W, int C, int mode) {
    // blockIdx.y = output row (n * Ho + oy), blockIdx.x walks (ox, 8-channel piece): 32-bit index math only
    const int Ho = mode == 2 ? (H + 1) >> 1 : H >> 1, Wo = mode == 2 ? (W + 1) >> 1 : W >> 1;
    const unsigned c8n = (unsigned)C >> 3;
    const unsigned q = blockIdx.x * 256 + threadIdx.x;
    if (q >= (unsigned)Wo * c8n) return;
    const unsigned ox = q / c8n, c8 = q - ox * c8n;
    const unsigned row = blockIdx.y, n = row / (unsigned)Ho, oy = row - n * (unsigned)Ho;
    const int dy = 2 * (int)oy + 1 < H ? 1 : 0, dx = 2 * (int)ox + 1 < W ? 1 : 0;   // (ceil mode: a clamped window re-reads its own row / column)
    const _Float16* p00 = in + (((size_t)n * H + 2 * oy) * W + 2 * ox) * in_ld + in_coff + 8 * c8;
    const h8v a = *reinterpret_cast<const h8v*>(p00), b = *reinterpret_cast<const h8v*>(p00 + (size_t)dx * in_ld);
    const h8v c = *reinterpret_cast<const h8v*>(p00 + (size_t)dy * W * in_ld), d = *reinterpret_cast<const h8v*>(p00 + ((size_t)dy * W + dx) * in_ld);
    h8v o;
    if (mode != 1) {
        o = __builtin_elementwise_max(__builtin_elementwise_max(a, b), __builtin_elementwise_max(c, d));
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)(((float)a[e] + (float)b[e] + (float)c[e] + (float)d[e]) * 0.25f);
    }
    *reinterpret_cast<h8v*>(out + ((size_t)row * Wo + ox) * C + 8 * c8) = o;
}

// [N,C,H,W] fp32 -> [N,H,W,cp] fp16 with the channels >= C written as zeros (round to nearest even, like Tensor.half()):
// the entry conversion of every trunk input in one pass instead of a zero fill plus a strided copy.  Thread = (pixel,
// 4-channel piece): plane reads are coalesced along x, a pixel's pieces are written by adjacent lanes.
__global__ void __launch_bounds__(256) k_nchw_to_nhwc_h(const float* __restrict__ in, _Float16* __restrict__ out, int N, int C, int HW, int cp) {
    const int c4n = cp >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * HW * c4n) return;
    const int c4 = (int)(idx % c4n);
    const long long px = idx / c4n;          // n * HW + p
    const int n = (int)(px / HW);
    const int pp = (int)(px - (long long)n * HW);
    h4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * c4 + j;
        v[j] = c < C ? (_Float16)in[((size_t)n * C + c) * HW + pp] : (_Float16)0.0f;
    }
    *reinterpret_cast<h4*>(out + (size_t)px * cp + 4 * c4) = v;
}

// out[n,y,x,:] = a[n, y*Ha/H, x*Wa/W, slice a] (nearest, as F.interpolate(size)) + b[n,y,x, slice b]; b == null: resize only.

// The same pass with either operand given as up to four channel SEGMENTS of equal width (separate tensors / slices): the 16-channel
// branches of an inception block write dense [N,H,W,16] maps instead of 32-byte slices of a 512-byte pixel row (partial-line
// writes: 3x3 64 -> 16 at 4 x 540 x 960 168 -> 118 us, 64 -> 1 139 -> 99, tools/thin_out_ab.py) and meet again here, where the
// block's 64-channel result is read for the level's sum.
// (ATen nearest: src = min(floor(dst * (in / out)), in - 1) with a float scale; up2: `a` stands for UpsamplingNearest2d(2)(a), never
//  materialised -- the resize indexes the doubled map and halves the index; b_up2: `b` likewise, of exactly the output's size.
//  blockIdx.y = image row, blockIdx.x walks (x, 8-channel piece) of that row: 32-bit index math only.)
struct SegOp {
    const _Float16* ptr[4];
    int ld[4], coff[4];
    int seg_c;     // channels per segment (a multiple of 8); one segment: = C
};
__global__ void __launch_bounds__(256) k_resize_add_segs(const SegOp a, int Ha, int Wa, const SegOp b, int has_b, _Float16* __restrict__ out, int N, int H,
                                                         int W, int C, int up2, int b_up2) {
    const unsigned c8n = (unsigned)C >> 3;
    const unsigned q = blockIdx.x * 256 + threadIdx.x;
    if (q >= (unsigned)W * c8n) return;
    const unsigned x = q / c8n, c8 = q - x * c8n;
    const unsigned row = blockIdx.y, n = row / (unsigned)H, y = row - n * (unsigned)H;
    const int Hs = Ha << up2, Ws = Wa << up2;
    const int ya = min((int)floorf((float)y * ((float)Hs / (float)H)), Hs - 1) >> up2;
    const int xa = min((int)floorf((float)x * ((float)Ws / (float)W)), Ws - 1) >> up2;
    const int ch = 8 * (int)c8;
    const int sa = ch / a.seg_c, ca = ch - sa * a.seg_c;
    const _Float16* ap = sa == 0 ? a.ptr[0] : sa == 1 ? a.ptr[1] : sa == 2 ? a.ptr[2] : a.ptr[3];
    const int ald = sa == 0 ? a.ld[0] : sa == 1 ? a.ld[1] : sa == 2 ? a.ld[2] : a.ld[3];
    const int aco = sa == 0 ? a.coff[0] : sa == 1 ? a.coff[1] : sa == 2 ? a.coff[2] : a.coff[3];
    h8v v = *reinterpret_cast<const h8v*>(ap + (((size_t)n * Ha + ya) * Wa + xa) * ald + aco + ca);
    if (has_b) {
        const int sb = ch / b.seg_c, cb = ch - sb * b.seg_c;
        const _Float16* bp = sb == 0 ? b.ptr[0] : sb == 1 ? b.ptr[1] : sb == 2 ? b.ptr[2] : b.ptr[3];
        const int bld = sb == 0 ? b.ld[0] : sb == 1 ? b.ld[1] : sb == 2 ? b.ld[2] : b.ld[3];
        const int bco = sb == 0 ? b.coff[0] : sb == 1 ? b.coff[1] : sb == 2 ? b.coff[2] : b.coff[3];
        v += *reinterpret_cast<const h8v*>(bp + (((size_t)n * (H >> b_up2) + (y >> b_up2)) * (W >> b_up2) + (x >> b_up2)) * bld + bco + cb);
    }
    *reinterpret_cast<h8v*>(out + ((size_t)row * W + x) * C + ch) = v;
}

// ---- OSVOS head (reference networks/vgg_osvos.py: side_prep -> upscale ConvTranspose2d(16,16,k=2s,stride=s) -> centre
//      crop -> cat -> fuse 1x1 (64 -> 1)).  Nothing non-linear sits between the transposed convolutions and the fuse,
//      so the fuse row is folded into each branch's kernel on the host (weff[b][ky][kx][ci] = sum_co fuse[16b+co] *
//      up_b[ci][co][ky][kx]) and one pass writes the logit: per output pixel 4 branches x 2x2 source pixels x 16
//      channels, fp32 accumulate.  Replaces 4 transposed convolutions on 16-channel full-resolution maps, 4 crops, a
//      concat and a convolution.
struct OsvosP {
    const _Float16* side[4];   // [N, hs, ws, ld] fp16, channels 0..15 live
    const _Float16* weff[4];   // [2s][2s][16] fp16
    int hs[4], ws[4], stride[4], oy[4], ox[4];   // crop offsets: output (y,x) = upsampled (y + oy, x + ox)
    int ld;
    float bias;
    float* out;                // [N, h, w] fp32
    int N, h, w, nb;
};
__global__ void __launch_bounds__(256) k_osvos_fuse(const OsvosP p) {
    const long long total = (long long)p.N * p.h * p.w;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % p.w);
    const int y = (int)((i / p.w) % p.h);
    const int n = (int)(i / ((long long)p.w * p.h));
    float acc = p.bias;
    for (int b = 0; b < p.nb; ++b) {
        const int s = p.stride[b], Y = y + p.oy[b], X = x + p.ox[b];
        const int iy1 = Y / s, ix1 = X / s;          // source pixel reached with tap (Y - iy1 s, X - ix1 s) in [0, s)
        const int ky1 = Y - iy1 * s, kx1 = X - ix1 * s;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int iy = iy1 - dy, ky = ky1 + dy * s;
            if (iy < 0 || iy >= p.hs[b]) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = ix1 - dx, kx = kx1 + dx * s;
                if (ix < 0 || ix >= p.ws[b]) continue;
                const h8* sp = reinterpret_cast<const h8*>(p.side[b] + (((size_t)n * p.hs[b] + iy) * p.ws[b] + ix) * p.ld);
                const h8* wp = reinterpret_cast<const h8*>(p.weff[b] + ((size_t)ky * 2 * s + kx) * 16);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const h8 a = sp[q], wv = wp[q];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc += (float)a[e] * (float)wv[e];
                }
            }
        }
    }
    p.out[i] = acc;
}

// ---- FlowNetC cost volume on MFMA, NHWC fp16 in, straight into the concat buffer (reference FlowNetC.py: Correlation(pad 20,
//      kernel 1, max_disp 20, stride1 1, stride2 2) + LeakyReLU(0.1); correlation_cuda_kernel.cu:74-147).
//      out[b][y][x][coff + (tj*21 + ti)] = lrelu( 1/C * sum_c a[b][y][x][c] * bb[b][y + 2(tj-10)][x + 2(ti-10)][c] ).
//      Workgroup = 32 pixels of one row; wave w takes the vertical displacements tj = w, w+4, ...  For one tj the full
//      product G = A^T B of the 32 pixels against the 72-column window of row y2 is 80 MFMAs (M = pixels, N = window
//      columns, K = C = 256) -- 3.4x more products than the band the volume keeps, but ~10 us of MFMA time for the whole
//      map against 350 us of LDS-bound scalar FMAs in k_correlation; the band (column - pixel even, 0..40) is picked out
//      of the accumulator tiles into an LDS image [32][441] and written as contiguous 882-byte pixel vectors.
constexpr int CORR_D = 21, CORR_OC = CORR_D * CORR_D;
__global__ void __launch_bounds__(256) k_corr_mfma(const _Float16* __restrict__ a, const _Float16* __restrict__ bb,
                                                   _Float16* __restrict__ out, int out_ld, int out_coff, int H, int W, int C) {
    __shared__ _Float16 stage[32 * CORR_OC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * 32, y = blockIdx.y, b = blockIdx.z;
    const int nks = C >> 5;   // 8 for C = 256
    const size_t img = (size_t)b * H * W;
    h8 Af[2][8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int px = x0 + 16 * mt + l15;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            h8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.0f;
            if (px < W && ks < nks) v = *reinterpret_cast<const h8*>(a + (img + (size_t)y * W + px) * C + 32 * ks + 8 * g);
            Af[mt][ks] = v;
        }
    }
    const float inv = 1.0f / (float)C;
    for (int tj = wv; tj < CORR_D; tj += 4) {
        const int y2 = y + 2 * (tj - 10);
        f4 acc[2][5];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (y2 >= 0 && y2 < H) {   // wave-uniform; a row outside the image contributes zeros (the padding)
#pragma unroll
            for (int nt = 0; nt < 5; ++nt) {
                const int col = x0 - 20 + 16 * nt + l15;
                const bool ok = col >= 0 && col < W;
                const _Float16* src = bb + (img + (size_t)y2 * W + (ok ? col : 0)) * C + 8 * g;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    h8 v;
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.0f;
                    if (ok && ks < nks) v = *reinterpret_cast<const h8*>(src + 32 * ks);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Af[mt][ks], v, acc[mt][nt], 0, 0, 0);
                }
            }
        }
        // band: window column cl = 16 nt + l15, pixel pl = 16 mt + 4 g + r; cl - pl = 2 ti
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 5; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pl = 16 * mt + 4 * g + r, d = 16 * nt + l15 - pl;
                    if (d >= 0 && d <= 40 && (d & 1) == 0) {
                        float v = acc[mt][nt][r] * inv;
                        v = v >= 0.0f ? v : 0.1f * v;
                        stage[pl * CORR_OC + tj * CORR_D + (d >> 1)] = (_Float16)v;
                    }
                }
    }
    __syncthreads();
    for (int idx = tid; idx < 32 * CORR_OC; idx += 256) {
        const int pl = idx / CORR_OC, tc = idx - pl * CORR_OC;
        if (x0 + pl < W) out[(img + (size_t)y * W + x0 + pl) * out_ld + out_coff + tc] = stage[idx];
    }
}

extern "C" {

int vsr_pool2x2_nhwc_f16(const void* in, int in_ld, int in_coff, void* out, int N, int H, int W, int C, int mode,
                         vsr_stream_t stream) {
    VSR_REQUIRE(in && out, "pool2x2: null pointer");
    VSR_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0 && (C & 7) == 0 && (in_ld & 7) == 0 && (in_coff & 7) == 0 && in_coff + C <= in_ld &&
                    (mode >= 0 && mode <= 2), "pool2x2: bad arguments");
    const int Ho = mode == 2 ? (H + 1) >> 1 : H >> 1, Wo = mode == 2 ? (W + 1) >> 1 : W >> 1;
    VSR_REQUIRE((long long)N * Ho <= 65535 && (long long)Wo * (C >> 3) < (1ll << 31), "pool2x2: more than 65535 output rows");
    hipLaunchKernelGGL(k_pool2, dim3(vsr::cdiv((long long)Wo * (C >> 3), 256), (unsigned)(N * Ho)), dim3(256), 0, vsr::S(stream),
                       (const _Float16*)in, in_ld, in_coff, (_Float16*)out, N, H, W, C, mode);
    return vsr::launched("pool2x2");
}

int vsr_nchw_f32_to_nhwc_f16(const float* in, void* out, int N, int C, int H, int W, int cp, vsr_stream_t stream) {
    VSR_REQUIRE(in && out, "nchw_to_nhwc: null pointer");
    VSR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && cp >= C && (cp & 3) == 0, "nchw_to_nhwc: bad shape");
    const long long total = (long long)N * H * W * (cp >> 2);
    hipLaunchKernelGGL(k_nchw_to_nhwc_h, dim3(vsr::cdiv(total, 256)), dim3(256), 0, vsr::S(stream), in, (_Float16*)out, N, C, H * W, cp);
    return vsr::launched("nchw_f32_to_nhwc_f16");
}

int vsr_resize_add_segs_nhwc_f16(const void* const* a_ptrs, const int* a_lds, const int* a_coffs, int a_nseg, int Ha, int Wa, int up2,
                                 const void* const* b_ptrs, const int* b_lds, const int* b_coffs, int b_nseg, int b_up2, void* out, int N, int H,
                                 int W, int C, vsr_stream_t stream) {
    VSR_REQUIRE(a_ptrs && a_lds && a_coffs && out && a_nseg >= 1 && a_nseg <= 4 && b_nseg >= 0 && b_nseg <= 4, "resize_add_segs: bad segment lists");
    VSR_REQUIRE(b_nseg == 0 || (b_ptrs && b_lds && b_coffs), "resize_add_segs: addend segments");
    VSR_REQUIRE((up2 == 0 || up2 == 1) && (b_up2 == 0 || (b_up2 == 1 && b_nseg > 0 && (H & 1) == 0 && (W & 1) == 0)),
                "resize_add_segs: up2 flags (an upsampled addend needs an even output size)");
    VSR_REQUIRE(N > 0 && H > 0 && W > 0 && Ha > 0 && Wa > 0 && C > 0 && (C & 7) == 0 && C % a_nseg == 0 && ((C / a_nseg) & 7) == 0 &&
                    (b_nseg == 0 || (C % b_nseg == 0 && ((C / b_nseg) & 7) == 0)), "resize_add_segs: channels per segment must be a multiple of 8");
    VSR_REQUIRE((long long)N * H <= 65535 && (long long)W * (C >> 3) < (1ll << 31), "resize_add_segs: more than 65535 image rows");
    SegOp a, b;
    for (int i = 0; i < 4; ++i) { a.ptr[i] = b.ptr[i] = nullptr; a.ld[i] = b.ld[i] = 8; a.coff[i] = b.coff[i] = 0; }
    a.seg_c = C / a_nseg;
    b.seg_c = b_nseg ? C / b_nseg : C;
    for (int i = 0; i < a_nseg; ++i) {
        VSR_REQUIRE(a_ptrs[i] && (a_lds[i] & 7) == 0 && (a_coffs[i] & 7) == 0 && a_coffs[i] + a.seg_c <= a_lds[i], "resize_add_segs: segment %d of a", i);
        a.ptr[i] = (const _Float16*)a_ptrs[i]; a.ld[i] = a_lds[i]; a.coff[i] = a_coffs[i];
    }
    for (int i = 0; i < b_nseg; ++i) {
        VSR_REQUIRE(b_ptrs[i] && (b_lds[i] & 7) == 0 && (b_coffs[i] & 7) == 0 && b_coffs[i] + b.seg_c <= b_lds[i], "resize_add_segs: segment %d of b", i);
        b.ptr[i] = (const _Float16*)b_ptrs[i]; b.ld[i] = b_lds[i]; b.coff[i] = b_coffs[i];
    }
    hipLaunchKernelGGL(k_resize_add_segs, dim3(vsr::cdiv((long long)W * (C >> 3), 256), (unsigned)(N * H)), dim3(256), 0, vsr::S(stream), a, Ha, Wa, b,
                       b_nseg > 0 ? 1 : 0, (_Float16*)out, N, H, W, C, up2, b_up2);
    return vsr::launched("resize_add_segs");
}

int vsr_osvos_fuse_f16(const void* const* side, const int* hs, const int* ws, int ld, const void* const* weff, const int* strides,
                       int nbranch, float bias, float* out, int N, int h, int w, vsr_stream_t stream) {
    VSR_REQUIRE(side && hs && ws && weff && strides && out, "osvos_fuse: null pointer");
    VSR_REQUIRE(nbranch >= 1 && nbranch <= 4 && N > 0 && h > 0 && w > 0 && ld >= 16 && (ld & 7) == 0, "osvos_fuse: bad arguments");
    OsvosP p;
    for (int b = 0; b < 4; ++b) {
        p.side[b] = nullptr; p.weff[b] = nullptr; p.hs[b] = p.ws[b] = p.stride[b] = 1; p.oy[b] = p.ox[b] = 0;
        if (b >= nbranch) continue;
        VSR_REQUIRE(side[b] && weff[b] && strides[b] >= 1 && hs[b] > 0 && ws[b] > 0, "osvos_fuse: branch %d", b);
        const int uh = (hs[b] + 1) * strides[b], uw = (ws[b] + 1) * strides[b];   // (hs - 1) s + 2 s
        VSR_REQUIRE(uh >= h && uw >= w, "osvos_fuse: branch %d upsamples to %dx%d < %dx%d", b, uh, uw, h, w);
        p.side[b] = (const _Float16*)side[b]; p.weff[b] = (const _Float16*)weff[b];
        p.hs[b] = hs[b]; p.ws[b] = ws[b]; p.stride[b] = strides[b];
        p.oy[b] = (uh - h) / 2; p.ox[b] = (uw - w) / 2;   // centre crop (vgg_osvos.py center_crop)
    }
    p.ld = ld; p.bias = bias; p.out = out; p.N = N; p.h = h; p.w = w; p.nb = nbranch;
    hipLaunchKernelGGL(k_osvos_fuse, dim3(vsr::cdiv((long long)N * h * w, 256)), dim3(256), 0, vsr::S(stream), p);
    return vsr::launched("osvos_fuse");
}

int vsr_flownetc_corr_nhwc_f16(const void* feat_a, const void* feat_b, void* out, int out_ld, int out_coff, int B, int H, int W, int C,
                               vsr_stream_t stream) {
    VSR_REQUIRE(feat_a && feat_b && out, "flownetc_corr: null pointer");
    VSR_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && (C & 31) == 0 && C <= 256, "flownetc_corr: C must be a multiple of 32 up to 256");
    VSR_REQUIRE(out_coff >= 0 && out_coff + CORR_OC <= out_ld && B <= 65535 && H <= 65535, "flownetc_corr: output slice / grid");
    hipLaunchKernelGGL(k_corr_mfma, dim3(vsr::cdiv(W, 32), H, B), dim3(256), 0, vsr::S(stream), (const _Float16*)feat_a,
                       (const _Float16*)feat_b, (_Float16*)out, out_ld, out_coff, H, W, C);
    return vsr::launched("flownetc_corr");
}

}  // extern "C"
