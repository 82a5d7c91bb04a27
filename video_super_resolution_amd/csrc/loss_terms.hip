// loss_terms.hip -- the pixel terms of the training loss on the device (include/vsr_hip_loss.h; libvsr_hip_loss.so is built from this
// source alone): object masking, the six image SSEs, the eight total-variation sums and the NHWC-4 half VGG inputs in one pass.
//
//   k_terms  : one workgroup (3 waves) = a strip of SF = 768 floats of a row (256 pixels, 192 groups of 16 bytes) by SR = 32 rows.
//              Thread i owns floats 4 i .. 4 i + 3 of the strip in all four frames and marches down the rows:
//                load    : O0, O1, O2, T and the mask of its four elements (WIDE: one aligned 16-byte load per frame and one 4-byte
//                          load of the mask; otherwise element loads): a frame is read once
//                own     : the masked values, the six SSE terms, the masked frames' store, and the h terms of TV against the
//                          previous row, which the thread still holds in registers; the row below the segment is read for these
//                          alone (O0, O1 and the mask)
//                stage   : O0, O1, mO0, mO1 as floats and all eight frames as halves into LDS; three threads add the three floats
//                          right of the strip (the w neighbours of its last pixel)
//                w + out : the w terms of TV from the element three floats to the right, read from LDS; the NHWC-4 half rows are
//                          regrouped by pixel from LDS (WIDE: two pixels = 16 bytes per store; otherwise 2-byte stores)
//              two barriers per row.  At the end a butterfly inside each wave, the three waves in order, 14 doubles to the workspace.
//   k_finish : one workgroup of 256 threads: thread t adds the partials t, t + 256, ... in that order, a fixed-order tree, then the
//              14 sums and the 6 x 2 terms.
// Nothing here is atomic and no order depends on timing: every number is the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): differences, squares and the
// quotients of the terms round operation by operation as the header writes them.
#include "vsr_common.h"

#include "../../include/vsr_hip_loss.h"

#pragma clang fp contract(off)

namespace {

constexpr int SF = VSR_LOSS_STRIP_FLOATS, SR = VSR_LOSS_SEGMENT_ROWS, FT = VSR_LOSS_FINISH_THREADS, NS = VSR_LOSS_NSUMS;
constexpr int NT = SF / 4;    // threads of a workgroup: one 16-byte group of the strip each
constexpr int SP = SF / 3;    // pixels of a strip
constexpr int NW = NT / 64;   // waves
static_assert(SF % 12 == 0 && NT % 64 == 0 && SP % 2 == 0, "a strip is a whole number of pixel pairs, 16-byte groups and waves");

typedef unsigned short us4 __attribute__((ext_vector_type(4)));
typedef unsigned short us8 __attribute__((ext_vector_type(8)));

// (float)((int)v & 255) with the saturating convert spelled out (v >= 2^31 -> 2^31 - 1, v <= -2^31 -> -2^31, NaN -> 0)
__device__ inline float low8(float v) {
    const int i = v >= 2147483648.0f ? 0x7fffffff : (v <= -2147483648.0f ? (int)0x80000000 : (v == v ? (int)v : 0));
    return (float)(i & 255);
}

__device__ inline unsigned short half_bits(float v) {
    const _Float16 h = (_Float16)v;   // round to nearest even, overflow to infinity
    return __builtin_bit_cast(unsigned short, h);
}

__device__ inline double sq_diff(float a, float b) {
    const double d = (double)a - (double)b;
    return d * d;
}

template <bool WIDE>
__global__ void __launch_bounds__(NT)
k_terms(const float* __restrict__ outputs, const float* __restrict__ target, const unsigned char* __restrict__ mask, int H, int W,
        float* __restrict__ masked, unsigned short* __restrict__ nhwc4, double* __restrict__ ws) {
    __shared__ __align__(16) float nbr[4][SF + 4];          // O0, O1, mO0, mO1 of the row: the strip + 3 floats to its right
    __shared__ __align__(16) unsigned short hv[8][SF];      // the eight frames of nhwc4 as halves, in element order
    __shared__ double red[NS][NW];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int RW = 3 * W;                                    // floats of a row
    const size_t N = (size_t)H * RW;                         // elements of a frame
    const int c0 = blockIdx.x * SF, c = c0 + 4 * tid;        // first column (in floats) of the strip, of this thread
    const int nv = c < RW ? min(4, RW - c) : 0;              // elements of this thread inside the row (WIDE: 4 or 0)
    const int y0 = blockIdx.y * SR;
    const int nown = min(SR, H - y0);                        // rows the workgroup owns
    const int nin = nown + (y0 + nown < H ? 1 : 0);          // + the row below, for the h terms of its last row
    const int px0 = blockIdx.x * SP, npx = min(SP, W - px0); // pixels of the strip
    const float* __restrict__ O0 = outputs;
    const float* __restrict__ O1 = outputs + N;
    const float* __restrict__ O2 = outputs + 2 * N;

    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    float p_o0[4] = {0, 0, 0, 0}, p_o1[4] = {0, 0, 0, 0}, p_m0[4] = {0, 0, 0, 0}, p_m1[4] = {0, 0, 0, 0};

    for (int r = 0; r < nin; ++r) {
        const int y = y0 + r;
        const bool own = r < nown;                           // (the same for every thread of the workgroup)
        const size_t e = (size_t)y * RW + c;
        float o0[4] = {0, 0, 0, 0}, o1[4] = {0, 0, 0, 0}, o2[4] = {0, 0, 0, 0}, tg[4] = {0, 0, 0, 0};
        unsigned char mk[4] = {1, 1, 1, 1};
        // ---- load
        if (WIDE) {
            if (nv) {
                const float4 a = *reinterpret_cast<const float4*>(O0 + e), b = *reinterpret_cast<const float4*>(O1 + e);
                const uchar4 m = *reinterpret_cast<const uchar4*>(mask + e);
                o0[0] = a.x, o0[1] = a.y, o0[2] = a.z, o0[3] = a.w;
                o1[0] = b.x, o1[1] = b.y, o1[2] = b.z, o1[3] = b.w;
                mk[0] = m.x, mk[1] = m.y, mk[2] = m.z, mk[3] = m.w;
                if (own) {
                    const float4 d = *reinterpret_cast<const float4*>(O2 + e), t = *reinterpret_cast<const float4*>(target + e);
                    o2[0] = d.x, o2[1] = d.y, o2[2] = d.z, o2[3] = d.w;
                    tg[0] = t.x, tg[1] = t.y, tg[2] = t.z, tg[3] = t.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    o0[k] = O0[e + k];
                    o1[k] = O1[e + k];
                    mk[k] = mask[e + k];
                    if (own) {
                        o2[k] = O2[e + k];
                        tg[k] = target[e + k];
                    }
                }
        }
        float m0[4], m1[4], m2[4], mt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m0[k] = mk[k] ? 0.0f : low8(o0[k]);
            m1[k] = mk[k] ? 0.0f : low8(o1[k]);
            m2[k] = mk[k] ? 0.0f : low8(o2[k]);
            mt[k] = mk[k] ? 0.0f : low8(tg[k]);
        }
        // ---- h terms of TV: this row against the previous one
        if (r > 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    acc[6] += sq_diff(o0[k], p_o0[k]);
                    acc[8] += sq_diff(o1[k], p_o1[k]);
                    acc[10] += sq_diff(m0[k], p_m0[k]);
                    acc[12] += sq_diff(m1[k], p_m1[k]);
                }
        }
        if (own) {
            // ---- SSE
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    acc[0] += sq_diff(o0[k], tg[k]);
                    acc[1] += sq_diff(m1[k], mt[k]);
                    acc[2] += sq_diff(o0[k], o1[k]);
                    acc[3] += sq_diff(o1[k], o2[k]);
                    acc[4] += sq_diff(m0[k], m1[k]);
                    acc[5] += sq_diff(m1[k], m2[k]);
                }
            // ---- the masked frames
            if (masked) {
                if (WIDE) {
                    if (nv) {
                        *reinterpret_cast<float4*>(masked + e) = make_float4(m0[0], m0[1], m0[2], m0[3]);
                        *reinterpret_cast<float4*>(masked + N + e) = make_float4(m1[0], m1[1], m1[2], m1[3]);
                        *reinterpret_cast<float4*>(masked + 2 * N + e) = make_float4(m2[0], m2[1], m2[2], m2[3]);
                        *reinterpret_cast<float4*>(masked + 3 * N + e) = make_float4(mt[0], mt[1], mt[2], mt[3]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < nv) {
                            masked[e + k] = m0[k];
                            masked[N + e + k] = m1[k];
                            masked[2 * N + e + k] = m2[k];
                            masked[3 * N + e + k] = mt[k];
                        }
                }
            }
            // ---- stage the row (elements outside the row are staged as 0 and never used)
            *reinterpret_cast<float4*>(&nbr[0][4 * tid]) = make_float4(o0[0], o0[1], o0[2], o0[3]);
            *reinterpret_cast<float4*>(&nbr[1][4 * tid]) = make_float4(o1[0], o1[1], o1[2], o1[3]);
            *reinterpret_cast<float4*>(&nbr[2][4 * tid]) = make_float4(m0[0], m0[1], m0[2], m0[3]);
            *reinterpret_cast<float4*>(&nbr[3][4 * tid]) = make_float4(m1[0], m1[1], m1[2], m1[3]);
            if (tid < 3) {                                   // the three floats right of the strip
                const int ch = c0 + SF + tid;
                float h0 = 0.0f, h1 = 0.0f, hm0 = 0.0f, hm1 = 0.0f;
                if (ch < RW) {
                    const size_t eh = (size_t)y * RW + ch;
                    h0 = O0[eh];
                    h1 = O1[eh];
                    const bool mh = mask[eh] != 0;
                    hm0 = mh ? 0.0f : low8(h0);
                    hm1 = mh ? 0.0f : low8(h1);
                }
                nbr[0][SF + tid] = h0;
                nbr[1][SF + tid] = h1;
                nbr[2][SF + tid] = hm0;
                nbr[3][SF + tid] = hm1;
            }
            if (nhwc4) {
                const float* fr[8] = {o0, o1, o2, tg, m0, m1, m2, mt};
#pragma unroll
                for (int f = 0; f < 8; ++f) {
                    us4 h;
#pragma unroll
                    for (int k = 0; k < 4; ++k) h[k] = half_bits(fr[f][k]);
                    *reinterpret_cast<us4*>(&hv[f][4 * tid]) = h;
                }
            }
        }
        __syncthreads();
        if (own) {
            // ---- w terms of TV: the element three floats to the right, while it is in the row
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k + 3 < RW) {
                    const int j = 4 * tid + k + 3;
                    acc[7] += sq_diff(nbr[0][j], o0[k]);
                    acc[9] += sq_diff(nbr[1][j], o1[k]);
                    acc[11] += sq_diff(nbr[2][j], m0[k]);
                    acc[13] += sq_diff(nbr[3][j], m1[k]);
                }
            // ---- the NHWC-4 half rows, by pixel
            if (nhwc4) {
                const size_t HW = (size_t)H * W;
                const size_t row = (size_t)y * W + px0;
                if (WIDE) {                                  // (W % 4 == 0: npx is even, a pair of pixels starts on 16 bytes)
                    for (int idx = tid; idx < 8 * (SP / 2); idx += NT) {
                        const int f = idx / (SP / 2), q = idx % (SP / 2);
                        if (2 * q < npx) {
                            const unsigned short* s = &hv[f][6 * q];
                            us8 o;
                            o[0] = s[0], o[1] = s[1], o[2] = s[2], o[3] = 0, o[4] = s[3], o[5] = s[4], o[6] = s[5], o[7] = 0;
                            *reinterpret_cast<us8*>(nhwc4 + ((size_t)f * HW + row + 2 * q) * 4) = o;
                        }
                    }
                } else {
                    for (int idx = tid; idx < 8 * SP; idx += NT) {
                        const int f = idx / SP, p = idx % SP;
                        if (p < npx) {
                            const unsigned short* s = &hv[f][3 * p];
                            unsigned short* d = nhwc4 + ((size_t)f * HW + row + p) * 4;
                            d[0] = s[0], d[1] = s[1], d[2] = s[2], d[3] = 0;
                        }
                    }
                }
            }
        }
        __syncthreads();   // the staged row is free for the next one
#pragma unroll
        for (int k = 0; k < 4; ++k) p_o0[k] = o0[k], p_o1[k] = o1[k], p_m0[k] = m0[k], p_m1[k] = m1[k];
    }

    // ---- the workgroup's 14 partials: a butterfly inside each wave (every lane ends with the same sum), then the waves in order
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double v = acc[k];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) red[k][wv] = v;
    }
    __syncthreads();
    if (tid < NS) {
        double v = red[tid][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[tid][w];
        ws[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NS + tid] = v;
    }
}

__global__ void __launch_bounds__(FT)
k_finish(const double* __restrict__ ws, unsigned nwg, int H, int W, double* __restrict__ sums, float* __restrict__ terms) {
    __shared__ double red[NS][FT];
    const int tid = threadIdx.x;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    for (unsigned i = tid; i < nwg; i += FT) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += ws[(size_t)i * NS + k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][tid] = s[k];
    for (int st = FT / 2; st > 0; st >>= 1) {
        __syncthreads();
        if (tid < st) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][tid] += red[k][tid + st];
        }
    }
    __syncthreads();
    if (tid < NS) sums[tid] = red[tid][0];
    if (tid < 6) {
        // the frame whose TV the call takes: O0, mO1, O0, O1, mO0, mO1 -> its h / w slots in `sums`
        const int tv_of[6] = {6, 12, 6, 8, 10, 12};
        const double n = 3.0 * (double)H * (double)W;
        const double count_h = 3.0 * (double)(H - 1) * (double)W, count_w = 3.0 * (double)H * (double)(W - 1);
        const double h = red[tv_of[tid]][0], w = red[tv_of[tid] + 1][0];
        terms[2 * tid] = (float)(red[tid][0] / n);
        terms[2 * tid + 1] = (float)(2.0 * (h / count_h + w / count_w));
    }
}

struct Geometry {
    unsigned strips, segs;
};

// the checks vsr_loss_ws_bytes and vsr_loss_pixel_terms share; `g` only when the result is VSR_OK
int check_shape(int H, int W, Geometry* g) {
    VSR_REQUIRE(H >= 2 && W >= 2, "loss_pixel_terms: H and W must be at least 2 (TV divides by H - 1 and W - 1), got %d x %d", H, W);
    VSR_REQUIRE(H <= VSR_LOSS_MAX_DIM && W <= VSR_LOSS_MAX_DIM, "loss_pixel_terms: grid overflow (H %d, W %d beyond %d)", H, W,
                VSR_LOSS_MAX_DIM);
    g->strips = vsr::cdiv(3ll * W, SF);
    g->segs = vsr::cdiv(H, SR);
    return VSR_OK;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

int vsr_loss_abi_version(void) { return VSR_LOSS_ABI_VERSION; }
const char* vsr_loss_last_error(void) { return vsr::err_buf(); }

size_t vsr_loss_ws_bytes(int H, int W) {
    Geometry g;
    if (check_shape(H, W, &g) != VSR_OK) return 0;
    return (size_t)g.strips * g.segs * NS * sizeof(double);
}

int vsr_loss_pixel_terms(const float* outputs, const float* target, const unsigned char* mask, int H, int W, float* masked, void* nhwc4,
                         double* sums, float* terms, void* ws, vsr_stream_t stream) {
    VSR_REQUIRE(outputs && target && mask && sums && terms && ws, "loss_pixel_terms: null pointer");
    Geometry g;
    const int rc0 = check_shape(H, W, &g);
    if (rc0) return rc0;
    auto P = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    VSR_REQUIRE(((P(outputs) | P(target) | P(masked) | P(terms)) & 3) == 0, "loss_pixel_terms: the float buffers must be 4-byte aligned");
    VSR_REQUIRE((P(nhwc4) & 1) == 0, "loss_pixel_terms: nhwc4 must be 2-byte aligned");
    VSR_REQUIRE(((P(sums) | P(ws)) & 7) == 0, "loss_pixel_terms: sums and the workspace must be 8-byte aligned");
    const size_t N = (size_t)H * W * 3;
    const size_t ws_bytes = (size_t)g.strips * g.segs * NS * sizeof(double);
    const struct { const void* p; size_t n; const char* name; } ins[3] = {{outputs, 3 * N * 4, "outputs"}, {target, N * 4, "target"},
                                                                          {mask, N, "mask"}},
        outs[5] = {{masked, 4 * N * 4, "masked"}, {nhwc4, (size_t)8 * H * W * 4 * 2, "nhwc4"}, {sums, NS * sizeof(double), "sums"},
                   {terms, 12 * sizeof(float), "terms"}, {ws, ws_bytes, "ws"}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            VSR_REQUIRE(!overlap(o.p, o.n, i.p, i.n), "loss_pixel_terms: the output %s overlaps the input %s", o.name, i.name);
    // 16-byte loads and stores: every frame base aligned and a row pitch of a whole number of 16-byte groups
    const bool wide = ((P(outputs) | P(target) | P(masked) | P(nhwc4)) & 15) == 0 && (P(mask) & 3) == 0 && W % 4 == 0;
    const dim3 grid(g.strips, g.segs), block(NT);
    hipStream_t s = vsr::S(stream);
    double* wsd = static_cast<double*>(ws);
    unsigned short* nh = static_cast<unsigned short*>(nhwc4);
    if (wide) hipLaunchKernelGGL(k_terms<true>, grid, block, 0, s, outputs, target, mask, H, W, masked, nh, wsd);
    else hipLaunchKernelGGL(k_terms<false>, grid, block, 0, s, outputs, target, mask, H, W, masked, nh, wsd);
    const int rc = vsr::launched("loss_pixel_terms/tiles");
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(FT), 0, s, (const double*)wsd, g.strips * g.segs, H, W, sums, terms);
    return vsr::launched("loss_pixel_terms/finish");
}

}  // extern "C"
