// frame_warp_error.hip -- the temporal warping error of consecutive HR frames on the device (include/vsr_hip_warp.h; libvsr_hip_warp.so
// is built from this source alone): per frame pair the float64 sums behind E_warp.
//
//   k_warp   : one workgroup (4 waves) = one tile of TW = 64 columns x TH = 16 rows of the scored region of one pair; lane l of wave v
//              takes column l and the rows v, v + 4, v + 8, v + 12 of the tile, one pixel at a time: the forward flow at the pixel and
//              at its right and lower neighbour (coalesced along x), then, only where the sample lies in the crop, the 2 x 2 gathers of
//              the backward flow and of frame b around it and the pixel of frame a.  Neighbouring lanes sample neighbouring places, so the
//              gathers are served by L1 / L2; nothing is staged in LDS.  Every index the gathers use has passed the in-frame test of the
//              header's step 2 (0 <= xa <= xb <= w - 1, rows alike), whatever the flow holds (NaN and infinities fail that test).
//              At the end a fixed-order tree over the 256 threads and one pair of doubles {sse, n_valid} into the workspace.
//   k_finish : one workgroup of FT = 256 threads per pair: thread t adds the partials t, t + 256, ... in that order, then the same tree;
//              thread 0 writes the pair's four numbers.
// Nothing here is atomic and no order depends on timing or on P: a pair's numbers are the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): every product and sum of the
// header's steps rounds once, as a float64 restatement in numpy does.
#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_warp.h"

#pragma clang fp contract(off)

namespace {

using vsr::sums::Luma;
using vsr::sums::quant;

constexpr int TW = VSR_WARP_TILE_W, TH = VSR_WARP_TILE_H, FT = VSR_WARP_FINISH_THREADS;
constexpr int NW = 4;   // waves per workgroup = rows of a tile in flight

struct Occ {
    double c1, c2, g1, g2;
};

// the planes of one source pixel: quantised when asked, then the three channels or their luma
template <bool YMODE, bool QUANT>
__device__ inline void planes_of(const float* __restrict__ px, const Luma& lu, double* out) {
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = QUANT ? quant(px[c]) : px[c];
    if (YMODE) {
        out[0] = vsr::sums::luma(lu, r[0], r[1], r[2]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (double)r[c];
    }
}

__device__ inline double bilinear(double q00, double q01, double q10, double q11, double wx, double ax, double wy, double ay) {
    const double r0 = wx * q00 + ax * q01;
    const double r1 = wx * q10 + ax * q11;
    return wy * r0 + ay * r1;
}

template <typename T, bool YMODE, bool QUANT>
__global__ void __launch_bounds__(NW * 64)
k_warp(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int y0, int x0, int h, int w, int shave,
       const T* __restrict__ fwd, const T* __restrict__ bwd, long long pair_stride, long long cs, long long xs, Luma lu, Occ oc,
       double* __restrict__ ws) {
    constexpr int NP = YMODE ? 1 : 3;
    __shared__ double red[2][NW * 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t frame = (size_t)blockIdx.z * H * W * 3;
    const float* __restrict__ fa = a + frame;
    const float* __restrict__ fb = b + frame;
    const T* __restrict__ ff = fwd + (long long)blockIdx.z * pair_stride;
    const T* __restrict__ bf = bwd + (long long)blockIdx.z * pair_stride;
    const int x = shave + blockIdx.x * TW + lane;
    const int ybase = shave + blockIdx.y * TH;
    const double xmax = (double)(w - 1), ymax = (double)(h - 1);

    double sse = 0.0, nvalid = 0.0;
    if (x < w - shave) {
        const int xn = min(x + 1, w - 1);
#pragma unroll 1
        for (int k = wv; k < TH; k += NW) {
            const int y = ybase + k;
            if (y >= h - shave) break;
            const int yn = min(y + 1, h - 1);
            const long long at = ((long long)y * w + x) * xs;
            const double u = (double)ff[at], v = (double)ff[cs + at];
            const double xf = (double)x + u, yf = (double)y + v;
            if (!(xf >= 0.0 && xf <= xmax && yf >= 0.0 && yf <= ymax)) continue;   // not in frame (NaN included): no index is formed
            const double xa = floor(xf), ya = floor(yf);
            const double ax = xf - xa, ay = yf - ya;
            const double wx = 1.0 - ax, wy = 1.0 - ay;
            const int ixa = (int)xa, iya = (int)ya;
            const int ixb = min(ixa + 1, w - 1), iyb = min(iya + 1, h - 1);
            // ---- consistent: the backward flow at the sample
            const long long s00 = ((long long)iya * w + ixa) * xs, s01 = ((long long)iya * w + ixb) * xs;
            const long long s10 = ((long long)iyb * w + ixa) * xs, s11 = ((long long)iyb * w + ixb) * xs;
            const double bu = bilinear((double)bf[s00], (double)bf[s01], (double)bf[s10], (double)bf[s11], wx, ax, wy, ay);
            const double bv = bilinear((double)bf[cs + s00], (double)bf[cs + s01], (double)bf[cs + s10], (double)bf[cs + s11], wx, ax, wy, ay);
            const double su = u + bu, sv = v + bv;
            const double m1 = u * u + v * v, m2 = bu * bu + bv * bv;
            const bool consistent = su * su + sv * sv <= oc.c1 * (m1 + m2) + oc.c2;
            // ---- smooth: one-sided differences of the forward flow
            const long long ar = ((long long)y * w + xn) * xs, ad = ((long long)yn * w + x) * xs;
            const double dux = (double)ff[ar] - u, duy = (double)ff[ad] - u;
            const double dvx = (double)ff[cs + ar] - v, dvy = (double)ff[cs + ad] - v;
            const bool smooth = (dux * dux + duy * duy) + (dvx * dvx + dvy * dvy) <= oc.g1 * m1 + oc.g2;
            if (!(consistent && smooth)) continue;
            // ---- the planes: frame a at the pixel, frame b around the sample (crop coordinates -> frame coordinates)
            double pa[NP], q00[NP], q01[NP], q10[NP], q11[NP];
            planes_of<YMODE, QUANT>(fa + ((size_t)(y0 + y) * W + x0 + x) * 3, lu, pa);
            planes_of<YMODE, QUANT>(fb + ((size_t)(y0 + iya) * W + x0 + ixa) * 3, lu, q00);
            planes_of<YMODE, QUANT>(fb + ((size_t)(y0 + iya) * W + x0 + ixb) * 3, lu, q01);
            planes_of<YMODE, QUANT>(fb + ((size_t)(y0 + iyb) * W + x0 + ixa) * 3, lu, q10);
            planes_of<YMODE, QUANT>(fb + ((size_t)(y0 + iyb) * W + x0 + ixb) * 3, lu, q11);
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                const double d = pa[c] - bilinear(q00[c], q01[c], q10[c], q11[c], wx, ax, wy, ay);
                sse += d * d;
            }
            nvalid += 1.0;
        }
    }
    vsr::sums::workgroup_pair<NW * 64>(red, tid, sse, nvalid, ws);
}

__global__ void __launch_bounds__(FT)
k_finish(const double* __restrict__ ws, double* __restrict__ sums, unsigned nwg, double planes, double n_pixels) {
    __shared__ double red[2][FT];
    const int tid = threadIdx.x;
    vsr::sums::finish_pair<FT>(ws + (size_t)blockIdx.x * nwg * 2, 0, nwg, red, tid);
    if (tid == 0) {
        double* out = sums + (size_t)blockIdx.x * 4;
        out[0] = red[0][0];
        out[1] = planes * red[1][0];
        out[2] = red[1][0];
        out[3] = n_pixels;
    }
}

struct Geometry {
    unsigned tiles_x, tiles_y;
};

// the checks vsr_warp_ws_bytes and vsr_warp_error share; `g` only when the result is VSR_OK
int check_region(int P, int h, int w, int shave, Geometry* g) {
    VSR_REQUIRE(P > 0 && h > 0 && w > 0, "warp_error: bad shape (P %d, crop %d x %d)", P, h, w);
    VSR_REQUIRE(shave >= 0 && 2 * (long long)shave < (h < w ? h : w), "warp_error: bad shave %d for a crop of %d x %d", shave, h, w);
    VSR_REQUIRE(P <= 65535 && h <= 65535 && w <= 65535, "warp_error: grid overflow (P %d, crop %d x %d beyond 65535)", P, h, w);
    g->tiles_x = vsr::cdiv(w - 2 * shave, TW);
    g->tiles_y = vsr::cdiv(h - 2 * shave, TH);
    return VSR_OK;
}

template <typename T>
void launch(bool ymode, bool quant, dim3 grid, hipStream_t s, const float* a, const float* b, int H, int W, int y0, int x0, int h, int w,
            int shave, const void* fwd, const void* bwd, long long ps, long long cs, long long xs, const Luma& lu, const Occ& oc, double* ws) {
    const dim3 block(NW * 64);
    const T* f = static_cast<const T*>(fwd);
    const T* g = static_cast<const T*>(bwd);
    if (ymode && quant) hipLaunchKernelGGL((k_warp<T, true, true>), grid, block, 0, s, a, b, H, W, y0, x0, h, w, shave, f, g, ps, cs, xs, lu, oc, ws);
    else if (ymode) hipLaunchKernelGGL((k_warp<T, true, false>), grid, block, 0, s, a, b, H, W, y0, x0, h, w, shave, f, g, ps, cs, xs, lu, oc, ws);
    else if (quant) hipLaunchKernelGGL((k_warp<T, false, true>), grid, block, 0, s, a, b, H, W, y0, x0, h, w, shave, f, g, ps, cs, xs, lu, oc, ws);
    else hipLaunchKernelGGL((k_warp<T, false, false>), grid, block, 0, s, a, b, H, W, y0, x0, h, w, shave, f, g, ps, cs, xs, lu, oc, ws);
}

}  // namespace

extern "C" {

int vsr_warp_abi_version(void) { return VSR_WARP_ABI_VERSION; }
const char* vsr_warp_last_error(void) { return vsr::err_buf(); }

size_t vsr_warp_ws_bytes(int P, int h, int w, int shave) {
    Geometry g;
    if (check_region(P, h, w, shave, &g) != VSR_OK) return 0;
    return (size_t)P * g.tiles_x * g.tiles_y * 2 * sizeof(double);
}

int vsr_warp_error(const float* frames_a, const float* frames_b, int P, int H, int W, int y0, int x0, int h, int w,
                   const void* flow_fwd, const void* flow_bwd, int flow_type, long long pair_stride, long long chan_stride,
                   long long pix_stride, int channels, int quantise, int shave, const float* luma4, const double* occ, double* sums,
                   void* ws, vsr_stream_t stream) {
    VSR_REQUIRE(frames_a && frames_b && flow_fwd && flow_bwd && sums && ws, "warp_error: null pointer");
    VSR_REQUIRE(occ, "warp_error: null occ (the four constants of the occlusion rule)");
    VSR_REQUIRE(flow_type == VSR_WARP_FLOW_F32 || flow_type == VSR_WARP_FLOW_F16, "warp_error: unknown flow_type %d", flow_type);
    VSR_REQUIRE(channels == VSR_WARP_RGB || channels == VSR_WARP_Y, "warp_error: unknown channels %d", channels);
    VSR_REQUIRE(quantise == 0 || quantise == 1, "warp_error: quantise must be 0 or 1, got %d", quantise);
    VSR_REQUIRE(H > 0 && W > 0, "warp_error: bad shape (frames of %d x %d)", H, W);
    Geometry g;
    const int rc0 = check_region(P, h, w, shave, &g);
    if (rc0) return rc0;
    VSR_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + h <= H && (long long)x0 + w <= W,
                "warp_error: the crop (%d, %d, %d x %d) leaves the frame of %d x %d", y0, x0, h, w, H, W);
    VSR_REQUIRE(H <= 65535 && W <= 65535, "warp_error: grid overflow (frames of %d x %d beyond 65535)", H, W);
    VSR_REQUIRE(pair_stride >= 0 && chan_stride >= 1 && pix_stride >= 1, "warp_error: bad flow strides (pair %lld, channel %lld, pixel %lld)",
                pair_stride, chan_stride, pix_stride);
    const bool ymode = channels == VSR_WARP_Y;
    VSR_REQUIRE(!ymode || luma4, "warp_error: null luma4 in Y mode");
    const uintptr_t pa = reinterpret_cast<uintptr_t>(frames_a), pb = reinterpret_cast<uintptr_t>(frames_b);
    VSR_REQUIRE(((pa | pb) & 3) == 0, "warp_error: the frames must be 4-byte aligned");
    const uintptr_t fmask = flow_type == VSR_WARP_FLOW_F32 ? 3 : 1;
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(flow_fwd) | reinterpret_cast<uintptr_t>(flow_bwd)) & fmask) == 0,
                "warp_error: the flows must be aligned to their element (%d bytes)", (int)fmask + 1);
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "warp_error: sums and the workspace must be 8-byte aligned");
    const Luma lu = ymode ? vsr::sums::luma_of(luma4) : Luma{};
    const Occ oc = {occ[0], occ[1], occ[2], occ[3]};
    const dim3 grid(g.tiles_x, g.tiles_y, P);
    hipStream_t s = vsr::S(stream);
    double* wsd = static_cast<double*>(ws);
    if (flow_type == VSR_WARP_FLOW_F32)
        launch<float>(ymode, quantise, grid, s, frames_a, frames_b, H, W, y0, x0, h, w, shave, flow_fwd, flow_bwd, pair_stride, chan_stride,
                      pix_stride, lu, oc, wsd);
    else
        launch<_Float16>(ymode, quantise, grid, s, frames_a, frames_b, H, W, y0, x0, h, w, shave, flow_fwd, flow_bwd, pair_stride, chan_stride,
                         pix_stride, lu, oc, wsd);
    const int rc = vsr::launched("warp_error/tiles");
    if (rc) return rc;
    const double planes = ymode ? 1.0 : 3.0;
    const double n_pixels = (double)(h - 2 * shave) * (double)(w - 2 * shave);
    hipLaunchKernelGGL(k_finish, dim3(P), dim3(FT), 0, s, (const double*)wsd, sums, g.tiles_x * g.tiles_y, planes, n_pixels);
    return vsr::launched("warp_error/finish");
}

}  // extern "C"
