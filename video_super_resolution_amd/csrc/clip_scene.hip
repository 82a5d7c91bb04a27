// clip_scene.hip -- scene cuts in a streamed clip on the device (include/vsr_hip_scene.h; libvsr_hip_scene.so is built from this source
// alone): the absolute luma difference of a pair of LR frames summed in float64, the cut rule on the sums, and the window and fed-back
// estimate composed under the rule's flags.
//
//   k_pair   : one workgroup of WT = 256 threads = WGP = VSR_SCENE_WG_PIXELS = 1024 consecutive pixels of one pair (grid = (chunks, 1, P)).
//              VEC: thread t takes the pixels 4 t .. 4 t + 3 of the chunk as three 16-byte loads per frame (12 floats = 4 pixels);
//              otherwise the pixels t, t + 256, t + 512, t + 768 as element loads.  Luma, quantisation and |difference| per pixel in
//              double, then a fixed-order tree over the 256 threads and one double into the workspace.
//   k_finish : one workgroup of FT = 256 threads per pair: thread t adds the partials t, t + 256, ... in that order, then the same tree;
//              thread 0 writes {sad, n}.
//   k_decide : one thread per pair: two divisions, one product, two comparisons.
//   k_window : one thread per LR pixel: the three 32-bit words of the pixel for x3[0], x3[1], x3[2] and est, each a copy of one input
//              word chosen by the two flags (uniform over the launch; a frame that loses the choice is not read).
// Nothing here is atomic and no order depends on timing or on P.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): every product and sum of the
// header's steps rounds once, as a float64 restatement in numpy does.
#include <cmath>
#include <cstdint>

#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_scene.h"

#pragma clang fp contract(off)

namespace {

using vsr::sums::Luma;

constexpr int WGP = VSR_SCENE_WG_PIXELS, FT = VSR_SCENE_FINISH_THREADS;
constexpr int WT = 256;          // threads of k_pair
constexpr int PPT = WGP / WT;    // pixels per thread
static_assert(PPT == 4, "the 16-byte path takes four pixels as three float4");

// the 8-bit luma code of one pixel: the header's steps 1 to 4
__device__ inline double code_of(const Luma& lu, float r, float g, float b) {
    double q = vsr::sums::luma(lu, r, g, b);
    q = q >= 0.0 ? q : 0.0;   // negatives and NaN
    q = q > 255.0 ? 255.0 : q;
    return rint(q);
}

template <bool VEC>
__global__ void __launch_bounds__(WT)
k_pair(const float* __restrict__ a, const float* __restrict__ b, unsigned long long n, Luma lu, double* __restrict__ ws) {
    __shared__ double red[WT];
    const int tid = threadIdx.x;
    const size_t frame = (size_t)blockIdx.z * n * 3;
    const float* __restrict__ fa = a + frame;
    const float* __restrict__ fb = b + frame;
    const unsigned long long base = (unsigned long long)blockIdx.x * WGP;
    double sad = 0.0;
    if (VEC) {   // n % 4 == 0: a group of four pixels lies inside the frame or outside it
        const unsigned long long p0 = base + (unsigned long long)tid * PPT;
        if (p0 < n) {
            const float4* __restrict__ va = reinterpret_cast<const float4*>(fa + p0 * 3);
            const float4* __restrict__ vb = reinterpret_cast<const float4*>(fb + p0 * 3);
            const float4 a0 = va[0], a1 = va[1], a2 = va[2];
            const float4 b0 = vb[0], b1 = vb[1], b2 = vb[2];
            sad += fabs(code_of(lu, a0.x, a0.y, a0.z) - code_of(lu, b0.x, b0.y, b0.z));
            sad += fabs(code_of(lu, a0.w, a1.x, a1.y) - code_of(lu, b0.w, b1.x, b1.y));
            sad += fabs(code_of(lu, a1.z, a1.w, a2.x) - code_of(lu, b1.z, b1.w, b2.x));
            sad += fabs(code_of(lu, a2.y, a2.z, a2.w) - code_of(lu, b2.y, b2.z, b2.w));
        }
    } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const unsigned long long p = base + (unsigned long long)k * WT + tid;
            if (p < n) {
                const float* __restrict__ pa = fa + p * 3;
                const float* __restrict__ pb = fb + p * 3;
                sad += fabs(code_of(lu, pa[0], pa[1], pa[2]) - code_of(lu, pb[0], pb[1], pb[2]));
            }
        }
    }
    red[tid] = sad;
    vsr::sums::tree<WT>(red, tid);
    if (tid == 0) ws[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(FT)
k_finish(const double* __restrict__ ws, double* __restrict__ sums, unsigned nwg, double n_pixels) {
    __shared__ double red[FT];
    const int tid = threadIdx.x;
    const double* p = ws + (size_t)blockIdx.x * nwg;
    double s = 0.0;
    for (unsigned i = tid; i < nwg; i += FT) s += p[i];
    red[tid] = s;
    vsr::sums::tree<FT>(red, tid);
    if (tid == 0) {
        double* out = sums + (size_t)blockIdx.x * 2;
        out[0] = red[0];
        out[1] = n_pixels;
    }
}

__global__ void __launch_bounds__(256)
k_decide(const double* __restrict__ sums, int P, const double* __restrict__ prev, double t_abs, double ratio, int* __restrict__ flags) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double m = sums[2 * (size_t)p] / sums[2 * (size_t)p + 1];
    double m_prev = 0.0;
    if (p > 0) m_prev = sums[2 * (size_t)(p - 1)] / sums[2 * (size_t)(p - 1) + 1];
    else if (prev) m_prev = prev[0] / prev[1];
    const double bar = ratio * m_prev;
    flags[p] = (m >= t_abs && m >= bar) ? 1 : 0;
}

// words, not floats: a copy of the bits whatever they encode
template <bool EST>
__global__ void __launch_bounds__(256)
k_window(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c, const uint32_t* __restrict__ prev,
         int S, int W, const int* __restrict__ flag_ab, const int* __restrict__ flag_bc, uint32_t* __restrict__ x3, uint32_t* __restrict__ est,
         int h, int w) {
    const unsigned long long n = (unsigned long long)h * w;
    const unsigned long long p = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const bool fab = flag_ab ? *flag_ab != 0 : false;
    const bool fbc = flag_bc ? *flag_bc != 0 : false;
    const size_t at = (size_t)p * 3, plane = (size_t)n * 3;
    uint32_t vb[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vb[k] = b[at + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) x3[plane + at + k] = vb[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = fab ? vb[k] : a[at + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) x3[at + k] = v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = fbc ? vb[k] : c[at + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) x3[2 * plane + at + k] = v[k];
    if (EST) {
        const unsigned y = (unsigned)(p / (unsigned)w), x = (unsigned)(p - (unsigned long long)y * (unsigned)w);
        const size_t src = ((size_t)y * S * W + (size_t)x * S) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = fab ? vb[k] : prev[src + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) est[at + k] = v[k];
    }
}

// the checks vsr_scene_ws_bytes and vsr_scene_pair_sums share; `chunks` only when the result is VSR_OK
int check_pairs(int P, int h, int w, unsigned* chunks) {
    VSR_REQUIRE(P > 0 && h > 0 && w > 0, "scene_pair_sums: bad shape (P %d, frames of %d x %d)", P, h, w);
    VSR_REQUIRE(P <= 65535 && h <= 65535 && w <= 65535, "scene_pair_sums: grid overflow (P %d, frames of %d x %d beyond 65535)", P, h, w);
    *chunks = vsr::cdiv((long long)h * w, WGP);
    return VSR_OK;
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

extern "C" {

int vsr_scene_abi_version(void) { return VSR_SCENE_ABI_VERSION; }
const char* vsr_scene_last_error(void) { return vsr::err_buf(); }

size_t vsr_scene_ws_bytes(int P, int h, int w) {
    unsigned chunks;
    if (check_pairs(P, h, w, &chunks) != VSR_OK) return 0;
    return (size_t)P * chunks * sizeof(double);
}

int vsr_scene_pair_sums(const float* a, const float* b, int P, int h, int w, const float* luma4, double* sums, void* ws,
                        vsr_stream_t stream) {
    VSR_REQUIRE(a && b && sums && ws, "scene_pair_sums: null pointer");
    VSR_REQUIRE(luma4, "scene_pair_sums: null luma4 (the four values of the luma row)");
    unsigned chunks;
    const int rc0 = check_pairs(P, h, w, &chunks);
    if (rc0) return rc0;
    VSR_REQUIRE(((addr(a) | addr(b)) & 3) == 0, "scene_pair_sums: the frames must be 4-byte aligned");
    VSR_REQUIRE(((addr(sums) | addr(ws)) & 7) == 0, "scene_pair_sums: sums and the workspace must be 8-byte aligned");
    const Luma lu = vsr::sums::luma_of(luma4);
    const unsigned long long n = (unsigned long long)h * w;
    const bool vec = ((addr(a) | addr(b)) & 15) == 0 && n % 4 == 0;
    const dim3 grid(chunks, 1, P);
    hipStream_t s = vsr::S(stream);
    double* wsd = static_cast<double*>(ws);
    if (vec) hipLaunchKernelGGL(k_pair<true>, grid, dim3(WT), 0, s, a, b, n, lu, wsd);
    else hipLaunchKernelGGL(k_pair<false>, grid, dim3(WT), 0, s, a, b, n, lu, wsd);
    const int rc = vsr::launched("scene_pair_sums/pixels");
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(P), dim3(FT), 0, s, (const double*)wsd, sums, chunks, (double)h * (double)w);
    return vsr::launched("scene_pair_sums/finish");
}

int vsr_scene_decide(const double* sums, int P, const double* prev_or_null, double t_abs, double ratio, int* flags, vsr_stream_t stream) {
    VSR_REQUIRE(sums && flags, "scene_decide: null pointer");
    VSR_REQUIRE(P > 0, "scene_decide: bad count (P %d)", P);
    VSR_REQUIRE(std::isfinite(t_abs) && t_abs >= 0.0, "scene_decide: t_abs must be finite and not negative, got %g", t_abs);
    VSR_REQUIRE(std::isfinite(ratio) && ratio >= 0.0, "scene_decide: ratio must be finite and not negative, got %g", ratio);
    VSR_REQUIRE(((addr(sums) | addr(prev_or_null)) & 7) == 0, "scene_decide: sums and prev must be 8-byte aligned");
    VSR_REQUIRE((addr(flags) & 3) == 0, "scene_decide: flags must be 4-byte aligned");
    hipLaunchKernelGGL(k_decide, dim3(vsr::cdiv(P, 256)), dim3(256), 0, vsr::S(stream), sums, P, prev_or_null, t_abs, ratio, flags);
    return vsr::launched("scene_decide");
}

int vsr_scene_window(const float* a, const float* b, const float* c, const float* prev_est_or_null, int H, int W,
                     const int* flag_ab_or_null, const int* flag_bc_or_null, float* x3, float* est_or_null, int h, int w,
                     vsr_stream_t stream) {
    VSR_REQUIRE(a && b && c && x3, "scene_window: null pointer");
    VSR_REQUIRE((prev_est_or_null != nullptr) == (est_or_null != nullptr),
                "scene_window: est and prev_est are both given or both null (got est %s, prev_est %s)", est_or_null ? "given" : "null",
                prev_est_or_null ? "given" : "null");
    VSR_REQUIRE(h > 0 && w > 0, "scene_window: bad shape (frames of %d x %d)", h, w);
    VSR_REQUIRE(h <= 65535 && w <= 65535, "scene_window: grid overflow (frames of %d x %d beyond 65535)", h, w);
    int S = 1;
    if (prev_est_or_null) {
        VSR_REQUIRE(H > 0 && W > 0, "scene_window: bad shape (estimate of %d x %d)", H, W);
        VSR_REQUIRE(H % h == 0 && W % w == 0, "scene_window: the estimate of %d x %d is no integer multiple of %d x %d", H, W, h, w);
        VSR_REQUIRE(H / h == W / w, "scene_window: unequal factors (%d down, %d across)", H / h, W / w);
        S = H / h;
    }
    VSR_REQUIRE(((addr(a) | addr(b) | addr(c) | addr(prev_est_or_null) | addr(x3) | addr(est_or_null)) & 3) == 0,
                "scene_window: the frames must be 4-byte aligned");
    VSR_REQUIRE(((addr(flag_ab_or_null) | addr(flag_bc_or_null)) & 3) == 0, "scene_window: the flags must be 4-byte aligned");
    const dim3 grid(vsr::cdiv((long long)h * w, 256));
    hipStream_t s = vsr::S(stream);
    const uint32_t *ua = reinterpret_cast<const uint32_t*>(a), *ub = reinterpret_cast<const uint32_t*>(b);
    const uint32_t *uc = reinterpret_cast<const uint32_t*>(c), *up = reinterpret_cast<const uint32_t*>(prev_est_or_null);
    uint32_t *ux = reinterpret_cast<uint32_t*>(x3), *ue = reinterpret_cast<uint32_t*>(est_or_null);
    if (est_or_null) hipLaunchKernelGGL(k_window<true>, grid, dim3(256), 0, s, ua, ub, uc, up, S, W, flag_ab_or_null, flag_bc_or_null, ux, ue, h, w);
    else hipLaunchKernelGGL(k_window<false>, grid, dim3(256), 0, s, ua, ub, uc, up, S, W, flag_ab_or_null, flag_bc_or_null, ux, ue, h, w);
    return vsr::launched("scene_window");
}

}  // extern "C"
