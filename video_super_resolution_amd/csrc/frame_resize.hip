// frame_resize.hip -- float32 RGB frames resampled by a separable, table-driven filter (include/vsr_hip_resize.h; libvsr_hip_resize.so
// is built from this source alone).  The tables are the caller's: nothing here knows which filter it applies.
//
//   k_resize : one workgroup (4 waves) = one tile of TW = 32 output columns x TH = 16 output rows of one frame, both passes in one launch.
//                tables  : the tile's TW x KX and TH x KY weights and its firsts into LDS, once (the firsts clamped to [-MAX_TAPS, n - 1]:
//                          first + k then never overflows and clamps to the same index).
//                groups  : the tile's output rows are taken in groups of consecutive rows whose source rows -- the span from the lowest
//                          to the highest clamped tap of the group -- fit the ROWS rows of the LDS intermediate.  Any one row needs
//                          at most MAX_TAPS = 33 <= ROWS, so a group is never empty.  ROWS is 80 (30 KB) or 40 (15 KB, seven workgroups
//                          per compute unit instead of four): the entry guesses from H / h and KY which the tile's span will fit; the
//                          guess decides how many groups a tile takes, never a bit of the result.  A x4 reduction (17 taps, 77 rows
//                          per tile), x2 (39 rows) and every enlargement give ONE group per tile; x8 (33 taps) gives three.  Tables
//                          in no order at all (the exact tests') fall into groups of a row or two and are as correct.
//                row pass: thread i takes intermediate element i, i + 256, ...: (source row r, float e = 3 X + c of the tile's row) from
//                          global memory, KX fmas, into mid[r][e].  Lanes run along the interleaved floats: three lanes share a source
//                          pixel, neighbouring pixels are scale * 12 bytes apart, so a wave's load touches scale * 256 bytes.  The
//                          taps are loaded CH = 9 at a time before their fmas (the clamp makes a load past KX harmless; its fma
//                          is not issued): the pass waits for memory once per nine taps, not once per tap.
//                column  : thread i takes output element (row, e) (WIDE: four consecutive floats, one 16-byte LDS read per tap and one
//                          16-byte store), KY fmas down mid's rows, quantise, store.
//              LDS: lanes index FLOATS, not pixels, in both passes, so the stride of three floats per pixel never becomes a lane stride:
//              consecutive lanes write and read consecutive dwords of mid (no bank conflict: 32 lanes on 32 banks; the 16-byte reads
//              take consecutive 16-byte slots).  The weights are read as sxw[X * KX + k] with three lanes per X (a broadcast) and an odd
//              KX as the stride between pixels: conflict-free for every K = 2 ceil(support) + 1.
//
// A pixel's two chains are evaluated by one thread each, in tap order, whatever the tile or group: the bits do not depend on geometry.
// The whole file is compiled without floating-point contraction (Makefile and the pragma below); the fmas are asked for by name.
#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_resize.h"

#pragma clang fp contract(off)

namespace {

constexpr int TW = VSR_RESIZE_TILE_W, TH = VSR_RESIZE_TILE_H, MT = VSR_RESIZE_MAX_TAPS;
constexpr int TWF = 3 * TW;   // floats of a tile's row
constexpr int ROWS_L = 80, ROWS_S = 40;   // rows of the row-filtered intermediate in LDS: 30 KB / 15 KB
constexpr int NT = 256;       // threads
constexpr int CH = 9;         // taps loaded together in the row pass

static_assert(TW % 4 == 0, "a 16-byte group must not straddle two tiles");
static_assert(ROWS_S >= MT && ROWS_L >= ROWS_S, "one output row's taps must fit the intermediate");

using vsr::sums::quant;

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool QUANT, bool WIDE, int ROWS>
__global__ void __launch_bounds__(NT)
k_resize(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w, const int* __restrict__ xf,
         const float* __restrict__ xw, int KX, const int* __restrict__ yf, const float* __restrict__ yw, int KY) {
    __shared__ __align__(16) float mid[ROWS][TWF];
    __shared__ float sxw[TW * MT];
    __shared__ float syw[TH * MT];
    __shared__ int sxf[TW];
    __shared__ int syf[TH];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int ncols = min(TW, w - x0), nrows = min(TH, h - y0);
    const int nfl = 3 * ncols;   // floats of the tile's row that exist
    for (int i = tid; i < ncols * KX; i += NT) sxw[i] = xw[(size_t)x0 * KX + i];
    for (int i = tid; i < nrows * KY; i += NT) syw[i] = yw[(size_t)y0 * KY + i];
    if (tid < ncols) sxf[tid] = min(max(xf[x0 + tid], -MT), W - 1);
    if (tid < nrows) syf[tid] = min(max(yf[y0 + tid], -MT), H - 1);
    __syncthreads();

    const float* __restrict__ fs = src + (size_t)blockIdx.z * H * W * 3;
    float* __restrict__ fd = dst + ((size_t)blockIdx.z * h + y0) * w * 3 + (size_t)x0 * 3;
    const size_t spitch = (size_t)W * 3, dpitch = (size_t)w * 3;

    int g0 = 0;
    while (g0 < nrows) {
        // ---- the group g0 .. g1-1 and the span lo .. hi of source rows it addresses (the same in every thread)
        int lo = clampi(syf[g0], H - 1), hi = clampi(syf[g0] + KY - 1, H - 1), g1 = g0 + 1;
        while (g1 < nrows) {
            const int l = min(lo, clampi(syf[g1], H - 1)), u = max(hi, clampi(syf[g1] + KY - 1, H - 1));
            if (u - l + 1 > ROWS) break;
            lo = l, hi = u, ++g1;
        }
        // ---- row pass: source rows lo .. hi, the tile's columns, into mid
        const int nmid = (hi - lo + 1) * TWF;
        for (int i = tid; i < nmid; i += NT) {
            const int r = i / TWF, e = i - r * TWF;
            if (e < nfl) {
                const int xl = e / 3, c = e - 3 * xl;
                const float* __restrict__ row = fs + (size_t)(lo + r) * spitch + c;
                const float* wk = &sxw[xl * KX];
                const int first = sxf[xl];
                float t = 0.0f;
                for (int k0 = 0; k0 < KX; k0 += CH) {
                    float v[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) v[j] = row[(size_t)clampi(first + k0 + j, W - 1) * 3];
#pragma unroll
                    for (int j = 0; j < CH; ++j)
                        if (k0 + j < KX) t = fmaf(wk[k0 + j], v[j], t);
                }
                mid[r][e] = t;
            }
        }
        __syncthreads();
        // ---- column pass: output rows g0 .. g1-1
        if (WIDE) {
            constexpr int Q = TWF / 4;
            const int nout = (g1 - g0) * Q;
            for (int i = tid; i < nout; i += NT) {
                const int yl = g0 + i / Q, e = 4 * (i % Q);
                if (e < nfl) {   // (w % 4 == 0 and TW % 4 == 0: the four floats exist together)
                    const float* wk = &syw[yl * KY];
                    const int first = syf[yl];
                    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                    for (int k = 0; k < KY; ++k) {
                        const float4 v = *reinterpret_cast<const float4*>(&mid[clampi(first + k, H - 1) - lo][e]);
                        const float wv = wk[k];
                        s0 = fmaf(wv, v.x, s0);
                        s1 = fmaf(wv, v.y, s1);
                        s2 = fmaf(wv, v.z, s2);
                        s3 = fmaf(wv, v.w, s3);
                    }
                    if (QUANT) s0 = quant(s0), s1 = quant(s1), s2 = quant(s2), s3 = quant(s3);
                    *reinterpret_cast<float4*>(fd + (size_t)yl * dpitch + e) = make_float4(s0, s1, s2, s3);
                }
            }
        } else {
            const int nout = (g1 - g0) * TWF;
            for (int i = tid; i < nout; i += NT) {
                const int yl = g0 + i / TWF, e = i % TWF;
                if (e < nfl) {
                    const float* wk = &syw[yl * KY];
                    const int first = syf[yl];
                    float s = 0.0f;
                    for (int k = 0; k < KY; ++k) s = fmaf(wk[k], mid[clampi(first + k, H - 1) - lo][e], s);
                    fd[(size_t)yl * dpitch + e] = QUANT ? quant(s) : s;
                }
            }
        }
        __syncthreads();   // mid is free for the next group
        g0 = g1;
    }
}

template <int ROWS>
void launch(bool quant, bool wide, dim3 grid, hipStream_t s, const float* src, float* dst, int H, int W, int h, int w, const int* xf,
            const float* xw, int KX, const int* yf, const float* yw, int KY) {
    const dim3 block(NT);
    if (quant && wide) hipLaunchKernelGGL((k_resize<true, true, ROWS>), grid, block, 0, s, src, dst, H, W, h, w, xf, xw, KX, yf, yw, KY);
    else if (quant) hipLaunchKernelGGL((k_resize<true, false, ROWS>), grid, block, 0, s, src, dst, H, W, h, w, xf, xw, KX, yf, yw, KY);
    else if (wide) hipLaunchKernelGGL((k_resize<false, true, ROWS>), grid, block, 0, s, src, dst, H, W, h, w, xf, xw, KX, yf, yw, KY);
    else hipLaunchKernelGGL((k_resize<false, false, ROWS>), grid, block, 0, s, src, dst, H, W, h, w, xf, xw, KX, yf, yw, KY);
}

}  // namespace

extern "C" {

int vsr_resize_abi_version(void) { return VSR_RESIZE_ABI_VERSION; }
const char* vsr_resize_last_error(void) { return vsr::err_buf(); }

int vsr_resize_frames(const float* src, float* dst, int F, int H, int W, int h, int w, const int* x_first, const float* x_weight, int KX,
                      const int* y_first, const float* y_weight, int KY, int quantise, vsr_stream_t stream) {
    VSR_REQUIRE(src && dst, "resize_frames: null frame pointer");
    VSR_REQUIRE(x_first && x_weight && y_first && y_weight, "resize_frames: null table pointer");
    VSR_REQUIRE(F > 0 && H > 0 && W > 0 && h > 0 && w > 0, "resize_frames: bad shape (F %d, %d x %d -> %d x %d)", F, H, W, h, w);
    VSR_REQUIRE(H <= 2147483583 && W <= 2147483583, "resize_frames: H %d or W %d beyond 2^31 - 65 (index arithmetic)", H, W);
    VSR_REQUIRE(KX >= 1 && KX <= MT, "resize_frames: KX %d outside 1..%d", KX, MT);
    VSR_REQUIRE(KY >= 1 && KY <= MT, "resize_frames: KY %d outside 1..%d", KY, MT);
    VSR_REQUIRE(quantise == 0 || quantise == 1, "resize_frames: quantise must be 0 or 1, got %d", quantise);
    VSR_REQUIRE(F <= 65535, "resize_frames: grid overflow (F %d beyond 65535: grid dimension z)", F);
    const unsigned tx = vsr::cdiv(w, TW), ty = vsr::cdiv(h, TH);
    VSR_REQUIRE(ty <= 65535u, "resize_frames: grid overflow (%u tiles of %d output rows beyond 65535: grid dimension y)", ty, TH);
    const unsigned long long lim = 1ull << 62;
    const unsigned long long sbytes = (unsigned long long)F * H, dbytes = (unsigned long long)F * h;   // (< 2^47 each; then by 12 W)
    VSR_REQUIRE(sbytes < lim / (12ull * W) && dbytes < lim / (12ull * w), "resize_frames: a frame set of 2^62 bytes or more");
    const unsigned long long sb = sbytes * W * 12ull, db = dbytes * w * 12ull;
    const uintptr_t ps = reinterpret_cast<uintptr_t>(src), pd = reinterpret_cast<uintptr_t>(dst);
    VSR_REQUIRE(((ps | pd) & 3) == 0, "resize_frames: the frames must be 4-byte aligned");
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(x_first) | reinterpret_cast<uintptr_t>(x_weight) | reinterpret_cast<uintptr_t>(y_first) |
                  reinterpret_cast<uintptr_t>(y_weight)) & 3) == 0, "resize_frames: the tables must be 4-byte aligned");
    VSR_REQUIRE(ps + sb <= pd || pd + db <= ps, "resize_frames: src and dst overlap");
    const bool wide = (pd & 15) == 0 && w % 4 == 0;   // 16-byte stores: an aligned base and rows of a whole number of 16-byte groups
    // the span a tile's rows will address if the tables are those of a resize from H to h (a guess that only chooses the LDS size)
    const bool small = (double)(TH - 1) * (double)H / (double)h + (double)KY <= (double)ROWS_S;
    const dim3 grid(tx, ty, F);
    hipStream_t s = vsr::S(stream);
    if (small) launch<ROWS_S>(quantise, wide, grid, s, src, dst, H, W, h, w, x_first, x_weight, KX, y_first, y_weight, KY);
    else launch<ROWS_L>(quantise, wide, grid, s, src, dst, H, W, h, w, x_first, x_weight, KX, y_first, y_weight, KY);
    return vsr::launched("resize_frames");
}

}  // extern "C"
