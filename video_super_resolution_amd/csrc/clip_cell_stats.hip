// clip_cell_stats.hip -- a resident group of frames measured per cell and frame in one launch (include/vsr_hip_cell.h; libvsr_hip_cell.so
// is built from this source alone): the spatial activity of every cell of VSR_CELL x VSR_CELL pixels and its absolute luma difference
// against the frame before, both on the 8-bit luma code of include/vsr_hip_scene.h.
//
//   k_cell : one workgroup of WT = 256 threads = one tile of TH x TW = 16 x 64 pixels (one cell down, four across; grid = (tiles across,
//            tiles down)), walking g = 0 .. G-1.  Thread (r, xt) = (tid / 16, tid % 16) owns the pixels 4 xt .. 4 xt + 3 of tile row r: 48
//            bytes, three 16-byte loads on the VEC path (a row of the tile is 768 consecutive bytes over 16 lanes), twelve element loads
//            with a test per pixel otherwise.  Its four codes of frame g - 1 stay in registers for the temporal term, so a frame is read
//            once.  The codes of frame g go to LDS as [17][LP] int32 for the spatial term's neighbours: row 16 is the first row of the tile
//            below (threads 0..15 load it, one more row of the same shape), column 64 the first column of the tile to the right (threads
//            16..31, one pixel each): the only reads beyond the tile.  A neighbour outside the frame is never read and its term is left
//            out.  Sums: int32 per thread, then over the four lanes of a cell's row and the four rows of the wave by lane exchanges, then
//            the four waves through 32 words of LDS; thread 2 j + c stores channel c of cell j.  Two barriers per frame: codes written |
//            neighbours read, partials written | next frame's codes.
// Integer sums of integers: exact in any order; nothing here is atomic.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): every product and sum of the luma
// rounds once, as a float64 restatement in numpy does.
#include <cmath>
#include <cstdint>

#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_cell.h"

#pragma clang fp contract(off)

namespace {

using vsr::sums::Luma;

constexpr int C = VSR_CELL, TH = VSR_CELL_TILE_H, TW = VSR_CELL_TILE_W;
constexpr int WT = 256;
constexpr int PPT = 4;            // pixels per thread: 48 bytes, three float4
constexpr int XT = TW / PPT;      // threads across a tile row
constexpr int CPT = TW / C;       // cells of a tile
constexpr int LP = TW + 4;        // LDS pitch in words: a row's four codes of a thread stay 16-byte aligned, the halo column fits
static_assert(TH == C && TW % C == 0, "a tile is one row of whole cells");
static_assert(XT * TH == WT && XT == 16 && C / PPT == 4, "lane = (r % 4) * 16 + xt: a cell's row is lanes 4 j .. 4 j + 3, a wave four rows");

// the 8-bit luma code of one pixel: steps 1 to 4 of the header
__device__ inline int code_of(const Luma& lu, float r, float g, float b) {
    double q = vsr::sums::luma(lu, r, g, b);
    q = q >= 0.0 ? q : 0.0;   // negatives and NaN
    q = q > 255.0 ? 255.0 : q;
    return (int)rint(q);
}

// the codes of the pixels (y, x .. x + 3) of frame `f`; 0 for a pixel outside the frame, which is not read
template <bool VEC>
__device__ inline void codes4(const float* __restrict__ f, int y, int x, int H, int W, const Luma& lu, int (&q)[PPT]) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) q[k] = 0;
    if (y >= H) return;
    const float* __restrict__ p = f + ((size_t)y * W + x) * 3;
    if (VEC) {   // W % 4 == 0 and x % 4 == 0: the group of four lies inside the row or outside it
        if (x >= W) return;
        const float4* __restrict__ v = reinterpret_cast<const float4*>(p);
        const float4 a = v[0], b = v[1], c = v[2];
        q[0] = code_of(lu, a.x, a.y, a.z);
        q[1] = code_of(lu, a.w, b.x, b.y);
        q[2] = code_of(lu, b.z, b.w, c.x);
        q[3] = code_of(lu, c.y, c.z, c.w);
    } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (x + k < W) q[k] = code_of(lu, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(WT)
k_cell(const float* __restrict__ frames, int G, int H, int W, Luma lu, int* __restrict__ stats, int Ch, int Cw) {
    __shared__ __attribute__((aligned(16))) int qs[(TH + 1) * LP];
    __shared__ int red[WT / 64][CPT][2];
    const int tid = threadIdx.x, r = tid / XT, xt = tid % XT;
    const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
    const int y = ty0 + r, x0 = tx0 + xt * PPT;
    const size_t plane = (size_t)H * W * 3;
    int prev[PPT] = {0, 0, 0, 0};
    for (int g = 0; g < G; ++g) {
        const float* __restrict__ f = frames + (size_t)g * plane;
        int q[PPT];
        codes4<VEC>(f, y, x0, H, W, lu, q);
#pragma unroll
        for (int k = 0; k < PPT; ++k) qs[r * LP + xt * PPT + k] = q[k];
        if (tid < XT) {   // the row below the tile
            int hq[PPT];
            codes4<VEC>(f, ty0 + TH, tx0 + tid * PPT, H, W, lu, hq);
#pragma unroll
            for (int k = 0; k < PPT; ++k) qs[TH * LP + tid * PPT + k] = hq[k];
        } else if (tid < 2 * XT) {   // the column right of the tile
            const int rr = tid - XT, yy = ty0 + rr, xx = tx0 + TW;
            int hq = 0;
            if (yy < H && xx < W) {
                const float* __restrict__ p = f + ((size_t)yy * W + xx) * 3;
                hq = code_of(lu, p[0], p[1], p[2]);
            }
            qs[rr * LP + TW] = hq;
        }
        __syncthreads();
        int act = 0, sad = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int x = x0 + k;
            if (y < H && x < W) {
                const int right = k + 1 < PPT ? q[k + 1] : qs[r * LP + xt * PPT + PPT];
                if (x + 1 < W) act += abs(q[k] - right);
                if (y + 1 < H) act += abs(q[k] - qs[(r + 1) * LP + xt * PPT + k]);
                if (g > 0) sad += abs(q[k] - prev[k]);
            }
            prev[k] = q[k];
        }
        // lane = (r % 4) * 16 + xt: bits 0, 1 run over the four threads of a cell's row, bits 4, 5 over the wave's four rows
#pragma unroll
        for (int m : {1, 2, 16, 32}) {
            act += __shfl_xor(act, m, 64);
            sad += __shfl_xor(sad, m, 64);
        }
        const int lane = tid & 63, wave = tid >> 6;
        if ((lane & 0x33) == 0) {
            red[wave][lane >> 2][0] = act;
            red[wave][lane >> 2][1] = sad;
        }
        __syncthreads();
        if (tid < 2 * CPT) {
            const int j = tid >> 1, c = tid & 1, cj = blockIdx.x * CPT + j;
            if (cj < Cw) stats[(((size_t)g * Ch + blockIdx.y) * Cw + cj) * 2 + c] = red[0][j][c] + red[1][j][c] + red[2][j][c] + red[3][j][c];
        }
    }
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

extern "C" {

int vsr_cell_abi_version(void) { return VSR_CELL_ABI_VERSION; }
const char* vsr_cell_last_error(void) { return vsr::err_buf(); }

int vsr_cell_stats(const float* frames, int G, int H, int W, const float* luma4, int* stats, vsr_stream_t stream) {
    VSR_REQUIRE(frames && stats, "cell_stats: null pointer");
    VSR_REQUIRE(luma4, "cell_stats: null luma4 (the four values of the luma row)");
    VSR_REQUIRE(G > 0 && H > 0 && W > 0, "cell_stats: bad shape (G %d, frames of %d x %d)", G, H, W);
    VSR_REQUIRE(H <= 65535 && W <= 65535, "cell_stats: grid overflow (frames of %d x %d beyond 65535)", H, W);
    VSR_REQUIRE(G <= VSR_CELL_MAX_G, "cell_stats: G = %d is beyond VSR_CELL_MAX_G = %d", G, VSR_CELL_MAX_G);
    VSR_REQUIRE(((addr(frames) | addr(stats)) & 3) == 0, "cell_stats: frames and stats must be 4-byte aligned");
    const Luma lu = vsr::sums::luma_of(luma4);
    const int Ch = vsr::cdiv(H, C), Cw = vsr::cdiv(W, C);
    const bool vec = (addr(frames) & 15) == 0 && W % 4 == 0;
    const dim3 grid(vsr::cdiv(W, TW), vsr::cdiv(H, TH));
    hipStream_t s = vsr::S(stream);
    if (vec) hipLaunchKernelGGL(k_cell<true>, grid, dim3(WT), 0, s, frames, G, H, W, lu, stats, Ch, Cw);
    else hipLaunchKernelGGL(k_cell<false>, grid, dim3(WT), 0, s, frames, G, H, W, lu, stats, Ch, Cw);
    return vsr::launched("cell_stats");
}

}  // extern "C"
