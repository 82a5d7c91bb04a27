// frame_sums.h -- the device helpers the float64-sum kernels share: quantisation as write-out does it, the luma of "y" mode, the
// fixed-order tree, and the two halves of "one pair of doubles per workgroup, then a finish kernel adds the partials".
//
// For frame_metric.hip, frame_msssim.hip (both also through frame_ssim.h), frame_warp_error.hip, frame_resize.hip, train_update.hip,
// clip_scene.hip and clip_cell_stats.hip ONLY: the sources compiled with -ffp-contract=off (Makefile) that state the pragma themselves, whose results the tests
// pin bit for bit.  Every operation below rounds once, in the order written, as it did when each of those sources held its own copy; no
// source built with contraction includes this header.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace vsr {
namespace sums {

// a sample as an 8-bit file holds it: clamped to 0..255, rounded half to even
__device__ inline float quant(float v) {
    v = v >= 0.0f ? v : 0.0f;   // negatives and NaN
    v = v > 255.0f ? 255.0f : v;
    return rintf(v);
}

// {a0, a1, a2, o}: row 0 of the matrix and its offset, as the caller's four floats give them
struct Luma {
    double a0, a1, a2, o;
};
inline Luma luma_of(const float* luma4) { return {(double)luma4[0], (double)luma4[1], (double)luma4[2], (double)luma4[3]}; }
__device__ inline double luma(const Luma& lu, float r, float g, float b) {
    return ((lu.o + lu.a0 * (double)r) + lu.a1 * (double)g) + lu.a2 * (double)b;
}

// fixed-order tree over N (a power of two) values in LDS; the total ends in red[0]
template <int N>
__device__ inline void tree(double* red, int tid) {
#pragma unroll
    for (int s = N / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    __syncthreads();
}

// two running sums per thread of a workgroup of N, each through the tree; the totals end in red[0][0] and red[1][0]
template <int N>
__device__ inline void tree_pair(double (*red)[N], int tid, double s0, double s1) {
    red[0][tid] = s0;
    red[1][tid] = s1;
    tree<N>(red[0], tid);
    tree<N>(red[1], tid);
}

// the end of a tile kernel of N threads: the threads' two running sums through the tree, one pair of doubles per workgroup into the
// workspace, workgroups numbered x fastest, then y, then z
template <int N>
__device__ inline void workgroup_pair(double (*red)[N], int tid, double s0, double s1, double* ws) {
    tree_pair<N>(red, tid, s0, s1);
    if (tid == 0) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        ws[2 * wg] = red[0][0];
        ws[2 * wg + 1] = red[1][0];
    }
}

// the body of a finish kernel of FT threads, one workgroup per sum over the pairs [i0, i1) of `p`: thread t adds the partials i0 + t,
// i0 + t + FT, ... in that order, then the same tree; the two totals end in red[0][0] and red[1][0], for thread 0's epilogue
template <int FT>
__device__ inline void finish_pair(const double* p, unsigned i0, unsigned i1, double (*red)[FT], int tid) {
    double s0 = 0.0, s1 = 0.0;
    for (unsigned i = i0 + tid; i < i1; i += FT) {
        s0 += p[2 * (size_t)i];
        s1 += p[2 * (size_t)i + 1];
    }
    tree_pair<FT>(red, tid, s0, s1);
}

}  // namespace sums
}  // namespace vsr
