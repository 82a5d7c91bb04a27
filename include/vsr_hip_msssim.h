/*
 * vsr_hip_msssim.h -- C ABI of libvsr_hip_msssim.so: HR frames scored against ground truth on MI355X (gfx950) at five scales: the sums
 * behind multi-scale SSIM (Wang, Simoncelli, Bovik 2003), per frame, plane and level, in float64.
 *
 * A library of its own (csrc/frame_msssim.hip alone; libvsr_hip_metric.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip_metric.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_msssim_last_error()` gives a
 * thread-local message).
 *
 * Frames: `a`, `b` float32 RGB [F,H,W,3], dense, in the model's 0..255 range.  Only 4-byte alignment is required: 16-byte loads are
 * taken where both bases are 16-byte aligned and W % 4 == 0, element loads otherwise; the values are the same.
 *
 * Result: `sums`, device double [F][P][5][2] = {cs_sum, ssim_sum} per frame, plane and level; P = 3 (VSR_MSSSIM_RGB: R, G, B) or 1
 * (VSR_MSSSIM_Y).  The library forms no mean and no power: the host divides by n_j = (h_j - 10) * (w_j - 10) and combines the levels
 * (driver.msssim).  Every element is written by every call.
 *
 * What is computed, in the order the switches apply:
 *   1. quantise (0 / 1).  1: every value is first taken to what write-out stores: v = v >= 0 ? v : 0 (negatives and NaN), v = v > 255 ?
 *      255 : v, v = rintf(v) (ties to even).  0: the floats as they are.
 *   2. shave >= 0: that many pixels are dropped on every side; h = H - 2 shave, w = W - 2 shave.
 *   3. channels.  VSR_MSSSIM_RGB: three planes, each the channel as a double.  VSR_MSSSIM_Y: one plane
 *      y = ((o + a0 * R) + a1 * G) + a2 * B, every operation in double and rounded once (no contraction), from the four float32 values
 *      of the HOST pointer luma4 = {a0, a1, a2, o}, read at the call and passed by value.  luma4 may be null in RGB mode.
 *      (Steps 1 to 3 are those of include/vsr_hip_metric.h.)  They give level 1: planes of h_1 x w_1 = h x w.
 *   4. Levels 2 to 5.  h_{j+1} = ceil(h_j / 2), w_{j+1} = ceil(w_j / 2), and
 *        p_{j+1}[y][x] = ((p00 + p01) + (p10 + p11)) * 0.25,  p_rc = p_j[min(2 y + r, h_j - 1)][min(2 x + c, w_j - 1)]
 *      in double, every operation rounded once: the 2 x 2 mean, an odd size repeating its last row or column (the symmetric padding of
 *      tf.image.ssim_multiscale and of the original MATLAB code).  The pooled planes are doubles in the workspace.  Five levels, always.
 *   5. At every level, per plane, the five windowed sums of step 6 of include/vsr_hip_metric.h: win11 is a HOST pointer to 11 doubles,
 *      a normalised 1-D window (driver.ssim_window), read at the call and passed by value; mu_a, mu_b, E[aa], E[bb], E[ab] over the
 *      VALID positions only: the map of level j is (h_j - 10) x (w_j - 10).  Each sum is s = fma(win[k], t_k, s) for k = 0..10 from
 *      s = 0, along the row and then down the column; the terms of the second moments are the products a*a, b*b, a*b, rounded once.
 *   6. The two maps, without contraction:
 *        s_aa = E[aa] - mu_a * mu_a,  s_bb alike,  s_ab = E[ab] - mu_a * mu_b
 *        cs   = (2 * s_ab + C2) / ((s_aa + s_bb) + C2)
 *        ssim = ((2 * (mu_a * mu_b) + C1) * (2 * s_ab + C2)) / (((mu_a * mu_a + mu_b * mu_b) + C1) * ((s_aa + s_bb) + C2))
 *      with C1 = (0.01 * 255)^2 and C2 = (0.03 * 255)^2.  a == b gives cs == ssim == 1.0 exactly at every position of every level.
 *   7. Reduction: per thread in double, per workgroup a fixed-order tree, one pair of partials per workgroup and plane into the
 *      workspace; a finish launch (one workgroup of VSR_MSSSIM_FINISH_THREADS per frame, plane and level) has thread t sum the level's
 *      partials t, t + threads, ... in that order and ends in the same tree.  No atomics: the numbers of a frame are bit-identical
 *      from run to run and depend neither on F nor on the frame's place in the batch.
 *
 * Launch geometry (csrc/frame_msssim.hip): three launches.  The pyramid pass: one workgroup per level-1 tile of
 * VSR_MSSSIM_PYR_ROWS x VSR_MSSSIM_PYR_COLS pixels (all planes, both frames), which holds every descendant of its pixels.  The
 * scoring pass: one workgroup per tile of VSR_MSSSIM_STRIP_WIDTH map columns by VSR_MSSSIM_SEGMENT_ROWS map rows of one level, the
 * tiles of all five levels in one grid.  The finish.
 */
#ifndef VSR_HIP_MSSSIM_H
#define VSR_HIP_MSSSIM_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_MSSSIM_ABI_VERSION 1

#define VSR_MSSSIM_RGB 0
#define VSR_MSSSIM_Y 1

#define VSR_MSSSIM_LEVELS 5
#define VSR_MSSSIM_MIN_SIZE 161 /* 161, 81, 41, 21, 11: the smallest that leaves one window at level 5 */

#define VSR_MSSSIM_PYR_ROWS 16
#define VSR_MSSSIM_PYR_COLS 64
#define VSR_MSSSIM_STRIP_WIDTH 64
#define VSR_MSSSIM_SEGMENT_ROWS 64
#define VSR_MSSSIM_FINISH_THREADS 64

int vsr_msssim_abi_version(void);
const char* vsr_msssim_last_error(void);

/* Bytes of workspace vsr_msssim_frames needs for these arguments: the pooled planes of levels 2 to 5 (both frames, every plane, as
 * doubles) and two doubles per scoring workgroup and plane.  0 for arguments that call would refuse.  The library never zeroes the
 * workspace and never reads a byte of it that the same call has not written. */
size_t vsr_msssim_ws_bytes(int F, int H, int W, int shave, int channels);

/* Refused before any launch, each with its message: a null a / b / win11 / sums / ws, a null luma4 in VSR_MSSSIM_Y; an unknown
 * `channels`; `quantise` other than 0 / 1; non-positive F / H / W; shave < 0; min(H, W) - 2 * shave < VSR_MSSSIM_MIN_SIZE; F, H or W
 * beyond 65535 (grid dimensions y and z; offsets are 64-bit); a or b not 4-byte aligned, sums or ws not 8-byte aligned. */
int vsr_msssim_frames(const float* a, const float* b, int F, int H, int W, int channels, int quantise, int shave, const float* luma4,
                      const double* win11, double* sums, void* ws, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_MSSSIM_H */
