/*
 * vsr_hip_metric.h -- C ABI of libvsr_hip_metric.so: HR frames scored against ground truth on MI355X (gfx950): the sums behind PSNR
 * and SSIM (Wang, Bovik, Sheikh, Simoncelli 2004), per frame, in float64.
 *
 * A library of its own (csrc/frame_metric.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_metric_last_error()` gives a
 * thread-local message).
 *
 * Frames: `a`, `b` float32 RGB [F,H,W,3], dense, in the model's 0..255 range.  Only 4-byte alignment is required: 16-byte loads are
 * taken where both bases are 16-byte aligned and W % 4 == 0 (then every frame starts on a multiple of 16 bytes and an aligned group of
 * four floats never leaves the buffer), element loads otherwise; the values are the same.
 *
 * Result: `sums`, device double [F][4] = {sse, n_sse, ssim_sum, n_ssim} per frame.  The host forms PSNR = 10 log10(255^2 n_sse / sse)
 * and SSIM = ssim_sum / n_ssim; the library does neither (an sse of 0 is a legitimate result).  The two slots of a metric that was
 * not asked for are written as 0.
 *
 * What is computed, in the order the switches apply:
 *   1. quantise (0 / 1).  1: every value is first taken to what write-out stores: v = v >= 0 ? v : 0 (negatives and NaN), v = v > 255 ?
 *      255 : v, v = rintf(v) (ties to even): the code vsr_frame_to_u8 stores.  0: the floats as they are.
 *   2. shave >= 0: that many pixels are dropped on every side, before either metric; h = H - 2 shave, w = W - 2 shave.
 *   3. channels.  VSR_METRIC_RGB: three planes; SSE over 3 h w terms, SSIM summed over the three planes' maps.
 *      VSR_METRIC_Y: one plane y = ((o + a0 * R) + a1 * G) + a2 * B, every operation in double and rounded once (no contraction), from
 *      the four float32 values of the HOST pointer luma4 = {a0, a1, a2, o}, read at the call and passed by value.  The library
 *      computes no coefficient (driver.yuv_coefficients row 0 is their source).  luma4 may be null in RGB mode.
 *   4. what: bit 0 (VSR_METRIC_SSE) and bit 1 (VSR_METRIC_SSIM).
 *   5. SSE: d = (double)x_a - (double)x_b, every term d * d rounded once in double, summed in double.  n_sse = planes * h * w.
 *   6. SSIM: win11 is a HOST pointer to 11 doubles, a normalised 1-D window (driver.ssim_window: exp(-(i - 5)^2 / (2 * 1.5^2)) over its
 *      sum), read at the call and passed by value; the 2-D window is its outer product, evaluated separably, rows first.  Five
 *      windowed sums per plane, in double: mu_a, mu_b, E[aa], E[bb], E[ab], over the VALID positions only (no padding): the map is
 *      (h - 10) x (w - 10).  Each sum is s = fma(win[k], t_k, s) for k = 0..10 from s = 0, along the row and then down the column;
 *      the terms of the second moments are the products a*a, b*b, a*b, rounded once: the three are formed by one sequence of
 *      operations, so a == b gives 1.0 exactly at every position.  Then, without contraction,
 *        s_aa = E[aa] - mu_a * mu_a,  s_bb alike,  s_ab = E[ab] - mu_a * mu_b
 *        ssim = ((2 * (mu_a * mu_b) + C1) * (2 * s_ab + C2)) / (((mu_a * mu_a + mu_b * mu_b) + C1) * ((s_aa + s_bb) + C2))
 *      with C1 = (0.01 * 255)^2 and C2 = (0.03 * 255)^2.  n_ssim = planes * (h - 10) * (w - 10).
 *   7. Reduction: per thread in double, per workgroup a fixed-order tree, one pair of partials per workgroup into `ws`; a second
 *      launch (one workgroup of VSR_METRIC_FINISH_THREADS per frame) has thread t sum the partials t, t + threads, ... in that order
 *      and ends in the same tree.  No atomics: the four numbers of a frame are bit-identical from run to run and do not depend on
 *      the F the frame travelled in.
 *
 * Launch geometry (csrc/frame_metric.hip): one workgroup scores a tile of VSR_METRIC_STRIP_WIDTH map columns by
 * VSR_METRIC_SEGMENT_ROWS map rows; grid = (strips, segments, F).
 */
#ifndef VSR_HIP_METRIC_H
#define VSR_HIP_METRIC_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_METRIC_ABI_VERSION 1

#define VSR_METRIC_SSE 1
#define VSR_METRIC_SSIM 2

#define VSR_METRIC_RGB 0
#define VSR_METRIC_Y 1

#define VSR_METRIC_STRIP_WIDTH 64
#define VSR_METRIC_SEGMENT_ROWS 64
#define VSR_METRIC_FINISH_THREADS 64

int vsr_metric_abi_version(void);
const char* vsr_metric_last_error(void);

/* Bytes of workspace vsr_metric_frames needs for these arguments: two doubles per workgroup.  0 for arguments that call would
 * refuse.  The library never zeroes the workspace and never reads a byte of it that the same call has not written. */
size_t vsr_metric_ws_bytes(int F, int H, int W, int shave, int what);

/* Refused before any launch, each with its message: a null a / b / sums / ws, a null win11 with VSR_METRIC_SSIM set, a null luma4 in
 * VSR_METRIC_Y; `what` outside 1..3; an unknown `channels`; `quantise` other than 0 / 1; non-positive F / H / W; shave < 0 or
 * 2 * shave >= min(H, W); VSR_METRIC_SSIM with min(H, W) - 2 * shave < 11; F, H or W beyond 65535 (grid dimensions y and z; offsets
 * are 64-bit); a or b not 4-byte aligned, sums or ws not 8-byte aligned. */
int vsr_metric_frames(const float* a, const float* b, int F, int H, int W, int what, int channels, int quantise, int shave,
                      const float* luma4, const double* win11, double* sums, void* ws, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_METRIC_H */
