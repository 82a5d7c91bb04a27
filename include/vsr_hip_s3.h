/*
 * vsr_hip_s3.h -- C ABI of libvsr_hip_s3.so: the fused FeedbackBlock stage of the scale-3 extension on MI355X (gfx950).
 *
 * include/vsr_hip.h declares the fused stage of the reference's x4 geometry and of the x2 extension; this header declares the
 * x3 one (ConvTranspose2d / Conv2d kernel 7, stride 3, padding 2), in a library of its own (csrc/sr_utd_s3.hip alone;
 * libvsr_hip.so, libvsr_hip_xcheck.so, libvsr_hip_grad.so and their headers are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * the last-error entry below gives a thread-local message).
 */
#ifndef VSR_HIP_S3_H
#define VSR_HIP_S3_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_S3_ABI_VERSION 1

int vsr_s3_abi_version(void);
const char* vsr_s3_last_error(void);

/* Sizes the host needs to prepare a call. */
#define VSR_S3_Q_BLOB_BYTES 0  /* bytes of the packed weight blob of one stage */
#define VSR_S3_Q_STRIP_WIDTH 1 /* LR columns one workgroup marches down (for choosing rows_per_seg) */
size_t vsr_s3_query(int what); /* unknown code: 0 */

/* One live chain of the FeedbackBlock at upscale factor 3, under the zero-fill semantic, in one launch:
 *   up   : ConvTranspose2d(32, 32, 7, stride 3, padding 2) + PReLU      LR [N,h,w,32] -> HR [N,3h,3w,32]
 *   tran : the chain's 32-column slice of the downtran 1x1 + PReLU, on the HR map
 *   down : Conv2d(32, 32, 7, stride 3, padding 2) + PReLU               HR -> LR [N,h,w,32]
 * in, out: fp16 NHWC, 16-byte aligned, distinct; the HR map is never written to memory.  fp16 products, fp32 accumulation.
 * blob: the stage's weights as MFMA fragments (VSR_S3_Q_BLOB_BYTES bytes, 16-byte aligned), per wave of the workgroup:
 *   wave 0 owns the HR phases (row, column) (1,1) (0,0), wave 1 (0,1) (2,1), wave 2 (1,0) (1,2), wave 3 (0,2) (2,0) (2,2);
 *   a phase x has the offsets d of {+1, 0, -1} for which k = x + 2 - 3 d lies in 0 .. 6, in that order; a wave's slots run over its
 *   phases in the order given, then the row offsets, then the column offsets (13 slots per wave, unused ones zero);
 *     [up  : wave 4][slot 13][mt 2][lane 64][8] fp16 = W_up[ci = 8 (lane / 16) + j][co = 16 mt + lane % 16][ky][kx]
 *     [down: wave 4][slot 13][mt 2][lane 64][8] fp16 = W_dn[co = 16 mt + lane % 16][ci = P(lane / 16, j)][ky][kx]
 *     [tran: mt 2][lane 64][8] fp16                  = W_dt[co = 16 mt + lane % 16][col0 + P(lane / 16, j)]
 *     float b_up[32], b_dt[32], b_dn[32], slope_up, slope_dt, slope_dn, padding to 128 floats
 *   with P(g, j) = 4 g + j for j < 4 and 16 + 4 g + (j - 4) otherwise (the accumulator-derived channel order).
 * rows_per_seg: LR rows one workgroup walks (0: all h rows); the segments recompute their halo rows, and neither this value
 *   nor N changes a bit of the output.  slopes_le_one != 0 promises that the three PReLU slopes are <= 1 (max instead of min / select).
 * Limits: N * h * w * 64 bytes below 4 GiB per launch (split the planes), N <= 65535, ceil(h / rows_per_seg) <= 65535. */
int vsr_s3_sr_utd_f16(const void* in, const void* blob, void* out, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                      vsr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VSR_HIP_S3_H */
