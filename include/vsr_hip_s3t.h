/*
 * vsr_hip_s3t.h -- C ABI of libvsr_hip_s3t.so: the one-launch tail of the SR net for the scale-3 extension on MI355X (gfx950).
 *
 * include/vsr_hip.h declares the fused tails of the reference's x4 geometry and of the x2 extension, include/vsr_hip_s3.h the
 * fused FeedbackBlock stage of the x3 one; this header declares the x3 tail (ConvTranspose2d kernel 7, stride 3, padding 2 +
 * PReLU, then conv_out 3x3), in a library of its own (csrc/sr_tail_s3.hip alone; libvsr_hip.so, libvsr_hip_xcheck.so,
 * libvsr_hip_grad.so, libvsr_hip_s3.so and their headers are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * the last-error entry below gives a thread-local message).
 */
#ifndef VSR_HIP_S3T_H
#define VSR_HIP_S3T_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_S3T_ABI_VERSION 1

int vsr_s3t_abi_version(void);
const char* vsr_s3t_last_error(void);

/* Sizes the host needs to prepare a call. */
#define VSR_S3T_Q_BLOB_BYTES 0      /* bytes of the packed weight blob without the folded compress_out */
#define VSR_S3T_Q_BLOB_FOLD_BYTES 1 /* ... with it (what the fold entry reads) */
#define VSR_S3T_Q_STRIP_WIDTH 2     /* LR columns one workgroup marches down (for choosing rows_per_seg) */
size_t vsr_s3t_query(int what);     /* unknown code: 0 */

/* The tail of the SR net at upscale factor 3 in one launch:
 *   out      : ConvTranspose2d(32, 32, 7, stride 3, padding 2) + bias + PReLU   LR [N,h,w,32] -> HR [N,3h,3w,32], rounded to fp16
 *   conv_out : Conv2d(32, 3, 3, padding 1) + bias, no activation                HR -> raw [N,3,3h,3w] float32
 * in: fp16 NHWC, 16-byte aligned; raw: float32 planes, 4-byte aligned, not overlapping any input; the HR map is never written to
 * memory.  fp16 products, fp32 accumulation.  decimate != 0: only the pixels (3i, 3j) leave -> raw [N,3,h,w], with exactly the
 * values the full frame has there.
 * blob: the weights as MFMA fragments (16-byte aligned), per wave of the workgroup:
 *   wave 0 owns the HR phases (row, column) (1,1) (0,0), wave 1 (0,1) (2,1), wave 2 (1,0) (1,2), wave 3 (0,2) (2,0) (2,2);
 *   a phase x has the offsets d of {+1, 0, -1} for which k = x + 2 - 3 d lies in 0 .. 6, in that order; a wave's slots run over its
 *   phases in the order given, then the row offsets, then the column offsets (13 slots per wave, unused ones zero) -- the `up` half
 *   of the stage's blob (include/vsr_hip_s3.h);
 *     [out     : wave 4][slot 13][mt 2][lane 64][8] fp16 = W_out[ci = 8 (lane / 16) + j][co = 16 mt + lane % 16][ky][kx]
 *     [conv_out: dy 3][dx 3][lane 64][8] fp16            = W_cv[co = lane % 16][ci = P(lane / 16, j)][dy][dx] for lane % 16 < 3, else 0
 *     float b_out[32], b_cv[3], zeros to [96], slope_out at [96], zeros to 128 floats          (VSR_S3T_Q_BLOB_BYTES end here)
 *     [compress_out: map 2][mt 2][lane 64][8] fp16       = W_co[co = 16 mt + lane % 16][col_map + 8 (lane / 16) + j]
 *     float b_co[32], slope_co, zeros to 64 floats                                              (VSR_S3T_Q_BLOB_FOLD_BYTES end here)
 *   with P(g, j) = 4 g + j for j < 4 and 16 + 4 g + (j - 4) otherwise (the accumulator-derived channel order of the HR ring).
 * rows_per_seg: LR rows one workgroup walks (0: all h rows); the segments recompute their halo rows, and neither this value,
 *   nor N, nor the strip a pixel falls in changes a bit of the output.  slopes_le_one != 0 promises slope_out <= 1 (max instead
 *   of min / select); the folded slope is looked at by the kernel either way.
 * Limits: N * h * w * 64 bytes below 4 GiB per launch (split the planes), N <= 65535, ceil(h / rows_per_seg) <= 65535. */
int vsr_s3t_sr_tail_f16(const void* in, const void* blob, float* raw, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                        int decimate, vsr_stream_t stream);

/* The same with the FeedbackBlock's last compress_out applied in the kernel's LR load path:
 *   in = PReLU(W_co[:, col_a ..] lr3 + W_co[:, col_b ..] lr6 + b_co + cmap), rounded to fp16 before and after the PReLU
 * lr3, lr6: fp16 NHWC [N,h,w,32]; cmap: float32 [h,w,32] (the constant map, shared by the planes), all 16-byte aligned.  The sums
 * run in the order of the 1x1 chain kernel (bias + map, then the two products), so the result equals that launch followed by
 * vsr_s3t_sr_tail_f16 bit for bit.  blob: VSR_S3T_Q_BLOB_FOLD_BYTES bytes.  Additional limit: h * w * 128 bytes below 4 GiB. */
int vsr_s3t_sr_tail_fold_f16(const void* lr3, const void* lr6, const float* cmap, const void* blob, float* raw, int N, int h, int w,
                             int rows_per_seg, int slopes_le_one, int decimate, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VSR_HIP_S3T_H */
