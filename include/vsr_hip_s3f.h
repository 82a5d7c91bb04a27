/*
 * vsr_hip_s3f.h -- C ABI of libvsr_hip_s3f.so: the fused FeedbackBlock stage of the scale-3 extension with the 1x1 chain that opens a
 * step folded into its LR load path, on MI355X (gfx950).
 *
 * include/vsr_hip_s3.h declares the plain x3 stage, include/vsr_hip_s3p.h its POST build and include/vsr_hip_s3t.h the x3 tail; this
 * header declares the stage's PRE builds, in a library of its own (csrc/sr_utd_s3f.hip + the kernel text of csrc/sr_utd_s3.h;
 * libvsr_hip.so, libvsr_hip_xcheck.so, libvsr_hip_grad.so, libvsr_hip_s3.so, libvsr_hip_s3t.so, libvsr_hip_s3p.so and their headers
 * are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * the last-error entry below gives a thread-local message).
 */
#ifndef VSR_HIP_S3F_H
#define VSR_HIP_S3F_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_S3F_ABI_VERSION 1

int vsr_s3f_abi_version(void);
const char* vsr_s3f_last_error(void);

/* Sizes the host needs to prepare a call. */
#define VSR_S3F_Q_BLOB_BYTES 0  /* bytes of the packed weight blob: stage + POST section + PRE section */
#define VSR_S3F_Q_STRIP_WIDTH 1 /* LR columns one workgroup marches down (for choosing rows_per_seg) */
size_t vsr_s3f_query(int what); /* unknown code: 0 */

/* The stage of vsr_s3_sr_utd_f16 (include/vsr_hip_s3.h: up -> tran -> down at upscale factor 3) applied to
 *   PRE3 (a, b, cmap given):   ut0(ci(feat, co(a, b, cmap)))      the chain compress_out -> compress_in -> first uptran slice
 *   PRE2 (a == b == cmap == NULL): ut0(ci(feat, feat))            the chain of step 0
 * evaluated per LR pixel in the stage's load path, exactly as the 1x1 chain launch (vsr_sr_chain1x1_f16) evaluates it: per 1x1 a
 * bias-seeded fp32 accumulator (+ cmap for co), the memory inputs in the order given (K = 32 in one MFMA per out-channel tile), then
 * the previous 1x1's activated tile, rounded to fp16, PReLU in fp16.  out receives exactly what vsr_s3_sr_utd_f16 writes for that
 * input; out_post (may be NULL: the build without POST) exactly what vsr_s3p_sr_utd_post_f16 (include/vsr_hip_s3p.h) writes.
 * feat, a, b, out, out_post: fp16 NHWC [N,h,w,32]; cmap: fp32 [h w, 32], shared by the planes.  All 16-byte aligned; no two of
 * feat, a, b, cmap, blob, out, out_post may overlap (checked on the byte ranges).  a, b, cmap: all three or none.
 * blob (VSR_S3F_Q_BLOB_BYTES bytes, 16-byte aligned): the blob of include/vsr_hip_s3p.h (VSR_S3P_Q_BLOB_BYTES bytes, byte for byte;
 *   the POST section is not read when out_post is NULL), then the PRE section: twelve A fragments [lane 64][8] fp16, fragment
 *   2 i + mt holding rows co = 16 mt + lane % 16 of matrix i,
 *     i = 0, 1: W_co over input a / b          k = col + 8 (lane / 16) + j                                  (natural channel order)
 *     i = 2:    W_ci[:, 0:32]  (feat)          k = 8 (lane / 16) + j                                         (natural)
 *     i = 3:    W_ci[:, 32:64] (chained)       k = 32 + (j < 4 ? 4 (lane / 16) + j : 16 + 4 (lane / 16) + j - 4)   (accumulator order)
 *     i = 4:    W_ut0                          k = col0 + the accumulator order of i = 3
 *     i = 5:    W_ci[:, 32:64]                 k = 32 + 8 (lane / 16) + j                                    (natural: read by PRE2)
 *   then float b_co[32], b_ci[32], b_ut0[32], slope_co, slope_ci, slope_ut0, zeros to 128 floats.  Weights are rounded fp32 -> fp16
 *   (round to nearest even), as the chain kernel rounds them at load.
 * rows_per_seg: as in include/vsr_hip_s3.h; neither it nor N changes a bit of either output.  slopes_le_one != 0 promises that the
 *   slopes of the stage, slope_post (when out_post is given) AND the three of the PRE section are <= 1 (max instead of min / select).
 * Limits: N * h * w * 64 bytes below 4 GiB per launch (split the planes), N <= 65535, ceil(h / rows_per_seg) <= 65535. */
int vsr_s3f_sr_utd_pre_f16(const void* feat, const void* a, const void* b, const void* cmap, const void* blob, void* out, void* out_post,
                           int N, int h, int w, int rows_per_seg, int slopes_le_one, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VSR_HIP_S3F_H */
