/*
 * vsr_hip_s3p.h -- C ABI of libvsr_hip_s3p.so: the fused FeedbackBlock stage of the scale-3 extension with the next group's uptran
 * slice applied inside the launch, on MI355X (gfx950).
 *
 * include/vsr_hip_s3.h declares the plain x3 stage and include/vsr_hip_s3t.h the x3 tail; this header declares the stage's POST
 * build, in a library of its own (csrc/sr_utd_s3p.hip + the kernel text of csrc/sr_utd_s3.h; libvsr_hip.so, libvsr_hip_xcheck.so,
 * libvsr_hip_grad.so, libvsr_hip_s3.so, libvsr_hip_s3t.so and their headers are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * the last-error entry below gives a thread-local message).
 */
#ifndef VSR_HIP_S3P_H
#define VSR_HIP_S3P_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_S3P_ABI_VERSION 1

int vsr_s3p_abi_version(void);
const char* vsr_s3p_last_error(void);

/* Sizes the host needs to prepare a call. */
#define VSR_S3P_Q_BLOB_BYTES 0  /* bytes of the packed weight blob of one stage with its POST section */
#define VSR_S3P_Q_STRIP_WIDTH 1 /* LR columns one workgroup marches down (for choosing rows_per_seg) */
size_t vsr_s3p_query(int what); /* unknown code: 0 */

/* The stage of vsr_s3_sr_utd_f16 (include/vsr_hip_s3.h: up -> tran -> down at upscale factor 3) and, in the same launch,
 *   post : the NEXT group's uptran slice, a 1x1 (32 -> 32) + PReLU on the stage's fp16 output     LR [N,h,w,32] -> LR [N,h,w,32]
 * out receives exactly what vsr_s3_sr_utd_f16 writes, out_post exactly what the 1x1 chain launch (vsr_sr_chain1x1_f16, one stage, one
 * input) computes from it: bias-seeded fp32 accumulator, K = 32 in one MFMA, rounded to fp16, PReLU in fp16.
 * in, out, out_post: fp16 NHWC, 16-byte aligned, no two of them overlapping (checked on the byte ranges).
 * blob (VSR_S3P_Q_BLOB_BYTES bytes, 16-byte aligned): the blob of include/vsr_hip_s3.h (VSR_S3_Q_BLOB_BYTES bytes, byte for byte), then
 *     [post: mt 2][lane 64][8] fp16 = W_post[co = 16 mt + lane % 16][col0 + 8 (lane / 16) + j]      (natural channel order)
 *     float b_post[32], slope_post, zeros to 64 floats
 * rows_per_seg: as in include/vsr_hip_s3.h; neither it nor N changes a bit of either output.  slopes_le_one != 0 promises that the
 *   three slopes of the stage AND slope_post are <= 1 (max instead of min / select).
 * Limits: N * h * w * 64 bytes below 4 GiB per launch (split the planes), N <= 65535, ceil(h / rows_per_seg) <= 65535. */
int vsr_s3p_sr_utd_post_f16(const void* in, const void* blob, void* out, void* out_post, int N, int h, int w, int rows_per_seg,
                            int slopes_le_one, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VSR_HIP_S3P_H */
