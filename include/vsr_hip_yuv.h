/*
 * vsr_hip_yuv.h -- C ABI of libvsr_hip_yuv.so: Y'CbCr 4:2:0 frames in and out on MI355X (gfx950).
 *
 * include/vsr_hip.h knows one pixel format either side of the path: packed 8-bit RGB (vsr_clip_ingest_u8, vsr_frame_to_u8).  This
 * header declares the 4:2:0 counterparts, in a library of its own (csrc/clip_yuv.hip alone; libvsr_hip.so and its header are
 * unchanged by it): what `ffmpeg -f rawvideo` and hardware decoders emit goes to the model's float32 RGB and back on the device.
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_yuv_last_error()` gives a
 * thread-local message).
 *
 * Frames: F frames of H x W luma samples (H, W even), packed back to back with no row padding; a frame holds 3/2 * H * W samples.
 *   VSR_YUV_420P     Y plane H x W, Cb plane H/2 x W/2, Cr plane H/2 x W/2                      uint8
 *   VSR_YUV_NV12     Y plane H x W, one H/2 x W/2 plane of interleaved (Cb, Cr)                 uint8
 *   VSR_YUV_420P10LE as VSR_YUV_420P       little-endian 16-bit words, the value in the LOW 10 bits (ingest masks with 0x3FF)
 *   VSR_YUV_P010LE   as VSR_YUV_NV12       little-endian 16-bit words, the value in the HIGH 10 bits (ingest shifts right by 6,
 *                                          write-out leaves the low 6 bits zero)
 * A frame's byte size is not a multiple of 4 in general (6 x 10 VSR_YUV_420P = 90 bytes): the kernels use wide accesses only where
 * the entry has checked that base address and width allow them, element accesses otherwise.  The 16-bit formats need an even address.
 *
 * Chroma siting: VSR_YUV_SITING_LEFT (chroma co-sited with the even luma columns, midway between two luma rows: H.264 / HEVC
 * default) or VSR_YUV_SITING_CENTER (midway in both directions: JPEG / MPEG-1).  Per axis, with c[] the chroma samples and indices
 * clamped to the plane:
 *   co-sited: luma index 2k   -> c[k]                          luma index 2k+1 -> 1/2 c[k] + 1/2 c[k+1]
 *   midway:   luma index 2k   -> 1/4 c[k-1] + 3/4 c[k]         luma index 2k+1 -> 3/4 c[k] + 1/4 c[k+1]
 * (bilinear on the chroma grid; every weight is dyadic, so the up-sampled value is exact in float32).  Write-out applies the matching
 * filter to the clamped R'G'B' values BEFORE the matrix: CENTER the mean of the 2 x 2 block, ((p00 + p01) + (p10 + p11)) / 4; LEFT per
 * row ((p[2cx-1] + p[2cx+1]) + 2 p[2cx]) / 4 with the column clamped at 0, then (row0 + row1) / 2.
 *
 * `coef12`: a HOST pointer to 12 floats, a row-major 3 x 3 matrix A followed by 3 offsets o; the entry reads them at the call and
 * hands them to the kernel by value.  The library computes no coefficient itself (driver.yuv_coefficients is their source); the
 * matrix acts on non-linear R'G'B' as the standards define, transfer functions are out of scope.
 */
#ifndef VSR_HIP_YUV_H
#define VSR_HIP_YUV_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_YUV_ABI_VERSION 1

#define VSR_YUV_420P 0
#define VSR_YUV_NV12 1
#define VSR_YUV_420P10LE 2
#define VSR_YUV_P010LE 3

#define VSR_YUV_SITING_LEFT 0
#define VSR_YUV_SITING_CENTER 1

int vsr_yuv_abi_version(void);
const char* vsr_yuv_last_error(void);

/* The 4:2:0 counterpart of vsr_clip_ingest_u8: frames [F, frame bytes] -> float32 RGB lr [F,h,w,3] and, when the pointer is not
 * null, hr [F,H,W,3].  lr is the nearest-neighbour decimation of the converted frame with ATen's index rule
 * src = min(floor(dst * (float)in / out), in - 1), as k_ingest_lr of csrc/clip_io.hip computes it; with h == H and w == W it is the
 * plain conversion.  Per output pixel, with Yc the luma code value and Cb', Cr' the up-sampled chroma values as floats (after the
 * mask / shift of the 10-bit formats):
 *   out[c] = min(max(fma(A[c][2], Cr', fma(A[c][1], Cb', fma(A[c][0], Yc, o[c]))), 0), 255)            c = 0, 1, 2
 * in exactly this order, each fma one rounding.  NaN cannot arise.
 * Refused before any launch: null pointers, an unknown fmt / siting, odd or non-positive H / W, h or w outside 1..H / 1..W, F, H
 * (so h) or W beyond 65535 (grid dimensions; the kernels index inside a frame with 32 bits), F * H * W of 2^41 or more (the grid of
 * the full-size pass), lr / hr not 16-byte aligned, a 16-bit format at an odd address. */
int vsr_yuv_ingest(const void* frames, int fmt, const float* coef12, int siting, float* lr, float* hr_or_null, int F, int H, int W,
                   int h, int w, vsr_stream_t stream);

/* float32 RGB [F,H,W,3] -> packed 4:2:0 frames [F, frame bytes].  Every value is first clamped to 0..255 (NaN -> 0, as vsr_frame_to_u8
 * does); luma per pixel, chroma from the filtered values (above), both with the forward coefficients in the same nested form:
 *   code[c] = fma(A[c][2], B, fma(A[c][1], G, fma(A[c][0], R, o[c])))                                   c = Y, Cb, Cr
 * then rintf (ties to even) and a clamp to 0..2^d - 1 (d = 8 or 10).  Every byte of the F frames is written, and nothing else.
 * Refused before any launch: null pointers, an unknown fmt / siting, odd or non-positive H / W, F, H or W beyond 65535 (grid
 * dimensions; 32-bit indices inside a frame), rgb not 16-byte aligned, a 16-bit format at an odd address. */
int vsr_yuv_write(const float* rgb, void* frames_out, int fmt, const float* coef12, int siting, int F, int H, int W,
                  vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_YUV_H */
