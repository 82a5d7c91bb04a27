/*
 * vsr_hip_pix.h -- C ABI of libvsr_hip_pix.so: planar Y'CbCr 4:2:2 and 4:4:4 frames in and out on MI355X (gfx950).
 *
 * include/vsr_hip_yuv.h declares the 4:2:0 boundary; this header declares the two layouts it leaves out, in a library of its own
 * (csrc/clip_pix.hip alone; libvsr_hip_yuv.so, its header and its ABI version are unchanged by it): what ProRes / broadcast
 * contribution feeds (4:2:2 10 bit) and screen or graded content (4:4:4) decode to goes to the model's float32 RGB and back on the
 * device.
 *
 * Conventions: those of include/vsr_hip_yuv.h (device pointers owned by the caller and used as given, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * `vsr_pix_last_error()` gives a thread-local message).
 *
 * Frames: F frames of H x W luma samples, packed back to back with no row, plane or frame padding.
 *   VSR_PIX_422P      Y plane H x W, Cb plane H x W/2, Cr plane H x W/2     uint8; W even, H any positive        2 H W samples
 *   VSR_PIX_444P      three H x W planes (Y, Cb, Cr)                        uint8; any positive H, W             3 H W samples
 *   VSR_PIX_422P10LE  as VSR_PIX_422P     little-endian 16-bit words, the value in the LOW 10 bits (ingest masks with 0x3FF)
 *   VSR_PIX_444P10LE  as VSR_PIX_444P     little-endian 16-bit words, the value in the LOW 10 bits (ingest masks with 0x3FF)
 * Neither a frame nor a plane starts on a multiple of 4 bytes in general (3 x 6 VSR_PIX_422P: planes at 0, 18, 27 of a 36-byte frame;
 * 5 x 7 VSR_PIX_444P: planes at 0, 35, 70 of a 105-byte frame): the kernels use wide accesses only where the entry has checked that
 * base address and shape put every one of them on a multiple of its width, element accesses otherwise.  The 16-bit formats need an
 * even address.
 *
 * Chroma siting, 4:2:2 (VSR_YUV_SITING_LEFT / VSR_YUV_SITING_CENTER of include/vsr_hip_yuv.h): the per-axis rule of that header on the
 * one axis that is subsampled.  There is NO vertical interpolation: row y of a chroma plane belongs to luma row y.  Horizontally,
 * with c[] the chroma samples of the row and indices clamped to 0 .. W/2 - 1:
 *   LEFT (co-sited):  luma column 2k -> c[k]                          luma column 2k+1 -> 1/2 c[k] + 1/2 c[k+1]
 *   CENTER (midway):  luma column 2k -> 1/4 c[k-1] + 3/4 c[k]         luma column 2k+1 -> 3/4 c[k] + 1/4 c[k+1]
 * (every weight is dyadic, so the up-sampled value is exact in float32).  Write-out applies the matching filter along the row to the
 * clamped R'G'B' values p[] BEFORE the matrix:
 *   LEFT:   ((p[2cx-1] + p[2cx+1]) + 2 p[2cx]) / 4, the column 2cx-1 clamped at 0          CENTER: (p[2cx] + p[2cx+1]) / 2
 * 4:4:4: Cb' and Cr' are the samples at the pixel, write-out computes chroma per pixel from the clamped values; `siting` must still
 * be one of the two known values and has no effect.
 *
 * `coef12`: a HOST pointer to 12 floats, a row-major 3 x 3 matrix A followed by 3 offsets o; the entry reads them at the call and
 * hands them to the kernel by value.  The library computes no coefficient itself (frames.pix_coefficients is their source).
 */
#ifndef VSR_HIP_PIX_H
#define VSR_HIP_PIX_H

#include "vsr_hip_yuv.h" /* VSR_OK / VSR_E_*, vsr_stream_t, VSR_YUV_SITING_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_PIX_ABI_VERSION 1

#define VSR_PIX_422P 0
#define VSR_PIX_444P 1
#define VSR_PIX_422P10LE 2
#define VSR_PIX_444P10LE 3

int vsr_pix_abi_version(void);
const char* vsr_pix_last_error(void);

/* frames [F, frame bytes] -> float32 RGB lr [F,h,w,3] and, when the pointer is not null, hr [F,H,W,3].  lr is the nearest-neighbour
 * decimation of the converted frame with ATen's index rule src = min(floor(dst * (float)in / out), in - 1), as k_yuv_lr of
 * csrc/clip_yuv.hip computes it; with h == H and w == W it is the plain conversion.  Per output pixel, with Yc the luma code value and
 * Cb', Cr' the chroma values at the pixel (above) as floats, after the mask of the 10-bit formats:
 *   out[c] = min(max(fma(A[c][2], Cr', fma(A[c][1], Cb', fma(A[c][0], Yc, o[c]))), 0), 255)            c = 0, 1, 2
 * in exactly this order, each fma one rounding.  NaN cannot arise.
 * Refused before any launch: null pointers, an unknown fmt / siting, non-positive F / H / W, an odd W for 4:2:2, h or w outside
 * 1..H / 1..W, F, H (so h) or W beyond 65535 (grid dimensions; the kernels index inside a frame with 32 bits), F * H * W of 2^41 or
 * more (the grid of the full-size pass), lr / hr not 16-byte aligned, a 16-bit format at an odd address. */
int vsr_pix_ingest(const void* frames, int fmt, const float* coef12, int siting, float* lr, float* hr_or_null, int F, int H, int W,
                   int h, int w, vsr_stream_t stream);

/* float32 RGB [F,H,W,3] -> packed frames [F, frame bytes].  Every value is first clamped to 0..255 (NaN -> 0); luma per pixel, chroma
 * per pixel (4:4:4) or from the row's filtered values (4:2:2, above), both with the forward coefficients in the same nested form:
 *   code[c] = fma(A[c][2], B, fma(A[c][1], G, fma(A[c][0], R, o[c])))                                   c = Y, Cb, Cr
 * then rintf (ties to even) and a clamp to 0..2^d - 1 (d = 8 or 10; the high 6 bits of a 16-bit word are zero).  Every byte of the
 * F frames is written once, and nothing else is.
 * Refused before any launch: null pointers, an unknown fmt / siting, non-positive F / H / W, an odd W for 4:2:2, F, H or W beyond
 * 65535, F * H * W of 2^41 or more (the grid of the 4:4:4 pass), rgb not 16-byte aligned, a 16-bit format at an odd address. */
int vsr_pix_write(const float* rgb, void* frames_out, int fmt, const float* coef12, int siting, int F, int H, int W,
                  vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_PIX_H */
