/*
 * vsr_hip_warp.h -- C ABI of libvsr_hip_warp.so: the temporal warping error of consecutive HR frames on MI355X (gfx950): frame t + 1
 * warped back onto frame t along an optical flow and the squared difference summed over the pixels that are not occluded (Lai et al.,
 * "Learning Blind Video Temporal Consistency", ECCV 2018; the occlusion rule is Ruder, Dosovitskiy, Brox 2016), per frame pair, in float64.
 *
 * A library of its own (csrc/frame_warp_error.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_warp_last_error()` gives a
 * thread-local message).
 *
 * Frames: `frames_a`, `frames_b` float32 RGB [P,H,W,3], dense, in the model's 0..255 range; pair p is a[p], the frame at time t,
 * against b[p], the frame at time t + 1.  Only 4-byte alignment is required: every load is an element load (a pixel's neighbours in
 * the 2 x 2 gathers come from L1 / L2), so the values do not depend on the alignment of a base or on the row pitch.
 *
 * Flows: a forward flow a -> b and a backward flow b -> a over the crop rectangle (y0, x0, h, w) of the frames (FlowNet2 sees the
 * StaticCenterCrop of a frame to multiples of 64; the library takes any rectangle inside the frame).  Channel 0 is the displacement
 * along x and channel 1 along y, in pixels.  Both flows are addressed alike, so that either producer is read in place: element
 * (p, c, y, x) lies at base + p * pair_stride + c * chan_stride + (y * w + x) * pix_stride, counted in elements of `flow_type`
 * (VSR_WARP_FLOW_F32: float, VSR_WARP_FLOW_F16: IEEE half; the row stride is w * pix_stride).  Planar float32 [P,2,h,w]: pair_stride
 * 2 h w, chan_stride h w, pix_stride 1.  The fp16 executor's NHWC map [P,h,w,ld] with the flow in channels 0 and 1: pair_stride
 * h w ld, chan_stride 1, pix_stride ld.  Half to double is exact: the two forms give the same bits for the same values.
 *
 * Result: `sums`, device double [P][4] = {sse, n_terms, n_valid, n_pixels} per pair, with n_terms = planes * n_valid and
 * n_pixels = (h - 2 shave) * (w - 2 shave).  The host forms E_warp = sse / n_terms / 255^2; the library does not (n_valid = 0 is a
 * legitimate result).
 *
 * What is computed.  `channels`, `quantise`, `shave` and `luma4` are the switches of vsr_metric_frames (include/vsr_hip_metric.h):
 * quantise 1 takes every frame value first to what write-out stores (v = v >= 0 ? v : 0, v = v > 255 ? 255 : v, v = rintf(v)); the
 * shave is counted inside the crop: the scored pixels are shave <= x < w - shave, shave <= y < h - shave in crop coordinates, while
 * samples may fall anywhere in the crop; VSR_WARP_Y scores one plane, the luma ((o + a0 * R) + a1 * G) + a2 * B in double from the four
 * float32 values of the HOST pointer luma4 = {a0, a1, a2, o}; VSR_WARP_RGB scores three.  `occ` is a HOST pointer to four doubles
 * {c1, c2, g1, g2}, read at the call and passed by value (Ruder et al.: {0.01, 0.5, 0.01, 0.002}).  Per scored pixel (x, y), everything in
 * double, every operation rounded once, nothing contracted:
 *   1. u, v: the forward flow at (x, y).  xf = x + u, yf = y + v.
 *   2. in frame:  xf >= 0 && xf <= w - 1 && yf >= 0 && yf <= h - 1  (false for NaN).  A pixel that is not in frame is not valid, and
 *      nothing else is evaluated for it.
 *   3. xa = floor(xf), ax = xf - xa, xb = min(xa + 1, w - 1); ya, ay, yb alike.  The bilinear value of a quantity q at the sample:
 *        r0 = (1 - ax) * q[ya][xa] + ax * q[ya][xb],  r1 alike on row yb,  r = (1 - ay) * r0 + ay * r1
 *      (the two weights 1 - ax and 1 - ay are formed once; each product and each sum is rounded).
 *   4. bu, bv: the backward flow sampled bilinearly at (xf, yf).
 *      consistent:  (u + bu)^2 + (v + bv)^2 <= c1 * ((u^2 + v^2) + (bu^2 + bv^2)) + c2.
 *   5. smooth (not a motion boundary): one-sided differences of the forward flow to the right and downward, the neighbour index
 *      clamped at the last column and row of the crop: dux = u(min(x + 1, w - 1), y) - u, duy = u(x, min(y + 1, h - 1)) - u, dvx, dvy alike;
 *        (dux^2 + duy^2) + (dvx^2 + dvy^2) <= g1 * (u^2 + v^2) + g2.
 *   6. valid = in frame && consistent && smooth.
 *   7. planes: per SOURCE pixel first the quantisation (when on), then for VSR_WARP_Y the luma; the interpolation comes after.
 *        d = planeA(x0 + x, y0 + y) - bilinear(planeB at the sample, inside the crop);  term d * d, summed over the planes of valid pixels.
 *   8. Reduction: per thread in double (its pixels top to bottom, a pixel's planes in order), per workgroup a fixed-order tree, one pair
 *      of partials {sse, n_valid} per workgroup into `ws`; a second launch (one workgroup of VSR_WARP_FINISH_THREADS per pair) has
 *      thread t sum the partials t, t + threads, ... in that order and ends in the same tree.  No atomics: the four numbers of a pair
 *      are bit-identical from run to run and do not depend on the P the pair travelled in.
 *
 * Launch geometry (csrc/frame_warp_error.hip): one thread per pixel and row, lanes along x; a workgroup scores a tile of
 * VSR_WARP_TILE_W columns by VSR_WARP_TILE_H rows of the scored region; grid = (tiles along x, tiles along y, P).
 */
#ifndef VSR_HIP_WARP_H
#define VSR_HIP_WARP_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_WARP_ABI_VERSION 1

#define VSR_WARP_RGB 0
#define VSR_WARP_Y 1

#define VSR_WARP_FLOW_F32 0
#define VSR_WARP_FLOW_F16 1

#define VSR_WARP_TILE_W 64
#define VSR_WARP_TILE_H 16
#define VSR_WARP_FINISH_THREADS 256

int vsr_warp_abi_version(void);
const char* vsr_warp_last_error(void);

/* Bytes of workspace vsr_warp_error needs for these arguments: two doubles per workgroup.  0 for arguments that call would refuse.
 * The library never zeroes the workspace and never reads a byte of it that the same call has not written. */
size_t vsr_warp_ws_bytes(int P, int h, int w, int shave);

/* Refused before any launch, each with its message: a null frames_a / frames_b / flow_fwd / flow_bwd / sums / ws; a null occ; a null
 * luma4 in VSR_WARP_Y; an unknown `flow_type` or `channels`; `quantise` other than 0 / 1; non-positive P / H / W / h / w; a crop outside
 * the frame (y0 < 0, x0 < 0, y0 + h > H or x0 + w > W); shave < 0 or 2 * shave >= min(h, w); P, H or W beyond 65535 (grid dimensions y
 * and z; offsets are 64-bit); pair_stride < 0, chan_stride < 1 or pix_stride < 1; frames not 4-byte aligned, flows not aligned to their
 * element, sums or ws not 8-byte aligned. */
int vsr_warp_error(const float* frames_a, const float* frames_b, int P, int H, int W, int y0, int x0, int h, int w,
                   const void* flow_fwd, const void* flow_bwd, int flow_type, long long pair_stride, long long chan_stride,
                   long long pix_stride, int channels, int quantise, int shave, const float* luma4, const double* occ, double* sums,
                   void* ws, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_WARP_H */
