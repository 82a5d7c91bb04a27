/*
 * vsr_hip_loss.h -- C ABI of libvsr_hip_loss.so: the pixel terms of the training loss on MI355X (gfx950): the object masking
 * (loss_function.py:87-101), the six image MSEs and the total-variation sums of `VSR.loss_calculate`'s six SR_loss calls
 * (loss_function.py:9-48, video_super_resolution.py:71-80), and the VGG inputs as NHWC-4 half frames, in one launch plus a finish.
 *
 * A library of its own (csrc/loss_terms.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip_metric.h (device pointers owned by the caller, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * `vsr_loss_last_error()` gives a thread-local message).
 *
 * Frames: `outputs` float32 [3,H,W,3] = O0, O1, O2 (high_frames), `target` float32 [H,W,3] = T, dense.  N = 3 H W elements per frame;
 * element e = (y W + x) 3 + c.  `mask`: N bytes, nonzero = masked.
 *
 * What is computed:
 *   1. Mask.  The reference hands numpy a [3,H,W] mask for [H,W,3] data, and numpy reshapes it: flat element e of a frame is masked by
 *      flat element e of the mask.  The kernel reads mask[e] for element e of every frame, never "per pixel".
 *   2. Masking rule.  m(v) = mask[e] ? 0 : (float)((int)v & 255): truncation toward zero, then the low eight bits (255.9 -> 255,
 *      256.5 -> 0, 300.2 -> 44, -0.5 -> 0, -3.7 -> 253); a masked or zero result is +0.  For every finite |v| < 2^31 this is numpy's
 *      `np.array(v, dtype=np.uint8)` with the masked entries filled with 0.  Outside that range the convert saturates and no equality
 *      with numpy is claimed: v >= 2^31 -> 2^31 - 1 -> 255, v <= -2^31 -> -2^31 -> 0, NaN -> 0.
 *      mO0, mO1, mO2, mT = m applied to O0, O1, O2, T.
 *   3. SSE, six sums over the N elements: (O0,T), (mO1,mT), (O0,O1), (O1,O2), (mO0,mO1), (mO1,mO2).  Each term is
 *      d = (double)a - (double)b, d * d rounded once, summed in double.
 *   4. TV, for each of O0, O1, mO0, mO1 two sums: h over a[y+1,x,c] - a[y,x,c] for y < H-1, w over a[y,x+1,c] - a[y,x,c] for
 *      x < W-1; differences and squares in double as for SSE.
 *   5. `sums`, device double [14] = {sse[6], h(O0), w(O0), h(O1), w(O1), h(mO0), w(mO0), h(mO1), w(mO1)}.
 *   6. `terms`, device float [6][2] = {image, tv} of the six SR_loss calls in loss_calculate's order: genSR (O0,T), objSR (mO1,mT),
 *      flow (O0,O1), flow (O1,O2), objflow (mO0,mO1), objflow (mO1,mO2).  image = sse / (3 H W); tv, of the call's FIRST frame
 *      (O0, mO1, O0, O1, mO0, mO1), = 2 * (h / (3 (H-1) W) + w / (3 H (W-1))).  Both formed in double, operation by operation, and
 *      rounded once to float32.
 *   7. `masked` (may be null), device float [4,H,W,3] = mO0, mO1, mO2, mT.
 *   8. `nhwc4` (may be null), device half [8,H,W,4] = O0, O1, O2, T, mO0, mO1, mO2, mT: every float rounded to half (ties to even,
 *      overflow to infinity), channel 3 = 0: bit for bit the NHWC-4 half frame the fp16 VGG executor makes of the same frame.
 *   9. Reduction: as include/vsr_hip_metric.h section 7: per thread in double, a fixed-order tree per workgroup (a butterfly inside
 *      each wave, then the waves in order), 14 partials per workgroup into `ws`; a finish launch (one workgroup of
 *      VSR_LOSS_FINISH_THREADS) has thread t sum the partials t, t + threads, ... in that order and ends in a fixed-order tree.  No
 *      atomics: every number is bit-identical from run to run.
 *
 * Loads: 16-byte loads and stores where outputs, target, masked and nhwc4 are 16-byte aligned, mask is 4-byte aligned and W % 4 == 0
 * (then every row starts on a multiple of 16 bytes); element loads and stores otherwise; the values are the same.
 *
 * Launch geometry (csrc/loss_terms.hip): one workgroup marches down VSR_LOSS_SEGMENT_ROWS rows of a strip of VSR_LOSS_STRIP_FLOATS
 * floats (a whole number of pixels and of 16-byte groups) of all four frames, the previous row in registers; grid = (strips, segments).
 * An input element comes from memory once, plus one halo row per segment and three halo floats per strip row.
 */
#ifndef VSR_HIP_LOSS_H
#define VSR_HIP_LOSS_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_LOSS_ABI_VERSION 1

#define VSR_LOSS_STRIP_FLOATS 768
#define VSR_LOSS_SEGMENT_ROWS 32
#define VSR_LOSS_FINISH_THREADS 256
#define VSR_LOSS_NSUMS 14
#define VSR_LOSS_MAX_DIM 65535

int vsr_loss_abi_version(void);
const char* vsr_loss_last_error(void);

/* Bytes of workspace vsr_loss_pixel_terms needs: VSR_LOSS_NSUMS doubles per workgroup.  0 for sizes that call would refuse.  The
 * library never zeroes the workspace and never reads a byte of it that the same call has not written. */
size_t vsr_loss_ws_bytes(int H, int W);

/* Refused before any launch, each with its message: a null outputs / target / mask / sums / terms / ws (`masked` and `nhwc4` may be
 * null); H or W below 2 (the reference divides by zero there); H or W beyond VSR_LOSS_MAX_DIM (grid dimension y; offsets are 64-bit);
 * outputs / target / masked / terms not 4-byte aligned, nhwc4 not 2-byte aligned, sums or ws not 8-byte aligned; an output range
 * (masked, nhwc4, sums, terms, ws) that overlaps an input range (outputs, target, mask). */
int vsr_loss_pixel_terms(const float* outputs, const float* target, const unsigned char* mask, int H, int W, float* masked, void* nhwc4,
                         double* sums, float* terms, void* ws, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_LOSS_H */
