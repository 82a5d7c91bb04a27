/*
 * vsr_hip_resize.h -- C ABI of libvsr_hip_resize.so: float32 RGB frames resampled on MI355X (gfx950) by a separable filter whose
 * coefficients the caller supplies as tables: antialiased bicubic LR frames, a bicubic baseline, or any other filter of finite support.
 *
 * A library of its own (csrc/frame_resize.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_resize_last_error()` gives a
 * thread-local message).
 *
 * Frames: `src` float32 RGB [F,H,W,3], `dst` float32 RGB [F,h,w,3], dense, in the model's 0..255 range.  Only 4-byte alignment is
 * required: 16-byte stores are taken where `dst` is 16-byte aligned and w % 4 == 0 (then every row of every frame starts on a multiple
 * of 16 bytes and an aligned group of four floats never leaves its row), element stores otherwise; the values are the same.
 *
 * Tables (DEVICE arrays, built by the caller: driver.resize_tables; the library computes no coefficient and cannot read them):
 *   x_first  int32   [w]       the first source column of output column X
 *   x_weight float32 [w][KX]   row-major: the KX weights of output column X, tap k at x_weight[X * KX + k]
 *   y_first  int32   [h]       the first source row of output row Y
 *   y_weight float32 [h][KY]   alike
 * A filter with fewer than K taps at some position pads its row with weights of 0 (a tap of weight 0 still reads its clamped pixel:
 * a NaN or an infinity there reaches the sum, as it would in any multiply-add).
 *
 * What is computed, per frame and per channel c (nothing mixes channels or frames):
 *   1. Row pass, for every source row r that some output row's taps address, and every output column X:
 *        t = 0;  for k = 0 .. KX-1, in this order:  t = fmaf(x_weight[X][k], src[r][clamp(x_first[X] + k, 0, W-1)][c], t)
 *      t is a float32 value, rounded once per fma.  The sum x_first[X] + k is the mathematical one (no wrap-around for any int32).
 *   2. Column pass, for every output pixel (Y, X):
 *        s = 0;  for k = 0 .. KY-1, in this order:  s = fmaf(y_weight[Y][k], t[clamp(y_first[Y] + k, 0, H-1)][X], s)
 *   3. quantise == 1: what an 8-bit file would hold: s = s >= 0 ? s : 0 (negatives and NaN), s = s > 255 ? 255 : s, s = rintf(s)
 *      (ties to even).  quantise == 0: s as it is (bicubic overshoots 0..255; this mode does not hide it).
 *   The index clamp is part of the contract: no table content makes a kernel read outside `src`.
 *   A pixel's result depends on its own two chains alone: not on the tile it fell in, on F, or on the launch geometry; two runs give
 *   the same bits.  (The source is compiled without floating-point contraction and asks for its fmas by name.)
 *
 * Launch geometry (csrc/frame_resize.hip): one launch does both passes.  A workgroup owns a tile of VSR_RESIZE_TILE_W output columns by
 * VSR_RESIZE_TILE_H output rows of one frame; grid = (tiles along x, tiles along y, F).  The row-filtered intermediate lives in LDS
 * and never goes to memory; there is no workspace.
 */
#ifndef VSR_HIP_RESIZE_H
#define VSR_HIP_RESIZE_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_RESIZE_ABI_VERSION 1

#define VSR_RESIZE_MAX_TAPS 33 /* antialiased bicubic down to x8: 2 * ceil(2 * 8) + 1 */
#define VSR_RESIZE_TILE_W 32
#define VSR_RESIZE_TILE_H 16

int vsr_resize_abi_version(void);
const char* vsr_resize_last_error(void);

/* Refused before any launch, each with its message: a null src / dst / table; non-positive F / H / W / h / w; H or W beyond 2^31 - 65
 * (the clamped tap index first + k is formed in 32 bits); KX or KY outside
 * 1..VSR_RESIZE_MAX_TAPS; `quantise` other than 0 / 1; F beyond 65535 (grid dimension z) or more than 65535 tiles of output rows (grid
 * dimension y: h beyond 65535 * VSR_RESIZE_TILE_H); a frame set of 2^62 bytes or more; src, dst or a table not 4-byte aligned; src
 * and dst byte ranges that overlap. */
int vsr_resize_frames(const float* src, float* dst, int F, int H, int W, int h, int w, const int* x_first, const float* x_weight, int KX,
                      const int* y_first, const float* y_weight, int KY, int quantise, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_RESIZE_H */
