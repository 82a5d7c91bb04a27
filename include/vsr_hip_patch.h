/*
 * vsr_hip_patch.h -- C ABI of libvsr_hip_patch.so: training samples cut from frames resident on MI355X (gfx950): a run of n
 * consecutive HR frames cropped to a patch, augmented by the eight symmetries of the square and by time reversal, and the LR patch that
 * belongs to it, for all B samples of a step in one launch.
 *
 * A library of its own (csrc/train_patch.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_patch_last_error()` gives a
 * thread-local message).  No atomics anywhere.
 *
 * vsr_patch_gather
 *   src    float32 RGB [G,H,W,3], dense: the frames as the ingest entries write them at full size.
 *   table  a HOST pointer to int32 [B][4] = {t0, y0, x0, flags}, read at the call and passed to the kernel by value (B <=
 *          VSR_PATCH_MAX_B rows: 1 KB of kernel arguments).  Because the table is on the host every row is validated before the launch:
 *          an origin can never become an out-of-range read.  flags: VSR_PATCH_FLIP_X | _FLIP_Y | _TRANSPOSE | _REVERSE_TIME.
 *   hr     [B,n,Ph,Pw,3], lr [B,n,Ph/S,Pw/S,3]; at least one of the two is given.
 *
 * For sample b, frame k and output pixel (i, j) of the HR patch:
 *   1. kk = REVERSE_TIME ? n-1-k : k
 *   2. (u, v) = TRANSPOSE ? (j, i) : (i, j)
 *   3. (ch, cw) = TRANSPOSE ? (Pw, Ph) : (Ph, Pw)      the crop taken from the source; the output is always Ph x Pw
 *   4. ii = FLIP_Y ? ch-1-u : u
 *   5. jj = FLIP_X ? cw-1-v : v
 *   6. hr[b][k][i][j][c] = src[t0+kk][y0+ii][x0+jj][c]
 * The three low bits give the eight symmetries of the square.  Pure data movement: every output element is a bit copy of an input
 * element (32-bit words; NaN payloads and signed zeros survive).
 *
 * The LR patch, two modes:
 *   lr_src_or_null == NULL (nearest, the reference's decimation):
 *          lr[b][k][i][j][c] = hr[b][k][i*S][j*S][c]
 *      the decimation of the AUGMENTED patch.  This keeps the relation the model sees at inference, LR[i][j] = HR[iS][jS].  Flipping a
 *      frame that was decimated before the flip would give HR[iS+S-1][jS] instead: another pixel phase, and the network would learn a
 *      mapping shifted by S-1 HR pixels.  hr_or_null may be null in this mode: lr is read from src, not from hr.
 *   lr_src given, float32 [G,H/S,W/S,3] (frames reduced beforehand, e.g. by an antialiased bicubic filter):
 *      steps 1 to 6 on lr_src with y0/S, x0/S, ch/S, cw/S and (i, j) over Ph/S x Pw/S.  A symmetric filter commutes with the flips, so
 *      this is the reduced augmented patch.  Needs H % S == 0, W % S == 0, y0 % S == 0 and x0 % S == 0.
 *
 * The launch: one grid for all B samples, all n frames and both outputs.  A workgroup moves one tile of VSR_PATCH_TILE x VSR_PATCH_TILE
 * output pixels; the tiles of the LR patches are a second region of the same grid.  Without TRANSPOSE a tile row is read along a
 * source row and written along an output row (reversed or not), with TRANSPOSE the tile goes through LDS so that both sides still run
 * along rows.
 */
#ifndef VSR_HIP_PATCH_H
#define VSR_HIP_PATCH_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_PATCH_ABI_VERSION 1

#define VSR_PATCH_MAX_B 64
#define VSR_PATCH_TILE 32

#define VSR_PATCH_FLIP_X 1
#define VSR_PATCH_FLIP_Y 2
#define VSR_PATCH_TRANSPOSE 4
#define VSR_PATCH_REVERSE_TIME 8

int vsr_patch_abi_version(void);
const char* vsr_patch_last_error(void);

/* Refused before any launch, each with its message: a null src / table, both outputs null; non-positive G / H / W / B / n / Ph / Pw; S
 * outside 1..8; Ph % S != 0 or Pw % S != 0; B beyond VSR_PATCH_MAX_B; G, H, W, n, Ph or Pw beyond 65535; with lr_src: H % S != 0 or
 * W % S != 0; per row: t0 < 0 or t0 + n > G, a negative origin or a crop that leaves the frame (the message names the row and the
 * crop), unknown flag bits, with lr_src an origin that is no multiple of S; a pointer not 4-byte aligned; an output whose extent
 * overlaps the extent of src, of lr_src or of the other output. */
int vsr_patch_gather(const float* src, int G, int H, int W, const float* lr_src_or_null, int S, const int* table, int B, int n, int Ph,
                     int Pw, float* hr_or_null, float* lr_or_null, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_PATCH_H */
