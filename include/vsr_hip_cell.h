/*
 * vsr_hip_cell.h -- C ABI of libvsr_hip_cell.so: a whole group of frames resident on MI355X (gfx950) measured in one launch, per cell of
 * VSR_CELL x VSR_CELL pixels and per frame: how much spatial detail the cell holds and how much it changed since the frame before.  The
 * clip trainer reads the small map to keep its samples off scene cuts and off flat patches.
 *
 * A library of its own (csrc/clip_cell_stats.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip_scene.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_cell_last_error()` gives a
 * thread-local message).  No atomics anywhere.
 *
 * vsr_cell_stats
 *   frames  float32 RGB [G,H,W,3], dense, in the model's 0..255 range: the trainer's resident group.
 *   luma4   a HOST pointer to four float32 {a0, a1, a2, o}, read at the call and passed by value (the library computes no coefficient).
 *   stats   int32 [G,Ch,Cw,2], Ch = ceil(H / VSR_CELL), Cw = ceil(W / VSR_CELL); every element is written.
 *
 * Per pixel and frame, q is the 8-bit luma code of include/vsr_hip_scene.h, steps 1 to 4: every operation in double and rounded once (no
 * contraction):
 *   1. y = ((o + a0 * R) + a1 * G) + a2 * B
 *   2. q = y >= 0 ? y : 0       (negatives and NaN)
 *   3. q = q > 255 ? 255 : q
 *   4. q = rint(q)              (ties to even)
 * Per frame g and cell (i, j), over the pixels (y, x) of the frame with y / VSR_CELL == i and x / VSR_CELL == j (the cells of the last row
 * and column of cells hold the pixels that exist):
 *   5. activity      stats[g][i][j][0] = the sum of (x + 1 < W ? |q[y][x] - q[y][x+1]| : 0) + (y + 1 < H ? |q[y][x] - q[y+1][x]| : 0)
 *      The neighbour may lie in the next cell; it never lies outside the frame.
 *   6. temporal SAD  stats[g][i][j][1] = the sum of |q_g[y][x] - q_{g-1}[y][x]| for g > 0, and 0 for g = 0.
 * Every value is an integer of at most VSR_CELL * VSR_CELL * 2 * 255 = 130560, summed in int32: exact, and independent of the order, of
 * G (frame g's activity is the same as row g of a longer group and as a group of one) and of which load path ran.  The sum of channel 1
 * over the cells of frame g is the `sad` vsr_scene_pair_sums gives for the pair (g - 1, g).
 *
 * The launch: one kernel, no finish pass.  A workgroup owns a tile of VSR_CELL_TILE_H x VSR_CELL_TILE_W pixels (one cell down, four
 * across) and walks g = 0 .. G-1 for it: a thread keeps the codes of its four pixels of frame g - 1 in registers, so each frame is read
 * once; the only extra reads are the row below the tile and the column right of it, the neighbours of the spatial term.  A cell's sum is
 * completed inside the workgroup.  16-byte loads where `frames` is 16-byte aligned and W % 4 == 0 (then every row of every frame starts on
 * a multiple of 16 bytes and an aligned group of four pixels never leaves its row), element loads otherwise; both give the same bits.
 * Offsets are 64-bit.
 */
#ifndef VSR_HIP_CELL_H
#define VSR_HIP_CELL_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_CELL_ABI_VERSION 1

#define VSR_CELL 16
#define VSR_CELL_TILE_H 16
#define VSR_CELL_TILE_W 64
#define VSR_CELL_MAX_G 65535

int vsr_cell_abi_version(void);
const char* vsr_cell_last_error(void);

/* Refused before any launch, each with its message: a null frames / stats / luma4; non-positive G / H / W; H or W beyond 65535 (the grid
 * is tiles across x tiles down); G beyond VSR_CELL_MAX_G (the grid does not depend on G: a workgroup walks the frames; the bound is the
 * one vsr_scene_pair_sums puts on its P); frames or stats not 4-byte aligned. */
int vsr_cell_stats(const float* frames, int G, int H, int W, const float* luma4, int* stats, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_CELL_H */
