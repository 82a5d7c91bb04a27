/*
 * vsr_hip_deint.h -- C ABI of libvsr_hip_deint.so: motion-adaptive deinterlacing of packed Y'CbCr frames on MI355X (gfx950).
 *
 * An interlaced frame holds two fields, the even rows and the odd rows, taken at two instants.  This library turns such a frame into a
 * progressive one BEFORE the conversion to RGB (include/vsr_hip_yuv.h, include/vsr_hip_pix.h): the rows of one field are kept as they
 * are, the rows of the other parity are rebuilt from the kept field and from the fields either side in time.  It is a library of its own
 * (csrc/clip_deint.hip alone; no other library, header or ABI version is changed by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller and used as given, kernels enqueued on `stream`, no
 * synchronisation / allocation / free, graph-capturable, no atomics; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * `vsr_deint_last_error()` gives a thread-local message).
 *
 * The library knows no pixel format.  A frame is a run of bytes at a base address and up to VSR_DEINT_MAX_PLANES planes inside it; a
 * plane is `rows` dense rows of `cols * comps` samples starting `offset` BYTES after the base (comps = 2: the interleaved CbCr plane of
 * nv12 / p010le; a sample only ever meets samples of its own column and component, so the kernel sees a row of cols * comps samples).
 * A sample is one byte or one little-endian 16-bit word; the value is s = word >> shift (shift = 6: p010le, the value in the high
 * 10 bits).  frames.deint_planes gives the planes of every layout of frames.PIX_FORMATS.
 *
 * THE RULE (this project's own, in the manner of yadif, without yadif's edge directions and without its vertical-consistency
 * refinement; not validated on real video).  Integer arithmetic in int32, `>>` arithmetic.  P, C, N: the same plane of `prev`, `cur`
 * and `next`, as values s.
 *
 *   rows y with y % 2 == keep:      out[y] is a BIT COPY of cur[y] (with shift = 6 the low 6 bits travel too)
 *   every other row y, sample x:
 *     1. yu = y - 1, yd = y + 1;  if yu < 0 then yu = yd;  if yd >= rows then yd = yu          (rows >= 2: one of the two at most)
 *     2. c = C[yu][x], e = C[yd][x]                                                            the kept field, above and below
 *     3. (B, A) = kept_first ? (P, C) : (C, N);  b = B[y][x], a = A[y][x]                      the two fields of the missing parity that
 *                                                                                              lie next to the kept field in time
 *     4. t = (b + a) >> 1,  sp = (c + e) >> 1                                                  temporal and spatial estimate
 *     5. td0 = |b - a|
 *     6. td1 = (|P[yu][x] - c| + |P[yd][x] - e|) >> 1,  td2 = (|N[yu][x] - c| + |N[yd][x] - e|) >> 1
 *     7. d = max(td0 >> 1, td1, td2)
 *     8. v = min(max(sp, t - d), t + d);  the output word is v << shift                        (low bits 0 with shift = 6)
 *
 * What follows from it:
 *   - where P == C == N: b = a = t, td0 = td1 = td2 = d = 0, v = t = C[y][x]: out == cur bit for bit when shift = 0 (weave: static
 *     content keeps its full vertical resolution); with shift = 6 the rebuilt rows lose cur's low 6 bits, nothing else;
 *   - v lies between sp and t (d >= 0, and v is sp clamped to t - d .. t + d), both of which are means of two input values: v stays in
 *     the range of the inputs for any 16-bit words, nothing overflows int32 and there is no clamp constant;
 *   - an output sample depends on at most 9 input samples of its own column and component (C at yu, yd; B, A at y; P and N at yu,
 *     yd; one of B, A is C at y), so the result does not depend on the tiling or on which load path ran.
 *
 * Aliasing: `prev`, `cur` and `next` may be one another (callers pass the same frame twice at the ends of a clip); `out` must not
 * overlap any of the three (the entry refuses an `out` EQUAL to one of them; any other overlap is the caller's to avoid).
 *
 * The launch: one kernel for all planes of the frame.  A workgroup covers VSR_DEINT_TILE_ROWS rows by VSR_DEINT_TILE_BYTES bytes of one
 * plane; a thread takes 16 bytes of one rebuilt row together with the kept row of the same pair.  A plane is moved with 16-byte
 * accesses where the four bases plus its offset and its row pitch are all multiples of 16, sample by sample otherwise (3 x 6 4:2:2 has
 * planes at bytes 18 and 27, 5 x 7 4:4:4 at 35 and 70; a row of 1030 bytes), both with the same bits; exactly the planes' bytes of
 * `out` are written, each once, and nothing else is.
 */
#ifndef VSR_HIP_DEINT_H
#define VSR_HIP_DEINT_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_DEINT_ABI_VERSION 1
#define VSR_DEINT_MAX_PLANES 3
#define VSR_DEINT_TILE_ROWS 8      /* rows of a plane one workgroup covers (4 pairs of a kept and a rebuilt row) */
#define VSR_DEINT_TILE_BYTES 1024  /* bytes of a row one workgroup covers (64 threads x 16 bytes) */

int vsr_deint_abi_version(void);
const char* vsr_deint_last_error(void);

/* offset in BYTES from the frame's base; a row is cols * comps samples, rows dense */
typedef struct {
    size_t offset;
    int rows, cols, comps;
} vsr_deint_plane;

/* One packed frame deinterlaced into `out` by the rule above, all `n_planes` planes in one launch.  `planes`: a HOST pointer, read at
 * the call and handed to the kernel by value.  `sample_bytes`: 1 | 2 (little endian); `shift`: 0, or 6 for p010le; `keep`: the parity of
 * the rows kept (0: even rows, the top field); `kept_first`: 1 when the kept field is the first of `cur`'s two in time, 0 when it is the
 * second.
 * Refused before any launch, each with its own message: a null pointer; n_planes outside 1..VSR_DEINT_MAX_PLANES; a plane of fewer than
 * 2 rows; non-positive cols or comps; comps > 2; sample_bytes not 1 or 2; shift not 0 or 6; shift = 6 with sample_bytes = 1; keep or
 * kept_first not 0 or 1; a base or a plane offset that is odd when sample_bytes = 2; rows beyond 65535 * VSR_DEINT_TILE_ROWS, a row
 * beyond 2^30 samples or 2^31 workgroups and more in all (the grid); `out` equal to an input. */
int vsr_deint_frame(const void* prev, const void* cur, const void* next, void* out, const vsr_deint_plane* planes, int n_planes,
                    int sample_bytes, int shift, int keep, int kept_first, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_DEINT_H */
