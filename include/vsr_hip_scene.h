/*
 * vsr_hip_scene.h -- C ABI of libvsr_hip_scene.so: scene cuts in a streamed clip, found and handled on MI355X (gfx950): the mean
 * absolute luma difference of consecutive LR frames, the cut rule on it, and the 3-frame window and fed-back estimate composed under
 * the rule's flags.  The decision is taken and acted upon on the device: the host never reads a flag to issue the next launch.
 *
 * A library of its own (csrc/clip_scene.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_scene_last_error()` gives a
 * thread-local message).  No atomics anywhere.
 *
 * Frames: float32 RGB [h,w,3], dense, in the model's 0..255 range, exactly as the LR ring of ClipRunner holds them.  Only 4-byte
 * alignment is required.  vsr_scene_pair_sums takes 16-byte loads where both bases are 16-byte aligned and h * w % 4 == 0 (then every
 * frame starts on a multiple of 16 bytes and an aligned group of four pixels never leaves the buffer), element loads otherwise; the
 * values are the same (the sums are integers below 2^53: exact in any order).
 *
 * vsr_scene_pair_sums: per pair p = (a[p], b[p]) the sums {sad, n}, device double [P][2].  Per pixel and frame, every operation in
 * double and rounded once (no contraction), from the four float32 values of the HOST pointer luma4 = {a0, a1, a2, o}, read at the call
 * and passed by value (the library computes no coefficient):
 *   1. y = ((o + a0 * R) + a1 * G) + a2 * B
 *   2. q = y >= 0 ? y : 0       (negatives and NaN)
 *   3. q = q > 255 ? 255 : q
 *   4. q = rint(q)              (ties to even): the 8-bit luma code
 *   5. term |q_a - q_b|;  sad = the sum of the terms over the h * w pixels;  n = h * w.
 *   6. Reduction: per thread in double, per workgroup (VSR_SCENE_WG_PIXELS pixels) a fixed-order tree, one partial per workgroup into
 *      `ws`; a second launch (one workgroup of VSR_SCENE_FINISH_THREADS per pair) has thread t sum the partials t, t + threads, ... in
 *      that order and ends in the same tree.  Both numbers are integers below 2^53, so they are exact and do not depend on the order,
 *      on the P the pair travelled in or on which load path ran.
 *
 * vsr_scene_decide: flags, device int32 [P], from rows of `sums` alone (one launch decides all P; no order between threads):
 *   1. m_p = sad_p / n_p                        (one double division)
 *   2. m_prev = m_{p-1} for p > 0; for p = 0: prev[0] / prev[1] where `prev_or_null` (device {sad, n} of the pair before) is given, else 0
 *   3. flag_p = (m_p >= t_abs) && (m_p >= ratio * m_prev) ? 1 : 0       (the product rounded once; false where m_p is NaN)
 *
 * vsr_scene_window: the window x3 [3,h,w,3] and the fed-back estimate est [1,h,w,3] under two device flags (int32; a null flag
 * pointer means 0; a flag is set where the word is not 0):
 *   x3[0] = flag_ab ? b : a,   x3[1] = b,   x3[2] = flag_bc ? b : c
 *   est   = flag_ab ? b : prev_est[y * S, x * S]      prev_est [1,H,W,3], H = S h, W = S w
 * (the nearest resize vsr_resize_estimate_f32 performs for an integer factor).  est_or_null and prev_est_or_null are both given or both
 * null (both null: the first window of a run; H and W are then ignored).  Pure data movement: every output element is a bit copy of an
 * input element (32-bit words; NaN payloads survive).  The outputs must not overlap the inputs.
 *
 * Why the rule has this form: the mean absolute luma difference is what ffmpeg's scene score and PySceneDetect's content detector both
 * rest on; the ratio against the previous pair keeps sustained fast motion from being read as a run of cuts.  Two known limits:
 *   - the ONSET of fast motion (a quiet pair followed by a busy one) can give one false cut.  Its cost is one window whose recurrence
 *     restarts from the middle frame;
 *   - the second of two cuts one frame apart is missed: its m_prev is the first cut's m.
 * The defaults t_abs = 15.0 (on the 0..255 luma scale) and ratio = 2.0 are the Python side's (frames.SCENE_THRESHOLDS); they are this
 * project's choice and have not been validated on real video.  The library takes both as arguments.
 */
#ifndef VSR_HIP_SCENE_H
#define VSR_HIP_SCENE_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_SCENE_ABI_VERSION 1

#define VSR_SCENE_WG_PIXELS 1024
#define VSR_SCENE_FINISH_THREADS 256

int vsr_scene_abi_version(void);
const char* vsr_scene_last_error(void);

/* Bytes of workspace vsr_scene_pair_sums needs for these arguments: one double per workgroup.  0 for arguments that call would
 * refuse.  The library never zeroes the workspace and never reads a byte of it that the same call has not written. */
size_t vsr_scene_ws_bytes(int P, int h, int w);

/* Refused before any launch, each with its message: a null a / b / luma4 / sums / ws; non-positive P / h / w; P, h or w beyond 65535
 * (grid dimension z; offsets are 64-bit); a or b not 4-byte aligned, sums or ws not 8-byte aligned. */
int vsr_scene_pair_sums(const float* a, const float* b, int P, int h, int w, const float* luma4, double* sums, void* ws,
                        vsr_stream_t stream);

/* Refused before any launch: a null sums / flags; non-positive P; t_abs or ratio negative or not finite; sums or prev_or_null not
 * 8-byte aligned, flags not 4-byte aligned. */
int vsr_scene_decide(const double* sums, int P, const double* prev_or_null, double t_abs, double ratio, int* flags, vsr_stream_t stream);

/* Refused before any launch: a null a / b / c / x3; est_or_null without prev_est_or_null or the reverse; non-positive h / w; h or w
 * beyond 65535; with prev_est: non-positive H / W, H % h != 0, W % w != 0, H / h != W / w; a pointer not 4-byte aligned. */
int vsr_scene_window(const float* a, const float* b, const float* c, const float* prev_est_or_null, int H, int W,
                     const int* flag_ab_or_null, const int* flag_bc_or_null, float* x3, float* est_or_null, int h, int w,
                     vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_SCENE_H */
