/*
 * vsr_hip_hgi.h -- C ABI of libvsr_hip_hgi.so: one inception block of the depth hourglass's inner levels in ONE launch on MI355X
 * (gfx950).  The block is cat(1x1 | 1x1 -> k1 x k1 | 1x1 -> k2 x k2 | 1x1 -> k3 x k3), every convolution followed by folded
 * BatchNorm and ReLU (reference pytorch_DIW_scratch.py:42-72 is one instance).
 *
 * A library of its own (csrc/conv_hg_inception.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_hgi_last_error()` gives a
 * thread-local message).  No atomics, no synchronisation between workgroups.
 *
 * One workgroup evaluates one branch on one 8 x 16 output tile of one image:
 *   1. the branch's 1x1 over the tile plus the halo (k - 1) / 2, read from x with buffer loads, + bias, ReLU, rounded to fp16 into an
 *      LDS patch; a patch pixel outside the image is ZERO (the k x k convolution's padding), not relu(bias);
 *   2. the k x k convolution from that patch, + bias, ReLU, rounded to fp16 into `out` at the branch's channel offset.
 * The plain 1x1 branch runs on the tile's own pixels.  The mid channels never reach memory.  fp16 rounding points are those of the
 * four-launch path (the mid after ReLU, the outputs); accumulation is fp32 on v_mfma_f32_16x16x32_f16, one fixed order per pixel: a
 * pixel's result does not depend on N, on its tile or on the workgroup that computed it.
 *
 * Weights are the packed slabs of igemm.HConv, unchanged: [tap][cin / 32][cout_pad][32] fp16, bias [cout_pad] float32.
 *   w1 / b1: the FUSED 1x1 of the block, rows [mid | mid | mid | o0] (cout_pad = c1_pad >= 3 mid + o0);
 *   wk[j] / bk[j]: branch j's k_j x k_j convolution, mid -> cout (cout_pad = cout).
 * x: NHWC fp16 [N,H,W,in_ld], the block reads channels [in_coff, in_coff + cin) and no others.
 * out: NHWC fp16 [N,H,W,out_ld], channels [0, o0 + 3 cout) = [o0 | cout | cout | cout] are written, every one of them, and nothing else.
 */
#ifndef VSR_HIP_HGI_H
#define VSR_HIP_HGI_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_HGI_ABI_VERSION 1

#define VSR_HGI_TILE_H 8
#define VSR_HGI_TILE_W 16

int vsr_hgi_abi_version(void);
const char* vsr_hgi_last_error(void);

/* 1 when a kernel exists for the block signature (the hourglass's _A to _G: k (3,5,7) or (3,7,11), mid 32 or 64, cout 32 or 64,
 * o0 32 or 64), else 0. */
int vsr_hgi_supported(int k1, int k2, int k3, int mid, int cout, int o0);

/* Workgroups of the launch for these arguments: 4 ceil(H / 8) ceil(W / 16) N; 0 for a shape the call would refuse. */
long long vsr_hgi_workgroups(int N, int H, int W);

/* Refused before any launch, each with its message: a null pointer; non-positive N / H / W or N beyond 65535; a signature
 * vsr_hgi_supported refuses; cin not 128 or 256; in_ld, in_coff, out_ld or c1_pad no multiple of 32; a slice or the result wider than
 * its row (in_coff + cin > in_ld, o0 + 3 cout > out_ld); c1_pad < 3 mid + o0; x, out, a weight slab or a bias not 16-byte aligned
 * (the kernel reads biases four at a time); x or out of 4 GiB or more (32-bit buffer offsets); x and out overlapping.  No pointer is dereferenced on the host. */
int vsr_hgi_inception_f16(const void* x, int in_ld, int in_coff, int cin, const void* w1, const float* b1, int c1_pad, int mid, int o0,
                          const void* wk1, const float* bk1, int k1, const void* wk2, const float* bk2, int k2, const void* wk3,
                          const float* bk3, int k3, int cout, void* out, int out_ld, int N, int H, int W, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_HGI_H */
