/*
 * vsr_hip_grad.h -- C ABI of libvsr_hip_grad.so: the adjoints of FlowNet2's three native operators on MI355X (gfx950).
 *
 * include/vsr_hip.h declares the forward of Resample2d, ChannelNorm and Correlation; this header declares their backward, in
 * a library of its own (csrc/flow_ops_bwd.hip alone; libvsr_hip.so and its header are unchanged by it).  The reference exports
 * `forward` and `backward` from each of its three extension modules; the gradients here are the derivatives of THIS
 * repository's forward kernels (csrc/flow_ops.hip), which restate the reference's forward bit for bit.
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, float32 NCHW, kernels enqueued on `stream`,
 * no synchronisation / allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched;
 * `vsr_grad_last_error()` gives a thread-local message).  In addition:
 *   - a gradient pointer named `*_or_null` may be null: that gradient is not needed and is not computed
 *     (autograd's needs_input_grad); at least one of an entry's gradients must be asked for;
 *   - every gradient buffer is written in full by the entry itself (an entry that scatters zeroes its destination on
 *     `stream` first): the caller passes uninitialised memory;
 *   - no gradient buffer may overlap an input.
 * Determinism: every gradient is a gather with a fixed summation order -- bit-identical from run to run -- except
 * d_img of vsr_grad_resample2d_f32, which is a scatter of float atomic adds and depends on arrival order in its last bits.
 *
 * All file:line citations are relative to the reference repository root.
 */
#ifndef VSR_HIP_GRAD_H
#define VSR_HIP_GRAD_H

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_GRAD_ABI_VERSION 1

int vsr_grad_abi_version(void);
const char* vsr_grad_last_error(void);

/* resample2d_cuda.backward(input1, input2, gradOutput, gradInput1, gradInput2, kernel_size, bilinear)
 *   resample2d_package/resample2d_cuda.cc:15-32, resample2d_kernel.cu:74-198,244-326.
 * img [B,C,H,W], flow [B,2,H,W], gout [B,C,H,W] -> d_img [B,C,H,W], d_flow [B,2,H,W].
 * With xf = x + flow[b,0,y,x], yf = y + flow[b,1,y,x], alpha = xf - floor(xf), beta = yf - floor(yf) and xL, xR, yT, yB the four
 * indices clamped independently (exactly the forward's, resample2d_kernel.cu:41-53):
 *   d_img  += gout[b,c,y,x] * {(1-alpha)(1-beta), alpha(1-beta), (1-alpha)beta, alpha beta} at (yT,xL), (yT,xR), (yB,xL), (yB,xR)
 *   d_flow[b,0,y,x] = sum_c gout * ((1-beta)(I[yT,xR]-I[yT,xL]) + beta (I[yB,xR]-I[yB,xL]))
 *   d_flow[b,1,y,x] = sum_c gout * ((1-alpha)(I[yB,xL]-I[yT,xL]) + alpha(I[yB,xR]-I[yT,xR]))
 * (the indices are constants of the derivative, as in the reference).  bilinear == 0: d_img is the scatter to the one rounded
 * pixel (resample2d_kernel.cu:65-70) and d_flow is zero.
 * NOT reproduced: the reference's image gradient takes alpha = xf - int(xf) (truncation; the alpha / beta lines of
 * kernel_resample2d_backward_input1, resample2d_kernel.cu:105-106) where its forward takes floor (resample2d_kernel.cu:45-46), so for xf < 0 it is not the
 * adjoint of its own forward.  Here both use floor.
 * d_img is zeroed on `stream`, then accumulated with float atomic adds (order-dependent in the last bits); d_flow is a gather,
 * one thread per pixel computing both components over all channels (the reference: one thread per component). */
int vsr_grad_resample2d_f32(const float* img, const float* flow, const float* gout, float* d_img_or_null, float* d_flow_or_null,
                            int B, int C, int H, int W, int kernel_size, int bilinear, vsr_stream_t stream);

/* channelnorm_cuda.backward(input1, output, gradOutput, gradInput1, norm_deg)
 *   channelnorm_package/channelnorm_cuda.cc:16-26, channelnorm_kernel.cu:62-96,133-174.
 * in [B,C,H,W], out [B,1,H,W] (the forward's result), gout [B,1,H,W] -> d_in [B,C,H,W]:
 *   d_in[b,c,y,x] = gout[b,0,y,x] * in[b,c,y,x] / (out[b,0,y,x] + 1e-9)                              (channelnorm_kernel.cu:92)
 * A pixel whose channels are all zero gets gradient 0, not NaN. */
int vsr_grad_channelnorm_f32(const float* in, const float* out, const float* gout, float* d_in, int B, int C, int H, int W,
                             vsr_stream_t stream);

/* correlation_cuda.backward(input1, input2, rbot1, rbot2, gradOutput, gradInput1, gradInput2, pad, k, max_disp, s1, s2, mult)
 *   correlation_package/correlation_cuda.cc:89-170, correlation_cuda_kernel.cu:150-334,429-564.
 * f1, f2 [B,C,H,W], gout [B,D*D,OH,OW] (geometry: vsr_correlation_out_shape of include/vsr_hip.h) -> d_f1, d_f2 [B,C,H,W].
 * With R = max_displacement / stride2, D = 2R+1, (y1, x1) = (oy, ox) * stride1 + max_displacement - pad_size:
 *   d_f1[b,c,y1,x1] = 1/C sum_{tj,ti} gout[b,(tj+R)D+ti+R,oy,ox]   * f2[b,c,y1+tj*s2,x1+ti*s2]
 *   d_f2[b,c,y2,x2] = 1/C sum_{tj,ti} gout[b,(tj+R)D+ti+R,oy',ox'] * f1[b,c,y2-tj*s2,x2-ti*s2],  (oy',ox') the output pixel of
 *                     that f1 position (positions off the stride1 grid or outside the output contribute nothing)
 * (zero outside the image; f1 positions that feed no output pixel get gradient 0).  kernel_size must be 1, as in the forward.
 * Both are gathers summed tj-major, ti-minor: bit-identical from run to run, no atomics, no padded scratch copies (the
 * reference's rbot1 / rbot2 do not exist here).  Refused before any launch, like the forward: D beyond 32, a displacement window of
 * 32 + 2R*stride2 columns beyond 480 (LDS; every window the forward admits fits), B * ceil(C/32) or H beyond 65535 (grid). */
int vsr_grad_correlation_f32(const float* f1, const float* f2, const float* gout, float* d_f1_or_null, float* d_f2_or_null, int B,
                             int C, int H, int W, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                             vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_GRAD_H */
