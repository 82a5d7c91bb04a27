/*
 * vsr_hip_opt.h -- C ABI of libvsr_hip_opt.so: the parameter update of the train step on MI355X (gfx950): Adam (Kingma & Ba 2015, the
 * arithmetic of torch.optim.Adam without amsgrad / maximize / decoupled decay) over any number of float32 tensors in ONE launch, and
 * the global gradient norm with its clip coefficient in two.
 *
 * A library of its own (csrc/train_update.hip alone; libvsr_hip.so, its header and every other library are unchanged by it).
 *
 * Conventions: those of include/vsr_hip.h (device pointers owned by the caller, kernels enqueued on `stream`, no synchronisation /
 * allocation / free, graph-capturable; 0 = enqueued, negative = VSR_E_* and nothing was launched; `vsr_opt_last_error()` gives a
 * thread-local message).
 *
 * The plan.  The tensor table and the chunk map of a launch live in device memory, not in kernel arguments, so one launch serves any
 * number of tensors.  A chunk is VSR_OPT_CHUNK = 4096 consecutive elements of one tensor, handled by one workgroup of
 * VSR_OPT_THREADS = 256 threads; the last chunk of a tensor is short.  The byte image of a plan is
 *     vsr_opt_plan_header_t                      (32 bytes)
 *     vsr_opt_tensor_t  [n_tensors]              (40 bytes each: p, g, m, v, n)
 *     vsr_opt_chunk_t   [n_chunks]               (8 bytes each: tensor, chunk index within the tensor), tensors in order, chunks in order
 * `vsr_opt_plan_bytes` sizes it and `vsr_opt_plan_fill` fills it, both on the host and without touching a GPU.  The caller uploads the
 * image (8-byte aligned on the device) and keeps the host image: the launch entries read the grid size from the host image and
 * validate it, the kernels read the device copy.  Element offsets are 64-bit (a chunk index times 4096 is formed in 64 bits).
 * The tensors of a plan must not overlap: no two of the p, m and v arrays of all its entries may share a byte, and no g may share one
 * with a p, m or v (the kernels treat them as distinct).
 *
 * Adam, per element, every operation in float32 and rounded once (no contraction into fma; the divide and the square root are the
 * correctly rounded ones), in this order:
 *     g1 = ctl ? g * c : g                          c = the first float of `ctl`
 *     g2 = wd != 0 ? g1 + wd * p : g1               (wd * p rounded, then the sum)
 *     m' = m + omb1 * (g2 - m)
 *     v' = b2 * v + omb2 * (g2 * g2)                (three products and one sum, each rounded)
 *     d  = sqrtf(v') / rs + eps
 *     p' = p - step_size * (m' / d)
 * The scalars are float32 values the CALLER forms in float64 and rounds once: omb1 = (float)(1 - beta1), b2 = (float)beta2,
 * omb2 = (float)(1 - beta2), step_size = (float)(lr / (1 - beta1^t)), rs = (float)sqrt(1 - beta2^t), eps, wd; the library computes none.
 * p, m and v are overwritten.  g is READ ONLY: a clipped step leaves the gradient as backward wrote it (torch.nn.utils.clip_grad_norm_
 * scales .grad in place; this library never does).  Non-finite gradients propagate as the formulas say: nothing is skipped on the device.
 *
 * Thread t of a chunk's workgroup owns the elements 4 (t + 256 j) + k, j = 0..3, k = 0..3, of the chunk.  A group of four is moved
 * with one 16-byte access where the four bases p, g, m, v of its tensor are all 16-byte aligned and the group is whole, and element
 * by element otherwise; the values are the same either way, and so is the order of the norm's sum.
 *
 * The gradient norm, over every tensor of the plan (only `g` and `n` of an entry are read):
 *   pass 1: one workgroup per chunk.  Thread t adds its terms (double)g * (double)g (each exact) in double, j outer, k inner, from 0;
 *           the 256 sums meet in a fixed tree (stride 128, 64, ... 1); one double per chunk into `ws`, chunks in plan order.
 *   pass 2: ONE workgroup of 256 threads.  Thread t adds the partials t, t + 256, ... in that order from 0, then the same tree;
 *           thread 0 writes ctl = vsr_opt_ctl_t {c, 0, sumsq}, c = (float)min(1.0, max_norm / (sqrt(sumsq) + 1e-6)), in double.
 * No atomics: sumsq is the same bits in every run.  It is a function of the plan's chunk sequence: tensors of zeros APPENDED to a plan
 * leave it unchanged (their partials add exact zeros behind the others), tensors inserted before others move the partials to other
 * threads and may change the last bits.  The workspace is never zeroed by the library and never read before the same call wrote it.
 */
#ifndef VSR_HIP_OPT_H
#define VSR_HIP_OPT_H

#include <stddef.h>

#include "vsr_hip.h" /* VSR_OK / VSR_E_*, vsr_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_OPT_ABI_VERSION 1

#define VSR_OPT_CHUNK 4096
#define VSR_OPT_THREADS 256
#define VSR_OPT_MAGIC 0x3154504fu      /* "OPT1" */
#define VSR_OPT_MAX_CHUNKS 2147483647u /* a grid's x dimension */

typedef struct vsr_opt_plan_header_t {
    unsigned int magic;
    int n_tensors;
    unsigned int n_chunks;
    unsigned int reserved; /* 0 */
    unsigned long long bytes;      /* of the whole image */
    unsigned long long n_elements; /* of all tensors */
} vsr_opt_plan_header_t;

typedef struct vsr_opt_tensor_t {
    float* p;
    const float* g;
    float* m;
    float* v;
    unsigned long long n; /* elements */
} vsr_opt_tensor_t;

typedef struct vsr_opt_chunk_t {
    unsigned int tensor;
    unsigned int index; /* chunk within the tensor: elements index * 4096 ... */
} vsr_opt_chunk_t;

typedef struct vsr_opt_ctl_t {
    float c; /* the clip coefficient */
    float pad;
    double sumsq; /* the squared gradient norm */
} vsr_opt_ctl_t;

int vsr_opt_abi_version(void);
const char* vsr_opt_last_error(void);

/* Bytes of the plan image for tensors of these element counts.  0 (with a message) for what vsr_opt_plan_fill would refuse: a null
 * `sizes`, n_tensors <= 0, a size of 0, more than VSR_OPT_MAX_CHUNKS chunks. */
size_t vsr_opt_plan_bytes(int n_tensors, const unsigned long long* sizes);

/* Fills `host_image` (`bytes` of it: what vsr_opt_plan_bytes gave for these sizes).  Refused, each with its message: a null image or
 * table, n_tensors <= 0, a tensor with a null p / g / m / v, with n == 0 or with a pointer that is not 4-byte aligned, more than
 * VSR_OPT_MAX_CHUNKS chunks, `bytes` other than the image's size. */
int vsr_opt_plan_fill(void* host_image, size_t bytes, int n_tensors, const vsr_opt_tensor_t* tensors);

/* One launch: every tensor of the plan takes the step above.  `ctl`: null (no clipping) or a device vsr_opt_ctl_t (4-byte aligned is
 * enough: only c is read).  Refused: a null plan_host / plan_dev, an image whose magic or size fields are not those vsr_opt_plan_fill
 * writes, a plan_dev that is not 8-byte aligned, a ctl that is not 4-byte aligned. */
int vsr_opt_adam_f32(const void* plan_host, const void* plan_dev, const void* ctl, float omb1, float b2, float omb2, float step_size,
                     float rs, float eps, float wd, vsr_stream_t stream);

/* Bytes of workspace vsr_opt_grad_norm needs: one double per chunk.  0 for an image that call would refuse. */
size_t vsr_opt_norm_ws_bytes(const void* plan_host);

/* Two launches: the squared norm of all gradients of the plan and the clip coefficient into `ctl` (a device vsr_opt_ctl_t, written
 * whole).  Refused: what vsr_opt_adam_f32 refuses of a plan, a null ctl / ws, a ctl or ws that is not 8-byte aligned, a max_norm that
 * is not a positive number (NaN included; +inf passes: c = 1). */
int vsr_opt_grad_norm(const void* plan_host, const void* plan_dev, double max_norm, void* ctl, void* ws, vsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSR_HIP_OPT_H */
