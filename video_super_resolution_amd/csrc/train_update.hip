// train_update.hip -- the parameter update of the train step on the device (include/vsr_hip_opt.h; libvsr_hip_opt.so is built from this
// source alone): Adam over any number of float32 tensors in one launch, the global gradient norm and its clip coefficient in two.
//
//   k_adam      : one workgroup (4 waves) = one chunk of 4096 consecutive elements of one tensor, found through the plan in device
//                 memory (chunk map -> tensor entry).  Thread t owns the groups of four elements t, t + 256, t + 512, t + 768: a whole
//                 group of a tensor whose four bases are 16-byte aligned moves with 16-byte loads and stores (one wave instruction =
//                 1 KiB contiguous), anything else element by element.  A full aligned chunk (every chunk but a tensor's last) issues
//                 its sixteen 16-byte loads before the first use (and stores twelve).  16 bytes read and 12 written per element, no reuse: a streaming kernel.
//   k_norm_part : the same walk over g alone; per thread a double sum in a fixed order, a fixed tree over the workgroup, one double per
//                 chunk into the workspace.
//   k_norm_fin  : one workgroup: thread t adds the partials t, t + 256, ... in that order, the same tree, thread 0 writes {c, 0, sumsq}.
// Nothing here is atomic and no order depends on timing: the norm is the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below) and without any fast-math flag: every
// operation of the header's formulas rounds once, and the float32 divide and square root are hipcc's default correctly rounded ones.
#include <cstdint>
#include <cstring>

#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_opt.h"

#pragma clang fp contract(off)

namespace {

constexpr int CH = VSR_OPT_CHUNK, NT = VSR_OPT_THREADS;
constexpr int GROUPS = CH / (4 * NT);   // groups of four elements per thread and chunk
static_assert(GROUPS * 4 * NT == CH, "a chunk is a whole number of groups per thread");
static_assert(sizeof(vsr_opt_plan_header_t) == 32 && sizeof(vsr_opt_tensor_t) == 40 && sizeof(vsr_opt_chunk_t) == 8 &&
                  sizeof(vsr_opt_ctl_t) == 16,
              "the plan image's layout is part of the ABI");

struct Scalars {
    float omb1, b2, omb2, step_size, rs, eps, wd;
};

// the header's formulas, one line per rounded operation
template <bool CLIP, bool WD>
__device__ inline void adam1(float& p, float g, float& m, float& v, const Scalars& s, float c) {
    if (CLIP) g = g * c;
    if (WD) {
        const float d = s.wd * p;
        g = g + d;
    }
    const float dm = g - m;
    const float sm = s.omb1 * dm;
    m = m + sm;
    const float gg = g * g;
    const float a = s.b2 * v;
    const float b = s.omb2 * gg;
    v = a + b;
    const float r = sqrtf(v);
    const float q = r / s.rs;
    const float d = q + s.eps;
    const float u = m / d;
    const float w = s.step_size * u;
    p = p - w;
}

template <bool CLIP, bool WD>
__device__ inline void adam4(float4& p, const float4& g, float4& m, float4& v, const Scalars& s, float c) {
    adam1<CLIP, WD>(p.x, g.x, m.x, v.x, s, c);
    adam1<CLIP, WD>(p.y, g.y, m.y, v.y, s, c);
    adam1<CLIP, WD>(p.z, g.z, m.z, v.z, s, c);
    adam1<CLIP, WD>(p.w, g.w, m.w, v.w, s, c);
}

struct Chunk {
    vsr_opt_tensor_t t;   // the bases moved to the chunk's first element
    unsigned cnt;         // its elements: 4096, or fewer in a tensor's last chunk
};

__device__ inline Chunk find_chunk(const void* plan) {
    const auto* hdr = static_cast<const vsr_opt_plan_header_t*>(plan);
    const auto* tensors = reinterpret_cast<const vsr_opt_tensor_t*>(hdr + 1);
    const auto* chunks = reinterpret_cast<const vsr_opt_chunk_t*>(tensors + hdr->n_tensors);
    const vsr_opt_chunk_t c = chunks[blockIdx.x];
    Chunk r;
    r.t = tensors[c.tensor];
    const unsigned long long base = (unsigned long long)c.index * CH;
    const unsigned long long left = r.t.n - base;
    r.cnt = left < (unsigned long long)CH ? (unsigned)left : (unsigned)CH;
    r.t.p += base;
    r.t.g += base;
    r.t.m += base;
    r.t.v += base;
    return r;
}

__device__ inline bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

template <bool CLIP, bool WD>
__global__ void __launch_bounds__(NT)
k_adam(const void* __restrict__ plan, const float* __restrict__ ctl, Scalars s) {
    const Chunk ck = find_chunk(plan);
    float* __restrict__ p = ck.t.p;
    const float* __restrict__ g = ck.t.g;
    float* __restrict__ m = ck.t.m;
    float* __restrict__ v = ck.t.v;
    const unsigned cnt = ck.cnt, tid = threadIdx.x;
    const float c = CLIP ? ctl[0] : 1.0f;
    const bool wide = aligned16(p, g, m, v);   // (a chunk starts 16 KiB into its tensor: the tensor's alignment is the chunk's)
    if (wide && cnt == CH) {
        float4 P[GROUPS], G[GROUPS], M[GROUPS], V[GROUPS];
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            const unsigned i = tid + NT * j;
            P[j] = reinterpret_cast<const float4*>(p)[i];
            G[j] = reinterpret_cast<const float4*>(g)[i];
            M[j] = reinterpret_cast<const float4*>(m)[i];
            V[j] = reinterpret_cast<const float4*>(v)[i];
        }
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            const unsigned i = tid + NT * j;
            adam4<CLIP, WD>(P[j], G[j], M[j], V[j], s, c);
            reinterpret_cast<float4*>(p)[i] = P[j];
            reinterpret_cast<float4*>(m)[i] = M[j];
            reinterpret_cast<float4*>(v)[i] = V[j];
        }
        return;
    }
    for (int j = 0; j < GROUPS; ++j) {
        const unsigned i = tid + NT * j, e0 = 4 * i;
        if (e0 >= cnt) break;
        if (wide && e0 + 4 <= cnt) {
            float4 P = reinterpret_cast<const float4*>(p)[i], M = reinterpret_cast<const float4*>(m)[i];
            float4 V = reinterpret_cast<const float4*>(v)[i];
            const float4 G = reinterpret_cast<const float4*>(g)[i];
            adam4<CLIP, WD>(P, G, M, V, s, c);
            reinterpret_cast<float4*>(p)[i] = P;
            reinterpret_cast<float4*>(m)[i] = M;
            reinterpret_cast<float4*>(v)[i] = V;
        } else {
            for (unsigned e = e0; e < e0 + 4 && e < cnt; ++e) {
                float P = p[e], M = m[e], V = v[e];
                adam1<CLIP, WD>(P, g[e], M, V, s, c);
                p[e] = P;
                m[e] = M;
                v[e] = V;
            }
        }
    }
}

__global__ void __launch_bounds__(NT)
k_norm_part(const void* __restrict__ plan, double* __restrict__ ws) {
    __shared__ double red[NT];
    const Chunk ck = find_chunk(plan);
    const float* __restrict__ g = ck.t.g;
    const unsigned cnt = ck.cnt, tid = threadIdx.x;
    const bool wide = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    double acc = 0.0;
    for (int j = 0; j < GROUPS; ++j) {
        const unsigned i = tid + NT * j, e0 = 4 * i;
        if (e0 >= cnt) break;
        if (wide && e0 + 4 <= cnt) {
            const float4 G = reinterpret_cast<const float4*>(g)[i];
            const double x = G.x, y = G.y, z = G.z, w = G.w;
            acc += x * x;
            acc += y * y;
            acc += z * z;
            acc += w * w;
        } else {
            for (unsigned e = e0; e < e0 + 4 && e < cnt; ++e) {
                const double x = g[e];
                acc += x * x;
            }
        }
    }
    red[tid] = acc;
    vsr::sums::tree<NT>(red, tid);
    if (tid == 0) ws[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(NT)
k_norm_fin(const double* __restrict__ ws, unsigned n_chunks, double max_norm, vsr_opt_ctl_t* __restrict__ ctl) {
    __shared__ double red[NT];
    const unsigned tid = threadIdx.x;
    double acc = 0.0;
    for (unsigned i = tid; i < n_chunks; i += NT) acc += ws[i];
    red[tid] = acc;
    vsr::sums::tree<NT>(red, tid);
    if (tid == 0) {
        const double sumsq = red[0];
        const double r = max_norm / (sqrt(sumsq) + 1e-6);
        vsr_opt_ctl_t out;
        out.c = (float)(r < 1.0 ? r : 1.0);   // (NaN compares false: a NaN norm gives c = 1 and the NaN gradients speak for themselves)
        out.pad = 0.0f;
        out.sumsq = sumsq;
        *ctl = out;
    }
}

// ---------------------------------------------------------------------------------------------------- the planner (host only)
unsigned long long chunks_of(unsigned long long n) { return (n + CH - 1) / CH; }

// the chunk count of these sizes, or a refusal; `what` names the entry in the message
int count_chunks(const char* what, int n_tensors, const unsigned long long* sizes, const vsr_opt_tensor_t* tensors,
                 unsigned long long* n_chunks, unsigned long long* n_elements) {
    VSR_REQUIRE(n_tensors > 0, "%s: n_tensors must be positive, got %d", what, n_tensors);
    unsigned long long nc = 0, ne = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const unsigned long long n = sizes ? sizes[i] : tensors[i].n;
        VSR_REQUIRE(n > 0, "%s: tensor %d has no elements", what, i);
        VSR_REQUIRE(n <= (unsigned long long)VSR_OPT_MAX_CHUNKS * CH, "%s: too many chunks for one grid (tensor %d alone has %llu elements)",
                    what, i, n);
        nc += chunks_of(n);
        ne += n;
        VSR_REQUIRE(nc <= VSR_OPT_MAX_CHUNKS, "%s: too many chunks for one grid (%llu after tensor %d, at most %u)", what, nc, i,
                    VSR_OPT_MAX_CHUNKS);
    }
    *n_chunks = nc;
    *n_elements = ne;
    return VSR_OK;
}

size_t image_bytes(int n_tensors, unsigned long long n_chunks) {
    return sizeof(vsr_opt_plan_header_t) + (size_t)n_tensors * sizeof(vsr_opt_tensor_t) + (size_t)n_chunks * sizeof(vsr_opt_chunk_t);
}

// what every entry checks of a host image; the header by value (the image need not be aligned)
int check_image(const char* what, const void* plan_host, vsr_opt_plan_header_t* h) {
    VSR_REQUIRE(plan_host, "%s: null plan", what);
    memcpy(h, plan_host, sizeof(*h));
    VSR_REQUIRE(h->magic == VSR_OPT_MAGIC, "%s: not a plan image (magic 0x%08x)", what, h->magic);
    VSR_REQUIRE(h->n_tensors > 0 && h->n_chunks > 0 && h->n_chunks <= VSR_OPT_MAX_CHUNKS && h->reserved == 0 &&
                    h->bytes == image_bytes(h->n_tensors, h->n_chunks),
                "%s: plan image of the wrong size (%llu bytes for %d tensors, %u chunks)", what, h->bytes, h->n_tensors, h->n_chunks);
    return VSR_OK;
}

// ... and what the launch entries check of the pair: the host image and its device copy
int check_plan(const char* what, const void* plan_host, const void* plan_dev, vsr_opt_plan_header_t* h) {
    VSR_REQUIRE(plan_host && plan_dev, "%s: null plan", what);
    const int rc = check_image(what, plan_host, h);
    if (rc) return rc;
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(plan_dev) & 7) == 0, "%s: the device plan must be 8-byte aligned", what);
    return VSR_OK;
}

}  // namespace

extern "C" {

int vsr_opt_abi_version(void) { return VSR_OPT_ABI_VERSION; }
const char* vsr_opt_last_error(void) { return vsr::err_buf(); }

size_t vsr_opt_plan_bytes(int n_tensors, const unsigned long long* sizes) {
    if (!sizes) {
        vsr::fail(VSR_E_ARG, "opt_plan_bytes: null pointer");
        return 0;
    }
    unsigned long long nc, ne;
    if (count_chunks("opt_plan_bytes", n_tensors, sizes, nullptr, &nc, &ne) != VSR_OK) return 0;
    return image_bytes(n_tensors, nc);
}

int vsr_opt_plan_fill(void* host_image, size_t bytes, int n_tensors, const vsr_opt_tensor_t* tensors) {
    VSR_REQUIRE(host_image && tensors, "opt_plan_fill: null pointer");
    unsigned long long nc, ne;
    const int rc = count_chunks("opt_plan_fill", n_tensors, nullptr, tensors, &nc, &ne);
    if (rc) return rc;
    for (int i = 0; i < n_tensors; ++i) {
        const vsr_opt_tensor_t& t = tensors[i];
        VSR_REQUIRE(t.p && t.g && t.m && t.v, "opt_plan_fill: tensor %d has a null pointer", i);
        VSR_REQUIRE(((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                      reinterpret_cast<uintptr_t>(t.v)) & 3) == 0,
                    "opt_plan_fill: tensor %d: every pointer must be 4-byte aligned", i);
    }
    VSR_REQUIRE(bytes == image_bytes(n_tensors, nc), "opt_plan_fill: image of the wrong size (%zu bytes given, the plan takes %zu)", bytes,
                image_bytes(n_tensors, nc));
    char* at = static_cast<char*>(host_image);
    const vsr_opt_plan_header_t h = {VSR_OPT_MAGIC, n_tensors, (unsigned)nc, 0u, (unsigned long long)bytes, ne};
    memcpy(at, &h, sizeof(h));
    at += sizeof(h);
    memcpy(at, tensors, (size_t)n_tensors * sizeof(vsr_opt_tensor_t));
    at += (size_t)n_tensors * sizeof(vsr_opt_tensor_t);
    for (int i = 0; i < n_tensors; ++i) {
        const unsigned k = (unsigned)chunks_of(tensors[i].n);
        for (unsigned j = 0; j < k; ++j) {
            const vsr_opt_chunk_t c = {(unsigned)i, j};
            memcpy(at, &c, sizeof(c));
            at += sizeof(c);
        }
    }
    return VSR_OK;
}

int vsr_opt_adam_f32(const void* plan_host, const void* plan_dev, const void* ctl, float omb1, float b2, float omb2, float step_size,
                     float rs, float eps, float wd, vsr_stream_t stream) {
    vsr_opt_plan_header_t h;
    const int rc = check_plan("opt_adam_f32", plan_host, plan_dev, &h);
    if (rc) return rc;
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(ctl) & 3) == 0, "opt_adam_f32: ctl must be 4-byte aligned");
    const Scalars s = {omb1, b2, omb2, step_size, rs, eps, wd};
    const dim3 grid(h.n_chunks), block(NT);
    hipStream_t st = vsr::S(stream);
    const float* c = static_cast<const float*>(ctl);
    const bool clip = ctl != nullptr, decay = wd != 0.0f;
    if (clip && decay) hipLaunchKernelGGL((k_adam<true, true>), grid, block, 0, st, plan_dev, c, s);
    else if (clip) hipLaunchKernelGGL((k_adam<true, false>), grid, block, 0, st, plan_dev, c, s);
    else if (decay) hipLaunchKernelGGL((k_adam<false, true>), grid, block, 0, st, plan_dev, c, s);
    else hipLaunchKernelGGL((k_adam<false, false>), grid, block, 0, st, plan_dev, c, s);
    return vsr::launched("opt_adam_f32");
}

size_t vsr_opt_norm_ws_bytes(const void* plan_host) {
    vsr_opt_plan_header_t h;
    if (check_image("opt_norm_ws_bytes", plan_host, &h) != VSR_OK) return 0;
    return (size_t)h.n_chunks * sizeof(double);
}

int vsr_opt_grad_norm(const void* plan_host, const void* plan_dev, double max_norm, void* ctl, void* ws, vsr_stream_t stream) {
    vsr_opt_plan_header_t h;
    const int rc = check_plan("opt_grad_norm", plan_host, plan_dev, &h);
    if (rc) return rc;
    VSR_REQUIRE(ctl && ws, "opt_grad_norm: null pointer");
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(ctl) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "opt_grad_norm: ctl and the workspace must be 8-byte aligned");
    VSR_REQUIRE(max_norm > 0.0, "opt_grad_norm: max_norm must be positive, got %g", max_norm);
    hipStream_t st = vsr::S(stream);
    double* wsd = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_norm_part, dim3(h.n_chunks), dim3(NT), 0, st, plan_dev, wsd);
    const int rc1 = vsr::launched("opt_grad_norm/partials");
    if (rc1) return rc1;
    hipLaunchKernelGGL(k_norm_fin, dim3(1), dim3(NT), 0, st, (const double*)wsd, h.n_chunks, max_norm, static_cast<vsr_opt_ctl_t*>(ctl));
    return vsr::launched("opt_grad_norm/finish");
}

}  // extern "C"
