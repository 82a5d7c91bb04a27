// sr_utd_s3f.hip -- the C entries of libvsr_hip_s3f.so (include/vsr_hip_s3f.h): the fused x3 FeedbackBlock stage with the 1x1 chain
// that opens a step (compress_out -> compress_in -> first uptran slice; step 0: compress_in -> uptran slice) folded into its LR load
// path (k_utd_s3_pre = the PRE = true forms of the kernel in sr_utd_s3.h, with and without POST).  A library of its own, as
// libvsr_hip_s3.so, libvsr_hip_s3t.so and libvsr_hip_s3p.so: own version entry, own error buffer, own query.
// As compiled by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage; max / select build): PRE + POST 211 / 208 VGPRs + 208 AGPRs,
// 72 / 84 SGPRs; PRE alone 198 / 196 + 208, 60 / 69; scratch 0 bytes per lane, occupancy 1 wave per SIMD; 65,024 / 58,624 bytes of
// dynamic LDS (the POST / plain kernel's 54,272 / 47,872 + the chain's ten fragments 10,240 + its three biases 512).
#include "sr_utd_s3.h"

#include "../../include/vsr_hip_s3f.h"

namespace {

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int vsr_s3f_abi_version(void) { return VSR_S3F_ABI_VERSION; }
const char* vsr_s3f_last_error(void) { return vsr::err_buf(); }

size_t vsr_s3f_query(int what) {
    switch (what) {
        case VSR_S3F_Q_BLOB_BYTES: return S3_BLOB_PRE_BYTES;
        case VSR_S3F_Q_STRIP_WIDTH: return S3_TX;
        default: return 0;
    }
}

int vsr_s3f_sr_utd_pre_f16(const void* feat, const void* a, const void* b, const void* cmap, const void* blob, void* out, void* out_post,
                           int N, int h, int w, int rows_per_seg, int slopes_le_one, vsr_stream_t stream) {
    VSR_REQUIRE(feat && blob && out, "s3f_sr_utd_pre: null pointer");
    VSR_REQUIRE((a && b && cmap) || (!a && !b && !cmap), "s3f_sr_utd_pre: a, b and cmap must be given together (all three: PRE3, none: PRE2)");
    VSR_REQUIRE(N > 0 && h > 0 && w > 0 && rows_per_seg >= 0 && N <= 65535, "s3f_sr_utd_pre: bad shape (N %d, h %d, w %d, rows_per_seg %d)", N, h, w,
                rows_per_seg);
    const size_t bytes = (size_t)N * h * w * NF * 2, cbytes = (size_t)h * w * NF * 4;
    // (pointer, bytes): absent ones are skipped; every pair is checked on its byte ranges
    const struct { const void* p; size_t n; } bufs[7] = {{feat, bytes}, {a, bytes}, {b, bytes}, {cmap, cbytes}, {blob, (size_t)S3_BLOB_PRE_BYTES},
                                                         {out, bytes}, {out_post, bytes}};
    for (int i = 0; i < 7; ++i)
        VSR_REQUIRE((reinterpret_cast<uintptr_t>(bufs[i].p) & 15) == 0, "s3f_sr_utd_pre: pointers must be 16-byte aligned");
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            VSR_REQUIRE(!bufs[i].p || !bufs[j].p || !ranges_overlap(bufs[i].p, bufs[i].n, bufs[j].p, bufs[j].n),
                        "s3f_sr_utd_pre: feat, a, b, cmap, blob, out and out_post must not overlap");
    if (bytes >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "s3f_sr_utd_pre: tensors beyond 4 GiB (split the planes)");
    if (cmap && cbytes >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "s3f_sr_utd_pre: constant map beyond 4 GiB");
    if (rows_per_seg == 0) rows_per_seg = h;   // one march per strip
    const unsigned strips = vsr::cdiv(w, S3_TX), segs = vsr::cdiv(h, rows_per_seg);
    VSR_REQUIRE(segs <= 65535, "s3f_sr_utd_pre: too many row segments");
    const size_t lds = S3_LDS + (out_post ? S3_LDS_POST : 0) + S3_LDS_PRE;
    const auto kern = out_post ? (slopes_le_one ? k_utd_s3_pre<true, true> : k_utd_s3_pre<false, true>)
                               : (slopes_le_one ? k_utd_s3_pre<true, false> : k_utd_s3_pre<false, false>);
    hipLaunchKernelGGL(kern, dim3(strips, segs, N), dim3(256), lds, vsr::S(stream), (const _Float16*)feat, (const _Float16*)a, (const _Float16*)b,
                       (const float*)cmap, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg, (_Float16*)out_post);
    return vsr::launched("s3f_sr_utd_pre");
}

}  // extern "C"
