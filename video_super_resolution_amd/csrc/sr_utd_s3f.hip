// sr_utd_s3f.hip -- the C entries of libvsr_hip_s3f.so (include/vsr_hip_s3f.h): the fused x3 FeedbackBlock stage with the 1x1 chain
// that opens a step (compress_out -> compress_in -> first uptran slice; step 0: compress_in -> uptran slice) folded into its LR load
// path (k_utd_s3_pre = the PRE = true forms of the kernel in sr_utd_s3.h, with and without POST).  A library of its own, as
// libvsr_hip_s3.so, libvsr_hip_s3t.so and libvsr_hip_s3p.so: own version entry, own error buffer, own query.
// As compiled by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage; max / select build): PRE + POST 211 / 208 VGPRs + 208 AGPRs,
// 72 / 84 SGPRs; PRE alone 198 / 196 + 208, 60 / 69; scratch 0 bytes per lane, occupancy 1 wave per SIMD; 65,024 / 58,624 bytes of
// dynamic LDS (the POST / plain kernel's 54,272 / 47,872 + the chain's ten fragments 10,240 + its three biases 512).
#include "sr_utd_s3.h"

#include "../../include/vsr_hip_s3f.h"

extern "C" {

int vsr_s3f_abi_version(void) { return VSR_S3F_ABI_VERSION; }
const char* vsr_s3f_last_error(void) { return vsr::err_buf(); }

size_t vsr_s3f_query(int what) {
    switch (what) {
        case VSR_S3F_Q_BLOB_BYTES: return S3_BLOB_PRE_BYTES;
        case VSR_S3F_Q_STRIP_WIDTH: return S30_TX;
        default: return 0;
    }
}

int vsr_s3f_sr_utd_pre_f16(const void* feat, const void* a, const void* b, const void* cmap, const void* blob, void* out, void* out_post,
                           int N, int h, int w, int rows_per_seg, int slopes_le_one, vsr_stream_t stream) {
    VSR_REQUIRE((a && b && cmap) || (!a && !b && !cmap), "s3f_sr_utd_pre: a, b and cmap must be given together (all three: PRE3, none: PRE2)");
    const size_t bytes = (size_t)N * h * w * NF * 2, cbytes = (size_t)h * w * NF * 4;
    const S3Buf bufs[] = {{feat, bytes, false}, {a, bytes, true}, {b, bytes, true}, {cmap, cbytes, true}, {blob, (size_t)S3_BLOB_PRE_BYTES, false},
                          {out, bytes, false}, {out_post, bytes, true}};
    dim3 grid;
    if (int rc = s3_stage_args("s3f_sr_utd_pre", bufs, 7, N, h, w, rows_per_seg, grid)) return rc;
    if (cmap && cbytes >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "s3f_sr_utd_pre: constant map beyond 4 GiB");
    const size_t lds = S3_LDS + (out_post ? S3_LDS_POST : 0) + S3_LDS_PRE;
    const auto kern = out_post ? (slopes_le_one ? k_utd_s3_pre<true, true> : k_utd_s3_pre<false, true>)
                               : (slopes_le_one ? k_utd_s3_pre<true, false> : k_utd_s3_pre<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, vsr::S(stream), (const _Float16*)feat, (const _Float16*)a, (const _Float16*)b,
                       (const float*)cmap, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg, (_Float16*)out_post);
    return vsr::launched("s3f_sr_utd_pre");
}

}  // extern "C"
