// sr_utd_s3p.hip -- the C entries of libvsr_hip_s3p.so (include/vsr_hip_s3p.h): the fused x3 FeedbackBlock stage with the NEXT group's
// uptran slice (1x1 + PReLU) applied to its finished output rows inside the launch (k_utd_s3_post = the POST = true form of the kernel
// in sr_utd_s3.h).  A library of its own, as libvsr_hip_s3.so and libvsr_hip_s3t.so: own version entry, own error buffer, own query.
// As compiled by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage; max / select build): 185 / 178 VGPRs + 208 AGPRs, 61 / 67
// SGPRs, scratch 0 bytes per lane, occupancy 1 wave per SIMD (the plain kernel: 176 / 170 + 208, 43 / 48); 54,272 bytes of dynamic
// LDS (the plain kernel's 47,872 + two output rows 4,096 + the 1x1's fragments 2,048 + its bias and slope 256).
#include "sr_utd_s3.h"

#include "../../include/vsr_hip_s3p.h"

extern "C" {

int vsr_s3p_abi_version(void) { return VSR_S3P_ABI_VERSION; }
const char* vsr_s3p_last_error(void) { return vsr::err_buf(); }

size_t vsr_s3p_query(int what) {
    switch (what) {
        case VSR_S3P_Q_BLOB_BYTES: return S3_BLOB_POST_BYTES;
        case VSR_S3P_Q_STRIP_WIDTH: return S30_TX;
        default: return 0;
    }
}

int vsr_s3p_sr_utd_post_f16(const void* in, const void* blob, void* out, void* out_post, int N, int h, int w, int rows_per_seg,
                            int slopes_le_one, vsr_stream_t stream) {
    const size_t bytes = (size_t)N * h * w * NF * 2;
    const S3Buf bufs[] = {{in, bytes, false}, {blob, (size_t)S3_BLOB_POST_BYTES, false}, {out, bytes, false}, {out_post, bytes, false}};
    dim3 grid;
    if (int rc = s3_stage_args("s3p_sr_utd_post", bufs, 4, N, h, w, rows_per_seg, grid)) return rc;
    hipLaunchKernelGGL(slopes_le_one ? k_utd_s3_post<true> : k_utd_s3_post<false>, grid, dim3(256), S3_LDS + S3_LDS_POST,
                       vsr::S(stream), (const _Float16*)in, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg, (_Float16*)out_post);
    return vsr::launched("s3p_sr_utd_post");
}

}  // extern "C"
