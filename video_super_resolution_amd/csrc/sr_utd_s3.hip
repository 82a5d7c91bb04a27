// sr_utd_s3.hip -- the C entries of libvsr_hip_s3.so (include/vsr_hip_s3.h): the fused x3 FeedbackBlock stage, plain build.  The
// kernel (k_utd_s3) and its description are in sr_utd_s3.h; this file instantiates its POST = false form only, so the library keeps
// its four exports and its register / LDS / scratch figures.
#include "sr_utd_s3.h"

#include "../../include/vsr_hip_s3.h"

extern "C" {

int vsr_s3_abi_version(void) { return VSR_S3_ABI_VERSION; }
const char* vsr_s3_last_error(void) { return vsr::err_buf(); }

size_t vsr_s3_query(int what) {
    switch (what) {
        case VSR_S3_Q_BLOB_BYTES: return S3_BLOB_BYTES;
        case VSR_S3_Q_STRIP_WIDTH: return S30_TX;
        default: return 0;
    }
}

int vsr_s3_sr_utd_f16(const void* in, const void* blob, void* out, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                      vsr_stream_t stream) {
    const size_t bytes = (size_t)N * h * w * NF * 2;
    const S3Buf bufs[] = {{in, bytes, false}, {blob, (size_t)S3_BLOB_BYTES, false}, {out, bytes, false}};
    dim3 grid;
    if (int rc = s3_stage_args("s3_sr_utd", bufs, 3, N, h, w, rows_per_seg, grid)) return rc;
    hipLaunchKernelGGL(slopes_le_one ? k_utd_s3<true> : k_utd_s3<false>, grid, dim3(256), S3_LDS, vsr::S(stream),
                       (const _Float16*)in, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg);
    return vsr::launched("s3_sr_utd");
}

}  // extern "C"
