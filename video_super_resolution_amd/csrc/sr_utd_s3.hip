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
        case VSR_S3_Q_STRIP_WIDTH: return S3_TX;
        default: return 0;
    }
}

int vsr_s3_sr_utd_f16(const void* in, const void* blob, void* out, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                      vsr_stream_t stream) {
    VSR_REQUIRE(in && blob && out, "s3_sr_utd: null pointer");
    VSR_REQUIRE(N > 0 && h > 0 && w > 0 && rows_per_seg >= 0 && N <= 65535, "s3_sr_utd: bad shape (N %d, h %d, w %d, rows_per_seg %d)", N, h, w, rows_per_seg);
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(blob) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0, "s3_sr_utd: pointers must be 16-byte aligned");
    VSR_REQUIRE(in != out, "s3_sr_utd: in and out must not overlap");
    if ((size_t)N * h * w * NF * 2 >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "s3_sr_utd: tensors beyond 4 GiB (split the planes)");
    if (rows_per_seg == 0) rows_per_seg = h;   // one march per strip
    const unsigned strips = vsr::cdiv(w, S3_TX), segs = vsr::cdiv(h, rows_per_seg);
    VSR_REQUIRE(segs <= 65535, "s3_sr_utd: too many row segments");
    hipLaunchKernelGGL(slopes_le_one ? k_utd_s3<true> : k_utd_s3<false>, dim3(strips, segs, N), dim3(256), S3_LDS, vsr::S(stream),
                       (const _Float16*)in, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg);
    return vsr::launched("s3_sr_utd");
}

}  // extern "C"
