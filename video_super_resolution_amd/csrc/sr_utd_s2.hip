// sr_utd_s2.hip -- k_utd_s2: the fused  up (deconv k6 s2 p2 + PReLU) -> tran (1x1 + PReLU) -> down (conv k6 s2 p2 + PReLU)
// stage of the FeedbackBlock for the scale-2 extension (SRFBN's (6, 2, 2) row in place of the reference's literal (8, 4, 2),
// SRProjectionModule.py:10-12,62-65,77-80 under the zero-fill semantic).  The x2 feature map (4.25 GB per tensor at LR
// 1080x1920 x 8 planes in fp16, 17 GB at 4K -> 8K) never leaves the registers; the unfused build (sr.py:_UnfusedStage: phase
// deconvolutions, in-place 1x1, strided convolution on the generic kernel) moves it through HBM three times and is kept as
// the cross-check.
//
// Design = k_utd3's register hand-over (sr_utd3.hip) with the x2 geometry:
//   * a workgroup of 4 waves marches down a strip of 30 LR columns; step m handles the HR row PAIR m (rows 2m, 2m+1).
//   * wave (r, c) = (HR row parity, HR column parity) deconvolves HR row 2m+r at the 32 columns 2q+c, q = x0-1 .. x0+30:
//     HR (2m+r, 2q+c) = b + sum_{dy,dx<3} W_up[ky = r+2dy][kx = c+2dx] . LR(m+1-dy, q+1-dx)     -> 9 taps x 2 x 2 MFMA 16x16x32
//     (K = 32 channels per tap, B operand = LR pixels from a 4-row LDS ring, A = weights in registers), PReLU, the 1x1 with the
//     accumulator tile re-used in place as its B operand (channel order permuted consistently in the packed weights), PReLU.
//   * the same wave convolves its tile as it lies in registers: HR row 2m+r is kernel row r, r+2, r+4 of the output rows m+1,
//     m, m-1 (three accumulator sets in flight), and HR column 2q+c is kernel column c+2s of output pixel j = q+1-s, i.e. the
//     tile shifted by s = 0, 1, 2 lanes (DPP row shifts; lane 15 / 14 of pixel tile 0 take lanes 0 / 1 of tile 1).
//   * the output row whose last kernel row was just added leaves as 4 partial tiles (one per wave) through LDS, summed in a
//     fixed order + bias + PReLU by all 256 threads.  One barrier per step.
// Per wave and step: 36 + 4 + 36 MFMA against ~48 activation VALU + 24 DPP: a better MFMA : VALU ratio than the x4 kernel
// (144 : 316), and 38 weight fragments (152 registers) instead of 64, so two workgroups share a CU.
#include "sr_strip30.h"

namespace {

constexpr int S2_BIAS_BYTES = 256 + 2048;    // b_up[32], b_dt[32] fp32 + the two 1x1 fragments (read at use: the kernel sits at the 256-register line)
constexpr int S2_LDS = S30_LR_BYTES + 2 * S30_PART_BUF + S2_BIAS_BYTES;

constexpr int S2_BLOB_UP = 0;                           // [wave 4][tap 9 = dy*3+dx][mt 2][lane 64][8] fp16
constexpr int S2_BLOB_DN = 4 * 18 * 1024;               // [wave 4][kernel-row slot 3][shift 3][mt 2][lane 64][8] fp16
constexpr int S2_BLOB_DT = S2_BLOB_DN + 4 * 18 * 1024;  // [mt 2][lane 64][8] fp16
constexpr int S2_BLOB_F32 = S2_BLOB_DT + 2 * 1024;      // b_up[32] b_dt[32] b_dn[32] slope_up slope_dt slope_dn
constexpr int S2_BLOB_POST = S2_BLOB_F32 + 512;         // POST: [mt 2][lane 64][8] fp16 (natural channel order), then b_post[32], slope_post (64 floats)
constexpr int S2_BLOB_BYTES = S2_BLOB_POST + 2048 + 256;
constexpr int S2_LDS_POST = 2 * S30_OROW + 2048 + 256;   // two rows + the 1x1's fragments + bias

// FLAT: one basic block per step -- pairs outside the image are computed and zeroed (two steps per march), the partial tiles
// are always stored and the reduce of a row that is not output stores to an out-of-range buffer offset -- so that the
// compiler may schedule across what were branch boundaries (A/B: vsr_sr_utd_s2_variant).
// POST: the NEXT group's uptran slice (1x1 + PReLU on this stage's output, SRProjectionModule.py:55-61 under the zero-fill semantic) applied
// to every finished output row inside this launch and written to `out2` -- at x2 the separate 1x1 launch it replaces is HBM-bound and
// costs a sixth of the stage (2.65 GB per 5 planes of 1080 x 1920).  The reduce leaves the row's fp16 values in LDS as well (orow);
// two steps later each wave multiplies one 16 x 16 quadrant (out-channel tile wv / 2, pixel tile wv % 2): 1 MFMA + 6 VALU per wave and
// step.  Same operation order as k_chain1x1_s (bias-seeded accumulator, K = 32 in one MFMA, fp16 PReLU): bit-identical.
template <bool ALLMAX, bool FLAT, bool POST>
__global__ void __launch_bounds__(256, 2)
k_utd_s2(const _Float16* __restrict__ in, const unsigned char* __restrict__ blob, _Float16* __restrict__ out, int h, int w,
         int rows_per_seg, _Float16* __restrict__ out2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const lrr = smem;
    unsigned char* const part = smem + S30_LR_BYTES;
    unsigned char* const orow = smem + S2_LDS;          // (POST only: the launch allocates S2_LDS + S2_LDS_POST)
    unsigned char* const postw = orow + 2 * S30_OROW;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int r = wv >> 1, c = wv & 1;          // HR row parity / HR column parity this wave owns
    const int x0 = blockIdx.x * S30_TX;
    const int n = blockIdx.z;
    const int r0 = blockIdx.y * rows_per_seg;
    const int r1 = min(h, r0 + rows_per_seg);
    if (r0 >= r1) return;   // uniform per workgroup

    // ---- weights -> registers, once per workgroup
    h8 Aup[9][2], Adn[3][3][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            Aup[t][mt] = *reinterpret_cast<const h8*>(blob + S2_BLOB_UP + (((wv * 9 + t) * 2 + mt) * 64 + lane) * 16);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                Adn[k][s][mt] = *reinterpret_cast<const h8*>(blob + S2_BLOB_DN + ((((wv * 3 + k) * 3 + s) * 2 + mt) * 64 + lane) * 16);
    const float* fpar = reinterpret_cast<const float*>(blob + S2_BLOB_F32);
    float* const bias_s = reinterpret_cast<float*>(smem + S30_LR_BYTES + 2 * S30_PART_BUF);
    if (tid < 64) bias_s[tid] = fpar[tid];   // (visible after the prologue's barrier)
    unsigned char* const adt_s = smem + S30_LR_BYTES + 2 * S30_PART_BUF + 256;
    if (tid < 128) *reinterpret_cast<u4v*>(adt_s + tid * 16) = *reinterpret_cast<const u4v*>(blob + S2_BLOB_DT + tid * 16);
    auto adt = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const h8*>(adt_s + (mt * 64 + lane) * 16); };
    // this lane's accumulator rows are channels {4g..4g+3} of tile mt
    auto bup = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(bias_s + 16 * mt + 4 * g); };
    auto bdt = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(bias_s + 32 + 16 * mt + 4 * g); };
    const float a_up = fpar[96], a_dt = fpar[97], a_dn = fpar[98];
    h2 a_post2 = {(_Float16)1.0f, (_Float16)1.0f};
    bool post_max = true;
    if (POST) {
        const float* ppar = reinterpret_cast<const float*>(blob + S2_BLOB_POST + 2048);
        if (tid < 128) *reinterpret_cast<u4v*>(postw + tid * 16) = *reinterpret_cast<const u4v*>(blob + S2_BLOB_POST + tid * 16);
        else if (tid < 160) *reinterpret_cast<float*>(postw + 2048 + (tid - 128) * 4) = ppar[tid - 128];
        a_post2 = h2{(_Float16)ppar[32], (_Float16)ppar[32]};
        post_max = ALLMAX || ppar[32] <= 1.0f;
    }
    const h2 a_up2 = {(_Float16)a_up, (_Float16)a_up}, a_dt2 = {(_Float16)a_dt, (_Float16)a_dt};
    const bool up_max = ALLMAX || a_up <= 1.0f, dt_max = ALLMAX || a_dt <= 1.0f;

    // ---- LR loader: 34 columns x 4 chunks of 16 bytes per row; out-of-image pieces read zeros (out-of-range buffer offset)
    const __amdgpu_buffer_rsrc_t in_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(in), 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    const bool lr_loader = tid < S30_LRC * 4;
    const int lr_px = tid >> 2, lr_ch = tid & 3, lr_col = x0 - 2 + lr_px;
    const bool lr_col_ok = lr_loader && lr_col >= 0 && lr_col < w;
    const int lr_st = lr_off(lr_px, lr_ch);
    auto fetch_lr = [&](int row) __attribute__((always_inline)) -> u4v {
        const unsigned off = (lr_col_ok && row >= 0 && row < h) ? (unsigned)(((((size_t)n * h + row) * w + lr_col) * NF + lr_ch * 8) * 2) : 0xFFFFFFFFu;
        return __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off, 0, 0);
    };
    auto lr_slot = [&](int row) __attribute__((always_inline)) { return ((row + 4) & 3) * S30_LR_SLOT; };   // (row >= -3)

    // ---- reduce role: output pixel tid>>3 (32 of them, 30 live), channels 4*(tid&7) .. +3
    const int rj = tid >> 3, rc4 = tid & 7;
    const f4 bdn = *reinterpret_cast<const f4*>(fpar + 64 + 4 * rc4);
    const bool red_ok = (rj < S30_TX) && (x0 + rj < w);
    const __amdgpu_buffer_rsrc_t out_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    typedef float f2v __attribute__((ext_vector_type(2)));
    const int part_wr = wv * S30_PART_W + l15 * PART_PX_PITCH + 4 * g * 4;   // + 64 mt + 16 nt PART_PX_PITCH
    const int part_rd = rj * PART_PX_PITCH + rc4 * 16;                       // + k S30_PART_W
    auto reduce_store = [&](int i, const unsigned char* pbase, bool ok) __attribute__((always_inline)) {
        f4 s = *reinterpret_cast<const f4*>(pbase + part_rd);
#pragma unroll
        for (int k = 1; k < 4; ++k) s += *reinterpret_cast<const f4*>(pbase + part_rd + k * S30_PART_W);
        s += bdn;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s[e] >= 0.0f ? s[e] : s[e] * a_dn;
        const unsigned lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[0], v[1]}, h2));
        const unsigned hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[2], v[3]}, h2));
        const unsigned off = (red_ok && ok) ? (unsigned)(((((size_t)n * h + i) * w + x0 + rj) * NF + 4 * rc4) * 2) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b64(u2v{lo, hi}, out_rsrc, off, 0, 0);
        if (POST) *reinterpret_cast<u2v*>(orow + (i & 1) * S30_OROW + lr_off(rj, rc4 >> 1) + (rc4 & 1) * 8) = u2v{lo, hi};
    };
    // POST: the 1x1 on finished row i (its fp16 values lie in orow[i & 1] since the barrier that followed its reduce): this wave's quadrant
    const __amdgpu_buffer_rsrc_t out2_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(POST ? out2 : out, 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    const int pmt = wv >> 1, ppx = 16 * (wv & 1) + l15;
    const bool post_px_ok = ppx < S30_TX && x0 + ppx < w;
    auto post_row = [&](int i) __attribute__((always_inline)) {
        const h8 b = *reinterpret_cast<const h8*>(orow + (i & 1) * S30_OROW + lr_off(ppx, g));
        const h8 a = *reinterpret_cast<const h8*>(postw + (pmt * 64 + lane) * 16);
        const f4 e = mfma16(a, b, *reinterpret_cast<const f4*>(postw + 2048 + (16 * pmt + 4 * g) * 4));
        const h2 p0 = prelu_h2(__builtin_convertvector(f2v{e[0], e[1]}, h2), a_post2, post_max);
        const h2 p1 = prelu_h2(__builtin_convertvector(f2v{e[2], e[3]}, h2), a_post2, post_max);
        const unsigned off = (post_px_ok && i >= r0 && i < r1) ? (unsigned)(((((size_t)n * h + i) * w + x0 + ppx) * NF + 16 * pmt + 4 * g) * 2) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b64(u2v{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)}, out2_rsrc, off, 0, 0);
    };

    // ---- prologue: LR rows r0-2, r0-1, r0 (the first pair, m = r0-1, reads them)
    if (lr_loader) {
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0 - 2) + lr_st) = fetch_lr(r0 - 2);
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0 - 1) + lr_st) = fetch_lr(r0 - 1);
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0) + lr_st) = fetch_lr(r0);
    }
    __syncthreads();

    // accumulators of the three output rows in flight: [0] row m-1 (gets its last kernel row in step m), [1] row m, [2] row m+1
    f4 acc[3][2][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[a][mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    // lanes whose HR column 2q+c lies outside the image hold the conv's zero padding
    bool col_ok[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int X = 2 * (x0 - 1 + 16 * nt + l15) + c;
        col_ok[nt] = X >= 0 && X < 2 * w;
    }

    for (int m = r0 - 1; m <= r1; ++m) {
        const u4v nxt = fetch_lr(m + 2);
        const bool pair_ok = m >= 0 && m < h;   // (uniform) pairs outside the image are the conv's zero padding
        // POST: the 1x1 of row m-3 (reduced at the end of step m-2: in orow since the barrier of step m-1) at the HEAD of the step, where its
        // LDS round trip and the MFMA's latency lie under the deconvolution's; at the end of the step it was a serial tail (+ 12 %)
        if (FLAT || pair_ok) {
            // ---- deconv of HR row 2m+r, columns 2q+c: 9 taps
            f4 d[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) d[mt][nt] = bup(mt);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const unsigned char* rowp = lrr + lr_slot(m + 1 - dy);
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    h8 B[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) B[nt] = *reinterpret_cast<const h8*>(rowp + lr_off(16 * nt + l15 + 2 - dx, g));
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) d[mt][nt] = mfma16(Aup[dy * 3 + dx][mt], B[nt], d[mt][nt]);
                }
            }
            // ---- PReLU -> 1x1 (accumulator tile as B operand) -> PReLU
            h8 T[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const h8 a1 = act_pack(d[0][nt], d[1][nt], a_up2, up_max);
                const f4 e0 = mfma16(adt(0), a1, bdt(0));
                const f4 e1 = mfma16(adt(1), a1, bdt(1));
                h8 t = act_pack(e0, e1, a_dt2, dt_max);
                if (!col_ok[nt] || (FLAT && !pair_ok)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[e] = (_Float16)0.0f;
                }
                T[nt] = t;
            }
            // ---- down conv from registers: kernel rows r, r+2, r+4 (output rows m+1, m, m-1), kernel columns c + 2 s
            h8 B[2];
            shift_tiles<0>(T, B);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[2 - k][mt][nt] = mfma16(Adn[k][0][mt], B[nt], acc[2 - k][mt][nt]);
            shift_tiles<1>(T, B);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[2 - k][mt][nt] = mfma16(Adn[k][1][mt], B[nt], acc[2 - k][mt][nt]);
            shift_tiles<2>(T, B);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[2 - k][mt][nt] = mfma16(Adn[k][2][mt], B[nt], acc[2 - k][mt][nt]);
        }
        // ---- output row m-1 has all its kernel rows: partial tile of this wave -> LDS; rotate the accumulator sets
        const bool row_out = (m - 1 >= r0) && (m - 1 < r1);
        unsigned char* const pbase = part + (m & 1) * S30_PART_BUF;
        if (FLAT || row_out) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    *reinterpret_cast<f4*>(pbase + part_wr + 64 * mt + 16 * nt * PART_PX_PITCH) = acc[0][mt][nt];
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                acc[0][mt][nt] = acc[1][mt][nt];
                acc[1][mt][nt] = acc[2][mt][nt];
                acc[2][mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        if (lr_loader) *reinterpret_cast<u4v*>(lrr + lr_slot(m + 2) + lr_st) = nxt;   // over row m-2 (last read in step m-1)
        __syncthreads();
        if (FLAT) reduce_store(m - 1, pbase, row_out);
        else if (row_out) reduce_store(m - 1, pbase, true);
        if (POST) post_row(m - 2);   // (reduced at the end of the previous step; rows outside [r0, r1): dropped)
    }
    if (POST) {
        __syncthreads();
        post_row(r1 - 1);
    }
}

}  // namespace

[[maybe_unused]] VSR_TUNABLE g_utd_s2_variant = 0;

extern "C" {

#if VSR_X
int vsr_sr_utd_s2_variant(int v) {
    const int old = g_utd_s2_variant;
    g_utd_s2_variant = v & 1;
    return old;
}
#endif

static int launch_utd_s2(const void* in, const void* blob, void* out, void* out2, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                         vsr_stream_t stream, const char* what) {
    VSR_REQUIRE(in && blob && out, "sr_utd_s2: null pointer");
    VSR_REQUIRE(N > 0 && h > 0 && w > 0 && rows_per_seg > 0 && N <= 65535, "sr_utd_s2: bad shape");
    VSR_REQUIRE((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(blob) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(out2) & 15) == 0, "sr_utd_s2: pointers must be 16-byte aligned");
    if ((size_t)N * h * w * NF * 2 >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "sr_utd_s2: tensors beyond 4 GiB");
    const unsigned strips = vsr::cdiv(w, S30_TX), segs = vsr::cdiv(h, rows_per_seg);
    VSR_REQUIRE(segs <= 65535, "sr_utd_s2: too many row segments");
    typedef void (*kern_t)(const _Float16*, const unsigned char*, _Float16*, int, int, int, _Float16*);
    kern_t k;
    if (out2) k = slopes_le_one ? k_utd_s2<true, false, true> : k_utd_s2<false, false, true>;
    else {
#if VSR_X   // (+ the branch-free "flat" build: bit-identical, measured level; cross-check library only)
        static const kern_t kerns[4] = {k_utd_s2<false, false, false>, k_utd_s2<true, false, false>, k_utd_s2<false, true, false>, k_utd_s2<true, true, false>};
        k = kerns[2 * g_utd_s2_variant + (slopes_le_one ? 1 : 0)];
#else
        k = slopes_le_one ? k_utd_s2<true, false, false> : k_utd_s2<false, false, false>;
#endif
    }
    hipLaunchKernelGGL(k, dim3(strips, segs, N), dim3(256), S2_LDS + (out2 ? S2_LDS_POST : 0), vsr::S(stream),
                       (const _Float16*)in, (const unsigned char*)blob, (_Float16*)out, h, w, rows_per_seg, (_Float16*)out2);
    return vsr::launched(what);
}

int vsr_sr_utd_s2_f16(const void* in, const void* blob, void* out, int N, int h, int w, int rows_per_seg, int slopes_le_one,
                      vsr_stream_t stream) {
    return launch_utd_s2(in, blob, out, nullptr, N, h, w, rows_per_seg, slopes_le_one, stream, "sr_utd_s2");
}

int vsr_sr_utd_s2_post_f16(const void* in, const void* blob, void* out, void* out_post, int N, int h, int w, int rows_per_seg,
                           int slopes_le_one, vsr_stream_t stream) {
    VSR_REQUIRE(out_post, "sr_utd_s2_post: null pointer");
    return launch_utd_s2(in, blob, out, out_post, N, h, w, rows_per_seg, slopes_le_one, stream, "sr_utd_s2_post");
}

}  // extern "C"

namespace vsr { size_t utd_s2_blob_bytes() { return S2_BLOB_BYTES; }  int utd_s2_strip_width() { return S30_TX; } }
