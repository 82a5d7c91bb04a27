// sr_utd_s3.h -- k_utd_s3 / k_utd_s3_post: the fused  up (deconv k7 s3 p2 + PReLU) -> tran (1x1 + PReLU) -> down (conv k7 s3 p2 + PReLU)
// stage of the FeedbackBlock for the scale-3 extension (SRFBN's (7, 3, 2) row, sr.py:sr_geometry, under the zero-fill
// semantic).  The x3 feature map (9 x h x w x 32 fp16 per plane: 4.2 GB per tensor at LR 720x1280 x 8 planes) never leaves the
// registers; the unfused build (sr.py:_UnfusedStage: nine phase deconvolutions, in-place 1x1, strided convolution on the generic
// kernel) moves it through HBM about four times and is kept as the cross-check.  The kernel text lives here once: sr_utd_s3.hip
// (libvsr_hip_s3.so, include/vsr_hip_s3.h) instantiates the plain build, sr_utd_s3p.hip (libvsr_hip_s3p.so, include/vsr_hip_s3p.h) the
// POST build, which also applies the next group's uptran 1x1 to its finished rows, sr_utd_s3f.hip (libvsr_hip_s3f.so,
// include/vsr_hip_s3f.h) the PRE builds, which evaluate the 1x1 chain that opens a FeedbackBlock step in the LR load path.
//
// Design = k_utd_s2's (sr_utd_s2.hip) with the x3 geometry:
//   * a workgroup of 4 waves marches down a strip of 30 LR columns; step m handles the HR row TRIPLE m (rows 3m, 3m+1, 3m+2)
//     at the 32 deconv positions q = x0-1 .. x0+30 (2 MFMA pixel tiles).  LR rows m-1, m, m+1 sit in a 4-row LDS ring.
//   * tap algebra of (7, 3, 2): HR row 3m+r takes kernel row ky = r + 2 - 3 di from LR row m+di, so r = 0 has ky {2, 5} (di 0, -1),
//     r = 1 has {0, 3, 6} (di +1, 0, -1), r = 2 has {1, 4} (di +1, 0); columns alike.  The nine phases (r, c) have
//     4 6 4 / 6 9 6 / 4 6 4 taps, 49 in all.  The down-convolution mirrors it: HR row 3m+r is kernel row r + 2 - 3 d of output row
//     m+d, HR column 3q+c kernel column c + 2 - 3 e of output pixel q+e.
//   * the imbalance is dealt with by giving the waves phase SETS of equal tap count instead of a row or a column phase each:
//         wave 0: (1,1) (0,0)          9 + 4     = 13 taps
//         wave 1: (0,1) (2,1)          6 + 6     = 12
//         wave 2: (1,0) (1,2)          6 + 6     = 12
//         wave 3: (0,2) (2,0) (2,2)    4 + 4 + 4 = 12
//     Three waves by row phase would carry 14 / 21 / 14 taps (the middle wave 1.5x the others, one SIMD idle); padding every phase
//     to 3 x 3 taps with zero weights would pay 81 / 49 = 1.65x the MFMAs.  The sets cost nothing but four specialisations of
//     the step body, chosen by a wave-uniform switch.
//   * per phase a wave deconvolves its HR row at its 32 columns (B operand = LR pixels from the ring, A = weights in
//     registers, bias-seeded accumulators), applies PReLU, the 1x1 with the accumulator tile re-used in place as its B operand
//     (channel order permuted consistently in the packed weights), PReLU, zeroes the lanes outside the image (the conv's zero
//     padding), and convolves the tile as it lies in registers: output rows m+1, m, m-1 (three accumulator sets in flight) and
//     output pixel q+e = the tile shifted by 1 - e lanes (DPP row shifts, as shift_tiles of the x2 kernel).
//   * the output row whose last kernel row was just added (m-1) leaves as 4 partial tiles (one per wave) through LDS, summed
//     in a fixed order + bias + PReLU by all 256 threads.  One barrier per step.  The order of every sum is fixed by (row,
//     strip) alone, so neither the row segmentation nor the planes of a launch change a bit.
// Per step (30 output pixels x 32 channels; 49 taps x 4 = 196 MFMA 16x16x32 each for up and down, 9 x 4 for the 1x1):
//         wave      MFMA up + 1x1 + down      activation VALU (2 act_pack + mask per tile)      DPP (12 per shifted tile pair)
//         0         52 + 8 + 52 = 112         112                                                48
//         1         48 + 8 + 48 = 104         112                                                48
//         2         48 + 8 + 48 = 104         112                                                36
//         3         48 + 12 + 48 = 108        168                                                48
// 428 MFMA per step against 448 if every wave ran at wave 0's count (96 %).
// Weights: 26 (wave 0) / 24 tap fragments of 4 registers for each of the two convolutions = 208 / 192 registers per lane, so the
// kernel runs one wave per SIMD on the 512-register budget (__launch_bounds__(256, 1)); the 1x1's two fragments and the biases
// are read from LDS at use.  The tap fragments are pinned in AGPRs (MFMA reads A from either file) and the file is compiled with
// -amdgpu-mfma-vgpr-form (Makefile) so that MFMA results stay in VGPRs: no v_accvgpr copy in the kernel; and with
// -amdgpu-sched-strategy=max-ilp, which places the activation VALU in the MFMAs' shadow better than the default scheduler (same
// instructions, same bits, 10 % less time).
// As compiled by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage; max / select build): 176 / 170 VGPRs + 208 AGPRs,
// 43 / 48 SGPRs, scratch 0 bytes per lane (no spill), occupancy 1 wave per SIMD; 47,872 bytes of dynamic LDS (ring 8,704 +
// partial tiles 2 x 18,432 + parameters 2,304).
// Measured on an MI355X (tools/utd_s3_time.py): 8 x 720 x 1280 in 1.75 ms = 924 TFLOP/s at 219,136 FLOP per pixel and plane,
// against 7.20 ms of the unfused launches.
#pragma once
#include "sr_s3_taps.h"
#include "sr_strip30.h"

namespace {

constexpr int S3_PAR_BYTES = 256 + 2048;     // b_up[32], b_dt[32] fp32 + the two 1x1 fragments
constexpr int S3_LDS = S30_LR_BYTES + 2 * S30_PART_BUF + S3_PAR_BYTES;
constexpr int S3_LDS_POST = 2 * S30_OROW + 2048 + 256;   // two rows + the uptran 1x1's two fragments + its bias and slope
constexpr int S3_PRE_FRAGS = 10;                         // PRE: co (2 inputs x 2 tiles), ci (feat half, chained half), ut0: A fragments of 1 KiB
constexpr int S3_LDS_PRE = S3_PRE_FRAGS * 1024 + 512;   // + b_co[32] b_ci[32] b_ut0[32] fp32 (the slopes are read from the blob)
static_assert(S3_LDS + S3_LDS_POST + S3_LDS_PRE <= 64 * 1024, "dynamic LDS without the large-LDS attribute");

constexpr int S3_SLOTS = 13;                                      // tap fragments per wave and convolution (waves 1-3 use 12)
constexpr int S3_BLOB_UP = 0;                                     // [wave 4][slot 13][mt 2][lane 64][8] fp16
constexpr int S3_BLOB_DN = 4 * S3_SLOTS * 2 * 1024;               // [wave 4][slot 13][mt 2][lane 64][8] fp16
constexpr int S3_BLOB_DT = 2 * S3_BLOB_DN;                        // [mt 2][lane 64][8] fp16
constexpr int S3_BLOB_F32 = S3_BLOB_DT + 2 * 1024;                // b_up[32] b_dt[32] b_dn[32] slope_up slope_dt slope_dn
constexpr int S3_BLOB_BYTES = S3_BLOB_F32 + 512;
constexpr int S3_BLOB_POST = S3_BLOB_BYTES;                       // POST: [mt 2][lane 64][8] fp16 (natural channel order), then b_post[32], slope_post (64 floats)
constexpr int S3_BLOB_POST_BYTES = S3_BLOB_POST + 2048 + 256;
// PRE: 12 fragments [lane 64][8] fp16 -- co input a (mt 0, 1), co input b, ci feat half, ci chained half (accumulator channel order),
// ut0 (accumulator order), ci second half in NATURAL order (PRE2: both halves multiply feat as it lies in memory) -- then b_co[32]
// b_ci[32] b_ut0[32] slope_co slope_ci slope_ut0 (128 floats)
constexpr int S3_BLOB_PRE = S3_BLOB_POST_BYTES;
constexpr int S3_BLOB_PRE_F32 = S3_BLOB_PRE + 12 * 1024;
constexpr int S3_BLOB_PRE_BYTES = S3_BLOB_PRE_F32 + 512;

// POST: the NEXT group's uptran slice (1x1 + PReLU on this stage's output) applied to every finished output row inside the launch and
// written to `out2`, as k_utd_s2<.., POST> does (sr_utd_s2.hip).  The reduce leaves the row's fp16 values in LDS as well (orow, two
// buffers); after the next barrier each wave multiplies one 16 x 16 quadrant (out-channel tile wv / 2, pixel tile wv % 2): 1 MFMA +
// 6 VALU per wave and step, outside the per-role switch.  Same operation order as k_chain1x1_s (bias-seeded accumulator, K = 32 in
// one MFMA, fp16 PReLU): bit-identical to the chain launch it replaces.  POST = false compiles to the kernel without any of it.
//
// PRE: the 1x1 chain that opens a FeedbackBlock step, applied in the LR load path instead of a launch of its own (k_chain1x1_s).  `in`
// is then `feat`, and the value written into the ring for LR pixel p is
//     PRE3 (pa != nullptr; steps >= 1):  ut0(ci(feat[p], co(pa[p], pb[p], cmap[p])))        cmap: [h w, 32] fp32, shared by the planes
//     PRE2 (pa == nullptr; step 0):      ut0(ci(feat[p], feat[p]))
// in k_chain1x1_s's own order of operations: per 1x1 a bias-seeded fp32 accumulator (+ cmap for co), the memory-input MFMAs t = 0, 1
// (K = 32 in one MFMA per out-channel tile), the MFMA on the previous 1x1's activated tile used in place as B operand, act_pack (round
// to fp16, PReLU in fp16).  Bit-identical to the chain launch.  The 34 staged columns are three 16-pixel MFMA tiles (the third with two
// live columns); wave 1 + T carries tile T: lane (l15, g) fetches the 16-byte chunk g of pixel 16 T + l15 of each input at the start
// of a step (as `nxt` of the plain build), runs the chain after its compute and writes its two 8-byte pieces (channels 4g .. 4g+3 and
// 16+4g .. 16+4g+3) into the ring before the step's barrier.  Pixels outside the image put ZEROS into the ring (the deconvolution's
// zero padding), not the chain's value of zero operands.  Per step and wave: PRE3 4 + 4 + 2 = 10 MFMAs, PRE2 2 + 2 + 2 = 6:
//         wave      plain     + PRE3     + PRE2          (+ 1 each with POST)
//         0         112       112        112
//         1         104       114        110
//         2         104       114        110
//         3         108       118        114
// PRE = false compiles to the kernels without any of it.
struct S3PreOps {
    u4v f, a, b;
    f4 cm[2];
};

template <bool ALLMAX, bool POST, bool PRE = false>
__device__ __forceinline__ void utd_s3_body(const _Float16* __restrict__ in, const unsigned char* __restrict__ blob, _Float16* __restrict__ out,
                                            int h, int w, int rows_per_seg, _Float16* __restrict__ out2,
                                            const _Float16* __restrict__ pa = nullptr, const _Float16* __restrict__ pb = nullptr,
                                            const float* __restrict__ cmap = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const lrr = smem;
    unsigned char* const part = smem + S30_LR_BYTES;
    [[maybe_unused]] unsigned char* const orow = smem + S3_LDS;   // (POST only: the launch allocates S3_LDS + S3_LDS_POST)
    [[maybe_unused]] unsigned char* const postw = orow + 2 * S30_OROW;
    [[maybe_unused]] unsigned char* const prew = smem + S3_LDS + (POST ? S3_LDS_POST : 0);   // (PRE only: + S3_LDS_PRE)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * S30_TX;
    const int n = blockIdx.z;
    const int r0 = blockIdx.y * rows_per_seg;
    const int r1 = min(h, r0 + rows_per_seg);
    if (r0 >= r1) return;   // uniform per workgroup

    // ---- weights -> registers, once per workgroup (slot 12 of waves 1-3 is zero padding that no step reads)
    h8 Aup[S3_SLOTS][2], Adn[S3_SLOTS][2];
#pragma unroll
    for (int t = 0; t < S3_SLOTS; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            Aup[t][mt] = *reinterpret_cast<const h8*>(blob + S3_BLOB_UP + (((wv * S3_SLOTS + t) * 2 + mt) * 64 + lane) * 16);
            Adn[t][mt] = *reinterpret_cast<const h8*>(blob + S3_BLOB_DN + (((wv * S3_SLOTS + t) * 2 + mt) * 64 + lane) * 16);
            // the tap fragments live in AGPRs (MFMA reads A from either file), everything the VALU touches in VGPRs: pinning the class
            // here keeps hipcc from parking fragments in VGPRs first and copying the rest out of AGPRs per use
            asm volatile("" : "+a"(Aup[t][mt]));
            asm volatile("" : "+a"(Adn[t][mt]));
        }
    const float* fpar = reinterpret_cast<const float*>(blob + S3_BLOB_F32);
    float* const bias_s = reinterpret_cast<float*>(smem + S30_LR_BYTES + 2 * S30_PART_BUF);
    if (tid < 64) bias_s[tid] = fpar[tid];   // (visible after the prologue's barrier)
    unsigned char* const adt_s = smem + S30_LR_BYTES + 2 * S30_PART_BUF + 256;
    if (tid < 128) *reinterpret_cast<u4v*>(adt_s + tid * 16) = *reinterpret_cast<const u4v*>(blob + S3_BLOB_DT + tid * 16);
    auto adt = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const h8*>(adt_s + (mt * 64 + lane) * 16); };
    // this lane's accumulator rows are channels {4g..4g+3} of tile mt
    auto bup = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(bias_s + 16 * mt + 4 * g); };
    auto bdt = [&](int mt) __attribute__((always_inline)) { return *reinterpret_cast<const f4*>(bias_s + 32 + 16 * mt + 4 * g); };
    const float a_up = fpar[96], a_dt = fpar[97], a_dn = fpar[98];
    const h2 a_up2 = {(_Float16)a_up, (_Float16)a_up}, a_dt2 = {(_Float16)a_dt, (_Float16)a_dt};
    const bool up_max = ALLMAX || a_up <= 1.0f, dt_max = ALLMAX || a_dt <= 1.0f;
    [[maybe_unused]] h2 a_post2 = {(_Float16)1.0f, (_Float16)1.0f};
    [[maybe_unused]] bool post_max = true;
    if constexpr (POST) {
        const float* ppar = reinterpret_cast<const float*>(blob + S3_BLOB_POST + 2048);
        if (tid < 128) *reinterpret_cast<u4v*>(postw + tid * 16) = *reinterpret_cast<const u4v*>(blob + S3_BLOB_POST + tid * 16);
        else if (tid < 160) *reinterpret_cast<float*>(postw + 2048 + (tid - 128) * 4) = ppar[tid - 128];   // (visible after the prologue's barrier)
        a_post2 = h2{(_Float16)ppar[32], (_Float16)ppar[32]};
        post_max = ALLMAX || ppar[32] <= 1.0f;
    }

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

    // ---- PRE: the folded chain.  Waves 1-3, pixel tile wv - 1 of the staged columns; lane = MFMA operand lane (pixel l15, chunk g)
    [[maybe_unused]] const bool pre3 = PRE && pa != nullptr;
    [[maybe_unused]] const int pre_px = PRE ? 16 * (wv - 1) + l15 : 0, pre_col = PRE ? x0 - 2 + pre_px : 0;
    [[maybe_unused]] const bool pre_lane = PRE && wv >= 1 && pre_px < S30_LRC;
    [[maybe_unused]] const bool pre_col_ok = pre_lane && pre_col >= 0 && pre_col < w;
    [[maybe_unused]] h2 a_co2 = {(_Float16)1.0f, (_Float16)1.0f}, a_ci2 = a_co2, a_ut2 = a_co2;
    [[maybe_unused]] bool co_max = true, ci_max = true, ut_max = true;
    [[maybe_unused]] __amdgpu_buffer_rsrc_t a_rsrc = in_rsrc, b_rsrc = in_rsrc, cm_rsrc = in_rsrc;
    if constexpr (PRE) {
        const unsigned char* const src = blob + S3_BLOB_PRE;
        for (int i = tid; i < S3_PRE_FRAGS * 64; i += 256) {
            int f = i >> 6;
            if (!pre3 && (f == 6 || f == 7)) f += 4;   // PRE2: the second half of ci in natural channel order (its B operand is feat)
            *reinterpret_cast<u4v*>(prew + i * 16) = *reinterpret_cast<const u4v*>(src + (f * 64 + (i & 63)) * 16);
        }
        const float* qpar = reinterpret_cast<const float*>(blob + S3_BLOB_PRE_F32);
        if (tid < 96) *reinterpret_cast<float*>(prew + S3_PRE_FRAGS * 1024 + tid * 4) = qpar[tid];
        a_co2 = h2{(_Float16)qpar[96], (_Float16)qpar[96]};
        a_ci2 = h2{(_Float16)qpar[97], (_Float16)qpar[97]};
        a_ut2 = h2{(_Float16)qpar[98], (_Float16)qpar[98]};
        co_max = ALLMAX || qpar[96] <= 1.0f, ci_max = ALLMAX || qpar[97] <= 1.0f, ut_max = ALLMAX || qpar[98] <= 1.0f;
        if (pre3) {
            a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(pa), 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
            b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(pb), 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
            cm_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(cmap), 0, (int)((size_t)h * w * NF * 4), 0x00020000);
        }
    }
    // out-of-image pixels (and the lanes of the third tile beyond column 33) read zeros: out-of-range buffer offsets
    [[maybe_unused]] auto fetch_pre = [&](int row) __attribute__((always_inline)) -> S3PreOps {
        const bool ok = pre_col_ok && row >= 0 && row < h;
        const unsigned off = ok ? (unsigned)(((((size_t)n * h + row) * w + pre_col) * NF + g * 8) * 2) : 0xFFFFFFFFu;
        S3PreOps o;
        o.f = __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off, 0, 0);
        if (pre3) {
            o.a = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, off, 0, 0);
            o.b = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, off, 0, 0);
            // this lane's accumulator rows: channels 4g .. 4g+3 of tile mt
            const unsigned c0 = ok ? (unsigned)((((size_t)row * w + pre_col) * NF + 4 * g) * 4) : 0xFFFFFFFFu;
            const unsigned c1 = ok ? c0 + 64u : 0xFFFFFFFFu;
            o.cm[0] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(cm_rsrc, c0, 0, 0));
            o.cm[1] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(cm_rsrc, c1, 0, 0));
        } else {
            o.a = o.b = u4v{0u, 0u, 0u, 0u};
            o.cm[0] = o.cm[1] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        return o;
    };
    [[maybe_unused]] auto pre_frag = [&](int f) __attribute__((always_inline)) { return *reinterpret_cast<const h8*>(prew + (f * 64 + lane) * 16); };
    [[maybe_unused]] auto pre_bias = [&](int s, int mt) __attribute__((always_inline)) {
        return *reinterpret_cast<const f4*>(prew + S3_PRE_FRAGS * 1024 + (32 * s + 16 * mt + 4 * g) * 4);
    };
    // the chain on the fetched operands of LR row `row` -> ring (two 8-byte pieces in natural channel order)
    [[maybe_unused]] auto pre_row = [&](const S3PreOps& o, int row) __attribute__((always_inline)) {
        const h8 f = __builtin_bit_cast(h8, o.f);
        h8 prev = f;   // (PRE2: ci's second input is feat itself)
        f4 c0, c1;
        if (pre3) {
            c0 = pre_bias(0, 0);
            c1 = pre_bias(0, 1);
            c0 += o.cm[0];
            c1 += o.cm[1];
            const h8 ia = __builtin_bit_cast(h8, o.a), ib = __builtin_bit_cast(h8, o.b);
            c0 = mfma16(pre_frag(0), ia, c0);
            c1 = mfma16(pre_frag(1), ia, c1);
            c0 = mfma16(pre_frag(2), ib, c0);
            c1 = mfma16(pre_frag(3), ib, c1);
            prev = act_pack(c0, c1, a_co2, co_max);
        }
        c0 = mfma16(pre_frag(4), f, pre_bias(1, 0));
        c1 = mfma16(pre_frag(5), f, pre_bias(1, 1));
        c0 = mfma16(pre_frag(6), prev, c0);
        c1 = mfma16(pre_frag(7), prev, c1);
        prev = act_pack(c0, c1, a_ci2, ci_max);
        c0 = mfma16(pre_frag(8), prev, pre_bias(2, 0));
        c1 = mfma16(pre_frag(9), prev, pre_bias(2, 1));
        prev = act_pack(c0, c1, a_ut2, ut_max);
        u4v v = __builtin_bit_cast(u4v, prev);
        if (!(pre_col_ok && row >= 0 && row < h)) v = u4v{0u, 0u, 0u, 0u};   // the deconvolution's zero padding
        if (pre_lane) {
            typedef unsigned int u2p __attribute__((ext_vector_type(2)));
            unsigned char* const rp = lrr + lr_slot(row) + (g & 1) * 8;
            *reinterpret_cast<u2p*>(rp + lr_off(pre_px, g >> 1)) = u2p{v[0], v[1]};
            *reinterpret_cast<u2p*>(rp + lr_off(pre_px, 2 + (g >> 1))) = u2p{v[2], v[3]};
        }
    };

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
    auto reduce_store = [&](int i, const unsigned char* pbase) __attribute__((always_inline)) {
        f4 s = *reinterpret_cast<const f4*>(pbase + part_rd);
#pragma unroll
        for (int k = 1; k < 4; ++k) s += *reinterpret_cast<const f4*>(pbase + part_rd + k * S30_PART_W);
        s += bdn;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s[e] >= 0.0f ? s[e] : s[e] * a_dn;
        const unsigned lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[0], v[1]}, h2));
        const unsigned hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[2], v[3]}, h2));
        const unsigned off = red_ok ? (unsigned)(((((size_t)n * h + i) * w + x0 + rj) * NF + 4 * rc4) * 2) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b64(u2v{lo, hi}, out_rsrc, off, 0, 0);
        if constexpr (POST) *reinterpret_cast<u2v*>(orow + (i & 1) * S30_OROW + lr_off(rj, rc4 >> 1) + (rc4 & 1) * 8) = u2v{lo, hi};
    };
    // POST: the 1x1 on finished row i (its fp16 values lie in orow[i & 1] since the barrier that followed its reduce): this wave's quadrant;
    // dead pixels and rows outside [r0, r1) store to an out-of-range buffer offset (dropped)
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t out2_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(POST ? out2 : out, 0, (int)((size_t)gridDim.z * h * w * NF * 2), 0x00020000);
    [[maybe_unused]] const int pmt = wv >> 1, ppx = 16 * (wv & 1) + l15;
    [[maybe_unused]] const bool post_px_ok = ppx < S30_TX && x0 + ppx < w;
    [[maybe_unused]] auto post_row = [&](int i) __attribute__((always_inline)) {
        const h8 b = *reinterpret_cast<const h8*>(orow + (i & 1) * S30_OROW + lr_off(ppx, g));
        const h8 a = *reinterpret_cast<const h8*>(postw + (pmt * 64 + lane) * 16);
        const f4 e = mfma16(a, b, *reinterpret_cast<const f4*>(postw + 2048 + (16 * pmt + 4 * g) * 4));
        const h2 p0 = prelu_h2(__builtin_convertvector(f2v{e[0], e[1]}, h2), a_post2, post_max);
        const h2 p1 = prelu_h2(__builtin_convertvector(f2v{e[2], e[3]}, h2), a_post2, post_max);
        const unsigned off = (post_px_ok && i >= r0 && i < r1) ? (unsigned)(((((size_t)n * h + i) * w + x0 + ppx) * NF + 16 * pmt + 4 * g) * 2) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b64(u2v{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)}, out2_rsrc, off, 0, 0);
    };

    // ---- prologue: LR rows r0-2, r0-1, r0 (the first triple, m = r0-1, reads them)
    if constexpr (PRE) {
        __syncthreads();   // the chain's fragments and biases are in LDS
        if (wv >= 1) {
            const S3PreOps o0 = fetch_pre(r0 - 2), o1 = fetch_pre(r0 - 1), o2 = fetch_pre(r0);
            pre_row(o0, r0 - 2);
            pre_row(o1, r0 - 1);
            pre_row(o2, r0);
        }
    } else if (lr_loader) {
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0 - 2) + lr_st) = fetch_lr(r0 - 2);
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0 - 1) + lr_st) = fetch_lr(r0 - 1);
        *reinterpret_cast<u4v*>(lrr + lr_slot(r0) + lr_st) = fetch_lr(r0);
    }
    __syncthreads();

    // accumulators of the three output rows in flight: [0] row m-1 (gets its last kernel rows in step m), [1] row m, [2] row m+1
    f4 acc[3][2][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[a][mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    // lanes whose deconv position q lies outside the image (HR columns 3q .. 3q+2) hold the conv's zero padding
    bool col_ok[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int q = x0 - 1 + 16 * nt + l15;
        col_ok[nt] = q >= 0 && q < w;
    }

    // ---- one step of wave role WV: its phases' deconv -> PReLU -> 1x1 -> PReLU -> down conv into the three accumulator sets
    auto compute = [&](auto role, int m) __attribute__((always_inline)) {
        constexpr int WV = decltype(role)::value;
#pragma unroll
        for (int p = 0; p < ph_cnt(WV); ++p) {
            const int r = ph_r(WV, p), c = ph_c(WV, p);
            f4 d[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) d[mt][nt] = bup(mt);
#pragma unroll
            for (int di = 1; di >= -1; --di) {
                if (!tap_ok(r, di)) continue;
                const unsigned char* rowp = lrr + lr_slot(m + di);
#pragma unroll
                for (int dj = 1; dj >= -1; --dj) {
                    if (!tap_ok(c, dj)) continue;
                    const int slot = tap_slot(WV, p, di, dj);
                    h8 B[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) B[nt] = *reinterpret_cast<const h8*>(rowp + lr_off(16 * nt + l15 + 1 + dj, g));
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) d[mt][nt] = mfma16(Aup[slot][mt], B[nt], d[mt][nt]);
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
                if (!col_ok[nt]) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[e] = (_Float16)0.0f;
                }
                T[nt] = t;
            }
            // ---- down conv from registers: kernel column c + 2 - 3 e of output pixel q + e (tile shifted 1 - e lanes), kernel row
            // r + 2 - 3 dd of output row m + dd
#pragma unroll
            for (int e = 1; e >= -1; --e) {
                if (!tap_ok(c, e)) continue;
                h8 B[2];
                if (e == 1) shift_tiles<0>(T, B);
                else if (e == 0) shift_tiles<1>(T, B);
                else shift_tiles<2>(T, B);
#pragma unroll
                for (int dd = 1; dd >= -1; --dd) {
                    if (!tap_ok(r, dd)) continue;
                    const int slot = tap_slot(WV, p, dd, e);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[dd + 1][mt][nt] = mfma16(Adn[slot][mt], B[nt], acc[dd + 1][mt][nt]);
                }
            }
        }
    };

    for (int m = r0 - 1; m <= r1; ++m) {
        [[maybe_unused]] u4v nxt;
        [[maybe_unused]] S3PreOps pnxt;
        if constexpr (PRE) {
            if (wv >= 1) pnxt = fetch_pre(m + 2);
        } else {
            nxt = fetch_lr(m + 2);
        }
        if (m >= 0 && m < h) {   // (uniform) triples outside the image are the conv's zero padding
            switch (wv) {
                case 0: compute(IntC<0>{}, m); break;
                case 1: compute(IntC<1>{}, m); break;
                case 2: compute(IntC<2>{}, m); break;
                default: compute(IntC<3>{}, m); break;
            }
        }
        // ---- output row m-1 has all its kernel rows: partial tile of this wave -> LDS; rotate the accumulator sets
        const bool row_out = (m - 1 >= r0) && (m - 1 < r1);
        unsigned char* const pbase = part + (m & 1) * S30_PART_BUF;
        if (row_out) {
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
        if constexpr (PRE) {
            if (wv >= 1) pre_row(pnxt, m + 2);   // over row m-2 (last read in step m-1)
        } else if (lr_loader) {
            *reinterpret_cast<u4v*>(lrr + lr_slot(m + 2) + lr_st) = nxt;   // over row m-2 (last read in step m-1)
        }
        __syncthreads();
        if (row_out) reduce_store(m - 1, pbase);
        // POST: row m-2 was reduced at the end of the previous step and lies in orow since this step's barrier; its 1x1 is issued here, after
        // the barrier and the reduce, before the next step's first MFMAs, common to all wave roles (rows outside [r0, r1): dropped)
        if constexpr (POST) post_row(m - 2);
    }
    if constexpr (POST) {   // the segment's last row (a one-row segment's only row)
        __syncthreads();
        post_row(r1 - 1);
    }
}

template <bool ALLMAX>
__global__ void __launch_bounds__(256, 1)
k_utd_s3(const _Float16* __restrict__ in, const unsigned char* __restrict__ blob, _Float16* __restrict__ out, int h, int w,
         int rows_per_seg) {
    utd_s3_body<ALLMAX, false>(in, blob, out, h, w, rows_per_seg, nullptr);
}

template <bool ALLMAX>
__global__ void __launch_bounds__(256, 1)
k_utd_s3_post(const _Float16* __restrict__ in, const unsigned char* __restrict__ blob, _Float16* __restrict__ out, int h, int w,
              int rows_per_seg, _Float16* __restrict__ out2) {
    utd_s3_body<ALLMAX, true>(in, blob, out, h, w, rows_per_seg, out2);
}

// PRE builds (libvsr_hip_s3f.so): `feat` in place of the stage's input, the step-opening 1x1 chain in the load path (pa == nullptr: PRE2)
template <bool ALLMAX, bool POST>
__global__ void __launch_bounds__(256, 1)
k_utd_s3_pre(const _Float16* __restrict__ feat, const _Float16* __restrict__ pa, const _Float16* __restrict__ pb, const float* __restrict__ cmap,
             const unsigned char* __restrict__ blob, _Float16* __restrict__ out, int h, int w, int rows_per_seg, _Float16* __restrict__ out2) {
    utd_s3_body<ALLMAX, POST, true>(feat, blob, out, h, w, rows_per_seg, out2, pa, pb, cmap);
}

// ---- host: what the three stage entries (sr_utd_s3.hip, sr_utd_s3p.hip, sr_utd_s3f.hip) check before they launch, and their grid
struct S3Buf {
    const void* p;
    size_t bytes;
    bool may_be_null;
};

// `what`: the entry's name in the messages; bufs: every buffer of the call with its length in bytes.  0 and `grid` (strips, row segments,
// planes) / `rows_per_seg` (0 -> h: one march per strip) when the call may launch, else the error code with the message set.  Overlap is
// refused on the byte ranges of EVERY pair of buffers given, after the size checks (which bound the ranges).
inline int s3_stage_args(const char* what, const S3Buf* bufs, int nbufs, int N, int h, int w, int& rows_per_seg, dim3& grid) {
    for (int i = 0; i < nbufs; ++i) VSR_REQUIRE(bufs[i].p || bufs[i].may_be_null, "%s: null pointer", what);
    VSR_REQUIRE(N > 0 && h > 0 && w > 0 && rows_per_seg >= 0 && N <= 65535, "%s: bad shape (N %d, h %d, w %d, rows_per_seg %d)", what, N, h, w,
                rows_per_seg);
    for (int i = 0; i < nbufs; ++i)
        VSR_REQUIRE((reinterpret_cast<uintptr_t>(bufs[i].p) & 15) == 0, "%s: pointers must be 16-byte aligned", what);
    if ((size_t)N * h * w * NF * 2 >= (1ull << 32) - 16) return vsr::fail(VSR_E_UNSUPPORTED, "%s: tensors beyond 4 GiB (split the planes)", what);
    if (rows_per_seg == 0) rows_per_seg = h;
    const unsigned strips = vsr::cdiv(w, S30_TX), segs = vsr::cdiv(h, rows_per_seg);
    VSR_REQUIRE(segs <= 65535, "%s: too many row segments", what);
    for (int i = 0; i < nbufs; ++i)
        for (int j = i + 1; j < nbufs; ++j)
            VSR_REQUIRE(!bufs[i].p || !bufs[j].p || !ranges_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes),
                        "%s: the buffers of a call must not overlap", what);
    grid = dim3(strips, segs, N);
    return VSR_OK;
}

}  // namespace
