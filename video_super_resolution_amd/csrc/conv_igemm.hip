// conv_igemm.hip -- generic NHWC fp16 convolution on MFMA (implicit GEMM, no im2col buffer) for the guidance trunks
// (FlowNet2, depth hourglass, OSVOS: reference models.py / networks/*.py, pytorch_DIW_scratch.py, vgg_osvos.py).
//
// GEMM view: rows = out-channels (A operand = weights), columns = output pixels (B operand = input pixels gathered
// per tap), K = taps x input channels walked as (tap, 32-channel chunk) steps.  With the out-channels on the MFMA
// rows each lane ends up with 4 consecutive channels of one pixel -> 8-byte NHWC stores.
//   workgroup: 128 output pixels x BN out-channels (BN = 64 / 32 / 16), 4 waves, wave w owns pixels [32w, 32w+32)
//   K step = two (tap, chunk) pairs (64 K elements) per barrier; LDS: double-buffered, per pair a weight tile [BN][32]
//        and a pixel tile [128][32] (64-byte rows, chunk index XOR row bits 1-2:
//        conflict-free ds_read_b128 for the 16x16x32 operand pattern, same scheme as the LR ring of k_utd)
//   one barrier per K step: global loads of step s+1 are in flight while step s is multiplied
// The K walk shared with conv_tile.hip (split-K range, table, pixel origin) is conv_kwalk.h; the patch kernels' vocabulary conv_patch.h.
// Epilogue: + bias (fp32), none / ReLU / LeakyReLU, fp16 store into a channel slice [out_coff, out_coff+Cout) of a
// tensor with out_ld channels (concatenations are written in place), with an output pixel stride/offset so the four
// phases of a k4 s2 transposed convolution are four ordinary 2x2-tap launches.
#include "conv_common.h"
#include "conv_kwalk.h"
#include "conv_patch.h"

namespace {

using vsrc::h8;
using vsrc::h4;
using vsrc::f4;
using vsrc::BM;
using vsrc::ConvP;
using vsrc::sw_off;
using vsrc::u4;
using vsrc::u2;
using vsrc::dma16;
using vsrc::patch_epilogue;
using vsrc::patch_epilogue_act;
using vsrc::patch_pixoff;
using vsrc::stage_patch;
using vsrc::patch_pieces;
using vsrc::stage_patch_cached;
using vsrc::PT_H;
using vsrc::PT_W;

struct C0 { static constexpr int value = 0; };
struct C1 { static constexpr int value = 1; };
struct C2 { static constexpr int value = 2; };
struct C3 { [[maybe_unused]] static constexpr int value = 3; };   // (sets 3 and 4: the five-set ring of the cross-check library)
struct C4 { [[maybe_unused]] static constexpr int value = 4; };


// Epilogue of the gather kernels.  This lane holds channels co0 + 16 mt + 4 g + {0..3} of pixels 32 wv + 16 nt + l15 (straight
// from the MFMA layout: the LDS-transposed epilogue of the patch kernels was measured here too and loses 10-25 % on these
// shorter, lower-resolution launches).  Split-K: the fp32 partial tile for k_splitk_finish.  The activation is a template
// constant (tested per value at run time it compiled to scalar branches per output value) and the bias is read as one 16-byte
// piece per out-channel tile.
template <int BN, int ACT>
__device__ __forceinline__ void gather_store(const ConvP& p, const f4 (&acc)[BN / 16][2], long long M, long long m0, int co0, int tid, int zsplit,
                                             int ph, int oy_off, int ox_off) {
    constexpr int MT = BN / 16;
    const int lane = tid & 63, wv = tid >> 6, l15 = lane & 15, g = lane >> 4;
    if (p.splits > 1) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const long long m = m0 + 32 * wv + 16 * nt + l15;
            if (m >= M) continue;
            float* wsp = p.ws + (((size_t)zsplit * (p.nphase > 1 ? 4 : 1) + ph) * M + m) * p.cout_pad + co0;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f4*>(wsp + 16 * mt + 4 * g) = acc[mt][nt];
        }
        return;
    }
    f4 bz[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)   // (bias: cout_pad floats, 16-byte aligned pieces)
        bz[mt] = p.bias ? *reinterpret_cast<const f4*>(p.bias + co0 + 16 * mt + 4 * g) : f4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool vec_ok = (p.out_coff & 3) == 0 && (p.out_ld & 3) == 0;   // (co0 + 16 mt + 4 g is a multiple of 4)
    const unsigned HoWo = (unsigned)(p.Ho * p.Wo);   // (M < 2^31: checked by the launchers; 32-bit divisions)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const long long m = m0 + 32 * wv + 16 * nt + l15;
        if (m >= M) continue;
        const int n = (int)((unsigned)m / HoWo);
        const int rem = (int)((unsigned)m - (unsigned)n * HoWo);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        _Float16* dst = p.out + (((size_t)n * p.outH + oy * p.oy_mul + oy_off) * p.outW + ox * p.ox_mul + ox_off) * p.out_ld +
                        p.out_coff;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int c = co0 + 16 * mt + 4 * g;
            if (c >= p.cout) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t = acc[mt][nt][r] + bz[mt][r];
                if (ACT == 1) t = fmaxf(t, 0.0f);
                else if (ACT == 2) t = t >= 0.0f ? t : t * p.slope;
                v[r] = t;
            }
            if (vec_ok && c + 4 <= p.cout) {
                *reinterpret_cast<h4*>(dst + c) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c + r < p.cout) dst[c + r] = (_Float16)v[r];
            }
        }
    }
}

// STEM: the input has 4 channels per pixel ([N,H,W,4] fp16, 3 live) and one K chunk is a whole kernel ROW: k = 4 kx + c
// for kx < 8 (packed weights [ky][cout_pad][32], zero where kx >= kw or c >= cin).  A 7x7 stem on an RGB image is 7 K
// chunks instead of 49 chunks that are 29/32 zero padding.
#if VSR_X   // the first gather build (pixel operand through LDS): cross-check library only
template <int BN, bool STEM = false>
__global__ void __launch_bounds__(256) k_conv_igemm(const ConvP p) {
    constexpr int MT = BN / 16;                 // out-channel tiles per wave
    constexpr int A_HALF = BN * 64;             // weight tile of one (tap, chunk)
    constexpr int B_HALF = BM * 64;             // pixel tile of one (tap, chunk)
    constexpr int STAGE = 2 * (A_HALF + B_HALF);  // one K step = two (tap, chunk) pairs = 64 K elements
    constexpr int A_PIECES = A_HALF / 16;       // 16-byte pieces per half
    constexpr int AP = (A_PIECES + 255) / 256;  // ... per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // operand ring [2][STAGE], then the K-walk table
    auto As = [&](int b, int hf) __attribute__((always_inline)) { return smem + b * STAGE + hf * (A_HALF + B_HALF); };
    auto Bs = [&](int b, int hf) __attribute__((always_inline)) { return smem + b * STAGE + hf * (A_HALF + B_HALF) + A_HALF; };
    u4* const tab = reinterpret_cast<u4*>(smem + 2 * STAGE);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const long long m0 = (long long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;
    const int nchunk = STEM ? 1 : p.cin >> 5;
    const int npair = STEM ? p.kh : p.kh * p.kw * nchunk;     // (tap, chunk) pairs; STEM: one per kernel row
    const int nk_all = (npair + 1) >> 1;        // K steps of two pairs (the odd tail pair is zero-filled)
    const vsrc::KRange kr = vsrc::k_range(p, blockIdx.z, nk_all);   // (split-K range and phase: conv_kwalk.h)
    const int ph = kr.ph, zsplit = kr.zsplit, pad_y = kr.pad_y, pad_x = kr.pad_x, oy_off = kr.oy_off, ox_off = kr.ox_off;
    const int ks_per = kr.ks_per, ks0 = kr.ks0, nk = kr.nk;
    const _Float16* const wpk = kr.wpk;

    const __amdgpu_buffer_rsrc_t w_rsrc = vsrc::kwalk_w_rsrc(p, wpk, npair), in_rsrc = vsrc::kwalk_in_rsrc(p);

    vsrc::build_kwalk<STEM>(p, tab, tid, ks0, nk, npair, nchunk, vsrc::kwalk_entries(ks_per, vsrc::KWALK_FIRST_LOOKAHEAD));   // (conv_kwalk.h)

    // ---- the two pixel pieces this thread stages per pair: piece q = tid + 256 r -> row q>>2, chunk piece q&3: four
    //      neighbouring lanes fetch the 64 contiguous bytes of one pixel's chunk (one L1 tag look-up per 64 bytes; in the MFMA
    //      fragment layout of k_conv_igemm_d every lane of a load sits in another cache line)
    const int bchunk = tid & 3;
    const int brow[2] = {tid >> 2, (tid + 256) >> 2};
    int piy0[2], pix0[2];
    unsigned pbase[2];
    bool xok0[2], xok1[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const vsrc::PixOrigin o = vsrc::pixel_origin<STEM>(p, m0 + brow[r], M, pad_y, pad_x, bchunk);
        piy0[r] = o.piy0; pix0[r] = o.pix0; pbase[r] = o.pbase;
        xok0[r] = (unsigned)pix0[r] < (unsigned)p.W;
        xok1[r] = (unsigned)(pix0[r] + 1) < (unsigned)p.W;
    }
    unsigned wlane[AP];
#pragma unroll
    for (int ap = 0; ap < AP; ++ap) wlane[ap] = tid + 256 * ap < A_PIECES ? (unsigned)(co0 * 64 + (tid + 256 * ap) * 16) : 0x40000000u;

    // Global -> register staging, two K steps deep, every load unconditional (out-of-range offsets where a piece does not exist).
    // (gload / lstore / wlane repeat k_conv_igemm_d's text with one set index: as shared functions they changed the K step's
    // register allocation in both kernels, LAB_NOTES.md "Trunk conv kernels".)
    u4 ra[2][2][AP], rb[2][2][2];
    __syncthreads();   // the table
    int q = 0;
    u4 en[2] = {tab[0], tab[1]};
    auto gload = [&](auto setc) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const u4 e = en[hf];
#pragma unroll
            for (int ap = 0; ap < AP; ++ap) ra[S][hf][ap] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, wlane[ap] + e[3], 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool rowok = (unsigned)(piy0[r] + (int)e[1]) < (unsigned)p.H;
                if (STEM) {
                    const u2 t0 = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, rowok && xok0[r] ? pbase[r] + e[0] : 0xFFFFFFFFu, 0, 0);
                    const u2 t1 = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, rowok && xok1[r] ? pbase[r] + e[0] + 8u : 0xFFFFFFFFu, 0, 0);
                    rb[S][hf][r] = u4{t0[0], t0[1], t1[0], t1[1]};
                } else {
                    const bool ok = rowok && (unsigned)(pix0[r] + (int)e[2]) < (unsigned)p.W;
                    rb[S][hf][r] = __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, ok ? pbase[r] + e[0] : 0xFFFFFFFFu, 0, 0);
                }
            }
        }
        q += 2;
        en[0] = tab[q];
        en[1] = tab[q + 1];
    };
    auto lstore = [&](int buf, auto setc) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
            for (int ap = 0; ap < AP; ++ap) {
                const int piece = tid + 256 * ap;
                if (piece < A_PIECES) *reinterpret_cast<u4*>(As(buf, hf) + sw_off(piece >> 2, piece & 3)) = ra[S][hf][ap];
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) *reinterpret_cast<u4*>(Bs(buf, hf) + sw_off(brow[r], bchunk)) = rb[S][hf][r];
        }
    };

    f4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    gload(C0{});
    lstore(ks0 & 1, C0{});
    gload(C1{});
    __syncthreads();
    // step ks: its data is in LDS buffer ks&1, step ks+1 is in register set `other`, step ks+2 is requested into set `mine`
    auto body = [&](int ks, auto mine, auto other) __attribute__((always_inline)) {
        const int buf = ks & 1;
        h8 af[2][MT], bf[2][2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) bf[0][nt] = *reinterpret_cast<const h8*>(Bs(buf, 0) + sw_off(32 * wv + 16 * nt + l15, g));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[0][mt] = *reinterpret_cast<const h8*>(As(buf, 0) + sw_off(16 * mt + l15, g));
        __builtin_amdgcn_sched_barrier(0);
        gload(mine);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) bf[1][nt] = *reinterpret_cast<const h8*>(Bs(buf, 1) + sw_off(32 * wv + 16 * nt + l15, g));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[1][mt] = *reinterpret_cast<const h8*>(As(buf, 1) + sw_off(16 * mt + l15, g));
        __builtin_amdgcn_sched_barrier(0);
        if (ks < nk) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[hf][mt], bf[hf][nt], acc[mt][nt], 0, 0, 0);
        }
        lstore(buf ^ 1, other);
        __syncthreads();
    };
    for (int ks = ks0; ks < nk; ks += 2) {
        body(ks, C0{}, C1{});
        body(ks + 1, C1{}, C0{});
    }

    if (p.splits > 1 || p.act == 0) gather_store<BN, 0>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
    else if (p.act == 1) gather_store<BN, 1>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
    else gather_store<BN, 2>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
}
#endif  // VSR_X


// k_conv_igemm with the PIXEL operand kept out of LDS.  A wave's MFMA B fragments are its own 32 pixels (lane: pixel
// l15 of tile nt, 16-byte channel piece g) and no other wave reads them, so the lanes load them from global memory
// straight in fragment layout -- the same 16-byte pieces the staging threads fetched -- three K steps deep in registers.
// Only the weight tile, shared by the four waves, still goes through LDS.  Per K step the LDS moves 40 KB instead of
// 72 KB against 256 MFMA cycles per wave, which is what bounded the gather kernel (LDS busy ~2x the MFMA time).
template <int BN, bool STEM = false, int D = 3>
__global__ void __launch_bounds__(256) k_conv_igemm_d(const ConvP p) {
    constexpr int MT = BN / 16;                 // out-channel tiles per wave
    constexpr int A_HALF = BN * 64;             // weight tile of one (tap, chunk)
    constexpr int STAGE = 2 * A_HALF;           // one K step = two (tap, chunk) pairs = 64 K elements
    constexpr int A_PIECES = A_HALF / 16;       // 16-byte pieces per half
    constexpr int AP = (A_PIECES + 255) / 256;  // ... per thread (2 for the 128-channel tile)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // weight ring [2][STAGE], then the K-walk table
    auto As = [&](int b, int hf) __attribute__((always_inline)) { return smem + b * STAGE + hf * A_HALF; };
    u4* const tab = reinterpret_cast<u4*>(smem + 2 * STAGE);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const long long m0 = (long long)blockIdx.x * BM;
    const int co0 = blockIdx.y * BN;
    const int nchunk = STEM ? 1 : p.cin >> 5;
    const int npair = STEM ? p.kh : p.kh * p.kw * nchunk;     // (tap, chunk) pairs; STEM: one per kernel row
    const int nk_all = (npair + 1) >> 1;        // K steps of two pairs (the odd tail pair is zero-filled)
    const vsrc::KRange kr = vsrc::k_range(p, blockIdx.z, nk_all);   // (split-K range and phase: conv_kwalk.h)
    const int ph = kr.ph, zsplit = kr.zsplit, pad_y = kr.pad_y, pad_x = kr.pad_x, oy_off = kr.oy_off, ox_off = kr.ox_off;
    const int ks_per = kr.ks_per, ks0 = kr.ks0, nk = kr.nk;
    const _Float16* const wpk = kr.wpk;

    const __amdgpu_buffer_rsrc_t w_rsrc = vsrc::kwalk_w_rsrc(p, wpk, npair), in_rsrc = vsrc::kwalk_in_rsrc(p);

    vsrc::build_kwalk<STEM>(p, tab, tid, ks0, nk, npair, nchunk, vsrc::kwalk_entries(ks_per, vsrc::kwalk_gather_lookahead(D)));   // (conv_kwalk.h)

    // ---- this lane's two pixels (tile r: row 32 wv + 16 r + l15 of the workgroup's 128) and its channel piece g: a 32-bit byte
    //      offset of (pixel, tap (0,0), chunk 0, piece g) -- wrapped modulo 2^32 where the padding makes it negative; adding the
    //      table's tap offset wraps it back -- plus the pixel's first input row / column for the bounds tests
    int piy0[2], pix0[2];
    unsigned pbase[2];
    bool xok0[2], xok1[2];   // STEM: the lane's two taps of a kernel row (columns fixed per lane)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 32 * wv + 16 * r + l15;
        const vsrc::PixOrigin o = vsrc::pixel_origin<STEM>(p, m0 + row, M, pad_y, pad_x, g);
        piy0[r] = o.piy0; pix0[r] = o.pix0; pbase[r] = o.pbase;
        xok0[r] = (unsigned)pix0[r] < (unsigned)p.W;
        xok1[r] = (unsigned)(pix0[r] + 1) < (unsigned)p.W;
    }

    // Global -> register staging, two K steps deep: the loads of step ks+2 are issued at the top of step ks and stored to
    // LDS at the end of step ks+1.  Every load is a buffer load whose offset is out of range when the piece does not
    // exist (padding, tail, idle thread) -- the hardware returns zeros -- so a step issues a FIXED number of loads and
    // hipcc can wait with a vmcnt for the older set only.
    u4 ra[D][2][AP], rb[D][2][2];
    unsigned wlane[AP];   // this thread's piece of a weight slab [cout_pad][32] fp16 (rows co0.. contiguous); an idle thread points past the slabs
#pragma unroll
    for (int ap = 0; ap < AP; ++ap) wlane[ap] = tid + 256 * ap < A_PIECES ? (unsigned)(co0 * 64 + (tid + 256 * ap) * 16) : 0x40000000u;
    __syncthreads();   // the table
    int q = 0;         // table index of the next step's first pair
    u4 en[2] = {tab[0], tab[1]};   // entries of the next request, read one step ahead (a broadcast ds_read_b128 each)
    auto gload = [&](auto setc, auto setb) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value, SB = decltype(setb)::value;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const u4 e = en[hf];
#pragma unroll
            for (int ap = 0; ap < AP; ++ap) ra[S][hf][ap] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, wlane[ap] + e[3], 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool rowok = (unsigned)(piy0[r] + (int)e[1]) < (unsigned)p.H;
                if (STEM) {   // this 16-byte piece = taps kx, kx+1 of kernel row ky: two 8-byte pixels
                    const u2 t0 = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, rowok && xok0[r] ? pbase[r] + e[0] : 0xFFFFFFFFu, 0, 0);
                    const u2 t1 = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, rowok && xok1[r] ? pbase[r] + e[0] + 8u : 0xFFFFFFFFu, 0, 0);
                    rb[SB][hf][r] = u4{t0[0], t0[1], t1[0], t1[1]};
                } else {
                    const bool ok = rowok && (unsigned)(pix0[r] + (int)e[2]) < (unsigned)p.W;
                    rb[SB][hf][r] = __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, ok ? pbase[r] + e[0] : 0xFFFFFFFFu, 0, 0);
                }
            }
        }
        q += 2;
        en[0] = tab[q];
        en[1] = tab[q + 1];
    };
    auto lstore = [&](int buf, auto setc) __attribute__((always_inline)) {
        constexpr int S = decltype(setc)::value;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
            for (int ap = 0; ap < AP; ++ap) {
                const int piece = tid + 256 * ap;
                if (piece < A_PIECES) *reinterpret_cast<u4*>(As(buf, hf) + sw_off(piece >> 2, piece & 3)) = ra[S][hf][ap];
            }
        }
    };

    f4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    // Control flow around the loads is kept UNIFORM: every step requests its six pieces whether or not they exist (steps past
    // the range get out-of-range offsets: zeros, no traffic), the loop runs whole groups of three steps and only the MFMAs of
    // a step past the range are skipped.  With a load under `if (ks + 2 < nk)` the compiler's wait-count pass has to assume
    // the younger loads were skipped and emitted s_waitcnt vmcnt(0) before the MFMAs of every third step -- the pipeline
    // drained, one memory latency exposed per three steps (seen in the ISA; this held the low-resolution layers at ~1 us per
    // K step).
    gload(C0{}, C0{});
    lstore(ks0 & 1, C0{});
    gload(C1{}, C1{});
    if constexpr (D == 5) {
        gload(C2{}, C2{});
        gload(C3{}, C3{});
    }
    __syncthreads();
    // step ks (i = ks - ks0): weights in LDS buffer ks&1, pixels in register set i%3; step ks+1 is in flight (weights in
    // register set (i+1)%3, pixels in set (i+1)%3); step ks+2 is requested at the top of the step into set (i+2)%3
    // Order inside a step (pinned with scheduling barriers: at one wave per SIMD -- the low-resolution layers -- nothing else
    // hides a latency): the weight fragments of the first half are read from LDS first, the next-but-one step's addresses and
    // loads are issued under that latency, the second half's fragments are requested, then the 4 MT MFMAs run back to back.
    // Read where they are used (two ds_read_b128, wait, two MFMAs, ...) the fragments exposed an LDS latency per pair of MFMAs.
    auto body = [&](int ks, auto cur, auto nxt, auto nw) __attribute__((always_inline)) {
        constexpr int BC = decltype(cur)::value;
        const int buf = ks & 1;
        h8 af[2][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[0][mt] = *reinterpret_cast<const h8*>(As(buf, 0) + sw_off(16 * mt + l15, g));
        __builtin_amdgcn_sched_barrier(0);
        gload(nw, nw);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[1][mt] = *reinterpret_cast<const h8*>(As(buf, 1) + sw_off(16 * mt + l15, g));
        __builtin_amdgcn_sched_barrier(0);
        if (ks < nk) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                h8 bf[2];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) bf[nt] = __builtin_bit_cast(h8, rb[BC][hf][nt]);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[hf][mt], bf[nt], acc[mt][nt], 0, 0, 0);
            }
        }
        lstore(buf ^ 1, nxt);
        __syncthreads();
    };
    if constexpr (D == 5) {
        // five sets: step ks+4 is requested at the top of step ks (four memory latencies in flight per wave -- for the launches
        // that put ONE workgroup on a CU, where no other wave hides them)
        for (int ks = ks0; ks < nk; ks += 5) {
            body(ks, C0{}, C1{}, C4{});
            body(ks + 1, C1{}, C2{}, C0{});
            body(ks + 2, C2{}, C3{}, C1{});
            body(ks + 3, C3{}, C4{}, C2{});
            body(ks + 4, C4{}, C0{}, C3{});
        }
    } else {
        for (int ks = ks0; ks < nk; ks += 3) {
            body(ks, C0{}, C1{}, C2{});
            body(ks + 1, C1{}, C2{}, C0{});
            body(ks + 2, C2{}, C0{}, C1{});
        }
    }

    if (p.splits > 1 || p.act == 0) gather_store<BN, 0>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
    else if (p.act == 1) gather_store<BN, 1>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
    else gather_store<BN, 2>(p, acc, M, m0, co0, tid, zsplit, ph, oy_off, ox_off);
}


// ---------------------------------------------------------------------------------------------------------------
// 1x1 convolutions over many pixels (the hourglass's fused inception 1x1s: 128 -> 208 at 4 x 540 x 960 ...): HBM-bound
// (cin + cout) * 2 bytes per pixel against 2*cin*cout FLOP.  k_conv_igemm re-reads the input once per 64 out-channels;
// here a persistent workgroup stages the whole weight matrix in LDS once, each wave keeps the K = cin operand of its 32
// pixels in registers (read once from HBM) and walks every out-channel tile from LDS.
//   512 threads = 8 waves x 32 pixels; LDS: [cin/32][cout_pad][32] fp16, rows of 64 B with the usual chunk swizzle.
constexpr int C1_MAX_CHUNKS = 8;   // cin <= 256
template <int NCH>
__global__ void __launch_bounds__(512) k_conv1x1_stream(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    // weights -> LDS (once per workgroup): piece q = 16 bytes = row q>>2 (a (chunk, cout) pair), chunk-of-row q&3
    const int rows = NCH * p.cout_pad;
    for (int q = tid; q < rows * 4; q += 512)
        *reinterpret_cast<uint4*>(wsm + sw_off(q >> 2, q & 3)) = *reinterpret_cast<const uint4*>(p.wpk + (size_t)q * 8);
    // bias beside the weights: a global load per out-channel block inside the persistent loop put one memory latency
    // (microseconds under this kernel's own traffic) in front of every block's stores
    float* const bsm = reinterpret_cast<float*>(wsm + (size_t)rows * 64);
    for (int q = tid; q < p.cout_pad; q += 512) bsm[q] = (p.bias && q < p.cout) ? p.bias[q] : 0.0f;
    __syncthreads();
    const int ntile = min(p.cout_pad >> 4, 2 * ((p.cout + 31) >> 5));   // whole 32-channel blocks of padding are skipped (208 -> 224 of 256)
    const long long nblk = (M + 255) / 256;
    // this wave's 32 pixels x cin, straight into MFMA B-operand registers (lane: pixel l15 of tile nt, chunk piece g);
    // the next block's pixels are requested before this block's tiles are computed and stored
    h8 bf[NCH][2], nx[NCH][2];
    auto fetch = [&](long long blk, h8 (&dst)[NCH][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const long long m = blk * 256 + 32 * wv + 16 * nt + l15;
            const _Float16* src = p.in + (size_t)(m < M ? m : M - 1) * p.in_ld + p.in_coff + 8 * g;
#pragma unroll
            for (int c = 0; c < NCH; ++c) dst[c][nt] = *reinterpret_cast<const h8*>(src + 32 * c);
        }
    };
    if ((long long)blockIdx.x < nblk) fetch(blockIdx.x, nx);
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long long mbase = blk * 256 + 32 * wv;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bf[c][nt] = nx[c][nt];
        if (blk + gridDim.x < nblk) fetch(blk + gridDim.x, nx);
        // out-channel blocks of 32 as two MFMA row tiles whose rows are interleaved in groups of four (tile A row i =
        // channel 8(i>>2) + (i&3), tile B the same + 4): a lane then owns 8 consecutive channels of a pixel -> 16-byte
        // stores, 64 contiguous bytes per pixel and instruction.  A trailing 16-channel tile uses rows in natural order.
        // The block's out-channel walk is straight-line code: all 2 NCH fragment reads of a 32-channel block issued before
        // its MFMAs, bias as two f4 from LDS, the activation as max(x,0) + s min(x,0) (s = 1 none, 0 ReLU, slope Leaky --
        // exact for all three) and uniform store conditions.  Written with per-element runtime branches this loop was
        // ~1000 branchy instructions per block (52 % of wave cycles stalled at issue, 24 % issuing: PMC), i.e. the kernel
        // ran at 3.3 TB/s on the 208/224-channel layers against 4.6 TB/s on the 128-channel one.
        const float nslope = p.act == 1 ? 0.0f : (p.act == 2 ? p.slope : 1.0f);
        const bool vec_ok = (p.out_coff & 7) == 0 && (p.out_ld & 7) == 0;
        int t = 0;
        for (; t + 1 < ntile; t += 2) {
            const int rowA = 16 * t + 8 * (l15 >> 2) + (l15 & 3);
            h8 a0[NCH], a1[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                a0[c] = *reinterpret_cast<const h8*>(wsm + sw_off(c * p.cout_pad + rowA, g));
                a1[c] = *reinterpret_cast<const h8*>(wsm + sw_off(c * p.cout_pad + rowA + 4, g));
            }
            const int c0 = 16 * t + 8 * g;   // this lane: channels c0 .. c0+7 of pixels l15 (nt 0) and 16 + l15 (nt 1)
            const f4 b0 = *reinterpret_cast<const f4*>(bsm + c0), b1 = *reinterpret_cast<const f4*>(bsm + c0 + 4);
            f4 acc[2][2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) { acc[0][nt] = b0; acc[1][nt] = b1; }
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[c], bf[c][nt], acc[0][nt], 0, 0, 0);
                    acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[c], bf[c][nt], acc[1][nt], 0, 0, 0);
                }
            const bool full = vec_ok && c0 + 8 <= p.cout;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const long long m = mbase + 16 * nt + l15;
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float x = acc[r >> 2][nt][r & 3];
                    v[r] = fmaxf(x, 0.0f) + nslope * fminf(x, 0.0f);
                }
                _Float16* dst = p.out + (size_t)(m < M ? m : 0) * p.out_ld + p.out_coff + c0;
                if (m < M && full) {
                    *reinterpret_cast<h8*>(dst) = h8{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                                                     (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
                } else if (m < M) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (c0 + r < p.cout) dst[r] = (_Float16)v[r];
                }
            }
        }
        if (t < ntile) {   // trailing 16-channel tile: rows in natural order, 4 channels per lane
            h8 a0[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) a0[c] = *reinterpret_cast<const h8*>(wsm + sw_off(c * p.cout_pad + 16 * t + l15, g));
            const int c0 = 16 * t + 4 * g;
            const f4 b0 = *reinterpret_cast<const f4*>(bsm + c0);
            f4 acc[2] = {b0, b0};
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[c], bf[c][nt], acc[nt], 0, 0, 0);
            const bool full = (p.out_coff & 3) == 0 && (p.out_ld & 3) == 0 && c0 + 4 <= p.cout;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const long long m = mbase + 16 * nt + l15;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[nt][r], 0.0f) + nslope * fminf(acc[nt][r], 0.0f);
                _Float16* dst = p.out + (size_t)(m < M ? m : 0) * p.out_ld + p.out_coff + c0;
                if (m < M && full) {
                    *reinterpret_cast<h4*>(dst) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                } else if (m < M) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c0 + r < p.cout) dst[r] = (_Float16)v[r];
                }
            }
        }
    }
}

// k_conv1x1_stream with CONTIGUOUS memory accesses on both sides (128 input channels: the hourglass's fused inception 1x1s).
// Ablation of k_conv1x1_stream<4> on 128 -> 208 at 4 x 540 x 960 (434 us): its loads alone need ~200 us for 531 MB and its stores +
// MFMAs 336 us for 863 MB -- a pixel is 256 B in and 448 B out, and in the MFMA fragment layout every load / store instruction
// touches 64 B of each of 16 pixels: 16 separate segments per KiB, where the 32-channel 1x1 chains of the SR net (16 pixels = 1 KiB
// contiguous) run at the device's copy rate.  Here a wave owns 32 pixels per block and two 8-KB LDS slots:
//   in : the block's [32 px][256 B] by LDS-DMA, 4 whole pixels (1 KiB contiguous) per instruction, one block ahead; the 16-byte
//        pieces are permuted INSIDE each pixel's 256 B on the source side (piece j at slot j ^ (pixel & 15)), so the B-fragment
//        ds_read_b128 of (pixel l15, piece 4 c + g) is conflict-free while every DMA instruction still reads 1 KiB contiguous;
//   out: once the block's fragments sit in registers its slot is free: the results of 128 out-channels go there as
//        [32 px][256 B] (same permutation), are read back lane-linearly and leave as 4 x 256 contiguous bytes per instruction.
// A wave synchronises with nobody after the weights are staged (its slots are its own; LDS executes a wave's accesses in order).
// Same products in the same order per accumulator as k_conv1x1_stream: bit-identical.
#if VSR_X   // the transposing 1x1 build (measured: does not pay): cross-check library only
constexpr int C1T_SLOT = 32 * 256;   // one wave's [32 px][256 B] image
__global__ void __launch_bounds__(256) k_conv1x1_t(const ConvP p) {
    constexpr int NCH = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const int rows = NCH * p.cout_pad;
    for (int q = tid; q < rows * 4; q += 256)
        *reinterpret_cast<uint4*>(wsm + sw_off(q >> 2, q & 3)) = *reinterpret_cast<const uint4*>(p.wpk + (size_t)q * 8);
    float* const bsm = reinterpret_cast<float*>(wsm + (size_t)rows * 64);
    for (int q = tid; q < p.cout_pad; q += 256) bsm[q] = (p.bias && q < p.cout) ? p.bias[q] : 0.0f;
    unsigned char* const slots = wsm + (size_t)rows * 64 + (size_t)p.cout_pad * 4 + (size_t)wv * 2 * C1T_SLOT;   // this wave's two slots
    __syncthreads();
    const long long nblk = (M + 127) / 128;
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(p.in), 0, (int)((size_t)M * p.in_ld * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((size_t)M * p.out_ld * 2), 0x00020000);
    // DMA piece k (0..7) of a block: pixels 4 k .. 4 k + 3 of the wave's 32; lane L -> pixel 4 k + (L >> 4), slot L & 15
    const int dq = lane >> 4, ds = lane & 15;
    auto fetch = [&](long long blk, int slot) __attribute__((always_inline)) {
        const long long m0 = blk * 128 + 32 * wv;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pl = 4 * k + dq;
            const long long m = m0 + pl;
            const unsigned off = m < M ? (unsigned)(((size_t)m * p.in_ld + p.in_coff) * 2 + ((ds ^ (pl & 15)) << 4)) : 0xFFFFFFFFu;
            dma16(in_rsrc, slots + slot * C1T_SLOT + 1024 * k, off);
        }
    };
    const float nslope = p.act == 1 ? 0.0f : (p.act == 2 ? p.slope : 1.0f);
    const int ngroup = (p.cout + 127) >> 7;            // groups of 128 out-channels
    // the [32 px][256 B] output tile of one 128-channel group -> global memory, 4 x 256 contiguous bytes per instruction:
    // lane L of piece k holds pixel 4 k + (L >> 4), channels 128 grp + 8 (L & 15) .. + 7
    auto store_group = [&](const unsigned char* tile, long long mbase, int grp) __attribute__((always_inline)) {
        const int npair = min(4, (p.cout_pad - 128 * grp) >> 5);
        const int ch = 128 * grp + 8 * ds;
        const bool ch_ok = ch + 8 <= p.cout && ds < 4 * npair;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pl = 4 * k + dq;
            const long long m = mbase + pl;
            const u4 v = *reinterpret_cast<const u4*>(tile + pl * 256 + ((ds ^ (pl & 15)) << 4));
            const unsigned off = (ch_ok && m < M) ? (unsigned)(((size_t)m * p.out_ld + p.out_coff + ch) * 2) : 0xFFFFFFFFu;
            __builtin_amdgcn_raw_buffer_store_b128(v, out_rsrc, off, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile has been read back: its slot may be rewritten
    };
    // Order of a trip (vector-memory loads and stores retire out of order with respect to each other, so there is no counted
    // wait that leaves "the stores" in flight: every wait is vmcnt(0), and the trip is ordered so that whatever is youngest
    // before that wait was issued at least half a block of MFMAs earlier):
    //   wait | fragments of block b -> registers | LAST group of block b-1: tile (other slot) -> stores | DMA of block b+1 into
    //   that slot | groups of block b: MFMAs -> tile (this block's own slot); all but the last group stored at once
    int cur = 0;
    bool have_prev = false;
    long long prev_mbase = 0;
    if ((long long)blockIdx.x >= nblk) return;
    fetch(blockIdx.x, 0);
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x, cur ^= 1) {
        unsigned char* const img = slots + cur * C1T_SLOT;
        unsigned char* const oth = slots + (cur ^ 1) * C1T_SLOT;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        h8 bf[NCH][2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int pl = 16 * nt + l15;
                bf[c][nt] = *reinterpret_cast<const h8*>(img + pl * 256 + (((4 * c + g) ^ (pl & 15)) << 4));
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the fragments are in registers: the slot is free for the output tile
        if (have_prev) store_group(oth, prev_mbase, ngroup - 1);
        fetch(blk + gridDim.x, cur ^ 1);   // (past the last block: out-of-range offsets, zeros, no traffic)
        const long long mbase = blk * 128 + 32 * wv;
        for (int grp = 0; grp < ngroup; ++grp) {
            const int npair = min(4, (p.cout_pad - 128 * grp) >> 5);
            for (int tp = 0; tp < npair; ++tp) {
                const int t = 8 * grp + 2 * tp;            // first of the pair's two 16-row tiles
                const int rowA = 16 * t + 8 * (l15 >> 2) + (l15 & 3);
                h8 a0[NCH], a1[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    a0[c] = *reinterpret_cast<const h8*>(wsm + sw_off(c * p.cout_pad + rowA, g));
                    a1[c] = *reinterpret_cast<const h8*>(wsm + sw_off(c * p.cout_pad + rowA + 4, g));
                }
                const int c0 = 16 * t + 8 * g;
                const f4 b0 = *reinterpret_cast<const f4*>(bsm + c0), b1 = *reinterpret_cast<const f4*>(bsm + c0 + 4);
                f4 acc[2][2];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) { acc[0][nt] = b0; acc[1][nt] = b1; }
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[c], bf[c][nt], acc[0][nt], 0, 0, 0);
                        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[c], bf[c][nt], acc[1][nt], 0, 0, 0);
                    }
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const float x = acc[r >> 2][nt][r & 3];
                        v[r] = fmaxf(x, 0.0f) + nslope * fminf(x, 0.0f);
                    }
                    const int pl = 16 * nt + l15;
                    *reinterpret_cast<h8*>(img + pl * 256 + (((4 * tp + g) ^ (pl & 15)) << 4)) =
                        h8{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3], (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
                }
            }
            asm volatile("" ::: "memory");   // (same wave, in-order LDS: the read-back sees the writes above)
            if (grp + 1 < ngroup) store_group(img, mbase, grp);
        }
        have_prev = true;
        prev_mbase = mbase;
    }
    // the last block's last group is still in its slot (cur has flipped once more)
    store_group(slots + (cur ^ 1) * C1T_SLOT, prev_mbase, ngroup - 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the zero-fill DMA past the last block has landed before the wave ends)
}
#endif  // VSR_X

// ---------------------------------------------------------------------------------------------------------------
// Stride-1 convolutions with a spatial kernel (the hourglass's 3x3..11x11 inception branches and final conv, FlowNet's
// 3x3 layers and predict_flow, OSVOS's VGG stages): the tap-by-tap gather of k_conv_igemm re-reads every input pixel
// kh*kw times from L2, which bounds these layers by L2 bandwidth; here a workgroup stages the 2-D input patch of an
// 8 x 32 output tile in LDS once per 32-channel chunk and walks the taps from LDS.
// M = 16*MT out-channels, N = pixels (wave w: tile rows 2w, 2w+1), K = taps x channels.



// MT = out-channel tiles (16 each) per workgroup; blockIdx.z walks blocks of 16*MT out-channels.
// Weights are not staged: each tap's A fragments are read straight from global memory (the packed slab of one
// (tap, chunk) is [cout_pad][32] fp16, so a wave's 16 rows x 64 B are one contiguous 1 KiB read, L2-resident and
// shared by every workgroup), prefetched one tap ahead of the MFMAs that use them.
template <int MT>
__global__ void __launch_bounds__(256) k_conv_patch(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    const int PH = PT_H + p.kh - 1, PW = PT_W + p.kw - 1;  // patch
    const int ntap = p.kh * p.kw;
    unsigned char* const patch = psm;                      // [PH][PW] pixels of 64 B (chunk XOR pixel-column bits 1-2)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const vsrc::PatchTile t0 = vsrc::patch_tile<PT_H, PT_W>(p, p.Wo);
    const int n = t0.n, oy0 = t0.oy0, ox0 = t0.ox0, iy0 = t0.iy0, ix0 = t0.ix0;
    const int co0 = blockIdx.z * 16 * MT;
    const int nchunk = p.cin >> 5;

    f4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[mt][t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    // this lane's four pixels: rows 2 wv + (t >> 1), columns 16 (t & 1) + l15 of the tile
    int poff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) poff[t] = (2 * wv + (t >> 1)) * PW + 16 * (t & 1) + l15;
    auto wfrag = [&](int tap, int ch, int mt) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(p.wpk + ((size_t)(tap * nchunk + ch) * p.cout_pad + co0 + 16 * mt + l15) * 32 + 8 * g);
    };
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();
        stage_patch(p, patch, n, ch, iy0, ix0, PH, PW, tid);
        h8 af[MT], afn[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = wfrag(0, ch, mt);
        __syncthreads();
        int tap = 0;
        for (int ky = 0; ky < p.kh; ++ky)
            for (int kx = 0; kx < p.kw; ++kx, ++tap) {
                const int tn = tap + 1 < ntap ? tap + 1 : tap;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) afn[mt] = wfrag(tn, ch, mt);  // next tap's weights in flight
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int pix = poff[t] + ky * PW + kx;
                    const int px = 16 * (t & 1) + l15 + kx;
                    const h8 bf = *reinterpret_cast<const h8*>(patch + pix * 64 + ((g ^ ((px >> 1) & 3)) << 4));
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf, acc[mt][t], 0, 0, 0);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) af[mt] = afn[mt];
            }
    }
    __syncthreads();   // every wave is done with the patch: its memory carries the output tile now
    patch_epilogue<MT, 4>(p, psm + wv * (4 * 16 * 32 * MT), co0, lane, [&](int t, int mt) { return acc[mt][t]; },
                          [&](int t, int li) { return patch_pixoff(p, n, oy0 + 2 * wv + (t >> 1), ox0 + 16 * (t & 1) + li); });
}

// The 16-out-channel case of the patch kernel (the hourglass's 16-wide 3x3..11x11 inception branches and its final
// conv): with one out-channel tile every pixel operand read from LDS feeds a single MFMA, and four waves issuing one
// ds_read_b128 per MFMA ask the LDS for twice what it delivers.  The operand of (output row y, tap row ky) is the
// operand of (y+1, ky-1): a wave therefore owns 4 rows x 16 columns of the tile, reads each patch row once per tap
// column and feeds it to the (up to) four output rows it belongs to -- KH+3 reads for 4 KH MFMAs.  The KH weight
// fragments of the current tap column stay in registers (fetched one tap column ahead from L2).
template <int KH>
__global__ void __launch_bounds__(256) k_conv_patch_rows(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    const int PH = PT_H + KH - 1, PW = PT_W + p.kw - 1;
    unsigned char* const patch = psm;                      // [PH][PW] pixels of 64 B (chunk XOR pixel-column bits 1-2)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const vsrc::PatchTile t0 = vsrc::patch_tile<PT_H, PT_W>(p, p.Wo);
    const int n = t0.n, oy0 = t0.oy0, ox0 = t0.ox0, iy0 = t0.iy0, ix0 = t0.ix0;
    const int nchunk = p.cin >> 5;
    const int ry0 = 4 * (wv >> 1), cx0 = 16 * (wv & 1);    // this wave's 4 x 16 pixels of the 8 x 32 tile

    f4 acc[4][1];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    auto wfrag = [&](int ky, int kx, int ch) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(p.wpk + ((size_t)((ky * p.kw + kx) * nchunk + ch) * 16 + l15) * 32 + 8 * g);
    };
    auto column = [&](int kx, const h8 (&af)[KH][1]) __attribute__((always_inline)) {
        const int px = cx0 + l15 + kx;
        const unsigned char* src = patch + (ry0 * PW + px) * 64 + ((g ^ ((px >> 1) & 3)) << 4);
        vsrc::walk_tap_column<KH, 4, 1>(src, PW, af, acc, [](int) {});
    };
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();
        stage_patch(p, patch, n, ch, iy0, ix0, PH, PW, tid);
        h8 a0[KH][1], a1[KH][1];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) a0[ky][0] = wfrag(ky, 0, ch);
        __syncthreads();
        for (int kx = 0; kx < p.kw; kx += 2) {   // two tap columns per trip: the weight sets swap roles without copies
            const int k1 = kx + 1 < p.kw ? kx + 1 : kx, k2 = kx + 2 < p.kw ? kx + 2 : kx;
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) a1[ky][0] = wfrag(ky, k1, ch);
            column(kx, a0);
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) a0[ky][0] = wfrag(ky, k2, ch);
            if (kx + 1 < p.kw) column(kx + 1, a1);
        }
    }
    __syncthreads();
    patch_epilogue<1, 4>(p, psm + wv * (4 * 16 * 32), 0, lane, [&](int r, int) { return acc[r][0]; },
                         [&](int r, int li) { return patch_pixoff(p, n, oy0 + ry0 + r, ox0 + cx0 + li); });
}

// k4 s2 p1 transposed convolution with few out-channels on many pixels (FlowNetSD's 192 -> 16 at 2 x 256 x 480, the 2 -> 2 flow
// upsamplings): ALL FOUR phases from ONE staged input patch.  Through the gather kernel every input pixel is fetched 16 times
// (4 phases x 2x2 taps) in the MFMA fragment layout, 64 L1 tag look-ups per load, for 4 MFMAs per K step at 16 out-channels:
// 199 us for a layer whose HBM time is 30 us.  Here a workgroup stages the (8+2) x (32+2)-pixel patch of an 8 x 32 input tile
// once per 32-channel chunk; a wave owns 4 rows x 16 columns, keeps the chunk's 16 weight fragments (4 phases x 2x2 taps) in
// registers and walks the 3 x 6 patch positions it needs: the fragment at offset (dy, dx) feeds every (phase, tap) with
// ky - pad_y(py) = dy and kx - pad_x(px) = dx (1, 2 or 4 of them).  Output pixel (2y + py, 2x + px).
__global__ void __launch_bounds__(256) k_deconv4s2_patch(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    constexpr int PH = PT_H + 2, PW = PT_W + 2;
    unsigned char* const patch = psm;                      // [PH][PW] pixels of 64 B (chunk XOR pixel-column bits 1-2)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const vsrc::PatchTile t0 = vsrc::patch_tile<PT_H, PT_W>(p, p.W);   // (tiles of the INPUT map)
    const int n = t0.n, oy0 = t0.oy0, ox0 = t0.ox0;
    const int co0 = blockIdx.z * 16;
    const int nchunk = p.cin >> 5;
    const int ry0 = 4 * (wv >> 1), cx0 = 16 * (wv & 1);    // this wave's 4 x 16 input pixels of the 8 x 32 tile

    f4 acc[4][4];
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ph][r] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();
        stage_patch(p, patch, n, ch, oy0 - 1, ox0 - 1, PH, PW, tid);
        h8 A[4][4];   // [phase py * 2 + px][tap ky * 2 + kx]
#pragma unroll
        for (int ph = 0; ph < 4; ++ph)
#pragma unroll
            for (int tap = 0; tap < 4; ++tap)
                A[ph][tap] = *reinterpret_cast<const h8*>(p.wpk_ph[ph] + ((size_t)(tap * nchunk + ch) * p.cout_pad + co0 + l15) * 32 + 8 * g);
        __syncthreads();
#pragma unroll
        for (int dxi = 0; dxi < 3; ++dxi) {
            const int pxl = cx0 + l15 + dxi;
            const unsigned char* src = patch + (ry0 * PW + pxl) * 64 + ((g ^ ((pxl >> 1) & 3)) << 4);
#pragma unroll
            for (int pr = 0; pr < 6; ++pr) {
                const h8 bf = *reinterpret_cast<const h8*>(src + pr * PW * 64);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int dy = pr - 1 - r;
                    if (dy < -1 || dy > 1) continue;
#pragma unroll
                    for (int py = 0; py < 2; ++py) {
                        const int ky = dy + (py == 0 ? 1 : 0);
                        if (ky < 0 || ky > 1) continue;
#pragma unroll
                        for (int px = 0; px < 2; ++px) {
                            const int kx = dxi - 1 + (px == 0 ? 1 : 0);
                            if (kx < 0 || kx > 1) continue;
                            acc[py * 2 + px][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[py * 2 + px][ky * 2 + kx], bf, acc[py * 2 + px][r], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();   // every wave is done with the patch: its memory carries the output tiles now
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {   // phase (py, px) = (ph >> 1, ph & 1): output pixel (2 y + py, 2 x + px)
        const vsrc::WaveOut wo = vsrc::wave_out(p.outH, p.outW, p.out_ld, n, oy0 + ry0, ox0 + cx0, 2, ph >> 1, 2, ph & 1, p.H, p.W);
        patch_epilogue<1, 4>(p, psm + wv * (4 * 16 * 32), co0, lane, [&](int r, int) { return acc[ph][r]; },
                             [&](int r, int li) { return r < wo.rows_ok && li < wo.cols_ok ? wo.wbase + r * wo.rstride + li * wo.cstride : -1ll; });
    }
}

// The patch kernel with a 16 x 32 output tile and 8 rows x 16 columns x MT out-channel tiles per wave.  Measured on
// MI355X (tools/patch_exp.py): k_conv_patch spends 15-33 % of its time on the per-tap weight fragments (every wave
// fetches every fragment, 1 KiB per 4 MFMAs, which is the L1's whole bandwidth) and one ds_read per 1-4 MFMAs.  Here
// a wave walks the patch one tap COLUMN at a time: the KH fragments of the column sit in registers, each patch row
// is read once and feeds the up-to-eight output rows it belongs to (row y, tap row ky = row y+1, tap row ky-1), and a
// fragment is replaced by the next column's as soon as its last row has used it.  Per column: 8 KH MT MFMAs for KH MT
// fragment loads and KH+7 LDS reads -- half the L1 traffic and a third to a sixth of the LDS traffic per MFMA.
using vsrc::P8_H;
using vsrc::P8_W;
using vsrc::P8_R;
template <int KH, int MT>
__global__ void __launch_bounds__(256) k_conv_patch_r8(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    const int PH = P8_H + KH - 1, PW = P8_W + p.kw - 1;
    unsigned char* const patch = psm;                      // [PH][PW] pixels of 64 B (chunk XOR pixel-column bits 1-2)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: scalar arithmetic downstream)
    const int l15 = lane & 15, g = lane >> 4;
    const vsrc::PatchTile t0 = vsrc::patch_tile<P8_H, P8_W>(p, p.Wo);
    const int n = t0.n, oy0 = t0.oy0, ox0 = t0.ox0, iy0 = t0.iy0, ix0 = t0.ix0;
    const int co0 = blockIdx.z * 16 * MT;
    const int nchunk = p.cin >> 5;
    const int ry0 = P8_R * (wv >> 1), cx0 = 16 * (wv & 1);

    f4 acc[P8_R][MT];
#pragma unroll
    for (int r = 0; r < P8_R; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[r][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    auto wfrag = [&](int ky, int kx, int ch, int mt) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(p.wpk + ((size_t)((ky * p.kw + kx) * nchunk + ch) * p.cout_pad + co0 + 16 * mt + l15) * 32 + 8 * g);
    };
    h8 A[KH][MT];
#pragma unroll
    for (int ky = 0; ky < KH; ++ky)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) A[ky][mt] = wfrag(ky, 0, 0, mt);
    // pieces of the patch this thread stages: descriptors kept across chunks where the layer has several and the kernel is square
    constexpr int NPC = vsrc::P8Geom<KH, MT>::NPC;
    constexpr bool CACHE = KH <= 7;
    unsigned poff[CACHE ? NPC : 1];
    int pdst[CACHE ? NPC : 1];
    const bool cached = CACHE && p.kw == KH && nchunk > 1;
    if (CACHE && cached) patch_pieces(p, iy0, ix0, PH, PW, tid, poff, pdst);
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();
        if (CACHE && cached) stage_patch_cached(p, patch, n, ch, iy0, poff, pdst);
        else stage_patch(p, patch, n, ch, iy0, ix0, PH, PW, tid);
        __syncthreads();
        for (int kx = 0; kx < p.kw; ++kx) {
            // the column after this one (next chunk's first at the end; the very last refresh re-reads its own)
            const bool last_col = kx + 1 == p.kw;
            const int nkx = last_col ? (ch + 1 < nchunk ? 0 : kx) : kx + 1, nch = last_col && ch + 1 < nchunk ? ch + 1 : ch;
            const int px = cx0 + l15 + kx;
            const unsigned char* src = patch + (ry0 * PW + px) * 64 + ((g ^ ((px >> 1) & 3)) << 4);
#pragma unroll
            for (int pr = 0; pr < KH + P8_R - 1; ++pr) {
                const h8 bf = *reinterpret_cast<const h8*>(src + pr * PW * 64);
#pragma unroll
                for (int r = 0; r < P8_R; ++r) {
                    const int ky = pr - r;
                    if (ky < 0 || ky >= KH) continue;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[ky][mt], bf, acc[r][mt], 0, 0, 0);
                }
                const int kd = pr - (P8_R - 1);   // tap row whose last output row was just fed: its registers take the next column
                if (kd >= 0 && kd < KH) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) A[kd][mt] = wfrag(kd, nkx, nch, mt);
                }
            }
        }
    }
    __syncthreads();
    const vsrc::WaveOut wo = vsrc::wave_out(p, n, oy0 + ry0, ox0 + cx0);
    patch_epilogue<MT, P8_R>(p, psm + wv * (P8_R * 16 * 32 * MT), co0, lane, [&](int r, int mt) { return acc[r][mt]; },
                             [&](int r, int li) { return r < wo.rows_ok && li < wo.cols_ok ? wo.wbase + r * wo.rstride + li * wo.cstride : -1ll; });
}

// k_conv_patch_r8 with the chunk's WEIGHT BLOCK staged in LDS once per workgroup.  In k_conv_patch_r8 every wave fetches every
// weight fragment of its column from L2 (1 KiB per fragment): a 3x3 layer at 32 out-channels per workgroup moves 72 KB of
// fragments per 32-channel chunk beside a 39-KB patch -- at three workgroups per CU that is ~100 GB/s per CU of L2 -> CU traffic,
// above what the chip delivers (55-70 GB/s per CU measured on the LDS-DMA tile kernel, LAB_NOTES.md 5.3), so the 3x3 layers with many
// channels sat at 600-990 TFLOP/s while the 11x11 ones (the same patch feeds 13x the MFMAs) reach 1100-1400.  Here the block
// [kh*kw][16 MT][32] of a chunk goes to LDS once (18 KB at 32 out-channels, 36 KB at 64, by LDS-DMA: the packed slab of a
// (tap, chunk) is contiguous), the four waves read their column's fragments from there, and with no weight traffic per wave a
// workgroup can own 64 out-channels (MT = 4: the patch is staged once for twice the MFMAs; round 2's MT = 4 build kept 12
// fragments in registers per column, needed 266, and lost).  Same loop nest per accumulator as k_conv_patch_r8: bit-identical.
template <int KH, int MT>
__global__ void __launch_bounds__(256, 2) k_conv_patch_lw(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    typedef vsrc::P8Geom<KH, MT> G;                   // (conv_patch.h)
    const int KW = KH;
    const int PH = G::PH, PW = G::PW;
    constexpr int PATCH_BYTES = G::PATCH_BYTES, NPC = G::NPC;
    constexpr int WROWS = G::WROWS;                   // weight rows (out-channels) of this workgroup
    constexpr int WTAP = G::WTAP;                     // one tap's block [16 MT][32] fp16
    unsigned char* const patch = psm;                 // [PH][PW] pixels of 64 B (chunk XOR pixel-column bits 1-2)
    unsigned char* const wts = psm + PATCH_BYTES;     // [KH*KW][16 MT] rows of 64 B, 16-byte pieces XOR row bits 1-2 (sw_off)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const vsrc::PatchTile t0 = vsrc::patch_tile<P8_H, P8_W>(p, p.Wo);
    const int n = t0.n, oy0 = t0.oy0, ox0 = t0.ox0, iy0 = t0.iy0, ix0 = t0.ix0;
    const int co0 = blockIdx.z * WROWS;
    const int nchunk = p.cin >> 5;
    const int ry0 = P8_R * (wv >> 1), cx0 = 16 * (wv & 1);

    f4 acc[P8_R][MT];
#pragma unroll
    for (int r = 0; r < P8_R; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[r][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    unsigned poff[NPC];
    int pdst[NPC];
    patch_pieces(p, iy0, ix0, PH, PW, tid, poff, pdst);
    // weight DMA: piece q (1 KiB = 16 rows) of tap t: rows 16 q .. of the block; lane L -> row 16 q + (L >> 2), slot L & 3, which
    // under the read swizzle holds chunk (L & 3) ^ ((row >> 1) & 3).  WPW pieces per wave and chunk, round-robin over the waves.
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(p.wpk), 0, (int)((size_t)KH * KW * nchunk * p.cout_pad * 64), 0x00020000);
    constexpr int WPIECES = KH * KH * MT;             // 1-KiB pieces of a chunk's block
    const int wrow_l = lane >> 2, wslot = lane & 3;
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();
        for (int q = wv; q < WPIECES; q += 4) {       // (wave-uniform)
            const int tap = q / MT, blk = q - tap * MT;
            const int row = 16 * blk + wrow_l;
            const unsigned off = (unsigned)(((size_t)(tap * nchunk + ch) * p.cout_pad + co0 + row) * 64 + ((wslot ^ ((row >> 1) & 3)) << 4));
            dma16(w_rsrc, wts + tap * WTAP + 1024 * blk, off);
        }
        stage_patch_cached(p, patch, n, ch, iy0, poff, pdst);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kx = 0; kx < KW; ++kx) {
            h8 A[KH][MT];
#pragma unroll
            for (int ky = 0; ky < KH; ++ky)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    A[ky][mt] = *reinterpret_cast<const h8*>(wts + (ky * KW + kx) * WTAP + sw_off(16 * mt + l15, g));
            const int px = cx0 + l15 + kx;
            const unsigned char* src = patch + (ry0 * PW + px) * 64 + ((g ^ ((px >> 1) & 3)) << 4);
            vsrc::walk_tap_column<KH, P8_R, MT>(src, PW, A, acc, [](int) {});
        }
    }
    __syncthreads();
    const vsrc::WaveOut wo = vsrc::wave_out(p, n, oy0 + ry0, ox0 + cx0);
    patch_epilogue<MT, P8_R>(p, psm + wv * (P8_R * 16 * 32 * MT), co0, lane, [&](int r, int mt) { return acc[r][mt]; },
                             [&](int r, int li) { return r < wo.rows_ok && li < wo.cols_ok ? wo.wbase + r * wo.rstride + li * wo.cstride : -1ll; });
}

// The hourglass stem (7x7, 3 -> 128, stride 1, at full resolution): 531 MB of output per 4-frame batch against 0.12
// TFLOP, i.e. a store-bound layer; through k_conv_igemm<.., STEM> it ran at 0.62 ms, gather-bound (49 x 8-byte pieces per
// output pixel).  Here a persistent workgroup keeps ALL its weights in registers (wave w: out-channels 32w..32w+31, 7
// tap rows x 2 tiles), stages the 14 x 22-pixel input patch of an 8 x 16 tile in LDS (8 bytes per pixel, next tile's
// patch requested before this tile's MFMAs) and walks it row by row: the B operand of (pixel x, tap row ky) is the 64
// bytes of pixels x-3 .. x+4 of one patch row (lane group g: pixels x-3+2g, +1), and each patch row feeds the up-to-
// seven output rows it belongs to.  The tile leaves through LDS as whole 256-byte pixel rows.
constexpr int ST_R = 8, ST_C = 16, ST_PH = ST_R + 6, ST_PW = ST_C + 8;   // (patch width: 16 + 6, padded to 24)
constexpr int ST_PATCH = ST_PH * ST_PW * 8, ST_OUT = ST_R * ST_C * 256;
__global__ void __launch_bounds__(256) k_stem7_rows(const ConvP p, int tiles_x, int tiles_y, int ntiles) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[2 * ST_PATCH + ST_OUT];
    unsigned char* const outs = sm + 2 * ST_PATCH;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(p.in), 0, (int)(unsigned)((size_t)p.N * p.H * p.W * 8), 0x00020000);
    // weights: A[ky][mt] = rows 32 wv + 16 mt + l15 of tap row ky ([ky][cout_pad][32] fp16, k = 4 kx + c)
    h8 A[7][2];
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            A[ky][mt] = *reinterpret_cast<const h8*>(p.wpk + ((size_t)ky * p.cout_pad + 32 * wv + 16 * mt + l15) * 32 + 8 * g);
    float bz[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) bz[mt][e] = p.bias ? p.bias[32 * wv + 16 * mt + 4 * g + e] : 0.0f;
    // patch pieces of this thread: q = tid, tid + 256 (< 14 x 24 = 336 pixels)
    auto fetch = [&](int tile, u2v (&v)[2]) __attribute__((always_inline)) {
        const int n = tile / (tiles_x * tiles_y), rem = tile - n * tiles_x * tiles_y;
        const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = tid + 256 * u;
            const int py = q / ST_PW, px = q - py * ST_PW;
            const int iy = ty * ST_R - 3 + py, ix = tx * ST_C - 3 + px;
            const bool ok = q < ST_PH * ST_PW && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            const unsigned off = ok ? (unsigned)((((size_t)n * p.H + iy) * p.W + ix) * 8) : 0xFFFFFFFFu;
            v[u] = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, off, 0, 0);
        }
    };
    auto stash = [&](int buf, const u2v (&v)[2]) __attribute__((always_inline)) {
        *reinterpret_cast<u2v*>(sm + buf * ST_PATCH + tid * 8) = v[0];
        if (tid + 256 < ST_PH * ST_PW) *reinterpret_cast<u2v*>(sm + buf * ST_PATCH + (tid + 256) * 8) = v[1];
    };
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    u2v nv[2];
    fetch(tile, nv);
    stash(0, nv);
    __syncthreads();
    int buf = 0;
    for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
        const int tnext = tile + (int)gridDim.x;
        fetch(tnext < ntiles ? tnext : tile, nv);
        f4 acc[ST_R][2];
#pragma unroll
        for (int r = 0; r < ST_R; ++r)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[r][mt] = f4{bz[mt][0], bz[mt][1], bz[mt][2], bz[mt][3]};
        const unsigned char* src = sm + buf * ST_PATCH + (l15 + 2 * g) * 8;
#pragma unroll
        for (int pr = 0; pr < ST_PH; ++pr) {
            const u2v b0 = *reinterpret_cast<const u2v*>(src + pr * ST_PW * 8);
            const u2v b1 = *reinterpret_cast<const u2v*>(src + pr * ST_PW * 8 + 8);
            typedef unsigned int u4v __attribute__((ext_vector_type(4)));
            const h8 bf = __builtin_bit_cast(h8, u4v{b0[0], b0[1], b1[0], b1[1]});
#pragma unroll
            for (int r = 0; r < ST_R; ++r) {
                const int ky = pr - r;
                if (ky < 0 || ky >= 7) continue;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[ky][mt], bf, acc[r][mt], 0, 0, 0);
            }
        }
        // activation, fp16, into the tile's LDS image: pixel q = 16 r + l15, 256 B per pixel, 16-byte pieces XOR (q & 15)
#pragma unroll
        for (int r = 0; r < ST_R; ++r)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float tt = acc[r][mt][e];
                    if (p.act == 1) tt = fmaxf(tt, 0.0f);
                    else if (p.act == 2) tt = tt >= 0.0f ? tt : tt * p.slope;
                    v[e] = tt;
                }
                *reinterpret_cast<h4*>(outs + (16 * r + l15) * 256 + (((4 * wv + 2 * mt + (g >> 1)) ^ l15) << 4) + ((g & 1) << 3)) =
                    h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            }
        stash(buf ^ 1, nv);
        __syncthreads();
        {
            const int n = tile / (tiles_x * tiles_y), rem = tile - n * tiles_x * tiles_y;
            const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
            const int j = lane & 15;
#pragma unroll
            for (int it = 0; it < 8; ++it) {   // wave: pixels 32 wv .. +31, four per instruction (16 lanes x 16 B each)
                const int q = 32 * wv + 4 * it + (lane >> 4);
                const int oy = ty * ST_R + (q >> 4), ox = tx * ST_C + (q & 15);
                const h8 v = *reinterpret_cast<const h8*>(outs + q * 256 + ((j ^ (q & 15)) << 4));
                if (oy < p.Ho && ox < p.Wo)
                    *reinterpret_cast<h8*>(p.out + (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.out_ld + p.out_coff + 8 * j) = v;
            }
        }
        __syncthreads();   // the tile image is rewritten by the next trip
    }
}

// sums the split-K partials in a fixed order, + bias, activation, fp16 store (4 channels per thread)
__global__ void __launch_bounds__(256) k_splitk_finish(const ConvP p) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const unsigned c4n = (unsigned)p.cout_pad >> 2;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;   // (split-K layers are small: M * cout_pad / 4 < 2^31, checked by the launcher)
    if (idx >= (unsigned)M * c4n) return;
    const unsigned m = idx / c4n;
    const int c = (int)(idx - m * c4n) * 4;
    if (c >= p.cout) return;
    const int ph = blockIdx.y, nph = p.nphase > 1 ? 4 : 1;
    const int oy_off = p.nphase > 1 ? p.oy_off_ph[ph] : p.oy_off, ox_off = p.nphase > 1 ? p.ox_off_ph[ph] : p.ox_off;
    f4 s = f4{0.0f, 0.0f, 0.0f, 0.0f};
    // (the partial tiles are requested eight at a time and added in the fixed order z = 0, 1, ...: same sum, one memory
    // latency per eight splits instead of one per split)
    const size_t zstride = (size_t)nph * M * p.cout_pad;
    const float* wp = p.ws + ((size_t)ph * M + m) * p.cout_pad + c;
    int z = 0;
    for (; z + 8 <= p.splits; z += 8) {
        f4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f4*>(wp + (size_t)(z + u) * zstride);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; z + 2 <= p.splits; z += 2) {
        const f4 v0 = *reinterpret_cast<const f4*>(wp + (size_t)z * zstride), v1 = *reinterpret_cast<const f4*>(wp + (size_t)(z + 1) * zstride);
        s += v0;
        s += v1;
    }
    if (z < p.splits) s += *reinterpret_cast<const f4*>(wp + (size_t)z * zstride);
    const unsigned HoWo = (unsigned)(p.Ho * p.Wo);
    const unsigned n = m / HoWo, rem = m - n * HoWo;
    const unsigned oy = rem / (unsigned)p.Wo, ox = rem - oy * (unsigned)p.Wo;
    _Float16* dst = p.out + (((size_t)n * p.outH + oy * p.oy_mul + oy_off) * p.outW + ox * p.ox_mul + ox_off) * p.out_ld +
                    p.out_coff;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (c + r >= p.cout) break;
        float t = s[r] + (p.bias ? p.bias[c + r] : 0.0f);
        if (p.act == 1) t = fmaxf(t, 0.0f);
        else if (p.act == 2) t = t >= 0.0f ? t : t * p.slope;
        dst[c + r] = (_Float16)t;
    }
}

}  // namespace


// k_conv_igemm_d<.., 5>: five register sets, four K steps in flight, for launches of at most one workgroup per CU (0 never -- the
// default --, 1 that rule, 2 always; vsr_conv2d_tuning(8000 + n)).  Measured (tools/trunks_time.py, one box): FlowNet2 3.06 / 3.09 /
// 3.16 ms, hourglass x4 4.76 / 4.66 / 4.70, OSVOS 1.186 / 1.177 / 1.230 for n = 0 / 1 / 2 -- inside the run-to-run spread: the
// low-resolution layers are not waiting on the depth of the prefetch.  Bit-identical to the three-set build (tests).
VSR_TUNABLE g_gather_deep = 0;
// k_conv_igemm_d's dynamic LDS: the double-buffered weight ring + the K-walk table of one workgroup's range of steps
template <int BN, bool STEM>
static int launch_gather(const ConvP& p, dim3 grid, hipStream_t stream) {
    const vsrc::KSteps k = vsrc::k_steps(STEM, p.kh, p.kw, p.cin, p.splits);
    const int npair = k.npair, ks_per = k.ks_per;
    // five register sets (four K steps in flight) where the launch leaves one workgroup on a CU: nothing else hides the
    // memory latency there and the registers are free (g_gather_deep: 0 never, 1 that rule, 2 always)
    const bool deep = g_gather_deep == 2 || (g_gather_deep == 1 && (long long)grid.x * grid.y * grid.z <= 256 && ks_per >= 8);
    const size_t lds = (size_t)BN * 256 + (size_t)vsrc::kwalk_entries(ks_per, vsrc::kwalk_gather_lookahead(deep ? 5 : 3)) * 16;
    if (lds > 64 * 1024) return vsr::fail(VSR_E_ARG, "conv2d: %d K steps per workgroup exceed the kernel's walk table (split K further)", ks_per);
    if ((unsigned long long)npair * p.cout_pad * 64 >= (1ull << 30)) return vsr::fail(VSR_E_ARG, "conv2d: packed weights beyond 1 GiB");
#if VSR_X
    if (deep) { hipLaunchKernelGGL((k_conv_igemm_d<BN, STEM, 5>), grid, dim3(256), lds, stream, p); return VSR_OK; }
#endif
    hipLaunchKernelGGL((k_conv_igemm_d<BN, STEM, 3>), grid, dim3(256), lds, stream, p);
    return VSR_OK;
}

#if VSR_X
template <int BN, bool STEM>
static int launch_gather_lds(const ConvP& p, dim3 grid, hipStream_t stream) {
    const vsrc::KSteps k = vsrc::k_steps(STEM, p.kh, p.kw, p.cin, p.splits);
    const int npair = k.npair, ks_per = k.ks_per;
    const size_t lds = (size_t)4 * (BN * 64 + BM * 64) + (size_t)vsrc::kwalk_entries(ks_per, vsrc::KWALK_FIRST_LOOKAHEAD) * 16;
    if (lds > 64 * 1024) return vsr::fail(VSR_E_ARG, "conv2d: %d K steps per workgroup exceed the kernel's walk table (split K further)", ks_per);
    if ((unsigned long long)npair * p.cout_pad * 64 >= (1ull << 30)) return vsr::fail(VSR_E_ARG, "conv2d: packed weights beyond 1 GiB");
    hipLaunchKernelGGL((k_conv_igemm<BN, STEM>), grid, dim3(256), lds, stream, p);
    return VSR_OK;
}
#endif  // VSR_X

VSR_TUNABLE g_splitk_fill = 128;   // split K when a launch has fewer workgroups than this, into ~2x as many (tools/probe_splitk.py; 256 until the
                                   // round-2 rebuild made a K step cheap: FlowNet2 3.7 -> 3.45 ms, hourglass 5.03 -> 4.88, OSVOS 1.25 -> 1.29)
VSR_TUNABLE g_tile_mode = 1;   // conv_tile.hip (two-operand LDS-DMA tile): 0 never, 1 (default) where tile_choice says it wins over the gather kernel, 3 every layer it can run, the patch kernels' too (tests) (vsr_conv2d_tuning(2000 + n))
// k_conv1x1_t (contiguous accesses through per-wave LDS slots) for 128-input-channel 1x1 layers: 0 never (default), 1 yes
// (vsr_conv2d_tuning(7000 + n)).  Measured per layer inside the hourglass (tools/trunk_layers.sh): level with k_conv1x1_stream
// (4 x 270 x 480 128 -> 128 57 vs 55 us, 128 -> 224 89-93 vs 90-91) and SLOWER on the largest layer (4 x 540 x 960 128 -> 208: 336 vs
// 371 us) -- the contiguity of the accesses was not what holds the streaming kernel (1.39 GB in 336 us = 4.1 TB/s; a hand-written
// kernel of that traffic shape reaches 5.1-5.6 TB/s, profiles/r03_stream_rates.txt).  Kept as the bit-identical cross-check build.
[[maybe_unused]] VSR_TUNABLE g_c1t_mode = 0;
VSR_TUNABLE g_lw_mode = 1;     // k_conv_patch_lw (weight block in LDS): 0 never, 1 heuristic, 2 wherever a build exists (vsr_conv2d_tuning(6000 + n))
VSR_TUNABLE g_tile_bn = 0, g_tile_splits = 0;   // experiments: force the tile width (64 / 128) / the split count (vsr_conv2d_tuning(4000 + bn), (5000 + n)); 0 = heuristic
VSR_TUNABLE g_pf_mode = 1;     // k_conv_patch_pf (persistent, prefetching; conv_patch_pf.hip): 0 never, 1 heuristic, 2 wherever a build exists (64 out-channels per workgroup where the count allows), 3 as 2 with at most 32 per workgroup (vsr_conv2d_tuning(9000 + n))
// The kernel-selection mode (vsr_conv2d_tuning(n), n < 1000) is decoded HERE, once, into the names the plan functions read:
//   code | no_patch force_patch no_r8 no_rows first_gather wide_always wide_never | meaning
//      0 |    .         .         .      .         .            .          .      | the heuristics (default; the only row of libvsr_hip.so)
//      1 |    x         .         .      .         .            .          .      | never an LDS-patch kernel, the tile kernel, the streaming 1x1, stem7_rows
//      2 |    .         x         .      .         .            .          .      | the patch kernels whenever legal
//      3 |    .         .         x      x         .            .          .      | heuristic without the row-reuse builds (r8 -- and pf / lw, which sit behind it -- and rows)
//      5 |    .         .         x      .         .            .          .      | heuristic without k_conv_patch_r8 (pf / lw with it)
//      6 |    .         x         x      .         .            .          .      | as 2 without r8
//      7 |    .         x         x      x         .            .          .      | as 2 without r8 and rows
//      8 |    .         .         .      .         x            .          .      | gather layers through the first build k_conv_igemm; no tile kernel, no deconv patch, no 128-wide tile
//     10 |    .         .         .      .         .            x          .      | 128-channel gather tiles always
//     11 |    .         .         .      .         .            .          x      | 128-channel gather tiles never
struct PatchSw {
    bool no_patch, force_patch, no_r8, no_rows, first_gather, wide_always, wide_never;
};
constexpr PatchSw decode_patch_mode(int m) {
    return PatchSw{m == 1, m == 2 || m == 6 || m == 7, m == 3 || m == 5 || m == 6 || m == 7, m == 3 || m == 7, m == 8, m == 10, m == 11};
}
#if VSR_X
static int g_patch_mode = 0;   // the code as set (what vsr_conv2d_tuning returns as the previous mode)
static PatchSw g_sw = decode_patch_mode(0);
#else
static constexpr PatchSw g_sw = decode_patch_mode(0);
#endif

// byte range a gather kernel's buffer resource and its 32-bit offsets cover (0xFFFFFFFF marks "outside the image")
static constexpr unsigned long long kGatherLimit = 0xFFFFFFFFull;

// ---- the route of one launch: decided by plan_conv / plan_stem / plan_deconv (pure: no HIP call, no pointer read, no state beyond the
// tunables above), named by route_name, launched by launch_route.  Decisions count by Mr / gxr (the route batch Nr); launches use M / gx.
enum class Kind { gather, gather_stem, tile, deconv4s2_patch, stem7_rows, patch_pf, patch_lw, patch_r8, patch, patch_rows, conv1x1_stream, conv1x1_t };
struct ConvRoute {
    Kind kind;
    int bn;       // gather / tile: out-channels per workgroup
    int mt;       // patch family: 16-channel tiles per workgroup
    int splits;   // split-K factor (gather / tile; 1 elsewhere)
    bool first_build;   // gather through k_conv_igemm (cross-check library)
};

// kernel sizes with a row-reuse build (k_conv_patch_r8 / k_conv_patch_rows): their slot in the kernel tables, -1: none
static int kh_slot(int kh) { return kh == 3 ? 0 : kh == 5 ? 1 : kh == 7 ? 2 : kh == 11 ? 3 : -1; }
#if VSR_X   // k_conv1x1_t's LDS: weights + bias + two slots per wave
static size_t c1t_lds(const ConvP& p) { return (size_t)(p.cin >> 5) * p.cout_pad * 64 + (size_t)p.cout_pad * 4 + (size_t)4 * 2 * C1T_SLOT; }
#endif

// The tail every split-K rule ends with: at least 4 K steps per split, at most 32 splits, none without a workspace, partial sums
// [splits][nph][max(M, Mr)][cout_pad] fp32 inside the workspace.
static int clamp_splits(int splits, int nk_all, int nph, long long M, long long Mr, int cout_pad, bool has_ws, size_t ws_bytes) {
    if (splits > nk_all / 4) splits = nk_all / 4;
    if (splits > 32) splits = 32;
    if (!has_ws) splits = 1;
    while (splits > 1 && (size_t)splits * nph * (M > Mr ? M : Mr) * cout_pad * sizeof(float) > ws_bytes) --splits;
    return splits < 1 ? 1 : splits;
}

// Where the tile kernel (conv_tile.hip) replaces the gather kernel -- from per-layer device times INSIDE the three trunks at the
// benchmark size, both kernels on the same layers in one process (tools/trunk_layers.sh; profiles/r03_tile_vs_gather_layers.txt):
//   * 128-channel tiles with >= 384 workgroups (two per CU cover each other's DMA waits), no split-K: FlowNet's 5x5 / 3x3
//     stride-2 layers at 1/4 and 1/8 resolution, OSVOS's 512-channel VGG stage at 68 x 120: -10 ... -21 %;
//   * 64-out-channel stride-2 layers on >= 1000 pixel tiles (FlowNetS conv1 / conv2 at 512 x 960): -8 ... -10 %;
//   * long-K layers on few pixels (50-200 workgroups of 128 channels, >= 64 K steps: FlowNet's 1056 -> 256 transposed
//     convolution at 16 x 30, 800 -> 256 at 32 x 60) split to ~320 workgroups: -15 ... -25 %;
//   * everything else stays: 64-channel tiles LOSE to the gather kernel (32 x 60 512 -> 512: 42 -> 54 us; the tile kernel moves
//     32 KB through LDS per 2.1 MFLOP step and measures ~55 GB/s per CU of L2 -> LDS fill, 3/4 of what LDS-DMA gathers reach
//     on this chip: it is fill-bound, and narrower tiles only lower its FLOP per byte), the LDS-patch kernels keep the
//     stride-1 k x k layers (they stage the input once per 32-channel chunk for all k x k taps).
// -> 0: not the tile kernel; 64 / 128: tile width, *splits set.  nph = 4: the four phases of a k4 s2 transposed convolution in one launch.
static int tile_choice(const ConvP& p, long long M, int nk_all, int nph, int* splits) {
    *splits = 1;
    const long long gx = vsr::cdiv(M, BM);
    const bool can128 = (p.cout_pad & 127) == 0;
    const long long nwg128 = can128 ? gx * (p.cout_pad / 128) * nph : 0;
    if (nwg128 >= 384) return 128;
    if (p.cout_pad == 64 && p.stride == 2 && gx * nph >= 1000) return 64;
    if (nwg128 >= 50 && nwg128 < 200 && nk_all >= 64) {
        *splits = (int)((320 + nwg128 - 1) / nwg128);
        return 128;
    }
    return 0;
}

// The tile kernel's route from tile_choice's answer (bn, splits): bn = 0 is a layer the heuristic leaves to the other kernels
// (mode 3 / experiments), which gets the widest tile and splits towards 320 workgroups below 200.
static ConvRoute plan_tile(const ConvP& p, long long M, long long Mr, int nk_all, int nph, int bn, int splits, bool has_ws, size_t ws_bytes) {
    const bool can128 = (p.cout_pad & 127) == 0;
    if (bn == 0) {
        const long long nwg = vsr::cdiv(Mr, BM) * (long long)(p.cout_pad / (can128 ? 128 : 64)) * nph;
        bn = can128 ? 128 : 64;
        if (nwg < 200) splits = (int)((320 + nwg - 1) / nwg);
    }
    if (g_tile_bn == 64 || (g_tile_bn == 128 && can128)) bn = g_tile_bn;   // (experiments)
    if (g_tile_splits > 0) splits = g_tile_splits;
    return ConvRoute{Kind::tile, bn, 0, clamp_splits(splits, nk_all, nph, M, Mr, p.cout_pad, has_ws, ws_bytes), false};
}

// Where k_conv_patch_pf replaces k_conv_patch_r8 / _lw: -> 0 (not) or the out-channel tiles (16 each) per workgroup.
static int pf_choice(const ConvP& p, int N) {
    const int natural = p.cout_pad == 16 ? 1 : (p.cout_pad & 63) == 0 ? 4 : (p.cout_pad & 31) == 0 ? 2 : 0;
    if (!natural) return 0;
    if (g_pf_mode >= 2) {
        int mt = natural;
        if (g_pf_mode == 3 && mt == 4) mt = 2;
        while (mt > 1 && !vsrc::patch_pf_has(p.kh, mt)) mt >>= 1;
        return vsrc::patch_pf_has(p.kh, mt) ? mt : 0;
    }
    // heuristic (mode 1), from per-layer measurements inside the trunks (tools/trunk_layers.sh, profiles/r04_patch_pf_layers.txt): the
    // prefetch pays on the THIN layers with several chunks on many pixels (16 out-channels: the hourglass's full-resolution 64 -> 16
    // and 64 -> 1, OSVOS's side convolutions: -8 ... -22 %); with 32 / 64 out-channels per workgroup the extra registers cost
    // an occupancy step and the build loses 0 ... 25 % to k_conv_patch_r8 / _lw (64 per workgroup: it spills)
    if (natural == 1 && p.kh == 3 && (p.cin >> 5) >= 2 && (long long)N * p.Ho * p.Wo >= 60000) return 1;
    return 0;
}

static ConvRoute plan_conv(const ConvP& p, int Nr, bool has_ws, size_t ws_bytes) {
    const int kh = p.kh, kw = p.kw, cin = p.cin, cout_pad = p.cout_pad, Ho = p.Ho, Wo = p.Wo;
    const long long M = (long long)p.N * Ho * Wo, Mr = (long long)Nr * Ho * Wo;
    const int nk_all = (kh * kw * (cin >> 5) + 1) >> 1;
    const bool unit_stride = p.stride == 1 && p.stride_x == 1;
    // stride-1 layers with a real spatial kernel and enough pixels: the 2-D LDS patch kernel (stages the input once per
    // 32-channel chunk instead of gathering it kh*kw times from L2).  Measured on MI355X (tools/conv_microbench.py).
    const int patch_lds = (PT_H + kh - 1) * (PT_W + kw - 1) * 64;
    const bool patch_legal = unit_stride && Ho >= 4 && Wo >= 16 && patch_lds <= 64 * 1024 && p.N <= 65535 && (cout_pad & 15) == 0 &&
                             (unsigned long long)(kh + 16) * p.W * p.in_ld * 2 < (1ull << 31);   // (staging: 32-bit byte offsets from the patch's first row)
    const bool patch_pays = (long long)Ho * Wo >= 8192 && kh * kw >= 9 && ((cout_pad == 16 && (cin >> 5) <= 8) || cout_pad >= 32);
    // the tile kernel (conv_tile.hip) where it wins (tile_choice); mode 3: every layer it can run, also the patch kernels' (tests)
    int tile_splits = 1;
    const int tile_bn = tile_choice(p, Mr, nk_all, 1, &tile_splits);
    const bool tile_can = g_tile_mode >= 1 && !g_sw.first_gather && !g_sw.no_patch && (cout_pad & 63) == 0;
    const bool tile_ok = tile_can && (g_tile_mode >= 3 || (tile_bn != 0 && !(kh == 1 && kw == 1 && Mr >= 65536)));
    if (tile_can && g_tile_mode >= 3 && !g_sw.force_patch) return plan_tile(p, M, Mr, nk_all, 1, tile_bn, tile_splits, has_ws, ws_bytes);
    if (patch_legal && !g_sw.no_patch && (patch_pays || g_sw.force_patch)) {
        // 16 x 32 tiles, 8 rows per wave (k_conv_patch_r8) where a build exists and the patch fits the LDS: 32 out-channels
        // per workgroup (grid.z walks the blocks; measured against 64 per workgroup on the 8 x 32 tile, tools/patch_exp.py:
        // 3x3 32->64 at 2x512x960 93 -> 75 us, 64->128 at 2x256x480 80 -> 67 us) or the layer's 16
        const int r8_lds = (P8_H + kh - 1) * (P8_W + kw - 1) * 64;
        const int r8_mt = (cout_pad & 31) == 0 ? 2 : (cout_pad == 16 ? 1 : 0);
        if (!g_sw.no_r8 && r8_mt && r8_lds <= 80 * 1024 && Ho >= 12 && kh_slot(kh) >= 0) {
            // the persistent, prefetching build (conv_patch_pf.hip): see pf_choice
            if (g_pf_mode >= 1 && kh == kw) {
                const int pf_mt = pf_choice(p, Nr);
                if (pf_mt) return ConvRoute{Kind::patch_pf, 0, pf_mt, 1, false};
            }
            // 3x3 layers on many pixels: the build with the weight block in LDS (k_conv_patch_lw), 64 out-channels per workgroup
            // (32 for a 32-channel layer with >= 64 inputs).  Measured per layer inside the trunks (tools/trunk_layers.sh,
            // profiles/r03_patch_lw_layers.txt): 540 x 960 64 -> 64 130 -> 97 us, 270 x 480 128 -> 128 110 -> 79, 64 -> 128 68 -> 54,
            // 256 x 480 64 -> 128 60 -> 51, 270 x 480 64 -> 32 42 -> 36; it LOSES below ~500 workgroups (128 x 240 224 -> 64 29 -> 37:
            // half as many workgroups as the 32-channel build) and for 5x5 / 7x7 (their weight block leaves one workgroup per CU).
            // g_lw_mode: 0 never, 1 this heuristic, 2 wherever a build exists (tests / A-B).
            if (g_lw_mode >= 1 && kh == kw) {
                const int lw_mt = (kh == 3 && (cout_pad & 63) == 0) ? 4 : ((cout_pad & 31) == 0 && (kh == 3 || kh == 5 || kh == 7) ? 2 : 0);
                const long long lw_wgs = lw_mt ? (long long)vsr::cdiv(Ho, P8_H) * vsr::cdiv(Wo, P8_W) * Nr * (cout_pad / (16 * lw_mt)) : 0;
                const bool lw_pays = g_lw_mode >= 2 || (kh == 3 && lw_wgs >= 500 && (lw_mt == 4 || (cin >> 5) >= 2));
                if (lw_mt && lw_pays) return ConvRoute{Kind::patch_lw, 0, lw_mt, 1, false};
            }
            return ConvRoute{Kind::patch_r8, 0, r8_mt, 1, false};
        }
        if ((cout_pad & 31) == 0) return ConvRoute{Kind::patch, 0, (cout_pad & 63) == 0 ? 4 : 2, 1, false};
        return ConvRoute{cout_pad == 16 && !g_sw.no_rows && kh_slot(kh) >= 0 ? Kind::patch_rows : Kind::patch, 0, 1, 1, false};
    }
    // 1x1 over many pixels with more than one 64-channel block of outputs: the streaming kernel (input read once)
    if (kh == 1 && kw == 1 && unit_stride && p.pad_y == 0 && p.pad_x == 0 && p.oy_mul == 1 && p.ox_mul == 1 && p.oy_off == 0 && p.ox_off == 0 &&
        p.outH == Ho && p.outW == Wo && (cin >> 5) <= C1_MAX_CHUNKS && (size_t)(cin >> 5) * cout_pad * 64 <= 128 * 1024 && cout_pad > 64 && Mr >= 65536 &&
        !g_sw.no_patch) {
#if VSR_X
        // 128 input channels, 8-aligned output slice: the build with contiguous KiB accesses on both sides (k_conv1x1_t)
        if (g_c1t_mode >= 1 && cin == 128 && (p.cout & 7) == 0 && (p.out_ld & 7) == 0 && (p.out_coff & 7) == 0 && c1t_lds(p) <= 160 * 1024 &&
            (unsigned long long)M * p.in_ld * 2 < kGatherLimit && (unsigned long long)M * p.out_ld * 2 < kGatherLimit && p.cout <= 256)
            return ConvRoute{Kind::conv1x1_t, 0, 0, 1, false};
#endif
        return ConvRoute{Kind::conv1x1_stream, 0, 0, 1, false};
    }
    if (tile_ok) return plan_tile(p, M, Mr, nk_all, 1, tile_bn, tile_splits, has_ws, ws_bytes);
    const unsigned gxr = vsr::cdiv(Mr, BM);   // (the workgroups the decisions count)
    // widest tile the padded count fills; 128 out-channels per workgroup (half the pixel-operand traffic per FLOP: these
    // layers run at the L2's bandwidth, 43 FLOP per byte with the 128 x 64 tile) when that still leaves 128 workgroups
    // before split-K (measured per layer, tools/probe_layers.py with VSR_TUNING=10 / 11)
    const bool wide = (cout_pad & 127) == 0 && !g_sw.first_gather && !g_sw.wide_never && (g_sw.wide_always || (long long)gxr * (cout_pad / 128) >= 128);
    const int bn = wide ? 128 : (cout_pad & 63) == 0 ? 64 : ((cout_pad & 31) == 0 ? 32 : 16);
    // split-K when the launch cannot fill the chip and K is long
    const long long wgs = (long long)gxr * (cout_pad / bn);
    int splits = 1;
    if (has_ws && wgs < g_splitk_fill && nk_all >= 8) splits = clamp_splits((int)((g_splitk_fill * 2 + wgs - 1) / wgs), nk_all, 1, M, Mr, cout_pad, has_ws, ws_bytes);
    return ConvRoute{Kind::gather, bn, 0, splits, g_sw.first_gather};
}

static ConvRoute plan_stem(const ConvP& p, int Nr, bool, size_t) {
    const long long Mr = (long long)Nr * p.Ho * p.Wo;
    // the hourglass stem's shape: persistent row-walking kernel with register-resident weights and full-line stores
    if (!g_sw.no_patch && p.kh == 7 && p.kw == 7 && p.stride == 1 && p.pad_y == 3 && p.pad_x == 3 && p.cout == 128 && p.cout_pad == 128 && p.Ho == p.H &&
        p.Wo == p.W && (p.out_ld & 7) == 0 && (p.out_coff & 7) == 0 && (unsigned long long)p.N * p.H * p.W * 8 < (1ull << 31) && Mr >= 65536 &&
        (long long)p.N * vsr::cdiv(p.Wo, ST_C) * vsr::cdiv(p.Ho, ST_R) < (1ll << 30))
        return ConvRoute{Kind::stem7_rows, 0, 0, 1, false};
    return ConvRoute{Kind::gather_stem, (p.cout_pad & 63) == 0 ? 64 : ((p.cout_pad & 31) == 0 ? 32 : 16), 0, 1, g_sw.first_gather};
}

static ConvRoute plan_deconv(const ConvP& p, int Nr, bool has_ws, size_t ws_bytes) {
    const int cout_pad = p.cout_pad, H = p.H, W = p.W;
    const long long M = (long long)p.N * H * W, Mr = (long long)Nr * H * W;
    const int nk_all = (4 * (p.cin >> 5) + 1) >> 1;
    const bool patch_on = !g_sw.no_patch && !g_sw.first_gather;
    // few out-channels on many pixels: all four phases from one staged input patch (k_deconv4s2_patch)
    if (patch_on && cout_pad <= 32 && (long long)H * W >= 8192 && H >= 4 && W >= 16 && p.N <= 65535 &&
        (unsigned long long)(PT_H + 18) * W * p.in_ld * 2 < (1ull << 31))
        return ConvRoute{Kind::deconv4s2_patch, 0, 0, 1, false};
    int tile_splits = 1;
    const int tile_bn = tile_choice(p, Mr, nk_all, 4, &tile_splits);
    if (g_tile_mode >= 1 && patch_on && (cout_pad & 63) == 0 && (g_tile_mode >= 3 || tile_bn != 0))
        return plan_tile(p, M, Mr, nk_all, 4, tile_bn, tile_splits, has_ws, ws_bytes);
    const int bn = (cout_pad & 63) == 0 ? 64 : ((cout_pad & 31) == 0 ? 32 : 16);
    const long long wgs = (long long)vsr::cdiv(Mr, BM) * (cout_pad / bn) * 4;   // (counted by the route batch)
    int splits = 1;
    if (has_ws && wgs < 128 && nk_all >= 8) splits = clamp_splits((int)(256 / wgs), nk_all, 4, M, Mr, cout_pad, has_ws, ws_bytes);
    return ConvRoute{Kind::gather, bn, 0, splits, g_sw.first_gather};
}

// The one place a route is spelled (vsr_last_route(); tests and tools parse these strings).
static void route_name(const ConvRoute& r, const ConvP& p) {
    const char* dc = p.nphase > 1 ? "deconv4s2 " : "";
    switch (r.kind) {
    case Kind::gather: vsr::route(r.splits > 1 ? "%sgather<%d>+splitk%d" : "%sgather<%d>", dc, r.bn, r.splits); break;
    case Kind::gather_stem: vsr::route("gather<%d,stem>", r.bn); break;
    case Kind::tile: vsr::route(r.splits > 1 ? "%stile<%d>+splitk%d" : "%stile<%d>", dc, r.bn, r.splits); break;
    case Kind::deconv4s2_patch: vsr::route("deconv4s2_patch"); break;
    case Kind::stem7_rows: vsr::route("stem7_rows"); break;
    case Kind::patch_pf: vsr::route("patch_pf<%d,%d>", p.kh, r.mt); break;
    case Kind::patch_lw: vsr::route("patch_lw<%d,%d>", p.kh, r.mt); break;
    case Kind::patch_r8: vsr::route("patch_r8<%d,%d>", p.kh, r.mt); break;
    case Kind::patch: vsr::route("patch<%d>", r.mt); break;
    case Kind::patch_rows: vsr::route("patch_rows<%d>", p.kh); break;
    case Kind::conv1x1_stream: vsr::route("conv1x1_stream<%d>", p.cin >> 5); break;
    case Kind::conv1x1_t: vsr::route("conv1x1_t"); break;
    }
}

// What vsr::launched calls a launch of the route in vsr_last_error(): the entry's name and, for every kind but the gather, the kernel family.
static const char* launch_name(const ConvRoute& r, const ConvP& p) {
    const bool dc = p.nphase > 1;
    switch (r.kind) {
    case Kind::gather: return dc ? "deconv4s2_nhwc_f16" : "conv2d_nhwc_f16";
    case Kind::gather_stem: return "conv2d_stem_f16";
    case Kind::tile: return dc ? "deconv4s2_nhwc_f16/tile" : "conv2d_nhwc_f16/tile";
    case Kind::deconv4s2_patch: return "deconv4s2_nhwc_f16/patch";
    case Kind::stem7_rows: return "conv2d_stem_f16/rows";
    case Kind::patch_pf: return "conv2d_nhwc_f16/patch_pf";
    case Kind::patch_lw: return "conv2d_nhwc_f16/patch_lw";
    case Kind::patch_r8: return "conv2d_nhwc_f16/patch_r8";
    case Kind::patch:
    case Kind::patch_rows: return "conv2d_nhwc_f16/patch";
    case Kind::conv1x1_stream: return "conv2d_nhwc_f16/1x1";
    case Kind::conv1x1_t: return "conv2d_nhwc_f16/1x1t";
    }
    return "conv2d";
}

// The gather kernels' one width-to-template switch (128 only without STEM; the first build has no 128).
// launch_gather_wide is defined below launch_route, and the kernel tables of launch_route list their kernels in the order the old
// ladder mentioned them, for one reason only: a code object holds its kernels in the order of their first mention, and this layout
// let the refactor be checked with a plain diff of the device assembly.  The order carries NO meaning: nothing indexes by it beyond
// the expressions next to each table, and a later change may reorder the tables (and move launch_gather_wide up here) freely.
static int launch_gather_wide(const ConvP& p, dim3 grid, hipStream_t st);
template <bool STEM>
static int launch_gather_bn(const ConvP& p, const ConvRoute& r, dim3 grid, hipStream_t st) {
#if VSR_X
    if (r.first_build)   // (pixel operand through LDS): cross-check / A-B
        return r.bn == 64 ? launch_gather_lds<64, STEM>(p, grid, st) : r.bn == 32 ? launch_gather_lds<32, STEM>(p, grid, st) : launch_gather_lds<16, STEM>(p, grid, st);
#endif
    if (!STEM && r.bn == 128) return launch_gather_wide(p, grid, st);
    return r.bn == 64 ? launch_gather<64, STEM>(p, grid, st) : r.bn == 32 ? launch_gather<32, STEM>(p, grid, st) : launch_gather<16, STEM>(p, grid, st);
}

typedef void (*conv_kernel_t)(const ConvP);
struct BigLds {   // a kernel whose dynamic LDS can exceed 64 KB: the limit is raised once per device (one bit each)
    conv_kernel_t k;
    unsigned long long raised;
};
static void raise_lds(BigLds& e) { vsr::raise_lds_limit_once(e.raised, e.k, 160 * 1024); }

// Launches the route `r` of the layer in `p` (p.splits / p.ws set from r) and, after a split-K launch, the finish.
static int launch_route(const ConvP& p, const ConvRoute& r, hipStream_t st) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const int kh = p.kh, nph = p.nphase > 1 ? p.nphase : 1;
    int rc = VSR_OK;
    switch (r.kind) {
    case Kind::gather:
    case Kind::gather_stem: {
        const dim3 grid(vsr::cdiv(M, BM), p.cout_pad / r.bn, nph * r.splits);
        rc = r.kind == Kind::gather ? launch_gather_bn<false>(p, r, grid, st) : launch_gather_bn<true>(p, r, grid, st);
        break;
    }
    case Kind::tile:
        rc = vsrc::launch_conv_tile(p, r.bn, st);
        break;
    case Kind::deconv4s2_patch:
        hipLaunchKernelGGL(k_deconv4s2_patch, dim3(vsr::cdiv(p.H, PT_H) * vsr::cdiv(p.W, PT_W), p.N, p.cout_pad / 16), dim3(256), (PT_H + 2) * (PT_W + 2) * 64, st, p);
        break;
    case Kind::stem7_rows: {
        const int tiles_x = (int)vsr::cdiv(p.Wo, ST_C), tiles_y = (int)vsr::cdiv(p.Ho, ST_R);
        const long long ntiles = (long long)p.N * tiles_x * tiles_y;
        const unsigned grid1 = (unsigned)(ntiles < 256 * 2 ? ntiles : 256 * 2);   // two 4-wave workgroups resident per CU (registers)
        hipLaunchKernelGGL(k_stem7_rows, dim3(grid1), dim3(256), 0, st, p, tiles_x, tiles_y, (int)ntiles);
        break;
    }
    case Kind::patch_pf:
        rc = vsrc::launch_conv_patch_pf(p, r.mt, st);
        break;
    case Kind::patch_lw:
    case Kind::patch_r8: {   // 16 x 32 tiles: the patch (lw: + the weight block), then the output tile
        static BigLds lw[4] = {{k_conv_patch_lw<3, 4>, 0}, {k_conv_patch_lw<3, 2>, 0}, {k_conv_patch_lw<5, 2>, 0}, {k_conv_patch_lw<7, 2>, 0}};
        static BigLds r8[4][2] = {{{k_conv_patch_r8<3, 2>, 0}, {k_conv_patch_r8<3, 1>, 0}}, {{k_conv_patch_r8<5, 2>, 0}, {k_conv_patch_r8<5, 1>, 0}},
                                  {{k_conv_patch_r8<7, 2>, 0}, {k_conv_patch_r8<7, 1>, 0}}, {{k_conv_patch_r8<11, 2>, 0}, {k_conv_patch_r8<11, 1>, 0}}};
        const bool is_lw = r.kind == Kind::patch_lw;
        BigLds& e = is_lw ? lw[r.mt == 4 ? 0 : 1 + kh_slot(kh)] : r8[kh_slot(kh)][2 - r.mt];
        static const int lw_lds[4] = {vsrc::P8Geom<3, 4>::LW_LDS, vsrc::P8Geom<3, 2>::LW_LDS, vsrc::P8Geom<5, 2>::LW_LDS, vsrc::P8Geom<7, 2>::LW_LDS};
        const int r8_patch = (P8_H + kh - 1) * (P8_W + p.kw - 1) * 64, r8_out = 4 * P8_R * 16 * 32 * r.mt;
        const int lds = is_lw ? lw_lds[r.mt == 4 ? 0 : 1 + kh_slot(kh)] : r8_patch > r8_out ? r8_patch : r8_out;
        if (lds > 64 * 1024) raise_lds(e);
        hipLaunchKernelGGL(e.k, dim3(vsr::cdiv(p.Ho, P8_H) * vsr::cdiv(p.Wo, P8_W), p.N, p.cout_pad / (16 * r.mt)), dim3(256), lds, st, p);
        break;
    }
    case Kind::patch:
    case Kind::patch_rows: {   // 8 x 32 tiles: the patch, then the output tile
        const int lds_patch = (PT_H + kh - 1) * (PT_W + p.kw - 1) * 64, lds_out = 4 * 4 * 16 * 32 * r.mt;
        static const conv_kernel_t ks[7] = {k_conv_patch<4>, k_conv_patch<2>, k_conv_patch_rows<3>, k_conv_patch_rows<5>, k_conv_patch_rows<7>,
                                            k_conv_patch_rows<11>, k_conv_patch<1>};
        const conv_kernel_t k = ks[r.kind == Kind::patch_rows ? 2 + kh_slot(kh) : r.mt == 4 ? 0 : r.mt == 2 ? 1 : 6];
        hipLaunchKernelGGL(k, dim3(vsr::cdiv(p.Ho, PT_H) * vsr::cdiv(p.Wo, PT_W), p.N, p.cout_pad / (16 * r.mt)), dim3(256), lds_patch > lds_out ? lds_patch : lds_out, st, p);
        break;
    }
    case Kind::conv1x1_stream: {
        static const conv_kernel_t k1[C1_MAX_CHUNKS] = {k_conv1x1_stream<1>, k_conv1x1_stream<2>, k_conv1x1_stream<3>, k_conv1x1_stream<4>,
                                                        k_conv1x1_stream<5>, k_conv1x1_stream<6>, k_conv1x1_stream<7>, k_conv1x1_stream<8>};
        const conv_kernel_t k = k1[(p.cin >> 5) - 1];
        const size_t k_lds = (size_t)(p.cin >> 5) * p.cout_pad * 64 + (size_t)p.cout_pad * 4;   // weights + bias
        if (k_lds > 48 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k_lds) != hipSuccess)
            return vsr::fail(VSR_E_LAUNCH, "conv2d/1x1: cannot reserve %zu bytes of LDS", k_lds);
        const int per_cu = (int)((160 * 1024) / k_lds) < 2 ? 1 : 2;   // 512-thread workgroups resident per CU
        const long long nblk = (M + 255) / 256;
        hipLaunchKernelGGL(k, dim3((unsigned)(nblk < 256LL * per_cu ? nblk : 256LL * per_cu)), dim3(512), k_lds, st, p);
        break;
    }
    case Kind::conv1x1_t: {
#if VSR_X
        static BigLds t = {k_conv1x1_t, 0};
        raise_lds(t);
        const size_t t_lds = c1t_lds(p);
        const int per_cu = (int)((160 * 1024) / t_lds) < 2 ? 1 : 2;
        const long long nblk = (M + 127) / 128;
        hipLaunchKernelGGL(k_conv1x1_t, dim3((unsigned)(nblk < 256LL * per_cu ? nblk : 256LL * per_cu)), dim3(256), t_lds, st, p);
#endif
        break;
    }
    }
    if (rc) return rc;
    if (r.splits > 1) {
        rc = vsr::launched(launch_name(r, p));
        if (rc) return rc;
        hipLaunchKernelGGL(k_splitk_finish, dim3(vsr::cdiv(M * (p.cout_pad >> 2), 256), nph), dim3(256), 0, st, p);
    }
    return vsr::launched(launch_name(r, p));
}
// (down here: see launch_gather_bn)
static int launch_gather_wide(const ConvP& p, dim3 grid, hipStream_t st) { return launch_gather<128, false>(p, grid, st); }

// ---- what the three entries share: fill, argument checks (no pointer is read), sub-batches, plan + name + launch
static ConvP make_convp(const void* in, int in_ld, int in_coff, const void* w_packed, const float* bias, void* out, int out_ld, int out_coff, int N, int H,
                        int W, int cin, int Ho, int Wo, int cout, int cout_pad, int kh, int kw, int stride, int stride_x, int pad_y, int pad_x, int outH,
                        int outW, int oy_mul, int oy_off, int ox_mul, int ox_off, int act, float slope) {
    ConvP p = {};
    p.in = (const _Float16*)in; p.wpk = (const _Float16*)w_packed; p.bias = bias; p.out = (_Float16*)out;
    p.in_ld = in_ld; p.in_coff = in_coff; p.out_ld = out_ld; p.out_coff = out_coff;
    p.N = N; p.H = H; p.W = W; p.cin = cin; p.Ho = Ho; p.Wo = Wo; p.cout = cout; p.cout_pad = cout_pad;
    p.kh = kh; p.kw = kw; p.stride = stride; p.stride_x = stride_x > 0 ? stride_x : stride; p.pad_y = pad_y; p.pad_x = pad_x;
    p.outH = outH; p.outW = outW; p.oy_mul = oy_mul; p.oy_off = oy_off; p.ox_mul = ox_mul; p.ox_off = ox_off;
    p.act = act; p.slope = slope; p.ws = nullptr; p.splits = 1; p.nphase = 0;
    return p;
}
// the stem reads [N,H,W,4] pixels as one 32-wide K chunk per kernel row
static ConvP make_stem(const void* in4, const void* w_packed, const float* bias, void* out, int out_ld, int out_coff, int N, int H, int W, int Ho, int Wo,
                       int cout, int cout_pad, int kh, int kw, int stride, int pad_y, int pad_x, int act, float slope) {
    return make_convp(in4, 4, 0, w_packed, bias, out, out_ld, out_coff, N, H, W, 32, Ho, Wo, cout, cout_pad, kh, kw, stride, 0, pad_y, pad_x, Ho, Wo, 1, 0, 1, 0,
                      act, slope);
}
// k4 s2 transposed convolution: four 2x2-tap phases in one launch; phase (py, px) writes output (2y + py, 2x + px), py = 0 gathers
// input rows y-1, y (HDeconv4s2).  w_packed4: the phases' packed weights, or null (a plan without a launch)
static ConvP make_deconv(const void* in, int in_ld, int in_coff, const void* const* w_packed4, const float* bias, void* out, int out_ld, int out_coff, int N,
                         int H, int W, int cin, int cout, int cout_pad, int act, float slope) {
    ConvP p = make_convp(in, in_ld, in_coff, nullptr, bias, out, out_ld, out_coff, N, H, W, cin, H, W, cout, cout_pad, 2, 2, 1, 1, 0, 0, 2 * H, 2 * W, 2, 0, 2, 0,
                         act, slope);
    p.nphase = 4;
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        p.wpk_ph[ph] = w_packed4 ? (const _Float16*)w_packed4[ph] : nullptr;
        p.pad_y_ph[ph] = py == 0 ? 1 : 0; p.pad_x_ph[ph] = px == 0 ? 1 : 0;
        p.oy_off_ph[ph] = py; p.ox_off_ph[ph] = px;
    }
    return p;
}

static int check_conv(const ConvP& p) {
    VSR_REQUIRE(p.N > 0 && p.H > 0 && p.W > 0 && p.Ho > 0 && p.Wo > 0 && p.cout > 0 && p.kh > 0 && p.kw > 0 && p.stride > 0, "conv2d: bad shape");
    VSR_REQUIRE(p.cin > 0 && (p.cin & 31) == 0, "conv2d: input channels %d must be padded to a multiple of 32", p.cin);
    VSR_REQUIRE((p.in_ld & 7) == 0 && (p.in_coff & 7) == 0 && p.in_coff + p.cin <= p.in_ld, "conv2d: input slice [%d,+%d) of %d channels", p.in_coff, p.cin, p.in_ld);
    VSR_REQUIRE(p.out_coff >= 0 && p.out_coff + p.cout <= p.out_ld, "conv2d: output slice [%d,+%d) of %d channels", p.out_coff, p.cout, p.out_ld);
    VSR_REQUIRE(p.cout_pad >= p.cout && (p.cout_pad & 15) == 0, "conv2d: cout_pad %d", p.cout_pad);
    VSR_REQUIRE((p.Ho - 1) * p.oy_mul + p.oy_off < p.outH && (p.Wo - 1) * p.ox_mul + p.ox_off < p.outW && p.oy_off >= 0 && p.ox_off >= 0,
                "conv2d: output window exceeds the destination tensor");
    VSR_REQUIRE(p.act >= 0 && p.act <= 2, "conv2d: activation %d", p.act);
    VSR_REQUIRE((unsigned long long)p.H * p.W * p.in_ld * 2 < kGatherLimit, "conv2d: one %dx%dx%d fp16 image exceeds the 4 GiB the kernels address", p.H, p.W, p.in_ld);
    return VSR_OK;
}
static int check_stem(const ConvP& p) {
    VSR_REQUIRE(p.N > 0 && p.H > 0 && p.W > 0 && p.Ho > 0 && p.Wo > 0 && p.cout > 0 && p.kh > 0 && p.kw > 0 && p.kw <= 8 && p.stride > 0, "conv2d_stem: bad shape");
    VSR_REQUIRE(p.out_coff >= 0 && p.out_coff + p.cout <= p.out_ld && p.cout_pad >= p.cout && (p.cout_pad & 15) == 0, "conv2d_stem: output slice");
    VSR_REQUIRE(p.act >= 0 && p.act <= 2, "conv2d_stem: activation %d", p.act);
    VSR_REQUIRE((unsigned long long)p.N * p.H * p.W * 8 < kGatherLimit, "conv2d_stem: input batch beyond the 4 GiB the kernel addresses");
    return VSR_OK;
}
static int check_deconv(const ConvP& p) {
    VSR_REQUIRE(p.N > 0 && p.H > 0 && p.W > 0 && p.cout > 0 && p.cin > 0 && (p.cin & 31) == 0, "deconv4s2: bad shape");
    VSR_REQUIRE((p.in_ld & 7) == 0 && (p.in_coff & 7) == 0 && p.in_coff + p.cin <= p.in_ld, "deconv4s2: input slice");
    VSR_REQUIRE(p.out_coff >= 0 && p.out_coff + p.cout <= p.out_ld && p.cout_pad >= p.cout && (p.cout_pad & 15) == 0, "deconv4s2: output slice");
    VSR_REQUIRE(p.act >= 0 && p.act <= 2, "deconv4s2: activation %d", p.act);
    VSR_REQUIRE((unsigned long long)p.H * p.W * p.in_ld * 2 < kGatherLimit, "deconv4s2: one %dx%dx%d fp16 image exceeds the 4 GiB the kernel addresses", p.H, p.W, p.in_ld);
    return VSR_OK;
}

// The gather kernels address the whole input batch through one buffer resource with 32-bit byte offsets (0xFFFFFFFF = "out of image"):
// a batch beyond that runs as sub-batches of whole images (images are independent).  run(q): q = p narrowed to one sub-batch;
// img_out: output elements per image (the input's follow from p: one image is below the limit, check_conv / check_deconv).
template <class F>
static int for_sub_batches(const ConvP& p, size_t img_out, F&& run) {
    const unsigned long long img_in = (unsigned long long)p.H * p.W * p.in_ld;
    const int per = img_in * 2 * p.N >= kGatherLimit ? (int)((kGatherLimit - 1) / (img_in * 2)) : p.N;
    for (int n0 = 0; n0 < p.N; n0 += per) {
        ConvP q = p;
        q.in = p.in + (size_t)n0 * img_in; q.out = p.out + (size_t)n0 * img_out; q.N = p.N - n0 < per ? p.N - n0 : per;
        const int rc = run(q);
        if (rc) return rc;
    }
    return VSR_OK;
}

// The three entries (the `kind` codes of vsr_conv2d_plan): their argument checks, their plan function and their words for too many pixels.
enum Entry { kConv = 0, kStem = 1, kDeconv = 2 };
struct EntryDef {
    int (*check)(const ConvP&);
    ConvRoute (*plan)(const ConvP&, int Nr, bool has_ws, size_t ws_bytes);
    const char* too_many;
};
static const EntryDef kEntries[3] = {
    {check_conv, plan_conv, "conv2d: %lld output pixels exceed the kernels' 32-bit pixel index"},
    {check_stem, plan_stem, "conv2d_stem: %lld output pixels exceed the kernels' 32-bit pixel index"},
    {check_deconv, plan_deconv, "deconv4s2: %lld output pixels per phase exceed the kernel's 32-bit pixel index"}};

// The route of `p` through the plan function of its entry, decided by the route batch (vsr_conv2d_route_batch) and written to
// vsr_last_route().
static int plan_named(Entry entry, const ConvP& p, bool has_ws, size_t ws_bytes, ConvRoute* r) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    if (M >= (1ll << 31)) return vsr::fail(VSR_E_ARG, kEntries[entry].too_many, M);
    *r = kEntries[entry].plan(p, vsr::route_batch(p.N), has_ws, ws_bytes);
    route_name(*r, p);
    return VSR_OK;
}

static int run_planned(Entry entry, ConvP& p, void* splitk_ws, size_t splitk_ws_bytes, vsr_stream_t stream) {
    ConvRoute r;
    const int rc = plan_named(entry, p, splitk_ws != nullptr, splitk_ws_bytes, &r);
    if (rc) return rc;
    p.splits = r.splits;
    p.ws = r.splits > 1 ? (float*)splitk_ws : nullptr;
    return launch_route(p, r, vsr::S(stream));
}

extern "C" {

#if VSR_X
int vsr_conv2d_tuning(int patch_mode) {
    const int old = g_patch_mode;
    if (patch_mode >= 9000) { g_pf_mode = patch_mode - 9000; return old; }
    if (patch_mode >= 8000) { g_gather_deep = patch_mode - 8000; return old; }
    if (patch_mode >= 7000) { g_c1t_mode = patch_mode - 7000; return old; }
    if (patch_mode >= 6000) { g_lw_mode = patch_mode - 6000; return old; }
    if (patch_mode >= 5000) { g_tile_splits = patch_mode - 5000; return old; }
    if (patch_mode >= 4000) { g_tile_bn = patch_mode - 4000; return old; }
    if (patch_mode >= 2000) { g_tile_mode = patch_mode - 2000; return old; }
    if (patch_mode >= 1000) {   // 1000 + n: split-K fill threshold n (experiments; default 128)
        g_splitk_fill = patch_mode - 1000;
        return old;
    }
    g_patch_mode = patch_mode;
    g_sw = decode_patch_mode(patch_mode);
    return old;
}
#endif  // VSR_X

int vsr_conv2d_route_batch(int num, int den) {
    VSR_REQUIRE(num >= 0 && den >= 0 && num <= 65535 && den <= 65535, "conv2d_route_batch: %d / %d", num, den);
    vsr::route_scale_ref() = vsr::RouteScale{num, den};
    return VSR_OK;
}

int vsr_deconv4s2_nhwc_f16(const void* in, int in_ld, int in_coff, const void* const* w_packed4, const float* bias, void* out,
                           int out_ld, int out_coff, int N, int H, int W, int cin, int cout, int cout_pad, int act, float slope,
                           void* splitk_ws, size_t splitk_ws_bytes, vsr_stream_t stream) {
    VSR_REQUIRE(in && w_packed4 && out, "deconv4s2: null pointer");
    const ConvP p = make_deconv(in, in_ld, in_coff, w_packed4, bias, out, out_ld, out_coff, N, H, W, cin, cout, cout_pad, act, slope);
    const int rc = check_deconv(p);
    if (rc) return rc;
    for (int ph = 0; ph < 4; ++ph) VSR_REQUIRE(p.wpk_ph[ph], "deconv4s2: phase %d weights", ph);
    return for_sub_batches(p, (size_t)4 * H * W * out_ld,
                           [&](ConvP& q) { return run_planned(kDeconv, q, splitk_ws, splitk_ws_bytes, stream); });
}

int vsr_conv2d_stem_f16(const void* in4, const void* w_packed, const float* bias, void* out, int out_ld, int out_coff, int N,
                        int H, int W, int Ho, int Wo, int cout, int cout_pad, int kh, int kw, int stride, int pad_y, int pad_x,
                        int act, float slope, vsr_stream_t stream) {
    VSR_REQUIRE(in4 && w_packed && out, "conv2d_stem: null pointer");
    ConvP p = make_stem(in4, w_packed, bias, out, out_ld, out_coff, N, H, W, Ho, Wo, cout, cout_pad, kh, kw, stride, pad_y, pad_x, act, slope);
    const int rc = check_stem(p);
    if (rc) return rc;
    return run_planned(kStem, p, nullptr, 0, stream);
}

int vsr_conv2d_nhwc_sx_f16(const void* in, int in_ld, int in_coff, const void* w_packed, const float* bias, void* out,
                           int out_ld, int out_coff, int N, int H, int W, int cin, int Ho, int Wo, int cout, int cout_pad,
                           int kh, int kw, int stride, int stride_x, int pad_y, int pad_x, int outH, int outW, int oy_mul, int oy_off,
                           int ox_mul, int ox_off, int act, float slope, void* splitk_ws, size_t splitk_ws_bytes,
                           vsr_stream_t stream) {
    VSR_REQUIRE(in && w_packed && out, "conv2d: null pointer");
    const ConvP p = make_convp(in, in_ld, in_coff, w_packed, bias, out, out_ld, out_coff, N, H, W, cin, Ho, Wo, cout, cout_pad, kh, kw, stride, stride_x,
                               pad_y, pad_x, outH, outW, oy_mul, oy_off, ox_mul, ox_off, act, slope);
    const int rc = check_conv(p);
    if (rc) return rc;
    return for_sub_batches(p, (size_t)outH * outW * out_ld,
                           [&](ConvP& q) { return run_planned(kConv, q, splitk_ws, splitk_ws_bytes, stream); });
}

#if VSR_X
int vsr_conv2d_plan(int kind, int in_ld, int N, int H, int W, int cin, int Ho, int Wo, int cout, int cout_pad, int kh, int kw, int stride,
                    int stride_x, int pad_y, int pad_x, int out_ld, int out_coff, int outH, int outW, int oy_mul, int oy_off, int ox_mul, int ox_off,
                    int has_ws, size_t ws_bytes) {
    VSR_REQUIRE(kind >= 0 && kind <= 2, "conv2d_plan: kind %d", kind);
    const ConvP p = kind == 0 ? make_convp(nullptr, in_ld, 0, nullptr, nullptr, nullptr, out_ld, out_coff, N, H, W, cin, Ho, Wo, cout, cout_pad, kh, kw, stride,
                                           stride_x, pad_y, pad_x, outH, outW, oy_mul, oy_off, ox_mul, ox_off, 0, 0.0f)
                  : kind == 1 ? make_stem(nullptr, nullptr, nullptr, nullptr, out_ld, out_coff, N, H, W, Ho, Wo, cout, cout_pad, kh, kw, stride, pad_y, pad_x, 0, 0.0f)
                              : make_deconv(nullptr, in_ld, 0, nullptr, nullptr, nullptr, out_ld, out_coff, N, H, W, cin, cout, cout_pad, 0, 0.0f);
    const int rc = kEntries[kind].check(p);
    if (rc) return rc;
    ConvRoute r;
    return plan_named((Entry)kind, p, has_ws != 0, ws_bytes, &r);
}
#endif  // VSR_X

}  // extern "C"
