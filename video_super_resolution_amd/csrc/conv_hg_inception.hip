// conv_hg_inception.hip -- one inception block of the depth hourglass's inner levels in ONE launch (include/vsr_hip_hgi.h;
// libvsr_hip_hgi.so is built from this source alone).  The block is cat(1x1 | 1x1 -> k1 | 1x1 -> k2 | 1x1 -> k3), every convolution
// + folded BatchNorm + ReLU (depth.py _A to _G).  Through trunk_exec._Inception's four launches the fused 1x1 writes a work buffer
// [mid1 | mid2 | mid3 | o0 ...] to memory, three k x k launches read their mid slice back, and at 33 x 60 to 135 x 240 most of those
// need a split-K finish: a dependent chain of 8-17 us launches (profiles/r04_layer_tables_mid_round.txt).
//
// Here a workgroup (4 waves) owns one BRANCH of one 8 x 16 output tile of one image (blockIdx = tile, image, branch; the branch
// with the largest kernel first):
//   1. mid patch: the branch's 1x1 over the tile + halo, (8 + k - 1) x (16 + k - 1) pixels in groups of 16, a wave's groups in one
//      or two passes: per 32-channel chunk the pixel operands come straight from x by buffer loads in the MFMA operand layout (a position
//      outside the image carries an out-of-range offset and reads zeros), the weight fragments from the packed 1x1 slab.  + bias,
//      ReLU, fp16 into the LDS patch in conv_patch.h's layout (64-byte pixels per 32-channel plane, 16-byte pieces XOR pixel-column
//      bits 1-2); a pixel outside the image is stored as ZERO -- the k x k convolution's padding -- not as relu(bias);
//   2. k x k from the patch: k_conv_patch_rows' walk (conv_igemm.hip; walk_tap_column of conv_patch.h): a wave owns one 16-wide
//      out-channel tile and R rows x 16 columns (cout 64: four tiles x 8 rows; cout 32: two tiles x two row groups of 4), the KH weight
//      fragments of a tap column in registers, fetched one column ahead; chunk-major, then tap-column-major;
//   3. patch_epilogue_act (bias, ReLU, fp16, whole 16-byte pieces) into the dense output at the branch's channel offset.
// The plain 1x1 branch is the fourth kind of workgroup: 2 rows x 16 columns per wave, no patch.
// Every pixel's sums run in one fixed order whatever its tile, image or batch: results do not depend on N or on the workgroup.
#include <cstdint>

#include "conv_patch.h"

#include "../../include/vsr_hip_hgi.h"

namespace {

using vsrc::ConvP;
using vsrc::f4;
using vsrc::h4;
using vsrc::h8;
using vsrc::u4;

constexpr int TH = VSR_HGI_TILE_H, TW = VSR_HGI_TILE_W;
constexpr int EPI_BYTES = 4 * 8 * 16 * 32;   // the epilogues' four wave slices (8 rows x 16 pixels x 32 B; plain: 2 x 16 x 128 B)

struct HgiP {
    const _Float16* x;
    const _Float16* w1;      // [cin/32][c1_pad][32], rows [mid | mid | mid | o0]
    const float* b1;         // [c1_pad]
    const _Float16* wk[3];   // [k*k][mid/32][cout][32]
    const float* bk[3];      // [cout]
    _Float16* out;
    int in_ld, in_coff, cin, c1_pad, out_ld, N, H, W, tiles_x;
    unsigned x_bytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_rsrc(const HgiP& p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.x), 0, (int)p.x_bytes, 0x00020000);
}
__device__ __forceinline__ h8 load_x(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    return __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
}
// the epilogue's view of a branch: conv_patch.h's epilogue reads bias / cout / out / out_coff / out_ld of a ConvP
__device__ __forceinline__ ConvP epi_of(const HgiP& p, const float* bias, int cout, int out_coff) {
    ConvP c = {};
    c.bias = bias; c.cout = cout; c.out = p.out; c.out_coff = out_coff; c.out_ld = p.out_ld; c.act = 1; c.slope = 0.0f;
    return c;
}

// branch j (0..2): 1x1 cin -> MID on the patch, then KH x KH MID -> COUT on the tile
template <int KH, int MID, int COUT>
__device__ __forceinline__ void hgi_branch(const HgiP& p, unsigned char* sm, int j, int o0, int n, int oy0, int ox0) {
    constexpr int PAD = (KH - 1) / 2, PH = TH + KH - 1, PW = TW + KH - 1, NPIX = PH * PW;
    constexpr int NG = (NPIX + 15) / 16, NGW = (NG + 3) / 4;   // 16-pixel groups of the patch; per wave
    constexpr int MTM = MID / 16, NCK = MID / 32, PLANE = NPIX * 64;
    constexpr int CT = COUT / 16, R = TH * CT / 4;             // out-channel tiles; rows per wave (8 or 4)
    static_assert(CT == 4 || CT == 2, "cout 32 or 64");
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int iy0 = oy0 - PAD, ix0 = ox0 - PAD;
    const __amdgpu_buffer_rsrc_t rsrc = x_rsrc(p);

    // ---- 1. the mid patch, GP of the wave's groups per pass (all of them where their accumulators fit 64 registers; else two passes:
    //         128 accumulator registers held the k = 11 build at one wave per SIMD)
    constexpr int GP = NGW * MTM > 16 ? (NGW + 1) / 2 : NGW;
#pragma unroll 1
    for (int i0 = 0; i0 < NGW; i0 += GP) {
        f4 acc[GP][MTM];
        unsigned xoff[GP];
#pragma unroll
        for (int i = 0; i < GP; ++i) {   // (a group past the wave's last lies past the patch: q >= NPIX)
            const int q = 16 * (wv + 4 * (i0 + i)) + l15, py = q / PW, px = q - py * PW;
            const int iy = iy0 + py, ix = ix0 + px;
            const bool ok = q < NPIX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            xoff[i] = ok ? (unsigned)((((size_t)n * p.H + iy) * p.W + ix) * p.in_ld + p.in_coff + 8 * g) * 2u : 0xFFFFFFFFu;
#pragma unroll
            for (int mt = 0; mt < MTM; ++mt) acc[i][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        const _Float16* w1 = p.w1 + ((size_t)(j * MID + l15)) * 32 + 8 * g;
        const int nchunk = p.cin >> 5;
        for (int ch0 = 0; ch0 < nchunk; ch0 += 2) {   // (cin is 128 or 256: an even number of chunks; two per trip, their loads together)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int ch = ch0 + cc;
                h8 a[MTM], b[GP];
#pragma unroll
                for (int mt = 0; mt < MTM; ++mt) a[mt] = *reinterpret_cast<const h8*>(w1 + ((size_t)ch * p.c1_pad + 16 * mt) * 32);
#pragma unroll
                for (int i = 0; i < GP; ++i) b[i] = load_x(rsrc, vsrc::cached_piece_off(xoff[i], ch));
#pragma unroll
                for (int i = 0; i < GP; ++i)
#pragma unroll
                    for (int mt = 0; mt < MTM; ++mt) acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[mt], b[i], acc[i][mt], 0, 0, 0);
            }
        }
        // this lane: mid channels 16 mt + 4 g + e of patch pixel q
#pragma unroll
        for (int i = 0; i < GP; ++i) {
            const int q = 16 * (wv + 4 * (i0 + i)) + l15, py = q / PW, px = q - py * PW;
            if (q >= NPIX) continue;
            const bool live = xoff[i] != 0xFFFFFFFFu;
#pragma unroll
            for (int mt = 0; mt < MTM; ++mt) {
                const f4 bz = *reinterpret_cast<const f4*>(p.b1 + j * MID + 16 * mt + 4 * g);
                _Float16 v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = live ? (_Float16)fmaxf(acc[i][mt][e] + bz[e], 0.0f) : (_Float16)0.0f;
                *reinterpret_cast<h4*>(sm + (mt >> 1) * PLANE + q * 64 + (((2 * (mt & 1) + (g >> 1)) ^ ((px >> 1) & 3)) << 4) + ((g & 1) << 3)) =
                    h4{v[0], v[1], v[2], v[3]};
            }
        }
    }
    __syncthreads();

    // ---- 2. KH x KH from the patch: this wave's out-channel tile ct, rows [ry0, ry0 + R) x 16 columns
    const int ct = wv % CT, ry0 = (wv / CT) * R;
    f4 acc[R][1];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    const _Float16* wk = p.wk[j] + ((size_t)(16 * ct + l15)) * 32 + 8 * g;
    auto wfrag = [&](int ky, int kx, int ch) __attribute__((always_inline)) {
        return *reinterpret_cast<const h8*>(wk + (size_t)((ky * KH + kx) * NCK + ch) * COUT * 32);
    };
#pragma unroll 1
    for (int ch = 0; ch < NCK; ++ch) {
        const unsigned char* const plane = sm + ch * PLANE;
        auto column = [&](int kx, const h8 (&af)[KH][1]) __attribute__((always_inline)) {
            const int px = l15 + kx;
            const unsigned char* src = plane + (ry0 * PW + px) * 64 + ((g ^ ((px >> 1) & 3)) << 4);
            vsrc::walk_tap_column<KH, R, 1>(src, PW, af, acc, [](int) {});
        };
        h8 a0[KH][1], a1[KH][1];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) a0[ky][0] = wfrag(ky, 0, ch);
#pragma unroll 1
        for (int kx = 0; kx < KH; kx += 2) {   // two tap columns per trip: the weight sets swap roles without copies
            const int k1 = kx + 1 < KH ? kx + 1 : kx, k2 = kx + 2 < KH ? kx + 2 : kx;
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) a1[ky][0] = wfrag(ky, k1, ch);
            column(kx, a0);
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) a0[ky][0] = wfrag(ky, k2, ch);
            if (kx + 1 < KH) column(kx + 1, a1);
        }
    }
    __syncthreads();   // every wave is done with the patch: its memory carries the output tile now

    // ---- 3. out
    const ConvP e = epi_of(p, p.bk[j], COUT, o0 + j * COUT);
    const long long nbase = (long long)n * p.H;
    vsrc::patch_epilogue_act<1, R, 1>(e, sm + wv * (R * 16 * 32), 16 * ct, lane, [&](int r, int) { return acc[r][0]; },
                                      [&](int r, int li) {
                                          const int oy = oy0 + ry0 + r, ox = ox0 + li;
                                          return oy < p.H && ox < p.W ? ((nbase + oy) * p.W + ox) * p.out_ld : -1ll;
                                      });
}

// the plain 1x1 branch: cin -> O0 on the tile's own pixels, 2 rows x 16 columns per wave
template <int MID, int O0>
__device__ __forceinline__ void hgi_plain(const HgiP& p, unsigned char* sm, int n, int oy0, int ox0) {
    constexpr int MT = O0 / 16;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = x_rsrc(p);
    f4 acc[2][MT];
    unsigned xoff[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int iy = oy0 + 2 * wv + t, ix = ox0 + l15;
        xoff[t] = iy < p.H && ix < p.W ? (unsigned)((((size_t)n * p.H + iy) * p.W + ix) * p.in_ld + p.in_coff + 8 * g) * 2u : 0xFFFFFFFFu;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const _Float16* w1 = p.w1 + ((size_t)(3 * MID + l15)) * 32 + 8 * g;
    const int nchunk = p.cin >> 5;
    for (int ch0 = 0; ch0 < nchunk; ch0 += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int ch = ch0 + cc;
            h8 a[MT], b[2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const h8*>(w1 + ((size_t)ch * p.c1_pad + 16 * mt) * 32);
#pragma unroll
            for (int t = 0; t < 2; ++t) b[t] = load_x(rsrc, vsrc::cached_piece_off(xoff[t], ch));
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[mt], b[t], acc[t][mt], 0, 0, 0);
        }
    }
    const ConvP e = epi_of(p, p.b1 + 3 * MID, O0, 0);
    const long long nbase = (long long)n * p.H;
    vsrc::patch_epilogue_act<MT, 2, 1>(e, sm + wv * (2 * 16 * 32 * MT), 0, lane, [&](int t, int mt) { return acc[t][mt]; },
                                       [&](int t, int li) {
                                           const int oy = oy0 + 2 * wv + t, ox = ox0 + li;
                                           return oy < p.H && ox < p.W ? ((nbase + oy) * p.W + ox) * p.out_ld : -1ll;
                                       });
}

template <int K1, int K2, int K3, int MID, int COUT, int O0>
__global__ void __launch_bounds__(256) k_hg_inception(const HgiP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
    const int n = blockIdx.y, oy0 = ty * TH, ox0 = tx * TW;
    switch (blockIdx.z) {   // (workgroup-uniform; the largest kernel is dispatched first)
    case 0: hgi_branch<K3, MID, COUT>(p, sm, 2, O0, n, oy0, ox0); break;
    case 1: hgi_branch<K2, MID, COUT>(p, sm, 1, O0, n, oy0, ox0); break;
    case 2: hgi_branch<K1, MID, COUT>(p, sm, 0, O0, n, oy0, ox0); break;
    default: hgi_plain<MID, O0>(p, sm, n, oy0, ox0); break;
    }
}

typedef void (*hgi_kernel_t)(const HgiP);
struct Sig {
    int k1, k2, k3, mid, cout, o0;
    hgi_kernel_t kern;
};
// depth.py: _A / _E, _B / _C, _D, _F, _G (cin is a run-time count of 32-channel chunks)
const Sig SIGS[] = {
    {3, 5, 7, 32, 32, 32, k_hg_inception<3, 5, 7, 32, 32, 32>},   {3, 5, 7, 32, 64, 64, k_hg_inception<3, 5, 7, 32, 64, 64>},
    {3, 7, 11, 64, 64, 64, k_hg_inception<3, 7, 11, 64, 64, 64>}, {3, 7, 11, 64, 32, 32, k_hg_inception<3, 7, 11, 64, 32, 32>},
    {3, 5, 7, 64, 32, 32, k_hg_inception<3, 5, 7, 64, 32, 32>},
};
const Sig* find_sig(int k1, int k2, int k3, int mid, int cout, int o0) {
    for (const Sig& s : SIGS)
        if (s.k1 == k1 && s.k2 == k2 && s.k3 == k3 && s.mid == mid && s.cout == cout && s.o0 == o0) return &s;
    return nullptr;
}
int lds_bytes(int k3, int mid) {
    const int patch = (TH + k3 - 1) * (TW + k3 - 1) * 64 * (mid / 32);
    return patch > EPI_BYTES ? patch : EPI_BYTES;
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

extern "C" {

int vsr_hgi_abi_version(void) { return VSR_HGI_ABI_VERSION; }
const char* vsr_hgi_last_error(void) { return vsr::err_buf(); }

int vsr_hgi_supported(int k1, int k2, int k3, int mid, int cout, int o0) { return find_sig(k1, k2, k3, mid, cout, o0) ? 1 : 0; }

long long vsr_hgi_workgroups(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || N > 65535) return 0;
    return 4ll * vsr::cdiv(H, TH) * vsr::cdiv(W, TW) * N;
}

int vsr_hgi_inception_f16(const void* x, int in_ld, int in_coff, int cin, const void* w1, const float* b1, int c1_pad, int mid, int o0,
                          const void* wk1, const float* bk1, int k1, const void* wk2, const float* bk2, int k2, const void* wk3,
                          const float* bk3, int k3, int cout, void* out, int out_ld, int N, int H, int W, vsr_stream_t stream) {
    VSR_REQUIRE(x && w1 && b1 && wk1 && bk1 && wk2 && bk2 && wk3 && bk3 && out, "hgi_inception: null pointer");
    VSR_REQUIRE(N > 0 && H > 0 && W > 0, "hgi_inception: bad shape (N %d, map of %d x %d)", N, H, W);
    VSR_REQUIRE(N <= 65535, "hgi_inception: grid overflow (N %d beyond 65535)", N);
    const Sig* sig = find_sig(k1, k2, k3, mid, cout, o0);
    VSR_REQUIRE(sig, "hgi_inception: no kernel for k (%d,%d,%d) mid %d cout %d o0 %d", k1, k2, k3, mid, cout, o0);
    VSR_REQUIRE(cin == 128 || cin == 256, "hgi_inception: cin %d (128 or 256)", cin);
    VSR_REQUIRE(in_ld > 0 && out_ld > 0 && in_coff >= 0 && c1_pad > 0 && ((in_ld | in_coff | out_ld | c1_pad) & 31) == 0,
                "hgi_inception: in_ld %d, in_coff %d, out_ld %d and c1_pad %d must be multiples of 32", in_ld, in_coff, out_ld, c1_pad);
    VSR_REQUIRE(in_coff + cin <= in_ld, "hgi_inception: the input slice [%d, %d) leaves its row of %d", in_coff, in_coff + cin, in_ld);
    VSR_REQUIRE(o0 + 3 * cout <= out_ld, "hgi_inception: the result of %d channels leaves its row of %d", o0 + 3 * cout, out_ld);
    VSR_REQUIRE(c1_pad >= 3 * mid + o0, "hgi_inception: c1_pad %d below the fused 1x1's %d rows", c1_pad, 3 * mid + o0);
    VSR_REQUIRE(((addr(x) | addr(out) | addr(w1) | addr(wk1) | addr(wk2) | addr(wk3)) & 15) == 0,
                "hgi_inception: x, out and the weight slabs must be 16-byte aligned");
    VSR_REQUIRE(((addr(b1) | addr(bk1) | addr(bk2) | addr(bk3)) & 15) == 0, "hgi_inception: the biases must be 16-byte aligned");
    const unsigned long long pixels = (unsigned long long)N * H * W;
    const unsigned long long x_bytes = pixels * in_ld * 2, out_bytes = pixels * out_ld * 2;
    VSR_REQUIRE(x_bytes < 0xFFFFFFF0ull && out_bytes < 0xFFFFFFF0ull, "hgi_inception: x (%llu B) or out (%llu B) reaches 4 GiB", x_bytes, out_bytes);
    VSR_REQUIRE(addr(x) + x_bytes <= addr(out) || addr(out) + out_bytes <= addr(x), "hgi_inception: x and out overlap");
    HgiP p;
    p.x = (const _Float16*)x; p.w1 = (const _Float16*)w1; p.b1 = b1;
    p.wk[0] = (const _Float16*)wk1; p.wk[1] = (const _Float16*)wk2; p.wk[2] = (const _Float16*)wk3;
    p.bk[0] = bk1; p.bk[1] = bk2; p.bk[2] = bk3;
    p.out = (_Float16*)out;
    p.in_ld = in_ld; p.in_coff = in_coff; p.cin = cin; p.c1_pad = c1_pad; p.out_ld = out_ld; p.N = N; p.H = H; p.W = W;
    p.tiles_x = (int)vsr::cdiv(W, TW);
    p.x_bytes = (unsigned)x_bytes;
    const unsigned long long tiles = (unsigned long long)p.tiles_x * vsr::cdiv(H, TH);
    VSR_REQUIRE(tiles < (1ull << 31), "hgi_inception: too many tiles");
    hipLaunchKernelGGL(sig->kern, dim3((unsigned)tiles, N, 4), dim3(256), lds_bytes(k3, mid), vsr::S(stream), p);
    return vsr::launched("hgi_inception");
}

}  // extern "C"
