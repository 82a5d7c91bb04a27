// clip_deint.hip -- motion-adaptive deinterlacing of packed Y'CbCr frames (include/vsr_hip_deint.h; libvsr_hip_deint.so is built from
// this source alone).  The rule is the header's, operation by operation; nothing here knows a pixel format.
//
//   k_deint<SB> : all planes of one frame in one launch: a flat grid, the workgroups of plane 0 first, then plane 1's, then plane 2's, each
//                 plane with as many as IT needs (a grid sized by the luma plane would start 1.5 times as many empty workgroups for the two
//                 quarter-size chroma planes of 4:2:0 as it starts full ones).  A workgroup of 64 x 4 threads covers 4 row pairs
//                 (rows 2p and 2p + 1: one kept, one rebuilt) by 1024 bytes; a wave is 1 KB of one pair.  One thread = 16 bytes of the
//                 rebuilt row + the same 16 bytes of the kept row: 8 loads (C above and below, B and A on the row, P and N above and
//                 below; one of B, A is C, and with prev == cur or next == cur more of them are one line) and 2 stores.  The kept row
//                 of a pair is always one of the two C rows the rebuilt row reads (above with keep = 0, below with keep = 1), so the
//                 copy costs no load.  A plane of an odd number of rows ends in half a pair: a kept row alone (keep = 0) is copied, a
//                 rebuilt row alone (keep = 1) reads the kept row above twice (the header's reflection).
//                 WIDE (per plane, decided by the entry): the four bases plus the plane's offset and the row pitch are multiples of
//                 16, so every access is one 16-byte load or store.  Otherwise the same 16 bytes are gathered sample by sample into the
//                 same four words (samples past the end of the row: 0, never stored) and stored sample by sample: one arithmetic for
//                 both, so the bits agree by construction.
// HBM-bound: cur once, out once, half of prev and of next at the kept rows, half of one of them at the rebuilt rows = 3.5 frames; the
// rows of C above and below are shared by two pairs and the second read is an L2 hit.  No LDS, no atomics.
#include "vsr_common.h"

#include "../../include/vsr_hip_deint.h"

namespace {

constexpr int kTX = 64, kTY = VSR_DEINT_TILE_ROWS / 2;   // threads: 64 chunks of 16 bytes x 4 row pairs
static_assert(kTX * 16 == VSR_DEINT_TILE_BYTES, "a workgroup's width is 64 threads of 16 bytes");

struct PlaneArg {
    size_t off;      // bytes from the base
    int rows;
    int row_bytes;   // cols * comps * sample_bytes
    int wide;        // every access of this plane is a 16-byte one
    unsigned bx;     // workgroups across a row
    unsigned first;  // the plane's first workgroup in the flat grid
};
struct Planes {
    PlaneArg p[VSR_DEINT_MAX_PLANES];
};

// steps 4 .. 8 of the header on values
__device__ inline int rule(int c, int e, int b, int a, int pu, int pd, int nu, int nd) {
    const int t = (b + a) >> 1, sp = (c + e) >> 1;
    const int td0 = abs(b - a);
    const int td1 = (abs(pu - c) + abs(pd - e)) >> 1;
    const int td2 = (abs(nu - c) + abs(nd - e)) >> 1;
    const int d = max(td0 >> 1, max(td1, td2));
    return min(max(sp, t - d), t + d);
}

// the 4 / SB samples of one 32-bit word
template <int SB>
__device__ inline unsigned rule_word(unsigned c, unsigned e, unsigned b, unsigned a, unsigned pu, unsigned pd, unsigned nu, unsigned nd,
                                     int shift) {
    constexpr int BITS = 8 * SB;
    constexpr unsigned MASK = (1u << BITS) - 1u;
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4 / SB; ++k) {
        const int s = BITS * k;
        const int v = rule((int)(((c >> s) & MASK) >> shift), (int)(((e >> s) & MASK) >> shift), (int)(((b >> s) & MASK) >> shift),
                           (int)(((a >> s) & MASK) >> shift), (int)(((pu >> s) & MASK) >> shift), (int)(((pd >> s) & MASK) >> shift),
                           (int)(((nu >> s) & MASK) >> shift), (int)(((nd >> s) & MASK) >> shift));
        r |= ((unsigned)v << shift) << s;
    }
    return r;
}

// one little-endian word at `p`, sample by sample; only the first `nb` bytes exist (the rest 0)
template <int SB>
__device__ inline unsigned load_word(const unsigned char* p, int nb) {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; j += SB)
        if (j < nb) w |= (SB == 2 ? (unsigned)*reinterpret_cast<const unsigned short*>(p + j) : (unsigned)p[j]) << (8 * j);
    return w;
}

template <int SB>
__device__ inline void store_word(unsigned char* p, int nb, unsigned w) {
#pragma unroll
    for (int j = 0; j < 4; j += SB) {
        if (j < nb) {
            if (SB == 2) *reinterpret_cast<unsigned short*>(p + j) = (unsigned short)(w >> (8 * j));
            else p[j] = (unsigned char)(w >> (8 * j));
        }
    }
}

// 16 bytes at `p` as four little-endian words; unless WIDE only the first `nb` bytes exist
template <int SB, bool WIDE>
__device__ inline uint4 load16(const unsigned char* p, int nb) {
    if constexpr (WIDE) return *reinterpret_cast<const uint4*>(p);
    else return make_uint4(load_word<SB>(p, nb), load_word<SB>(p + 4, nb - 4), load_word<SB>(p + 8, nb - 8), load_word<SB>(p + 12, nb - 12));
}

template <int SB, bool WIDE>
__device__ inline void store16(unsigned char* p, int nb, const uint4& v) {
    if constexpr (WIDE) {
        *reinterpret_cast<uint4*>(p) = v;
    } else {
        store_word<SB>(p, nb, v.x);
        store_word<SB>(p + 4, nb - 4, v.y);
        store_word<SB>(p + 8, nb - 8, v.z);
        store_word<SB>(p + 12, nb - 12, v.w);
    }
}

template <int SB, bool WIDE>
__device__ inline void pair16(const unsigned char* P, const unsigned char* C, const unsigned char* N, unsigned char* __restrict__ O,
                              int rows, size_t pitch, size_t xb, int nb, int pr, int shift, int keep, int kept_first) {
    const int yk = 2 * pr + keep, ym = 2 * pr + 1 - keep;   // the kept and the rebuilt row of pair `pr` (2 * pr < rows)
    if (ym >= rows) {   // half a pair: the last row of an odd plane is a kept one
        store16<SB, WIDE>(O + (size_t)yk * pitch + xb, nb, load16<SB, WIDE>(C + (size_t)yk * pitch + xb, nb));
        return;
    }
    int yu = ym - 1, yd = ym + 1;
    if (yu < 0) yu = yd;
    if (yd >= rows) yd = yu;
    const size_t ou = (size_t)yu * pitch + xb, om = (size_t)ym * pitch + xb, od = (size_t)yd * pitch + xb;
    const unsigned char* B = kept_first ? P : C;
    const unsigned char* A = kept_first ? C : N;
    const uint4 c = load16<SB, WIDE>(C + ou, nb), e = load16<SB, WIDE>(C + od, nb);
    const uint4 b = load16<SB, WIDE>(B + om, nb), a = load16<SB, WIDE>(A + om, nb);
    const uint4 pu = load16<SB, WIDE>(P + ou, nb), pd = load16<SB, WIDE>(P + od, nb);
    const uint4 nu = load16<SB, WIDE>(N + ou, nb), nd = load16<SB, WIDE>(N + od, nb);
    uint4 v;
    v.x = rule_word<SB>(c.x, e.x, b.x, a.x, pu.x, pd.x, nu.x, nd.x, shift);
    v.y = rule_word<SB>(c.y, e.y, b.y, a.y, pu.y, pd.y, nu.y, nd.y, shift);
    v.z = rule_word<SB>(c.z, e.z, b.z, a.z, pu.z, pd.z, nu.z, nd.z, shift);
    v.w = rule_word<SB>(c.w, e.w, b.w, a.w, pu.w, pd.w, nu.w, nd.w, shift);
    store16<SB, WIDE>(O + om, nb, v);
    // the kept row of the pair is the C row above (keep = 0: yk = ym - 1 = yu) or below (keep = 1: yk = ym + 1 = yd, when it exists)
    // (selected word by word: a select of the two uint4 goes through scratch)
    if (yk < rows)
        store16<SB, WIDE>(O + (size_t)yk * pitch + xb, nb, make_uint4(keep ? e.x : c.x, keep ? e.y : c.y, keep ? e.z : c.z, keep ? e.w : c.w));
}

template <int SB>
__global__ void __launch_bounds__(kTX * kTY)
k_deint(const unsigned char* prev, const unsigned char* cur, const unsigned char* next, unsigned char* __restrict__ out, Planes planes,
        int shift, int keep, int kept_first) {
    // the plane this workgroup belongs to (`first` of an absent plane is the grid's size; selects: no indexed copy in scratch)
    const unsigned g = blockIdx.x;
    const PlaneArg pl = g < planes.p[1].first ? planes.p[0] : g < planes.p[2].first ? planes.p[1] : planes.p[2];
    const unsigned local = g - pl.first, by = local / pl.bx, bx = local - by * pl.bx;
    const int pr = (int)by * kTY + threadIdx.y;
    const size_t xb = ((size_t)bx * kTX + threadIdx.x) * 16;
    if (2 * pr >= pl.rows || xb >= (size_t)pl.row_bytes) return;   // (the ragged last workgroup of a row or of the plane)
    const size_t left = (size_t)pl.row_bytes - xb;
    const int nb = left < 16 ? (int)left : 16;
    const unsigned char *P = prev + pl.off, *C = cur + pl.off, *N = next + pl.off;
    unsigned char* O = out + pl.off;
    if (pl.wide) pair16<SB, true>(P, C, N, O, pl.rows, (size_t)pl.row_bytes, xb, nb, pr, shift, keep, kept_first);
    else pair16<SB, false>(P, C, N, O, pl.rows, (size_t)pl.row_bytes, xb, nb, pr, shift, keep, kept_first);
}

}  // namespace

extern "C" {

int vsr_deint_abi_version(void) { return VSR_DEINT_ABI_VERSION; }
const char* vsr_deint_last_error(void) { return vsr::err_buf(); }

int vsr_deint_frame(const void* prev, const void* cur, const void* next, void* out, const vsr_deint_plane* planes, int n_planes,
                    int sample_bytes, int shift, int keep, int kept_first, vsr_stream_t stream) {
    VSR_REQUIRE(prev && cur && next && out && planes, "deint_frame: null pointer");
    VSR_REQUIRE(n_planes >= 1 && n_planes <= VSR_DEINT_MAX_PLANES, "deint_frame: n_planes %d outside 1..%d", n_planes, VSR_DEINT_MAX_PLANES);
    VSR_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "deint_frame: sample_bytes %d is not 1 or 2", sample_bytes);
    VSR_REQUIRE(shift == 0 || shift == 6, "deint_frame: shift %d is not 0 or 6", shift);
    VSR_REQUIRE(shift == 0 || sample_bytes == 2, "deint_frame: shift 6 needs 16-bit samples (sample_bytes 2)");
    VSR_REQUIRE((keep == 0 || keep == 1) && (kept_first == 0 || kept_first == 1), "deint_frame: keep %d and kept_first %d must each be 0 or 1",
                keep, kept_first);
    const uintptr_t base[4] = {reinterpret_cast<uintptr_t>(prev), reinterpret_cast<uintptr_t>(cur), reinterpret_cast<uintptr_t>(next),
                               reinterpret_cast<uintptr_t>(out)};
    VSR_REQUIRE(sample_bytes == 1 || ((base[0] | base[1] | base[2] | base[3]) & 1) == 0, "deint_frame: 16-bit samples at an odd byte address");
    Planes arg = {};
    long long total = 0;
    for (int i = 0; i < n_planes; ++i) {
        const vsr_deint_plane& q = planes[i];
        VSR_REQUIRE(q.cols > 0 && q.comps > 0, "deint_frame: plane %d: cols %d and comps %d must be positive", i, q.cols, q.comps);
        VSR_REQUIRE(q.comps <= 2, "deint_frame: plane %d: comps %d beyond 2", i, q.comps);
        VSR_REQUIRE(q.rows >= 2, "deint_frame: plane %d has %d rows (two fields need at least 2)", i, q.rows);
        VSR_REQUIRE(sample_bytes == 1 || (q.offset & 1) == 0, "deint_frame: plane %d: 16-bit samples at an odd byte offset %zu", i, q.offset);
        const long long samples = (long long)q.cols * q.comps;
        VSR_REQUIRE(q.rows <= 65535 * VSR_DEINT_TILE_ROWS && samples <= (1ll << 30),
                    "deint_frame: grid overflow (plane %d: %d rows beyond %d or a row of %lld samples beyond 2^30)", i, q.rows,
                    65535 * VSR_DEINT_TILE_ROWS, samples);
        const long long row_bytes = samples * sample_bytes;   // <= 2^31
        VSR_REQUIRE(row_bytes <= 0x7fffffffll, "deint_frame: grid overflow (plane %d: a row of %lld bytes)", i, row_bytes);
        PlaneArg& a = arg.p[i];
        a.off = q.offset;
        a.rows = q.rows;
        a.row_bytes = (int)row_bytes;
        a.wide = ((base[0] | base[1] | base[2] | base[3] | q.offset | (uintptr_t)row_bytes) & 15) == 0;
        const long long bx = vsr::cdiv(vsr::cdiv(row_bytes, 16), kTX), by = vsr::cdiv((q.rows + 1) / 2, kTY);
        a.bx = (unsigned)bx;
        a.first = (unsigned)total;
        total += bx * by;
        VSR_REQUIRE(total <= 0x7fffffffll, "deint_frame: grid overflow (%lld workgroups up to plane %d)", total, i);
    }
    for (int i = n_planes; i < VSR_DEINT_MAX_PLANES; ++i) arg.p[i].first = (unsigned)total, arg.p[i].bx = 1;   // absent: no workgroup is below it
    VSR_REQUIRE(out != prev && out != cur && out != next, "deint_frame: out is one of the inputs (it must not overlap any of them)");
    const dim3 grid((unsigned)total), block(kTX, kTY);
    hipStream_t s = vsr::S(stream);
    const unsigned char *p = (const unsigned char*)prev, *c = (const unsigned char*)cur, *n = (const unsigned char*)next;
    if (sample_bytes == 2) hipLaunchKernelGGL((k_deint<2>), grid, block, 0, s, p, c, n, (unsigned char*)out, arg, shift, keep, kept_first);
    else hipLaunchKernelGGL((k_deint<1>), grid, block, 0, s, p, c, n, (unsigned char*)out, arg, shift, keep, kept_first);
    return vsr::launched("deint_frame");
}

}  // extern "C"
