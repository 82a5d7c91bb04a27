// train_patch.hip -- training samples cut from frames on the device (include/vsr_hip_patch.h; libvsr_hip_patch.so is built from this
// source alone): a run of n frames cropped, flipped, transposed and reversed in time, and the LR patch that belongs to it.
//
//   k_gather : one workgroup of WT = 256 threads = one tile of T x T = VSR_PATCH_TILE^2 output pixels of one frame of one sample
//              (grid = (HR tiles + LR tiles, n, B)).  A tile is T rows of T * 3 = 96 words.  The two regions of grid.x run the same body
//              on two `Job`s: where the source is, how large its frames are, by how much the origin is divided and with which step the
//              source is walked (the nearest LR patch walks `src` with step S; the other two jobs walk their source with step 1).
//              Without TRANSPOSE thread e of the tile takes word e % 96 of row e / 96: source and output both run along a row, and a
//              horizontal flip only reverses the order of the pixels inside the 384 bytes a tile row covers.  A thread's 12 loads are all
//              issued before its first store (a load-store pair per iteration took 30.9 us where this takes 20.6: LAB_NOTES).
//              With TRANSPOSE the tile is read along source rows into LDS as [source row][source column] and written along output rows
//              from [output column][output row].  Row pitch LP = 99 words: a write takes consecutive words (no conflict); a read has lane
//              (column jl, word c) at jl * 99 + c + const, bank (3 jl + c + const) % 32 under the modulus of ds_read_b32: the 32 lanes of
//              a half-wave (jl = 0..10, c = 0..2) fall on 32 consecutive values of 3 jl + c, one bank each.  (The pitch 97 would be odd
//              too and gives bank jl + c: three lanes on a bank.)
// The table travels by value in the kernel arguments; every row was validated on the host, so the kernel tests only the tile's ragged edge.
#include <cstdint>

#include "vsr_common.h"

#include "../../include/vsr_hip_patch.h"

namespace {

constexpr int T = VSR_PATCH_TILE, MAXB = VSR_PATCH_MAX_B;
constexpr int WT = 256;
constexpr int ROW = T * 3;               // words of a tile row
constexpr int LP = ROW + 3;              // LDS pitch in words: 3 (mod 32), see above
constexpr int ITER = T * ROW / WT;       // words per thread
static_assert(T * ROW % WT == 0, "a tile is a whole number of words per thread");
static_assert(LP % 32 == 3, "the transposed read is conflict-free for a pitch of 3 modulo 32");

struct Row {
    int t0, y0, x0, flags;
};
struct Table {
    Row row[MAXB];
};

// one gather: out [B,n,oh,ow,3] from frames of fh x fw pixels at `src`; a row's origin is divided by `div`, the source walked by `step`
struct Job {
    const uint32_t* src;
    uint32_t* out;
    int fh, fw, oh, ow, div, step;
    unsigned tiles_x, tiles;
};

__device__ inline void gather_tile(const Job& J, const Row r, unsigned tile, int k, int b, int n, uint32_t* lds) {
    const int tid = threadIdx.x;
    const bool tr = r.flags & VSR_PATCH_TRANSPOSE;
    const int i0 = (int)(tile / J.tiles_x) * T, j0 = (int)(tile % J.tiles_x) * T;
    const int kk = (r.flags & VSR_PATCH_REVERSE_TIME) ? n - 1 - k : k;
    const int ch = tr ? J.ow : J.oh, cw = tr ? J.oh : J.ow;   // the crop in units of output pixels
    // source row of u: oy + sy * u, source column of v: ox + sx * v (in pixels of the job's source)
    const int oy = r.y0 / J.div + ((r.flags & VSR_PATCH_FLIP_Y) ? J.step * ch - 1 : 0);
    const int ox = r.x0 / J.div + ((r.flags & VSR_PATCH_FLIP_X) ? J.step * cw - 1 : 0);
    const int sy = (r.flags & VSR_PATCH_FLIP_Y) ? -J.step : J.step;
    const int sx = (r.flags & VSR_PATCH_FLIP_X) ? -J.step : J.step;
    const uint32_t* __restrict__ fsrc = J.src + (size_t)(r.t0 + kk) * J.fh * J.fw * 3;
    uint32_t* __restrict__ fout = J.out + ((size_t)b * n + k) * J.oh * J.ow * 3;
    if (!tr) {
        uint32_t v[ITER];   // all of a thread's loads in flight before its first store
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int e = it * WT + tid;
            const int row = e / ROW, d = e - row * ROW, px = d / 3, c = d - px * 3;
            const int i = i0 + row, j = j0 + px;
            v[it] = (i < J.oh && j < J.ow) ? fsrc[((size_t)(oy + sy * i) * J.fw + (ox + sx * j)) * 3 + c] : 0u;
        }
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int e = it * WT + tid;
            const int row = e / ROW, d = e - row * ROW, px = d / 3;
            const int i = i0 + row, j = j0 + px;
            if (i < J.oh && j < J.ow) fout[((size_t)i * J.ow + j) * 3 + (d - px * 3)] = v[it];
        }
        return;
    }
    // transposed: output (i, j) is source (u, v) = (j, i).  In: LDS row jl = the source row of output column j0 + jl.
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int e = it * WT + tid;
        const int jl = e / ROW, d = e - jl * ROW, il = d / 3, c = d - il * 3;
        const int i = i0 + il, j = j0 + jl;
        if (i < J.oh && j < J.ow) lds[jl * LP + d] = fsrc[((size_t)(oy + sy * j) * J.fw + (ox + sx * i)) * 3 + c];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int e = it * WT + tid;
        const int il = e / ROW, d = e - il * ROW, jl = d / 3, c = d - jl * 3;
        const int i = i0 + il, j = j0 + jl;
        if (i < J.oh && j < J.ow) fout[((size_t)i * J.ow + j) * 3 + c] = lds[jl * LP + il * 3 + c];
    }
}

__global__ void __launch_bounds__(WT)
k_gather(Job hr, Job lr, Table table, int n) {
    __shared__ uint32_t lds[T * LP];
    const int b = blockIdx.z, k = blockIdx.y;
    const Row r = table.row[b];
    if (blockIdx.x < hr.tiles) gather_tile(hr, r, blockIdx.x, k, b, n, lds);
    else gather_tile(lr, r, blockIdx.x - hr.tiles, k, b, n, lds);
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

inline bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
    return addr(a) < addr(b) + nb && addr(b) < addr(a) + na;
}

Job job(const float* src, float* out, int fh, int fw, int oh, int ow, int div, int step) {
    Job j;
    j.src = reinterpret_cast<const uint32_t*>(src);
    j.out = reinterpret_cast<uint32_t*>(out);
    j.fh = fh, j.fw = fw, j.oh = oh, j.ow = ow, j.div = div, j.step = step;
    j.tiles_x = vsr::cdiv(ow, T);
    j.tiles = out ? j.tiles_x * vsr::cdiv(oh, T) : 0;
    return j;
}

}  // namespace

extern "C" {

int vsr_patch_abi_version(void) { return VSR_PATCH_ABI_VERSION; }
const char* vsr_patch_last_error(void) { return vsr::err_buf(); }

int vsr_patch_gather(const float* src, int G, int H, int W, const float* lr_src_or_null, int S, const int* table, int B, int n, int Ph,
                     int Pw, float* hr_or_null, float* lr_or_null, vsr_stream_t stream) {
    VSR_REQUIRE(src, "patch_gather: null src");
    VSR_REQUIRE(table, "patch_gather: null table (a host pointer to B rows of {t0, y0, x0, flags})");
    VSR_REQUIRE(hr_or_null || lr_or_null, "patch_gather: both outputs are null");
    VSR_REQUIRE(G > 0 && H > 0 && W > 0, "patch_gather: bad source shape (%d frames of %d x %d)", G, H, W);
    VSR_REQUIRE(B > 0 && n > 0 && Ph > 0 && Pw > 0, "patch_gather: bad sample shape (B %d, n %d, patch of %d x %d)", B, n, Ph, Pw);
    VSR_REQUIRE(S >= 1 && S <= 8, "patch_gather: S must lie in 1..8, got %d", S);
    VSR_REQUIRE(Ph % S == 0 && Pw % S == 0, "patch_gather: the patch of %d x %d is no multiple of S = %d", Ph, Pw, S);
    VSR_REQUIRE(B <= MAXB, "patch_gather: B = %d is beyond VSR_PATCH_MAX_B = %d (the table travels in the kernel arguments)", B, MAXB);
    VSR_REQUIRE(G <= 65535 && H <= 65535 && W <= 65535 && n <= 65535 && Ph <= 65535 && Pw <= 65535,
                "patch_gather: grid overflow (G %d, H %d, W %d, n %d, patch of %d x %d beyond 65535)", G, H, W, n, Ph, Pw);
    if (lr_src_or_null)
        VSR_REQUIRE(H % S == 0 && W % S == 0, "patch_gather: with lr_src the frames of %d x %d must be a multiple of S = %d", H, W, S);
    Table t;
    for (int b = 0; b < B; ++b) {
        const Row r = {table[4 * b], table[4 * b + 1], table[4 * b + 2], table[4 * b + 3]};
        VSR_REQUIRE((r.flags & ~15) == 0, "patch_gather: row %d has unknown flag bits (flags %d; known: 1 | 2 | 4 | 8)", b, r.flags);
        VSR_REQUIRE(r.t0 >= 0 && r.t0 <= G - n, "patch_gather: row %d takes frames %d .. %d of %d", b, r.t0, r.t0 + n - 1, G);
        const bool tr = r.flags & VSR_PATCH_TRANSPOSE;
        const int ch = tr ? Pw : Ph, cw = tr ? Ph : Pw;
        VSR_REQUIRE(r.y0 >= 0 && r.x0 >= 0 && r.y0 <= H - ch && r.x0 <= W - cw,
                    "patch_gather: row %d: the crop of %d x %d at (%d, %d) leaves the frame of %d x %d", b, ch, cw, r.y0, r.x0, H, W);
        if (lr_src_or_null)
            VSR_REQUIRE(r.y0 % S == 0 && r.x0 % S == 0, "patch_gather: row %d: with lr_src the origin (%d, %d) must be a multiple of S = %d", b,
                        r.y0, r.x0, S);
        t.row[b] = r;
    }
    for (int b = B; b < MAXB; ++b) t.row[b] = Row{0, 0, 0, 0};
    VSR_REQUIRE(((addr(src) | addr(lr_src_or_null) | addr(hr_or_null) | addr(lr_or_null)) & 3) == 0,
                "patch_gather: the frames and the patches must be 4-byte aligned");
    const unsigned long long src_bytes = 12ull * G * H * W, lsrc_bytes = 12ull * G * (H / S) * (W / S);
    const unsigned long long hr_bytes = 12ull * B * n * Ph * Pw, lr_bytes = 12ull * B * n * (Ph / S) * (Pw / S);
    VSR_REQUIRE(!hr_or_null || !overlap(hr_or_null, hr_bytes, src, src_bytes), "patch_gather: hr overlaps src");
    VSR_REQUIRE(!lr_or_null || !overlap(lr_or_null, lr_bytes, src, src_bytes), "patch_gather: lr overlaps src");
    if (lr_src_or_null) {
        VSR_REQUIRE(!hr_or_null || !overlap(hr_or_null, hr_bytes, lr_src_or_null, lsrc_bytes), "patch_gather: hr overlaps lr_src");
        VSR_REQUIRE(!lr_or_null || !overlap(lr_or_null, lr_bytes, lr_src_or_null, lsrc_bytes), "patch_gather: lr overlaps lr_src");
    }
    VSR_REQUIRE(!hr_or_null || !lr_or_null || !overlap(hr_or_null, hr_bytes, lr_or_null, lr_bytes), "patch_gather: hr overlaps lr");
    const Job jh = job(src, hr_or_null, H, W, Ph, Pw, 1, 1);
    const Job jl = lr_src_or_null ? job(lr_src_or_null, lr_or_null, H / S, W / S, Ph / S, Pw / S, S, 1)
                                  : job(src, lr_or_null, H, W, Ph / S, Pw / S, 1, S);
    hipLaunchKernelGGL(k_gather, dim3(jh.tiles + jl.tiles, n, B), dim3(WT), 0, vsr::S(stream), jh, jl, t, n);
    return vsr::launched("patch_gather");
}

}  // extern "C"
