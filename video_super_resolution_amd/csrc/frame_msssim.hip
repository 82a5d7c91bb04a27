// frame_msssim.hip -- HR frames scored against ground truth on the device at five scales (include/vsr_hip_msssim.h;
// libvsr_hip_msssim.so is built from this source alone): per frame, plane and level the float64 sums behind multi-scale SSIM.
//
//   k_pyramid : one workgroup (4 waves) = one level-1 tile of PR = 16 rows x PC = 64 columns of the shaved plane, all planes, both
//               frames.  The tile's origin is a multiple of 16 both ways, so it holds every descendant of its pixels at levels 2 to 5
//               (8 x 32, 4 x 16, 2 x 8, 1 x 4 positions), the clamped last row / column of an odd size included: level j + 1 reads rows
//               2 y and min(2 y + 1, h_j - 1) of level j, both inside the tile.  Wave v stages rows 4 v .. 4 v + 3 of a and b in LDS as
//               they lie in memory (WIDE: one aligned 16-byte load per lane; otherwise element loads); thread (y, x) forms the level-2
//               value of each plane and frame from its 2 x 2 pixels (quantise, luma or channel, to double); levels 3 to 5 follow from
//               LDS with 64, 16 and 4 threads.  Every value goes to the workspace as a double; level 1 never does.
//   k_score   : one workgroup (4 waves) = one tile of SW = 64 map columns x SR = 64 map rows of ONE level of one frame; the grid's x
//               runs over the tiles of level 1, then level 2, ... level 5.  The tile is scored by the march of frame_ssim.h, the one
//               k_metric of frame_metric.hip runs: a level-1 tile stages and converts the float32 frames (load, convert), a tile of a
//               higher level reads its row of doubles from the workspace straight into the converted row.  Two running sums per
//               thread (cs, ssim), at the end of a plane's pass a fixed-order tree over the 256 threads and one pair of doubles per
//               plane into the workspace.
//   k_finish  : one workgroup of 64 threads per (level, plane, frame): thread t adds the level's partials t, t + 64, ... in that order,
//               then the same tree; thread 0 writes the two numbers.
// Nothing here is atomic and no order depends on timing or on F: a frame's numbers are the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): luma, the 2 x 2 mean and the two
// formulas round operation by operation as the header writes them; the window sums ask for their fmas by name.
#include "frame_ssim.h"

#include "../../include/vsr_hip_msssim.h"

#pragma clang fp contract(off)

namespace {

using namespace vsr::ssim;

constexpr int NL = VSR_MSSSIM_LEVELS;
constexpr int PR = VSR_MSSSIM_PYR_ROWS, PC = VSR_MSSSIM_PYR_COLS, FT = VSR_MSSSIM_FINISH_THREADS;
constexpr int PYR = 8 * 32 + 4 * 16 + 2 * 8 + 1 * 4;   // doubles of one plane's descendants of a pyramid tile
static_assert(VSR_MSSSIM_STRIP_WIDTH == SW && VSR_MSSSIM_SEGMENT_ROWS == SR, "the header's tile is the march's");

// the five levels of one call: sizes, where a level's pooled planes start inside one plane's block of the workspace (levels 2 to 5),
// and the scoring tiles, numbered level by level
struct Plan {
    int h[NL], w[NL];
    unsigned strips[NL], t0[NL + 1];
    unsigned long long off[NL], plane_doubles;   // off[0] is unused: level 1 is the frames themselves
};

template <bool YMODE, bool QUANT, bool WIDE>
__global__ void __launch_bounds__(NW * 64)
k_pyramid(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int shave, Luma lu, Plan pl, double* __restrict__ pyr) {
    constexpr int P = YMODE ? 1 : 3;
    __shared__ __align__(16) float raw[PR][2][RAW];
    __shared__ int start[PR];
    __shared__ double lv[2][P][PYR];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x0 = blockIdx.x * PC, y0 = blockIdx.y * PR;
    const int n1r = min(PR, pl.h[0] - y0), n1c = min(PC, pl.w[0] - x0);
    const size_t frame = (size_t)blockIdx.z * H * W * 3;
    const float* __restrict__ fa = a + frame;
    const float* __restrict__ fb = b + frame;
    // ---- load: wave v takes rows 4 v .. 4 v + 3
#pragma unroll
    for (int k = 0; k < PR / NW; ++k) {
        const int r = wv * (PR / NW) + k;
        if (r < n1r) {
            const size_t s = ((size_t)(shave + y0 + r) * W + shave + x0) * 3;
            const int o = stage_row<WIDE>(raw[r], fa, fb, s, n1c * 3, lane);
            if (lane == 0) start[r] = o;
        }
    }
    __syncthreads();
    // ---- levels 2 to 5: level k + 1 has (PR >> k) x (PC >> k) positions in the tile
    int nr = n1r, nc = n1c;   // the valid rows / columns of the level below
    int src = 0, dst = 0;     // where the level below / this level start in lv[][][]
#pragma unroll
    for (int k = 1; k < NL; ++k) {
        const int rows = PR >> k, cols = PC >> k;
        const int mr = (nr + 1) >> 1, mc = (nc + 1) >> 1;
        const int ty = tid / cols, tx = tid % cols;
        if (tid < rows * cols && ty < mr && tx < mc) {
            const int r0 = 2 * ty, r1 = min(2 * ty + 1, nr - 1), c0 = 2 * tx, c1 = min(2 * tx + 1, nc - 1);
            const size_t at = pl.off[k] + (size_t)((y0 >> k) + ty) * pl.w[k] + (x0 >> k) + tx;
#pragma unroll
            for (int ab = 0; ab < 2; ++ab)
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    double p00, p01, p10, p11;
                    if (k == 1) {
                        const float* q0 = &raw[r0][ab][start[r0]];
                        const float* q1 = &raw[r1][ab][start[r1]];
                        p00 = level1<YMODE, QUANT>(q0 + 3 * c0, p, lu);
                        p01 = level1<YMODE, QUANT>(q0 + 3 * c1, p, lu);
                        p10 = level1<YMODE, QUANT>(q1 + 3 * c0, p, lu);
                        p11 = level1<YMODE, QUANT>(q1 + 3 * c1, p, lu);
                    } else {
                        const double* q = &lv[ab][p][src];
                        const int pitch = cols * 2;
                        p00 = q[r0 * pitch + c0], p01 = q[r0 * pitch + c1], p10 = q[r1 * pitch + c0], p11 = q[r1 * pitch + c1];
                    }
                    const double m = ((p00 + p01) + (p10 + p11)) * 0.25;
                    lv[ab][p][dst + ty * cols + tx] = m;
                    pyr[(((size_t)blockIdx.z * 2 + ab) * P + p) * pl.plane_doubles + at] = m;
                }
        }
        __syncthreads();
        nr = mr, nc = mc;
        src = dst, dst += rows * cols;
    }
}

template <bool YMODE, bool QUANT, bool WIDE>
__global__ void __launch_bounds__(NW * 64)
k_score(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int shave, Luma lu, Win win, Plan pl,
        const double* __restrict__ pyr, double* __restrict__ part) {
    constexpr int P = YMODE ? 1 : 3;
    constexpr int HALO = K - 1;
    __shared__ __align__(16) float raw[NW][2][RAW];
    __shared__ double xs[NW][2][XS];
    __shared__ double ring[RING][5][SW];
    __shared__ double red[2][NW * 64];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int lev = 0;
#pragma unroll
    for (int j = 1; j < NL; ++j) lev += blockIdx.x >= pl.t0[j] ? 1 : 0;
    const unsigned tile = blockIdx.x - pl.t0[lev];
    const int h = pl.h[lev], w = pl.w[lev];
    const int mh = h - HALO, mw = w - HALO;                  // the map of this level
    const int ox0 = (tile % pl.strips[lev]) * SW, oy0 = (tile / pl.strips[lev]) * SR;
    const int ncols_out = min(SW, mw - ox0), nrows_out = min(SR, mh - oy0);
    const int ncols_in = ncols_out + HALO, nrows_in = nrows_out + HALO;
    const size_t frame = (size_t)blockIdx.z * H * W * 3;
    const float* __restrict__ fa = a + frame;
    const float* __restrict__ fb = b + frame;
    const int nfl = ncols_in * 3;                            // floats of a row of a level-1 tile
    const int nsteps = (nrows_in + NW - 1) / NW;

    for (int p = 0; p < P; ++p) {
        // the pooled planes of this level (levels 2 to 5)
        const double* __restrict__ da = pyr + (((size_t)blockIdx.z * 2 + 0) * P + p) * pl.plane_doubles + pl.off[lev];
        const double* __restrict__ db = pyr + (((size_t)blockIdx.z * 2 + 1) * P + p) * pl.plane_doubles + pl.off[lev];
        double cs = 0.0, ssim = 0.0;
        for (int t = 0; t < nsteps; ++t) {
            const int ri = t * NW + wv;                      // input row of this wave, relative to the tile
            const bool row_on = ri < nrows_in;
            if (lev == 0) {
                int o = 0;                                   // where the row starts in raw[]
                // ---- load
                if (row_on) {
                    const size_t s = ((size_t)(shave + oy0 + ri) * W + shave + ox0) * 3;
                    o = stage_row<WIDE>(raw[wv], fa, fb, s, nfl, lane);
                }
                __syncthreads();
                // ---- convert
                if (row_on) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int j = lane + 64 * k;
                        if (j < ncols_in) {
                            xs[wv][0][j] = level1<YMODE, QUANT>(&raw[wv][0][o + 3 * j], p, lu);
                            xs[wv][1][j] = level1<YMODE, QUANT>(&raw[wv][1][o + 3 * j], p, lu);
                        }
                    }
                }
            } else if (row_on) {
                // ---- load: the row of doubles as the pyramid pass left it
                const size_t s = (size_t)(oy0 + ri) * w + ox0;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int j = lane + 64 * k;
                    if (j < ncols_in) {
                        xs[wv][0][j] = da[s + j];
                        xs[wv][1][j] = db[s + j];
                    }
                }
            }
            __syncthreads();
            if (row_on && lane < ncols_out) row_pass(win, &xs[wv][0][lane], &xs[wv][1][lane], ring[ri % RING], lane);
            __syncthreads();
            const int q = t * NW + wv - (K - 1);
            if (q >= 0 && q < nrows_out && lane < ncols_out) {
                const Terms m = column_pass(win, ring, q, lane);
                cs += m.num_cs / m.den_cs;
                ssim += (m.num_l * m.num_cs) / (m.den_l * m.den_cs);
            }
            // (the next step's ring stores come after a barrier of that step, two at level 1: every read above has been issued by
            // then; xs[wv] is written and read by wave wv alone)
        }
        // ---- a pass is over: the threads' sums through the tree, one pair per plane
        vsr::sums::tree_pair<NW * 64>(red, tid, cs, ssim);
        if (tid == 0) {
            double* out = part + (((size_t)blockIdx.z * P + p) * pl.t0[NL] + blockIdx.x) * 2;
            out[0] = red[0][0];
            out[1] = red[1][0];
        }
        __syncthreads();   // the ring, the staging rows and red[] are free for the next plane
    }
}

// grid (level, plane, frame)
__global__ void __launch_bounds__(FT)
k_finish(const double* __restrict__ part, double* __restrict__ sums, Plan pl) {
    __shared__ double red[2][FT];
    const int tid = threadIdx.x, lev = blockIdx.x;
    const size_t fp = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    vsr::sums::finish_pair<FT>(part + fp * pl.t0[NL] * 2, pl.t0[lev], pl.t0[lev + 1], red, tid);
    if (tid == 0) {
        double* out = sums + (fp * NL + lev) * 2;
        out[0] = red[0][0];
        out[1] = red[1][0];
    }
}

// the checks vsr_msssim_ws_bytes and vsr_msssim_frames share; `pl` only when the result is VSR_OK
int check_shape(int F, int H, int W, int shave, int channels, Plan* pl) {
    VSR_REQUIRE(channels == VSR_MSSSIM_RGB || channels == VSR_MSSSIM_Y, "msssim_frames: unknown channels %d", channels);
    VSR_REQUIRE(F > 0 && H > 0 && W > 0, "msssim_frames: bad shape (F %d, H %d, W %d)", F, H, W);
    VSR_REQUIRE(shave >= 0, "msssim_frames: bad shave %d", shave);
    const long long m = (long long)(H < W ? H : W) - 2 * (long long)shave;
    VSR_REQUIRE(m >= VSR_MSSSIM_MIN_SIZE, "msssim_frames: five levels need %d pixels each way after the shave, got %lld",
                VSR_MSSSIM_MIN_SIZE, m);
    VSR_REQUIRE(F <= 65535 && H <= 65535 && W <= 65535, "msssim_frames: grid overflow (F %d, H %d, W %d beyond 65535)", F, H, W);
    int h = H - 2 * shave, w = W - 2 * shave;
    unsigned long long off = 0;
    pl->t0[0] = 0;
    for (int j = 0; j < NL; ++j) {
        pl->h[j] = h, pl->w[j] = w;
        pl->off[j] = j ? off : 0;
        if (j) off += (unsigned long long)h * w;
        pl->strips[j] = vsr::cdiv(w - (K - 1), SW);
        pl->t0[j + 1] = pl->t0[j] + pl->strips[j] * vsr::cdiv(h - (K - 1), SR);
        h = (h + 1) / 2, w = (w + 1) / 2;
    }
    pl->plane_doubles = off;
    return VSR_OK;
}

}  // namespace

extern "C" {

int vsr_msssim_abi_version(void) { return VSR_MSSSIM_ABI_VERSION; }
const char* vsr_msssim_last_error(void) { return vsr::err_buf(); }

size_t vsr_msssim_ws_bytes(int F, int H, int W, int shave, int channels) {
    Plan pl;
    if (check_shape(F, H, W, shave, channels, &pl) != VSR_OK) return 0;
    const size_t P = channels == VSR_MSSSIM_Y ? 1 : 3;
    return (size_t)F * P * (2 * (size_t)pl.plane_doubles + 2 * (size_t)pl.t0[NL]) * sizeof(double);
}

int vsr_msssim_frames(const float* a, const float* b, int F, int H, int W, int channels, int quantise, int shave, const float* luma4,
                      const double* win11, double* sums, void* ws, vsr_stream_t stream) {
    const char* who = "msssim_frames";
    Plan pl;
    bool wide;
    if (int rc = check_pointers(who, a, b, sums, ws)) return rc;
    VSR_REQUIRE(win11, "msssim_frames: null win11");
    if (int rc = check_shape(F, H, W, shave, channels, &pl)) return rc;
    if (int rc = check_quantise(who, quantise)) return rc;
    const bool ymode = channels == VSR_MSSSIM_Y;
    if (int rc = check_frames(who, ymode, luma4, a, b, W, sums, ws, &wide)) return rc;
    const Win win = win_of(win11);
    const Luma lu = ymode ? vsr::sums::luma_of(luma4) : Luma{};
    const int P = ymode ? 1 : 3;
    // the workspace: the pooled planes [F][2][P][plane_doubles], then the partials [F][P][tiles][2]
    double* pyr = static_cast<double*>(ws);
    double* part = pyr + (size_t)F * 2 * P * pl.plane_doubles;
    const dim3 pgrid(vsr::cdiv(pl.w[0], PC), vsr::cdiv(pl.h[0], PR), F), sgrid(pl.t0[NL], 1, F), block(NW * 64);
    hipStream_t s = vsr::S(stream);
    int rc = VSR_OK;
    dispatch(quantise != 0, wide, [&](auto Q_, auto W_) {
        constexpr bool Q = decltype(Q_)::value, WD = decltype(W_)::value;
        const auto both = [&](auto Y_) {
            constexpr bool Y = decltype(Y_)::value;
            hipLaunchKernelGGL((k_pyramid<Y, Q, WD>), pgrid, block, 0, s, a, b, H, W, shave, lu, pl, pyr);
            rc = vsr::launched("msssim_frames/pyramid");
            if (rc) return;
            hipLaunchKernelGGL((k_score<Y, Q, WD>), sgrid, block, 0, s, a, b, H, W, shave, lu, win, pl, (const double*)pyr, part);
            rc = vsr::launched("msssim_frames/tiles");
        };
        if (ymode) both(std::true_type{});
        else both(std::false_type{});
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(NL, P, F), dim3(FT), 0, s, (const double*)part, sums, pl);
    return vsr::launched("msssim_frames/finish");
}

}  // extern "C"
