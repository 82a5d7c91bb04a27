// frame_metric.hip -- HR frames scored against ground truth on the device (include/vsr_hip_metric.h; libvsr_hip_metric.so is built
// from this source alone): per frame the float64 sums behind PSNR and SSIM.
//
//   k_metric : one workgroup (4 waves) = one tile of SW = 64 map columns x SR = 64 map rows of one frame, scored by the march of
//              frame_ssim.h (load, convert, rows, columns; three barriers per step); with SSIM the tile reads (SW + 10) x (SR + 10)
//              pixels of the shaved plane, without it the map IS the plane, there is no halo and the march ends at convert.  A frame
//              is read about once plus halo from HBM; the second and third plane of RGB read their rows again through the L2 of the
//              same compute unit.  SSE is taken in the convert step, from the pixels the tile OWNS (the first SW x SR of its rectangle;
//              the last strip / segment also owns its halo), in the first pass for all three channels; in Y mode the luma is formed
//              once, for the SSE and for the converted row.  At the end a fixed-order tree over the 256 threads and one pair of
//              doubles into the workspace.
//   k_finish : one workgroup of 64 threads per frame: thread t adds the partials t, t + 64, ... in that order, then the same tree;
//              thread 0 writes the frame's four numbers (0 in the slots not asked for).
// Nothing here is atomic and no order depends on timing or on F: a frame's numbers are the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): luma, the SSE terms and the SSIM
// formula round operation by operation as the header writes them; the window sums ask for their fmas by name.
#include "frame_ssim.h"

#include "../../include/vsr_hip_metric.h"

#pragma clang fp contract(off)

namespace {

using namespace vsr::ssim;

constexpr int FT = VSR_METRIC_FINISH_THREADS;
static_assert(VSR_METRIC_STRIP_WIDTH == SW && VSR_METRIC_SEGMENT_ROWS == SR, "the header's tile is the march's");

template <bool SSIM, bool YMODE, bool QUANT, bool WIDE>
__global__ void __launch_bounds__(NW * 64)
k_metric(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int shave, int want_sse, Luma lu, Win win,
         double* __restrict__ ws) {
    constexpr int HALO = SSIM ? K - 1 : 0;
    __shared__ __align__(16) float raw[NW][2][RAW];
    __shared__ double xs[NW][2][XS];
    __shared__ double ring[SSIM ? RING : 1][5][SW];
    __shared__ double red[2][NW * 64];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h = H - 2 * shave, w = W - 2 * shave;
    const int mh = h - HALO, mw = w - HALO;                 // the map; without SSIM the plane itself
    const int ox0 = blockIdx.x * SW, oy0 = blockIdx.y * SR;
    const int ncols_out = min(SW, mw - ox0), nrows_out = min(SR, mh - oy0);
    const int ncols_in = ncols_out + HALO, nrows_in = nrows_out + HALO;
    const bool last_strip = blockIdx.x == gridDim.x - 1, last_seg = blockIdx.y == gridDim.y - 1;
    const size_t frame = (size_t)blockIdx.z * H * W * 3;
    const float* __restrict__ fa = a + frame;
    const float* __restrict__ fb = b + frame;
    const int nfl = ncols_in * 3;                            // floats of a row of the tile
    const int nsteps = (nrows_in + NW - 1) / NW;
    const int planes = (SSIM && !YMODE) ? 3 : 1;             // passes of the march (SSE alone: one pass takes all three channels)

    double sse = 0.0, ssim = 0.0;
    for (int p = 0; p < planes; ++p) {
        const bool do_sse = want_sse && p == 0;
        for (int t = 0; t < nsteps; ++t) {
            const int ri = t * NW + wv;                      // input row of this wave, relative to the tile
            const bool row_on = ri < nrows_in;
            int o = 0;                                       // where the row starts in raw[]
            // ---- load
            if (row_on) {
                const size_t s = ((size_t)(shave + oy0 + ri) * W + shave + ox0) * 3;
                o = stage_row<WIDE>(raw[wv], fa, fb, s, nfl, lane);
            }
            __syncthreads();
            // ---- convert (+ SSE)
            if (row_on) {
                const bool row_owned = ri < SR || last_seg;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int j = lane + 64 * k;
                    if (j < ncols_in) {
                        const float* qa = &raw[wv][0][o + 3 * j];
                        const float* qb = &raw[wv][1][o + 3 * j];
                        const bool owned = do_sse && row_owned && (j < SW || last_strip);
                        if (YMODE || owned) {
                            float ra[3], rb[3];
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                ra[c] = QUANT ? quant(qa[c]) : qa[c];
                                rb[c] = QUANT ? quant(qb[c]) : qb[c];
                            }
                            if (YMODE) {
                                const double ya = vsr::sums::luma(lu, ra[0], ra[1], ra[2]);
                                const double yb = vsr::sums::luma(lu, rb[0], rb[1], rb[2]);
                                if (owned) {
                                    const double d = ya - yb;
                                    sse += d * d;
                                }
                                if (SSIM) xs[wv][0][j] = ya, xs[wv][1][j] = yb;
                            } else {
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    const double d = (double)ra[c] - (double)rb[c];
                                    sse += d * d;
                                }
                            }
                        }
                        if (SSIM && !YMODE) {
                            xs[wv][0][j] = level1<false, QUANT>(qa, p, lu);
                            xs[wv][1][j] = level1<false, QUANT>(qb, p, lu);
                        }
                    }
                }
            }
            if (SSIM) {
                __syncthreads();
                if (row_on && lane < ncols_out) row_pass(win, &xs[wv][0][lane], &xs[wv][1][lane], ring[ri % RING], lane);
                __syncthreads();
                const int q = t * NW + wv - (K - 1);
                if (q >= 0 && q < nrows_out && lane < ncols_out) {
                    const Terms m = column_pass(win, ring, q, lane);
                    ssim += (m.num_l * m.num_cs) / (m.den_l * m.den_cs);
                }
            }
        }
        __syncthreads();   // a pass is over: the ring and the staging rows are free for the next plane
    }
    vsr::sums::workgroup_pair<NW * 64>(red, tid, sse, ssim, ws);
}

__global__ void __launch_bounds__(FT)
k_finish(const double* __restrict__ ws, double* __restrict__ sums, unsigned nwg, int what, double n_sse, double n_ssim) {
    __shared__ double red[2][FT];
    const int tid = threadIdx.x;
    vsr::sums::finish_pair<FT>(ws + (size_t)blockIdx.x * nwg * 2, 0, nwg, red, tid);
    if (tid == 0) {
        double* out = sums + (size_t)blockIdx.x * 4;
        out[0] = (what & VSR_METRIC_SSE) ? red[0][0] : 0.0;
        out[1] = (what & VSR_METRIC_SSE) ? n_sse : 0.0;
        out[2] = (what & VSR_METRIC_SSIM) ? red[1][0] : 0.0;
        out[3] = (what & VSR_METRIC_SSIM) ? n_ssim : 0.0;
    }
}

struct Geometry {
    unsigned strips, segs;
    int mh, mw;   // the map (the shaved plane itself without SSIM)
};

// the checks vsr_metric_ws_bytes and vsr_metric_frames share; `g` only when the result is VSR_OK
int check_shape(int F, int H, int W, int shave, int what, Geometry* g) {
    VSR_REQUIRE(what >= 1 && what <= 3, "metric_frames: unknown what %d (bit 0 SSE, bit 1 SSIM)", what);
    VSR_REQUIRE(F > 0 && H > 0 && W > 0, "metric_frames: bad shape (F %d, H %d, W %d)", F, H, W);
    VSR_REQUIRE(shave >= 0 && 2 * (long long)shave < (H < W ? H : W), "metric_frames: bad shave %d for %d x %d", shave, H, W);
    const int m = (H < W ? H : W) - 2 * shave;
    VSR_REQUIRE(!(what & VSR_METRIC_SSIM) || m >= K, "metric_frames: SSIM needs 11 pixels each way after the shave, got %d", m);
    VSR_REQUIRE(F <= 65535 && H <= 65535 && W <= 65535, "metric_frames: grid overflow (F %d, H %d, W %d beyond 65535)", F, H, W);
    const int halo = (what & VSR_METRIC_SSIM) ? K - 1 : 0;
    g->mh = H - 2 * shave - halo;
    g->mw = W - 2 * shave - halo;
    g->strips = vsr::cdiv(g->mw, SW);
    g->segs = vsr::cdiv(g->mh, SR);
    return VSR_OK;
}

}  // namespace

extern "C" {

int vsr_metric_abi_version(void) { return VSR_METRIC_ABI_VERSION; }
const char* vsr_metric_last_error(void) { return vsr::err_buf(); }

size_t vsr_metric_ws_bytes(int F, int H, int W, int shave, int what) {
    Geometry g;
    if (check_shape(F, H, W, shave, what, &g) != VSR_OK) return 0;
    return (size_t)F * g.strips * g.segs * 2 * sizeof(double);
}

int vsr_metric_frames(const float* a, const float* b, int F, int H, int W, int what, int channels, int quantise, int shave,
                      const float* luma4, const double* win11, double* sums, void* ws, vsr_stream_t stream) {
    const char* who = "metric_frames";
    Geometry g;
    bool wide;
    if (int rc = check_pointers(who, a, b, sums, ws)) return rc;
    if (int rc = check_shape(F, H, W, shave, what, &g)) return rc;
    VSR_REQUIRE(channels == VSR_METRIC_RGB || channels == VSR_METRIC_Y, "metric_frames: unknown channels %d", channels);
    if (int rc = check_quantise(who, quantise)) return rc;
    const bool ssim = (what & VSR_METRIC_SSIM) != 0, ymode = channels == VSR_METRIC_Y;
    VSR_REQUIRE(!ssim || win11, "metric_frames: null win11 with SSIM asked for");
    if (int rc = check_frames(who, ymode, luma4, a, b, W, sums, ws, &wide)) return rc;
    const Win win = ssim ? win_of(win11) : Win{};
    const Luma lu = ymode ? vsr::sums::luma_of(luma4) : Luma{};
    const int planes = ymode ? 1 : 3;
    const double hw = (double)(H - 2 * shave) * (double)(W - 2 * shave);
    const double n_sse = planes * hw, n_ssim = ssim ? planes * ((double)g.mh * (double)g.mw) : 0.0;
    const dim3 grid(g.strips, g.segs, F);
    hipStream_t s = vsr::S(stream);
    const int want_sse = what & VSR_METRIC_SSE;
    double* wsd = static_cast<double*>(ws);
    dispatch(ssim, ymode, [&](auto S_, auto Y_) {
        dispatch(quantise != 0, wide, [&](auto Q_, auto W_) {
            hipLaunchKernelGGL((k_metric<decltype(S_)::value, decltype(Y_)::value, decltype(Q_)::value, decltype(W_)::value>), grid,
                               dim3(NW * 64), 0, s, a, b, H, W, shave, want_sse, lu, win, wsd);
        });
    });
    const int rc = vsr::launched("metric_frames/tiles");
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(F), dim3(FT), 0, s, (const double*)wsd, sums, g.strips * g.segs, what, n_sse, n_ssim);
    return vsr::launched("metric_frames/finish");
}

}  // extern "C"
