// frame_metric.hip -- HR frames scored against ground truth on the device (include/vsr_hip_metric.h; libvsr_hip_metric.so is built
// from this source alone): per frame the float64 sums behind PSNR and SSIM.
//
//   k_metric : one workgroup (4 waves) = one tile of SW = 64 map columns x SR = 64 map rows of one frame; with SSIM the tile reads
//              (SW + 10) x (SR + 10) pixels of the shaved plane, without it the map IS the plane and there is no halo.  The tile
//              marches down its rows four at a time: wave v takes input row 4 t + v.
//                load    : the row's 74 x 3 floats of a and b into LDS as they lie in memory (WIDE: one aligned 16-byte load per lane;
//                          otherwise four element loads per lane): a frame is read about once plus halo from HBM; the second and third
//                          plane of RGB read their rows again through the L2 of the same compute unit
//                convert : lane l takes pixels l and l + 64: quantise, luma (Y) or channel p (RGB, p the plane of this pass), both
//                          frames, to doubles in LDS; SSE is taken here, from the pixels the tile OWNS (the first SW x SR of its
//                          rectangle; the last strip / segment also owns its halo), in the first pass for all three channels
//                rows    : lane c = map column c: the five 11-tap sums along the row into an LDS ring of NW + 10 = 14 rows
//                columns : wave v takes map row 4 t + v - 10 (its eleven ring rows are complete): the five 11-tap sums down the
//                          column, the formula, the thread's running sum
//              three barriers per step.  RGB runs the march once per plane with one ring (36 KB; three rings would leave one workgroup
//              per compute unit).  At the end a fixed-order tree over the 256 threads and one pair of doubles into the workspace.
//   k_finish : one workgroup of 64 threads per frame: thread t adds the partials t, t + 64, ... in that order, then the same tree;
//              thread 0 writes the frame's four numbers (0 in the slots not asked for).
// Nothing here is atomic and no order depends on timing or on F: a frame's numbers are the same bits in every run.
//
// The whole file is compiled without floating-point contraction (Makefile and the pragma below): luma, the SSE terms and the SSIM
// formula round operation by operation as the header writes them; the window sums ask for their fmas by name.
#include "frame_sums.h"
#include "vsr_common.h"

#include "../../include/vsr_hip_metric.h"

#pragma clang fp contract(off)

namespace {

using vsr::sums::Luma;
using vsr::sums::quant;

constexpr int SW = VSR_METRIC_STRIP_WIDTH, SR = VSR_METRIC_SEGMENT_ROWS, FT = VSR_METRIC_FINISH_THREADS;
constexpr int NW = 4;              // waves per workgroup = input rows per step
constexpr int K = 11;              // window taps
constexpr int RING = NW + K - 1;   // ring rows: the 11 rows of the oldest map row of a step up to the newest input row
constexpr int RAW = 256;           // floats of one staged row: 74 x 3 = 222, + 3 before an aligned start, rounded up to 64 lanes x 4
constexpr int XS = 80;             // doubles of one converted row (74 used)

struct Win {
    double w[K];
};

template <bool SSIM, bool YMODE, bool QUANT, bool WIDE>
__global__ void __launch_bounds__(NW * 64)
k_metric(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int shave, int want_sse, Luma lu, Win win,
         double* __restrict__ ws) {
    constexpr int HALO = SSIM ? K - 1 : 0;
    constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
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
                if (WIDE) {
                    const size_t s4 = s & ~(size_t)3;        // H * W * 3 is a multiple of 4: an aligned group ends inside the frame
                    o = (int)(s - s4);
                    if (4 * lane < o + nfl) {
                        *reinterpret_cast<float4*>(&raw[wv][0][4 * lane]) = *reinterpret_cast<const float4*>(fa + s4 + 4 * lane);
                        *reinterpret_cast<float4*>(&raw[wv][1][4 * lane]) = *reinterpret_cast<const float4*>(fb + s4 + 4 * lane);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = lane + 64 * k;
                        if (i < nfl) {
                            raw[wv][0][i] = fa[s + i];
                            raw[wv][1][i] = fb[s + i];
                        }
                    }
                }
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
                            const float va = qa[p], vb = qb[p];
                            xs[wv][0][j] = (double)(QUANT ? quant(va) : va);
                            xs[wv][1][j] = (double)(QUANT ? quant(vb) : vb);
                        }
                    }
                }
            }
            if (SSIM) {
                __syncthreads();
                // ---- rows: five 11-tap sums into the ring
                if (row_on && lane < ncols_out) {
                    double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const double va = xs[wv][0][lane + k], vb = xs[wv][1][lane + k];
                        const double paa = va * va, pbb = vb * vb, pab = va * vb;
                        sa = __builtin_fma(win.w[k], va, sa);
                        sb = __builtin_fma(win.w[k], vb, sb);
                        saa = __builtin_fma(win.w[k], paa, saa);
                        sbb = __builtin_fma(win.w[k], pbb, sbb);
                        sab = __builtin_fma(win.w[k], pab, sab);
                    }
                    const int slot = ri % RING;
                    ring[slot][0][lane] = sa;
                    ring[slot][1][lane] = sb;
                    ring[slot][2][lane] = saa;
                    ring[slot][3][lane] = sbb;
                    ring[slot][4][lane] = sab;
                }
                __syncthreads();
                // ---- columns: map row q needs input rows q .. q + 10, all in the ring once row 4 t + 3 is
                const int q = t * NW + wv - (K - 1);
                if (q >= 0 && q < nrows_out && lane < ncols_out) {
                    double ma = 0.0, mb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
                    int slot = q % RING;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        ma = __builtin_fma(win.w[k], ring[slot][0][lane], ma);
                        mb = __builtin_fma(win.w[k], ring[slot][1][lane], mb);
                        eaa = __builtin_fma(win.w[k], ring[slot][2][lane], eaa);
                        ebb = __builtin_fma(win.w[k], ring[slot][3][lane], ebb);
                        eab = __builtin_fma(win.w[k], ring[slot][4][lane], eab);
                        slot = slot + 1 == RING ? 0 : slot + 1;
                    }
                    const double maa = ma * ma, mbb = mb * mb, mab = ma * mb;
                    const double s_aa = eaa - maa, s_bb = ebb - mbb, s_ab = eab - mab;
                    ssim += ((2.0 * mab + C1) * (2.0 * s_ab + C2)) / (((maa + mbb) + C1) * ((s_aa + s_bb) + C2));
                }
                // (the next step's ring stores come after its first two barriers: every read above has been issued by then)
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
    vsr::sums::finish_pair<FT>(ws, nwg, red, tid);
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

template <bool SSIM, bool YMODE>
void launch(bool quant, bool wide, dim3 grid, hipStream_t s, const float* a, const float* b, int H, int W, int shave, int want_sse,
            const Luma& lu, const Win& win, double* ws) {
    const dim3 block(NW * 64);
    if (quant && wide) hipLaunchKernelGGL((k_metric<SSIM, YMODE, true, true>), grid, block, 0, s, a, b, H, W, shave, want_sse, lu, win, ws);
    else if (quant) hipLaunchKernelGGL((k_metric<SSIM, YMODE, true, false>), grid, block, 0, s, a, b, H, W, shave, want_sse, lu, win, ws);
    else if (wide) hipLaunchKernelGGL((k_metric<SSIM, YMODE, false, true>), grid, block, 0, s, a, b, H, W, shave, want_sse, lu, win, ws);
    else hipLaunchKernelGGL((k_metric<SSIM, YMODE, false, false>), grid, block, 0, s, a, b, H, W, shave, want_sse, lu, win, ws);
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
    VSR_REQUIRE(a && b && sums && ws, "metric_frames: null pointer");
    Geometry g;
    const int rc0 = check_shape(F, H, W, shave, what, &g);
    if (rc0) return rc0;
    VSR_REQUIRE(channels == VSR_METRIC_RGB || channels == VSR_METRIC_Y, "metric_frames: unknown channels %d", channels);
    VSR_REQUIRE(quantise == 0 || quantise == 1, "metric_frames: quantise must be 0 or 1, got %d", quantise);
    const bool ssim = (what & VSR_METRIC_SSIM) != 0, ymode = channels == VSR_METRIC_Y;
    VSR_REQUIRE(!ssim || win11, "metric_frames: null win11 with SSIM asked for");
    VSR_REQUIRE(!ymode || luma4, "metric_frames: null luma4 in Y mode");
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    VSR_REQUIRE(((pa | pb) & 3) == 0, "metric_frames: the frames must be 4-byte aligned");
    VSR_REQUIRE(((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "metric_frames: sums and the workspace must be 8-byte aligned");
    Win win = {};
    if (ssim)
        for (int i = 0; i < K; ++i) win.w[i] = win11[i];
    const Luma lu = ymode ? vsr::sums::luma_of(luma4) : Luma{};
    // 16-byte loads: both bases aligned and a row pitch (so a frame) of a whole number of 16-byte groups
    const bool wide = ((pa | pb) & 15) == 0 && W % 4 == 0;
    const int planes = ymode ? 1 : 3;
    const double hw = (double)(H - 2 * shave) * (double)(W - 2 * shave);
    const double n_sse = planes * hw, n_ssim = ssim ? planes * ((double)g.mh * (double)g.mw) : 0.0;
    const dim3 grid(g.strips, g.segs, F);
    hipStream_t s = vsr::S(stream);
    const int want_sse = what & VSR_METRIC_SSE;
    double* wsd = static_cast<double*>(ws);
    if (ssim && ymode) launch<true, true>(quantise, wide, grid, s, a, b, H, W, shave, want_sse, lu, win, wsd);
    else if (ssim) launch<true, false>(quantise, wide, grid, s, a, b, H, W, shave, want_sse, lu, win, wsd);
    else if (ymode) launch<false, true>(quantise, wide, grid, s, a, b, H, W, shave, want_sse, lu, win, wsd);
    else launch<false, false>(quantise, wide, grid, s, a, b, H, W, shave, want_sse, lu, win, wsd);
    const int rc = vsr::launched("metric_frames/tiles");
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(F), dim3(FT), 0, s, (const double*)wsd, sums, g.strips * g.segs, what, n_sse, n_ssim);
    return vsr::launched("metric_frames/finish");
}

}  // extern "C"
