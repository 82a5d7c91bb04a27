// sr_strip30.h -- the strip geometry shared by the x2 / x3 fused kernels (sr_utd_s2.hip, sr_utd_s2w.hip, sr_tail_s2.hip, sr_utd_s3.h,
// sr_tail_s3.hip): a workgroup marches down a strip of 30 LR columns at 32 deconv positions, with LR rows m-1, m, m+1 and the row being
// loaded in a 4-row LDS ring.  LDS totals, blob offsets and HR rings are each kernel's own, written through these.
#pragma once
#include "sr_f16_common.h"

namespace {

constexpr int S30_TX = 30;                     // LR output columns per strip (32 deconv positions = 2 MFMA pixel tiles)
constexpr int S30_LRC = 34;                    // staged LR columns x0-2 .. x0+31
constexpr int S30_LR_SLOT = S30_LRC * 64;
constexpr int S30_LR_BYTES = 4 * S30_LR_SLOT;  // rows m-1, m, m+1 + the row being loaded
constexpr int S30_PART_W = 32 * PART_PX_PITCH;   // one wave's fp32 partial tile of an output row
constexpr int S30_PART_BUF = 4 * S30_PART_W;
constexpr int S30_OROW = 2048;                 // POST: a finished output row as fp16 [32 px][64 B], 16-byte pieces swizzled (lr_off)

}  // namespace
