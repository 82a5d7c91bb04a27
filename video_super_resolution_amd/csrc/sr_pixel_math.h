// sr_pixel_math.h -- per-pixel float helpers of the SR kernels, fp16 and fp32 paths alike (no layout, no vector type: sr_f32.hip,
// sr_f32_mfma.hip, sr_scale.hip and sr_train.hip include it without the fp16 stages' constants; sr_f16_common.h passes it on).
// An inline function compiles under the flags and pragmas of the file that includes it.
#pragma once
#include "vsr_common.h"

namespace {

__device__ __forceinline__ float prelu(float v, float a) { return v >= 0.0f ? v : v * a; }

// bilinear xS, align_corners=False, as ATen's upsample_bilinear2d: src = (dst+0.5)/S-0.5 clamped at 0,
// i1 = min(i0+1, n-1).  `inv` = 1/S as ATen forms it (0.25, 0.5 exact; 1/3 rounded once, like `1.0 / scale_factor`
// cast to float there).
__device__ __forceinline__ void bil(int dst, int n, float inv, int& i0, int& i1, float& l1) {
    float src = ((float)dst + 0.5f) * inv - 0.5f;
    if (src < 0.0f) src = 0.0f;
    i0 = (int)src;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

// the bilinear sample of four neighbours, every product-sum an explicit fma and nothing else fused: the decimated and the full-frame
// builds of the fusion kernels round identically
__device__ __forceinline__ float lerp4(float v00, float v01, float v10, float v11, float lx, float ly) {
#pragma clang fp contract(off)
    const float top = __builtin_fmaf(lx, v01, (1.0f - lx) * v00);
    const float bot = __builtin_fmaf(lx, v11, (1.0f - lx) * v10);
    return __builtin_fmaf(ly, bot, (1.0f - ly) * top);
}

}  // namespace
