// Weighted Blended OIT (rendering mode 8): the gather of WBOITGather.glsl:21-27 and the resolve of WBOITResolve.glsl:38-48 under the
// numerics contract of DESIGN.md 4 (float32, one operation at a time, left to right, no contraction).  What the reference adds and
// multiplies in the blend unit in the racing invocations' order is here five 64-bit integer sums per pixel in the fixed point of
// lv_mboit.h -- SR, SG, SB, SA (the weighted premultiplied colour and alpha) and SL (the sum of -log(1 - alpha), whose exp is the
// reference's product of 1 - alpha: DESIGN.md 5 item 15) -- so that a frame does not depend on that order.
// tests/test_wboit_restatement.py states the same on the CPU, bit for bit.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_mboit.h"

#define LV_WBOIT_SUMS 5u                      // SR, SG, SB, SA, SL
#define LV_WBOIT_MAX_COUNT 131071u            // the sums stay exact: a term is at most 1024 * 2^36 = 2^46 (LV_MBOIT_STREAM_MAX_COUNT)
#define LV_WBOIT_WEIGHT_REFERENCE 0u          // wboit_depth_weight = reference: the line WBOITGather.glsl:23 runs (Vulkan's z in [0, 1])
#define LV_WBOIT_WEIGHT_OPENGL 1u             // wboit_depth_weight = opengl: the line the shader keeps as a comment

// WBOITGather.glsl:21-24.  z is the window depth in [0, 1]; under LV_WBOIT_WEIGHT_REFERENCE B is negative for every such z, the
// product is negative and the weight is the clamp's lower bound 0.01.  fmaxf drops a NaN: 0.01.
__device__ __forceinline__ float lv_wboit_weight(float alpha, float z, uint32_t weightMode) {
    const float A = fminf(1.0f, alpha) * 8.0f + 0.01f;
    const float B = weightMode == LV_WBOIT_WEIGHT_OPENGL ? ((-z) * 0.95f) + 1.0f : ((2.0f * z - 1.0f) * 0.95f) - 1.0f;
    const float raw = (((((A * A) * A) * 1e8f) * B) * B) * B;
    return fminf(fmaxf(raw, 0.01f), 300.0f);
}

// the revealage term of a fragment: -log(1 - alpha), saturated where the reference's product becomes 0, 0 where it stays
__device__ __forceinline__ long long lv_wboit_revealage_term(float alpha) {
    const float t = 1.0f - alpha;
    if (t <= 0.0f) return lv_mboit_fixed(LV_MBOIT_FIXED_LIMIT);
    if (!(t < 1.0f)) return 0;   // t >= 1 or NaN
    return lv_mboit_fixed(-lv_log_det(t));
}

// the five terms of a kept fragment with the straight colour `color` at window depth z: the ONE statement of them
__device__ __forceinline__ void lv_wboit_terms(const f4& color, float z, uint32_t weightMode, long long t[LV_WBOIT_SUMS]) {
    const float w = lv_wboit_weight(color.w, z, weightMode);
    t[0] = lv_mboit_fixed((color.x * color.w) * w);
    t[1] = lv_mboit_fixed((color.y * color.w) * w);
    t[2] = lv_mboit_fixed((color.z * color.w) * w);
    t[3] = lv_mboit_fixed(color.w * w);
    t[4] = lv_wboit_revealage_term(color.w);
}

// the fragment's store: up to five 64-bit adds with unused results (integer adds: any order gives the same sums)
__device__ __forceinline__ void lv_wboit_add(unsigned long long* sums, const f4& color, float z, uint32_t weightMode) {
    long long t[LV_WBOIT_SUMS];
    lv_wboit_terms(color, z, weightMode, t);
#pragma unroll
    for (uint32_t k = 0u; k < LV_WBOIT_SUMS; k++)
        if (t[k] != 0) atomicAdd(sums + k, (unsigned long long)t[k]);
}

// WBOITResolve.glsl:38-48, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour.  (The shader's isinf branch cannot be reached:
// the terms saturate, so no sum is infinite.)
__device__ __forceinline__ uint32_t lv_wboit_resolve_pixel(const LvUniforms& U, const unsigned long long* sums, uint32_t count) {
    f4 r;
    r.x = U.background[0]; r.y = U.background[1]; r.z = U.background[2]; r.w = U.background[3];
    if (count != 0u) {
        const float R = lv_exp_det(-lv_mboit_unfixed((long long)sums[4]));
        if (!(R > 0.9999f)) {
            const float den = fmaxf(lv_mboit_unfixed((long long)sums[3]), 1e-5f);
            const float a = 1.0f - R;
            r.x = (lv_mboit_unfixed((long long)sums[0]) / den) * a + U.background[0] * (1.0f - a);
            r.y = (lv_mboit_unfixed((long long)sums[1]) / den) * a + U.background[1] * (1.0f - a);
            r.z = (lv_mboit_unfixed((long long)sums[2]) / den) * a + U.background[2] * (1.0f - a);
            r.w = a + U.background[3] * (1.0f - a);
        }
    }
    return lv_pack_unorm4x8(r);
}
