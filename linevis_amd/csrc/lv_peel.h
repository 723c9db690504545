// Depth peeling (rendering mode 9, DepthPeelingRenderer.cpp:271-332 with DepthPeelingGather.glsl) and depth complexity (rendering mode
// 5, DepthComplexityRenderer.cpp with DepthComplexityResolve.glsl:48-57) under the numerics contract of DESIGN.md 4 (float32, one
// operation at a time, left to right, no contraction): every rule of the two modes, stated once.
// tests/test_depth_peeling_restatement.py states the same on the CPU, bit for bit.
//
// The peel key.  A pixel's layer of pass i is the fragment that survives the gather's discard (z <= previous layer's depth, i != 0) and
// the pipeline's depth test (cleared to 1.0, LESS): the smallest z above the previous layer's and below 1.0, the first in primitive
// order among equal depths.  Here that is ONE 64-bit atomicMin per fragment on (bits(z) << 32) | primitive key.  The bit patterns
// order as the floats do because z >= 0 for every kept fragment: lv_prism_accept admits only nearDist <= -vz <= farDist, and the
// window depth clip.z / clip.w of a perspective or orthographic projection with those planes maps that interval onto [0, 1] (+-
// rounding; a z that rounds below +0 would be -0 or negative: lv_peel_candidate refuses the sign bit, so such a fragment is never
// peeled, as a fragment in front of the near plane is not).  An empty slot is bits(1.0) << 32: z >= 1.0 can never win it.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"

#define LV_PEEL_MAX_LAYERS 2000u                       // DepthPeelingRenderer.cpp:288: min(maxDepthComplexity, 2000) passes
#define LV_PEEL_Z_ONE 0x3F800000u                      // bits(1.0f): the depth buffer's clear value
#define LV_PEEL_SLOT_EMPTY (0x3F800000ull << 32)       // nothing peeled in this pass
#define LV_PEEL_DONE 0xFFFFFFFEu                       // requested-pixel word of a pixel whose last pass peeled nothing (LV_PEEL_MASK_DONE)
#define LV_DC_MAX_COLOUR_CAP 512u                      // DepthComplexityResolve.glsl:52: min(numFragmentsMaxColor, 512)
// Measured knobs (tools/probe_depth_peeling.py, profiles/depth_peeling_c4.json), config-4 scene, mode-9 frame, three
// processes each, interleaved: both off 93.17 ... 93.32 ms; LV_PEEL_MASK_DONE 40.14 ... 41.46 ms -> on; LV_PEEL_PRELOAD 93.26 ... 93.41
// ms (and 40.41 ... 40.83 ms on top of LV_PEEL_MASK_DONE): no gain over the spread -> off.
#ifndef LV_PEEL_MASK_DONE
#define LV_PEEL_MASK_DONE 1     // 1: a finished pixel leaves the requested-pixel mask, later passes drop it in stage A
#endif
#ifndef LV_PEEL_PRELOAD
#define LV_PEEL_PRELOAD 0       // 1: a relaxed load of the slot first; the atomic is skipped when the key is not below it
#endif

// the per-pixel words of a mode-9 frame, addressed like ppllCount
struct LvPeelBuffers {
    unsigned long long* slot;   // this pass' smallest (z bits << 32) | key
    uint32_t* prevZ;            // z bits of the layer peeled last
    float4* accum;              // the FRONT_TO_BACK_PREMUL_ALPHA accumulator
    uint32_t* layers;           // layers peeled so far
};

// the device words of k_dc_reduce (lv_depth_complexity_get_stats)
struct LvDcStats {
    unsigned long long total;   // fragments of the requested pixels
    uint32_t used;              // requested pixels with at least one fragment
    uint32_t maxCount, minCount;
    uint32_t pad;
};

__device__ __forceinline__ unsigned long long lv_peel_key(uint32_t zbits, uint32_t primKey) {
    return ((unsigned long long)zbits << 32) | primKey;
}
// may a kept fragment with window depth bits zbits become this pass' layer: 0 <= z < 1.0 and, after the first pass, z > the last layer's
__device__ __forceinline__ bool lv_peel_candidate(uint32_t zbits, uint32_t prevZ, bool first) {
    return zbits < LV_PEEL_Z_ONE && (first || zbits > prevZ);
}
// the fragment's store
__device__ __forceinline__ void lv_peel_offer(unsigned long long* slot, unsigned long long key) {
#if LV_PEEL_PRELOAD
    // slots only decrease within a pass: a stale value can only skip less
    if (key >= __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
#endif
    atomicMin(slot, key);
}
// FRONT_TO_BACK_PREMUL_ALPHA of the layer's straight colour c into the accumulator A: all four channels with the old A.a
__device__ __forceinline__ float4 lv_peel_accumulate(float4 A, const f4& c) {
    const float t = 1.0f - A.w;
    float4 r;
    r.x = A.x + (c.x * c.w) * t;
    r.y = A.y + (c.y * c.w) * t;
    r.z = A.z + (c.z * c.w) * t;
    r.w = A.w + c.w * t;
    return r;
}
// BACK_TO_FRONT_PREMUL_ALPHA of the accumulator over the clear colour, all four channels
__device__ __forceinline__ uint32_t lv_peel_blit_pixel(const LvUniforms& U, float4 A) {
    const float t = 1.0f - A.w;
    f4 r;
    r.x = A.x + U.background[0] * t;
    r.y = A.y + U.background[1] * t;
    r.z = A.z + U.background[2] * t;
    r.w = A.w + U.background[3] * t;
    return lv_pack_unorm4x8(r);
}

// numFragmentsMaxColor of DepthComplexityRenderer.cpp:332 (intensity 1.5) from the frame's maximum, or the option's explicit value
__device__ __forceinline__ uint32_t lv_dc_max_colour(uint32_t maxComplexity, uint32_t explicitMaxColour) {
    if (explicitMaxColour != 0u) return explicitMaxColour;
    return uint32_t(float(max(maxComplexity, 4u)) / 1.5f);
}
// DepthComplexityResolve.glsl:48-57 with renderColor = (0, 1, 1, 1), then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour
__device__ __forceinline__ uint32_t lv_dc_resolve_pixel(const LvUniforms& U, uint32_t n, uint32_t maxColour) {
    const float percentage = clampf(float(n) / float(min(maxColour, LV_DC_MAX_COLOUR_CAP)), 0.0f, 1.0f) * 1.0f;
    f4 r;
    r.x = 0.0f * percentage + U.background[0] * (1.0f - percentage);
    r.y = 1.0f * percentage + U.background[1] * (1.0f - percentage);
    r.z = 1.0f * percentage + U.background[2] * (1.0f - percentage);
    r.w = percentage + U.background[3] * (1.0f - percentage);
    return lv_pack_unorm4x8(r);
}

// lv_peel.hip: one launch of k_peel_layer<shade, fast> over the viewport (grid = its 8 x 8-pixel waves, four to a workgroup)
void lv_peel_launch_layer(hipStream_t st, uint32_t grid, int shade, int fast, const LvUniforms& U, const LvSceneDev& S, uint32_t* startOffset,
                          const LvPeelBuffers& B);
