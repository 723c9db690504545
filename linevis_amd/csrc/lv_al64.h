// Atomic Loop 64 (rendering mode 10): the insert of AtomicLoop64Gather.glsl:70-79 and the blend of AtomicLoop64Resolve.glsl:69-87
// under the numerics contract of DESIGN.md 4, and the build-owned tail: what the reference blends into the framebuffer
// in the racing invocations' order is here five 64-bit integer sums per pixel, so that a frame does not depend on that order.
// Per pixel: K slots of 8 B {window depth bits << 32 | packUnorm4x8(colour)}, ascending, then the sums SA, SR, SG, SB, SL.
// tests/test_atomic_loop_restatement.py states the same on the CPU, bit for bit.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_mboit.h"

#define LV_AL64_EMPTY 0xFFFFFFFFFFFFFFFFull   // clear value of a slot (AtomicLoop64Resolve.glsl:80)
#define LV_AL64_TAIL 5u                       // SA, SR, SG, SB, SL
#ifndef LV_AL64_SHORTCUT
#define LV_AL64_SHORTCUT 1                    // lv_al64_insert loads slot[K - 1] first (0: without; measured)
#endif
#define LV_AL64_MAX_COUNT 131071u             // SL stays exact: a term is at most 1024 * 2^36 = 2^46 (LV_MBOIT_STREAM_MAX_COUNT)

// the absorbance term of a carried fragment with 8-bit alpha a8, in the fixed point of lv_mboit.h (256 values)
__device__ __forceinline__ long long lv_al64_term(uint32_t a8) {
    if (a8 == 0u) return 0;
    if (a8 == 255u) return lv_mboit_fixed(LV_MBOIT_FIXED_LIMIT);
    return lv_mboit_fixed(-lv_log_det(1.0f - float(a8) / 255.0f));
}

// a fragment no slot kept: its 8-bit channels into the pixel's five sums (integer adds: any order gives the same sums)
__device__ __forceinline__ void lv_al64_tail_add(unsigned long long* tail, unsigned long long key) {
    const uint32_t c = uint32_t(key);
    const uint32_t r8 = c & 0xFFu, g8 = (c >> 8) & 0xFFu, b8 = (c >> 16) & 0xFFu, a8 = c >> 24;
    if (a8 == 0u) return;   // every term is 0
    atomicAdd(tail + 0, (unsigned long long)a8);
    if (r8) atomicAdd(tail + 1, (unsigned long long)(a8 * r8));
    if (g8) atomicAdd(tail + 2, (unsigned long long)(a8 * g8));
    if (b8) atomicAdd(tail + 3, (unsigned long long)(a8 * b8));
    atomicAdd(tail + 4, (unsigned long long)lv_al64_term(a8));
}

// AtomicLoop64Gather.glsl:70-79.  Every exchange keeps the multiset slots + carried values, so the K slots end as the K smallest keys
// in ascending order whatever order the lanes arrive in; at most K atomics, no lock and no waiting on another lane.
__device__ __forceinline__ void lv_al64_insert(unsigned long long* slots, uint32_t K, unsigned long long key, unsigned long long* tailAcc) {
#if LV_AL64_SHORTCUT
    // the last slot first: slots only decrease, so a stale value is larger and the test can only fire less often; a key at or above
    // it has K keys at or below it in the slots already and belongs to the tail
    if (key >= __hip_atomic_load(slots + (K - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        lv_al64_tail_add(tailAcc, key);
        return;
    }
#endif
    unsigned long long v = key;
    for (uint32_t i = 0u; i < K; i++) {
        const unsigned long long old = atomicMin(slots + i, v);
        if (old == LV_AL64_EMPTY) return;
        if (old > v) v = old;
    }
    lv_al64_tail_add(tailAcc, v);
}

// AtomicLoop64Resolve.glsl:69-87 over the framebuffer under the layers: the clear colour, or the tail's weighted average blended
// over it (BACK_TO_FRONT_STRAIGHT_ALPHA); alphaOut = 0 gives that framebuffer (mode 3's rule for the reference's 0 / 0)
__device__ __forceinline__ uint32_t lv_al64_resolve_pixel(const LvUniforms& U, const unsigned long long* slots, uint32_t K,
                                                          const unsigned long long* tail) {
    float col[3] = {0.0f, 0.0f, 0.0f}, tr = 1.0f;
    for (uint32_t i = 0u; i < K; i++) {
        const unsigned long long v = slots[i];
        if (v == LV_AL64_EMPTY) break;
        const f4 src = lv_unpack_unorm4x8(uint32_t(v));
        const float wgt = tr * src.w;
        col[0] = col[0] + wgt * src.x;
        col[1] = col[1] + wgt * src.y;
        col[2] = col[2] + wgt * src.z;
        tr = tr * (1.0f - src.w);
    }
    float fb[4] = {U.background[0], U.background[1], U.background[2], U.background[3]};
    const unsigned long long sa = tail[0];
    if (sa != 0ull) {
        const float at = 1.0f - lv_exp_det(-lv_mboit_unfixed((long long)tail[4]));
        const float fsa = float(sa);
#pragma unroll
        for (int k = 0; k < 3; k++) fb[k] = ((float(tail[1 + k]) / fsa) / 255.0f) * at + U.background[k] * (1.0f - at);
        fb[3] = at + U.background[3] * (1.0f - at);
    }
    const float a = 1.0f - tr;
    f4 r;
    r.x = fb[0]; r.y = fb[1]; r.z = fb[2]; r.w = fb[3];
    if (a > 0.0f) {
        r.x = (col[0] / a) * a + fb[0] * (1.0f - a);
        r.y = (col[1] / a) * a + fb[1] * (1.0f - a);
        r.z = (col[2] / a) * a + fb[2] * (1.0f - a);
        r.w = a + fb[3] * (1.0f - a);
    }
    return lv_pack_unorm4x8(r);
}
