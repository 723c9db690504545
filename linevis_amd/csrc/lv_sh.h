// lv_sh.h -- the spatial-hashing denoiser of the RTAO pass (ambient_occlusion_denoiser = "Spatial Hashing"): the definitions the
// kernels of lv_sh.hip share, and the one place its semantics are written down.
//
// Reference: SpatialHashingDenoiser.{hpp,cpp}, Data/Shaders/Denoiser/SH_Denoise.glsl.  The AO of every RTAO iteration is accumulated in
// WORLD space, in a hash map of cells keyed by (cell size, floor(position / cell size), trunc(normal * s_nd)) at four cell sizes per
// hit; a read pass averages the cells a hit falls into, coarser ones only while fewer than 60 samples are together; three a-trous
// passes smooth the result.  The reference's write pass claims slots without atomics, read-modify-writes a replacement counter from
// every invocation and evicts on racing values: its map depends on scheduling.  This build states the same algorithm so that it does
// not ("build-owned" below = decided here, not by the reference).
//
// INPUTS of one denoise: the hits of the iteration -- world position, world normal, pixel -- and the iteration's own (not accumulated)
// AO image.  In a frame they are the compacted primary hits of the RTAO pass (g0.xyz, g2.xyz, g1.w of the G-buffer, lv_tile.h); one
// lane per hit in both passes.  A record whose normal is (0, 0, 0) is a miss (glsl:261) and is skipped.
//
// CELL SIZE (s_wd_calc, glsl:200-206), in float32, every operation rounded once:
//   dis      = sqrtf(((dx * dx + dy * dy) + dz * dz)), d = position - cam                     (len3, lv_device.h)
//   s_w      = dis * tanSp,  tanSp = tanf(s_p / float(height)) computed once on the host
//   quot     = s_w / s_min,  s_min = powf(10.0f, float(s_min_exp)) computed on the host
//   log_step = floor(log2(quot)) := the biased exponent field of quot's bits - 127 (build-owned: exact where log2 of a value next to a
//              power of two would round across it); a quot that is not a positive normal float (0, denormal, negative, inf, NaN) makes
//              the hit skipped, like a miss
//   s_wd     = ldexpf(s_min, log_step);  level l = 0 .. 3 uses s_wd * 2^l
//
// KEYS (glsl:58-65,122-176), literal: s = max(s_wd_l, s_min); c = floorf(position / s) per component (IEEE division); n =
// ivec3(normalize(normal) * s_nd) truncating toward zero, normalize = the shading code's (norm3s, lv_device.h: a * r(a . a) with r(x) the
// correctly rounded 1 / sqrt(min(max(x, 2^-60), 2^60))); "s_nd = 0" HACK: the hashed words are the bits of
// 0.0f + float(n_i); all sums wrap in uint32
//   H4D  = wang(bits(s) + wang(bits(c.z) + wang(bits(c.y) + wang(bits(c.x)))))
//   hash = wang(bits(n.z) + wang(bits(n.y) + wang(bits(n.x) + H4D)))
//   H4Dc = wang(bits(c.x) + wang(bits(c.y) + wang(bits(c.z) + wang(bits(s)))))
//   chk  = wang(bits(n.x) + wang(bits(n.y) + wang(bits(n.z) + H4Dc)))
//   slot i of the probe window = uint32(hash + i) % numCells, i = 0 .. 9 (LINEAR_SEARCH_LENGTH)
//
// CELL (16 B, build-owned): a 64-bit key word (chk << 32) | hash and a 64-bit accumulator (sum << 28) | count.  The hash takes the
// place of the reference's replacement counter: a match is on the PAIR, so two keys never merge because they share a checksum.  The
// EMPTY sentinel is the key word 0 (a cleared map is all zero bytes, the reference's fill(0)); the one key whose word would be 0 (chk =
// hash = 0) is stored as the word 1 << 32 and probes from slot 0 like before.
//   contribution: q = uint(floorf(occlusion * 100.0f + 0.5f)), occlusion clamped to [0, 1] first (NaN -> 0): the reference's "Uint
//                 Quantized Atomic Add" mode with round() pinned.  ONE 64-bit atomicAdd of (q << 28) | 1 (integer sums: any order)
//   claim:        64-bit atomicCAS(key word, EMPTY -> key).  A lane walks its window; at each slot it learns the slot's final key (its
//                 own on a won claim, the winner's on a lost one, the stored one otherwise -- a key word never changes once set) and
//                 takes the first slot that holds its key.  Two lanes with one key therefore agree on the slot.
//   NO EVICTION:  a contribution whose window holds ten other keys is dropped and counted.  While dropped == 0 the map as a set of
//                 (key, sum, count) and everything read from it are independent of the execution order.
//
// CLEARS: at the start of a denoise when occupied > numCells / 2 (decided on the device, k_sh_begin); forced by the host when the
// pixels written since the last host-known clear plus this image's would reach 2^28 (no count or sum can wrap: count < 2^28, sum <=
// 100 * count < 2^36), after lv_set_lines / lv_set_trajectories / a changed line_width or spatial_hashing_s_p / _s_min_exp / _s_nd, and by
// lv_spatial_hashing_reset; a changed spatial_hashing_num_cells allocates a new (empty) map.  Camera and viewport do not clear it.
//
// READ (glsl:365-440): levels in order; in a level the first slot of the window that holds the key (the walk may stop at an EMPTY slot:
// without eviction the key cannot lie behind one); ao += float(sum) / 100.0f, samples += count; stop after the level at which samples
// >= 60; result = samples > 0 ? ao / float(samples) : 0.  Misses and skipped hits read 0.  show_grid_cells is not built.
//
// TAIL (SpatialHashingDenoiser.cpp:82-87): three passes of EAWDenoise.Compute (k_eaw_pass<true>) on the read image with the WORLD-space
// normal and position maps, useColorWeights = false, phiPosition = 0.3 * 1e-6, phiNormal = 0.1, step widths 1, 2, 4 -- fixed, not the
// eaw_denoiser_* options.  The maps hold {x, y, z, 0}, 0 on a miss: the fourth components are equal everywhere as they are in the
// reference's maps ({.., 0} and {.., 1}), so they never enter a distance.
#ifndef LV_SH_H
#define LV_SH_H

#include "lv_device.h"

#define LV_SH_PROBES 10u        // LINEAR_SEARCH_LENGTH
#define LV_SH_LEVELS 4
#define LV_SH_MIN_SAMPLES 60u   // min_nr_samples, glsl:386
#define LV_SH_COUNT_BITS 28
#define LV_SH_COUNT_MASK 0x0FFFFFFFull

struct LvShCell { unsigned long long key, acc; };

// clears: since the last reset; stored, dropped, occupied: since the last clear; ticket: k_sh_begin's count of finished workgroups
struct LvShCounters {
    unsigned long long stored, dropped;
    uint32_t occupied, clears, ticket, pad;
};

struct LvShParams {
    float cam[3];
    float tanSp, sMin, sNd;
    uint32_t numCells;
};

namespace {

__device__ __forceinline__ uint32_t lv_sh_wang(uint32_t seed) {
    seed = (seed ^ 61u) ^ (seed >> 16);
    seed *= 9u;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2du;
    seed = seed ^ (seed >> 15);
    return seed;
}

// s_wd of a hit; false: the hit is skipped
__device__ __forceinline__ bool lv_sh_cell_size(const LvShParams& P, f3 position, float& swd) {
    const float dis = len3(position - mk3(P.cam[0], P.cam[1], P.cam[2]));
    const float sw = dis * P.tanSp;
    const float quot = sw / P.sMin;
    const uint32_t e = __float_as_uint(quot) >> 23;   // sign and exponent: 1 .. 254 = a positive normal float
    swd = 0.0f;
    if (e == 0u || e >= 255u) return false;
    swd = ldexpf(P.sMin, int(e) - 127);
    return true;
}

// trunc(normalize(normal) * s_nd) as the three hashed words
struct LvShNormal { uint32_t x, y, z; };
__device__ __forceinline__ LvShNormal lv_sh_normal(const LvShParams& P, f3 normal) {
    const f3 n = norm3s(normal) * P.sNd;
    LvShNormal r;
    r.x = __float_as_uint(0.0f + float(int(n.x)));
    r.y = __float_as_uint(0.0f + float(int(n.y)));
    r.z = __float_as_uint(0.0f + float(int(n.z)));
    return r;
}

// key word of (position, normal) at cell size swdLevel; hash = its low word
__device__ __forceinline__ unsigned long long lv_sh_key(const LvShParams& P, f3 position, const LvShNormal& n, float swdLevel) {
    const float s = fmaxf(swdLevel, P.sMin);
    const uint32_t bs = __float_as_uint(s);
    const uint32_t cx = __float_as_uint(floorf(position.x / s)), cy = __float_as_uint(floorf(position.y / s)),
                   cz = __float_as_uint(floorf(position.z / s));
    const uint32_t h4 = lv_sh_wang(bs + lv_sh_wang(cz + lv_sh_wang(cy + lv_sh_wang(cx))));
    const uint32_t hash = lv_sh_wang(n.z + lv_sh_wang(n.y + lv_sh_wang(n.x + h4)));
    const uint32_t c4 = lv_sh_wang(cx + lv_sh_wang(cy + lv_sh_wang(cz + lv_sh_wang(bs))));
    const uint32_t chk = lv_sh_wang(n.x + lv_sh_wang(n.y + lv_sh_wang(n.z + c4)));
    const unsigned long long key = ((unsigned long long)chk << 32) | hash;
    return key ? key : 1ull << 32;
}

__device__ __forceinline__ uint32_t lv_sh_slot(unsigned long long key, uint32_t i, uint32_t numCells) {
    return (uint32_t(key) + i) % numCells;
}

} // namespace

#endif
