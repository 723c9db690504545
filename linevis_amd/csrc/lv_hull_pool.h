// The simulation-mesh hull in the pooled modes 2 (per-pixel linked lists) and 3 (MLAB), hull_fragment_pool = on: the semantics, stated
// once.  tests/test_hull_pool_restatement.py states the same on the CPU.
//
// The reference draws the hull inside the gather of its pooled renderers (PerPixelLinkedListLineRenderer.cpp:448-461, after the
// lines): a hull fragment goes through gatherFragment like a line fragment, shares the node pool and is sorted / folded with the
// lines.  Coverage, the depth rule 0 <= z < 1, the interpolated position and normal and the colour are lv_hull.h's, unchanged; the
// mode's gather then gives the entry:
//   mode 2 (LinkedListGather.glsl:34-60)  alpha < 0.001: discarded.  Kept: the 8-byte entry {lv_pack_unorm4x8(straight colour),
//          bits(depth)}, depth = length(fragmentPositionWorld - cameraPosition) -- len3(pos - camera), the expression lv_shade_prism
//          hands lv_prism_accept for a line fragment's node depth.  Discarded: the DEAD entry {0, LV_PPLL_DEAD}, 0x10000 added to the
//          pixel's count word, counted in prismDiscards -- as for a line fragment.
//   mode 3 (MLABGather.glsl:63-91)        the same discard.  Kept: {packUnorm4x8(rgb * a, 1 - a), bits(z), key} with z the window depth
//          the hull fragment already has and key = (numSegs << 6) + triangle: the reference draws the hull after the lines and its
//          ordered interlock folds in primitive order, so every hull fragment of a pixel folds after every line fragment (line keys
//          are < numSegs << 6), in triangle order.  Discarded: {0, LV_PPLL_DEAD, LV_MLAB_NO_KEY}.  A frame whose keys would reach
//          LV_MLAB_NO_KEY or wrap -- (numSegs << 6) + numHullTriangles > 0xFFFFFFFE -- is refused (lv_hull_pool_keys_fit).
//   both   a stored hull fragment adds 1 to the pixel's 16-bit count under the rasteriser's saturation rule (lv_hull_record, below), a
//          kept one adds 1 to the frame's fragCounter; a pixel outside the requested mask of a tile list stores nothing, so a pixel is
//          stored once however often tiles repeat.  The hull's slots are taken before the lines' (below), so where mode 2's pool runs
//          full the lines are dropped first; the reference draws the hull last and would drop the hull first.  Everything behind
//          the fragment stage -- the scan, the selection of the nearest, the resolves, lv_ppll_get_buffers -- is the lines' code and
//          sees a hull entry as any other.
//
// The device path (lv_hull.hip), two launches in the LV_KERNEL_HULL slot:
//   k_hull_pass<LV_HULL_STORE_RECORD>  in the front end, after the requested pixels are marked and BEFORE the line rasteriser: per kept
//          fragment a slot of the shared record pool from dc->fragAlloc -- wave-aggregated chunks of LV_HULL_CHUNK slots, one global
//          atomic per chunk, so mode 2's drop rule, mode 3's read-back of the need, the regrowth and LV_E_CAPACITY cover the hull
//          with the lines' host logic -- and a rank from the pixel's count.  The record is {y * width + x + 1, LV_PPLL_DEAD,
//          triangle}: word 1 is what the lines' fragment stage skips a slot by (its instructions stay as they are), word 0 is
//          non-zero, which tells a hull record from every chunk tail and dead record {0, LV_PPLL_DEAD, stale}.
//   k_hull_shade_records<ENTRY>        next to the lines' fragment stage: one lane per hull record, the fragment again from the
//          triangle and the pixel (lv_hull_setup, lv_vis_cover, lv_hull_fragment<true>), the entry above at run start + rank.
// Ranks: running first, the hull holds ranks [0, h) of a pixel's run.  The 12-byte record has no room for the rank beside the pixel,
// the dead mark and the triangle, so the fragment stage hands the h ranks out again from a per-pixel counter of its own (4 bytes per
// padded pixel, zeroed per frame, addressed like the counts).  Which hull fragment takes which of the h entries never shows: both
// resolves order by key.  No host synchronisation, no memory that grows with the fragments beyond the pool.
// Restrictions (refused at render time while a hull is drawn): the hull store fills the segment rasteriser's record pool only --
// ppll_prism_rasteriser = lbvh, ppll_fragment_source = capsule_entry and line quads have none.  Pooled mode 6 draws no hull, as the
// reference.  Not built: mode 1, the hull under use_mlat.
#pragma once
#include "lv_hull.h"

#define LV_HULL_STORE_RECORD 4   // modes 2 and 3: a record of the shared pool
#ifndef LV_HULL_SHADE_BLOCKS_PER_CU
#define LV_HULL_SHADE_BLOCKS_PER_CU 8u   // workgroups of k_hull_shade_records per CU (grid-stride over the record pool)
#endif
#ifndef LV_HULL_CHUNK
#define LV_HULL_CHUNK 128u       // record slots a wave of the hull launch reserves per global atomic (>= LV_WAVE: a batch is <= 64)
#endif

inline bool lv_hull_pool_keys_fit(uint64_t numSegs, uint64_t numTris) {
    return numSegs <= (0xFFFFFFFEull >> 6) && (numSegs << 6) + numTris <= 0xFFFFFFFEull;
}

// the wave's chunk of record slots {next slot, slots left}: a workgroup of k_hull_pass is ONE wave.  Read and written with relaxed
// atomics: the leader of a batch is whichever lane comes first among those that hold a fragment, so a lane reads what ANOTHER lane
// wrote a batch earlier -- with plain accesses the compiler, which sees one thread, keeps the pair in registers across the pixel loop
// (it hoisted the load out of the loop, and batches led by different lanes handed out the same slots)
__device__ __forceinline__ uint32_t* lv_hull_chunk() {
    __shared__ uint32_t s_chunk[2];
    return s_chunk;
}
__device__ __forceinline__ uint32_t lv_hull_chunk_get(int i) {
    return __hip_atomic_load(lv_hull_chunk() + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lv_hull_chunk_set(int i, uint32_t v) {
    __hip_atomic_store(lv_hull_chunk() + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The RECORD store of one kept fragment, called by whichever lanes of the wave hold one (the chunk logic of k_ppll_raster_prism's
// coverage stage on the active lanes, the leader keeping the chunk as k_ppll_gather does).  records / poolSlots: the record pool.
// The rank is a full-word atomicAdd on the pixel's count, undone at rk >= 0xFFFF with a dead record: the high half -- the discard count
// -- is still 0 while the rasterisers run, so once the count saturates every later lane fails and undoes its add (testing the low
// half only let lanes behind the one that hit 0xFFFF wrap around to ranks 0, 1, ... a second time).
// false: no record -- the fragment stage never sees the fragment, but the reference's fragCounter counts it.
// Any grouping of the lanes into batches is valid -- one batch of every lane that holds a fragment, or several smaller ones, however
// the compiler lays out the divergent pixel loops --: a batch only has to finish its read-modify-write of the chunk pair before the
// next one starts, which one wave issuing its LDS operations in order guarantees, and the slots of two batches never overlap.
__device__ __forceinline__ bool lv_hull_record(uint32_t* __restrict__ records, uint32_t poolSlots, uint32_t* __restrict__ fragCount,
                                               uint32_t addr, uint32_t pixel, uint32_t tri, LvDevCounters* dc) {
    const unsigned long long mask = __ballot(1);
    const uint32_t lane = threadIdx.x;
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0u, left = 0u, base2 = 0u;
    if (int(lane) == leader) {
        const uint32_t n = uint32_t(__popcll(mask));
        base = lv_hull_chunk_get(0); left = lv_hull_chunk_get(1);
        if (left < n) {
            base2 = atomicAdd(&dc->fragAlloc, (unsigned)LV_HULL_CHUNK);
            lv_hull_chunk_set(0, base2 + (n - left));
            lv_hull_chunk_set(1, LV_HULL_CHUNK - (n - left));
        } else {
            lv_hull_chunk_set(0, base + n);
            lv_hull_chunk_set(1, left - n);
        }
    }
    base = uint32_t(__shfl(int(base), leader, 64)); left = uint32_t(__shfl(int(left), leader, 64));
    base2 = uint32_t(__shfl(int(base2), leader, 64));
    const uint32_t rankInBatch = uint32_t(__popcll(mask & ((1ull << lane) - 1ull)));
    const uint32_t insertIndex = rankInBatch < left ? base + rankInBatch : base2 + (rankInBatch - left);
    if (insertIndex >= poolSlots) return false;
    const uint32_t rk = atomicAdd(&fragCount[addr], 1u);
    if (rk < 0xFFFFu) {
        records[3 * size_t(insertIndex) + 0] = pixel + 1u;
        records[3 * size_t(insertIndex) + 1] = LV_PPLL_DEAD;
        records[3 * size_t(insertIndex) + 2] = tri;
        return true;
    }
    atomicSub(&fragCount[addr], 1u);   // (the per-pixel count shares its word with the count of discarded fragments: 16 bits each)
    records[3 * size_t(insertIndex) + 0] = 0u;
    records[3 * size_t(insertIndex) + 1] = LV_PPLL_DEAD;
    return false;
}

// the interpolated world position of the covered fragment: the two steps lv_hull_fragment takes to it, on the same operands
__device__ __forceinline__ f3 lv_hull_position(const LvVisTri& T, const float e[3]) {
    float b[3];
    lv_prism_weights(e, b);
    return lv_prism_mix3(b, T.V[0], T.V[1], T.V[2]);
}

// lv_hull.hip: the waves of ONE launch of k_hull_pass (each may leave the tail of a chunk unused), and the fragment stage of the hull
// records: ONE launch of k_hull_shade_records<entry> over the record pool.  frags: the fragment array (8-B entries, 12-B in mode 3);
// pixelOffset, blockBase: the runs (lv_run_start); ranks: the zeroed per-pixel counters; keyBase: numSegs << 6 (mode 3)
uint32_t lv_hull_launch_waves(uint32_t numCUs, uint32_t numTris, uint32_t height);
void lv_hull_shade_launch(hipStream_t st, int entry, uint32_t numCUs, const LvUniforms& U, const LvPrismDev& R, const LvHullDev& H,
                          const uint32_t* records, uint32_t* frags, const uint32_t* pixelOffset, const uint32_t* blockBase,
                          uint32_t* fragCount, uint32_t* ranks, LvDevCounters* dc, uint32_t poolSlots, uint32_t keyBase);
