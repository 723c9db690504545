// lv_hull.hip -- the kernel of the simulation-mesh hull pass (lv_hull.h).  It lives here, not in lv_render.hip, for the reason
// lv_deferred.hip does: the kernels of lv_render.hip, lv_peel.hip and lv_deferred.hip compile to the instructions they had;
// lv_render.hip holds the host code and calls the launch wrapper below.
#include "lv_internal.h"
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_deferred.h"
#include "lv_hull.h"
#include "lv_hull_pool.h"

namespace {

// what a launch of k_hull_pass writes to (RECORD: buf = the record pool, arg = its slots -- no new member, so that the kernel arguments
// of the other instances stay where they are)
struct LvHullOut {
    const uint32_t* requested;
    uint32_t* fragCount;
    unsigned long long* buf;
    uint32_t arg;
    LvHullList list;
};

// pixel (x, y) of the triangle's rectangle: coverage, the depth rule, the requested-pixel mask, the shading, the mode's store -- what
// stage C of k_stream_pass / k_dc_count_pass does for a line fragment.  kept: the fragment passed the depth rule on a requested pixel;
// the return value: it was stored (mode 10: past the gather's discard; RECORD: it got NO record -- what the rasteriser adds to fragCounter,
// the fragment stage adds the ones it keeps)
template <int STORE>
__device__ __forceinline__ bool lv_hull_pixel(const LvUniforms& U, const LvPrismDev& R, const LvHullDev& H, const LvVisRows& Z,
                                              const LvVisTri& T, const f3 N[3], uint32_t tri, uint32_t x, uint32_t y, const LvHullOut& O,
                                              LvDevCounters* dc, bool& kept) {
    kept = false;
    float e[3];
    if (!lv_vis_cover(R, T, x, y, e)) return false;
    const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
    if (O.requested && O.requested[addr] != 0u) return false;
    uint32_t zbits;
    f4 color;
    if (!lv_hull_fragment<STORE != LV_HULL_STORE_COUNT>(U, H, Z, T, N, e, zbits, color)) return false;
    kept = true;
    if constexpr (STORE == LV_HULL_STORE_RECORD) {
        return !lv_hull_record(reinterpret_cast<uint32_t*>(O.buf), O.arg, O.fragCount, addr, y * U.width + x, tri, dc);
    } else if constexpr (STORE == LV_HULL_STORE_COUNT) {
        atomicAdd(&O.fragCount[addr], 1u);
    } else if constexpr (STORE == LV_HULL_STORE_WBOIT) {
        lv_wboit_add(O.buf + size_t(addr) * LV_WBOIT_SUMS, color, __uint_as_float(zbits), O.arg);
        atomicAdd(&O.fragCount[addr], 1u);
    } else if constexpr (STORE == LV_HULL_STORE_AL64) {
        if (!(color.w >= 0.001f)) return false;   // AtomicLoop64Gather.glsl:56-59
        const unsigned long long key = ((unsigned long long)zbits << 32) | lv_pack_unorm4x8(color);
        unsigned long long* slots = O.buf + size_t(addr) * (size_t(O.arg) + LV_AL64_TAIL);
        lv_al64_insert(slots, O.arg, key, slots + O.arg);
        atomicAdd(&O.fragCount[addr], 1u);
    } else {
        const unsigned long long i = atomicAdd(O.list.counter, 1ull);
        if (i < O.list.capacity) {
            O.list.pixel[i] = y * U.width + x;
            O.list.triangle[i] = tri;
            O.list.depth[i] = __uint_as_float(zbits);
            O.list.rgba[i] = make_float4(color.x, color.y, color.z, color.w);
        }
    }
    return true;
}

// The skeleton of k_vis_raster: one lane per triangle; a lane walks a rectangle of at most LV_HULL_SMALL pixels itself, the larger ones
// are handed to the whole wave through a ballot, one after the other, and covered 8 x 8 pixels at a time with the triangle's setup done
// once per wave.  Hull triangles are few and large, so the wave's path is the common one: a workgroup is ONE wave (no LDS, nothing
// shared between waves), and the grid's y splits the viewport into bands of bandRows rows (a multiple of 8) -- a wave covers the part
// of its 64 triangles' rectangles inside its band, so that a mesh of a few hundred triangles still fills the device.  A pixel belongs
// to one band: which wave covers it never shows in the result.  Every loop is bounded by the band-clipped rectangle or by the 64 lanes.
template <int STORE>
__global__ __launch_bounds__(LV_WAVE) void k_hull_pass(const LvUniforms U, const LvPrismDev R, const LvHullDev H, const LvHullOut O,
                                                       uint32_t bandRows, LvDevCounters* dc, uint32_t collectStats) {
    const uint32_t lane = threadIdx.x, tri = blockIdx.x * LV_WAVE + lane;
    const int bandY0 = int(blockIdx.y * bandRows), bandY1 = min(bandY0 + int(bandRows), int(U.height)) - 1;
    const LvVisRows Z = lv_vis_rows(U);
    if constexpr (STORE == LV_HULL_STORE_RECORD) {   // the wave's chunk of record slots: none yet
        if (lane < 2u) lv_hull_chunk_set(int(lane), 0u);
        __syncthreads();
    }
    LvVisTri T;
    f3 N[3];
    bool live = tri < H.numTris && lv_hull_setup(U, H, tri, T, N);
    if (live) {
        T.y0 = max(T.y0, bandY0); T.y1 = min(T.y1, bandY1);
        live = T.y0 <= T.y1;
    }
    const uint32_t area = live ? uint32_t(T.x1 - T.x0 + 1) * uint32_t(T.y1 - T.y0 + 1) : 0u;
    const bool large = area > LV_HULL_SMALL;
    uint32_t keptLane = 0u, storedLane = 0u;   // the small rectangles' fragments, per lane
    if (live && !large) {
        for (int y = T.y0; y <= T.y1; y++)
            for (int x = T.x0; x <= T.x1; x++) {
                bool kept;
                storedLane += lv_hull_pixel<STORE>(U, R, H, Z, T, N, tri, uint32_t(x), uint32_t(y), O, dc, kept) ? 1u : 0u;
                keptLane += kept ? 1u : 0u;
            }
    }
    uint32_t keptSum = 0u, storedSum = 0u;     // the large rectangles' fragments, per wave (ballots)
    unsigned long long queue = __ballot(large);
    while (queue != 0ull) {
        const int src = __ffsll((long long)queue) - 1;
        queue &= queue - 1ull;
        const uint32_t t = uint32_t(__shfl(int(tri), src, 64));
        LvVisTri W;
        f3 M[3];
        if (!lv_hull_setup(U, H, t, W, M)) continue;   // (the same answer as its own lane's: true)
        W.y0 = max(W.y0, bandY0); W.y1 = min(W.y1, bandY1);
        for (int cy = W.y0; cy <= W.y1; cy += 8)
            for (int cx = W.x0; cx <= W.x1; cx += 8) {
                const int x = cx + int(lane & 7u), y = cy + int(lane >> 3);
                bool kept = false, stored = false;
                if (x <= W.x1 && y <= W.y1) stored = lv_hull_pixel<STORE>(U, R, H, Z, W, M, t, uint32_t(x), uint32_t(y), O, dc, kept);
                keptSum += uint32_t(__popcll(__ballot(kept)));
                storedSum += uint32_t(__popcll(__ballot(stored)));
            }
    }
    if constexpr (STORE == LV_HULL_STORE_LIST) return;   // (an inspection call: the frame's counters are not its to touch)
    if constexpr (STORE == LV_HULL_STORE_RECORD) {
        // the slots this wave reserved but did not use are part of the range the fragment stages walk: mark them dead
        __syncthreads();
        uint32_t* records = reinterpret_cast<uint32_t*>(O.buf);
        const uint32_t base = lv_hull_chunk_get(0), left = lv_hull_chunk_get(1);
        for (uint32_t k = lane; k < left; k += LV_WAVE)
            if (base + k < O.arg) { records[3 * size_t(base + k) + 0] = 0u; records[3 * size_t(base + k) + 1] = LV_PPLL_DEAD; }
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        keptLane += (uint32_t)__shfl_xor(int(keptLane), ofs, 64);
        storedLane += (uint32_t)__shfl_xor(int(storedLane), ofs, 64);
    }
    keptSum += keptLane; storedSum += storedLane;
    // lv_stats.fragments: every stored fragment (mode 10: past the discard); hits: every kept one -- as k_stream_pass / k_dc_count_pass
    if (lane == 0u && storedSum > 0u) atomicAdd(&dc->fragCounter, storedSum);
    if (collectStats != 0u && lane == 0u && keptSum > 0u) atomicAdd(&dc->hits, (unsigned long long)keptSum);
}

// The fragment stage of the hull records (lv_hull_pool.h): one lane per record {pixel + 1, LV_PPLL_DEAD, triangle} of the shared record
// pool, grid-stride over [0, min(fragAlloc, poolSlots)) like k_ppll_shade_prism, whose records carry a live word 1 and whose chunk tails
// and dead records carry word 0 == 0.  The fragment is computed again from the triangle and the pixel -- the same functions on the same
// operands as k_hull_pass, so it is covered and kept again; a record that were not is stored as a discarded fragment, never left
// unwritten -- and written as the mode's entry to run start + rank, the rank from the pixel's counter in `ranks`.
template <int ENTRY>
__global__ __launch_bounds__(LV_BLOCK) void k_hull_shade_records(const LvUniforms U, const LvPrismDev R, const LvHullDev H,
                                                                 const uint32_t* __restrict__ records, uint32_t* __restrict__ frags,
                                                                 const uint32_t* __restrict__ pixelOffset,
                                                                 const uint32_t* __restrict__ blockBase, uint32_t* __restrict__ fragCount,
                                                                 uint32_t* __restrict__ ranks, LvDevCounters* dc, uint32_t poolSlots,
                                                                 uint32_t keyBase) {
    const uint32_t numSlots = min(dc->fragAlloc, poolSlots);   // the chunk allocator's high-water mark
    const LvVisRows Z = lv_vis_rows(U);
    const f3 cam = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    uint32_t localSum = 0u, localDead = 0u;
    for (uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x; i < numSlots; i += gridDim.x * LV_BLOCK) {
        const uint32_t w0 = records[3 * size_t(i) + 0], w1 = records[3 * size_t(i) + 1], tri = records[3 * size_t(i) + 2];
        if (w1 != LV_PPLL_DEAD || w0 == 0u) continue;   // a line record; a chunk tail or a dead record
        const uint32_t pixel = w0 - 1u, x = pixel % U.width, y = pixel / U.width;
        LvVisTri T;
        f3 N[3];
        float e[3];
        uint32_t zbits = 0u;
        f4 color;
        color.x = 0.0f; color.y = 0.0f; color.z = 0.0f; color.w = 0.0f;
        const bool kept = tri < H.numTris && lv_hull_setup(U, H, tri, T, N) && lv_vis_cover(R, T, x, y, e) &&
                          lv_hull_fragment<true>(U, H, Z, T, N, e, zbits, color);
        const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
        const size_t dst = size_t(lv_run_start(pixelOffset, blockBase, addr)) + atomicAdd(&ranks[addr], 1u);
        if (kept && color.w >= 0.001f) {   // gatherFragment: discard below, LinkedListGather.glsl:34 (MLABGather.glsl:64)
            if constexpr (ENTRY == LV_ENTRY_MLAB) {
                f4 m;   // packUnorm4x8(vec4(color.rgb * color.a, 1.0 - color.a)), MLABGather.glsl:76
                m.x = color.x * color.w; m.y = color.y * color.w; m.z = color.z * color.w; m.w = 1.0f - color.w;
                uint32_t* en = frags + 3 * dst;
                en[0] = lv_pack_unorm4x8(m);
                en[1] = zbits;
                en[2] = keyBase + tri;
            } else {
                reinterpret_cast<uint2*>(frags)[dst] = make_uint2(lv_pack_unorm4x8(color), __float_as_uint(len3(lv_hull_position(T, e) - cam)));
            }
            localSum++;
        } else {
            if constexpr (ENTRY == LV_ENTRY_MLAB) {
                uint32_t* en = frags + 3 * dst;
                en[0] = 0u; en[1] = LV_PPLL_DEAD; en[2] = LV_MLAB_NO_KEY;
            } else {
                reinterpret_cast<uint2*>(frags)[dst] = make_uint2(0u, LV_PPLL_DEAD);
            }
            atomicAdd(&fragCount[addr], 0x10000u);
            localDead++;
        }
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        localSum += (uint32_t)__shfl_xor(int(localSum), ofs, 64);
        localDead += (uint32_t)__shfl_xor(int(localDead), ofs, 64);
    }
    if (lv_lane() == 0 && localSum > 0u) atomicAdd(&dc->fragCounter, localSum);   // fragCounter of the reference: every fragment counts
    if (lv_lane() == 0 && localDead > 0u) atomicAdd(&dc->prismDiscards, localDead);
}

} // namespace

// the launch geometry of k_hull_pass: blocks of 64 triangles x bands of bandRows rows
static dim3 lv_hull_grid(uint32_t numCUs, uint32_t numTris, uint32_t height, uint32_t& bandRows) {
    const uint32_t triBlocks = (numTris + LV_WAVE - 1u) / LV_WAVE;
    const uint32_t maxBands = (height + 7u) / 8u;
    const uint32_t wanted = (numCUs * LV_HULL_WAVES_PER_CU + triBlocks - 1u) / triBlocks;
    const uint32_t bands = wanted < 1u ? 1u : (wanted > maxBands ? maxBands : wanted);
    bandRows = (((height + bands - 1u) / bands + 7u) / 8u) * 8u;
    return dim3(triBlocks, (height + bandRows - 1u) / bandRows);
}
uint32_t lv_hull_launch_waves(uint32_t numCUs, uint32_t numTris, uint32_t height) {
    if (numTris == 0u || height == 0u) return 0u;
    uint32_t bandRows;
    const dim3 grid = lv_hull_grid(numCUs, numTris, height, bandRows);
    return grid.x * grid.y;
}

void lv_hull_launch(hipStream_t st, int store, uint32_t numCUs, const LvUniforms& U, const LvPrismDev& R, const LvHullDev& H,
                    const uint32_t* requested, uint32_t* fragCount, unsigned long long* buf, uint32_t arg, LvDevCounters* dc, bool stats,
                    const LvHullList& L) {
    if (H.numTris == 0u || U.width == 0u || U.height == 0u) return;
    uint32_t bandRows;
    const dim3 grid = lv_hull_grid(numCUs, H.numTris, U.height, bandRows);
    const LvHullOut O = {requested, fragCount, buf, arg, L};
    const uint32_t cs = stats ? 1u : 0u;
    switch (store) {
    case LV_HULL_STORE_COUNT: k_hull_pass<LV_HULL_STORE_COUNT><<<grid, LV_WAVE, 0, st>>>(U, R, H, O, bandRows, dc, cs); break;
    case LV_HULL_STORE_WBOIT: k_hull_pass<LV_HULL_STORE_WBOIT><<<grid, LV_WAVE, 0, st>>>(U, R, H, O, bandRows, dc, cs); break;
    case LV_HULL_STORE_AL64: k_hull_pass<LV_HULL_STORE_AL64><<<grid, LV_WAVE, 0, st>>>(U, R, H, O, bandRows, dc, cs); break;
    case LV_HULL_STORE_RECORD: k_hull_pass<LV_HULL_STORE_RECORD><<<grid, LV_WAVE, 0, st>>>(U, R, H, O, bandRows, dc, cs); break;
    default: k_hull_pass<LV_HULL_STORE_LIST><<<grid, LV_WAVE, 0, st>>>(U, R, H, O, bandRows, dc, cs); break;
    }
}

void lv_hull_shade_launch(hipStream_t st, int entry, uint32_t numCUs, const LvUniforms& U, const LvPrismDev& R, const LvHullDev& H,
                          const uint32_t* records, uint32_t* frags, const uint32_t* pixelOffset, const uint32_t* blockBase,
                          uint32_t* fragCount, uint32_t* ranks, LvDevCounters* dc, uint32_t poolSlots, uint32_t keyBase) {
    const uint32_t grid = numCUs * LV_HULL_SHADE_BLOCKS_PER_CU;
    if (entry == LV_ENTRY_MLAB)
        k_hull_shade_records<LV_ENTRY_MLAB><<<grid, LV_BLOCK, 0, st>>>(U, R, H, records, frags, pixelOffset, blockBase, fragCount, ranks, dc,
                                                                     poolSlots, keyBase);
    else
        k_hull_shade_records<LV_ENTRY_PPLL><<<grid, LV_BLOCK, 0, st>>>(U, R, H, records, frags, pixelOffset, blockBase, fragCount, ranks, dc,
                                                                     poolSlots, keyBase);
}
