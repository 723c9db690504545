// lv_linequad.hip -- the kernel of the line-quads pass (lv_linequad.h).  It lives here, not in lv_render.hip, for the reason lv_hull.hip
// does: the kernels of lv_render.hip, lv_peel.hip, lv_deferred.hip and lv_hull.hip compile to the instructions they had; lv_render.hip
// holds the host code and calls the launch wrapper below.
#include "lv_internal.h"
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_deferred.h"
#include "lv_linequad.h"

namespace {

// what a launch of k_linequad_pass writes to
struct LvLineQuadOut {
    const uint32_t* requested;
    uint32_t* fragCount;
    unsigned long long* buf;
    uint32_t arg;
    LvLineQuadList list;
};

// pixel (x, y) of the quad's rectangle: coverage, the requested-pixel mask, then per covered triangle the kept rules, the shading and
// the mode's store -- what stage C of k_stream_pass / k_dc_count_pass does for a prism fragment.  kept: fragments that passed the kept
// rules on a requested pixel; the return value: fragments stored (mode 10: past the gather's discard)
template <int STORE>
__device__ __forceinline__ uint32_t lv_linequad_pixel(const LvUniforms& U, const LvSceneDev& S, const LvVisRows& Z, const LvLineQuad& Q,
                                                      uint32_t leaf, uint32_t x, uint32_t y, const LvLineQuadOut& O, uint32_t& kept) {
    kept = 0u;
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    const unsigned mask = lv_linequad_coverage(S.prism, Q, o, x, y);
    if (mask == 0u) return 0u;
    const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
    if (O.requested && O.requested[addr] != 0u) return 0u;
    uint32_t stored = 0u;
    for (uint32_t t = 0u; t < 2u; t++) {
        if (((mask >> t) & 1u) == 0u) continue;
        uint32_t zbits;
        f4 color;
        if (!lv_linequad_fragment<STORE != LV_LINEQUAD_STORE_COUNT>(U, S, Z, Q, t, x, y, zbits, color)) continue;
        kept++;
        if constexpr (STORE == LV_LINEQUAD_STORE_COUNT) {
            atomicAdd(&O.fragCount[addr], 1u);
        } else if constexpr (STORE == LV_LINEQUAD_STORE_WBOIT) {
            lv_wboit_add(O.buf + size_t(addr) * LV_WBOIT_SUMS, color, __uint_as_float(zbits), O.arg);
            atomicAdd(&O.fragCount[addr], 1u);
        } else if constexpr (STORE == LV_LINEQUAD_STORE_AL64) {
            if (!(color.w >= 0.001f)) continue;   // AtomicLoop64Gather.glsl:56-59
            const unsigned long long key = ((unsigned long long)zbits << 32) | lv_pack_unorm4x8(color);
            unsigned long long* slots = O.buf + size_t(addr) * (size_t(O.arg) + LV_AL64_TAIL);
            lv_al64_insert(slots, O.arg, key, slots + O.arg);
            atomicAdd(&O.fragCount[addr], 1u);
        } else {
            const unsigned long long i = atomicAdd(O.list.counter, 1ull);
            if (i < O.list.capacity) {
                O.list.pixel[i] = y * U.width + x;
                O.list.segment[i] = S.leafSeg[leaf];
                O.list.triangle[i] = t;
                O.list.depth[i] = __uint_as_float(zbits);
                O.list.rgba[i] = make_float4(color.x, color.y, color.z, color.w);
            }
        }
        stored++;
    }
    return stored;
}

// The skeleton of k_hull_pass without its row bands: one lane per segment; a lane walks a rectangle of at most LV_LINEQUAD_SMALL pixels
// itself -- a quad is a line width wide and a segment long, a few dozen pixels at most in the scenes this is built for --, the larger
// ones (a segment next to the camera; the whole viewport when a vertex has clip w <= 0) are handed to the whole wave through a ballot,
// one after the other, and covered 8 x 8 pixels at a time.  A workgroup is ONE wave: no LDS, nothing shared between waves.  Every loop
// is bounded by a rectangle inside the viewport or by the 64 lanes.
template <int STORE>
__global__ __launch_bounds__(LV_WAVE) void k_linequad_pass(const LvUniforms U, const LvSceneDev S, const uint32_t* __restrict__ leafList,
                                                           const LvLineQuadOut O, LvDevCounters* dc, uint32_t collectStats) {
    const uint32_t lane = threadIdx.x, item = blockIdx.x * LV_WAVE + lane;
    const uint32_t numItems = leafList ? dc->prismListCount : S.numSegs;
    const LvVisRows Z = lv_vis_rows(U);
    const uint32_t leaf = item < numItems ? (leafList ? leafList[item] : item) : 0u;
    LvLineQuad Q;
    const bool live = item < numItems && leaf < S.numSegs && lv_linequad_setup(U, S, leaf, Q);
    const uint32_t area = live ? uint32_t(Q.x1 - Q.x0 + 1) * uint32_t(Q.y1 - Q.y0 + 1) : 0u;
    const bool large = area > LV_LINEQUAD_SMALL;
    uint32_t keptSum = 0u, storedSum = 0u;   // per lane
    if (live && !large) {
        for (int y = Q.y0; y <= Q.y1; y++)
            for (int x = Q.x0; x <= Q.x1; x++) {
                uint32_t kept;
                storedSum += lv_linequad_pixel<STORE>(U, S, Z, Q, leaf, uint32_t(x), uint32_t(y), O, kept);
                keptSum += kept;
            }
    }
    unsigned long long queue = __ballot(large);
    while (queue != 0ull) {
        const int src = __ffsll((long long)queue) - 1;
        queue &= queue - 1ull;
        const uint32_t l = uint32_t(__shfl(int(leaf), src, 64));
        LvLineQuad W;
        if (!lv_linequad_setup(U, S, l, W)) continue;   // (the same answer as its own lane's: true)
        for (int cy = W.y0; cy <= W.y1; cy += 8)
            for (int cx = W.x0; cx <= W.x1; cx += 8) {
                const int x = cx + int(lane & 7u), y = cy + int(lane >> 3);
                if (x <= W.x1 && y <= W.y1) {
                    uint32_t kept;
                    storedSum += lv_linequad_pixel<STORE>(U, S, Z, W, l, uint32_t(x), uint32_t(y), O, kept);
                    keptSum += kept;
                }
            }
    }
    if constexpr (STORE == LV_LINEQUAD_STORE_LIST) return;   // (an inspection call: the frame's counters are not its to touch)
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        keptSum += (uint32_t)__shfl_xor(int(keptSum), ofs, 64);
        storedSum += (uint32_t)__shfl_xor(int(storedSum), ofs, 64);
    }
    // lv_stats.fragments: every stored fragment (mode 10: past the discard); hits: every kept one -- as k_stream_pass / k_dc_count_pass
    if (lane == 0u && storedSum > 0u) atomicAdd(&dc->fragCounter, storedSum);
    if (collectStats != 0u && lane == 0u && keptSum > 0u) atomicAdd(&dc->hits, (unsigned long long)keptSum);
}

} // namespace

void lv_linequad_launch(hipStream_t st, int store, const LvUniforms& U, const LvSceneDev& S, const uint32_t* leafList,
                        const uint32_t* requested, uint32_t* fragCount, unsigned long long* buf, uint32_t arg, LvDevCounters* dc, bool stats,
                        const LvLineQuadList& L) {
    if (S.numSegs == 0u || U.width == 0u || U.height == 0u) return;
    const uint32_t grid = (S.numSegs + LV_WAVE - 1u) / LV_WAVE;
    const LvLineQuadOut O = {requested, fragCount, buf, arg, L};
    const uint32_t cs = stats ? 1u : 0u;
    switch (store) {
    case LV_LINEQUAD_STORE_COUNT: k_linequad_pass<LV_LINEQUAD_STORE_COUNT><<<grid, LV_WAVE, 0, st>>>(U, S, leafList, O, dc, cs); break;
    case LV_LINEQUAD_STORE_WBOIT: k_linequad_pass<LV_LINEQUAD_STORE_WBOIT><<<grid, LV_WAVE, 0, st>>>(U, S, leafList, O, dc, cs); break;
    case LV_LINEQUAD_STORE_AL64: k_linequad_pass<LV_LINEQUAD_STORE_AL64><<<grid, LV_WAVE, 0, st>>>(U, S, leafList, O, dc, cs); break;
    default: k_linequad_pass<LV_LINEQUAD_STORE_LIST><<<grid, LV_WAVE, 0, st>>>(U, S, leafList, O, dc, cs); break;
    }
}
