// lv_deferred.hip -- the kernels of the deferred visibility-buffer renderer (rendering mode 1, lv_deferred.h).  They live here, not in
// lv_render.hip, so that the existing kernels of that file compile to the instructions they had; lv_render.hip holds
// the frame function and calls the launch wrappers below.
#include "lv_internal.h"
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_deferred.h"

namespace {

__global__ __launch_bounds__(LV_BLOCK) void k_vis_clear(unsigned long long* __restrict__ words, size_t n) {
    const size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i < n) words[i] = LV_VIS_EMPTY;
}

// pixel (x, y) of the triangle's rectangle: coverage, the depth rule, the requested-pixel mask, ONE atomicMin
__device__ __forceinline__ void lv_vis_pixel(const LvUniforms& U, const LvPrismDev& R, const LvVisRows& Z, const LvVisTri& T, uint32_t tri,
                                             uint32_t x, uint32_t y, const uint32_t* __restrict__ requested, unsigned long long* words) {
    float e[3];
    if (!lv_vis_cover(R, T, x, y, e)) return;
    const uint32_t zbits = lv_vis_depth_bits(Z, T, e);
    if (!lv_peel_candidate(zbits, 0u, true)) return;   // 0 <= z < 1
    const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
    if (requested && requested[addr] != 0u) return;
    lv_vis_offer(words + addr, lv_peel_key(zbits, tri));
}

// One lane per triangle.  A lane walks a rectangle of at most LV_VIS_SMALL pixels itself; the larger ones (close-ups, a camera inside
// the data) are handed to the whole wave, one after the other, and covered 8 x 8 pixels at a time.  The hand-over needs no queue in
// memory: a wave holds at most one large triangle per lane, so the ballot of those lanes IS the queue and a lane broadcast reads its
// entries.  Every loop is bounded by the viewport-clipped rectangle or by the 64 lanes.
__global__ __launch_bounds__(LV_BLOCK) void k_vis_raster(const LvUniforms U, const LvSceneDev S, uint32_t numTris, uint32_t cull,
                                                         const uint32_t* __restrict__ requested, unsigned long long* words) {
    const uint32_t tri = blockIdx.x * LV_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    const LvVisRows Z = lv_vis_rows(U);
    LvVisTri T;
    const bool live = tri < numTris && lv_vis_setup(U, S, tri, cull != 0u, T);
    const uint32_t area = live ? uint32_t(T.x1 - T.x0 + 1) * uint32_t(T.y1 - T.y0 + 1) : 0u;
    const bool large = area > LV_VIS_SMALL;
    if (live && !large) {
        for (int y = T.y0; y <= T.y1; y++)
            for (int x = T.x0; x <= T.x1; x++) lv_vis_pixel(U, S.prism, Z, T, tri, uint32_t(x), uint32_t(y), requested, words);
    }
    unsigned long long queue = __ballot(large);
    while (queue != 0ull) {
        const int src = __ffsll((long long)queue) - 1;
        queue &= queue - 1ull;
        const uint32_t t = uint32_t(__shfl(int(tri), src, 64));
        LvVisTri W;
        if (!lv_vis_setup(U, S, t, cull != 0u, W)) continue;   // (the same answer as its own lane's: true)
        for (int cy = W.y0; cy <= W.y1; cy += 8)
            for (int cx = W.x0; cx <= W.x1; cx += 8) {
                const int x = cx + int(lane & 7u), y = cy + int(lane >> 3);
                if (x <= W.x1 && y <= W.y1) lv_vis_pixel(U, S.prism, Z, W, t, uint32_t(x), uint32_t(y), requested, words);
            }
    }
}

// lv_stats.fragments of a mode-1 frame: the requested viewport pixels that got a winner, counted from the words
__global__ __launch_bounds__(LV_BLOCK) void k_vis_count(const LvUniforms U, const uint32_t* __restrict__ requested,
                                                        const unsigned long long* __restrict__ words, LvDevCounters* dc) {
    const size_t n = size_t(U.width) * U.height;
    uint32_t count = 0u;
    for (size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x; p < n; p += size_t(gridDim.x) * LV_BLOCK) {
        const uint32_t addr = lv_ppll_addr(uint32_t(p % U.width), uint32_t(p / U.width), U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
        if (requested && requested[addr] != 0u) continue;
        if (uint32_t(words[addr]) != LV_VIS_NO_PRIMITIVE) count++;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) count += (uint32_t)__shfl_xor(int(count), ofs, 64);
    if (lv_lane() == 0 && count > 0u) atomicAdd(&dc->fragCounter, count);
}

// One lane per (tile, pixel) cell, one wave per workgroup, the cells and groups of k_wboit_resolve.  A pure function of the pixel's
// word: tiles that repeat or overlap write the same bytes.
template <int BANDS>
__global__ __launch_bounds__(LV_WAVE) void k_deferred_shade(const LvUniforms U, const LvSceneDev S, const LvTiles T,
                                                            const unsigned long long* __restrict__ words, uint32_t* __restrict__ out,
                                                            uint32_t numGroups) {
    const uint32_t lane = threadIdx.x;
    const uint32_t groupsX = T.blocksX / 4u, groupsPerTile = groupsX * (T.blocksY / 4u);
    for (uint32_t g = blockIdx.x; g < numGroups; g += gridDim.x) {
        const uint32_t slot = g >> 6, cell = g & 63u;
        const uint32_t grp = T.groupOrder ? T.groupOrder[slot] : slot;
        const uint32_t tile = grp / groupsPerTile, gi = grp % groupsPerTile;
        const uint32_t lx = (gi % groupsX) * 64u + (cell & 7u) * 8u + (lane & 7u);
        const uint32_t ly = (gi / groupsX) * 64u + (cell >> 3) * 8u + (lane >> 3);
        const bool inTile = lx < T.tileW && ly < T.tileH;
        if (!__any(inTile)) continue;
        const uint32_t x = T.tilesXY[2 * tile] + lx, y = T.tilesXY[2 * tile + 1] + ly;
        const uint32_t outIndex = (tile * T.tileH + ly) * T.tileW + lx;
        if (!inTile) continue;
        f4 c;
        c.x = U.background[0]; c.y = U.background[1]; c.z = U.background[2]; c.w = U.background[3];
        if (x < U.width && y < U.height) {
            const unsigned long long word = words[lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)];
            const uint32_t tri = uint32_t(word);
            if (tri != LV_VIS_NO_PRIMITIVE) {
                const LvDeferredFrag F = lv_deferred_fragment(U, S, x, y, __uint_as_float(uint32_t(word >> 32)), tri);
                const float aoTexel = U.useAmbientOcclusion ? S.ao[size_t(y) * U.width + x] : 1.0f;
                float hitT;
                c = lv_shade_triangle_barycentric<BANDS>(S, U, aoTexel, tri, F.u, F.v, F.w, F.pos, hitT);
            }
        }
        out[outIndex] = lv_pack_unorm4x8(c);
    }
}

__global__ __launch_bounds__(LV_BLOCK) void k_deferred_tf(const float4* __restrict__ tf, uint32_t n, float4* __restrict__ tfOpaque) {
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4 c = tf[i];
    c.w = 1.0f;
    tfOpaque[i] = c;
}

__global__ __launch_bounds__(LV_BLOCK) void k_vis_read(const unsigned long long* __restrict__ words, uint32_t width, uint32_t height,
                                                       uint32_t paddedW, uint32_t tileW, uint32_t tileH, uint32_t* __restrict__ outPrimitive,
                                                       float* __restrict__ outDepth) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p >= size_t(width) * height) return;
    const unsigned long long word = words[lv_ppll_addr(uint32_t(p % width), uint32_t(p / width), paddedW, tileW, tileH)];
    outPrimitive[p] = uint32_t(word);
    outDepth[p] = __uint_as_float(uint32_t(word >> 32));
}

__global__ __launch_bounds__(LV_BLOCK) void k_vis_pack(const uint32_t* __restrict__ primitive, const float* __restrict__ depth, size_t n,
                                                       unsigned long long* __restrict__ words) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p < n) words[p] = lv_peel_key(__float_as_uint(depth[p]), primitive[p]);
}

inline uint32_t lv_grid(size_t n) { return uint32_t((n + LV_BLOCK - 1) / LV_BLOCK); }

} // namespace

void lv_vis_launch_clear(hipStream_t st, unsigned long long* words, size_t n) {
    if (n) k_vis_clear<<<lv_grid(n), LV_BLOCK, 0, st>>>(words, n);
}
void lv_vis_launch_raster(hipStream_t st, const LvUniforms& U, const LvSceneDev& S, uint32_t numTris, bool cull, const uint32_t* requested,
                          unsigned long long* words) {
    if (numTris) k_vis_raster<<<lv_grid(numTris), LV_BLOCK, 0, st>>>(U, S, numTris, cull ? 1u : 0u, requested, words);
}
void lv_vis_launch_count(hipStream_t st, uint32_t grid, const LvUniforms& U, const uint32_t* requested, const unsigned long long* words,
                         LvDevCounters* dc) {
    k_vis_count<<<grid, LV_BLOCK, 0, st>>>(U, requested, words, dc);
}
void lv_deferred_launch_shade(hipStream_t st, uint32_t numGroups, int bands, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T,
                              const unsigned long long* words, uint32_t* out) {
    if (bands == LV_SHADE_BANDS) k_deferred_shade<LV_SHADE_BANDS><<<numGroups, LV_WAVE, 0, st>>>(U, S, T, words, out, numGroups);
    else if (bands == LV_SHADE_HELICITY) k_deferred_shade<LV_SHADE_HELICITY><<<numGroups, LV_WAVE, 0, st>>>(U, S, T, words, out, numGroups);
    else k_deferred_shade<LV_SHADE_PLAIN><<<numGroups, LV_WAVE, 0, st>>>(U, S, T, words, out, numGroups);
}
void lv_deferred_launch_tf(hipStream_t st, const float4* tf, uint32_t n, float4* tfOpaque) {
    if (n) k_deferred_tf<<<lv_grid(n), LV_BLOCK, 0, st>>>(tf, n, tfOpaque);
}
void lv_vis_launch_read(hipStream_t st, const unsigned long long* words, uint32_t w, uint32_t h, uint32_t paddedW, uint32_t tileW,
                        uint32_t tileH, uint32_t* outPrimitive, float* outDepth) {
    k_vis_read<<<lv_grid(size_t(w) * h), LV_BLOCK, 0, st>>>(words, w, h, paddedW, tileW, tileH, outPrimitive, outDepth);
}
void lv_vis_launch_pack(hipStream_t st, const uint32_t* primitive, const float* depth, size_t n, unsigned long long* words) {
    k_vis_pack<<<lv_grid(n), LV_BLOCK, 0, st>>>(primitive, depth, n, words);
}
