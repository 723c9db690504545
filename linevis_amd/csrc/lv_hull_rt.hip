// lv_hull_rt.hip -- the ray tracer's colour pass with the simulation-mesh hull (hull_ray_tracing = on; semantics: lv_hull_rt.h).
//
//   k_render_rt_hull    TubeRayTracing.RayGen/.Miss with the hull BLAS in the TLAS: k_render_rt's loop, each step the nearer of the
//                       closest line hit and the closest hull hit (ClosestHitHull, TubeRayTracing.glsl:359-431)
//   k_trace_rays_hull   the closest hull hit of arbitrary rays (lv_trace_rays_hull)
//
// A translation unit of its own: k_render_rt and the other tile kernels keep their code.
#include "lv_internal.h"
#include "lv_trace.h"
#include "lv_tile.h"
#include "lv_hull_rt.h"

namespace {

// Block and tile geometry, sample loop, blend and store are k_render_rt's.  Both walks are wave-cooperative: control flow around
// them is wave-uniform, lanes that are done or outside the view pass active = false.  They run one after the other on the SAME LDS
// stack window and the same per-wave scratch (lv_trace_closest leaves both free when it returns).
// rec: rt_record_hits -- one record per step that hit, appended in whatever order the lanes arrive (lv_rt_get_hits sorts nothing).
// Register limit: k_render_rt's LV_RT_MIN_WAVES waves per SIMD where the variant fits it without scratch; the helicity-band and the
// banded triangle-mesh variants do not (12 - 44 B per lane at 128 VGPRs) and are compiled for 3 waves per SIMD (tools/isa_report.py).
constexpr int lv_hull_rt_min_waves(bool stats, int prim, int bands) {
    return (stats || prim == LV_PRIM_ELLIPTIC) ? 1
           : (bands == LV_SHADE_HELICITY || (prim == LV_PRIM_TRIANGLE && bands != LV_SHADE_PLAIN)) ? 3 : LV_RT_MIN_WAVES;
}
template <bool STATS, int PRIM, int BANDS>
__global__ __launch_bounds__(LV_BLOCK, lv_hull_rt_min_waves(STATS, PRIM, BANDS)) void k_render_rt_hull(
        const LvUniforms U, const LvSceneDev S, const LvHullRtDev R, const LvTiles T, uint32_t* __restrict__ out, LvDevCounters* dc,
        uint32_t* __restrict__ rec, uint32_t recCap) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    LvPixel px;
    if (!lv_block_pixel(U, T, px)) return;
    const unsigned long long tg0 = lv_group_clock();
    const LvStackMem sm = lv_stack_mem(s_stack, S.stackOverflow);
    const LvSceneDev SH = lv_hull_rt_view(S, R);
    LvCounters cnt = {0, 0, 0, 0};
    const bool capped = U.useCappedTubes != 0 || U.lssGeometry != 0;
    const float HIT_DISTANCE_EPSILON = 1e-5f;
    const float aoTexel = (px.inView && U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(px.y) * U.width + px.x] : 1.0f;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t nSamples = U.useJitteredRays ? U.numSamplesPerFrame : 1u;
    for (uint32_t sampleIdx = 0; sampleIdx < nSamples; sampleIdx++) { // uniform trip count
        float xix = 0.5f, xiy = 0.5f;
        if (U.useJitteredRays) {
            uint32_t seed = U.useDeterministicSampling
                    ? lv_tea(19u, U.frameNumber * U.numSamplesPerFrame + sampleIdx)
                    : lv_tea(px.x + px.y * U.width, U.frameNumber * U.numSamplesPerFrame + sampleIdx);
            xix = lv_rnd(seed);
            xiy = lv_rnd(seed);
        }
        f3 o, d;
        lv_primary_ray(U, px.x, px.y, xix, xiy, o, d);
        float fc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float tMin = 0.0001f;
        const float tMax = 1000.0f;
        bool tracing = px.inView;
        for (uint32_t hitIdx = 0; hitIdx < U.maxDepthComplexity && __any(tracing); hitIdx++) {
            const LvHit h = lv_trace_closest<STATS, false, PRIM>(S, U.radius, capped, tracing, o, d, tMin, tMax, sm, cm, cnt);
            // the hull hit only matters in front of the line hit: [tMin, tL] (a tie goes to the line)
            const LvHit hh = lv_trace_closest<STATS, false, LV_PRIM_TRIANGLE, false, true>(SH, 0.0f, false, tracing, o, d, tMin, h.found ? h.t : tMax, sm, cm, cnt);
            if (tracing) {
                const bool hull = hh.found && (!h.found || hh.t < h.t);
                f4 hc;
                float payloadHitT;
                if (hull) {
                    hc = lv_hull_rt_hit(U, R, hh.leaf, o, d, payloadHitT);
                    if (STATS) cnt.hits++;
                } else if (h.found) {
                    hc = PRIM == LV_PRIM_TRIANGLE   ? lv_shade_hit_triangle<BANDS>(S, U, aoTexel, o, d, h.leaf, payloadHitT)
                         : PRIM == LV_PRIM_ELLIPTIC ? lv_shade_hit_elliptic(S, U, aoTexel, o, d, h, payloadHitT)
                                                    : lv_shade_hit<BANDS>(S, U, aoTexel, o, d, h, payloadHitT);
                    if (STATS) cnt.hits++;
                } else { // Miss, TubeRayTracing.glsl:290-297
                    hc.x = U.background[0]; hc.y = U.background[1]; hc.z = U.background[2]; hc.w = U.background[3];
                    payloadHitT = 0.0f;
                }
                if (STATS && rec && (hull || h.found)) {
                    const uint32_t slot = atomicAdd(&dc->mlatTraceCount, 1u);
                    if (slot < recCap) {
                        uint32_t* r = rec + size_t(slot) * LV_RT_HIT_WORDS;
                        r[0] = px.y * U.width + px.x;
                        r[1] = (sampleIdx << 16) | hitIdx;
                        r[2] = hull ? (LV_RT_HIT_HULL | hh.leaf)
                                    : PRIM == LV_PRIM_TRIANGLE ? (h.leaf << 2) : ((S.leafSeg[h.leaf] << 2) | uint32_t(h.kind));
                        r[3] = __float_as_uint(hull ? hh.t : h.t);
                        r[4] = __float_as_uint(payloadHitT);
                        r[5] = __float_as_uint(hc.x); r[6] = __float_as_uint(hc.y); r[7] = __float_as_uint(hc.z); r[8] = __float_as_uint(hc.w);
                    }
                }
                tMin = payloadHitT + fmaxf(payloadHitT * HIT_DISTANCE_EPSILON, 1e-7f);
                fc[0] = fc[0] + ((1.0f - fc[3]) * hc.w) * hc.x;
                fc[1] = fc[1] + ((1.0f - fc[3]) * hc.w) * hc.y;
                fc[2] = fc[2] + ((1.0f - fc[3]) * hc.w) * hc.z;
                fc[3] = fc[3] + (1.0f - fc[3]) * hc.w;
                if (!(hull || h.found) || fc[3] > 0.99f) tracing = false;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] += fc[k];
    }
    if (px.inView) {
        if (U.useJitteredRays) {
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] /= float(U.numSamplesPerFrame);
        }
        f4 c; c.x = acc[0]; c.y = acc[1]; c.z = acc[2]; c.w = acc[3];
        out[px.outIndex] = lv_store_color(S, U, px.x, px.y, c);
    } else if (px.inTile) {
        f4 c; c.x = U.background[0]; c.y = U.background[1]; c.z = U.background[2]; c.w = U.background[3];
        out[px.outIndex] = lv_pack_unorm4x8(c);
    }
    lv_group_cost_add(T, px, tg0);
    if (STATS) { lv_flush_max_nodes(cnt, dc); lv_flush_counters(cnt, dc); }
}

// as k_trace_rays_tri on the hull LBVH
__global__ __launch_bounds__(LV_BLOCK) void k_trace_rays_hull(const LvSceneDev S, const LvHullRtDev R, const float* __restrict__ org,
                                                              const float* __restrict__ dir, float tMin, float tMax, uint32_t n,
                                                              float* __restrict__ outT, uint32_t* __restrict__ outTri, float* __restrict__ outUV) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    const bool valid = i < n;
    LvCounters cnt = {0, 0, 0, 0};
    const uint32_t j = valid ? i : 0u;
    const f3 o = mk3(org[3 * size_t(j)], org[3 * size_t(j) + 1], org[3 * size_t(j) + 2]);
    const f3 d = mk3(dir[3 * size_t(j)], dir[3 * size_t(j) + 1], dir[3 * size_t(j) + 2]);
    const LvSceneDev SH = lv_hull_rt_view(S, R);
    const LvHit h = lv_trace_closest<false, false, LV_PRIM_TRIANGLE, false, true>(SH, 0.0f, false, valid, o, d, tMin, tMax,
                                                                     lv_stack_mem(s_stack, S.stackOverflow), cm, cnt);
    if (!valid) return;
    float t = tMax, u = 0.0f, v = 0.0f;
    if (h.found) lv_hull_rt_tuv(R, h.leaf, o, d, t, u, v);
    outT[i] = h.found ? h.t : tMax;
    outTri[i] = h.found ? h.leaf : 0xFFFFFFFFu;
    outUV[2 * size_t(i)] = u;
    outUV[2 * size_t(i) + 1] = v;
}

template <bool STATS>
int launchHullRt(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvHullRtDev& R, const LvTiles& T, uint32_t gridTiles,
                 uint32_t* out, LvDevCounters* dc, bool tri, uint32_t* rec, uint32_t recCap) {
    hipStream_t st = ctx->stream;
#define LV_LAUNCH_RT_HULL(PR, BA) \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_RENDER_RT, (k_render_rt_hull<STATS, PR, BA><<<gridTiles, LV_BLOCK, 0, st>>>(U, S, R, T, out, dc, rec, recCap)))
    // the variants of the colour pass, as lv_rt_frame selects them
    if (tri && U.useHelicityBands) LV_LAUNCH_RT_HULL(LV_PRIM_TRIANGLE, LV_SHADE_HELICITY);
    else if (tri && U.useBands) LV_LAUNCH_RT_HULL(LV_PRIM_TRIANGLE, LV_SHADE_BANDS);
    else if (tri) LV_LAUNCH_RT_HULL(LV_PRIM_TRIANGLE, LV_SHADE_PLAIN);
    else if (U.useHelicityBands) LV_LAUNCH_RT_HULL(LV_PRIM_CAPSULE, LV_SHADE_HELICITY);
    else if (U.useEllipticTubes) LV_LAUNCH_RT_HULL(LV_PRIM_ELLIPTIC, LV_SHADE_BANDS);
    else if (U.useBands) LV_LAUNCH_RT_HULL(LV_PRIM_CAPSULE, LV_SHADE_BANDS);
    else LV_LAUNCH_RT_HULL(LV_PRIM_CAPSULE, LV_SHADE_PLAIN);
#undef LV_LAUNCH_RT_HULL
    return LV_OK;
}

} // namespace

int lv_hull_rt_render(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvHullRtDev& R, const LvTiles& T, uint32_t gridTiles,
                      uint32_t* out, LvDevCounters* dc, bool triangles, uint32_t* rec, uint32_t recCap) {
    return (ctx->opt.collectStats || rec) ? launchHullRt<true>(ctx, U, S, R, T, gridTiles, out, dc, triangles, rec, recCap)
                                          : launchHullRt<false>(ctx, U, S, R, T, gridTiles, out, dc, triangles, nullptr, 0u);
}

void lv_hull_rt_trace_rays(hipStream_t st, const LvSceneDev& S, const LvHullRtDev& R, const float* org, const float* dir, float tMin, float tMax,
                           uint32_t n, float* outT, uint32_t* outTri, float* outUV) {
    k_trace_rays_hull<<<uint32_t((uint64_t(n) + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(S, R, org, dir, tMin, tMax, n, outT, outTri, outUV);
}
