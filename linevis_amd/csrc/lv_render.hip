// lv_render.hip -- frame kernels of the hot path and their orchestration.
//
// Kernel                reference program it replaces
//   k_render_rt         TubeRayTracing.RayGen/.Miss (+ driver traversal, IntersectionTube, ClosestHitTubeAnalytic)
//                       Data/Shaders/Renderers/RayTracing/TubeRayTracing.glsl:61-82,198-298
//   k_ao_primary        VulkanRayTracedAmbientOcclusion.Compute, primary-ray half (glsl:178-281) + wave compaction
//   k_ao_rays           .. sample loop (glsl:288-306) as persistent waves pulling AO rays from a global queue
//   k_ao_reduce         .. per-pixel sum in sample order + accumulate/store (glsl:309-319)
//   k_ppll_gather       tube rasterisation + gatherFragment, Data/Shaders/Renderers/PPLL/LinkedListGather.glsl:33-72
//   k_ppll_resolve      LinkedListResolve.Fragment + frontToBackPQ, LinkedListResolve.glsl:57-105, LinkedListSort.glsl:177-238
//   k_depth_minmax      ComputeDepthValues.Compute + MinMaxReduce.Compute, Data/Shaders/DepthCues/*.glsl
//   k_bake_setup        VulkanAmbientOcclusionBaker.Compute, line-point interpolation + ray origins (glsl:110-131,231-262);
//                       its sample loop runs as the BAKE instantiation of k_ao_rays, the running mean in k_ao_reduce<true>
// The triangle instantiations (LV_PRIM_TRIANGLE) of k_ao_primary / k_ao_rays / k_render_rt trace the reference's
// triangle tubes (RTAO geometry, "Triangle Mesh" geometry mode: ClosestHitTubeTriangles, TubeRayTracing.glsl:301-352).
// Host orchestration follows VulkanRayTracer::render (VulkanRayTracer.cpp:131-154), LineRenderer::renderBase
// (LineRenderer.cpp:248-277) and PerPixelLinkedListLineRenderer::render (PerPixelLinkedListLineRenderer.cpp:399-427).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "lv_internal.h"
#include "lv_trace.h"
#include "lv_tile.h"
#include "lv_mboit.h"
#include "lv_al64.h"
#include "lv_wboit.h"
#include "lv_peel.h"
#include "lv_deferred.h"
#include "lv_hull.h"
#include "lv_hull_pool.h"
#include "lv_hull_rt.h"
#include "lv_linequad.h"

namespace {

// ================================================================ ray tracer colour pass
// Control flow is wave-uniform around every trace (lv_trace_closest is a wave-cooperative routine): the sample loop and
// the transparency loop run while ANY lane of the wave still needs a trace; lanes that are done pass active = false.
// PRE: the hits of every pixel's ray were traced ahead of the RTAO pass (lv_colour_first_hits, launched together with the RTAO
// primaries: k_primary_pair) and wait in firstHit[k * stride + px.outIndex] = {t bits, (leaf << 2) | kind or LV_INVALID}, k = position in
// the transparency loop, k < LV_PRE_HITS; the kernel shades them and only traces where a pixel's loop goes deeper than that.  Same hits,
// same frame, byte for byte: which hit follows which depends on the alpha of the shaded hit, and alpha (transfer function x silhouette
// coverage) does not depend on the ambient occlusion.
#define LV_PRE_HITS 4u
template <bool STATS, int PRIM, int BANDS = LV_SHADE_PLAIN, bool PRE = false, int FAST = 0>
__global__ __launch_bounds__(LV_BLOCK, (STATS || PRIM == LV_PRIM_ELLIPTIC) ? 1 : LV_RT_MIN_WAVES) void k_render_rt(const LvUniforms U, const LvSceneDev S, const LvTiles T,
                                                        uint32_t* __restrict__ out, LvDevCounters* dc,
                                                        const uint2* __restrict__ firstHit = nullptr, const size_t firstHitStride = 0) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    LvPixel px;
    if (!lv_block_pixel(U, T, px)) return;
    const unsigned long long tg0 = lv_group_clock();
    const LvStackMem sm = lv_stack_mem(s_stack, S.stackOverflow);
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
        // traceRayTransparent, TubeRayTracing.glsl:61-82
        float fc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float tMin = 0.0001f;
        const float tMax = 1000.0f;
        bool tracing = px.inView;
        for (uint32_t hitIdx = 0; hitIdx < U.maxDepthComplexity && __any(tracing); hitIdx++) {
            LvHit h;
            if (PRE && hitIdx < LV_PRE_HITS && sampleIdx == 0u) {
                h.found = false; h.t = 0.0f; h.leaf = 0u; h.kind = 0;
                if (tracing) {
                    const uint2 fh = firstHit[size_t(hitIdx) * firstHitStride + px.outIndex];
                    h.found = fh.y != LV_INVALID;
                    h.t = __uint_as_float(fh.x);
                    h.leaf = fh.y >> 2;
                    h.kind = int(fh.y & 3u);
                }
            } else {
                h = lv_trace_closest<STATS, false, PRIM>(S, U.radius, capped, tracing, o, d, tMin, tMax, sm, cm, cnt);
            }
            if (tracing) {
                f4 hc;
                float payloadHitT;
                if (h.found) {
                    hc = PRIM == LV_PRIM_TRIANGLE   ? lv_shade_hit_triangle<BANDS>(S, U, aoTexel, o, d, h.leaf, payloadHitT)
                         : PRIM == LV_PRIM_ELLIPTIC ? lv_shade_hit_elliptic(S, U, aoTexel, o, d, h, payloadHitT)
                                                    : lv_shade_hit<BANDS, FAST>(S, U, aoTexel, o, d, h, payloadHitT);
                    if (STATS) cnt.hits++;
                } else { // Miss, TubeRayTracing.glsl:290-297
                    hc.x = U.background[0]; hc.y = U.background[1]; hc.z = U.background[2]; hc.w = U.background[3];
                    payloadHitT = 0.0f;
                }
                tMin = payloadHitT + fmaxf(payloadHitT * HIT_DISTANCE_EPSILON, 1e-7f);
                fc[0] = fc[0] + ((1.0f - fc[3]) * hc.w) * hc.x;
                fc[1] = fc[1] + ((1.0f - fc[3]) * hc.w) * hc.y;
                fc[2] = fc[2] + ((1.0f - fc[3]) * hc.w) * hc.z;
                fc[3] = fc[3] + (1.0f - fc[3]) * hc.w;
                if (!h.found || fc[3] > 0.99f) tracing = false;
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

// ================================================================ RTAO
// G-buffer layout: LvAoLayout, lv_tile.h
// G-buffer entry of a pixel whose primary ray hit: 3 x float4
//   g0 = {hit position, offsetFactor}, g1 = {surface tangent, pixel index bits}, g2 = {surface normal, 0}
template <bool STATS, int PRIM>
__device__ __forceinline__ void lv_ao_primary_body(const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t blockId,
                                                   unsigned* s_stack, LvCoopMem& cm,
                                                   const float* aoIn, float* ao, float4* __restrict__ gbuf,
                                                   uint32_t* __restrict__ groupCount, LvDevCounters* dc,
                                                   const float4* featNormalIn, float4* featNormal,
                                                   const float4* featPositionIn, float4* featPosition,
                                                   const LvSvgfFeat& SF) {
    LvPixel px;
    if (!lv_block_pixel(U, T, px, blockId)) return;
    const unsigned long long tg0 = lv_group_clock();
    LvCounters cnt = {0, 0, 0, 0};
    bool hasHit = false;
    float4 g0, g1, g2;
    const uint32_t pix = px.x + px.y * U.width;
    const uint32_t globalFrameNumber = U.aoGlobalFrameNumber; // VulkanRayTracedAmbientOcclusion.cpp:576-581
    uint32_t seed = lv_tea(pix, globalFrameNumber);
    float xix = 0.5f, xiy = 0.5f;
    if (U.aoJitterPrimary) { xix = lv_rnd(seed); xiy = lv_rnd(seed); }
    f3 o, d;
    lv_primary_ray(U, px.x, px.y, xix, xiy, o, d);
    // wave-cooperative: every lane calls, lanes outside the viewport only help testing
    const LvHit h = lv_trace_closest<STATS, false, PRIM>(S, U.radius, U.useCappedTubes != 0, px.inView, o, d, 0.0001f,
                                                         1000.0f, lv_stack_mem(s_stack, S.stackOverflow), cm, cnt);
    if (px.inView) {
        if (h.found && PRIM == LV_PRIM_TRIANGLE) {
            // barycentric reconstruction, VulkanRayTracedAmbientOcclusion.glsl:219-263,280
            hasHit = true;
            const uint32_t i0 = S.triIdx[3 * size_t(h.leaf)], i1 = S.triIdx[3 * size_t(h.leaf) + 1],
                           i2 = S.triIdx[3 * size_t(h.leaf) + 2];
            const lv_tube_vertex& vd0 = S.triVerts[i0];
            const lv_tube_vertex& vd1 = S.triVerts[i1];
            const lv_tube_vertex& vd2 = S.triVerts[i2];
            const f3 p0 = mk3(vd0.vertexPosition[0], vd0.vertexPosition[1], vd0.vertexPosition[2]);
            const f3 p1 = mk3(vd1.vertexPosition[0], vd1.vertexPosition[1], vd1.vertexPosition[2]);
            const f3 p2 = mk3(vd2.vertexPosition[0], vd2.vertexPosition[1], vd2.vertexPosition[2]);
            float tt = 0.0f, bu = 0.0f, bv = 0.0f; // same function, same inputs as the winning test: identical (t, u, v)
            lv_ray_triangle(o, d, mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), p0, p1, p2, S.triPad, tt, bu, bv);
            const float b0 = (1.0f - bu) - bv;
            const lv_line_point& lp0 = S.triPoints[vd0.vertexLinePointIndex & 0x7FFFFFFFu];
            const lv_line_point& lp1 = S.triPoints[vd1.vertexLinePointIndex & 0x7FFFFFFFu];
            const lv_line_point& lp2 = S.triPoints[vd2.vertexLinePointIndex & 0x7FFFFFFFu];
            auto lerp3 = [&](const float* a, const float* b, const float* c) {
                return (mk3(a[0], a[1], a[2]) * b0 + mk3(b[0], b[1], b[2]) * bu) + mk3(c[0], c[1], c[2]) * bv;
            };
            const f3 vertexPositionWorld = lerp3(vd0.vertexPosition, vd1.vertexPosition, vd2.vertexPosition);
            const f3 surfaceNormal = norm3(lerp3(vd0.vertexNormal, vd1.vertexNormal, vd2.vertexNormal));
            const f3 linePosition = lerp3(lp0.linePosition, lp1.linePosition, lp2.linePosition);
            const f3 surfaceTangent = norm3(lerp3(lp0.lineTangent, lp1.lineTangent, lp2.lineTangent));
            const float offsetFactor = len3(linePosition - vertexPositionWorld) / U.subdivisionCorrectionFactor;
            g0 = make_float4(vertexPositionWorld.x, vertexPositionWorld.y, vertexPositionWorld.z, offsetFactor);
            g1 = make_float4(surfaceTangent.x, surfaceTangent.y, surfaceTangent.z, __uint_as_float(pix));
            g2 = make_float4(surfaceNormal.x, surfaceNormal.y, surfaceNormal.z, 0.0f);
        } else if (h.found && PRIM == LV_PRIM_ELLIPTIC) {
            // band data: the reference's RTAO pass traces the elliptic TRIANGLE tubes (createCappedTriangleEllipticTubesRenderDataCPU);
            // the build traces the analytic tubelets of the colour pass -- the same substitution as capsules for circular tubes
            hasHit = true;
            const uint32_t seg = S.leafSeg[h.leaf];
            const lv_line_point& lp0 = S.points[S.segIdx[2 * seg]];
            const lv_line_point& lp1 = S.points[S.segIdx[2 * seg + 1]];
            const LvEllipticSurface E = lv_elliptic_surface(U, o, d, h.t, lp0, lp1);
            const f3 vertexPositionWorld = o + d * h.t;
            const f3 t0 = mk3(lp0.lineTangent[0], lp0.lineTangent[1], lp0.lineTangent[2]);
            const f3 t1 = mk3(lp1.lineTangent[0], lp1.lineTangent[1], lp1.lineTangent[2]);
            const f3 surfaceTangent = norm3((1.0f - E.t) * t0 + E.t * t1);
            const float offsetFactor = len3(E.linePosition - vertexPositionWorld) / U.subdivisionCorrectionFactor;
            g0 = make_float4(vertexPositionWorld.x, vertexPositionWorld.y, vertexPositionWorld.z, offsetFactor);
            g1 = make_float4(surfaceTangent.x, surfaceTangent.y, surfaceTangent.z, __uint_as_float(pix));
            g2 = make_float4(E.normal.x, E.normal.y, E.normal.z, 0.0f);
        } else if (h.found) {
            hasHit = true;
            const float4 ra = S.segs[2 * h.leaf], rb = S.segs[2 * h.leaf + 1];
            const uint32_t seg = S.leafSeg[h.leaf];
            const lv_line_point& lp0 = S.points[S.segIdx[2 * seg]];
            const lv_line_point& lp1 = S.points[S.segIdx[2 * seg + 1]];
            const f3 P0 = mk3(ra.x, ra.y, ra.z), P1 = mk3(rb.x, rb.y, rb.z);
            f3 vertexPositionWorld = o + d * h.t;
            f3 v = P1 - P0;
            float ts;
            if (h.kind == 0) ts = dot3(v, vertexPositionWorld - P0) / dot3(v, v);
            else ts = h.kind == 1 ? 0.0f : 1.0f;
            f3 linePosition = h.kind == 0 ? P0 + ts * v : (h.kind == 1 ? P0 : P1);
            f3 surfaceNormal = norm3(vertexPositionWorld - linePosition);
            f3 t0 = mk3(lp0.lineTangent[0], lp0.lineTangent[1], lp0.lineTangent[2]);
            f3 t1 = mk3(lp1.lineTangent[0], lp1.lineTangent[1], lp1.lineTangent[2]);
            f3 surfaceTangent = norm3((1.0f - ts) * t0 + ts * t1);
            float offsetFactor = len3(linePosition - vertexPositionWorld) / U.subdivisionCorrectionFactor;
            g0 = make_float4(vertexPositionWorld.x, vertexPositionWorld.y, vertexPositionWorld.z, offsetFactor);
            g1 = make_float4(surfaceTangent.x, surfaceTangent.y, surfaceTangent.z, __uint_as_float(pix));
            g2 = make_float4(surfaceNormal.x, surfaceNormal.y, surfaceNormal.z, 0.0f);
        } else {
            // miss: aoFactor = 1, accumulate (glsl:311-319)
            float aoFactor = 1.0f;
            if (U.aoFrameNumber != 0) aoFactor = mixf(aoIn[pix], aoFactor, 1.0f / float(U.aoFrameNumber + 1));
            ao[pix] = aoFactor;
        }
    }
    // denoiser feature maps (VulkanRayTracedAmbientOcclusion.glsl:321-399, WRITE_NORMAL_MAP / WRITE_POSITION_MAP with
    // accumulation): view-space normal {xyz, 0} and view-space position {xyz, 1} of the primary hit; a miss leaves
    // surfaceNormal = vertexPositionWorld = 0 (glsl:211-212); running means over the iterations
    if (featNormal && px.inView) {
        const f3 sn = hasHit ? mk3(g2.x, g2.y, g2.z) : mk3(0.0f, 0.0f, 0.0f);
        const f3 vp = hasHit ? mk3(g0.x, g0.y, g0.z) : mk3(0.0f, 0.0f, 0.0f);
        // camNormal = (transpose(inverseViewMatrix) * vec4(surfaceNormal, 0)).xyz, VulkanRayTracedAmbientOcclusion.cpp:569
        const float* m = U.invView;
        f3 n = mk3(((m[0] * sn.x + m[1] * sn.y) + m[2] * sn.z) + m[3] * 0.0f, ((m[4] * sn.x + m[5] * sn.y) + m[6] * sn.z) + m[7] * 0.0f,
                   ((m[8] * sn.x + m[9] * sn.y) + m[10] * sn.z) + m[11] * 0.0f);
        const f4 pv = mulM4(U.view, vp.x, vp.y, vp.z, 1.0f);
        f3 q = mk3(pv.x, pv.y, pv.z);
        if (U.aoFrameNumber != 0) {
            const float a = 1.0f / float(U.aoFrameNumber + 1);
            const float4 on = featNormalIn[pix], op = featPositionIn[pix];
            n = mk3(mixf(on.x, n.x, a), mixf(on.y, n.y, a), mixf(on.z, n.z, a));
            const float len = len3(n);
            if (len > 1e-5f) n = mk3(n.x / len, n.y / len, n.z / len);
            q = mk3(mixf(op.x, q.x, a), mixf(op.y, q.y, a), mixf(op.z, q.z, a));
        }
        featNormal[pix] = make_float4(n.x, n.y, n.z, 0.0f);
        featPosition[pix] = make_float4(q.x, q.y, q.z, 1.0f);
    }
    if (SF.normalDepth && px.inView) {
        // SVGF's maps, not accumulated: world-space normal (0 on a miss), depth = -z_view (farDistance on a miss), flow =
        // writePos - the hit's pixel position under last frame's view-projection, depth fwidth = |cot| of the angles between
        // the view-space normal and the camera x / y axes (glsl:350-464)
        const f3 sn = hasHit ? mk3(g2.x, g2.y, g2.z) : mk3(0.0f, 0.0f, 0.0f);
        const f3 vp = hasHit ? mk3(g0.x, g0.y, g0.z) : mk3(0.0f, 0.0f, 0.0f);
        const f4 pv = mulM4(U.view, vp.x, vp.y, vp.z, 1.0f);
        float fx = 0.0f, fy = 0.0f, fw = 0.0f;
        if (hasHit) {
            f4 ndc = mulM4(SF.lastFrameViewProj, vp.x, vp.y, vp.z, 1.0f);
            ndc.x /= ndc.w; ndc.y /= ndc.w;
            fx = float(px.x) - ((0.5f * ndc.x + 0.5f) * float(U.width) - 0.5f);
            fy = float(px.y) - ((0.5f * ndc.y + 0.5f) * float(U.height) - 0.5f);
            const float* m = U.invView;
            const float A = ((m[0] * sn.x + m[1] * sn.y) + m[2] * sn.z) + m[3] * 0.0f;
            const float B = ((m[4] * sn.x + m[5] * sn.y) + m[6] * sn.z) + m[7] * 0.0f;
            fw = fabsf(A / sqrtf(1.0f - A * A)) + fabsf(B / sqrtf(1.0f - B * B));
        }
        SF.normalDepth[pix] = make_float4(sn.x, sn.y, sn.z, hasHit ? -pv.z : U.farDist);
        SF.flowFwidth[pix] = make_float4(fx, fy, fw, 0.0f);
    }
    // active-ray compaction: ballot + prefix popcount, one atomic per wave -- PER 64x64-PIXEL GROUP (all pixels of a wave
    // belong to one group): the G-buffer is segmented by group, slot = group * 4096 + position inside the group's segment,
    // and k_ao_rays walks the segments in group (= Morton tile) order.  The AO rays in flight at any moment then belong to two
    // or three neighbouring 64x64 groups instead of the ~50 groups whose workgroups of THIS kernel run concurrently, so
    // that their working set (the geometry within the AO radius of those groups) fits the L2s; with one global counter the
    // G-buffer order followed the interleaving of the running workgroups (L2 hit rate 88 % on the 64 MB capsule scene, 56 % on
    // the 1 GB triangle scene).
    const unsigned long long mask = __ballot(hasHit);
    if (mask) {
        const unsigned lane = lv_lane();
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&groupCount[px.group], unsigned(__popcll(mask)));
        base = __shfl(base, 0, 64);
        if (hasHit) {
            const size_t slot = lv_ao_group_base(lv_ao_layout(T), px.group) + base + unsigned(__popcll(mask & ((1ull << lane) - 1ull)));
            gbuf[3 * size_t(slot) + 0] = g0;
            gbuf[3 * size_t(slot) + 1] = g1;
            gbuf[3 * size_t(slot) + 2] = g2;
        }
    }
    lv_group_cost_add(T, px, tg0);
    if (STATS) lv_flush_counters(cnt, dc);
}

template <bool STATS, int PRIM>
__global__ __launch_bounds__(LV_BLOCK) void k_ao_primary(const LvUniforms U, const LvSceneDev S, const LvTiles T,
                                                         const float* aoIn, float* ao, float4* __restrict__ gbuf,
                                                         uint32_t* __restrict__ groupCount, LvDevCounters* dc,
                                                         const float4* featNormalIn, float4* featNormal,
                                                         const float4* featPositionIn, float4* featPosition,
                                                         const LvSvgfFeat SF) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    lv_ao_primary_body<STATS, PRIM>(U, S, T, blockIdx.x, s_stack, cm, aoIn, ao, gbuf, groupCount, dc, featNormalIn, featNormal, featPositionIn,
                                    featPosition, SF);
}

// The colour pass' ray of every pixel (sample 0: the pixel centre, or the jittered position of TubeRayTracing.glsl:236-262) against the
// capsules, through the transparency loop of traceRayTransparent (TubeRayTracing.glsl:61-82) for up to LV_PRE_HITS hits: which hits the
// loop visits depends on the alpha of the shaded hits, and alpha does not depend on the ambient occlusion (lv_compute_fragment_color_t:
// out.w = transfer function alpha x silhouette coverage) -- the hits are shaded here WITHOUT ambient occlusion, for their alpha and
// payload distance only.  firstHit[k * stride + px.outIndex] = {t bits, (leaf << 2) | kind}, LV_INVALID = miss;
// k_render_rt<..., PRE = true> shades them with the AO image after the RTAO pass.
template <bool STATS, int BANDS>
__device__ __forceinline__ void lv_colour_first_hits(const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t blockId,
                                                     unsigned* s_stack, LvCoopMem& cm, uint2* __restrict__ firstHit, size_t stride,
                                                     LvDevCounters* dc) {
    LvPixel px;
    if (!lv_block_pixel(U, T, px, blockId)) return;
    const unsigned long long tg0 = lv_group_clock();
    const LvStackMem sm = lv_stack_mem(s_stack, S.stackOverflow);
    LvCounters cnt = {0, 0, 0, 0};
    LvUniforms UA = U;            // the same shading without the AO term (S.ao is not there yet)
    UA.useAmbientOcclusion = 0u;
    UA.aoProjectLookup = 0u;
    float xix = 0.5f, xiy = 0.5f;
    if (U.useJitteredRays) {   // as k_render_rt, sampleIdx = 0
        uint32_t seed = U.useDeterministicSampling ? lv_tea(19u, U.frameNumber * U.numSamplesPerFrame)
                                                   : lv_tea(px.x + px.y * U.width, U.frameNumber * U.numSamplesPerFrame);
        xix = lv_rnd(seed);
        xiy = lv_rnd(seed);
    }
    f3 o, d;
    lv_primary_ray(U, px.x, px.y, xix, xiy, o, d);
    const bool capped = U.useCappedTubes != 0 || U.lssGeometry != 0;
    const float HIT_DISTANCE_EPSILON = 1e-5f;
    float tMin = 0.0001f, alpha = 0.0f;
    bool tracing = px.inView;
    for (uint32_t hitIdx = 0; hitIdx < LV_PRE_HITS && hitIdx < U.maxDepthComplexity && __any(tracing); hitIdx++) {
        const LvHit h = lv_trace_closest<STATS, false, LV_PRIM_CAPSULE>(S, U.radius, capped, tracing, o, d, tMin, 1000.0f, sm, cm, cnt);
        if (tracing) {
            firstHit[size_t(hitIdx) * stride + px.outIndex] =
                    h.found ? make_uint2(__float_as_uint(h.t), (h.leaf << 2) | uint32_t(h.kind)) : make_uint2(0u, LV_INVALID);
            if (!h.found) {
                tracing = false;
            } else {
                float payloadHitT;
                const f4 hc = lv_shade_hit<BANDS>(S, UA, 1.0f, o, d, h, payloadHitT);
                tMin = payloadHitT + fmaxf(payloadHitT * HIT_DISTANCE_EPSILON, 1e-7f);
                alpha = alpha + (1.0f - alpha) * hc.w;
                if (alpha > 0.99f) tracing = false;
            }
        }
    }
    lv_group_cost_add(T, px, tg0);
    if (STATS) { lv_flush_max_nodes(cnt, dc); lv_flush_counters(cnt, dc); }
}

// k_ao_primary and the colour pass' first-hit trace in ONE launch: workgroups [0, gridAo) trace the RTAO primaries (scene SA: the
// triangle tubes or the capsules, tiles TA), workgroups [gridAo, gridAo + gridColour) the colour rays (scene SC, tiles TC).  Both are
// latency-bound chains of dependent node fetches with one ray per lane; on a rank that owns 1/8 of the tiles neither fills the GPU
// (4 waves per SIMD), and run one after the other they were 0.44 of a 1.27-ms frame (profiles/shard_probe_r05_c3t.json).  Together
// their waves share the CUs and the two chains overlap.
template <bool STATS, int PRIM, int BANDS>
__global__ __launch_bounds__(LV_BLOCK) void k_primary_pair(const LvUniforms U, const LvSceneDev SA, const LvTiles TA, const uint32_t gridAo,
                                                           const float* aoIn, float* ao, float4* __restrict__ gbuf,
                                                           uint32_t* __restrict__ groupCount, LvDevCounters* dc,
                                                           const float4* featNormalIn, float4* featNormal,
                                                           const float4* featPositionIn, float4* featPosition,
                                                           const LvSvgfFeat SF, const LvSceneDev SC, const LvTiles TC,
                                                           uint2* __restrict__ firstHit, const size_t firstHitStride) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    if (blockIdx.x < gridAo)
        lv_ao_primary_body<STATS, PRIM>(U, SA, TA, blockIdx.x, s_stack, cm, aoIn, ao, gbuf, groupCount, dc, featNormalIn, featNormal,
                                        featPositionIn, featPosition, SF);
    else
        lv_colour_first_hits<STATS, BANDS>(U, SC, TC, blockIdx.x - gridAo, s_stack, cm, firstHit, firstHitStride, dc);
}

// exclusive prefix sum of the per-tile hit-pixel counts: tileBase[t] = first compacted-pixel ordinal of tile t,
// tileBase[numTiles] = dc->aoCount = all hit pixels of the launch (one workgroup; numTiles is a few hundred to a few thousand)
__global__ __launch_bounds__(LV_BLOCK) void k_ao_tile_scan(const uint32_t* __restrict__ tileCount, uint32_t numTiles,
                                                           uint32_t* __restrict__ tileBase, LvDevCounters* dc) {
    __shared__ uint32_t s_part[LV_BLOCK];
    const uint32_t per = (numTiles + LV_BLOCK - 1u) / LV_BLOCK;
    const uint32_t b = threadIdx.x * per, e = min(b + per, numTiles);
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; i++) sum += tileCount[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < LV_BLOCK; i++) { const uint32_t v = s_part[i]; s_part[i] = run; run += v; }
        tileBase[numTiles] = run;
        dc->aoCount = run;
        dc->aoQueueHead = 0ull; // the ray queue of the k_ao_rays launch that follows
    }
    __syncthreads();
    uint32_t run = s_part[threadIdx.x];
    for (uint32_t i = b; i < e; i++) { tileBase[i] = run; run += tileCount[i]; }
}

// Best hit of an AO ray in LDS, merged with one atomicMin per hit.  The AO value is t / aoRadius or 0 / 1: it never reads which
// primitive was hit, and the primitive index in a (t, primitive) key only orders hits of EQUAL t, which give equal output.  So the
// key is the bit pattern of t alone (t >= 0: the patterns order like the values); "no hit" is the pattern one above aoRadius's, which
// no accepted hit (t <= aoRadius) can reach, so a hit at exactly aoRadius still differs from a miss.  As a float that pattern is the
// next value above aoRadius: the culling interval of a ray without a hit is one ulp wider than aoRadius, which is conservative.
// The wave-cooperative routines of the tile kernels keep 64-bit keys: they return the primitive.
// LV_AO_KEY64=1 (measurement knob): the 64-bit key (t bits << 32 | primitive) of the earlier rounds.
#ifndef LV_AO_KEY64
#define LV_AO_KEY64 0
#endif
#if LV_AO_KEY64
typedef unsigned long long lv_ao_key;
__device__ __forceinline__ lv_ao_key lv_ao_key_none(float aoRadius) { return ((unsigned long long)__float_as_uint(aoRadius) << 32) | 0xFFFFFFFFull; }
__device__ __forceinline__ lv_ao_key lv_ao_key_hit(float t, unsigned low) { return ((unsigned long long)__float_as_uint(t) << 32) | low; }
__device__ __forceinline__ float lv_ao_key_t(lv_ao_key key) { return __uint_as_float(unsigned(key >> 32)); }
#else
typedef unsigned lv_ao_key;
__device__ __forceinline__ lv_ao_key lv_ao_key_none(float aoRadius) { return __float_as_uint(aoRadius) + 1u; }
__device__ __forceinline__ lv_ao_key lv_ao_key_hit(float t, unsigned) { return __float_as_uint(t); }
__device__ __forceinline__ float lv_ao_key_t(lv_ao_key key) { return __uint_as_float(key); }
#endif

// One AO sample ray from its pixel's G-buffer entry and its sample index (sampleHemisphere + the frame transform,
// VulkanRayTracedAmbientOcclusion.glsl:151-156,288-306): {o.xy}{o.z, d.x}{d.yz} into gen[0 .. 2].
template <bool BAKE>
__device__ __forceinline__ void lv_ao_generate_ray(const LvUniforms& U, float4 g0, float4 g1, float4 g2, uint32_t smpIdx, uint32_t spp,
                                                   const uint2* __restrict__ lcgSkip, float2* gen) {
    const uint32_t pix = __float_as_uint(g1.w);
    const f3 pos = mk3(g0.x, g0.y, g0.z), T = mk3(g1.x, g1.y, g1.z), N = mk3(g2.x, g2.y, g2.z);
    const f3 B = cross3(N, T);
    uint32_t seed;
    if (BAKE) {
        const uint32_t sub = __float_as_uint(g2.w);
        const uint2 skip = lcgSkip[2u * (sub * spp + smpIdx)];
        seed = skip.x * lv_tea(pix /* = vertex */, U.aoFrameNumber) + skip.y;
    } else {
        seed = lv_tea(pix, U.aoGlobalFrameNumber * spp + smpIdx);
    }
    const float xi0 = lv_rnd(seed), xi1 = lv_rnd(seed);
    float sn, cs;
    lv_sincos2pi(xi1, sn, cs); // sampleHemisphere, glsl:151-156
    const float rs = sqrtf(1.0f - xi0 * xi0);
    const f3 smp = mk3(cs * rs, sn * rs, xi0);
    const f3 dirU = mk3((T.x * smp.x + B.x * smp.y) + N.x * smp.z, (T.y * smp.x + B.y * smp.y) + N.y * smp.z,
                        (T.z * smp.x + B.z * smp.y) + N.z * smp.z);
    const f3 d = norm3(dirU);
    const f3 o = BAKE ? pos : pos + d * g0.w;
    gen[0] = make_float2(o.x, o.y);
    gen[1] = make_float2(o.z, d.x);
    gen[2] = make_float2(d.y, d.z);
}

// AO sample rays: PERSISTENT waves that keep three kinds of work apart and run each of them with (nearly) all
// 64 lanes busy.  AO ray r belongs to compacted pixel r / spp, sample r % spp.
//
//   generate  a wave takes LV_AO_CHUNK consecutive ray indices from the global queue head with one atomic and turns
//             them into rays 64 at a time -- TEA seed, hemisphere sample, frame transform, normalisation -- into an LDS
//             buffer (s_gen); idle lanes later pick a ready ray from there (two ds_read_b128), so the ~330-instruction
//             setup always runs at full width.
//   descend   a lane owns a ray only while it is alive; every lane with an inner node does one node step per
//             iteration (LDS-staged stack).  Leaves are NOT tested by the lane that meets them: (owner lane, leaf) is
//             appended to a wave-local FIFO in LDS (ballot + prefix popcount, no atomics).
//   test      as soon as 64 pairs wait, all 64 lanes take one pair each, read the owner's ray from LDS, run the
//             capsule test (8 IEEE divisions + 4 square roots, ~350 instructions) and merge into the owner's best hit
//             with one 32-bit LDS atomicMin on the bits of t (lv_ao_key: AO never reads the primitive).  The leaf test is the expensive phase; with one ray per thread it ran at
//             17-27 % lane utilisation (measured), here at ~100 %.
// A finished ray is retired (samples[r] written, lane idle) once the FIFO head has passed its last queued leaf.
// Scheduling inside a wave: test when >= 64 pairs wait; refill when >= LV_REFILL_THRESHOLD lanes are idle; otherwise
// descend; flush partial batches only when nothing else can make progress.  Once the global queue is empty (drain) the
// rays left in a wave are finished together: nobody retires early, idle lanes take over stacked subtrees of busy ones.
// All wave-level state (queue chunk, s_gen window, FIFO head / tail, the decisions above) derives from ballots, kernel arguments
// and readfirstlane, so the compiler keeps it in scalar registers and takes the decisions with scalar branches (LV_AO_SCALAR_STATE).
// Resources: 31 KB LDS and <= 96 VGPRs -> 5 workgroups = 20 waves per CU; the kernel is VALU-issue-bound and needs that
// occupancy to hide the dependent node fetches (12 -> 16 -> 20 waves per CU: -16 %, -7 %).
// BAKE: the static prebaker's rays (VulkanAmbientOcclusionBaker.glsl:230-281).  G-buffer slot = parametrisation vertex *
// numTubeSubdivisions + subdivision with g0 = {ray origin, -}, g1 = {tangent, vertex}, g2 = {surface normal, subdivision};
// the reference draws the (subdivision, ray) samples of a vertex from ONE LCG stream seeded with tea(vertex, frame), so
// sample j starts from the stream advanced by 2 j steps: seed_j = A_j * seed_0 + C_j (lcgSkip[j] = {A_j, C_j}).
// PIXEL_GEN (host: spp % 64 == 0, not BAKE, ao_ray_generation = per_pixel): the generate phase looks its pixel up once per batch on
// scalar registers instead of once per lane; same rays, same order, same scheduling.
template <bool STATS, bool ANY_HIT, int PRIM, bool BAKE = false, bool LIT = false, bool PIXEL_GEN = false>
__global__ __launch_bounds__(LV_AO_BLOCK, LV_AO_MIN_WAVES) void k_ao_rays(const LvUniforms U, const LvSceneDev S,
                                                         const float4* __restrict__ gbuf, float* __restrict__ samples,
                                                         LvDevCounters* dc, const uint32_t* __restrict__ tileBase,
                                                         uint32_t numTiles, const LvAoLayout tileCapacity,
                                                         const uint2* __restrict__ lcgSkip = nullptr) {
    __shared__ unsigned s_stack[LV_AO_STACK_LDS * LV_AO_BLOCK];
    // LDS budget: 16 KB + 6 + 6 + 2 + 1 = 31 KB per workgroup -> 5 workgroups (20 waves) per CU; the kernel hides the
    // latency of its dependent node fetches with occupancy (measured: 12 -> 16 waves/CU -16 %, 16 -> 20 another -7 %)
    __shared__ float2 s_ray[3 * LV_AO_BLOCK];              // current ray of every lane: {o.xy}{o.z, d.x}{d.yz} (24 B)
    __shared__ float2 s_gen[3 * LV_AO_BLOCK];              // generated rays waiting for a lane
    __shared__ unsigned s_queue[LV_AO_BLOCK / LV_WAVE][LV_AO_QCAP];
    __shared__ lv_ao_key s_key[LV_AO_BLOCK];               // best hit of every lane's ray
    __shared__ uint4 s_genState[PIXEL_GEN ? LV_AO_BLOCK / LV_WAVE : 1]; // PIXEL_GEN: {genLo, genHi, genSlot0, -} of every wave (generate phase)

    const uint32_t spp = U.aoSamplesPerFrame;
    const unsigned long long total = (unsigned long long)(dc->aoCount) * spp;
    // rays a wave takes from the global queue per atomic: LV_AO_CHUNK, or half of it when the launch holds fewer than LV_AO_SMALL_CHUNKS
    // such chunks per persistent wave (a rank that owns 1/8 of the tiles: ~4 chunks of 128 per wave -- the last chunk of the slowest
    // wave is then a quarter of the kernel)
    const unsigned chunk = total < (unsigned long long)gridDim.x * (LV_AO_BLOCK / LV_WAVE) * LV_AO_CHUNK * LV_AO_SMALL_CHUNKS ? LV_AO_CHUNK_SMALL
                                                                                                                             : LV_AO_CHUNK;
    const bool capped = U.useCappedTubes != 0;
    const float radius = U.radius;
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    float2* rayW = &s_ray[3 * LV_WAVE * w];
    float2* genW = &s_gen[3 * LV_WAVE * w];
    unsigned* queueW = s_queue[w];
    lv_ao_key* keyW = &s_key[LV_WAVE * w];
    uint4* genStateW = &s_genState[PIXEL_GEN ? w : 0];
    if (PIXEL_GEN && lane == 0) genStateW[0] = make_uint4(0u, 0u, 0u, 0u);
    const lv_ao_key keyInit = lv_ao_key_none(U.aoRadius);
    // literal roots: cull against best + r / |d| (AO directions are normalised: |d| = 1 to rounding, 1.001 covers it)
    // elliptic tubelets: bandWidth / |d| (lv_intersect_elliptic_tube's own-box rule)
    const float litSlack = PRIM == LV_PRIM_ELLIPTIC ? S.ellBandWidth * 1.001f : (PRIM == LV_PRIM_CAPSULE && LIT) ? radius * 1.001f : 0.0f;

    LvStackT<LV_AO_STACK_LDS, LV_AO_BLOCK> st;
    st.init(s_stack, S.stackOverflow);
    LvCounters cnt = {0, 0, 0, 0};
    unsigned long long phIt[3] = {0, 0, 0}, phLn[3] = {0, 0, 0};
    unsigned long long mayAxis = 0, mayBoth = 0, primHits = 0;

    // wave-uniform state
    unsigned long long chunkNext = 0, chunkEnd = 0, genBase = 0;
    unsigned genCount = 0, genPos = 0;      // rays in s_gen: [genPos, genCount)
    unsigned head = 0, tail = 0;            // leaf FIFO (absolute sequence numbers)
    bool sourceDry = (S.numSegs == 0) || (total == 0);
    // lane state
    bool hasRay = false, enq = false;
    unsigned long long r = 0;
    f3 inv = mk3(0, 0, 0), oi = mk3(0, 0, 0);
    float tHi = 0.0f; // upper end of the node steps' slab interval: the ray's best hit (or aoRadius) + litSlack, summed where the hit changes
    unsigned cur = LV_INVALID, lastSeq = 0;
    unsigned owner = lane; // lane whose ray this lane descends for: its own, except in the drain phase (below)
    // queued (owner, leaf) pairs that start a test phase: a little less than a full wave -- the stint ends sooner for the lanes whose
    // ray is finished and waits for it, at the price of test phases that run at 56 / 64 (LV_AO_TEST_BATCH*, measured)
    constexpr unsigned TB = PRIM == LV_PRIM_TRIANGLE ? LV_AO_TEST_BATCH_TRI : LV_AO_TEST_BATCH;

    while (true) {
        // ---- leaves reached in the previous step join the FIFO -- while fewer than 64 pairs wait, so that it never holds
        // more than 63 + 64 (LV_AO_QCAP = 128); with a full batch waiting the test phase below runs first
        {
            const bool isLeaf = tail - head < LV_WAVE && cur != LV_INVALID && (cur & LV_LEAF_BIT);
            const unsigned long long mL = __ballot(isLeaf);
            if (mL) {
                if (isLeaf) {
                    const unsigned idx = tail + unsigned(__popcll(mL & below));
                    queueW[idx % LV_AO_QCAP] = (owner << LV_REF_BITS) | (cur & LV_REF_MASK);
                    lastSeq = idx;
                    enq = true;
                    cur = lv_pop_or_done(st);
                }
                tail += unsigned(__popcll(mL));
                if (tail - head < TB) continue; // a popped reference may be a leaf again
            }
        }
        const bool canRefill = (genPos < genCount) || !sourceDry;
        // DRAIN phase: no ray is left to hand out.  What remains in the wave is finished together, like one call of
        // lv_trace_closest: nobody retires early, lanes without work take over stacked subtrees of the lanes that still
        // descend (for THEIR rays: hits merge into the owner's key), and all samples are written at the end.  Without
        // it the kernel's last ~0.3 ms were a handful of lanes per wave walking their long rays alone -- a fixed cost that
        // weighs more the fewer tiles a GPU owns.
        const bool drain = !canRefill;
        // ---- retire rays whose traversal is finished and whose queued leaves have all been tested
        if (!drain && hasRay && cur == LV_INVALID && (!enq || int(head - lastSeq) > 0)) {
            const lv_ao_key key = keyW[lane];
            float occ = 1.0f;
            if (key != keyInit) occ = U.aoUseDistance ? lv_ao_key_t(key) / U.aoRadius : 0.0f;
            samples[r] = occ;
            hasRay = false;
        }
        const unsigned long long mNode = __ballot(cur != LV_INVALID && !(cur & LV_LEAF_BIT));
        const unsigned long long mIdle = __ballot(!hasRay);
        const int nNode = __popcll(mNode), nIdle = __popcll(mIdle);
        const unsigned q = tail - head;

        if (q >= TB || (q > 0 && nNode == 0 && !(canRefill && nIdle > 0))) {
            // ---- test phase: one (owner, leaf) pair per lane
            const unsigned n = q < LV_WAVE ? q : LV_WAVE;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (STATS && lane == 0) { phIt[2]++; phLn[2] += n; }
            if (lane < n) {
                const unsigned e = queueW[(head + lane) % LV_AO_QCAP];
                const unsigned owner = e >> LV_REF_BITS, leaf = e & LV_REF_MASK;
                const float2 r0 = rayW[3 * owner], r1 = rayW[3 * owner + 1], r2 = rayW[3 * owner + 2];
                if (STATS) cnt.prims += PRIM == LV_PRIM_TRIANGLE ? S.triLeafSize : 1u; // primitives tested
                float t; unsigned low;
                if (lv_leaf_test<PRIM, LIT ? 1 : 0, !STATS>(S, leaf, mk3(r0.x, r0.y, r1.x), mk3(r1.y, r2.x, r2.y), radius, capped, t, low, 0.0f,
                                                    U.aoRadius)) {
                    if (t >= 0.0f && t <= U.aoRadius) { // traceAoRay: closest hit in [0, aoRadius], glsl:158-175
                        atomicMin(&keyW[owner], lv_ao_key_hit(t, low));
                        if (STATS) primHits++;
                    }
                }
                if (STATS && PRIM == LV_PRIM_CAPSULE) {
                    const float4 sa = S.segs[2 * size_t(leaf)], sb = S.segs[2 * size_t(leaf) + 1];
                    const f3 ro = mk3(r0.x, r0.y, r1.x), rd = mk3(r1.y, r2.x, r2.y);
                    const bool ma = lv_capsule_may_hit_axis(ro, rd, mk3(sa.x, sa.y, sa.z), mk3(sb.x, sb.y, sb.z), radius);
                    const bool mb = lv_capsule_may_hit_sphere(ro, rd, mk3(sa.x, sa.y, sa.z), mk3(sb.x, sb.y, sb.z), radius);
                    mayAxis += ma ? 1u : 0u;
                    mayBoth += (ma && mb) ? 1u : 0u;
                }
            }
            head += n;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            {
                const lv_ao_key key = keyW[owner];
                tHi = lv_ao_key_t(key) + litSlack; // shrinks the slab interval of the following node steps
                if (ANY_HIT && key != keyInit) { cur = LV_INVALID; st.clear(); }
            }
            continue;
        }
        if (drain) {
            if (nNode == 0) { // FIFO empty (q == 0 here), nobody descends: the wave is done
                if (hasRay) {
                    const lv_ao_key key = keyW[lane];
                    float occ = 1.0f;
                    if (key != keyInit) occ = U.aoUseDistance ? lv_ao_key_t(key) / U.aoRadius : 0.0f;
                    samples[r] = occ;
                }
                break;
            }
            if (nNode <= LV_HANDOVER_MAX_BUSY) { // subtree hand-over, as in lv_trace_closest (exchange slots: the idle s_gen)
                const bool idle = cur == LV_INVALID;
                const bool donor = !idle && st.has_entries();
                const unsigned long long mFree = __ballot(idle), mDonor = __ballot(donor);
                const unsigned nPairs = min(unsigned(__popcll(mFree)), unsigned(__popcll(mDonor)));
                if (nPairs) {
                    if (donor) {
                        const unsigned rk = unsigned(__popcll(mDonor & below));
                        if (rk < nPairs) genW[rk] = make_float2(__uint_as_float(st.pop()), __uint_as_float(owner));
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (idle) {
                        const unsigned rk = unsigned(__popcll(mFree & below));
                        if (rk < nPairs) {
                            const float2 x = genW[rk];
                            cur = __float_as_uint(x.x);
                            owner = __float_as_uint(x.y);
                            const float2 r0 = rayW[3 * owner], r1 = rayW[3 * owner + 1], r2 = rayW[3 * owner + 2];
                            inv = lv_traversal_inv(mk3(r1.y, r2.x, r2.y));
                            oi = mk3(r0.x * inv.x, r0.y * inv.y, r1.x * inv.z);
                            tHi = lv_ao_key_t(keyW[owner]) + litSlack;
                            st.clear();
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    continue; // the reference taken over may be a leaf
                }
            }
        }
        if (canRefill && nIdle > 0 && (nIdle >= LV_REFILL_THRESHOLD || nNode < LV_NODE_MIN_ACTIVE)) {
            // ---- generate phase: keep s_gen stocked (all 64 lanes), then hand rays to the idle lanes
            if (genPos >= genCount) {
                if (chunkNext >= chunkEnd) {
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(&dc->aoQueueHead, (unsigned long long)chunk);
#if LV_AO_SCALAR_STATE
                    // lane 0's value through readfirstlane, which the compiler knows to be wave-uniform: everything derived from it
                    // (sourceDry, canRefill, drain, genCount, genPos, head, tail and the loop's decisions) then is provably uniform too --
                    // scalar registers and scalar branches.  Through __shfl it counts as divergent, and with it the whole main loop:
                    // counters in vector registers, decisions as lane masks, a dozen vector copies on every trip round the loop.
                    chunkNext = (unsigned long long)__builtin_amdgcn_readfirstlane(unsigned(base)) |
                                ((unsigned long long)__builtin_amdgcn_readfirstlane(unsigned(base >> 32)) << 32);
#else
                    chunkNext = __shfl(base, 0, 64);
#endif
                    chunkEnd = chunkNext + chunk;
                    if (chunkEnd > total) chunkEnd = total;
                    if (chunkNext >= total) { chunkNext = chunkEnd = total; sourceDry = true; }
                }
                const unsigned long long left = chunkEnd - chunkNext;
                const unsigned n = left < LV_WAVE ? unsigned(left) : LV_WAVE;
                if (STATS && lane == 0 && n) { phIt[0]++; phLn[0] += n; }
                if (PIXEL_GEN) {
                    // spp is a multiple of 64 and so is every chunk start: the 64 rays of this batch are samples [genSmp0, genSmp0 + 64) of
                    // ONE pixel.  Its ordinal, its group and its G-buffer slot are wave-uniform (scalar registers, scalar loads); per lane
                    // only the sample index differs.  The same integers and the same float operations as below: the same rays, bit for bit.
                    if (n) {
                        // batch number -> (pixel ordinal, first sample): 32 bits (the host checks the launch's size), no division at spp = 64
                        const uint32_t b = __builtin_amdgcn_readfirstlane(uint32_t(chunkNext / LV_WAVE)), bpp = spp / LV_WAVE;
                        const uint32_t genOrdinal = bpp == 1u ? b : __builtin_amdgcn_readfirstlane(b / bpp);
                        const uint32_t genSmp0 = (b - genOrdinal * bpp) * LV_WAVE;
                        // the group the wave's previous batch was found in: its ordinals [genLo, genHi) and its first G-buffer slot.  Kept in
                        // LDS, not in registers: the kernel has no scalar register to spare across its main loop
                        const uint4 gs = genStateW[0];
                        uint32_t genLo = __builtin_amdgcn_readfirstlane(gs.x), genHi = __builtin_amdgcn_readfirstlane(gs.y);
                        uint32_t genSlot0 = __builtin_amdgcn_readfirstlane(gs.z);
                        if (genOrdinal - genLo >= genHi - genLo) { // left that group (or the first batch: 0 >= 0)
                            uint32_t lo = 0, hi = numTiles;        // lv_ao_slot's search, once per group a wave passes through
                            while (hi - lo > 1u) {
                                const uint32_t mid = (lo + hi) >> 1;
                                if (tileBase[mid] <= genOrdinal) lo = mid; else hi = mid;
                            }
                            genLo = __builtin_amdgcn_readfirstlane(tileBase[lo]);
                            genHi = __builtin_amdgcn_readfirstlane(tileBase[lo + 1u]);
                            genSlot0 = __builtin_amdgcn_readfirstlane(uint32_t(lv_ao_group_base(tileCapacity, lo)));
                            if (lane == 0) genStateW[0] = make_uint4(genLo, genHi, genSlot0, 0u);
                        }
                        const size_t slot = size_t(genSlot0) + (genOrdinal - genLo);
                        const float4 g0 = gbuf[3 * slot + 0], g1 = gbuf[3 * slot + 1], g2 = gbuf[3 * slot + 2];
                        lv_ao_generate_ray<false>(U, g0, g1, g2, genSmp0 + lane, spp, lcgSkip, &genW[3 * lane]);
                    }
                } else if (lane < n) {
                    const unsigned long long rr = chunkNext + lane;
                    const uint32_t smpIdx = uint32_t(rr % spp);
                    const size_t slot = lv_ao_slot(tileBase, numTiles, tileCapacity, uint32_t(rr / spp));
                    const float4 g0 = gbuf[3 * slot + 0], g1 = gbuf[3 * slot + 1], g2 = gbuf[3 * slot + 2];
                    lv_ao_generate_ray<BAKE>(U, g0, g1, g2, smpIdx, spp, lcgSkip, &genW[3 * lane]);
                }
                genBase = chunkNext;
                chunkNext += n;
                genCount = n;
                genPos = 0;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            const unsigned avail = genCount - genPos;
            const unsigned k = unsigned(nIdle) < avail ? unsigned(nIdle) : avail;
            if (!hasRay) {
                const unsigned rank = unsigned(__popcll(mIdle & below));
                if (rank < k) {
                    const unsigned gs = genPos + rank;
                    const float2 r0 = genW[3 * gs], r1 = genW[3 * gs + 1], r2 = genW[3 * gs + 2];
                    rayW[3 * lane] = r0;
                    rayW[3 * lane + 1] = r1;
                    rayW[3 * lane + 2] = r2;
                    keyW[lane] = keyInit;
                    inv = lv_traversal_inv(mk3(r1.y, r2.x, r2.y));
                    oi = mk3(r0.x * inv.x, r0.y * inv.y, r1.x * inv.z);
                    tHi = U.aoRadius + litSlack;
                    r = genBase + gs;
                    owner = lane;
                    cur = 0;
                    st.clear();
                    enq = false;
                    hasRay = true;
                    if (STATS) cnt.rays++;
                }
            }
            genPos += k;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            continue;
        }
        if (nNode > 0) {
            // ---- descend phase: tight loop of node steps; leaves met on the way join the FIFO.  Leave it only when a
            // full batch of leaf tests waits or nobody descends any more (leaving earlier for a retire/refill pass
            // was measured slower: the per-pass bookkeeping outweighs the idle lanes).
            int nNow;
            do {
                if (STATS && lane == 0) { phIt[1]++; }
                if (STATS && !(cur & LV_LEAF_BIT)) phLn[1]++;
                if (!(cur & LV_LEAF_BIT)) cur = lv_node_step<STATS>(S, cur, oi, inv, 0.0f - litSlack, tHi, st, cnt);
                const bool isLeaf = cur != LV_INVALID && (cur & LV_LEAF_BIT);
                const unsigned long long mL = __ballot(isLeaf);
                if (mL) {
                    if (isLeaf) {
                        const unsigned idx = tail + unsigned(__popcll(mL & below));
                        queueW[idx % LV_AO_QCAP] = (owner << LV_REF_BITS) | (cur & LV_REF_MASK);
                        lastSeq = idx;
                        enq = true;
                        cur = lv_pop_or_done(st);
                    }
                    tail += unsigned(__popcll(mL));
                }
                nNow = __popcll(__ballot(!(cur & LV_LEAF_BIT)));
            } while (tail - head < TB && nNow >= (drain ? LV_HANDOVER_MAX_BUSY + 1 : 1));
            continue;
        }
        if (nIdle == LV_WAVE && !canRefill) break; // nothing alive, nothing left to fetch
    }
    if (STATS) {
        lv_flush_counters(cnt, dc, true);
        for (int k = 0; k < 3; k++) {
            const unsigned long long it = lv_wave_sum_u64(phIt[k]), ln = lv_wave_sum_u64(phLn[k]);
            if (lane == 0) { atomicAdd(&dc->aoPhaseIters[k], it); atomicAdd(&dc->aoPhaseLanes[k], ln); }
        }
        const unsigned long long sa = lv_wave_sum_u64(mayAxis), sb = lv_wave_sum_u64(mayBoth), sh = lv_wave_sum_u64(primHits);
        if (lane == 0) { atomicAdd(&dc->aoPrimMayAxis, sa); atomicAdd(&dc->aoPrimMayBoth, sb); atomicAdd(&dc->aoPrimHits, sh); }
    }
}

template <bool BAKE>
__global__ __launch_bounds__(LV_BLOCK) void k_ao_reduce(const LvUniforms U, const float4* __restrict__ gbuf,
                                                        const float* __restrict__ samples, const float* aoIn, float* ao,
                                                        const LvDevCounters* dc, const uint32_t* __restrict__ tileBase,
                                                        uint32_t numTiles, const LvAoLayout tileCapacity) {
    const uint32_t slot = blockIdx.x * LV_BLOCK + threadIdx.x; // compacted-pixel ordinal (= row of `samples`)
    if (slot >= dc->aoCount) return;
    const uint32_t spp = U.aoSamplesPerFrame;
    float aoFactor = 0.0f; // summed strictly in sample order, like the reference's loop (glsl:288-306)
    if ((spp & 3u) == 0u) {
        // 16-byte loads: the lanes of a wave read rows that are spp * 4 bytes apart, so every load instruction touches
        // 64 different cache lines whatever its width -- dwordx4 quarters the number of L1 accesses
        const float4* row = reinterpret_cast<const float4*>(samples + size_t(slot) * spp);
        for (uint32_t s = 0; s < spp / 4u; s++) {
            const float4 v = row[s];
            aoFactor += v.x; aoFactor += v.y; aoFactor += v.z; aoFactor += v.w;
        }
    } else {
        for (uint32_t s = 0; s < spp; s++) aoFactor += samples[size_t(slot) * spp + s];
    }
    aoFactor /= float(spp);
    // screen space: the pixel of the compacted slot; prebaker: ambientOcclusionFactors[subdiv + N * vertex] = the slot
    const uint32_t pix = BAKE ? slot : __float_as_uint(gbuf[3 * lv_ao_slot(tileBase, numTiles, tileCapacity, slot) + 1].w);
    // aoIn == ao except where tiles overlap (the 1-pixel rings of a halo, a tile listed twice): a pixel may then be processed twice
    // in one pass, and the running mean must read the PREVIOUS pass' image to stay idempotent (lv_run_ao)
    if (U.aoFrameNumber != 0) aoFactor = mixf(aoIn[pix], aoFactor, 1.0f / float(U.aoFrameNumber + 1));
    ao[pix] = aoFactor;
}

// The same reduction with coalesced loads (spp a multiple of 4): a workgroup of 128 threads owns 128 consecutive rows of
// `samples`; per chunk of 64 samples the rows' 256-byte pieces are copied into LDS (16 lanes per row, one float4 each) with a row
// pitch of 65 floats (conflict-free column walks), then every thread adds ITS row's chunk in sample order into its accumulator --
// the same sequence of additions as the loop above, so the same bits.  (k_ao_reduce reads every row 16 B at a time with one
// cache line per lane: 75 us for config 3's 91 MB, against 91 MB / HBM rate.)  Persistent: blocks stride over dc->aoCount.
#define LV_REDUCE_ROWS 128u
__global__ __launch_bounds__(LV_REDUCE_ROWS) void k_ao_reduce_rows(const LvUniforms U, const float4* __restrict__ gbuf,
                                                                   const float* __restrict__ samples, const float* aoIn, float* ao,
                                                                   const LvDevCounters* dc, const uint32_t* __restrict__ tileBase,
                                                                   uint32_t numTiles, const LvAoLayout tileCapacity) {
    __shared__ float s_rows[LV_REDUCE_ROWS * 65u];
    const uint32_t count = dc->aoCount, spp = U.aoSamplesPerFrame, t = threadIdx.x;
    for (uint32_t row0 = blockIdx.x * LV_REDUCE_ROWS; row0 < count; row0 += gridDim.x * LV_REDUCE_ROWS) {
        const uint32_t rows = min(LV_REDUCE_ROWS, count - row0);
        float aoFactor = 0.0f;
        for (uint32_t c0 = 0; c0 < spp; c0 += 64u) {
            const uint32_t cols4 = min(64u, spp - c0) / 4u; // float4s per row in this chunk
            __syncthreads();
            for (uint32_t idx = t; idx < rows * cols4; idx += LV_REDUCE_ROWS) {
                const uint32_t r = idx / cols4, c4 = idx % cols4;
                const float4 v = *reinterpret_cast<const float4*>(samples + size_t(row0 + r) * spp + c0 + 4u * c4);
                float* d = s_rows + r * 65u + 4u * c4;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            __syncthreads();
            if (t < rows)
                for (uint32_t j = 0; j < 4u * cols4; j++) aoFactor += s_rows[t * 65u + j];
        }
        if (t < rows) {
            const uint32_t slot = row0 + t;
            aoFactor /= float(spp);
            const uint32_t pix = __float_as_uint(gbuf[3 * lv_ao_slot(tileBase, numTiles, tileCapacity, slot) + 1].w);
            if (U.aoFrameNumber != 0) aoFactor = mixf(aoIn[pix], aoFactor, 1.0f / float(U.aoFrameNumber + 1));
            ao[pix] = aoFactor;
        }
    }
}

// One a-trous pass of the EAW denoiser (EAWDenoise.glsl) over the AO image: colorTexture = vec4(ao, ao, ao, 1) -- the three
// colour channels stay equal and alpha stays 1 through every pass, so one float per pixel carries the image.
//   COMPUTE = true   EAWDenoise.Compute (:128-292; eaw_denoiser_use_shared_memory = true, the default): B-spline kernel
//                    {1, 2/3, 1/6}, neighbours outside the image skipped, ONE exp of the summed exponents, colour term x step width
//   COMPUTE = false  EAWDenoise.Fragment (:16-126): Gaussian kernel, clamp-to-edge sampling, min(exp(.), 1) per enabled feature
// One thread per pixel of the (dilated) tiles; "inside" refers to the whole viewport, so tiles reproduce the full frame.
struct LvEawParams {
    float phiColor, phiPosition, phiNormal;
    uint32_t useColor, usePosition, useNormal;
    int stepWidth;
};
template <bool COMPUTE>
__global__ __launch_bounds__(LV_BLOCK) void k_eaw_pass(const LvUniforms U, const LvTiles T, const LvEawParams E,
                                                       const float* __restrict__ src, float* __restrict__ dst,
                                                       const float4* __restrict__ featNormal,
                                                       const float4* __restrict__ featPosition) {
    const uint32_t perTile = T.tileW * T.tileH;
    const uint64_t gid = uint64_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (gid >= uint64_t(T.numTiles) * perTile) return;
    const uint32_t tile = uint32_t(gid / perTile), rem = uint32_t(gid % perTile);
    const uint32_t gxu = T.tilesXY[2 * tile] + rem % T.tileW, gyu = T.tilesXY[2 * tile + 1] + rem / T.tileW;
    if (gxu >= U.width || gyu >= U.height) return;
    const int gx = int(gxu), gy = int(gyu), W = int(U.width), H = int(U.height);
    const size_t ci = size_t(gy) * U.width + gx;
    const float centerColor = src[ci];
    const float4 cP = E.usePosition ? featPosition[ci] : make_float4(0, 0, 0, 0);
    const float4 cN = E.useNormal ? featNormal[ci] : make_float4(0, 0, 0, 0);
    auto dist4 = [](float4 a, float4 b) {
        const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
        return ((dx * dx + dy * dy) + dz * dz) + dw * dw;
    };
    float sum, accumW;
    if (COMPUTE) {
        const float kernelValues[3] = {1.0f, 2.0f / 3.0f, 1.0f / 6.0f};
        accumW = kernelValues[0] * kernelValues[0];
        sum = centerColor * accumW;
        for (int y = -2; y <= 2; ++y) {
            for (int x = -2; x <= 2; ++x) {
                const int ox = gx + x * E.stepWidth, oy = gy + y * E.stepWidth;
                const bool inside = ox >= 0 && oy >= 0 && ox < W && oy < H;
                if (!inside || (x == 0 && y == 0)) continue;
                const size_t oi = size_t(oy) * U.width + ox;
                const float kernelValue = kernelValues[x < 0 ? -x : x] * kernelValues[y < 0 ? -y : y];
                const float offsetColor = src[oi];
                float e = 0.0f;
                if (E.useColor) {
                    const float d = centerColor - offsetColor;
                    const float distColor = ((d * d + d * d) + d * d) + 0.0f * 0.0f;
                    e = e - (distColor * float(E.stepWidth)) / E.phiColor;
                }
                if (E.usePosition) e = e - dist4(cP, featPosition[oi]) / E.phiPosition;
                if (E.useNormal) e = e - dist4(cN, featNormal[oi]) / E.phiNormal;
                const float weight = expf(e);
                sum += (offsetColor * weight) * kernelValue;
                accumW += weight * kernelValue;
            }
        }
    } else {
        sum = 0.0f; accumW = 0.0f;
        for (int i = 0; i < 25; i++) {
            const float x = float(i % 5 - 2), y = float(i / 5 - 2);
            const float kernelValue = expf(-(x * x + y * y) / 2.0f);
            const int ox = min(max(gx + (i % 5 - 2) * E.stepWidth, 0), W - 1);
            const int oy = min(max(gy + (i / 5 - 2) * E.stepWidth, 0), H - 1);
            const size_t oi = size_t(oy) * U.width + ox;
            const float offsetColor = src[oi];
            float weight = 1.0f;
            if (E.useColor) {
                const float d = centerColor - offsetColor;
                const float distColor = ((d * d + d * d) + d * d) + 0.0f * 0.0f;
                weight *= fminf(expf(-distColor / E.phiColor), 1.0f);
            }
            if (E.usePosition) weight *= fminf(expf(-dist4(cP, featPosition[oi]) / E.phiPosition), 1.0f);
            if (E.useNormal) weight *= fminf(expf(-dist4(cN, featNormal[oi]) / E.phiNormal), 1.0f);
            sum += (offsetColor * weight) * kernelValue;
            accumW += weight * kernelValue;
        }
    }
    dst[ci] = sum / accumW;
}

// VulkanAmbientOcclusionBaker.glsl:110-131,231-262: interpolated line point of every parametrisation vertex and the ray
// origin / frame of each of its tube subdivisions, written in the G-buffer format of k_ao_rays.
__global__ __launch_bounds__(LV_BLOCK) void k_bake_setup(const lv_line_point* __restrict__ linePoints, uint32_t numLinePoints,
                                                         const float* __restrict__ samplingLocations,
                                                         uint32_t numParametrizationVertices, uint32_t numTubeSubdivisions,
                                                         float lineRadius, float4* __restrict__ gbuf, uint32_t useBands,
                                                         float bandRadius, float minBandThickness) {
    const uint32_t slot = blockIdx.x * LV_BLOCK + threadIdx.x;
    if (slot >= numParametrizationVertices * numTubeSubdivisions) return;
    const uint32_t vertex = slot / numTubeSubdivisions, sub = slot % numTubeSubdivisions;
    const float samplingLocation = samplingLocations[vertex];
    const uint32_t lowerIdx = uint32_t(samplingLocation);
    const uint32_t upperIdx = min(lowerIdx + 1u, numLinePoints - 1u);
    const float f = samplingLocation - floorf(samplingLocation);
    const lv_line_point& lo = linePoints[lowerIdx];
    const lv_line_point& up = linePoints[upperIdx];
    auto ld = [](const float* p) { return mk3(p[0], p[1], p[2]); };
    auto mix3 = [&](f3 a, f3 b) { return mk3(mixf(a.x, b.x, f), mixf(a.y, b.y, f), mixf(a.z, b.z, f)); };
    const f3 binormalLower = cross3(ld(lo.lineTangent), ld(lo.lineNormal));
    const f3 binormalUpper = cross3(ld(up.lineTangent), ld(up.lineNormal));
    const f3 position = mix3(ld(lo.linePosition), ld(up.linePosition));
    const f3 tangent = norm3(mix3(ld(lo.lineTangent), ld(up.lineTangent)));
    const f3 normal = norm3(mix3(ld(lo.lineNormal), ld(up.lineNormal)));
    const f3 binormal = norm3(mix3(binormalLower, binormalUpper));
    float sinAngle, cosAngle;
    lv_sincos2pi(float(sub) / float(numTubeSubdivisions), sinAngle, cosAngle);
    f3 surfaceNormal = cosAngle * normal + sinAngle * binormal;
    f3 rayOrigin = position + (lineRadius + 1e-6f) * surfaceNormal;
    if (useBands) {   // USE_BANDS, "bands with minimum thickness" (glsl:233-256): elliptic cross-section, pushed out by 1e-3
        surfaceNormal = norm3(cosAngle * normal + (minBandThickness * sinAngle) * binormal);
        rayOrigin = position + (bandRadius + 1e-3f) * ((minBandThickness * cosAngle) * normal + sinAngle * binormal);
    }
    gbuf[3 * size_t(slot) + 0] = make_float4(rayOrigin.x, rayOrigin.y, rayOrigin.z, 0.0f);
    gbuf[3 * size_t(slot) + 1] = make_float4(tangent.x, tangent.y, tangent.z, __uint_as_float(vertex));
    gbuf[3 * size_t(slot) + 2] = make_float4(surfaceNormal.x, surfaceNormal.y, surfaceNormal.z, __uint_as_float(sub));
}

// ================================================================ PPLL
// The ray interval [tMin, tMax] of every pixel is cut into numSlices depth slices (boundaries spread evenly over the
// ray's passage through the scene box); workgroup = (16x16 pixel block, slice).  All-hits traversal cannot cull, so the
// slices cost no extra traversal, but a wave in front of the dense core of a data set -- hundreds of fragments per pixel,
// each one shaded -- no longer forms a multi-millisecond critical path while the rest of the GPU idles: its work is spread
// over numSlices workgroups.  A slice accepts t in [lo, hi) (the last one up to tMax inclusive), so every fragment is
// produced exactly once; each workgroup builds partial lists in LDS and splices them into the pixel's global list.
template <bool STATS, int PRIM = LV_PRIM_CAPSULE, int BANDS = LV_SHADE_PLAIN>
__global__ __launch_bounds__(LV_BLOCK, PRIM == LV_PRIM_PRISM ? LV_PRISM_MIN_WAVES : LV_GATHER_MIN_WAVES) void k_ppll_gather(const LvUniforms U, const LvSceneDev S, const LvTiles T,
                                                          uint32_t* __restrict__ nodes, uint32_t* __restrict__ startOffset,
                                                          uint32_t* __restrict__ fragCount, LvDevCounters* dc,
                                                          uint32_t numSlices, uint32_t poolSlots) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    __shared__ uint32_t s_head[LV_BLOCK];  // head of this workgroup's partial list of every thread's pixel
    __shared__ uint32_t s_tail[LV_BLOCK];  // its first inserted node (whose `next` is patched when splicing)
    __shared__ uint32_t s_count[LV_BLOCK]; // fragments of every thread's pixel in this slice
    __shared__ unsigned s_allocBase[LV_BLOCK / LV_WAVE], s_allocLeft[LV_BLOCK / LV_WAVE]; // per-wave chunk of node slots
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    LV_HITQ_SHARED(LV_BLOCK / LV_WAVE);
    LV_HITQ_MEM(hq);
    __shared__ unsigned s_prismQueue[PRIM == LV_PRIM_PRISM ? LV_BLOCK / LV_WAVE : 1][PRIM == LV_PRIM_PRISM ? LV_HITQ_CAP : 1];
    LvPixel px;
    const uint32_t slice = blockIdx.x % numSlices;
    if (!lv_block_pixel(U, T, px, blockIdx.x / numSlices)) return;
    if (PRIM == LV_PRIM_PRISM) hq.prismQueue = s_prismQueue[threadIdx.x >> 6];
    const unsigned long long tg0 = lv_group_clock();
    LvCounters cnt = {0, 0, 0, 0};
    // (the slices of a pixel are ONE ray: lv_trace_all counts a ray per active call, corrected below)
    const unsigned waveBase = threadIdx.x & ~63u;
    s_head[threadIdx.x] = 0xFFFFFFFFu;
    s_tail[threadIdx.x] = 0xFFFFFFFFu;
    s_count[threadIdx.x] = 0u;
    if ((threadIdx.x & 63u) == 0u) { s_allocBase[threadIdx.x >> 6] = 0u; s_allocLeft[threadIdx.x >> 6] = 0u; }
    const float aoTexel = (px.inView && U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(px.y) * U.width + px.x] : 1.0f;
    f3 o, d;
    lv_primary_ray(U, px.x, px.y, 0.5f, 0.5f, o, d);
    const float tMin = 0.0001f, tMax = 1000.0f;
    float lo = tMin, hi = __uint_as_float(__float_as_uint(tMax) + 1u); // t <= tMax  <=>  t < nextafter(tMax)
    if (numSlices > 1u && S.numSegs != 0) {
        // passage of the ray through the scene box (= the root node's grid, origin + [0, 255] * scale)
        const float4 q0 = S.nodes[0], q1 = S.nodes[1];
        const f3 bmin = mk3(q0.x, q0.y, q0.z);
        const f3 bmax = mk3(q0.x + 255.0f * q0.w, q0.y + 255.0f * q1.x, q0.z + 255.0f * q1.y);
        const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        const float tx0 = (bmin.x - o.x) * inv.x, tx1 = (bmax.x - o.x) * inv.x;
        const float ty0 = (bmin.y - o.y) * inv.y, ty1 = (bmax.y - o.y) * inv.y;
        const float tz0 = (bmin.z - o.z) * inv.z, tz1 = (bmax.z - o.z) * inv.z;
        float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fminf(tz0, tz1));
        float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
        tn = fminf(fmaxf(tn, tMin), tMax);
        tf = fminf(fmaxf(tf, tn), tMax);
        // interior boundaries only steer the load balance; b_0 = tMin and b_numSlices = tMax keep the partition exact
        const float w = (tf - tn) / float(numSlices);
        if (slice > 0u) lo = tn + w * float(slice);
        if (slice + 1u < numSlices) hi = tn + w * float(slice + 1u);
    }
    const bool active = px.inView && lo < hi;
    uint32_t prismDropped = 0u;
    if (STATS && active && slice != 0u && S.numSegs != 0) cnt.rays--;
    // Fragments of a pixel are produced by whichever lane is handed the (pixel, segment) hit: the lane shades with the
    // owner's ray + AO texel and links the node with an LDS atomic exchange on the owner's list head (the reference's
    // atomicExchange(startOffset[pixel]), LinkedListGather.glsl:55, kept in LDS until the slice is finished).
    // second payload word: the owner's pixel -- the lane that shades a fragment rebuilds the rays through the 2 x 2 quad partners
    // for fwidth(ribbonPosition) of the raster fragment colour (LvRasterQuad)
    lv_trace_all<STATS, false, PRIM>(S, U.radius, U.useCappedTubes != 0, active, o, d, lo, hi, aoTexel,
                        __uint_as_float(px.x | (px.y << 16)), lv_stack_mem(s_stack, S.stackOverflow), cm, hq, cnt,
                        [&](unsigned owner, uint32_t leaf, float t, int kind, f3 ro, f3 rd, float ownerAo, float ownerPixel) {
        // The rasterised prism: this kernel is the RASTERISER -- it finds which triangles cover which pixels, gives every covered
        // triangle its node and links it into the pixel's list (in the deterministic order of the owner's wave) -- and leaves the
        // FRAGMENT STAGE to k_ppll_shade_prism: the node carries {pixel, segment leaf | triangle << 26} until that kernel replaces
        // the two words by {colour, depth}.  A wave in front of the dense core covers two orders of magnitude more fragments than
        // the average wave; with the fragment stage (~3000 instructions) inline its serial shade batches were the kernel's critical
        // path, as a second pass over the node pool the fragments are shaded one per lane, evenly over the whole GPU.
        uint32_t word0, word1;
        if (PRIM == LV_PRIM_PRISM) {
            word0 = __float_as_uint(ownerPixel);
            word1 = leaf | (unsigned(kind) << 26);
        } else {
            LvHit h; h.t = t; h.leaf = leaf; h.kind = kind; h.found = true;
            float hitT;
            const bool rasterApply = U.ppllRasterColour != 0u;
            const uint32_t pxy = __float_as_uint(ownerPixel);
            const LvRasterQuad rq = lv_make_raster_quad(U, pxy & 0xFFFFu, pxy >> 16);
            f4 color = PRIM == LV_PRIM_ELLIPTIC ? lv_shade_hit_elliptic(S, U, ownerAo, ro, rd, h, hitT, true, rq, rasterApply)
                                                : lv_shade_hit<BANDS>(S, U, ownerAo, ro, rd, h, hitT, true, rq, rasterApply);
            if (STATS) cnt.hits++;
            if (color.w < 0.001f) return; // gatherFragment: discard, LinkedListGather.glsl:34
            word0 = lv_pack_unorm4x8(color);
            word1 = __float_as_uint(hitT);
        }
        // wave-aggregated node allocation: slots come from a per-wave chunk; one global atomic per LV_PPLL_CHUNK fragments
        // instead of one per batch (a returning atomic on one address costs microseconds under load and sat on the
        // critical path of the waves in front of dense geometry).  A batch that does not fit takes the rest of the old
        // chunk first and continues in a new one, so only the tail a wave leaves behind when it exits stays unused; the
        // pool carries that much slack (poolSlots >= ppllLinkedListSize + waves * LV_PPLL_CHUNK), i.e. no fragment the
        // reference's exact atomicAdd(fragCounter) allocator would have stored is dropped here.
        const unsigned long long mask = __ballot(1);
        const unsigned lane = lv_lane();
        const int leader = __ffsll((long long)mask) - 1;
        unsigned base = 0, left = 0, base2 = 0;
        if (int(lane) == leader) {
            const unsigned n = unsigned(__popcll(mask)), w = threadIdx.x >> 6;
            base = s_allocBase[w]; left = s_allocLeft[w];
            if (left < n) {
                base2 = atomicAdd(&dc->fragAlloc, (unsigned)LV_PPLL_CHUNK);
                s_allocBase[w] = base2 + (n - left);
                s_allocLeft[w] = LV_PPLL_CHUNK - (n - left);
            } else {
                s_allocBase[w] = base + n;
                s_allocLeft[w] = left - n;
            }
        }
        base = __shfl(base, leader, 64); left = __shfl(left, leader, 64); base2 = __shfl(base2, leader, 64);
        const unsigned rank = unsigned(__popcll(mask & ((1ull << lane) - 1ull)));
        const uint32_t insertIndex = rank < left ? base + rank : base2 + (rank - left);
        if (PRIM == LV_PRIM_PRISM) {
            // record {pixel, leaf | triangle << 26, rank}: rank = how many fragments the pixel had before this one, in the
            // deterministic order of the owner's wave -- the pixel's fragments end up in ONE contiguous run of the fragment array
            // (exclusive scan of the per-pixel counts -> offset; k_ppll_shade_prism writes to offset + rank), not in a linked list
            // whose 12-B nodes are scattered over 128-B lines (the resolve pass fetched 5.8 x the bytes it used)
            bool stored = false;
            if (insertIndex < poolSlots) {
                const uint32_t rk = atomicAdd(&s_count[waveBase + owner], 1u);
                if (rk < 0xFFFFu) {
                    nodes[3 * size_t(insertIndex) + 0] = word0;
                    nodes[3 * size_t(insertIndex) + 1] = word1;
                    nodes[3 * size_t(insertIndex) + 2] = rk;
                    stored = true;
                } else {   // (the per-pixel count shares its word with the count of discarded fragments: 16 bits each)
                    atomicSub(&s_count[waveBase + owner], 1u);
                    nodes[3 * size_t(insertIndex) + 0] = 0u;
                    nodes[3 * size_t(insertIndex) + 1] = LV_PPLL_DEAD;
                }
            }
            if (!stored) prismDropped++;   // no record: the fragment stage never sees it, but the reference's fragCounter counts it
            return;
        }
        atomicAdd(&s_count[waveBase + owner], 1u);
        if (insertIndex < poolSlots) {
            const uint32_t next = atomicExch(&s_head[waveBase + owner], insertIndex);
            if (next == 0xFFFFFFFFu) s_tail[waveBase + owner] = insertIndex;
            nodes[3 * size_t(insertIndex) + 0] = word0;
            nodes[3 * size_t(insertIndex) + 1] = word1;
            nodes[3 * size_t(insertIndex) + 2] = next;
        }
    }, [](unsigned) {});
    if (PRIM == LV_PRIM_PRISM) {
        // the slots this wave reserved but did not use are part of the range the fragment stage walks: mark them dead
        const unsigned w = threadIdx.x >> 6;
        const unsigned base = s_allocBase[w], left = s_allocLeft[w];
        for (unsigned k = lv_lane(); k < left; k += LV_WAVE)
            if (base + k < poolSlots) { nodes[3 * size_t(base + k) + 0] = 0u; nodes[3 * size_t(base + k) + 1] = LV_PPLL_DEAD; }
    }
    const uint32_t numFrags = s_count[threadIdx.x];
    uint32_t total = 0;
    if (PRIM == LV_PRIM_PRISM) {
        // one slice, one workgroup per pixel: the count is final (k_ppll_clear zeroed the pixels without fragments)
        if (px.inView && numFrags > 0u) fragCount[lv_ppll_addr(px.x, px.y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)] = numFrags;
    } else if (px.inView && numFrags > 0u) {
        const uint32_t addr = lv_ppll_addr(px.x, px.y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
        const uint32_t head = s_head[threadIdx.x], tail = s_tail[threadIdx.x];
        if (head != 0xFFFFFFFFu) { // splice the partial list in front of what other slices linked so far
            const uint32_t old = atomicExch(&startOffset[addr], head);
            nodes[3 * size_t(tail) + 2] = old;
        }
        total = atomicAdd(&fragCount[addr], numFrags) + numFrags; // the last slice to arrive sees the pixel's total
    }
    uint32_t m = total, sum = px.inView ? numFrags : 0u;
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        m = max(m, (uint32_t)__shfl_xor(m, ofs, 64));
        sum += (uint32_t)__shfl_xor(sum, ofs, 64);
    }
    if (PRIM == LV_PRIM_PRISM) {
        // fragCounter / maxDepthComplexity count KEPT fragments: the fragment stage adds the ones it keeps (and counts the ones it
        // discards in the upper half of the pixel's count word: the resolve pass reads the maximum), here only those without a record
        sum = prismDropped;
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) sum += (uint32_t)__shfl_xor(sum, ofs, 64);
        m = 0u;
    }
    if (lv_lane() == 0 && m > 0) atomicMax(&dc->maxDepthComplexity, m);
    if (lv_lane() == 0 && sum > 0) atomicAdd(&dc->fragCounter, sum); // fragCounter of the reference: every fragment counts
    lv_group_cost_add(T, px, tg0);
    if (STATS) lv_flush_counters(cnt, dc);
}

// (lv_run_start, the start of a pixel's run in the fragment array: lv_device.h)
// Fragment stage of ppll_fragment_source = raster_prism: one lane per record of the coverage kernel (k_ppll_gather<LV_PRIM_PRISM>),
// grid-stride over the record pool -- LinePassGeometryShaderTubes.glsl:732-1129 on the perspective-correct inputs (lv_shade_prism) +
// the store of gatherFragment (LinkedListGather.glsl:33-72): {colour, depth} goes to slot pixelOffset[pixel] + rank of the fragment
// array, so that every pixel's fragments form one contiguous run in the order the coverage kernel met them.  A fragment the shader
// discards (alpha < 0.001, :34) or the `kept` rules reject leaves a DEAD entry {0, LV_PPLL_DEAD} that the resolve pass steps over,
// and is counted in the upper 16 bits of the pixel's count word.  No atomics on the pool, none per kept fragment.
// MLAB (rendering mode 3, MLABGather.glsl:63-91): the entry is 12 B {packUnorm4x8(rgb * a, 1 - a), window depth, primitive key}
// instead, the key = leafSeg[leaf] << 6 | triangle orders the pixel's fragments as the reference's ordered interlock folds them
// (index-buffer order: segment by segment, triangles 2k, 2k + 1 of a segment); a discarded fragment is {0, LV_PPLL_DEAD, LV_MLAB_NO_KEY}.
// (LV_MLAB_NO_KEY and the LV_ENTRY_* formats: lv_device.h -- the hull's fragment stage in lv_hull.hip writes the same entries)
// window depth gl_FragCoord.z = clip.z / clip.w of a world position: rows z and w of proj * view in lv_clip_rows' order
__device__ __forceinline__ float lv_window_depth(const LvUniforms& U, f3 p) {
    float mz[4], mw[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        mz[c] = 0.0f; mw[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {   // column-major 4 x 4
            mz[c] += U.proj[4 * k + 2] * U.view[4 * c + k];
            mw[c] += U.proj[4 * k + 3] * U.view[4 * c + k];
        }
    }
    const float cz = ((mz[0] * p.x + mz[1] * p.y) + mz[2] * p.z) + mz[3];
    const float cw = ((mw[0] * p.x + mw[1] * p.y) + mw[2] * p.z) + mw[3];
    return cz / cw;
}
// the interpolated world position of the fragment (leaf, triangle tt) on the viewing ray d: the steps of lv_shade_prism up to I.pos, on
// the same operands (the normals do not enter the position).  The MLAB instances recompute them (about 0.04 ms of config 4's fragment
// stage) rather than pass I.pos out of lv_shade_prism: an output argument there changed the code of the mode-2 instances
// (scheduling of the helicity variants), which must stay as they are.
__device__ __forceinline__ f3 lv_prism_frag_pos(const LvSceneDev& S, const LvUniforms& U, const float* ringTab, f3 d, uint32_t leaf, uint32_t tt) {
    const LvPrismDev& R = S.prism;
    uint32_t pi[2];
    LvPrismPoint pt[2];
    lv_prism_frames(S, leaf, S.segs[2 * size_t(leaf)], S.segs[2 * size_t(leaf) + 1], pt, pi);
    const LvPrismTri T = lv_prism_tri_setup(ringTab, R.n, pt, pi, R.radius, tt);
    f3 nrm[3];
#pragma unroll
    for (int i = 0; i < 3; i++) nrm[i] = norm3q<false>(T.dir[i]);
    const f3 cam = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    const LvPrismPlanes pl = lv_prism_planes(R, T, cam, d);
    return lv_prism_interpolate(T, nrm, pl, d).pos;
}
// MBOIT (rendering mode 6, MBOITPass1.glsl:44-52 / MBOITPass2.glsl:21-37): the entry is the straight float32 colour gatherFragment
// receives (16 B, entry dst of the colour array) and the view depth -screenSpacePosition.z (4 B, entry dst of the depth array that
// starts poolSlots colour entries in); only the `kept` rules discard (the alpha < 0.001 discard lives in the gather shaders of modes
// 2 and 3, not in MBOIT's); a discarded fragment's depth word is LV_PPLL_DEAD.
// view depth of a world position: row z of the view matrix in one fixed float32 order, negated
__device__ __forceinline__ float lv_view_depth(const LvUniforms& U, f3 p) {
    return -(((U.view[2] * p.x + U.view[6] * p.y) + U.view[10] * p.z) + U.view[14]);
}
template <bool STATS, int SHADE = LV_SHADE_PLAIN, int FAST = 0, int ENTRY = LV_ENTRY_PPLL>
__global__ __launch_bounds__(LV_BLOCK, LV_PRISM_SHADE_MIN_WAVES) void k_ppll_shade_prism(const LvUniforms U, const LvSceneDev S,
                                                                   const uint32_t* __restrict__ records, uint2* __restrict__ frags,
                                                                   const uint32_t* __restrict__ pixelOffset,
                                                                   const uint32_t* __restrict__ blockBase, uint32_t* __restrict__ fragCount,
                                                                   LvDevCounters* dc, uint32_t poolSlots) {
    __shared__ float s_prismRing[4 * LV_PRISM_MAX_SUBDIV];
    if (threadIdx.x < LV_PRISM_MAX_SUBDIV) {   // ring tables [c | s | cp | sn] in LDS: the triangle a lane shades is a per-lane index
        s_prismRing[threadIdx.x] = S.prism.c[threadIdx.x];
        s_prismRing[LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.s[threadIdx.x];
        s_prismRing[2 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.cp[threadIdx.x];
        s_prismRing[3 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.sn[threadIdx.x];
    }
    __syncthreads();
    const uint32_t numSlots = min(dc->fragAlloc, poolSlots);   // the chunk allocator's high-water mark
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u); // the gather's ray interval [tMin, tMax]
    unsigned long long hits = 0;
    uint32_t localSum = 0u, localDead = 0u;
    // 256-slot items, item (sweep s, position p) to workgroup (p - 5 s) mod G: the dead tails of the rasteriser's record chunks end on
    // chunk boundaries, i.e. at fixed positions modulo the chunk size -- a fixed position per workgroup gave some workgroups only tails
    // and others none (chunks of 4096 slots: 0.71 instead of 0.29 ms)
    const uint32_t G = gridDim.x;
    for (uint32_t sweep = 0u, first = 0u; first < numSlots; sweep++, first += G * LV_BLOCK) {
        const uint32_t i = first + ((blockIdx.x + 5u * sweep) % G) * LV_BLOCK + threadIdx.x;
        if (i >= numSlots) continue;
        const uint32_t w0 = records[3 * size_t(i) + 0], w1 = records[3 * size_t(i) + 1], rank = records[3 * size_t(i) + 2];
        if (w1 == LV_PPLL_DEAD) continue;   // slot of a chunk tail
        const uint32_t px = w0 & 0xFFFFu, py = w0 >> 16;
        const uint32_t leaf = w1 & 0x03FFFFFFu, tt = w1 >> 26;
        const float aoTexel = (U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(py) * U.width + px] : 1.0f;
        f3 oo, d;
        lv_primary_ray(U, px, py, 0.5f, 0.5f, oo, d);
        const LvRasterQuad rq = lv_make_raster_quad(U, px, py);
        bool kept;
        float depth;
        const f4 color = lv_shade_prism<SHADE, FAST>(S, U, s_prismRing, aoTexel, o, d, tLo, tHi, leaf, tt, rq, U.ppllRasterColour != 0u, depth, kept);
        if (STATS && kept) hits++;
        const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
        const size_t dst = size_t(lv_run_start(pixelOffset, blockBase, addr)) + rank;
        if (kept && (ENTRY == LV_ENTRY_MBOIT || color.w >= 0.001f)) {   // gatherFragment: discard below, LinkedListGather.glsl:34 (MLABGather.glsl:64)
            if constexpr (ENTRY == LV_ENTRY_MBOIT) {
                reinterpret_cast<uint4*>(frags)[dst] = make_uint4(__float_as_uint(color.x), __float_as_uint(color.y),
                                                                  __float_as_uint(color.z), __float_as_uint(color.w));
                (reinterpret_cast<uint32_t*>(frags) + 4 * size_t(poolSlots))[dst] =
                        __float_as_uint(lv_view_depth(U, lv_prism_frag_pos(S, U, s_prismRing, d, leaf, tt)));
            } else if constexpr (ENTRY == LV_ENTRY_MLAB) {
                f4 m;   // packUnorm4x8(vec4(color.rgb * color.a, 1.0 - color.a)), MLABGather.glsl:76
                m.x = color.x * color.w; m.y = color.y * color.w; m.z = color.z * color.w; m.w = 1.0f - color.w;
                uint32_t* e = reinterpret_cast<uint32_t*>(frags) + 3 * dst;
                e[0] = lv_pack_unorm4x8(m);
                e[1] = __float_as_uint(lv_window_depth(U, lv_prism_frag_pos(S, U, s_prismRing, d, leaf, tt)));
                e[2] = (S.leafSeg[leaf] << 6) | tt;
            } else {
                frags[dst] = make_uint2(lv_pack_unorm4x8(color), __float_as_uint(depth));
            }
            localSum++;
        } else {
            if constexpr (ENTRY == LV_ENTRY_MBOIT) {
                (reinterpret_cast<uint32_t*>(frags) + 4 * size_t(poolSlots))[dst] = LV_PPLL_DEAD;
            } else if constexpr (ENTRY == LV_ENTRY_MLAB) {
                uint32_t* e = reinterpret_cast<uint32_t*>(frags) + 3 * dst;
                e[0] = 0u; e[1] = LV_PPLL_DEAD; e[2] = LV_MLAB_NO_KEY;
            } else {
                frags[dst] = make_uint2(0u, LV_PPLL_DEAD);
            }
            atomicAdd(&fragCount[addr], 0x10000u);
            localDead++;
        }
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        localSum += (uint32_t)__shfl_xor(localSum, ofs, 64);
        localDead += (uint32_t)__shfl_xor(localDead, ofs, 64);
    }
    if (lv_lane() == 0 && localSum > 0u) atomicAdd(&dc->fragCounter, localSum); // fragCounter of the reference: every fragment counts
    if (lv_lane() == 0 && localDead > 0u) atomicAdd(&dc->prismDiscards, localDead);
    if (STATS) {
        hits = lv_wave_sum_u64(hits);
        if (lv_lane() == 0 && hits) atomicAdd(&dc->hits, hits);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The rasteriser front end of ppll_fragment_source = raster_prism (ppll_prism_rasteriser = "segments", default): like the hardware
// the reference draws with, it walks the PRIMITIVES, not the pixels.  One lane per line segment (leaf order = Morton order: the 64
// segments of a wave are neighbours on screen): the 2 N ring vertices are projected with the frame's view-projection matrix, their
// bounding rectangle -- widened by LV_PRISM_BBOX_MARGIN pixels against the rounding of that projection -- gives the candidate pixels,
// and each candidate (pixel, segment) pair is decided by EXACTLY the coverage test of the LBVH front end (lv_prism_coverage_pts on the
// pixel-centre viewing ray: ray-space edge functions, fill rule), so both front ends produce the same fragments bit for bit; the
// rectangle only has to be conservative.  Config 4: 1 M segments of ~1 x 3 pixels -> 9.4 M coverage tests, where the all-hits walk
// of the 2.07 M viewing rays visited 41.9 M nodes and tested 19.7 M candidates (13.7 M of them up to the coverage stage).
//   k_ppll_mark_tiles   startOffset[pixel] = 0 for the pixels of the requested tiles (k_ppll_clear left 0xFFFFFFFF everywhere):
//                       a rank of a sharded frame rasterises into its own tiles only
//   k_ppll_raster_prism coverage -> record {pixel, leaf | triangle << 26, rank}; rank = atomicAdd on the pixel's count.  The order of
//                       a pixel's fragments is therefore not defined -- as in the reference, whose fragment shader invocations race
//                       on atomicExchange(startOffset) -- and nothing downstream depends on it: the resolve pass orders by the
//                       (depth, colour) key and, where a pixel holds more fragments than the sort arrays, keeps the nearest ones.
#define LV_PRISM_COARSE 32u
#define LV_PRISM_BBOX_MARGIN 0.015625f   // 1/64 pixel: two orders of magnitude above the rounding of the projection at 4K
#ifndef LV_PRISM_RASTER_CHUNK
#define LV_PRISM_RASTER_CHUNK 512u      // record slots a wave reserves per global atomic
#endif
#ifndef LV_PRISM_RASTER_MIN_WAVES
#define LV_PRISM_RASTER_MIN_WAVES 3
#endif
#ifndef LV_PRISM_RASTER_BLOCKS_PER_CU
#define LV_PRISM_RASTER_BLOCKS_PER_CU 3
#endif
template <bool STATS>
__global__ __launch_bounds__(LV_BLOCK) void k_ppll_mark_tiles(const LvUniforms U, const LvTiles T, uint32_t* __restrict__ startOffset,
                                                              uint32_t* __restrict__ coarse, LvDevCounters* dc) {
    LvPixel px;
    if (!lv_block_pixel(U, T, px)) return;
    if (px.inView) {
        startOffset[lv_ppll_addr(px.x, px.y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)] = 0u;
        // coarse map (LV_PRISM_COARSE-pixel cells): which parts of the viewport hold requested pixels at all -- the segment rasteriser of a
        // rank of a sharded frame drops the segments that project elsewhere before their set-up
        coarse[(px.y / LV_PRISM_COARSE) * ((U.width + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE) + px.x / LV_PRISM_COARSE] = 1u;
    }
    if (STATS) {   // one viewing ray per requested pixel: the rays whose coverage the rasteriser decides
        const unsigned long long n = (unsigned long long)__popcll(__ballot(px.inView));
        if (lv_lane() == 0 && n) atomicAdd(&dc->rays, n);
    }
}

// Offsets of the pixels' runs: exclusive scan of the per-pixel record counts.  Workgroup b of k_ppll_scan scans its LV_SCAN_ITEMS counts
// (in address order) and writes the offsets relative to its own first pixel and its total; k_ppll_scan_bases (one workgroup) turns the
// totals into bases.  Run of pixel a = lv_run_start(...) = startOffset[a] + blockBase[a / LV_SCAN_ITEMS].  (rocPRIM's scan: three
// launches, 24 us of a 0.85 ms frame.)  Pixels with more records than the sort arrays hold go on the list for k_ppll_select_nearest
// -- records, not kept fragments: the fragment stage has not run yet; that kernel copes with the superset.
#define LV_SCAN_ROUNDS (LV_SCAN_ITEMS / (4u * LV_BLOCK))   // uint4s per thread
__device__ __forceinline__ uint32_t lv_block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const unsigned lane = lv_lane(), w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up(int(incl), ofs, 64);
        if (int(lane) >= ofs) incl += t;
    }
    __syncthreads();   // (s_wave may still be read from the previous call)
    if (lane == 63u) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (uint32_t k = 0; k < LV_BLOCK / LV_WAVE; k++) {
        const uint32_t t = s_wave[k];
        if (k < w) before += t;
        total += t;
    }
    return before + incl - v;
}
__global__ __launch_bounds__(LV_BLOCK) void k_ppll_scan(const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ startOffset,
                                                        uint32_t n, uint32_t* __restrict__ blockTotals, uint32_t maxFrags,
                                                        uint32_t* __restrict__ overflowList, LvDevCounters* dc) {
    __shared__ uint32_t s_wave[LV_BLOCK / LV_WAVE];
    // round r: thread t owns the four addresses of uint4 number r * LV_BLOCK + t of the workgroup's block (coalesced)
    uint4 v[LV_SCAN_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < LV_SCAN_ROUNDS; r++) {
        const uint32_t first = blockIdx.x * LV_SCAN_ITEMS + (r * LV_BLOCK + threadIdx.x) * 4u;
        v[r] = first < n ? *reinterpret_cast<const uint4*>(fragCount + first) : make_uint4(0u, 0u, 0u, 0u);   // (n is a multiple of 4)
    }
    uint32_t carry = 0u;
#pragma unroll
    for (uint32_t r = 0; r < LV_SCAN_ROUNDS; r++) {
        const uint32_t first = blockIdx.x * LV_SCAN_ITEMS + (r * LV_BLOCK + threadIdx.x) * 4u;
        const uint32_t c0 = v[r].x & 0xFFFFu, c1 = v[r].y & 0xFFFFu, c2 = v[r].z & 0xFFFFu, c3 = v[r].w & 0xFFFFu;
        if (max(max(c0, c1), max(c2, c3)) > maxFrags) {
            if (c0 > maxFrags) overflowList[atomicAdd(&dc->ppllOverflowPixels, 1u)] = first;
            if (c1 > maxFrags) overflowList[atomicAdd(&dc->ppllOverflowPixels, 1u)] = first + 1u;
            if (c2 > maxFrags) overflowList[atomicAdd(&dc->ppllOverflowPixels, 1u)] = first + 2u;
            if (c3 > maxFrags) overflowList[atomicAdd(&dc->ppllOverflowPixels, 1u)] = first + 3u;
        }
        uint32_t total;
        const uint32_t before = carry + lv_block_exclusive_scan(((c0 + c1) + c2) + c3, s_wave, total);
        if (first < n) *reinterpret_cast<uint4*>(startOffset + first) = make_uint4(before, before + c0, before + c0 + c1, before + c0 + c1 + c2);
        carry += total;
    }
    if (threadIdx.x == 0u) blockTotals[blockIdx.x] = carry;
}
// second launch, one workgroup: the blocks' totals -> the blocks' bases.  (One launch with "the last workgroup to finish does this"
// was slower than rocPRIM's three: 2 028 / 507 workgroups x a returning agent-scope atomic on one counter = 69 / 29 us.)
__global__ __launch_bounds__(LV_BLOCK) void k_ppll_scan_bases(const uint32_t* __restrict__ blockTotals, uint32_t* __restrict__ blockBase,
                                                              uint32_t numBlocks) {
    __shared__ uint32_t s_wave[LV_BLOCK / LV_WAVE];
    uint32_t carry = 0u;
    for (uint32_t i0 = 0u; i0 < numBlocks; i0 += LV_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t t = i < numBlocks ? blockTotals[i] : 0u;
        uint32_t chunk;
        const uint32_t ex = lv_block_exclusive_scan(t, s_wave, chunk);
        if (i < numBlocks) blockBase[i] = carry + ex;
        carry += chunk;
    }
}

// Keep-the-nearest selection.  The order of a pixel's run is not defined (the rasteriser's lanes race for the ranks, as the reference's
// fragment shader invocations race for the list heads), so nothing downstream may depend on it: a pixel with more kept fragments than
// the sort arrays hold keeps the K = ppllMaxNumFrags NEAREST by the (depth, colour) key -- one of the subsets the reference's race
// can leave in the first K nodes of a list, and the one that loses the least.  One wave per listed pixel permutes the run in place so
// that those K come first (the resolve pass then reads the first K live entries of every run, in whatever order):
//   the K-th smallest depth by a radix select over its 31 bits (a ballot + population count per 64 entries and bit), ties at that
//   depth by the same select over the colour; then entries below the threshold key go to the front, the rest (dead entries included)
//   behind them.  Runs of up to 64 * LV_SELECT_REGS entries live in registers throughout; longer ones are re-read from memory per bit
//   and permuted through their slots of the (by then free) record pool.
// In the resolve pass itself this selection sat on the critical path of the few hundred waves over the dense core (a max-heap per
// lane: +0.23 ms on config 4 for 2 235 such pixels; the whole wave per pixel: +0.65 ms, every lane of those waves overflows); as a pass
// of its own the pixels are spread over the whole GPU.
#define LV_SELECT_REGS 8
template <bool REGS>
__device__ __forceinline__ void lv_select_nearest(uint2* __restrict__ run, uint2* __restrict__ temp, uint32_t n, uint32_t K,
                                                  uint32_t lane) {
    uint32_t kd[LV_SELECT_REGS], kc[LV_SELECT_REGS];
    const uint32_t rounds = (n + LV_WAVE - 1u) / LV_WAVE;
    if (REGS) {
#pragma unroll
        for (uint32_t r = 0; r < LV_SELECT_REGS; r++) {
            const uint32_t i = r * LV_WAVE + lane;
            uint2 e = make_uint2(0u, LV_PPLL_DEAD);
            if (r < rounds && i < n) e = run[i];
            kd[r] = e.y;   // live depths are positive floats (< 0x7F800000): ordered like their bits, below the dead pattern 0xFFFFFFFF
            kc[r] = e.x;
        }
    } else {
        for (uint32_t i = lane; i < n; i += LV_WAVE) temp[i] = run[i];   // (each lane reads back only what it wrote itself)
    }
    // number of entries with pred(depth bits, colour)
#define LV_SELECT_COUNT(cnt, PRED)                                                                             \
    do {                                                                                                       \
        cnt = 0u;                                                                                              \
        if (REGS) {                                                                                            \
            _Pragma("unroll") for (uint32_t r = 0; r < LV_SELECT_REGS; r++)                                    \
                if (r < rounds) { const uint32_t D = kd[r], C = kc[r]; (void)C; cnt += uint32_t(__popcll(__ballot(PRED))); } \
        } else {                                                                                               \
            for (uint32_t i0 = 0u; i0 < n; i0 += LV_WAVE) {                                                    \
                const uint32_t i = i0 + lane;                                                                  \
                const uint2 e = i < n ? temp[i] : make_uint2(0u, LV_PPLL_DEAD);                                \
                const uint32_t D = e.y, C = e.x; (void)C;                                                      \
                cnt += uint32_t(__popcll(__ballot(PRED)));                                                     \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
    {   // (the list holds the pixels with more than K RECORDS: where the fragment stage discarded enough of them, all live entries are kept)
        uint32_t live;
        LV_SELECT_COUNT(live, D < 0x80000000u);
        K = min(K, live);
        if (K == 0u) return;
    }
    uint32_t V = 0u;   // K-th smallest depth
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = V | (1u << bit);
        uint32_t cnt;
        LV_SELECT_COUNT(cnt, D < cand);
        if (cnt < K) V = cand;
    }
    uint32_t less;
    LV_SELECT_COUNT(less, D < V);
    const uint32_t need = K - less;   // >= 1 of the entries at depth V, smallest colours first
    uint32_t W = 0u;   // need-th smallest colour among them
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = W | (1u << bit);
        uint32_t cnt;
        LV_SELECT_COUNT(cnt, D == V && C < cand);
        if (cnt < need) W = cand;
    }
#undef LV_SELECT_COUNT
    uint32_t below;   // entries strictly below the threshold key (V, W); K - below of the entries equal to it are kept too
    {
        uint32_t c2;
        if (REGS) {
            c2 = 0u;
#pragma unroll
            for (uint32_t r = 0; r < LV_SELECT_REGS; r++)
                if (r < rounds) c2 += uint32_t(__popcll(__ballot(kd[r] == V && kc[r] < W)));
        } else {
            c2 = 0u;
            for (uint32_t i0 = 0u; i0 < n; i0 += LV_WAVE) {
                const uint32_t i = i0 + lane;
                const uint2 e = i < n ? temp[i] : make_uint2(0u, LV_PPLL_DEAD);
                c2 += uint32_t(__popcll(__ballot(e.y == V && e.x < W)));
            }
        }
        below = less + c2;
    }
    // destinations: [0, below) entries below the key, [below, K) the first K - below entries equal to it, [K, n) everything else
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t posA = 0u, posB = below, posC = K;
    auto place = [&](uint32_t D, uint32_t C, bool valid) {
        const bool a = valid && (D < V || (D == V && C < W));
        const bool b = valid && D == V && C == W;
        const unsigned long long ma = __ballot(a), mb = __ballot(b);
        const uint32_t rankB = posB + uint32_t(__popcll(mb & lt));
        const bool bKept = b && rankB < K;
        const bool c = valid && !a && !bKept;
        const unsigned long long mc = __ballot(c);
        uint32_t dst = 0u;
        if (a) dst = posA + uint32_t(__popcll(ma & lt));
        else if (bKept) dst = rankB;
        else if (c) dst = posC + uint32_t(__popcll(mc & lt));
        if (valid) run[dst] = make_uint2(C, D);
        posA += uint32_t(__popcll(ma));
        posB = min(K, posB + uint32_t(__popcll(mb)));
        posC += uint32_t(__popcll(mc));
    };
    if (REGS) {
#pragma unroll
        for (uint32_t r = 0; r < LV_SELECT_REGS; r++)
            if (r < rounds) place(kd[r], kc[r], r * LV_WAVE + lane < n);
    } else {
        for (uint32_t i0 = 0u; i0 < n; i0 += LV_WAVE) {
            const uint32_t i = i0 + lane;
            const uint2 e = i < n ? temp[i] : make_uint2(0u, LV_PPLL_DEAD);
            place(e.y, e.x, i < n);
        }
    }
}

__global__ __launch_bounds__(LV_WAVE) void k_ppll_select_nearest(const LvUniforms U, uint2* __restrict__ frags, uint2* __restrict__ temp,
                                                                 const uint32_t* __restrict__ startOffset,
                                                                 const uint32_t* __restrict__ blockBase,
                                                                 const uint32_t* __restrict__ fragCount,
                                                                 const uint32_t* __restrict__ overflowList, const LvDevCounters* dc) {
    const uint32_t count = dc->ppllOverflowPixels, lane = threadIdx.x;
    for (uint32_t p = blockIdx.x; p < count; p += gridDim.x) {
        const uint32_t addr = overflowList[p];
        const uint32_t off = lv_run_start(startOffset, blockBase, addr), n = fragCount[addr] & 0xFFFFu;
        if (n <= LV_WAVE * LV_SELECT_REGS) lv_select_nearest<true>(frags + off, nullptr, n, U.ppllMaxNumFrags, lane);
        else lv_select_nearest<false>(frags + off, temp + off, n, U.ppllMaxNumFrags, lane);
    }
}

// rows x, y, w of proj * view (clip = M * (p, 1)) as the segment rasteriser and its cull pass use them
__device__ __forceinline__ void lv_clip_rows(const LvUniforms& U, float mx[4], float my[4], float mw[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        mx[c] = 0.0f; my[c] = 0.0f; mw[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {   // column-major 4 x 4
            mx[c] += U.proj[4 * k + 0] * U.view[4 * c + k];
            my[c] += U.proj[4 * k + 1] * U.view[4 * c + k];
            mw[c] += U.proj[4 * k + 3] * U.view[4 * c + k];
        }
    }
}
// a world position through those rows: clip w, x and y
struct LvClipPoint { float cw, ccx, ccy; };
__device__ __forceinline__ LvClipPoint lv_clip_point(const float mx[4], const float my[4], const float mw[4], const f3& v) {
    LvClipPoint c;
    c.cw = ((mw[0] * v.x + mw[1] * v.y) + mw[2] * v.z) + mw[3];
    c.ccx = ((mx[0] * v.x + mx[1] * v.y) + mx[2] * v.z) + mx[3];
    c.ccy = ((my[0] * v.x + my[1] * v.y) + my[2] * v.z) + my[3];
    return c;
}
// Stage A of the segment rasteriser, one statement for k_ppll_raster_prism and k_mboit_stream_pass (pooled and streamed frames are
// equal byte for byte): a lane's walk over the candidate pixels of its segment
struct LvSegWalk {
    int x0, x1, y0, y1;   // the screen rectangle (none: x1 < x0)
    // oriented box: |(pixel centre - c) . a - aMid| <= aHalf and |(pixel centre - c) . n - nMid| <= nHalf, n = (-a.y, a.x)
    float ax, ay, cx0, cy0, aMid, aHalf, nMid, nHalf;
};
// the set-up per segment: its frames ({centre, normal, binormal} x 2 + the two point indices) into the wave's block of LDS, where
// stage B reads them, then rectangle and oriented box of the projected ring vertices
__device__ __forceinline__ LvSegWalk lv_seg_walk_setup(const LvUniforms& U, const LvSceneDev& S, float (*segLds)[LV_WAVE], const float mx[4],
                                                       const float my[4], const float mw[4], float halfW, float halfH, float wEps,
                                                       uint32_t N, bool valid, uint32_t leaf, unsigned lane) {
    const LvPrismDev& R = S.prism;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    float ax = 1.0f, ay = 0.0f, cx0 = 0.0f, cy0 = 0.0f, aMid = 0.0f, aHalf = 3.0e38f, nMid = 0.0f, nHalf = 3.0e38f;
    if (valid) {
        const float4 pa = S.segs[2 * size_t(leaf)], pb = S.segs[2 * size_t(leaf) + 1];
        uint32_t pi[2];
        LvPrismPoint pt[2];
        lv_prism_frames(S, leaf, pa, pb, pt, pi);
#pragma unroll
        for (int e = 0; e < 2; e++) {
            segLds[9 * e + 0][lane] = pt[e].centre.x; segLds[9 * e + 1][lane] = pt[e].centre.y; segLds[9 * e + 2][lane] = pt[e].centre.z;
            segLds[9 * e + 3][lane] = pt[e].normal.x; segLds[9 * e + 4][lane] = pt[e].normal.y; segLds[9 * e + 5][lane] = pt[e].normal.z;
            segLds[9 * e + 6][lane] = pt[e].binormal.x; segLds[9 * e + 7][lane] = pt[e].binormal.y; segLds[9 * e + 8][lane] = pt[e].binormal.z;
            segLds[18 + e][lane] = __uint_as_float(pi[e]);
        }
        // axis of the oriented box: the projected centres (any direction gives a valid box; this one gives a tight one)
        bool axisOk = true;
        float wcx[2], wcy[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const auto [cw, ccx, ccy] = lv_clip_point(mx, my, mw, pt[e].centre);
            axisOk = axisOk && cw > wEps;
            wcx[e] = (ccx / cw + 1.0f) * halfW;
            wcy[e] = (ccy / cw + 1.0f) * halfH;
        }
        if (axisOk) {
            const float dx = wcx[1] - wcx[0], dy = wcy[1] - wcy[0], l2 = dx * dx + dy * dy;
            if (l2 > 1e-12f && l2 < 1e30f) { const float il = 1.0f / sqrtf(l2); ax = dx * il; ay = dy * il; }
            cx0 = wcx[0]; cy0 = wcy[0];
        }
        float lox = 3.0e38f, hix = -3.0e38f, loy = 3.0e38f, hiy = -3.0e38f;
        float loa = 3.0e38f, hia = -3.0e38f, lon = 3.0e38f, hin = -3.0e38f;
        bool anyFront = false, anyBehind = false;
        for (uint32_t k = 0; k < N; k++) {
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const f3 v = lv_prism_pos(pt[e], lv_prism_dir(pt[e], R.cp[k], R.s[k]), R.radius);
                const auto [cw, ccx, ccy] = lv_clip_point(mx, my, mw, v);
                if (cw > wEps) {
                    const float wx = (ccx / cw + 1.0f) * halfW, wy = (ccy / cw + 1.0f) * halfH;
                    lox = fminf(lox, wx); hix = fmaxf(hix, wx); loy = fminf(loy, wy); hiy = fmaxf(hiy, wy);
                    const float ta = (wx - cx0) * ax + (wy - cy0) * ay, tn = (wy - cy0) * ax - (wx - cx0) * ay;
                    loa = fminf(loa, ta); hia = fmaxf(hia, ta); lon = fminf(lon, tn); hin = fmaxf(hin, tn);
                    anyFront = true;
                } else anyBehind = true;
            }
        }
        if (anyFront) {   // (all vertices behind the camera plane: no viewing ray meets the prism at a positive depth)
            if (anyBehind) { lox = 0.0f; loy = 0.0f; hix = float(U.width); hiy = float(U.height); }   // straddles the camera plane
            else if (axisOk) {
                // (the projected coordinates carry a relative rounding error of a few ulp: the margin also covers the box's own arithmetic)
                aMid = 0.5f * (loa + hia); aHalf = 0.5f * (hia - loa) + LV_PRISM_BBOX_MARGIN;
                nMid = 0.5f * (lon + hin); nHalf = 0.5f * (hin - lon) + LV_PRISM_BBOX_MARGIN;
            }
            // pixel x is a candidate iff its centre x + 0.5 lies in [lo - margin, hi + margin]
            const float fx0 = fmaxf(ceilf(lox - LV_PRISM_BBOX_MARGIN - 0.5f), 0.0f);
            const float fy0 = fmaxf(ceilf(loy - LV_PRISM_BBOX_MARGIN - 0.5f), 0.0f);
            const float fx1 = fminf(floorf(hix + LV_PRISM_BBOX_MARGIN - 0.5f), float(U.width) - 1.0f);
            const float fy1 = fminf(floorf(hiy + LV_PRISM_BBOX_MARGIN - 0.5f), float(U.height) - 1.0f);
            if (fx0 <= fx1 && fy0 <= fy1) { x0 = int(fx0); x1 = int(fx1); y0 = int(fy0); y1 = int(fy1); }
        }
    }
    return LvSegWalk{x0, x1, y0, y1, ax, ay, cx0, cy0, aMid, aHalf, nMid, nHalf};
}
// is the walk's pixel a candidate: inside the oriented box and, in a frame that leaves tiles out, requested
__device__ __forceinline__ bool lv_seg_walk_candidate(const LvUniforms& U, const LvSegWalk& w, int px, int py, uint32_t allRequested,
                                                      const uint32_t* __restrict__ startOffset) {
    const float qx = (float(px) + 0.5f) - w.cx0, qy = (float(py) + 0.5f) - w.cy0;
    bool cand = fabsf((qx * w.ax + qy * w.ay) - w.aMid) <= w.aHalf && fabsf((qy * w.ax - qx * w.ay) - w.nMid) <= w.nHalf;
    if (cand && !allRequested)
        cand = startOffset[lv_ppll_addr(uint32_t(px), uint32_t(py), U.ppllPaddedW, U.ppllTileW, U.ppllTileH)] == 0u;
    return cand;
}
// the next pixel of the rectangle, row by row; false after the last
__device__ __forceinline__ bool lv_seg_walk_advance(const LvSegWalk& w, int& px, int& py) {
    if (++px > w.x1) { px = w.x0; return ++py <= w.y1; }
    return true;
}
// The front of stage B, again one statement for both kernels: the (pixel, segment) pair in slot q of the wave's queue and the coverage
// mask of the pixel-centre viewing ray over the segment's triangles, the frames read back from the wave's block of LDS
// (no requested-tile test here: a whole-viewport frame requests every pixel, a rank of a sharded frame filters in stage A)
template <int NT>
__device__ __forceinline__ unsigned lv_seg_pair_coverage(const LvPrismDev& R, const float (*segLds)[LV_WAVE], const uint32_t* qLeaf,
                                                         const uint32_t* qPix, unsigned q, const f3& o, uint32_t& leaf, uint32_t& pix) {
    leaf = qLeaf[q];
    pix = qPix[q];
    const f3 d = lv_prism_cov_dir(R, pix & 0xFFFFu, pix >> 16);   // the pixel's coverage direction (unnormalised, lv_prism.h)
    const uint32_t sl = leaf >> 26;   // the pair's segment among the wave's 64 = the lane that queued it
    leaf &= 0x03FFFFFFu;
    LvPrismPoint pt[2];
    uint32_t pi[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        pt[e].centre = mk3(segLds[9 * e + 0][sl], segLds[9 * e + 1][sl], segLds[9 * e + 2][sl]);
        pt[e].normal = mk3(segLds[9 * e + 3][sl], segLds[9 * e + 4][sl], segLds[9 * e + 5][sl]);
        pt[e].binormal = mk3(segLds[9 * e + 6][sl], segLds[9 * e + 7][sl], segLds[9 * e + 8][sl]);
        pi[e] = __float_as_uint(segLds[18 + e][sl]);
    }
    return lv_prism_coverage_pts<NT>(R, pt, pi, R.radius, o, d);
}
// Sharded frame (a rank renders a tile list): ONE pass per frame over the segments' 32-B records decides which of them can touch a
// requested pixel at all and appends those to a list; k_ppll_raster_prism then walks the list, so that the segments of the other ranks'
// tiles cost this rank 32 B and ~60 instructions each instead of a slot of the rasteriser's waves (frames, oriented box, an empty
// pixel walk) -- with every rank looping over all segments the rasteriser took 0.20 ms for an eighth of config 4's tiles against 0.29 ms
// for all of them (profiles/shard_probe_r04_c4.json).  The test is conservative: both line points projected, the prism lies within
// `radius` of the segment; near the camera plane: undecided = kept.  Order of the list: blocks of <= 64 segments in leaf (= Morton)
// order, the blocks in the order the waves' appends arrive -- the fragments do not depend on it (the ranks race anyway).
#define LV_CULL_PER_BLOCK 2048u   // segments per workgroup of k_ppll_cull_segments (one global append each)
__global__ __launch_bounds__(LV_BLOCK) void k_ppll_cull_segments(const LvUniforms U, const LvSceneDev S, const uint32_t* __restrict__ coarse,
                                                                 uint32_t* __restrict__ leafList, LvDevCounters* dc) {
    const LvPrismDev& R = S.prism;
    float mx[4], my[4], mw[4];
    lv_clip_rows(U, mx, my, mw);
    const float halfW = 0.5f * float(U.width), halfH = 0.5f * float(U.height);
    const float wEps = 1e-3f * U.nearDist;
    const unsigned lane = lv_lane();
    // workgroup b owns the LV_CULL_PER_BLOCK consecutive segments from b * LV_CULL_PER_BLOCK: survivors are collected in LDS and
    // appended with ONE global atomic per workgroup (one per wave and 64 segments: 15.6 K returning atomics on one address at ~13 ns
    // each = 0.12 ms on config 4, more than the pass saves)
    __shared__ uint32_t s_keep[LV_CULL_PER_BLOCK];
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0u) s_n = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * LV_CULL_PER_BLOCK, last = min(first + LV_CULL_PER_BLOCK, S.numSegs);
    for (uint32_t leafBase = first + (threadIdx.x & ~63u); leafBase < last; leafBase += LV_BLOCK) {
        const uint32_t leaf = leafBase + lane;
        bool mine = false;
        if (leaf < last) {
            const float4 pa = S.segs[2 * size_t(leaf)], pb = S.segs[2 * size_t(leaf) + 1];
            const f3 centre[2] = {mk3(pa.x, pa.y, pa.z), mk3(pb.x, pb.y, pb.z)};
            mine = true;
            // does the segment project into a coarse cell with requested pixels?  Both line points with a generous bound of the
            // projected radius
            float lo[2] = {3.0e38f, 3.0e38f}, hi[2] = {-3.0e38f, -3.0e38f};
            bool decided = true;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const auto [cw, ccx, ccy] = lv_clip_point(mx, my, mw, centre[e]);
                if (!(cw > 4.0f * R.radius + wEps)) { decided = false; continue; }
                const float sx = (ccx / cw + 1.0f) * halfW, sy = (ccy / cw + 1.0f) * halfH;
                // |d screen| <= f r / (w - r) (1 + |x / w|) for a point within r of the centre: tangent of the off-axis angle from the
                // centre's own clip coordinates, 25 % and 2 pixels on top.  With a lens shift (proj[8], proj[9] != 0: clip.x = proj[0] x
                // + proj[8] z) the view-space tangent is (ndc + shift) / proj[0]; bounded by the sum of the magnitudes (adds 0 without)
                const float tanOff = (fabsf(ccx / cw) + fabsf(U.proj[8])) / fabsf(U.proj[0]) + (fabsf(ccy / cw) + fabsf(U.proj[9])) / fabsf(U.proj[5]);
                const float rp = 1.25f * (1.0f + tanOff) * R.radius * fmaxf(fabsf(U.proj[0]) * halfW, fabsf(U.proj[5]) * halfH) / (cw - R.radius) + 2.0f;
                lo[0] = fminf(lo[0], sx - rp); hi[0] = fmaxf(hi[0], sx + rp); lo[1] = fminf(lo[1], sy - rp); hi[1] = fmaxf(hi[1], sy + rp);
            }
            if (decided) {
                const float cwid = float((U.width + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE), chgt = float((U.height + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE);
                const float c0x = fmaxf(floorf(lo[0] / float(LV_PRISM_COARSE)), 0.0f), c1x = fminf(floorf(hi[0] / float(LV_PRISM_COARSE)), cwid - 1.0f);
                const float c0y = fmaxf(floorf(lo[1] / float(LV_PRISM_COARSE)), 0.0f), c1y = fminf(floorf(hi[1] / float(LV_PRISM_COARSE)), chgt - 1.0f);
                mine = false;
                if (c1x - c0x <= 3.0f && c1y - c0y <= 3.0f) {
                    for (float cy = c0y; cy <= c1y; cy += 1.0f)
                        for (float cx = c0x; cx <= c1x; cx += 1.0f) mine = mine || coarse[uint32_t(cy) * uint32_t(cwid) + uint32_t(cx)] != 0u;
                } else mine = c0x <= c1x && c0y <= c1y;   // (a large footprint: not worth the look-ups)
            }
        }
        const unsigned long long m = __ballot(mine);
        if (m) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(&s_n, uint32_t(__popcll(m)));
            base = __builtin_amdgcn_readfirstlane(base);
            if (mine) s_keep[base + uint32_t(__popcll(m & ((1ull << lane) - 1ull)))] = leaf;
        }
    }
    __syncthreads();
    const uint32_t n = s_n;
    if (threadIdx.x == 0u && n) s_base = atomicAdd(&dc->prismListCount, n);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += LV_BLOCK) leafList[s_base + i] = s_keep[i];
}

#define LV_PRISM_RASTER_QUEUE 128u   // (pixel, segment) pairs a wave holds between the two stages (>= 2 * LV_WAVE, power of two)
template <bool STATS, int NT>
__global__ __launch_bounds__(LV_BLOCK, LV_PRISM_RASTER_MIN_WAVES) void k_ppll_raster_prism(const LvUniforms U, const LvSceneDev S,
                                                                   uint32_t* __restrict__ records,
                                                                   const uint32_t* __restrict__ startOffset,
                                                                   uint32_t* __restrict__ fragCount, LvDevCounters* dc,
                                                                   uint32_t poolSlots, uint32_t allRequested,
                                                                   const uint32_t* __restrict__ leafList) {
    // Two stages per wave, joined by a queue in LDS:
    //  A  one lane per segment: the candidate pixels of its screen rectangle that also lie in the ORIENTED box of the projected ring
    //     vertices (axis = the projected segment; a 1 x 3-pixel segment at 45 degrees fills a third of its rectangle) and in a
    //     requested tile are queued as (pixel, segment) pairs -- a dozen instructions per candidate;
    //  B  whenever 64 pairs are waiting: one lane per pair, the coverage test of the pixel-centre viewing ray (~650 instructions,
    //     all lanes busy whatever the shapes of the segments) and the records of the covered triangles.
    // Both boxes only have to contain the prism's projection (widened by LV_PRISM_BBOX_MARGIN against rounding): the fragments are
    // decided by the coverage test alone.  With the test inline in stage A (the first version) a wave iterated as long as its largest
    // rectangle and two of three candidates missed: 0.39 ms on config 4; queued: see DESIGN.md.
    __shared__ uint32_t s_qLeaf[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE], s_qPix[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE];
    // the frames of the wave's 64 segments ({centre, normal, binormal} x 2 + the two point indices; [component][segment]): stage B
    // reads them from here -- re-fetching 96 B per pair through L2 was what its waves waited for
    __shared__ float s_seg[LV_BLOCK / LV_WAVE][20][LV_WAVE];
    const LvPrismDev& R = S.prism;
    const uint32_t N = NT > 0 ? uint32_t(NT) : R.n;
    const unsigned lane = lv_lane();
    uint32_t* qLeaf = s_qLeaf[threadIdx.x >> 6];
    uint32_t* qPix = s_qPix[threadIdx.x >> 6];
    float (*segLds)[LV_WAVE] = s_seg[threadIdx.x >> 6];
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    float mx[4], my[4], mw[4];   // rows of proj * view (clip = M * (p, 1)); x, y and w only
    lv_clip_rows(U, mx, my, mw);
    const float halfW = 0.5f * float(U.width), halfH = 0.5f * float(U.height);
    const float wEps = 1e-3f * U.nearDist;
    unsigned allocBase = 0u, allocLeft = 0u;   // this wave's chunk of record slots (wave-uniform)
    unsigned qHead = 0u, qCount = 0u;          // the queue (wave-uniform)
    unsigned long long tests = 0;
    uint32_t dropped = 0u;

    // stage B on the m <= 64 oldest pairs of the queue
    auto coverageStage = [&](unsigned m) {
        unsigned mask = 0u;
        uint32_t addr = 0u, leaf = 0u, pix = 0u;
        if (lane < m) {
            mask = lv_seg_pair_coverage<NT>(R, segLds, qLeaf, qPix, (qHead + lane) & (LV_PRISM_RASTER_QUEUE - 1u), o, leaf, pix);
            addr = lv_ppll_addr(pix & 0xFFFFu, pix >> 16, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            if (STATS) tests++;
        }
        while (__any(mask != 0u)) {
            const bool hit = mask != 0u;
            const unsigned long long hm = __ballot(hit);
            const unsigned n = unsigned(__popcll(hm));
            const unsigned rankInBatch = unsigned(__popcll(hm & ((1ull << lane) - 1ull)));
            unsigned base = allocBase, left = allocLeft, base2 = 0u;
            if (left < n) {
                if (lane == 0u) base2 = atomicAdd(&dc->fragAlloc, (unsigned)LV_PRISM_RASTER_CHUNK);
                base2 = __builtin_amdgcn_readfirstlane(base2);
                allocBase = base2 + (n - left);
                allocLeft = LV_PRISM_RASTER_CHUNK - (n - left);
            } else {
                allocBase = base + n;
                allocLeft = left - n;
            }
            if (hit) {
                const unsigned tt = unsigned(__ffs(int(mask))) - 1u;
                mask &= mask - 1u;
                const uint32_t insertIndex = rankInBatch < left ? base + rankInBatch : base2 + (rankInBatch - left);
                bool stored = false;
                if (insertIndex < poolSlots) {
                    const uint32_t rk = atomicAdd(&fragCount[addr], 1u);
                    // (the FULL word: the high half -- the discard count -- is still 0 in this stage, so once the count saturates every
                    // later lane fails and undoes its add; testing the low half only let lanes behind the one that hit 0xFFFF wrap
                    // around to ranks 0, 1, ... a second time)
                    if (rk < 0xFFFFu) {
                        records[3 * size_t(insertIndex) + 0] = pix;
                        records[3 * size_t(insertIndex) + 1] = leaf | (tt << 26);
                        records[3 * size_t(insertIndex) + 2] = rk;
                        stored = true;
                    } else {   // (the per-pixel count shares its word with the count of discarded fragments: 16 bits each)
                        atomicSub(&fragCount[addr], 1u);
                        records[3 * size_t(insertIndex) + 0] = 0u;
                        records[3 * size_t(insertIndex) + 1] = LV_PPLL_DEAD;
                    }
                }
                if (!stored) dropped++;   // no record: the fragment stage never sees it, but the reference's fragCounter counts it
            }
        }
        qHead = (qHead + m) & (LV_PRISM_RASTER_QUEUE - 1u);
        qCount -= m;
    };

    // (static interleave: wave w takes segments [64 (w + k numWaves), + 64).  Work queues were slower, whatever the order: tickets over
    // consecutive blocks of 256 / 1024 segments 0.42 / 0.80 ms (consecutive = spatially clustered: the blocks of the dense core cost
    // many times the average and end up as the tail), over blocks in a scrambled order (ticket * prime mod count) 0.38 / 0.33 / 0.37 /
    // 0.49 ms for 64 / 128 / 256 / 512 segments per ticket -- small tickets pay the returning atomic on one address (13 ns each, 15.6 K
    // of them), large ones the variance again -- against 0.29 ms)
    const uint32_t waveId = blockIdx.x * (LV_BLOCK / LV_WAVE) + (threadIdx.x >> 6), numWaves = gridDim.x * (LV_BLOCK / LV_WAVE);
    // the work list: every segment (leaf order), or -- a rank of a sharded frame -- the segments k_ppll_cull_segments kept
    const uint32_t numItems = leafList ? dc->prismListCount : S.numSegs;
    for (uint32_t itemBase = waveId * LV_WAVE; itemBase < numItems; itemBase += numWaves * LV_WAVE) {
        const bool valid = itemBase + lane < numItems;
        const uint32_t leaf = !valid ? 0u : (leafList ? leafList[itemBase + lane] : itemBase + lane);
        const LvSegWalk w = lv_seg_walk_setup(U, S, segLds, mx, my, mw, halfW, halfH, wEps, N, valid, leaf, lane);
        int px = w.x0, py = w.y0;
        bool more = valid && w.x1 >= w.x0 && w.y1 >= w.y0;
        while (__any(more)) {
            const bool cand = more && lv_seg_walk_candidate(U, w, px, py, allRequested, startOffset);
            const unsigned long long cm = __ballot(cand);
            if (cand) {
                const unsigned q = (qHead + qCount + unsigned(__popcll(cm & ((1ull << lane) - 1ull)))) & (LV_PRISM_RASTER_QUEUE - 1u);
                qLeaf[q] = leaf | (lane << 26);
                qPix[q] = uint32_t(px) | (uint32_t(py) << 16);
            }
            qCount += unsigned(__popcll(cm));
            if (qCount >= LV_WAVE) coverageStage(LV_WAVE);
            if (more) more = lv_seg_walk_advance(w, px, py);
        }
        while (qCount > 0u) coverageStage(qCount < LV_WAVE ? qCount : LV_WAVE);   // (the next 64 segments replace the frames in LDS)
    }
    // the slots this wave reserved but did not use are part of the range the fragment stage walks: mark them dead
    for (unsigned k = lane; k < allocLeft; k += LV_WAVE)
        if (allocBase + k < poolSlots) { records[3 * size_t(allocBase + k) + 0] = 0u; records[3 * size_t(allocBase + k) + 1] = LV_PPLL_DEAD; }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) dropped += (uint32_t)__shfl_xor(dropped, ofs, 64);
    if (lane == 0u && dropped > 0u) atomicAdd(&dc->fragCounter, dropped);
    if (STATS) {
        tests = lv_wave_sum_u64(tests);
        if (lane == 0u && tests) atomicAdd(&dc->prims, tests);
    }
}

// clear(): LinkedListClear.glsl:46-55 (start offsets = -1) + fragmentCounterBuffer->fill(0), and the per-pixel fragment counts
// (startValue: 0xFFFFFFFF = empty list / pixel not requested; the segment rasteriser of a frame whose tiles cover the whole viewport
// passes 0 = every pixel requested and skips k_ppll_mark_tiles; viewingRays: those pixels' viewing rays for the statistics)
__global__ __launch_bounds__(LV_BLOCK) void k_ppll_clear(uint4* __restrict__ startOffset, uint4* __restrict__ fragCount, size_t n4,
                                                         LvDevCounters* dc, uint32_t startValue, unsigned long long viewingRays) {
    const size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i < n4) {
        startOffset[i] = make_uint4(startValue, startValue, startValue, startValue);
        fragCount[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (i == 0) {
        dc->fragCounter = 0u; dc->fragAlloc = 0u; dc->prismDiscards = 0u; dc->ppllOverflowPixels = 0u; dc->prismListCount = 0u;
        if (viewingRays) atomicAdd(&dc->rays, viewingRays);
    }
}

// per-thread fragment arrays interleaved over the wave: entry i of lane l at [i * 64 + l]
struct LvFragArrays {
    uint32_t* col;
    float* dep;
    __device__ __forceinline__ uint32_t& c(uint32_t i) { return col[i * LV_WAVE]; }
    __device__ __forceinline__ float& d(uint32_t i) { return dep[i * LV_WAVE]; }
    // (depth, colour) key order: the reference compares depth only and leaves ties to rasterisation order
    __device__ __forceinline__ bool gt(uint32_t a, uint32_t b) {
        float da = d(a), db = d(b);
        return da > db || (da == db && c(a) > c(b));
    }
    __device__ __forceinline__ void swap(uint32_t a, uint32_t b) {
        uint32_t tc = c(a); c(a) = c(b); c(b) = tc;
        float td = d(a); d(a) = d(b); d(b) = td;
    }
};

// minHeapSink4, LinkedListSort.glsl:177-205
__device__ __forceinline__ void lv_min_heap_sink4(LvFragArrays& A, uint32_t x, uint32_t fragsCount) {
    uint32_t c, t;
    while ((t = 4 * x + 1) < fragsCount) {
        if (t + 1 < fragsCount && A.gt(t, t + 1)) c = t + 1; else c = t;
        if (t + 2 < fragsCount && A.gt(c, t + 2)) c = t + 2;
        if (t + 3 < fragsCount && A.gt(c, t + 3)) c = t + 3;
        if (!A.gt(x, c)) return;
        A.swap(x, c);
        x = c;
    }
}

// ---- sorting_mode != "Priority Queue" (SORTING_MODE_NAMES, src/Renderers/PPLL.hpp:32-50): the whole list is sorted, then every
// fragment is blended (blendFTB, LinkedListSort.glsl:45-59; the priority queue alone stops at alpha 0.99).  All comparisons
// go through the (depth, colour) key like the heap's, so the seven modes differ in cost and -- bitonic sort on a list whose length
// is no power of two, the quicksorts when their fixed stack overflows -- in what the shader's algorithm leaves unsorted.
struct LvSortStack { // LinkedListQuicksort.glsl:30-55: pushes beyond STACK_SIZE are dropped, an empty stack pops 0
    int mem[64];
    int size, counter;
    __device__ __forceinline__ void push(int v) { if (counter < size) mem[counter++] = v; }
    __device__ __forceinline__ int pop() { return counter > 0 ? mem[--counter] : 0; }
};
__device__ __forceinline__ bool lv_key_less(float da, uint32_t ca, float db, uint32_t cb) {
    return da < db || (da == db && ca < cb);
}
__device__ __forceinline__ void lv_gap_insertion_pass(LvFragArrays& A, uint32_t n, uint32_t gap) {
    for (uint32_t i = gap; i < n; ++i) { // insertionSort (:80-104) is the pass with gap 1, shellSort (:107-137) four of them
        const uint32_t fc = A.c(i);
        const float fd = A.d(i);
        uint32_t j = i;
        while (j >= gap && lv_key_less(fd, fc, A.d(j - gap), A.c(j - gap))) {
            A.c(j) = A.c(j - gap);
            A.d(j) = A.d(j - gap);
            j -= gap;
        }
        A.c(j) = fc;
        A.d(j) = fd;
    }
}
__device__ __forceinline__ void lv_max_heap_sink(LvFragArrays& A, uint32_t x, uint32_t n) { // :140-157
    uint32_t c;
    while ((c = 2 * x + 1) < n) {
        if (c + 1 < n && A.gt(c + 1, c)) ++c;
        if (!A.gt(c, x)) return;
        A.swap(x, c);
        x = c;
    }
}
__device__ __forceinline__ int lv_sort_stack_size(uint32_t maxFrags) { // PerPixelLinkedListLineRenderer.cpp:178
    const int s = int(ceil(log2(double(maxFrags))) * 2 + 4);
    return s < 0 ? 0 : (s > 64 ? 64 : s);
}
__device__ void lv_sort_fragments(uint32_t mode, LvFragArrays& A, uint32_t n, uint32_t maxFrags) {
    if (mode == 1u) { // bubbleSort :62-77
        bool changed;
        do {
            changed = false;
            for (uint32_t i = 0; i + 1 < n; ++i)
                if (A.gt(i, i + 1)) { A.swap(i, i + 1); changed = true; }
        } while (changed);
    } else if (mode == 2u) {
        lv_gap_insertion_pass(A, n, 1u);
    } else if (mode == 3u) {
        lv_gap_insertion_pass(A, n, 24u);
        lv_gap_insertion_pass(A, n, 9u);
        lv_gap_insertion_pass(A, n, 4u);
        lv_gap_insertion_pass(A, n, 1u);
    } else if (mode == 4u) { // heapSort :159-172
        for (uint32_t i = (n + 1) / 2; i > 0; --i) lv_max_heap_sink(A, i - 1, n);
        for (uint32_t i = 1; i < n; ++i) {
            A.swap(0, n - i);
            lv_max_heap_sink(A, 0, n - i);
        }
    } else if (mode == 5u) { // bitonicSort :241-262, with the reference's guards (no padding to a power of two)
        for (uint32_t k = 2; k <= n; k *= 2)
            for (uint32_t j = k / 2; j > 0; j /= 2)
                for (uint32_t i = 0; i < n; i++) {
                    const uint32_t l = i ^ j;
                    if (l > i && l < n) {
                        const bool up = (i & k) == 0u;
                        if (up ? A.gt(i, l) : A.gt(l, i)) A.swap(i, l);
                    }
                }
    } else {
        LvSortStack st;
        st.size = lv_sort_stack_size(maxFrags);
        st.counter = 0;
        st.push(0);
        st.push(int(n) - 1);
        if (mode == 6u) { // quicksort :93-114 with the Lomuto partition :57-68
            while (st.counter != 0) {
                const int high = st.pop(), low = st.pop();
                const float pd = A.d(uint32_t(high));
                const uint32_t pc = A.c(uint32_t(high));
                int i = low;
                for (int j = low; j <= high; j++)
                    if (lv_key_less(A.d(uint32_t(j)), A.c(uint32_t(j)), pd, pc)) { A.swap(uint32_t(i), uint32_t(j)); i++; }
                A.swap(uint32_t(i), uint32_t(high));
                const int pivot = i;
                if (low < pivot - 1) { st.push(low); st.push(pivot - 1); }
                if (pivot + 1 < high) { st.push(pivot + 1); st.push(high); }
            }
        } else { // quicksortHybrid :116-141 with the Hoare partition :70-91, finished by an insertion sort
            if (n > 16u)
                while (st.counter != 0) {
                    const int high = st.pop(), low = st.pop();
                    const uint32_t a = uint32_t(low), m = uint32_t((low + high) / 2), b = uint32_t(high);
                    const bool ab = A.gt(m, a), ba2 = A.gt(a, b), bm = A.gt(m, b); // a < m, b < a, b < m
                    const uint32_t mnmb = A.gt(m, b) ? b : m, mnab = A.gt(a, b) ? b : a;
                    const uint32_t p = ab ? (ba2 ? a : mnmb) : (bm ? m : mnab);
                    const float pd = A.d(p);
                    const uint32_t pc = A.c(p);
                    int i = low - 1, j = high + 1, pivot;
                    for (;;) {
                        do { i = i + 1; } while (lv_key_less(A.d(uint32_t(i)), A.c(uint32_t(i)), pd, pc));
                        do { j = j - 1; } while (lv_key_less(pd, pc, A.d(uint32_t(j)), A.c(uint32_t(j))));
                        if (i >= j) { pivot = j; break; }
                        A.swap(uint32_t(i), uint32_t(j));
                    }
                    if (low + 16 < pivot) { st.push(low); st.push(pivot - 1); }
                    if (pivot + 16 < high) { st.push(pivot + 1); st.push(high); }
                }
            lv_gap_insertion_pass(A, n, 1u);
        }
    }
}

// One wave per workgroup; fragment arrays in LDS when they fit, else in a global scratch slab.
// ARRAYS (frames of ppll_fragment_source = raster_prism): the pixel's fragments are the contiguous run frags[startOffset[pixel] ...
// + count) of 8-B {colour, depth} entries (startOffset = exclusive scan of the counts), in no defined order.
template <bool USE_LDS, bool PQ = true, bool ARRAYS = false>
__global__ __launch_bounds__(LV_WAVE) void k_ppll_resolve(const LvUniforms U, const LvTiles T,
                                                          const uint32_t* __restrict__ nodes,
                                                          const uint32_t* __restrict__ startOffset,
                                                          uint32_t* __restrict__ out, uint32_t* __restrict__ scratch,
                                                          uint32_t numGroups, const uint32_t* __restrict__ fragCount,
                                                          LvDevCounters* dc, const uint32_t* __restrict__ blockBase) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    uint32_t maxCount = 0u;   // raster_prism frames: the largest per-pixel fragment count (kept fragments) is collected here
    const uint32_t maxFrags = U.ppllMaxNumFrags;
    const uint32_t lane = threadIdx.x;
    LvFragArrays A;
    if (USE_LDS) {
        A.col = reinterpret_cast<uint32_t*>(s_dyn) + lane;
        A.dep = reinterpret_cast<float*>(s_dyn) + size_t(maxFrags) * LV_WAVE + lane;
    } else {
        uint32_t* base = scratch + size_t(blockIdx.x) * 2 * maxFrags * LV_WAVE;
        A.col = base + lane;
        A.dep = reinterpret_cast<float*>(base) + size_t(maxFrags) * LV_WAVE + lane;
    }
    // A wave resolves one 8 x 8 pixel cell; the 64 cells of a 64 x 64-pixel group are consecutive, and the groups come in the dispatch
    // order of the tile kernels (LvTiles::groupOrder: most expensive group of the previous frame first), so that the long waves over
    // the dense core of a data set start first.
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
        const bool inView = inTile && x < U.width && y < U.height;
        float res[4] = {U.background[0], U.background[1], U.background[2], U.background[3]};
        uint32_t fragOffset = 0xFFFFFFFFu;
        uint32_t numFrags = 0;
        if (ARRAYS) {
            // the first maxFrags live entries of the run: where a pixel kept more, k_ppll_select_nearest moved the nearest to the front
            if (inView) {
                const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
                fragOffset = lv_run_start(startOffset, blockBase, addr);
                const uint32_t v = fragCount[addr];
                const uint32_t n = v & 0xFFFFu;                // entries of the run; v >> 16 of them are dead
                maxCount = max(maxCount, n - (v >> 16));
                const uint2* __restrict__ run = reinterpret_cast<const uint2*>(nodes) + fragOffset;
                for (uint32_t j = 0u; j < n && numFrags < maxFrags; j += 4u) {   // four independent loads in flight per step
                    uint2 e[4];
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) e[k] = j + k < n ? run[j + k] : make_uint2(0u, LV_PPLL_DEAD);
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        if ((e[k].y == LV_PPLL_DEAD && e[k].x == 0u) || numFrags >= maxFrags) continue;
                        A.c(numFrags) = e[k].x;
                        A.d(numFrags) = __uint_as_float(e[k].y);
                        numFrags++;
                    }
                }
            }
            // the whole-list sorts see the fragments in ascending key order (what they leave unsorted depends on their input)
            if (!PQ && numFrags > 1u) {
                for (uint32_t i = numFrags / 2u; i > 0u; --i) lv_max_heap_sink(A, i - 1u, numFrags);
                for (uint32_t i = numFrags - 1u; i > 0u; --i) { A.swap(0u, i); lv_max_heap_sink(A, 0u, i); }
            }
        } else if (inView) {
            fragOffset = startOffset[lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)];
        }
        if (inView) {
            while (!ARRAYS && numFrags < maxFrags) {
                if (fragOffset == 0xFFFFFFFFu) break;
                const uint32_t c = nodes[3 * size_t(fragOffset) + 0], db = nodes[3 * size_t(fragOffset) + 1];
                fragOffset = nodes[3 * size_t(fragOffset) + 2];
                // dead node (LV_PPLL_DEAD): a linked slot whose fragment the fragment stage of the rasterised prism discarded; it is
                // not part of the list (gatherFragment never stored it, LinkedListGather.glsl:34).  Lists of the reference cannot
                // contain this pattern: a node's depth is a length.
                if (db == LV_PPLL_DEAD && c == 0u) continue;
                A.c(numFrags) = c;
                A.d(numFrags) = __uint_as_float(db);
                numFrags++;
            }
            if (!PQ && numFrags > 0) {
                lv_sort_fragments(U.ppllSortingMode, A, numFrags, maxFrags);
                float ray[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (uint32_t i = 0; i < numFrags; i++) { // blendFTB
                    f4 src = lv_unpack_unorm4x8(A.c(i));
                    ray[0] = ray[0] + ((1.0f - ray[3]) * src.w) * src.x;
                    ray[1] = ray[1] + ((1.0f - ray[3]) * src.w) * src.y;
                    ray[2] = ray[2] + ((1.0f - ray[3]) * src.w) * src.z;
                    ray[3] = ray[3] + (1.0f - ray[3]) * src.w;
                }
                const float a = ray[3];
                if (a > 0.0f) {
#pragma unroll
                    for (int k = 0; k < 3; k++) res[k] = (ray[k] / a) * a + U.background[k] * (1.0f - a);
                    res[3] = a + U.background[3] * (1.0f - a);
                }
            }
            if (PQ && numFrags > 0) {
                // frontToBackPQ, LinkedListSort.glsl:207-238
                uint32_t i;
                for (i = numFrags / 4; i > 0; --i) lv_min_heap_sink4(A, i, numFrags);
                float ray[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                i = 0;
                while (i < numFrags && ray[3] < 0.99f) {
                    lv_min_heap_sink4(A, 0, numFrags - i++);
                    f4 src = lv_unpack_unorm4x8(A.c(0));
                    ray[0] = ray[0] + ((1.0f - ray[3]) * src.w) * src.x;
                    ray[1] = ray[1] + ((1.0f - ray[3]) * src.w) * src.y;
                    ray[2] = ray[2] + ((1.0f - ray[3]) * src.w) * src.z;
                    ray[3] = ray[3] + (1.0f - ray[3]) * src.w;
                    A.c(0) = A.c(numFrags - i);
                    A.d(0) = A.d(numFrags - i);
                }
                const float a = ray[3];
                if (a > 0.0f) {
                    // straight alpha rgb/A, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour
                    // (LinkedListSort.glsl:236-237, PerPixelLinkedListLineRenderer.cpp:70,395-397)
#pragma unroll
                    for (int k = 0; k < 3; k++) res[k] = (ray[k] / a) * a + U.background[k] * (1.0f - a);
                    res[3] = a + U.background[3] * (1.0f - a);
                }
            }
        }
        f4 c; c.x = res[0]; c.y = res[1]; c.z = res[2]; c.w = res[3];
        if (inTile) out[outIndex] = lv_pack_unorm4x8(c);
    }
    if (ARRAYS) {
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
        if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
    }
}

// ================================================================ MLAB (rendering mode 3)
// Multi-Layer Alpha Blending [Salvi and Vaidyanathan 2014] as MLABRenderer runs it with its default ordered fragment shader interlock
// (MLABRenderer.hpp:133-135): every pixel folds its fragments in primitive order into K = numLayers nodes.  Gather, then fold: the
// fragment stage (k_ppll_shade_prism<..., MLAB = true>) leaves each pixel's fragments as one contiguous run of 12-B entries {colour,
// window depth, primitive key}; k_mlab_resolve orders a run by key and folds it into K + 1 nodes held in registers -- no K x W x H
// node buffer and no per-pixel lock.  Runs longer than a lane's LDS share go to k_mlab_resolve_long (one workgroup per pixel).
#define LV_MLAB_INFINITE 1e30f      // DISTANCE_INFINITE (MLABHeader.glsl)
#define LV_MLAB_CLEAR 0xFF000000u   // clearPixel's premulColor: rgb 0, transmittance 1 (MLABHeader.glsl:186)
#ifndef LV_MLAB_LDS
#define LV_MLAB_LDS 32u             // run entries one lane of k_mlab_resolve orders in LDS (12 B each: 24 KB per wave)
#endif
#define LV_MLAB_LONG_BLOCK 256u     // threads of k_mlab_resolve_long
#define LV_MLAB_LONG_TILE 1024u     // keys per LDS tile of its ranking pass

// K + 1 nodes {depth, premulColor} for K <= C: every loop over the nodes is unrolled with a runtime guard (a runtime index would put
// the arrays in scratch memory)
template <int C>
struct LvMlabNodes {
    float d[C + 1];
    uint32_t c[C + 1];
    __device__ __forceinline__ void clear() {   // clearPixel
#pragma unroll
        for (int i = 0; i <= C; i++) { d[i] = LV_MLAB_INFINITE; c[i] = LV_MLAB_CLEAR; }
    }
    // loadFragmentNodes (node K = DISTANCE_INFINITE, MLABHeader.glsl:161) + multiLayerAlphaBlending (MLABGather.glsl:38-60)
    __device__ __forceinline__ void insert(float fd, uint32_t fc, uint32_t K) {
#pragma unroll
        for (int i = 0; i <= C; i++) {
            if (uint32_t(i) == K) d[i] = LV_MLAB_INFINITE;   // (the passes before i = K touched nodes < K only)
            if (uint32_t(i) <= K && fd <= d[i]) {             // one bubble pass over K + 1 entries
                const float td = d[i];
                const uint32_t tc = c[i];
                d[i] = fd; c[i] = fc;
                fd = td; fc = tc;
            }
        }
        float dK = LV_MLAB_INFINITE;
        uint32_t cK = 0u, cP = 0u;
#pragma unroll
        for (int i = 0; i <= C; i++) {
            if (uint32_t(i) == K) { dK = d[i]; cK = c[i]; }
            if (uint32_t(i) + 1u == K) cP = c[i];
        }
        if (dK != LV_MLAB_INFINITE) {   // merge nodes K - 1 and K; the merged node keeps the depth of node K - 1
            const f4 src = lv_unpack_unorm4x8(cP), dst = lv_unpack_unorm4x8(cK);
            f4 m;
            m.x = src.x + dst.x * src.w;
            m.y = src.y + dst.y * src.w;
            m.z = src.z + dst.z * src.w;
            m.w = src.w * dst.w;   // transmittance
            const uint32_t merged = lv_pack_unorm4x8(m);
#pragma unroll
            for (int i = 0; i < C; i++)
                if (uint32_t(i) + 1u == K) c[i] = merged;
        }
    }
    // MLABResolve.glsl:51-77, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour (MLABRenderer.cpp:78) as mode 2's resolve
    // writes it; alphaOut = 0 (no fragment, or only fragments whose 1 - a packs to 255) gives the background
    __device__ __forceinline__ uint32_t resolve(const LvUniforms& U, uint32_t K) const {
        float col[3] = {0.0f, 0.0f, 0.0f}, tr = 1.0f;
#pragma unroll
        for (int i = 0; i < C; i++) {
            if (uint32_t(i) < K) {
                const f4 src = lv_unpack_unorm4x8(c[i]);
                col[0] = col[0] + tr * src.x;
                col[1] = col[1] + tr * src.y;
                col[2] = col[2] + tr * src.z;
                tr *= src.w;
            }
        }
        const float a = 1.0f - tr;
        f4 r;
        r.x = U.background[0]; r.y = U.background[1]; r.z = U.background[2]; r.w = U.background[3];
        if (a > 0.0f) {
            r.x = (col[0] / a) * a + U.background[0] * (1.0f - a);
            r.y = (col[1] / a) * a + U.background[1] * (1.0f - a);
            r.z = (col[2] / a) * a + U.background[2] * (1.0f - a);
            r.w = a + U.background[3] * (1.0f - a);
        }
        return lv_pack_unorm4x8(r);
    }
};

// start of a pixel's run: frames address the runs through k_ppll_scan's block bases, lv_mlab_resolve_buffers with absolute offsets
__device__ __forceinline__ uint32_t lv_mlab_run_start(const uint32_t* __restrict__ startOffset, const uint32_t* __restrict__ blockBase,
                                                      uint32_t addr) {
    return blockBase ? lv_run_start(startOffset, blockBase, addr) : startOffset[addr];
}

// One lane per pixel, one wave per workgroup, the cells and groups of k_ppll_resolve.  The lane copies the live entries of its run
// into LDS, builds a 4-ary min-heap on the key and folds the entries as it pops them (no early stop).  A run of more than LV_MLAB_LDS
// entries is appended to longList {pixel address, output index}; k_mlab_resolve_long writes that pixel.  An entry per (tile, pixel)
// pair -- a tile list may repeat or overlap pixels --: longCap = tiles x tile pixels entries (the append is clamped to it as well).
template <int C>
__global__ __launch_bounds__(LV_WAVE) void k_mlab_resolve(const LvUniforms U, const LvTiles T, const uint32_t* __restrict__ frags,
                                                          const uint32_t* __restrict__ startOffset,
                                                          const uint32_t* __restrict__ blockBase,
                                                          const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                          uint32_t numGroups, uint32_t K, uint2* __restrict__ longList,
                                                          uint32_t longCap, LvDevCounters* dc) {
    __shared__ uint32_t s_key[LV_MLAB_LDS][LV_WAVE], s_col[LV_MLAB_LDS][LV_WAVE];
    __shared__ float s_dep[LV_MLAB_LDS][LV_WAVE];
    const uint32_t lane = threadIdx.x;
    uint32_t maxCount = 0u;
    // hole-based sink of a 4-ary min-heap on the key (keys are unique within a pixel)
    auto sink = [&](uint32_t x, uint32_t cnt) {
        const uint32_t k = s_key[x][lane], c = s_col[x][lane];
        const float dd = s_dep[x][lane];
        for (;;) {
            const uint32_t t = 4u * x + 1u;
            if (t >= cnt) break;
            uint32_t best = t, bk = s_key[t][lane];
            for (uint32_t u = 1u; u < 4u; u++)
                if (t + u < cnt && s_key[t + u][lane] < bk) { best = t + u; bk = s_key[t + u][lane]; }
            if (k < bk) break;
            s_key[x][lane] = bk; s_col[x][lane] = s_col[best][lane]; s_dep[x][lane] = s_dep[best][lane];
            x = best;
        }
        s_key[x][lane] = k; s_col[x][lane] = c; s_dep[x][lane] = dd;
    };
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
        const bool inView = inTile && x < U.width && y < U.height;
        bool write = inTile;
        LvMlabNodes<C> L;
        L.clear();
        if (inView) {
            const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            const uint32_t v = fragCount[addr];
            const uint32_t n = v & 0xFFFFu;   // entries of the run; v >> 16 of them are dead
            maxCount = max(maxCount, n - (v >> 16));
            if (n > LV_MLAB_LDS) {
                const uint32_t item = atomicAdd(&dc->mlabLongPixels, 1u);
                if (item < longCap) longList[item] = make_uint2(addr, outIndex);
                write = false;
            } else {
                const uint32_t* __restrict__ run = frags + 3 * size_t(lv_mlab_run_start(startOffset, blockBase, addr));
                uint32_t m = 0u;
                for (uint32_t j = 0u; j < n; j++) {
                    const uint32_t key = run[3 * j + 2];
                    if (key == LV_MLAB_NO_KEY) continue;
                    s_key[m][lane] = key;
                    s_col[m][lane] = run[3 * j + 0];
                    s_dep[m][lane] = __uint_as_float(run[3 * j + 1]);
                    m++;
                }
                for (uint32_t i = m > 1u ? (m - 2u) / 4u + 1u : 0u; i > 0u; --i) sink(i - 1u, m);
                for (uint32_t left = m; left > 0u; --left) {
                    L.insert(s_dep[0][lane], s_col[0][lane], K);
                    if (left > 1u) {
                        s_key[0][lane] = s_key[left - 1u][lane];
                        s_col[0][lane] = s_col[left - 1u][lane];
                        s_dep[0][lane] = s_dep[left - 1u][lane];
                        sink(0u, left - 1u);
                    }
                }
            }
        }
        const uint32_t packed = L.resolve(U, K);
        if (write) out[outIndex] = packed;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
    if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
}

// The pixels k_mlab_resolve listed, one workgroup each (persistent grid).  Ranking: the rank of a live entry is the number of live
// keys below its key (dead entries carry LV_MLAB_NO_KEY, above every key), counted against LDS tiles of the run's keys; entry j
// goes to scratch[run start + rank] -- every entry of the run is read, none is skipped, whatever the run's length.  Then the
// workgroup stages the ordered run through LDS and one lane folds it.
template <int C>
__global__ __launch_bounds__(LV_MLAB_LONG_BLOCK) void k_mlab_resolve_long(const LvUniforms U, const uint32_t* __restrict__ frags,
                                                                         const uint32_t* __restrict__ startOffset,
                                                                         const uint32_t* __restrict__ blockBase,
                                                                         const uint32_t* __restrict__ fragCount,
                                                                         uint32_t* __restrict__ out, uint32_t K,
                                                                         const uint2* __restrict__ longList, uint32_t longCap,
                                                                         uint2* __restrict__ scratch, const LvDevCounters* dc) {
    __shared__ uint32_t s_tile[LV_MLAB_LONG_TILE];
    __shared__ uint2 s_ordered[LV_MLAB_LONG_BLOCK];
    const uint32_t tid = threadIdx.x, count = min(dc->mlabLongPixels, longCap);
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint2 li = longList[item];
        const uint32_t addr = li.x, outIndex = li.y;
        const uint32_t start = lv_mlab_run_start(startOffset, blockBase, addr);
        const uint32_t v = fragCount[addr], n = v & 0xFFFFu, live = n - (v >> 16);
        const uint32_t* __restrict__ run = frags + 3 * size_t(start);
        for (uint32_t b = 0u; b < n; b += 4u * LV_MLAB_LONG_BLOCK) {
            uint32_t key[4], rank[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t j = b + uint32_t(e) * LV_MLAB_LONG_BLOCK + tid;
                key[e] = j < n ? run[3 * size_t(j) + 2] : LV_MLAB_NO_KEY;
            }
            for (uint32_t t0 = 0u; t0 < n; t0 += LV_MLAB_LONG_TILE) {
                __syncthreads();
                for (uint32_t i = tid; i < LV_MLAB_LONG_TILE; i += LV_MLAB_LONG_BLOCK)
                    s_tile[i] = t0 + i < n ? run[3 * size_t(t0 + i) + 2] : LV_MLAB_NO_KEY;
                __syncthreads();
                const uint32_t m = min(LV_MLAB_LONG_TILE, n - t0);
                for (uint32_t i = 0u; i < m; i++) {
                    const uint32_t k = s_tile[i];
#pragma unroll
                    for (int e = 0; e < 4; e++) rank[e] += k < key[e] ? 1u : 0u;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t j = b + uint32_t(e) * LV_MLAB_LONG_BLOCK + tid;
                if (key[e] != LV_MLAB_NO_KEY && rank[e] < live)
                    scratch[size_t(start) + rank[e]] = make_uint2(run[3 * size_t(j) + 0], run[3 * size_t(j) + 1]);
            }
        }
        __syncthreads();
        LvMlabNodes<C> L;
        L.clear();
        for (uint32_t b = 0u; b < live; b += LV_MLAB_LONG_BLOCK) {
            if (b + tid < live) s_ordered[tid] = scratch[size_t(start) + b + tid];
            __syncthreads();
            if (tid == 0u) {
                const uint32_t m = min(LV_MLAB_LONG_BLOCK, live - b);
                for (uint32_t i = 0u; i < m; i++) L.insert(__uint_as_float(s_ordered[i].y), s_ordered[i].x, K);
            }
            __syncthreads();
        }
        if (tid == 0u) out[outIndex] = L.resolve(U, K);
    }
}

// Frames of mode 3: 1 in dc->mlabSaturated when a pixel's 16-bit record count saturated (the rasteriser then drops its fragments)
__global__ __launch_bounds__(LV_BLOCK) void k_mlab_check_counts(const uint4* __restrict__ fragCount, size_t n4, LvDevCounters* dc) {
    const size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i >= n4) return;
    const uint4 v = fragCount[i];
    const bool full = (v.x & 0xFFFFu) == 0xFFFFu || (v.y & 0xFFFFu) == 0xFFFFu || (v.z & 0xFFFFu) == 0xFFFFu || (v.w & 0xFFFFu) == 0xFFFFu;
    if (full) atomicOr(&dc->mlabSaturated, 1u);
}

// ================================================================ MBOIT (rendering mode 6)
// Moment-based order-independent transparency [Muenstermann et al. 2018] as MBOITRenderer runs it with power moments stored as
// float32 (4 / 6 / 8 of them): the fragment stage (k_ppll_shade_prism<..., LV_ENTRY_MBOIT>) leaves each pixel's fragments as one
// contiguous run -- straight float32 colour in a 16-B array, view depth in a 4-B array behind it --, and one kernel sweeps a run
// twice: moments (generateMoments), then per fragment the reconstructed transmittance and the weighted colour sums
// (resolveMoments + MBOITPass2), then the blend (MBOITBlend).  A pixel's moments live in registers between the sweeps: no moment
// image, no atomics on memory, no ordering.  Every sum is a sum of 64-bit fixed-point terms (lv_mboit.h), so the frame does not
// depend on the order the rasteriser left the fragments in.  Short runs: one lane per pixel (k_mboit_resolve); runs of more than
// LV_MBOIT_LONG entries: one wave per pixel, the lanes striding over the run and the integer sums reduced over the wave
// (k_mboit_resolve_long), listed as k_mlab_resolve lists its long pixels.
#ifndef LV_MBOIT_LONG
#define LV_MBOIT_LONG 32u   // config 4, resolve of N = 4: 0.327 / 0.172 / 0.181 / 0.270 ms at 16 / 32 / 48 / 128
#endif

// a run of n entries, this lane taking first, first + step, ...; WAVE: the 64 lanes share the run (sums reduced over the wave, every
// lane returns the pixel).  mom (nullable): b_0 and the normalised moments of the pixel, zeros under the threshold.
template <int N, bool WAVE>
__device__ __forceinline__ uint32_t lv_mboit_run(const LvUniforms& U, const LvMboitParams& M, const uint4* __restrict__ rgba,
                                                 const uint32_t* __restrict__ zbits, uint32_t n, uint32_t first, uint32_t step,
                                                 float* __restrict__ mom, uint32_t& degenerate) {
    long long s[1 + N];
#pragma unroll
    for (int k = 0; k <= N; k++) s[k] = 0;
    for (uint32_t j = first; j < n; j += step) {
        const uint32_t zb = zbits[j];
        if (zb == LV_PPLL_DEAD) continue;
        lv_mboit_moments<N>(__uint_as_float(rgba[j].w), __uint_as_float(zb), M, s);
    }
    if (WAVE) {
#pragma unroll
        for (int k = 0; k <= N; k++) s[k] = (long long)lv_wave_sum_u64((unsigned long long)s[k]);
    }
    float b_0, nb[N];
    LvMboitPixel<N> X;
    const bool covered = lv_mboit_pixel<N>(s, M, b_0, nb, X);
    if (mom && first == 0u) {
        mom[0] = covered ? b_0 : 0.0f;
#pragma unroll
        for (int k = 0; k < N; k++) mom[1 + k] = covered ? nb[k] : 0.0f;
    }
    long long c[4] = {0, 0, 0, 0};
    if (covered) {
        for (uint32_t j = first; j < n; j += step) {
            const uint32_t zb = zbits[j];
            if (zb == LV_PPLL_DEAD) continue;
            const uint4 q = rgba[j];
            f4 col;
            col.x = __uint_as_float(q.x); col.y = __uint_as_float(q.y); col.z = __uint_as_float(q.z); col.w = __uint_as_float(q.w);
            lv_mboit_colour<N>(col, __uint_as_float(zb), b_0, X, M, c);
        }
        if (WAVE) {
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = (long long)lv_wave_sum_u64((unsigned long long)c[k]);
        }
        if (c[3] == 0 && first == 0u) degenerate++;
    }
    return lv_mboit_blend(U, covered, b_0, c);
}

// One lane per pixel, one wave per workgroup, the cells and groups of k_ppll_resolve / k_mlab_resolve.  rgba / zbits: the colour and
// the view-depth array, indexed alike.  Long runs go to longList {pixel address, output index}: one entry per (tile, pixel) pair,
// longCap = tiles x tile pixels.  moments (nullable): (1 + N) floats per output index.
template <int N>
__global__ __launch_bounds__(LV_WAVE) void k_mboit_resolve(const LvUniforms U, const LvTiles T, const LvMboitParams M,
                                                           const uint4* __restrict__ rgba, const uint32_t* __restrict__ zbits,
                                                           const uint32_t* __restrict__ startOffset,
                                                           const uint32_t* __restrict__ blockBase,
                                                           const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                           uint32_t numGroups, uint2* __restrict__ longList, uint32_t longCap,
                                                           float* __restrict__ moments, LvDevCounters* dc) {
    const uint32_t lane = threadIdx.x;
    uint32_t maxCount = 0u, degenerate = 0u;
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
        const bool inView = inTile && x < U.width && y < U.height;
        bool write = inTile;
        uint32_t n = 0u, start = 0u;
        if (inView) {
            const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            const uint32_t v = fragCount[addr];
            n = v & 0xFFFFu;   // entries of the run; v >> 16 of them are dead
            maxCount = max(maxCount, n - (v >> 16));
            if (n > LV_MBOIT_LONG) {
                const uint32_t item = atomicAdd(&dc->mlabLongPixels, 1u);
                if (item < longCap) longList[item] = make_uint2(addr, outIndex);
                write = false;
                n = 0u;
            } else if (n) {
                start = lv_mlab_run_start(startOffset, blockBase, addr);
            }
        }
        float* mom = (moments && write) ? moments + size_t(outIndex) * (1 + N) : nullptr;
        const uint32_t packed = lv_mboit_run<N, false>(U, M, rgba + start, zbits + start, n, 0u, 1u, mom, degenerate);
        if (write) out[outIndex] = packed;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
        degenerate += (uint32_t)__shfl_xor(degenerate, ofs, 64);
    }
    if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
    if (M.stats && lane == 0 && degenerate > 0u) atomicAdd(&dc->mboitDegenerate, degenerate);
}

// The pixels k_mboit_resolve listed, one wave each (persistent grid)
template <int N>
__global__ __launch_bounds__(LV_WAVE) void k_mboit_resolve_long(const LvUniforms U, const LvMboitParams M, const uint4* __restrict__ rgba,
                                                                const uint32_t* __restrict__ zbits,
                                                                const uint32_t* __restrict__ startOffset,
                                                                const uint32_t* __restrict__ blockBase,
                                                                const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                                const uint2* __restrict__ longList, uint32_t longCap,
                                                                float* __restrict__ moments, LvDevCounters* dc) {
    const uint32_t lane = threadIdx.x, count = min(dc->mlabLongPixels, longCap);
    uint32_t degenerate = 0u;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint2 li = longList[item];
        const uint32_t start = lv_mlab_run_start(startOffset, blockBase, li.x);
        const uint32_t n = fragCount[li.x] & 0xFFFFu;
        float* mom = moments ? moments + size_t(li.y) * (1 + N) : nullptr;
        const uint32_t packed = lv_mboit_run<N, true>(U, M, rgba + start, zbits + start, n, lane, LV_WAVE, mom, degenerate);
        if (lane == 0u) out[li.y] = packed;
    }
    if (M.stats && lane == 0u && degenerate > 0u) atomicAdd(&dc->mboitDegenerate, degenerate);
}

// the box of the line points for computeDepthRange (MBOITRenderer.cpp:485): six ordered maxima (the minima as maxima of -x)
__global__ __launch_bounds__(LV_BLOCK) void k_mboit_points_box(const lv_line_point* __restrict__ points, uint32_t numPoints, LvDevCounters* dc) {
    float v[6] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x; i < numPoints; i += gridDim.x * LV_BLOCK) {
        const float* p = points[i].linePosition;
#pragma unroll
        for (int k = 0; k < 3; k++) { v[k] = fmaxf(v[k], -p[k]); v[3 + k] = fmaxf(v[3 + k], p[k]); }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        v[k] = lv_wave_max(v[k]);
        if (lv_lane() == 0) atomicMax(&dc->mboitBoxOrd[k], lv_f2ord(v[k]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mboit_fragment_storage = streamed: mode 6 without a fragment pool.  As the reference's MBOITRenderer the frame draws the geometry
// twice and accumulates with atomics -- here 64-bit integer atomics on the fixed-point terms of lv_mboit.h, so every sum is the sum
// the pooled sweeps form and the frame equals the pooled one byte for byte.  Per padded pixel (addressed like ppllCount) the
// accumulators hold 1 + N moment sums and 4 colour sums of 8 bytes each; ppllCount is the full 32-bit count of kept fragments.
//   k_mboit_stream_pass   the segment rasteriser (stages A and B of k_ppll_raster_prism, same work list and requested-pixel mask)
//                         and the fragment stage in one launch: covered triangles go to a second wave-local LDS queue as
//                         (pixel, leaf | triangle << 26) and stage C shades 64 of them at a time, one lane each, exactly as
//                         k_ppll_shade_prism<..., LV_ENTRY_MBOIT> does.  colourPass = 0: the fragment's moment terms (and 1 on the
//                         pixel's count); colourPass = 1: the pixel's moment sums are complete, the fragment adds its colour terms.
//   k_mboit_stream_blend  the cells and groups of k_mboit_resolve over the frame's tile list: lv_mboit_blend, the degenerate-pixel
//                         counter, the maximum count and the overflow flag (a count above LV_MBOIT_STREAM_MAX_COUNT)
// The sums are exact while |sum| < 2^63: terms saturate at 1024 * 2^36 = 2^46, so for up to 2^17 - 1 kept fragments per pixel.
#define LV_MBOIT_STREAM_MAX_COUNT 131071u
#ifndef LV_MBOIT_STREAM_MIN_WAVES
#define LV_MBOIT_STREAM_MIN_WAVES 2   // the fragment stage alone holds 164 VGPRs (LV_PRISM_SHADE_MIN_WAVES)
#endif
#define LV_MBOIT_STREAM_QUEUE 128u   // fragments a wave holds between stages B and C (>= 2 * LV_WAVE, power of two)

template <int N>
__device__ __forceinline__ void lv_mboit_stream_moments(unsigned long long* a, float alpha, float viewDepth, const LvMboitParams& M) {
    long long s[1 + N];
#pragma unroll
    for (int k = 0; k <= N; k++) s[k] = 0;
    lv_mboit_moments<N>(alpha, viewDepth, M, s);
#pragma unroll
    for (int k = 0; k <= N; k++)
        if (s[k] != 0) atomicAdd(a + k, (unsigned long long)s[k]);
}
template <int N>
__device__ __forceinline__ void lv_mboit_stream_colour(unsigned long long* a, const f4& color, float viewDepth, const LvMboitParams& M) {
    long long s[1 + N];
#pragma unroll
    for (int k = 0; k <= N; k++) s[k] = (long long)a[k];   // complete: the moments launch has finished
    float b_0, nb[N];
    LvMboitPixel<N> X;
    if (!lv_mboit_pixel<N>(s, M, b_0, nb, X)) return;
    long long c[4] = {0, 0, 0, 0};
    lv_mboit_colour<N>(color, viewDepth, b_0, X, M, c);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (c[k] != 0) atomicAdd(a + 1 + N + k, (unsigned long long)c[k]);
}

template <int NT, int SHADE, int FAST>
__global__ __launch_bounds__(LV_BLOCK, LV_MBOIT_STREAM_MIN_WAVES) void k_mboit_stream_pass(const LvUniforms U, const LvSceneDev S,
                                                                   const LvMboitParams M, const uint32_t* __restrict__ startOffset,
                                                                   uint32_t* __restrict__ fragCount, unsigned long long* acc,
                                                                   LvDevCounters* dc, uint32_t allRequested,
                                                                   const uint32_t* __restrict__ leafList, uint32_t numMoments,
                                                                   uint32_t colourPass) {
    __shared__ uint32_t s_qLeaf[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE], s_qPix[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE];
    __shared__ uint32_t s_fFrag[LV_BLOCK / LV_WAVE][LV_MBOIT_STREAM_QUEUE], s_fPix[LV_BLOCK / LV_WAVE][LV_MBOIT_STREAM_QUEUE];
    __shared__ float s_seg[LV_BLOCK / LV_WAVE][20][LV_WAVE];
    __shared__ float s_prismRing[4 * LV_PRISM_MAX_SUBDIV];
    // what stages A and B keep per lane, parked here while stage C runs: the fragment stage needs the registers (with them live
    // across it the kernel spilled to scratch at two waves per SIMD)
    __shared__ uint32_t s_park[19][LV_BLOCK];
    if (threadIdx.x < LV_PRISM_MAX_SUBDIV) {
        s_prismRing[threadIdx.x] = S.prism.c[threadIdx.x];
        s_prismRing[LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.s[threadIdx.x];
        s_prismRing[2 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.cp[threadIdx.x];
        s_prismRing[3 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.sn[threadIdx.x];
    }
    __syncthreads();
    const LvPrismDev& R = S.prism;
    const uint32_t N = NT > 0 ? uint32_t(NT) : R.n;
    const unsigned lane = lv_lane();
    uint32_t* qLeaf = s_qLeaf[threadIdx.x >> 6];
    uint32_t* qPix = s_qPix[threadIdx.x >> 6];
    uint32_t* fFrag = s_fFrag[threadIdx.x >> 6];
    uint32_t* fPix = s_fPix[threadIdx.x >> 6];
    float (*segLds)[LV_WAVE] = s_seg[threadIdx.x >> 6];
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    float mx[4], my[4], mw[4];
    lv_clip_rows(U, mx, my, mw);
    const float halfW = 0.5f * float(U.width), halfH = 0.5f * float(U.height);
    const float wEps = 1e-3f * U.nearDist;
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u);
    const size_t accStride = 1u + numMoments + 4u;
    const bool count = colourPass == 0u, stats = M.stats != 0u && count;   // the statistics are the moments launch's
    unsigned qHead = 0u, qCount = 0u;   // (pixel, segment) pairs (wave-uniform)
    unsigned fHead = 0u, fCount = 0u;   // covered triangles (wave-uniform)
    unsigned long long tests = 0, hits = 0;
    uint32_t keptSum = 0u;
    // stage A's walk over the lane's segment: candidate rectangle and oriented box, position in it
    uint32_t leafA = 0u;
    LvSegWalk w = {};
    int px = 0, py = 0;
    bool more = false;

    // stage C on the m <= 64 oldest fragments of the queue.  (Both stages are lambdas with ONE call site each: a second site keeps
    // the compiler from inlining them, and their by-reference captures -- U and S among them -- then live in scratch.)
    auto fragmentStage = [&](unsigned m) __attribute__((always_inline)) {
        if (lane < m) {
            const unsigned q = (fHead + lane) & (LV_MBOIT_STREAM_QUEUE - 1u);
            const uint32_t w0 = fPix[q], w1 = fFrag[q];
            const uint32_t px = w0 & 0xFFFFu, py = w0 >> 16;
            const uint32_t leaf = w1 & 0x03FFFFFFu, tt = w1 >> 26;
            const float aoTexel = (U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(py) * U.width + px] : 1.0f;
            f3 oo, d;
            lv_primary_ray(U, px, py, 0.5f, 0.5f, oo, d);
            const LvRasterQuad rq = lv_make_raster_quad(U, px, py);
            bool kept;
            float depth;
            const f4 color = lv_shade_prism<SHADE, FAST>(S, U, s_prismRing, aoTexel, o, d, tLo, tHi, leaf, tt, rq, U.ppllRasterColour != 0u, depth, kept);
            if (kept) {   // (only the `kept` rules discard in mode 6)
                const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
                const float z = lv_view_depth(U, lv_prism_frag_pos(S, U, s_prismRing, d, leaf, tt));
                unsigned long long* a = acc + size_t(addr) * accStride;
                if (count) {
                    if (numMoments == 4u) lv_mboit_stream_moments<4>(a, color.w, z, M);
                    else if (numMoments == 6u) lv_mboit_stream_moments<6>(a, color.w, z, M);
                    else lv_mboit_stream_moments<8>(a, color.w, z, M);
                    atomicAdd(&fragCount[addr], 1u);
                    keptSum++;
                    if (stats) hits++;
                } else {
                    if (numMoments == 4u) lv_mboit_stream_colour<4>(a, color, z, M);
                    else if (numMoments == 6u) lv_mboit_stream_colour<6>(a, color, z, M);
                    else lv_mboit_stream_colour<8>(a, color, z, M);
                }
            }
        }
        fHead = (fHead + m) & (LV_MBOIT_STREAM_QUEUE - 1u);
        fCount -= m;
    };

    // stage B on the m <= 64 oldest pairs of the queue (k_ppll_raster_prism's, the covered triangles queued instead of recorded);
    // flush: the wave's last batch -- stage C also takes what is left in its queue
    auto coverageStage = [&](unsigned m, bool flush) __attribute__((always_inline)) {
        unsigned mask = 0u;
        uint32_t leaf = 0u, pix = 0u;
        if (lane < m) {
            mask = lv_seg_pair_coverage<NT>(R, segLds, qLeaf, qPix, (qHead + lane) & (LV_PRISM_RASTER_QUEUE - 1u), o, leaf, pix);
            if (stats) tests++;
        }
        while (true) {
            const bool hit = mask != 0u;
            const unsigned long long hm = __ballot(hit);
            if (hm == 0ull && !(flush && fCount > 0u)) break;
            if (hit) {
                const unsigned tt = unsigned(__ffs(int(mask))) - 1u;
                mask &= mask - 1u;
                const unsigned q = (fHead + fCount + unsigned(__popcll(hm & ((1ull << lane) - 1ull)))) & (LV_MBOIT_STREAM_QUEUE - 1u);
                fPix[q] = pix;
                fFrag[q] = leaf | (tt << 26);
            }
            fCount += unsigned(__popcll(hm));
            if (fCount >= LV_WAVE || hm == 0ull) {
                uint32_t* park = &s_park[0][threadIdx.x];
                const float pf[8] = {w.ax, w.ay, w.cx0, w.cy0, w.aMid, w.aHalf, w.nMid, w.nHalf};
                const uint32_t pu[11] = {mask, leaf, pix, leafA, uint32_t(w.x0), uint32_t(w.x1), uint32_t(w.y0), uint32_t(w.y1),
                                         uint32_t(px), uint32_t(py), more ? 1u : 0u};
#pragma unroll
                for (int i = 0; i < 8; i++) park[i * LV_BLOCK] = __float_as_uint(pf[i]);
#pragma unroll
                for (int i = 0; i < 11; i++) park[(8 + i) * LV_BLOCK] = pu[i];
                fragmentStage(fCount < LV_WAVE ? fCount : LV_WAVE);
                w.ax = __uint_as_float(park[0]); w.ay = __uint_as_float(park[LV_BLOCK]); w.cx0 = __uint_as_float(park[2 * LV_BLOCK]);
                w.cy0 = __uint_as_float(park[3 * LV_BLOCK]); w.aMid = __uint_as_float(park[4 * LV_BLOCK]); w.aHalf = __uint_as_float(park[5 * LV_BLOCK]);
                w.nMid = __uint_as_float(park[6 * LV_BLOCK]); w.nHalf = __uint_as_float(park[7 * LV_BLOCK]);
                mask = park[8 * LV_BLOCK]; leaf = park[9 * LV_BLOCK]; pix = park[10 * LV_BLOCK]; leafA = park[11 * LV_BLOCK];
                w.x0 = int(park[12 * LV_BLOCK]); w.x1 = int(park[13 * LV_BLOCK]); w.y0 = int(park[14 * LV_BLOCK]); w.y1 = int(park[15 * LV_BLOCK]);
                px = int(park[16 * LV_BLOCK]); py = int(park[17 * LV_BLOCK]); more = park[18 * LV_BLOCK] != 0u;
            }
        }
        qHead = (qHead + m) & (LV_PRISM_RASTER_QUEUE - 1u);
        qCount -= m;
    };

    const uint32_t waveId = blockIdx.x * (LV_BLOCK / LV_WAVE) + (threadIdx.x >> 6), numWaves = gridDim.x * (LV_BLOCK / LV_WAVE);
    const uint32_t numItems = leafList ? dc->prismListCount : S.numSegs;
    for (uint32_t itemBase = waveId * LV_WAVE; itemBase < numItems; itemBase += numWaves * LV_WAVE) {
        const bool valid = itemBase + lane < numItems;
        const uint32_t leaf = !valid ? 0u : (leafList ? leafList[itemBase + lane] : itemBase + lane);
        leafA = leaf;
        w = lv_seg_walk_setup(U, S, segLds, mx, my, mw, halfW, halfH, wEps, N, valid, leaf, lane);
        px = w.x0; py = w.y0;
        more = valid && w.x1 >= w.x0 && w.y1 >= w.y0;
        const bool lastItem = itemBase + numWaves * LV_WAVE >= numItems;   // (overflow: numItems < 2^26)
        while (true) {
            const bool drain = !__any(more);   // every rectangle walked: the rest of the pairs, 64 at a time
            const bool cand = more && lv_seg_walk_candidate(U, w, px, py, allRequested, startOffset);
            const unsigned long long cm = __ballot(cand);
            if (cand) {
                const unsigned q = (qHead + qCount + unsigned(__popcll(cm & ((1ull << lane) - 1ull)))) & (LV_PRISM_RASTER_QUEUE - 1u);
                qLeaf[q] = leafA | (lane << 26);
                qPix[q] = uint32_t(px) | (uint32_t(py) << 16);
            }
            qCount += unsigned(__popcll(cm));
            if (qCount >= LV_WAVE || drain) coverageStage(qCount < LV_WAVE ? qCount : LV_WAVE, lastItem && drain && qCount <= LV_WAVE);
            if (drain && qCount == 0u) break;   // (the next 64 segments replace the frames in LDS)
            if (more) more = lv_seg_walk_advance(w, px, py);
        }
    }
    if (count) {
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) keptSum += (uint32_t)__shfl_xor(keptSum, ofs, 64);
        if (lane == 0u && keptSum > 0u) atomicAdd(&dc->fragCounter, keptSum);   // fragCounter of the reference: every kept fragment
    }
    if (stats) {
        tests = lv_wave_sum_u64(tests);
        hits = lv_wave_sum_u64(hits);
        if (lane == 0u && tests) atomicAdd(&dc->prims, tests);
        if (lane == 0u && hits) atomicAdd(&dc->hits, hits);
    }
}

// One lane per pixel, one wave per workgroup, the cells and groups of k_mboit_resolve
__global__ __launch_bounds__(LV_WAVE) void k_mboit_stream_blend(const LvUniforms U, const LvTiles T, const LvMboitParams M,
                                                                const unsigned long long* __restrict__ acc,
                                                                const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                                uint32_t numGroups, uint32_t numMoments, LvDevCounters* dc) {
    const uint32_t lane = threadIdx.x;
    uint32_t maxCount = 0u, degenerate = 0u;
    const size_t accStride = 1u + numMoments + 4u;
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
        long long c[4] = {0, 0, 0, 0};
        float b_0 = 0.0f;
        if (inTile && x < U.width && y < U.height) {
            const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            maxCount = max(maxCount, fragCount[addr]);
            const unsigned long long* a = acc + size_t(addr) * accStride;
            b_0 = lv_mboit_unfixed((long long)a[0]);
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = (long long)a[1u + numMoments + k];
        }
        const bool covered = !(b_0 < LV_MBOIT_B0_MIN);   // lv_mboit_pixel's threshold
        if (covered && c[3] == 0) degenerate++;
        const uint32_t packed = lv_mboit_blend(U, covered, b_0, c);
        if (inTile) out[outIndex] = packed;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
        degenerate += (uint32_t)__shfl_xor(degenerate, ofs, 64);
    }
    if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
    if (lane == 0 && maxCount > LV_MBOIT_STREAM_MAX_COUNT) atomicOr(&dc->mboitOverflow, 1u);
    if (M.stats && lane == 0 && degenerate > 0u) atomicAdd(&dc->mboitDegenerate, degenerate);
}

// lv_mboit_get_moments: b_0 and the normalised b_1 ... b_N of every pixel of the viewport, row-major, zeros under the threshold
// (the expressions of lv_mboit_pixel on the frame's moment sums)
__global__ __launch_bounds__(LV_BLOCK) void k_mboit_stream_moments(const unsigned long long* __restrict__ acc, uint32_t width,
                                                                  uint32_t height, uint32_t paddedW, uint32_t tileW, uint32_t tileH,
                                                                  uint32_t numMoments, float* __restrict__ out) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p >= size_t(width) * height) return;
    const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
    const unsigned long long* a = acc + size_t(lv_ppll_addr(x, y, paddedW, tileW, tileH)) * (1u + numMoments + 4u);
    float* o = out + p * (1u + numMoments);
    const float b_0 = lv_mboit_unfixed((long long)a[0]);
    const bool covered = !(b_0 < LV_MBOIT_B0_MIN);
    o[0] = covered ? b_0 : 0.0f;
    for (uint32_t k = 0; k < numMoments; k++) o[1u + k] = covered ? lv_mboit_unfixed((long long)a[1u + k]) / b_0 : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The streamed fragment pass of modes 8 and 10: ONE launch per frame, no fragment pool.
//   k_stream_pass   the skeleton: stage A walks the wave's 64 segments and queues (pixel, segment) pairs in LDS, stage B tests 64 pairs
//                   at a time (lv_seg_walk_* / lv_seg_pair_coverage, as k_ppll_raster_prism) and queues the covered triangles in a
//                   second LDS queue, stage C shades 64 of them, one lane per fragment, while the 19 words stages A and B keep per lane
//                   are parked in LDS.  A mode supplies the meaning of `buf` and `arg` and two pieces of stage C: the fragment's
//                   store, and the two lines that count kept and stored fragments.
//                     MODE = LV_RENDERING_MODE_ATOMIC_LOOP_64   buf: (K + 5) words per pixel, arg: K, store: lv_al64_insert
//                     MODE = LV_RENDERING_MODE_WBOIT            buf: 5 sums per pixel, arg: the weight mode, store: lv_wboit_add
// It is a single __global__ template with the mode's text under `if constexpr`, not an inlined helper: with the body as a
// __forceinline__ device function that takes stage C as a lambda, every instance gained 20 to 30 VGPRs (mode 10's
// <0, 1, 0> instance reached 256 and spilled); as a __forceinline__ function template on the mode behind two thin kernels every instance
// still changed by a few dozen instructions.  This shape compiles every instance to the instructions of the two kernels it
// replaces (tools/isa_report.py --compare; EXPERIMENTS.md).
// k_mboit_stream_pass is not an instance.  Joining it would take:
//   - LvMboitParams out of the kernel's signature, and its two launches per frame (count / colour) expressed as modes;
//   - its per-lane counters with wave reductions at the end replaced by the per-wave ballot counts below;
//   - the scalarised wave index and uniform() constants, which change its code at the edge of its register budget.
template <int MODE, int NT, int SHADE, int FAST>
__global__ __launch_bounds__(LV_BLOCK, LV_MBOIT_STREAM_MIN_WAVES) void k_stream_pass(const LvUniforms U, const LvSceneDev S,
                                                                   const uint32_t* __restrict__ startOffset,
                                                                   uint32_t* __restrict__ fragCount, unsigned long long* buf,
                                                                   LvDevCounters* dc, uint32_t allRequested,
                                                                   const uint32_t* __restrict__ leafList, uint32_t arg,
                                                                   uint32_t collectStats) {
    static_assert(MODE == LV_RENDERING_MODE_ATOMIC_LOOP_64 || MODE == LV_RENDERING_MODE_WBOIT, "k_stream_pass: no stage C for this mode");
    __shared__ uint32_t s_qLeaf[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE], s_qPix[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE];
    __shared__ uint32_t s_fFrag[LV_BLOCK / LV_WAVE][LV_MBOIT_STREAM_QUEUE], s_fPix[LV_BLOCK / LV_WAVE][LV_MBOIT_STREAM_QUEUE];
    __shared__ float s_seg[LV_BLOCK / LV_WAVE][20][LV_WAVE];
    __shared__ float s_prismRing[4 * LV_PRISM_MAX_SUBDIV];
    // what stages A and B keep per lane, parked here while stage C runs (as k_mboit_stream_pass, for the registers of stage C)
    __shared__ uint32_t s_park[19][LV_BLOCK];
    if (threadIdx.x < LV_PRISM_MAX_SUBDIV) {
        s_prismRing[threadIdx.x] = S.prism.c[threadIdx.x];
        s_prismRing[LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.s[threadIdx.x];
        s_prismRing[2 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.cp[threadIdx.x];
        s_prismRing[3 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.sn[threadIdx.x];
    }
    __syncthreads();
    const LvPrismDev& R = S.prism;
    const uint32_t N = NT > 0 ? uint32_t(NT) : R.n;
    const unsigned lane = lv_lane();
    // (the wave's index as a scalar: the five LDS bases and the item counter below then hold no vector registers either)
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* qLeaf = s_qLeaf[wave];
    uint32_t* qPix = s_qPix[wave];
    uint32_t* fFrag = s_fFrag[wave];
    uint32_t* fPix = s_fPix[wave];
    float (*segLds)[LV_WAVE] = s_seg[wave];
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    // the frame's set-up constants are the same in every lane: kept in scalar registers, so that the 15 of them do not hold vector
    // registers across stage C
    auto uniform = [](float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); };
    float mx[4], my[4], mw[4];
    lv_clip_rows(U, mx, my, mw);
#pragma unroll
    for (int c = 0; c < 4; c++) { mx[c] = uniform(mx[c]); my[c] = uniform(my[c]); mw[c] = uniform(mw[c]); }
    const float halfW = uniform(0.5f * float(U.width)), halfH = uniform(0.5f * float(U.height));
    const float wEps = uniform(1e-3f * U.nearDist);
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u);
    [[maybe_unused]] const size_t stride = size_t(arg) + LV_AL64_TAIL;   // mode 10: words per pixel (here, not in stage C: there its instances compile differently)
    const bool stats = collectStats != 0u;
    unsigned qHead = 0u, qCount = 0u;   // (pixel, segment) pairs (wave-uniform)
    unsigned fHead = 0u, fCount = 0u;   // covered triangles (wave-uniform)
    // the frame's counters, per wave (ballots: wave-uniform values need no vector registers across the stages)
    unsigned long long tests = 0, hits = 0;
    uint32_t keptSum = 0u;
    // stage A's walk over the lane's segment: candidate rectangle and oriented box, position in it
    uint32_t leafA = 0u;
    LvSegWalk w = {};
    int px = 0, py = 0;
    bool more = false;

    // stage C on the m <= 64 oldest fragments of the queue, shaded as k_ppll_shade_prism shades them, with the window depth of mode 3.
    //   mode 10: the `kept` rules, then the gather's discard (AtomicLoop64Gather.glsl:56); key = window depth bits << 32 |
    //            packUnorm4x8(colour), inserted
    //   mode 8:  only the `kept` rules discard (WBOITGather.glsl has no alpha test); the five terms added
    // (One call site, as in k_mboit_stream_pass.)
    auto fragmentStage = [&](unsigned m) __attribute__((always_inline)) {
        bool hit = false;
        [[maybe_unused]] bool stored = false;
        if (lane < m) {
            const unsigned q = (fHead + lane) & (LV_MBOIT_STREAM_QUEUE - 1u);
            const uint32_t w0 = fPix[q], w1 = fFrag[q];
            const uint32_t px = w0 & 0xFFFFu, py = w0 >> 16;
            const uint32_t leaf = w1 & 0x03FFFFFFu, tt = w1 >> 26;
            const float aoTexel = (U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(py) * U.width + px] : 1.0f;
            f3 oo, d;
            lv_primary_ray(U, px, py, 0.5f, 0.5f, oo, d);
            const LvRasterQuad rq = lv_make_raster_quad(U, px, py);
            bool kept;
            float depth;
            const f4 color = lv_shade_prism<SHADE, FAST>(S, U, s_prismRing, aoTexel, o, d, tLo, tHi, leaf, tt, rq, U.ppllRasterColour != 0u, depth, kept);
            hit = kept;
            if constexpr (MODE == LV_RENDERING_MODE_ATOMIC_LOOP_64) {
                if (kept && color.w >= 0.001f) {
                    const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
                    const float z = lv_window_depth(U, lv_prism_frag_pos(S, U, s_prismRing, d, leaf, tt));
                    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | lv_pack_unorm4x8(color);
                    unsigned long long* slots = buf + size_t(addr) * stride;
                    lv_al64_insert(slots, arg, key, slots + arg);
                    atomicAdd(&fragCount[addr], 1u);
                    stored = true;
                }
            } else {
                if (kept) {
                    const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
                    const float z = lv_window_depth(U, lv_prism_frag_pos(S, U, s_prismRing, d, leaf, tt));
                    lv_wboit_add(buf + size_t(addr) * LV_WBOIT_SUMS, color, z, arg);
                    atomicAdd(&fragCount[addr], 1u);
                }
            }
        }
        if constexpr (MODE == LV_RENDERING_MODE_ATOMIC_LOOP_64) {   // every fragment past the discard; hits: every kept one
            keptSum += uint32_t(__popcll(__ballot(stored)));
            if (stats) hits += (unsigned long long)__popcll(__ballot(hit));
        } else {   // every kept fragment
            const uint32_t keptNow = uint32_t(__popcll(__ballot(hit)));
            keptSum += keptNow;
            if (stats) hits += (unsigned long long)keptNow;
        }
        fHead = (fHead + m) & (LV_MBOIT_STREAM_QUEUE - 1u);
        fCount -= m;
    };

    // stage B on the m <= 64 oldest pairs of the queue (k_mboit_stream_pass's: the covered triangles go to the second queue);
    // flush: the wave's last batch -- stage C also takes what is left in its queue
    auto coverageStage = [&](unsigned m, bool flush) __attribute__((always_inline)) {
        unsigned mask = 0u;
        uint32_t leaf = 0u, pix = 0u;
        if (lane < m) {
            mask = lv_seg_pair_coverage<NT>(R, segLds, qLeaf, qPix, (qHead + lane) & (LV_PRISM_RASTER_QUEUE - 1u), o, leaf, pix);
        }
        if (stats) tests += m;
        while (true) {
            const bool hit = mask != 0u;
            const unsigned long long hm = __ballot(hit);
            if (hm == 0ull && !(flush && fCount > 0u)) break;
            if (hit) {
                const unsigned tt = unsigned(__ffs(int(mask))) - 1u;
                mask &= mask - 1u;
                const unsigned q = (fHead + fCount + unsigned(__popcll(hm & ((1ull << lane) - 1ull)))) & (LV_MBOIT_STREAM_QUEUE - 1u);
                fPix[q] = pix;
                fFrag[q] = leaf | (tt << 26);
            }
            fCount += unsigned(__popcll(hm));
            if (fCount >= LV_WAVE || hm == 0ull) {
                uint32_t* park = &s_park[0][threadIdx.x];
                const float pf[8] = {w.ax, w.ay, w.cx0, w.cy0, w.aMid, w.aHalf, w.nMid, w.nHalf};
                const uint32_t pu[11] = {mask, leaf, pix, leafA, uint32_t(w.x0), uint32_t(w.x1), uint32_t(w.y0), uint32_t(w.y1),
                                         uint32_t(px), uint32_t(py), more ? 1u : 0u};
#pragma unroll
                for (int i = 0; i < 8; i++) park[i * LV_BLOCK] = __float_as_uint(pf[i]);
#pragma unroll
                for (int i = 0; i < 11; i++) park[(8 + i) * LV_BLOCK] = pu[i];
                fragmentStage(fCount < LV_WAVE ? fCount : LV_WAVE);
                w.ax = __uint_as_float(park[0]); w.ay = __uint_as_float(park[LV_BLOCK]); w.cx0 = __uint_as_float(park[2 * LV_BLOCK]);
                w.cy0 = __uint_as_float(park[3 * LV_BLOCK]); w.aMid = __uint_as_float(park[4 * LV_BLOCK]); w.aHalf = __uint_as_float(park[5 * LV_BLOCK]);
                w.nMid = __uint_as_float(park[6 * LV_BLOCK]); w.nHalf = __uint_as_float(park[7 * LV_BLOCK]);
                mask = park[8 * LV_BLOCK]; leaf = park[9 * LV_BLOCK]; pix = park[10 * LV_BLOCK]; leafA = park[11 * LV_BLOCK];
                w.x0 = int(park[12 * LV_BLOCK]); w.x1 = int(park[13 * LV_BLOCK]); w.y0 = int(park[14 * LV_BLOCK]); w.y1 = int(park[15 * LV_BLOCK]);
                px = int(park[16 * LV_BLOCK]); py = int(park[17 * LV_BLOCK]); more = park[18 * LV_BLOCK] != 0u;
            }
        }
        qHead = (qHead + m) & (LV_PRISM_RASTER_QUEUE - 1u);
        qCount -= m;
    };

    const uint32_t waveId = blockIdx.x * (LV_BLOCK / LV_WAVE) + wave, numWaves = gridDim.x * (LV_BLOCK / LV_WAVE);
    const uint32_t numItems = leafList ? dc->prismListCount : S.numSegs;
    for (uint32_t itemBase = waveId * LV_WAVE; itemBase < numItems; itemBase += numWaves * LV_WAVE) {
        const bool valid = itemBase + lane < numItems;
        const uint32_t leaf = !valid ? 0u : (leafList ? leafList[itemBase + lane] : itemBase + lane);
        leafA = leaf;
        w = lv_seg_walk_setup(U, S, segLds, mx, my, mw, halfW, halfH, wEps, N, valid, leaf, lane);
        px = w.x0; py = w.y0;
        more = valid && w.x1 >= w.x0 && w.y1 >= w.y0;
        const bool lastItem = itemBase + numWaves * LV_WAVE >= numItems;   // (overflow: numItems < 2^26)
        while (true) {
            const bool drain = !__any(more);   // every rectangle walked: the rest of the pairs, 64 at a time
            const bool cand = more && lv_seg_walk_candidate(U, w, px, py, allRequested, startOffset);
            const unsigned long long cm = __ballot(cand);
            if (cand) {
                const unsigned q = (qHead + qCount + unsigned(__popcll(cm & ((1ull << lane) - 1ull)))) & (LV_PRISM_RASTER_QUEUE - 1u);
                qLeaf[q] = leafA | (lane << 26);
                qPix[q] = uint32_t(px) | (uint32_t(py) << 16);
            }
            qCount += unsigned(__popcll(cm));
            if (qCount >= LV_WAVE || drain) coverageStage(qCount < LV_WAVE ? qCount : LV_WAVE, lastItem && drain && qCount <= LV_WAVE);
            if (drain && qCount == 0u) break;   // (the next 64 segments replace the frames in LDS)
            if (more) more = lv_seg_walk_advance(w, px, py);
        }
    }
    if (lane == 0u && keptSum > 0u) atomicAdd(&dc->fragCounter, keptSum);
    if (stats) {
        if (lane == 0u && tests) atomicAdd(&dc->prims, tests);
        if (lane == 0u && hits) atomicAdd(&dc->hits, hits);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Atomic Loop 64 (rendering mode 10, AtomicLoop64Renderer): the K nearest fragments of every pixel exactly, the rest as a weighted
// average behind them (lv_al64.h).  (K + 5) x 8 B per padded pixel (addressed like ppllCount), no fragment pool, no regrowth, no
// read-back; ppllCount is the 32-bit count of the fragments past the discard.
//   k_stream_pass<10>    (above) with lv_al64_insert as the fragment's store
//   k_al64_resolve       the cells and groups of k_mboit_stream_blend over the frame's tile list: lv_al64_resolve_pixel, the maximum
//                        count and the overflow flag (a count above LV_AL64_MAX_COUNT)
// The buffer is cleared per frame and not by the resolve (as the reference does): a tile list may repeat or overlap pixels.
__global__ __launch_bounds__(LV_BLOCK) void k_al64_clear(unsigned long long* __restrict__ buf, size_t numWords, uint32_t K) {
    const uint32_t stride = K + LV_AL64_TAIL;
    for (size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x; i < numWords; i += size_t(gridDim.x) * LV_BLOCK)
        buf[i] = uint32_t(i % stride) < K ? LV_AL64_EMPTY : 0ull;
}

// One lane per pixel, one wave per workgroup, the cells and groups of k_mboit_stream_blend
__global__ __launch_bounds__(LV_WAVE) void k_al64_resolve(const LvUniforms U, const LvTiles T, const unsigned long long* __restrict__ buf,
                                                          const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                          uint32_t numGroups, uint32_t K, LvDevCounters* dc) {
    const uint32_t lane = threadIdx.x;
    uint32_t maxCount = 0u;
    const size_t stride = size_t(K) + LV_AL64_TAIL;
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
        uint32_t packed;
        if (x < U.width && y < U.height) {
            const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            maxCount = max(maxCount, fragCount[addr]);
            const unsigned long long* slots = buf + size_t(addr) * stride;
            packed = lv_al64_resolve_pixel(U, slots, K, slots + K);
        } else {
            f4 r;
            r.x = U.background[0]; r.y = U.background[1]; r.z = U.background[2]; r.w = U.background[3];
            packed = lv_pack_unorm4x8(r);
        }
        out[outIndex] = packed;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
    if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
    if (lane == 0 && maxCount > LV_AL64_MAX_COUNT) atomicOr(&dc->mboitOverflow, 1u);
}

// lv_atomic_loop_resolve_buffers: one lane per given key, all lanes racing; pixel = the run of `offsets` that holds the key (binary
// search over the numPixels + 1 ascending offsets on the device)
__global__ __launch_bounds__(LV_BLOCK) void k_al64_insert_given(const unsigned long long* __restrict__ keys, uint64_t numKeys,
                                                               const unsigned long long* __restrict__ offsets, uint32_t numPixels,
                                                               unsigned long long* buf, uint32_t* __restrict__ fragCount, uint32_t K) {
    const uint64_t i = uint64_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i >= numKeys) return;
    uint32_t lo = 0u, hi = numPixels;   // the last p in [0, numPixels) with offsets[p] <= i  (offsets[0] = 0, offsets[numPixels] = numKeys > i)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    unsigned long long* slots = buf + size_t(lo) * (size_t(K) + LV_AL64_TAIL);
    lv_al64_insert(slots, K, keys[i], slots + K);
    atomicAdd(&fragCount[lo], 1u);
}

// lv_atomic_loop_get_buffers: the slots and the tail sums of every pixel of the viewport, row-major
__global__ __launch_bounds__(LV_BLOCK) void k_al64_read(const unsigned long long* __restrict__ buf, uint32_t width, uint32_t height,
                                                       uint32_t paddedW, uint32_t tileW, uint32_t tileH, uint32_t K,
                                                       unsigned long long* __restrict__ outSlots, unsigned long long* __restrict__ outTail) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p >= size_t(width) * height) return;
    const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
    const unsigned long long* a = buf + size_t(lv_ppll_addr(x, y, paddedW, tileW, tileH)) * (size_t(K) + LV_AL64_TAIL);
    for (uint32_t i = 0u; i < K; i++) outSlots[p * K + i] = a[i];
    for (uint32_t i = 0u; i < LV_AL64_TAIL; i++) outTail[p * LV_AL64_TAIL + i] = a[K + i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weighted Blended OIT (rendering mode 8, WBOITRenderer): every per-pixel quantity is a sum (lv_wboit.h).  5 x 8 B per padded pixel
// (addressed like ppllCount), no fragment pool, no regrowth, no read-back; ppllCount is the 32-bit count of the kept fragments.
//   k_stream_pass<8>     (above) with lv_wboit_add as the fragment's store
//   k_wboit_resolve      the cells and groups of k_al64_resolve over the frame's tile list: lv_wboit_resolve_pixel, the maximum
//                        count and the overflow flag (a count above LV_WBOIT_MAX_COUNT)
// The sums are zeroed per frame (a memset) and not by the resolve: a tile list may repeat or overlap pixels.

// One lane per pixel, one wave per workgroup, the cells and groups of k_al64_resolve
__global__ __launch_bounds__(LV_WAVE) void k_wboit_resolve(const LvUniforms U, const LvTiles T, const unsigned long long* __restrict__ sums,
                                                           const uint32_t* __restrict__ fragCount, uint32_t* __restrict__ out,
                                                           uint32_t numGroups, LvDevCounters* dc) {
    const uint32_t lane = threadIdx.x;
    uint32_t maxCount = 0u;
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
        uint32_t packed;
        if (x < U.width && y < U.height) {
            const uint32_t addr = lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
            const uint32_t count = fragCount[addr];
            maxCount = max(maxCount, count);
            packed = lv_wboit_resolve_pixel(U, sums + size_t(addr) * LV_WBOIT_SUMS, count);
        } else {
            f4 r;
            r.x = U.background[0]; r.y = U.background[1]; r.z = U.background[2]; r.w = U.background[3];
            packed = lv_pack_unorm4x8(r);
        }
        out[outIndex] = packed;
    }
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) maxCount = max(maxCount, (uint32_t)__shfl_xor(maxCount, ofs, 64));
    if (lane == 0 && maxCount > 0u) atomicMax(&dc->maxDepthComplexity, maxCount);
    if (lane == 0 && maxCount > LV_WBOIT_MAX_COUNT) atomicOr(&dc->mboitOverflow, 1u);
}

// lv_wboit_resolve_buffers: one lane per given fragment {r, g, b, alpha, window depth}, all lanes racing; pixel = the run of `offsets`
// that holds the fragment (binary search over the numPixels + 1 ascending offsets on the device)
__global__ __launch_bounds__(LV_BLOCK) void k_wboit_add_given(const float* __restrict__ entries, uint64_t numEntries,
                                                             const unsigned long long* __restrict__ offsets, uint32_t numPixels,
                                                             unsigned long long* sums, uint32_t* __restrict__ fragCount,
                                                             uint32_t weightMode) {
    const uint64_t i = uint64_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i >= numEntries) return;
    uint32_t lo = 0u, hi = numPixels;   // the last p in [0, numPixels) with offsets[p] <= i  (offsets[0] = 0, offsets[numPixels] = numEntries > i)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const float* e = entries + size_t(i) * 5u;
    f4 color;
    color.x = e[0]; color.y = e[1]; color.z = e[2]; color.w = e[3];
    lv_wboit_add(sums + size_t(lo) * LV_WBOIT_SUMS, color, e[4], weightMode);
    atomicAdd(&fragCount[lo], 1u);
}

// lv_wboit_get_buffers: the five sums and the count of every pixel of the viewport, row-major
__global__ __launch_bounds__(LV_BLOCK) void k_wboit_read(const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ fragCount,
                                                        uint32_t width, uint32_t height, uint32_t paddedW, uint32_t tileW, uint32_t tileH,
                                                        unsigned long long* __restrict__ outSums, uint32_t* __restrict__ outCounts) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p >= size_t(width) * height) return;
    const uint32_t x = uint32_t(p % width), y = uint32_t(p / width);
    const uint32_t addr = lv_ppll_addr(x, y, paddedW, tileW, tileH);
    for (uint32_t i = 0u; i < LV_WBOIT_SUMS; i++) outSums[p * LV_WBOIT_SUMS + i] = sums[size_t(addr) * LV_WBOIT_SUMS + i];
    if (outCounts) outCounts[p] = fragCount[addr];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Depth complexity (rendering mode 5, DepthComplexityRenderer) and depth peeling (rendering mode 9, DepthPeelingRenderer); the rules
// are lv_peel.h's.  Both walk the kept fragments of the rasterised prism WITHOUT shading them: whether a fragment is kept
// (lv_prism_accept) and its window depth need the interpolated position only.
//   k_dc_count_pass   one launch: ppllCount[pixel] += 1 per kept fragment (modes 5 and 9; gatherInc of DepthComplexityGatherInc.glsl)
//   k_dc_reduce       total, used pixels, maximum and minimum of the requested pixels' counts into device words
//   k_dc_resolve      mode 5's frame (the cells and groups of k_wboit_resolve); reads the maximum from device memory
//   k_peel_pass       one launch per layer: 64-bit atomicMin of (z bits << 32 | primitive key) into the pixel's slot
//   k_peel_layer      (lv_peel.hip) one lane per VIEWPORT pixel (a tile list may repeat or overlap pixels; a pixel must be accumulated
//                     once): shades the slot's winner as stage C of k_stream_pass<8> shades, accumulates, resets the slot.  In a file
//                     of its own: as a kernel of this one it changed the code of every kernel here that calls lv_shade_prism and
//                     lv_prism_frag_pos (38 instances), which must compile as they do
//   k_peel_blit       the accumulator over the clear colour, over the tile list's cells (a pure read)
// Mode 9 shades every peeled layer once; its D passes are a rasteriser plus a position evaluation each.

// The steps of lv_shade_prism up to lv_prism_accept, on the same operands (as lv_prism_frag_pos: the normals do not enter the
// position): decides bit for bit what the shading stage decides, and returns the interpolated position.
__device__ __forceinline__ bool lv_prism_frag_kept(const LvSceneDev& S, const LvUniforms& U, const float* ringTab, f3 o, f3 d, float tLo,
                                                   float tHi, uint32_t leaf, uint32_t tt, f3& pos) {
    const LvPrismDev& R = S.prism;
    uint32_t pi[2];
    LvPrismPoint pt[2];
    lv_prism_frames(S, leaf, S.segs[2 * size_t(leaf)], S.segs[2 * size_t(leaf) + 1], pt, pi);
    const LvPrismTri T = lv_prism_tri_setup(ringTab, R.n, pt, pi, R.radius, tt);
    f3 nrm[3];
#pragma unroll
    for (int i = 0; i < 3; i++) nrm[i] = norm3q<false>(T.dir[i]);
    const f3 cam = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    const LvPrismPlanes pl = lv_prism_planes(R, T, cam, d);
    pos = lv_prism_interpolate(T, nrm, pl, d).pos;
    return lv_prism_accept(R, pt, R.radius, o, d, pos, len3(pos - o), tLo, tHi);
}

// The loop of the two passes: stages A and B of k_ppll_raster_prism (one LDS queue of (pixel, segment) pairs), stage B's lane then
// loops over the bits of its coverage mask and calls onKept(addr, leaf, tt, pos) for every kept fragment.  Without a 2 100-instruction
// shading stage behind it there is no second queue and nothing to park: a covered pair has 1 - 2 triangles (front faces of a convex
// prism), so the loop is short and the lanes of a batch stay together.  COUNTERS: the frame's fragCounter and statistics (the count
// pass; the peel passes walk the same fragments again and must not add them again).
template <int NT, bool COUNTERS, class OnKept>
__device__ __forceinline__ void lv_kept_fragments_walk(const LvUniforms& U, const LvSceneDev& S, const uint32_t* __restrict__ startOffset,
                                                       LvDevCounters* dc, uint32_t allRequested, const uint32_t* __restrict__ leafList,
                                                       uint32_t collectStats, OnKept&& onKept) {
    __shared__ uint32_t s_qLeaf[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE], s_qPix[LV_BLOCK / LV_WAVE][LV_PRISM_RASTER_QUEUE];
    __shared__ float s_seg[LV_BLOCK / LV_WAVE][20][LV_WAVE];
    __shared__ float s_prismRing[4 * LV_PRISM_MAX_SUBDIV];
    if (threadIdx.x < LV_PRISM_MAX_SUBDIV) {
        s_prismRing[threadIdx.x] = S.prism.c[threadIdx.x];
        s_prismRing[LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.s[threadIdx.x];
        s_prismRing[2 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.cp[threadIdx.x];
        s_prismRing[3 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.sn[threadIdx.x];
    }
    __syncthreads();
    const LvPrismDev& R = S.prism;
    const uint32_t N = NT > 0 ? uint32_t(NT) : R.n;
    const unsigned lane = lv_lane();
    uint32_t* qLeaf = s_qLeaf[threadIdx.x >> 6];
    uint32_t* qPix = s_qPix[threadIdx.x >> 6];
    float (*segLds)[LV_WAVE] = s_seg[threadIdx.x >> 6];
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    float mx[4], my[4], mw[4];
    lv_clip_rows(U, mx, my, mw);
    const float halfW = 0.5f * float(U.width), halfH = 0.5f * float(U.height);
    const float wEps = 1e-3f * U.nearDist;
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u);   // the interval of the streamed passes' stage C
    const bool stats = COUNTERS && collectStats != 0u;
    unsigned qHead = 0u, qCount = 0u;   // the queue (wave-uniform)
    unsigned long long tests = 0;
    uint32_t keptLane = 0u;

    // stage B on the m <= 64 oldest pairs of the queue
    auto coverageStage = [&](unsigned m) {
        if (lane < m) {
            uint32_t leaf, pix;
            unsigned mask = lv_seg_pair_coverage<NT>(R, segLds, qLeaf, qPix, (qHead + lane) & (LV_PRISM_RASTER_QUEUE - 1u), o, leaf, pix);
            if (mask != 0u) {
                const uint32_t px = pix & 0xFFFFu, py = pix >> 16;
                const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
                f3 oo, d;
                lv_primary_ray(U, px, py, 0.5f, 0.5f, oo, d);   // the viewing ray the shading stage shades on
                while (mask != 0u) {
                    const unsigned tt = unsigned(__ffs(int(mask))) - 1u;
                    mask &= mask - 1u;
                    f3 pos;
                    if (lv_prism_frag_kept(S, U, s_prismRing, o, d, tLo, tHi, leaf, tt, pos)) {
                        keptLane++;
                        onKept(addr, leaf, tt, pos);
                    }
                }
            }
        }
        if (stats) tests += m;
        qHead = (qHead + m) & (LV_PRISM_RASTER_QUEUE - 1u);
        qCount -= m;
    };

    const uint32_t waveId = blockIdx.x * (LV_BLOCK / LV_WAVE) + (threadIdx.x >> 6), numWaves = gridDim.x * (LV_BLOCK / LV_WAVE);
    const uint32_t numItems = leafList ? dc->prismListCount : S.numSegs;
    for (uint32_t itemBase = waveId * LV_WAVE; itemBase < numItems; itemBase += numWaves * LV_WAVE) {
        const bool valid = itemBase + lane < numItems;
        const uint32_t leaf = !valid ? 0u : (leafList ? leafList[itemBase + lane] : itemBase + lane);
        const LvSegWalk w = lv_seg_walk_setup(U, S, segLds, mx, my, mw, halfW, halfH, wEps, N, valid, leaf, lane);
        int px = w.x0, py = w.y0;
        bool more = valid && w.x1 >= w.x0 && w.y1 >= w.y0;
        while (__any(more)) {
            const bool cand = more && lv_seg_walk_candidate(U, w, px, py, allRequested, startOffset);
            const unsigned long long cm = __ballot(cand);
            if (cand) {
                const unsigned q = (qHead + qCount + unsigned(__popcll(cm & ((1ull << lane) - 1ull)))) & (LV_PRISM_RASTER_QUEUE - 1u);
                qLeaf[q] = leaf | (lane << 26);
                qPix[q] = uint32_t(px) | (uint32_t(py) << 16);
            }
            qCount += unsigned(__popcll(cm));
            if (qCount >= LV_WAVE) coverageStage(LV_WAVE);
            if (more) more = lv_seg_walk_advance(w, px, py);
        }
        while (qCount > 0u) coverageStage(qCount < LV_WAVE ? qCount : LV_WAVE);   // (the next 64 segments replace the frames in LDS)
    }
    if (COUNTERS) {
        const unsigned long long kept = lv_wave_sum_u64(keptLane);
        if (lane == 0u && kept) atomicAdd(&dc->fragCounter, uint32_t(kept));   // every kept fragment
        if (stats) {
            if (lane == 0u && tests) atomicAdd(&dc->prims, tests);
            if (lane == 0u && kept) atomicAdd(&dc->hits, kept);
        }
    }
}

template <int NT>
__global__ __launch_bounds__(LV_BLOCK, LV_PRISM_RASTER_MIN_WAVES) void k_dc_count_pass(const LvUniforms U, const LvSceneDev S,
                                                               const uint32_t* __restrict__ startOffset,
                                                               uint32_t* __restrict__ fragCount, LvDevCounters* dc,
                                                               uint32_t allRequested, const uint32_t* __restrict__ leafList,
                                                               uint32_t collectStats) {
    lv_kept_fragments_walk<NT, true>(U, S, startOffset, dc, allRequested, leafList, collectStats,
                                     [&](uint32_t addr, uint32_t, uint32_t, const f3&) { atomicAdd(&fragCount[addr], 1u); });
}

// first: pass 0 (the gather's `i != 0`: any depth below 1.0)
template <int NT>
__global__ __launch_bounds__(LV_BLOCK, LV_PRISM_RASTER_MIN_WAVES) void k_peel_pass(const LvUniforms U, const LvSceneDev S,
                                                           const uint32_t* __restrict__ startOffset, unsigned long long* slot,
                                                           const uint32_t* __restrict__ prevZ, LvDevCounters* dc,
                                                           uint32_t allRequested, const uint32_t* __restrict__ leafList,
                                                           uint32_t first) {
    lv_kept_fragments_walk<NT, false>(U, S, startOffset, dc, allRequested, leafList, 0u,
                                      [&](uint32_t addr, uint32_t leaf, uint32_t tt, const f3& pos) {
        const uint32_t zbits = __float_as_uint(lv_window_depth(U, pos));
        if (lv_peel_candidate(zbits, prevZ[addr], first != 0u)) lv_peel_offer(slot + addr, lv_peel_key(zbits, (S.leafSeg[leaf] << 6) | tt));
    });
}

// The requested pixels of the viewport, grid-stride, one lane per pixel: total, used pixels, maximum, minimum; wave reductions, then one
// atomic per wave and word.  (One wave per 64 pixels -- 32 K waves on a 1920 x 1080 viewport, five atomics each on the same five
// addresses -- took 0.62 ms on config 4; the grid is a few workgroups per CU instead.)
__global__ __launch_bounds__(LV_BLOCK) void k_dc_reduce(const LvUniforms U, const uint32_t* __restrict__ startOffset,
                                                       const uint32_t* __restrict__ fragCount, uint32_t allRequested, LvDcStats* st,
                                                       LvDevCounters* dc) {
    const size_t pixels = size_t(U.width) * U.height;
    unsigned long long total = 0ull;
    uint32_t used = 0u, hi = 0u, lo = 0xFFFFFFFFu;
    for (size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x; p < pixels; p += size_t(gridDim.x) * LV_BLOCK) {
        const uint32_t addr = lv_ppll_addr(uint32_t(p % U.width), uint32_t(p / U.width), U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
        if (allRequested == 0u && startOffset[addr] != 0u) continue;
        const uint32_t n = fragCount[addr];
        total += n;
        used += n != 0u ? 1u : 0u;
        hi = max(hi, n);
        lo = min(lo, n);
    }
    total = lv_wave_sum_u64(total);
    used = uint32_t(lv_wave_sum_u64(used));
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
        hi = max(hi, (uint32_t)__shfl_xor(hi, ofs, 64));
        lo = min(lo, (uint32_t)__shfl_xor(lo, ofs, 64));
    }
    if (lv_lane() == 0u) {
        if (total) atomicAdd(&st->total, total);
        if (used) atomicAdd(&st->used, used);
        if (hi) { atomicMax(&st->maxCount, hi); atomicMax(&dc->maxDepthComplexity, hi); }
        if (lo != 0xFFFFFFFFu) atomicMin(&st->minCount, lo);
    }
}

// One lane per pixel, one wave per workgroup, the cells and groups of k_wboit_resolve
__global__ __launch_bounds__(LV_WAVE) void k_dc_resolve(const LvUniforms U, const LvTiles T, const uint32_t* __restrict__ fragCount,
                                                        const LvDcStats* __restrict__ st, uint32_t explicitMaxColour,
                                                        uint32_t* __restrict__ out, uint32_t numGroups) {
    const uint32_t lane = threadIdx.x;
    const uint32_t maxColour = lv_dc_max_colour(st->maxCount, explicitMaxColour);
    const uint32_t groupsX = T.blocksX / 4u, groupsPerTile = groupsX * (T.blocksY / 4u);
    for (uint32_t g = blockIdx.x; g < numGroups; g += gridDim.x) {
        const uint32_t slot = g >> 6, cell = g & 63u;
        const uint32_t grp = T.groupOrder ? T.groupOrder[slot] : slot;
        const uint32_t tile = grp / groupsPerTile, gi = grp % groupsPerTile;
        const uint32_t lx = (gi % groupsX) * 64u + (cell & 7u) * 8u + (lane & 7u);
        const uint32_t ly = (gi / groupsX) * 64u + (cell >> 3) * 8u + (lane >> 3);
        if (!(lx < T.tileW && ly < T.tileH)) continue;
        const uint32_t x = T.tilesXY[2 * tile] + lx, y = T.tilesXY[2 * tile + 1] + ly;
        const uint32_t n = (x < U.width && y < U.height) ? fragCount[lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)] : 0u;
        out[(tile * T.tileH + ly) * T.tileW + lx] = lv_dc_resolve_pixel(U, n, maxColour);
    }
}

// The cells and groups of k_wboit_resolve: a pure read of the accumulators
__global__ __launch_bounds__(LV_WAVE) void k_peel_blit(const LvUniforms U, const LvTiles T, const float4* __restrict__ accum,
                                                       uint32_t* __restrict__ out, uint32_t numGroups) {
    const uint32_t lane = threadIdx.x;
    const uint32_t groupsX = T.blocksX / 4u, groupsPerTile = groupsX * (T.blocksY / 4u);
    for (uint32_t g = blockIdx.x; g < numGroups; g += gridDim.x) {
        const uint32_t slot = g >> 6, cell = g & 63u;
        const uint32_t grp = T.groupOrder ? T.groupOrder[slot] : slot;
        const uint32_t tile = grp / groupsPerTile, gi = grp % groupsPerTile;
        const uint32_t lx = (gi % groupsX) * 64u + (cell & 7u) * 8u + (lane & 7u);
        const uint32_t ly = (gi / groupsX) * 64u + (cell >> 3) * 8u + (lane >> 3);
        if (!(lx < T.tileW && ly < T.tileH)) continue;
        const uint32_t x = T.tilesXY[2 * tile] + lx, y = T.tilesXY[2 * tile + 1] + ly;
        float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (x < U.width && y < U.height) A = accum[lv_ppll_addr(x, y, U.ppllPaddedW, U.ppllTileW, U.ppllTileH)];
        out[(tile * T.tileH + ly) * T.tileW + lx] = lv_peel_blit_pixel(U, A);
    }
}

// every word of a mode-9 frame (n padded pixels) and the reduce's words
__global__ __launch_bounds__(LV_BLOCK) void k_peel_clear(LvPeelBuffers B, size_t n, LvDcStats* st) {
    const size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i < n) {
        if (B.slot) {
            B.slot[i] = LV_PEEL_SLOT_EMPTY;
            B.prevZ[i] = 0u;
            B.accum[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            B.layers[i] = 0u;
        }
    }
    if (i == 0) { st->total = 0ull; st->used = 0u; st->maxCount = 0u; st->minCount = 0xFFFFFFFFu; st->pad = 0u; }
}

// lv_depth_peeling_resolve_buffers: one lane per given entry {r, g, b, a, z, key}, all lanes racing for the pixel's slot; pixel = the
// run of `offsets` that holds the entry (the binary search of k_wboit_add_given)
__global__ __launch_bounds__(LV_BLOCK) void k_peel_given(const uint32_t* __restrict__ entries, uint64_t numEntries,
                                                        const unsigned long long* __restrict__ offsets, uint32_t numPixels,
                                                        LvPeelBuffers B, uint32_t first) {
    const uint64_t i = uint64_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (i >= numEntries) return;
    uint32_t lo = 0u, hi = numPixels;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t zbits = entries[size_t(i) * 6u + 4u];
    if (lv_peel_candidate(zbits, B.prevZ[lo], first != 0u)) lv_peel_offer(B.slot + lo, lv_peel_key(zbits, entries[size_t(i) * 6u + 5u]));
}
// ... and its layer kernel: one lane per pixel; the winner is the entry of the pixel's run with the slot's key (unique within a run)
__global__ __launch_bounds__(LV_BLOCK) void k_peel_layer_given(const uint32_t* __restrict__ entries,
                                                              const unsigned long long* __restrict__ offsets, uint32_t numPixels,
                                                              LvPeelBuffers B) {
    const uint32_t p = blockIdx.x * LV_BLOCK + threadIdx.x;
    if (p >= numPixels) return;
    const unsigned long long won = B.slot[p];
    if (won >= LV_PEEL_SLOT_EMPTY) return;
    const uint32_t key = uint32_t(won), zbits = uint32_t(won >> 32);
    for (unsigned long long i = offsets[p]; i < offsets[p + 1]; i++) {
        const uint32_t* e = entries + size_t(i) * 6u;
        if (e[5] != key || e[4] != zbits) continue;
        f4 c;
        c.x = __uint_as_float(e[0]); c.y = __uint_as_float(e[1]); c.z = __uint_as_float(e[2]); c.w = __uint_as_float(e[3]);
        B.accum[p] = lv_peel_accumulate(B.accum[p], c);
        break;
    }
    B.prevZ[p] = zbits;
    B.layers[p] += 1u;
    B.slot[p] = LV_PEEL_SLOT_EMPTY;
}

// lv_depth_peeling_get_buffers / lv_depth_complexity_get_buffers: the per-pixel words of the viewport, row-major (null = not wanted)
__global__ __launch_bounds__(LV_BLOCK) void k_peel_read(LvPeelBuffers B, const uint32_t* __restrict__ fragCount, uint32_t width,
                                                       uint32_t height, uint32_t paddedW, uint32_t tileW, uint32_t tileH,
                                                       float4* __restrict__ outAccum, uint32_t* __restrict__ outLayers,
                                                       uint32_t* __restrict__ outCounts) {
    const size_t p = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x;
    if (p >= size_t(width) * height) return;
    const uint32_t addr = lv_ppll_addr(uint32_t(p % width), uint32_t(p / width), paddedW, tileW, tileH);
    if (outAccum) outAccum[p] = B.accum[addr];
    if (outLayers) outLayers[p] = B.layers[addr];
    outCounts[p] = fragCount[addr];
}

// ================================================================ depth range
__global__ __launch_bounds__(LV_BLOCK) void k_depth_minmax(const LvUniforms U, const lv_line_point* __restrict__ points,
                                                           uint32_t numPoints, LvDevCounters* dc) {
    // ComputeDepthValues.glsl:58-98; the 256-wide shared-memory tree + MinMaxReduce passes collapse into a wave
    // reduction and two atomics per wave (min/max are order independent, so the result is identical).
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    const float EPSILON = 1e-2f;
    float mn = U.farDist, mx = U.nearDist;
    if (i < numPoints) {
        const float* p = points[i].linePosition;
        f4 ssp = mulM4(U.view, p[0], p[1], p[2], 1.0f);
        f4 ndc = mulM4(U.proj, ssp.x, ssp.y, ssp.z, ssp.w);
        float nx = ndc.x / ndc.w, ny = ndc.y / ndc.w, nz = ndc.z / ndc.w;
        if (nx >= -1.0f && ny >= -1.0f && nz >= -1.0f && nx <= 1.0f && ny <= 1.0f && nz <= 1.0f) {
            float depth = clampf(-ssp.z, U.nearDist, U.farDist);
            mn = depth - EPSILON;
            mx = depth + EPSILON;
        }
    }
    mn = lv_wave_min(mn);
    mx = lv_wave_max(mx);
    if (lv_lane() == 0) {
        atomicMin(&dc->depthOrd[0], lv_f2ord(mn));
        atomicMax(&dc->depthOrd[1], lv_f2ord(mx));
    }
}
__global__ void k_depth_init(const LvUniforms U, LvDevCounters* dc) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        dc->depthOrd[0] = lv_f2ord(U.farDist);
        dc->depthOrd[1] = lv_f2ord(U.nearDist);
    }
}
__global__ void k_depth_finalize(const LvDevCounters* dc, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = lv_ord2f(dc->depthOrd[0]);
        out[1] = lv_ord2f(dc->depthOrd[1]);
    }
}

// ================================================================ arbitrary rays (parity inspection)
template <int PRIM, bool FAST_INV = false>
__global__ __launch_bounds__(LV_BLOCK) void k_trace_rays(const LvSceneDev S, float radius, uint32_t capped,
                                                         const float* __restrict__ org, const float* __restrict__ dir,
                                                         float tMin, float tMax, uint32_t n, float* __restrict__ outT,
                                                         uint32_t* __restrict__ outSeg, uint32_t* __restrict__ outKind) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    const bool valid = i < n;
    LvCounters cnt = {0, 0, 0, 0};
    const uint32_t j = valid ? i : 0u;
    f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]);
    f3 d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
    LvHit h = lv_trace_closest<false, false, PRIM, FAST_INV>(S, radius, capped != 0, valid, o, d, tMin, tMax,
                                                             lv_stack_mem(s_stack, S.stackOverflow), cm, cnt);
    if (!valid) return;
    outT[i] = h.found ? h.t : tMax;
    outSeg[i] = h.found ? S.leafSeg[h.leaf] : 0xFFFFFFFFu;
    outKind[i] = h.found ? uint32_t(h.kind) : 0u;
}

template <bool FAST_INV>
__global__ __launch_bounds__(LV_BLOCK) void k_trace_rays_tri(const LvSceneDev S, const float* __restrict__ org,
                                                             const float* __restrict__ dir, float tMin, float tMax,
                                                             uint32_t n, float* __restrict__ outT,
                                                             uint32_t* __restrict__ outTri, float* __restrict__ outUV) {
    __shared__ unsigned s_stack[LV_STACK_LDS * LV_BLOCK];
    LV_COOP_SHARED(LV_BLOCK / LV_WAVE);
    LV_COOP_MEM(cm);
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    const bool valid = i < n;
    LvCounters cnt = {0, 0, 0, 0};
    const uint32_t j = valid ? i : 0u;
    f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]);
    f3 d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
    LvHit h = lv_trace_closest<false, false, LV_PRIM_TRIANGLE, FAST_INV>(S, 0.0f, false, valid, o, d, tMin, tMax,
                                                                         lv_stack_mem(s_stack, S.stackOverflow), cm, cnt);
    if (!valid) return;
    float t = tMax, u = 0.0f, v = 0.0f;
    if (h.found) {
        const uint32_t* ti = S.triIdx + 3 * size_t(h.leaf);
        const float* a = S.triVerts[ti[0]].vertexPosition;
        const float* b = S.triVerts[ti[1]].vertexPosition;
        const float* c = S.triVerts[ti[2]].vertexPosition;
        lv_ray_triangle(o, d, mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]),
                        mk3(c[0], c[1], c[2]), S.triPad, t, u, v);
    }
    outT[i] = h.found ? h.t : tMax;
    outTri[i] = h.found ? h.leaf : 0xFFFFFFFFu;
    outUV[2 * size_t(i)] = u;
    outUV[2 * size_t(i) + 1] = v;
}

inline uint32_t nblocks(uint64_t n, uint32_t bs = LV_BLOCK) { return uint32_t((n + bs - 1) / bs); }

void padTiling(uint32_t& w, uint32_t& h, uint32_t tw, uint32_t th) {
    // LineRenderer::getScreenSizeWithTiling, LineRenderer.cpp:805-812
    if (w % tw != 0) w = (w / tw + 1) * tw;
    if (h % th != 0) h = (h / th + 1) * th;
}

LvSceneDev sceneDev(const lv_ctx* ctx) {
    LvSceneDev S;
    S.nodes = (const float4*)ctx->nodes.ptr;
    S.segs = (const float4*)ctx->segs.ptr;
    S.segAxis = (const float4*)ctx->segAxis.ptr;
    S.prismFrames = (const float4*)ctx->prismFrames.ptr;
    S.leafSeg = (const uint32_t*)ctx->leafSeg.ptr;
    S.segToLeaf = (const uint32_t*)ctx->segToLeaf.ptr;
    S.points = (const lv_line_point*)ctx->points.ptr;
    S.numPoints = ctx->numPoints;
    S.segIdx = (const uint32_t*)ctx->segIdx.ptr;
    S.tf = (const float4*)ctx->tf.ptr;
    S.twistTex = (const float4*)ctx->twistTex.ptr;
    S.depthMinMax = (const float*)ctx->depthMinMax.ptr;
    S.ao = ctx->aoResult ? ctx->aoResult : (const float*)ctx->ao.ptr;
    S.stackOverflow = nullptr;
    S.accum = nullptr;
    S.numSegs = ctx->numSegs;
    S.literalIntersection = lv_literal_intersection(ctx) ? 1u : 0u;
    S.ellBandWidth = ctx->opt.bandWidth;
    S.ellMinBandThickness = ctx->opt.minBandThickness;
    {   // cameraPosition, as lv_fill_uniforms
        const float* m = ctx->invView;
        S.ellCamPos[0] = ((m[0] * 0.0f + m[4] * 0.0f) + m[8] * 0.0f) + m[12] * 1.0f;
        S.ellCamPos[1] = ((m[1] * 0.0f + m[5] * 0.0f) + m[9] * 0.0f) + m[13] * 1.0f;
        S.ellCamPos[2] = ((m[2] * 0.0f + m[6] * 0.0f) + m[10] * 0.0f) + m[14] * 1.0f;
    }
    S.tris = nullptr; S.triIdx = nullptr; S.triVerts = nullptr; S.triPoints = nullptr; S.triPad = 0.0f; S.triLeafSize = 1u; S.triPairs = 0u;
    S.bakedAo = (const float*)ctx->bakedAo.ptr;
    S.bakedBlendingWeights = (const float*)ctx->bakeBlendingWeights.ptr;
    return S;
}

// scene view for the triangle-tube kernels: `nodes` = triangle LBVH, numSegs = triangle count
LvSceneDev sceneDevTriangles(const lv_ctx* ctx) {
    LvSceneDev S = sceneDev(ctx);
    S.nodes = (const float4*)ctx->triNodes.ptr;
    S.numSegs = ctx->numTris;
    S.tris = (const float4*)ctx->tris.ptr;
    S.triIdx = (const uint32_t*)ctx->triIdx.ptr;
    S.triVerts = (const lv_tube_vertex*)ctx->triVerts.ptr;
    S.triPoints = (const lv_line_point*)ctx->triPoints.ptr;
    S.triPad = ctx->triPad;
    S.triLeafSize = ctx->triLeafSize;
    S.triPairs = ctx->triLeafPairs ? 1u : 0u;
    return S;
}

} // namespace

// host copy of lv_sincos2pi (lv_device.h): the same float32 operations in the same order (the library is built with -ffp-contract=off)
static void lv_sincos2pi_host(float xi, float& s, float& c) {
    float q = xi * 4.0f;
    float fq = floorf(q);
    int quad = int(fq) & 3;
    float r = q - fq;
    bool swp = r > 0.5f;
    float rr = swp ? (1.0f - r) : r;
    float a = rr * 1.57079632679489662f;
    float a2 = a * a;
    float sp = a * (1.0f + a2 * (-1.0f / 6.0f + a2 * (1.0f / 120.0f + a2 * (-1.0f / 5040.0f + a2 * (1.0f / 362880.0f)))));
    float cp = 1.0f + a2 * (-0.5f + a2 * (1.0f / 24.0f + a2 * (-1.0f / 720.0f + a2 * (1.0f / 40320.0f + a2 * (-1.0f / 3628800.0f)))));
    float sa = swp ? cp : sp;
    float ca = swp ? sp : cp;
    if (quad == 0) { s = sa; c = ca; }
    else if (quad == 1) { s = ca; c = -sa; }
    else if (quad == 2) { s = -sa; c = -ca; }
    else { s = -ca; c = sa; }
}
// ppll_fragment_source: "auto" = the rasterised prism wherever it is built (plain flow lines), the capsule probe for band data
bool lv_ppll_prism_source(const lv_ctx* ctx) {
    const LvOptions& o = ctx->opt;
    if (o.ppllFragmentSource == 1) return false;
    // auto: the prism wherever its fragment stage is built -- plain tubes, band data (USE_BANDS), rotating helicity bands, each with
    // the screen-space or the prebaked AO; not band data with helicity bands (the raster shaders' NUM_TUBE_SUBDIVISIONS >= 8 && USE_AMBIENT_OCCLUSION && USE_BANDS path)
    const bool built = !(o.helicityBands && o.useRibbons);
    return o.ppllFragmentSource == 2 ? true : built;
}
// per-frame constants of the rasterised prism (LvPrismDev)
// constants of the coverage direction (lv_prism.h "viewing ray"); float32, one fixed order -- the CPU checker of the test-suite states the same
static void lv_prism_cov_constants(const float* invView, const float* invProj, uint32_t width, uint32_t height, float C0[3], float Cx[3],
                                   float Cy[3]) {
    auto mul3 = [&](const float* v, float out[3]) {   // invView3 * v
        for (int k = 0; k < 3; k++) out[k] = (invView[k] * v[0] + invView[4 + k] * v[1]) + invView[8 + k] * v[2];
    };
    const float p23[3] = {invProj[8] + invProj[12], invProj[9] + invProj[13], invProj[10] + invProj[14]};
    float a[3], b[3], c[3];
    mul3(invProj, a);
    mul3(invProj + 4, b);
    mul3(p23, c);
    const float sx = 2.0f / float(width), sy = 2.0f / float(height);
    for (int k = 0; k < 3; k++) {
        Cx[k] = a[k] * sx;
        Cy[k] = b[k] * sy;
        C0[k] = (c[k] - a[k]) - b[k];
    }
}

static void lv_fill_prism(const lv_ctx* ctx, const LvUniforms& U, LvPrismDev& R) {
    uint32_t n = ctx->opt.tubeNumSubdivisions;
    if (n < 3u) n = 3u;
    if (n > LV_PRISM_MAX_SUBDIV) n = LV_PRISM_MAX_SUBDIV;
    R.n = n;
    for (uint32_t k = 0; k < LV_PRISM_MAX_SUBDIV; k++) { R.c[k] = 1.0f; R.s[k] = 0.0f; }
    for (uint32_t k = 0; k < n; k++) lv_sincos2pi_host(float(k) / float(n), R.s[k], R.c[k]);
    // band data: the elliptic ring of the rasterisers' USE_BANDS vertex stage
    R.bands = U.useBands ? 1u : 0u;
    R.radius = U.useBands ? U.bandWidth * 0.5f : U.radius;
    R.thickness = U.useBands ? U.minThickness : 1.0f;
    for (uint32_t k = 0; k < LV_PRISM_MAX_SUBDIV; k++) { R.cp[k] = R.thickness * R.c[k]; R.sn[k] = R.thickness * R.s[k]; }
    for (int k = 0; k < 3; k++) R.right[k] = U.invView[k];
    R.viewZ[0] = U.view[2]; R.viewZ[1] = U.view[6]; R.viewZ[2] = U.view[10]; R.viewZ[3] = U.view[14];
    R.nearDist = U.nearDist;
    R.farDist = U.farDist;
    lv_prism_cov_constants(U.invView, U.invProj, U.width, U.height, R.covC0, R.covCx, R.covCy);
}

void lv_fill_uniforms(const lv_ctx* ctx, LvUniforms& U) {
    memset(&U, 0, sizeof(U));
    memcpy(U.view, ctx->view, 64);
    memcpy(U.proj, ctx->proj, 64);
    memcpy(U.invView, ctx->invView, 64);
    memcpy(U.invProj, ctx->invProj, 64);
    // rayOrigin = (inverseViewMatrix * vec4(0,0,0,1)).xyz, TubeRayTracing.glsl:202 (also used as cameraPosition)
    const float* m = ctx->invView;
    U.camPos[0] = ((m[0] * 0.0f + m[4] * 0.0f) + m[8] * 0.0f) + m[12] * 1.0f;
    U.camPos[1] = ((m[1] * 0.0f + m[5] * 0.0f) + m[9] * 0.0f) + m[13] * 1.0f;
    U.camPos[2] = ((m[2] * 0.0f + m[6] * 0.0f) + m[10] * 0.0f) + m[14] * 1.0f;
    U.fovY = ctx->fovY;
    for (int k = 0; k < 4; k++) {
        U.background[k] = ctx->background[k];
        U.foreground[k] = 1.0f - ctx->background[k]; // LineData.cpp:1282-1283
    }
    const LvOptions& o = ctx->opt;
    U.lineWidth = o.lineWidth;
    U.radius = o.lineWidth * 0.5f; // TubeRayTracing.glsl:453
    U.lssGeometry = (o.rtLss && !o.rtTriangleMesh) ? 1u : 0u;
    U.useBands = o.useRibbons ? 1u : 0u;
    U.useEllipticTubes = (o.useRibbons && o.ellipticTubes) ? 1u : 0u;
    U.bandWidth = o.bandWidth;
    U.minBandThickness = o.minBandThickness;
    U.minThickness = o.thickBands ? o.minBandThickness : 1e-2f; // MIN_THICKNESS, LineDataFlow.cpp:2425-2430
    U.useHelicityBands = o.helicityBands ? 1u : 0u;
    U.numSubdivisionsBands = o.bandSubdivisions;
    U.separatorBaseWidth = o.separatorWidth;
    U.helicityRotationFactor = o.helicityRotationFactor;
    U.useTwistTexture = (o.helicityBands && o.useTwistLineTexture && ctx->twistLevels != 0u) ? 1u : 0u;   // LineDataFlow.cpp:2437
    U.twistFilterMode = o.twistFilterMode;
    U.twistW = ctx->twistW; U.twistH = ctx->twistH; U.twistLevels = ctx->twistLevels;
    U.uniformHelicityBandWidth = o.uniformTwistLineWidth ? 1u : 0u;
    U.ppllRasterColour = o.ppllRayTracerColour ? 0u : 1u;
    U.nearDist = ctx->nearDist;
    U.farDist = ctx->farDist;
    U.width = ctx->width;
    U.height = ctx->height;
    U.maxDepthComplexity = o.maxDepthComplexity;
    U.numSamplesPerFrame = o.numSamplesPerFrame;
    // multi-frame accumulation (num_accumulated_frames > 1): the caller renders frame after frame and passes frame_number
    U.frameNumber = o.numAccumulatedFrames > 1u ? o.frameNumber : 0u;
    U.useJitteredRays = (o.numAccumulatedFrames > 1u || o.numSamplesPerFrame > 1u) ? 1u : 0u; // VulkanRayTracer.cpp:420-426
    U.useDeterministicSampling = o.useDeterministicSampling;
    U.useCappedTubes = o.useCappedTubes;
    U.useHalos = o.useHalos;
    U.useDepthCues = o.depthCueStrength > 0.0f;
    U.useAmbientOcclusion = o.useAmbientOcclusion;
    U.depthCueStrength = o.depthCueStrength;
    U.aoStrength = o.aoStrength;
    U.aoGamma = o.aoGamma;
    U.attrMin = ctx->attrMin;
    U.attrMax = ctx->attrMax;
    U.tfN = ctx->tfN;
    U.aoSamplesPerFrame = o.aoSamplesPerFrame;
    U.aoUseDistance = o.aoUseDistance;
    U.aoJitterPrimary = o.aoJitterPrimary;
    U.aoFrameNumber = 0;
    U.aoGlobalFrameNumber = 0;
    U.aoRadius = o.aoRadius;
    // VulkanRayTracedAmbientOcclusion.cpp:588
    U.subdivisionCorrectionFactor = cosf(3.1415926535897932f / float(o.tubeNumSubdivisions));
    // PerPixelLinkedListLineRenderer.cpp:109-126,175,257
    const bool large = ctx->numSegs > 1000000u;
    U.ppllMaxNumFrags = o.ppllMaxNumFrags ? o.ppllMaxNumFrags : (large ? 380u : 100u);
    const uint32_t avg = o.ppllExpectedAvgDepthComplexity ? o.ppllExpectedAvgDepthComplexity : (large ? 120u : 20u);
    U.ppllTileW = o.ppllTileW;
    U.ppllSortingMode = o.ppllSortingMode;
    U.ppllTileH = o.ppllTileH;
    uint32_t pw = ctx->width, ph = ctx->height;
    padTiling(pw, ph, o.ppllTileW, o.ppllTileH);
    U.ppllPaddedW = pw;
    U.ppllPaddedH = ph;
    uint64_t pool = uint64_t(avg) * pw * ph;
    if (pool > 0xFFFFFFF0ull) pool = 0xFFFFFFF0ull; // node indices are 32 bit
    U.ppllLinkedListSize = uint32_t(pool);
    U.aoPrebaked = (o.useAmbientOcclusion && o.aoPrebaked) ? 1u : 0u;
    U.bakeNumLineVertices = ctx->bakeNumLineVertices;
    U.bakeNumParametrizationVertices = ctx->bakeNumParametrizationVertices;
    U.bakeNumTubeSubdivisions = o.bakeNumTubeSubdivisions;
}

int lv_frame_depth_range(lv_ctx* ctx) {
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->depthMinMax, 16))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->counters, sizeof(LvDevCounters)))) return rc;
    LvDevCounters* dc = (LvDevCounters*)ctx->counters.ptr;
    k_depth_init<<<1, 64, 0, st>>>(U, dc);
    if (ctx->numPoints)
        k_depth_minmax<<<nblocks(ctx->numPoints), LV_BLOCK, 0, st>>>(U, (const lv_line_point*)ctx->points.ptr,
                                                                      ctx->numPoints, dc);
    k_depth_finalize<<<1, 64, 0, st>>>(dc, (float*)ctx->depthMinMax.ptr);
    LV_HIP(ctx, hipGetLastError());
    return LV_OK;
}

// ---------------------------------------------------------------- launch geometry of a tile list (the host side of lv_block_pixel)
// numTiles tiles of tileW x tileH pixels, each in 16x16-pixel blocks that fill whole 64x64 groups
static LvTiles lv_tiles(const uint32_t* tilesXY, uint32_t numTiles, uint32_t tileW, uint32_t tileH) {
    LvTiles T{};
    T.tilesXY = tilesXY; T.numTiles = numTiles; T.tileW = tileW; T.tileH = tileH;
    T.blocksX = ((tileW + 63u) / 64u) * 4u; T.blocksY = ((tileH + 63u) / 64u) * 4u;
    return T;
}
static uint64_t lv_tiles_blocks(const LvTiles& T) { return uint64_t(T.numTiles) * T.blocksX * T.blocksY; }
// workgroups of a tile kernel: a multiple of 8 XCDs x LV_XCD_GROUP (a launch bounds the blocks by 0x7FFFFFF0 first)
static uint64_t lv_tiles_grid(const LvTiles& T) { return (lv_tiles_blocks(T) + 127u) / 128u * 128u; }
static uint64_t lv_tiles_groups(const LvTiles& T) { return uint64_t(T.numTiles) * (T.blocksX / 4u) * (T.blocksY / 4u); }   // 64 x 64 pixels
static uint64_t lv_tiles_cells(const LvTiles& T) { return lv_tiles_groups(T) * 64u; }   // 8 x 8 pixels: one wave of a resolve each
static uint64_t lv_tiles_pixels(const LvTiles& T) { return uint64_t(T.numTiles) * T.tileW * T.tileH; }

// persistent grid of k_ao_rays: enough workgroups to fill every CU at the kernel's LDS-limited residency
static uint64_t lv_ao_grid(const lv_ctx* ctx, uint64_t maxRays) {
    uint64_t gridRays = uint64_t(ctx->numCUs) * LV_AO_BLOCKS_PER_CU;
    if (gridRays > (maxRays + LV_AO_BLOCK - 1) / LV_AO_BLOCK) gridRays = (maxRays + LV_AO_BLOCK - 1) / LV_AO_BLOCK;
    return gridRays ? gridRays : 1;
}

// Launch geometry of a frame's RTAO pass (lv_run_ao) for the colour pass' tiles Tcolour.  The pass runs on those tiles dilated by
// haloPx pixels: 1 when the colour rays are jittered (the AO lookup blends the four texels around the projected hit,
// AmbientOcclusion.glsl:84-99), plus the 2 * (2^iterations - 1) pixels the EAW denoiser reads around every pixel it filters (a-trous
// passes with step widths 1, 2, 4, ...).  SVGF is temporal -- its history is read at reprojected positions anywhere in the picture --
// so with it the pass covers the whole viewport as one tile at the origin, no halo, whatever tiles the call renders.  So does Spatial
// Hashing: its map accumulates every hit of the viewport exactly once per iteration, whatever tiles, shards or ranks draw the frame.
struct LvAoGeometry {
    bool wholeViewport;
    uint32_t haloPx, numTiles, tileW, tileH;
    uint64_t maxPixels;
    // workgroups of k_ao_primary, of k_ao_rays, and of k_primary_pair (the RTAO primaries' and the colour pass' in one launch)
    uint64_t gridTiles, gridRays, gridPair;
};
static LvAoGeometry lv_ao_geometry(const lv_ctx* ctx, const LvUniforms& U, const LvTiles& Tcolour) {
    LvAoGeometry G;
    const bool eaw = ctx->opt.eawEnabled && ctx->opt.eawIterations > 0u;
    G.wholeViewport = ctx->opt.svgfEnabled || ctx->opt.shEnabled;
    G.haloPx = G.wholeViewport ? 0u : (U.aoProjectLookup ? 1u : 0u) + (eaw ? 2u * ((1u << ctx->opt.eawIterations) - 1u) : 0u);
    G.numTiles = G.wholeViewport ? 1u : Tcolour.numTiles;
    G.tileW = G.wholeViewport ? ctx->width : Tcolour.tileW + 2u * G.haloPx;
    G.tileH = G.wholeViewport ? ctx->height : Tcolour.tileH + 2u * G.haloPx;
    const LvTiles T = lv_tiles(nullptr, G.numTiles, G.tileW, G.tileH);
    G.gridTiles = lv_tiles_grid(T);
    G.maxPixels = lv_tiles_pixels(T);
    G.gridRays = lv_ao_grid(ctx, G.maxPixels * U.aoSamplesPerFrame);
    G.gridPair = G.gridTiles + lv_tiles_grid(Tcolour);
    return G;
}

// ---------------------------------------------------------------- the global part of the traversal stacks
// Entries of one thread's slab column (0: the LDS window holds the whole stack).  A step of the 4-wide tree pushes at most 3
// references per level: the logical stack never holds more than M = 3 * levels + 2 entries, and a step at level d (root: 0) finds at
// most 3 d <= M - 5 of them.  The window is W = ldsSlots - 1 entries (slot 0: the sentinel) and a thread spills only at sp + 3 > ldsSlots,
// i.e. with >= W - 2 entries in the window:
//   M <= W: a step finds at most W - 5 entries, so nothing ever spills -- no slab, LvStackT never touches its pointer;
//   else:   before a spill, spilled + (W - 2) <= entries <= M, so afterwards spilled <= M - (W - 2) + K; spills and refills move whole
//           blocks of K = LV_STACK_SPILL_BLOCK, hence the column is that bound rounded up to a multiple of K.
static uint64_t lv_overflow_entries(uint64_t wideLevels, uint32_t ldsSlots) {
    const uint64_t M = 3ull * wideLevels + 2, W = ldsSlots - 1u, K = LV_STACK_SPILL_BLOCK;
    return M > W ? (M - (W - 2) + K + K - 1) / K * K : 0;
}
// Bytes of the slab for one launch, one column per thread.  LvStackT addresses its column by 32-bit byte offsets from the slab's base:
// a launch whose slab would not fit them is refused (lv_prepare_overflow, the asynchronous bake)
static constexpr size_t LV_OVERFLOW_MAX_BYTES = 0xFFFFFFFFull;
// tree: which LBVH the launch walks -- 0 (false) the capsules', 1 (true) the triangle tubes', LV_TREE_HULL the hull's
#define LV_TREE_HULL 2
static size_t lv_overflow_bytes(const lv_ctx* ctx, uint64_t gridBlocks, uint32_t ldsSlots, int tree) {
    const uint32_t levels = tree == LV_TREE_HULL ? ctx->hullWideDepth : tree ? ctx->triWideDepth : ctx->wideDepth;
    return size_t(gridBlocks) * LV_BLOCK * lv_overflow_entries(levels, ldsSlots) * 4;
}
// ... for every launch of a frame: lv_frame_render reserves ctx->stackOverflow once, BEFORE it builds a scene view, because a later,
// larger request would free the slab under the views built before it.  Same geometries as the launches: lv_ao_geometry.
static size_t lv_frame_overflow_bytes(const lv_ctx* ctx, const LvUniforms& U, const LvTiles& T, int mode, bool pairPrimaries) {
    const uint64_t gridTiles = lv_tiles_grid(T);
    size_t need = lv_overflow_bytes(ctx, gridTiles, LV_STACK_LDS, false);
    if (ctx->opt.rtTriangleMesh && mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER)
        need = std::max(need, lv_overflow_bytes(ctx, gridTiles, LV_STACK_LDS, true));
    if (mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER && lv_rt_hull_kernel(ctx) && lv_hull_drawn(ctx))   // k_render_rt_hull's second walk
        need = std::max(need, lv_overflow_bytes(ctx, gridTiles, LV_STACK_LDS, LV_TREE_HULL));
    if (U.useAmbientOcclusion && !U.aoPrebaked) {
        const LvAoGeometry G = lv_ao_geometry(ctx, U, T);
        const bool tri = lv_ao_triangle_tubes(ctx);
        need = std::max(need, lv_overflow_bytes(ctx, std::max(G.gridRays, G.gridTiles), LV_AO_STACK_LDS, tri));
        if (pairPrimaries) {   // one slab for both halves of the launch, for the deeper of the two trees
            need = std::max(need, lv_overflow_bytes(ctx, G.gridPair, LV_STACK_LDS, false));
            if (tri) need = std::max(need, lv_overflow_bytes(ctx, G.gridPair, LV_STACK_LDS, true));
        }
    }
    if (U.aoPrebaked && !ctx->bakeValid)   // the synchronous bake (lv_bake_ambient_occlusion)
        need = std::max(need, lv_overflow_bytes(ctx, uint64_t(ctx->numCUs) * LV_AO_BLOCKS_PER_CU, LV_AO_STACK_LDS, true));
    return need;
}
// Points a scene view of a frame at the slab.  Nothing inside a frame moves it: a launch the reservation did not cover is an error.
static int lv_prepare_overflow(lv_ctx* ctx, LvSceneDev& S, const char* launch, uint64_t gridBlocks, uint32_t ldsEntries = LV_STACK_LDS,
                               int tree = 0) {
    S.stackOverflow = nullptr;
    const size_t bytes = lv_overflow_bytes(ctx, gridBlocks, ldsEntries, tree);
    if (bytes == 0) return LV_OK;
    if (bytes > LV_OVERFLOW_MAX_BYTES)
        return lv_fail(ctx, LV_E_CAPACITY, "%s: the traversal stacks would need %llu bytes; a launch addresses at most 4 GiB of them", launch,
                       (unsigned long long)bytes);
    if (!ctx->stackOverflow.ptr || ctx->stackOverflow.bytes < bytes)
        return lv_fail(ctx, LV_E_CAPACITY, "%s: the traversal stacks need %llu bytes, the frame reserved %llu", launch,
                       (unsigned long long)bytes, (unsigned long long)ctx->stackOverflow.bytes);
    S.stackOverflow = (unsigned*)ctx->stackOverflow.ptr;
    return LV_OK;
}
// ... of an entry point outside a frame, which reserves for its one launch
static int lv_reserve_overflow(lv_ctx* ctx, LvSceneDev& S, const char* launch, uint64_t gridBlocks, uint32_t ldsEntries = LV_STACK_LDS,
                               int tree = 0) {
    const size_t bytes = lv_overflow_bytes(ctx, gridBlocks, ldsEntries, tree);
    int rc;
    if (bytes && (rc = lv_buf_reserve(ctx, ctx->stackOverflow, bytes))) return rc;
    return lv_prepare_overflow(ctx, S, launch, gridBlocks, ldsEntries, tree);
}

// ---------------------------------------------------------------- dispatch order of the tile kernels
// A tile kernel lasts as long as its last workgroup, and the cost of a 64x64-pixel group spans orders of magnitude (a group over
// the core of a bundle against one over the background).  In tile-list order the heavy groups start whenever their turn
// comes and the launch ends with a tail of a few of them; started first (longest processing time first) the light groups fill
// the gaps behind them.  The cost is what the group's waves took in the previous frame (LvTiles::groupCost) -- with a
// camera that moves a little per frame a good predictor, and only a predictor: every order renders the same image.
// One workgroup sorts (cost descending, group index ascending) with a bitonic network in LDS and clears the cost array.
#define LV_ORDER_MAX_GROUPS 8192u
__global__ __launch_bounds__(1024) void k_group_order(uint32_t* __restrict__ cost0, uint32_t* __restrict__ order0, uint32_t n0,
                                                      uint32_t* __restrict__ cost1, uint32_t* __restrict__ order1, uint32_t n1) {
    extern __shared__ unsigned long long s_keys[];
    uint32_t* cost = blockIdx.x ? cost1 : cost0;
    uint32_t* order = blockIdx.x ? order1 : order0;
    const uint32_t n = blockIdx.x ? n1 : n0;
    if (n == 0u) return;
    uint32_t np = 1u;
    while (np < n) np <<= 1;
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
        s_keys[i] = i < n ? ((unsigned long long)(~cost[i]) << 32) | i : ~0ull;
        if (i < n) cost[i] = 0u;
    }
    __syncthreads();
    if (n <= blockDim.x) {
        // up to 1 024 groups (a 1920 x 1080 viewport has 510): rank sort -- the keys are distinct (the group index is their low word), so
        // a key's position is the number of smaller keys; every lane reads the same LDS word per step (a broadcast), one barrier in all.
        // The bitonic network below needs 45 barrier-separated steps for 512 keys: 11 us per frame, 6 % of a config-2 frame.
        if (threadIdx.x < n) {
            const unsigned long long mine = s_keys[threadIdx.x];
            uint32_t rank = 0u;
            for (uint32_t i = 0u; i < n; i++) rank += s_keys[i] < mine ? 1u : 0u;
            order[rank] = uint32_t(mine);
        }
        return;
    }
    for (uint32_t k = 2u; k <= np; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s_keys[i], b = s_keys[l];
                    if ((a > b) == ((i & k) == 0u)) { s_keys[i] = b; s_keys[l] = a; }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) order[i] = uint32_t(s_keys[i]);
}

// Points T at the dispatch order / cost array of launch geometry `which` (0 colour pass, 1 RTAO pass); a new tile list or
// geometry starts from zero cost (= tile-list order).  The sort itself is queued by lv_group_order_sort.
static int lv_group_order_prepare(lv_ctx* ctx, LvTiles& T, int which) {
    T.groupOrder = nullptr;
    T.groupCost = nullptr;
    lv_ctx::GroupOrder& G = ctx->groupOrder[which];
    G.active = false;
    const uint64_t n64 = lv_tiles_groups(T);
    if (!ctx->opt.dispatchByCost || n64 < 2u || n64 > LV_ORDER_MAX_GROUPS) { G.n = 0; return LV_OK; }
    const uint32_t n = uint32_t(n64);
    int rc;
    if ((rc = lv_buf_reserve(ctx, G.cost, size_t(n) * 4))) return rc;
    if ((rc = lv_buf_reserve(ctx, G.order, size_t(n) * 4))) return rc;
    if (G.n != n || G.tileW != T.tileW || G.tileH != T.tileH || G.generation != ctx->tilesGeneration) {
        LV_HIP(ctx, hipMemsetAsync(G.cost.ptr, 0, size_t(n) * 4, ctx->stream));
        G.n = n; G.tileW = T.tileW; G.tileH = T.tileH; G.generation = ctx->tilesGeneration;
    }
    T.groupOrder = (const uint32_t*)G.order.ptr;
    T.groupCost = (uint32_t*)G.cost.ptr;
    G.active = true;
    return LV_OK;
}

// Queued once per frame, in front of the frame's first tile kernel (every geometry of the frame is prepared by then).
static int lv_group_order_sort(lv_ctx* ctx) {
    if (ctx->groupOrderSorted) return LV_OK;
    ctx->groupOrderSorted = true;
    const lv_ctx::GroupOrder& A = ctx->groupOrder[0];
    const lv_ctx::GroupOrder& B = ctx->groupOrder[1];
    const uint32_t nA = A.active ? A.n : 0u, nB = B.active ? B.n : 0u;
    const uint32_t nMax = nA > nB ? nA : nB;
    if (nMax == 0u) return LV_OK;
    uint32_t np = 1u;
    while (np < nMax) np <<= 1;
    k_group_order<<<nB ? 2 : 1, 1024, size_t(np) * 8, ctx->stream>>>((uint32_t*)A.cost.ptr, (uint32_t*)A.order.ptr, nA,
                                                                    (uint32_t*)B.cost.ptr, (uint32_t*)B.order.ptr, nB);
    LV_HIP(ctx, hipGetLastError());
    return LV_OK;
}

// the one-tile list of a pass over the whole viewport (SVGF, Spatial Hashing and its a-trous tail): origin (0, 0)
static int lv_full_frame_tile(lv_ctx* ctx) {
    if (ctx->fullFrameTile.ptr) return LV_OK;
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->fullFrameTile, 8))) return rc;
    LV_HIP(ctx, hipMemsetAsync(ctx->fullFrameTile.ptr, 0, 8, ctx->stream));
    return LV_OK;
}

// EAWBlitPass(renderer, 3) of the spatial-hashing denoiser (SpatialHashingDenoiser.cpp:82-87): useColorWeights = false,
// phiPositionScale = 1e-6 on the EAW defaults (phiPosition 0.3, phiNormal 0.1, EAWDenoiser.hpp:82-93), normal and position weights on
int lv_eaw_tail(lv_ctx* ctx, uint32_t w, uint32_t h, const float* src, const float4* normalMap, const float4* positionMap, float* ping,
                float* pong, const float** result) {
    int rc;
    if ((rc = lv_full_frame_tile(ctx))) return rc;
    const LvTiles T = lv_tiles((const uint32_t*)ctx->fullFrameTile.ptr, 1u, w, h);
    LvUniforms U;
    memset(&U, 0, sizeof U);   // k_eaw_pass reads the extent only
    U.width = w;
    U.height = h;
    LvEawParams E;
    E.phiColor = 0.49f;
    E.phiPosition = 0.3f * 0.000001f;
    E.phiNormal = 0.1f * 1.0f;
    E.useColor = 0u; E.usePosition = 1u; E.useNormal = 1u;
    E.stepWidth = 1;
    float* bufs[2] = {ping, pong};
    const hipStream_t st = ctx->stream;
    auto passes = [&]() {   // one timer record for the three
        for (int i = 0; i < 3; i++) {
            k_eaw_pass<true><<<nblocks(uint64_t(w) * h), LV_BLOCK, 0, st>>>(U, T, E, src, bufs[i & 1], normalMap, positionMap);
            src = bufs[i & 1];
            E.stepWidth *= 2;
        }
    };
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_SH_TAIL, passes());
    LV_HIP(ctx, hipGetLastError());
    *result = src;
    return LV_OK;
}

// pairColour: the colour pass' scene view when its first-hit trace rides along with the RTAO primaries of the first iteration
// (k_primary_pair; lv_frame_render decides) -- the hits land in ctx->firstHit, *paired says whether the launch happened
static int lv_run_ao(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& Tcolour, const LvSceneDev* pairColour = nullptr,
                     bool* paired = nullptr) {
    hipStream_t st = ctx->stream;
    LvDevCounters* dc = (LvDevCounters*)ctx->counters.ptr;
    const uint32_t spp = U.aoSamplesPerFrame;
    int rc;
    // The tiles of the pass (lv_ao_geometry): the colour pass', dilated by the halo -- origins - haloPx, modulo 2^32: pixels left of /
    // above the viewport fail the inView test.  Rings of adjacent tiles overlap -- those pixels are simply computed twice, which is
    // why the running mean below reads the previous pass' image (ping-pong) instead of updating in place.  Or the whole viewport.
    const LvAoGeometry G = lv_ao_geometry(ctx, U, Tcolour);
    const bool eaw = ctx->opt.eawEnabled && ctx->opt.eawIterations > 0u;
    const bool whole = G.wholeViewport, svgf = ctx->opt.svgfEnabled, sh = ctx->opt.shEnabled, halo = G.haloPx != 0u;
    const uint32_t haloPx = G.haloPx, gridTiles = uint32_t(G.gridTiles), gridTilesColour = uint32_t(lv_tiles_grid(Tcolour));
    const uint64_t maxPixelsColour = lv_tiles_pixels(Tcolour), maxPixels = G.maxPixels;
    LvTiles T = Tcolour;
    if (whole) {
        if ((rc = lv_full_frame_tile(ctx))) return rc;
        T = lv_tiles((const uint32_t*)ctx->fullFrameTile.ptr, G.numTiles, G.tileW, G.tileH);
        if (svgf && (rc = lv_svgf_prepare(ctx))) return rc;
    }
    if (halo) {
        const uint32_t n = Tcolour.numTiles;
        if ((rc = lv_buf_reserve(ctx, ctx->tilesHaloDev, size_t(n) * 8))) return rc;
        if (!ctx->tilesHaloUploaded || ctx->tilesHalo != haloPx) {
            if (ctx->tilesHaloUploaded) LV_HIP(ctx, hipStreamSynchronize(st)); // the staging copy may still be in flight
            ctx->tilesHaloHost.resize(2 * size_t(n));
            for (size_t i = 0; i < 2 * size_t(n); i++) ctx->tilesHaloHost[i] = ctx->tilesHost[i] - haloPx;
            LV_HIP(ctx, hipMemcpyAsync(ctx->tilesHaloDev.ptr, ctx->tilesHaloHost.data(), size_t(n) * 8, hipMemcpyHostToDevice, st));
            ctx->tilesHaloUploaded = true;
            ctx->tilesHalo = haloPx;
        }
        T = lv_tiles((const uint32_t*)ctx->tilesHaloDev.ptr, G.numTiles, G.tileW, G.tileH);
        if (lv_tiles_blocks(T) > 0x7FFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    }
    // Tiles that share pixels -- the rings of a halo, a tile the caller lists twice -- compute those pixels once per tile.  The running
    // mean of iteration > 0 reads the previous iteration's image: updated in place, the second copy of a pixel could read what the first
    // had just written and blend the new factor in twice.  Such passes read one image and write the other.
    const bool pingPong = halo || (!whole && ctx->tilesOverlap);
    if (pingPong && (rc = lv_buf_reserve(ctx, ctx->aoAlt, size_t(ctx->width) * ctx->height * 4))) return rc;
    const size_t numPix = size_t(ctx->width) * ctx->height;
    if (eaw) {
        for (LvDeviceBuffer* b : {&ctx->featNormal, &ctx->featNormalAlt, &ctx->featPosition, &ctx->featPositionAlt})
            if ((rc = lv_buf_reserve(ctx, *b, numPix * 16))) return rc;
        if ((rc = lv_buf_reserve(ctx, ctx->eawPing, numPix * 4))) return rc;
        if ((rc = lv_buf_reserve(ctx, ctx->eawPong, numPix * 4))) return rc;
    }
    // G-buffer: one segment of 4096 slots per 64x64-pixel group of the launch (k_ao_primary); samples: compact
    if (lv_tiles_groups(T) > 0x000FFFFFull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    const uint32_t numGroups = uint32_t(lv_tiles_groups(T));
    // dispatch order: the colour pass' (same launch geometry: both passes add to one cost array) or, on dilated tiles / the
    // whole viewport, one of its own
    if ((whole || halo) && (rc = lv_group_order_prepare(ctx, T, 1))) return rc;
    if ((rc = lv_group_order_sort(ctx))) return rc;
    const LvAoLayout tileCap = lv_ao_layout(T);   // segments sized by the pixels a group really holds
    if ((rc = lv_buf_reserve(ctx, ctx->aoGbuf, size_t(maxPixels) * 48))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->aoSamples, size_t(maxPixels) * spp * 4))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->aoList, (2 * size_t(numGroups) + 1) * 4))) return rc; // per-group counts, then bases
    uint32_t* tileCount = (uint32_t*)ctx->aoList.ptr;
    uint32_t* tileBase = tileCount + numGroups;
    ctx->aoNumGroups = whole ? 0u : numGroups; // whole-viewport pass: no per-tile costs of the caller's tile list (lv_get_ao_tile_costs)
    ctx->aoGroupsPerTile = tileCap.groupsPerTile;
    const bool tri = lv_ao_triangle_tubes(ctx);
    // RTAO geometry: the capsules of the colour pass, or the reference's triangle tubes (own LBVH, own scene view)
    LvSceneDev SA = tri ? sceneDevTriangles(ctx) : S;
    if ((rc = lv_prepare_overflow(ctx, SA, "RTAO pass", std::max(G.gridRays, G.gridTiles), LV_AO_STACK_LDS, tri))) return rc;
    // the paired launch: gridTiles + gridTilesColour workgroups share one slab (columns are indexed by the launch's global thread id)
    LvSceneDev SCpair = pairColour ? *pairColour : S;
    LvSceneDev SApair = SA;
    if (pairColour && ((rc = lv_prepare_overflow(ctx, SCpair, "paired primaries (colour rays)", G.gridPair)) ||
                       (rc = lv_prepare_overflow(ctx, SApair, "paired primaries (RTAO rays)", G.gridPair, LV_STACK_LDS, tri))))
        return rc;
    const bool stats = ctx->opt.collectStats;
    // progressive mode (num_accumulated_frames > 1): one RTAO iteration per rendered frame while frame_number <
    // ambient_occlusion_iterations (ambientOcclusionBaker->updateIterative(), LineRenderer.cpp:257-264), accumulated in ctx->ao
    const bool progressive = ctx->opt.numAccumulatedFrames > 1u;
    if (ctx->aoRestart) {
        // the denoiser changed (lv_set_option): the accumulated AO image and the feature maps belong to another pipeline
        if (progressive && ctx->opt.frameNumber != 0u)
            return lv_fail(ctx, LV_E_STATE, "ambient_occlusion_denoiser changed: restart the accumulation with frame_number = 0");
        ctx->aoRestart = false;
    }
    const float* shResult = nullptr;
    const uint32_t iterBegin = progressive ? ctx->opt.frameNumber : 0u;
    const uint32_t iterEnd = progressive ? std::min(ctx->opt.frameNumber + 1u, ctx->opt.aoIterations) : ctx->opt.aoIterations;
    for (uint32_t iter = iterBegin; iter < iterEnd; iter++) {
        U.aoFrameNumber = iter; // rtaoRenderPass->setFrameNumber(accumulatedFramesCounter), VulkanRayTracedAmbientOcclusion.cpp:92
        U.aoGlobalFrameNumber = iter;
        LvSvgfFeat SF;
        SF.normalDepth = nullptr;
        SF.flowFwidth = nullptr;
        if (whole) {
            // DISABLE_ACCUMULATION + useGlobalFrameNumber (SVGF.hpp:81-82, SpatialHashingDenoiser.hpp:83-84;
            // VulkanRayTracedAmbientOcclusion.cpp:415-421,576-581)
            U.aoFrameNumber = 0;
            U.aoGlobalFrameNumber = ctx->aoGlobalFrameNumber;
        }
        if (svgf) {
            SF.normalDepth = (float4*)ctx->svgf.normalDepth.ptr;
            SF.flowFwidth = (float4*)ctx->svgf.flowFwidth.ptr;
            float vp[16];
            lv_mat4_mul(ctx->proj, ctx->view, vp);
            memcpy(SF.lastFrameViewProj, ctx->lastFrameViewProjValid ? ctx->lastFrameViewProj : vp, sizeof vp);
            memcpy(ctx->lastFrameViewProj, vp, sizeof vp);
            ctx->lastFrameViewProjValid = true;
        }
        ctx->aoGlobalFrameNumber++;
        LV_HIP(ctx, hipMemsetAsync(tileCount, 0, size_t(numGroups) * 4, st));
        const uint32_t grid = uint32_t(G.gridRays);
        const float4* g = (const float4*)ctx->aoGbuf.ptr;
        // overlapping tiles: read the previous pass' image, write the other buffer, swap; otherwise update in place
        const float* aoIn = (const float*)ctx->ao.ptr;
        float* ao = pingPong ? (float*)ctx->aoAlt.ptr : (float*)ctx->ao.ptr;
        float* smp = (float*)ctx->aoSamples.ptr;
        // feature maps of the denoiser: same ping-pong as the AO image (the EAW halo makes the tiles overlap)
        const float4* fnIn = eaw ? (const float4*)ctx->featNormal.ptr : nullptr;
        float4* fnOut = eaw ? (float4*)ctx->featNormalAlt.ptr : nullptr;
        const float4* fpIn = eaw ? (const float4*)ctx->featPosition.ptr : nullptr;
        float4* fpOut = eaw ? (float4*)ctx->featPositionAlt.ptr : nullptr;
        const bool pairNow = pairColour && iter == iterBegin;
        if (pairNow && paired) *paired = true;
#define LV_LAUNCH_PAIR(ST, PR, BA)                                                                            \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_AO_PRIMARY, (k_primary_pair<ST, PR, BA><<<gridTiles + gridTilesColour, LV_BLOCK, 0, st>>>( \
            U, SApair, T, gridTiles, aoIn, ao, (float4*)ctx->aoGbuf.ptr, tileCount, dc, fnIn, fnOut, fpIn, fpOut, SF, SCpair, Tcolour, \
            (uint2*)ctx->firstHit.ptr, size_t(maxPixelsColour))))
#define LV_LAUNCH_AOP(ST, PR)                                                                                 \
    do {                                                                                                      \
        if (pairNow && U.useHelicityBands) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_HELICITY);                         \
        else if (pairNow && U.useBands) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_BANDS);                               \
        else if (pairNow) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_PLAIN);                                             \
        else                                                                                                  \
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_AO_PRIMARY, (k_ao_primary<ST, PR><<<gridTiles, LV_BLOCK, 0, st>>>(  \
                    U, SA, T, aoIn, ao, (float4*)ctx->aoGbuf.ptr, tileCount, dc, fnIn, fnOut, fpIn, fpOut, SF))); \
    } while (0)
#define LV_LAUNCH_AO(ST, AH, PR, LI, PG) \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_AO_RAYS, (k_ao_rays<ST, AH, PR, false, LI, PG><<<grid, LV_AO_BLOCK, 0, st>>>( \
            U, SA, g, smp, dc, tileBase, numGroups, tileCap)))
#define LV_LAUNCH_AO3(ST, AH, PG)                                      \
    do {                                                               \
        if (tri) LV_LAUNCH_AO(ST, AH, LV_PRIM_TRIANGLE, false, PG);    \
        else if (U.useEllipticTubes) LV_LAUNCH_AO(ST, AH, LV_PRIM_ELLIPTIC, false, PG); \
        else if (lv_literal_intersection(ctx)) LV_LAUNCH_AO(ST, AH, LV_PRIM_CAPSULE, true, PG); \
        else LV_LAUNCH_AO(ST, AH, LV_PRIM_CAPSULE, false, PG);         \
    } while (0)
#define LV_LAUNCH_AO2(ST, AH) \
    do { if (!ST && pixelGen) LV_LAUNCH_AO3(ST, AH, !ST); else LV_LAUNCH_AO3(ST, AH, false); } while (0)
        const bool ell = U.useEllipticTubes != 0u;
        if (stats) { if (tri) LV_LAUNCH_AOP(true, LV_PRIM_TRIANGLE); else if (ell) LV_LAUNCH_AOP(true, LV_PRIM_ELLIPTIC); else LV_LAUNCH_AOP(true, LV_PRIM_CAPSULE); }
        else { if (tri) LV_LAUNCH_AOP(false, LV_PRIM_TRIANGLE); else if (ell) LV_LAUNCH_AOP(false, LV_PRIM_ELLIPTIC); else LV_LAUNCH_AOP(false, LV_PRIM_CAPSULE); }
        k_ao_tile_scan<<<1, LV_BLOCK, 0, st>>>(tileCount, numGroups, tileBase, dc);
        const bool anyHit = !U.aoUseDistance;
        // ao_ray_generation = per_pixel: a batch of 64 rays is 64 samples of one pixel whenever spp and both chunk sizes are multiples of
        // 64 (k_ao_rays, PIXEL_GEN); batch numbers and G-buffer slots must fit 32 bits.  The collect_stats instantiations generate per ray.
        const bool pixelGen = ctx->opt.aoPixelGeneration && spp % LV_WAVE == 0u && LV_AO_CHUNK % LV_WAVE == 0u &&
                              LV_AO_CHUNK_SMALL % LV_WAVE == 0u && maxPixels < (1ull << 32) && maxPixels * spp < (1ull << 38);
        if (stats) { if (anyHit) LV_LAUNCH_AO2(true, true); else LV_LAUNCH_AO2(true, false); }
        else { if (anyHit) LV_LAUNCH_AO2(false, true); else LV_LAUNCH_AO2(false, false); }
#undef LV_LAUNCH_AO2
#undef LV_LAUNCH_AO3
#undef LV_LAUNCH_AO
#undef LV_LAUNCH_AOP
#undef LV_LAUNCH_PAIR
        if ((spp & 3u) == 0u) {
            const uint64_t rowBlocks = (maxPixels + LV_REDUCE_ROWS - 1) / LV_REDUCE_ROWS;
            const uint64_t cap = uint64_t(ctx->numCUs) * 16u;
            k_ao_reduce_rows<<<uint32_t(rowBlocks < cap ? rowBlocks : cap), LV_REDUCE_ROWS, 0, st>>>(U, g, smp, aoIn, ao, dc, tileBase,
                                                                                                      numGroups, tileCap);
        } else {
            k_ao_reduce<false><<<nblocks(maxPixels), LV_BLOCK, 0, st>>>(U, g, smp, aoIn, ao, dc, tileBase, numGroups, tileCap);
        }
        if (pingPong) std::swap(ctx->ao, ctx->aoAlt);
        if (eaw) { std::swap(ctx->featNormal, ctx->featNormalAlt); std::swap(ctx->featPosition, ctx->featPositionAlt); }
        // temporal denoiser: denoise() belongs to every _render (VulkanRayTracedAmbientOcclusion.cpp:633-651), its history advances
        // with every RTAO iteration
        if (svgf && (rc = lv_svgf_denoise(ctx, ctx->svgf, ctx->width, ctx->height, (const float*)ctx->ao.ptr))) return rc;
        // Spatial_Hashing_Denoiser::denoise() sits in the same place: the map takes every iteration's hits and AO
        if (sh && (rc = lv_sh_denoise_frame(ctx, U.camPos, tileBase, numGroups, tileCap.tileW, tileCap.tileH, tileCap.groupsX,
                                            tileCap.groupsPerTile, &dc->aoCount, maxPixels, &shResult)))
            return rc;
    }
    if (iterEnd > iterBegin || !ctx->aoResult)
        ctx->aoResult = svgf ? (const float*)ctx->svgf.result.ptr : (sh && shResult) ? shResult : (const float*)ctx->ao.ptr;
    if (eaw && iterEnd > iterBegin) {
        // denoiser->denoise() after the RTAO pass (VulkanRayTracedAmbientOcclusion.cpp:633-651): the accumulation keeps running
        // on the raw image, the colour pass samples the denoised one
        LvEawParams E;
        E.phiColor = ctx->opt.eawPhiColor * 1.0f;         // weight scales of the AO mode, Denoiser.cpp:59-61
        E.phiPosition = ctx->opt.eawPhiPosition * 0.0001f;
        E.phiNormal = ctx->opt.eawPhiNormal * 1.0f;
        E.useColor = ctx->opt.eawColorWeights; E.usePosition = ctx->opt.eawPositionWeights; E.useNormal = ctx->opt.eawNormalWeights;
        E.stepWidth = 1;
        const uint64_t threads = lv_tiles_pixels(T);
        const float* src = (const float*)ctx->ao.ptr;
        float* bufs[2] = {(float*)ctx->eawPing.ptr, (float*)ctx->eawPong.ptr};
        for (uint32_t i = 0; i < ctx->opt.eawIterations; i++) {
            float* dst = bufs[i & 1u];
            if (ctx->opt.eawUseSharedMemory)
                k_eaw_pass<true><<<nblocks(threads), LV_BLOCK, 0, st>>>(U, T, E, src, dst, (const float4*)ctx->featNormal.ptr,
                                                                         (const float4*)ctx->featPosition.ptr);
            else
                k_eaw_pass<false><<<nblocks(threads), LV_BLOCK, 0, st>>>(U, T, E, src, dst, (const float4*)ctx->featNormal.ptr,
                                                                          (const float4*)ctx->featPosition.ptr);
            src = dst;
            E.stepWidth *= 2;
        }
        ctx->aoResult = src;
    }
    S.ao = ctx->aoResult;
    LV_HIP(ctx, hipGetLastError());
    return LV_OK;
}

// The fold of mode 3 over the runs in ctx->ppllNodes / ppllStart (+ blockBase) / ppllCount: K = mlab_num_layers picks the node
// capacity C in {8, 16, 32, 64}; scratch holds the ordered long runs (>= the fragment array's entries x 8 B)
static int lv_mlab_fold(lv_ctx* ctx, const LvUniforms& U, const LvTiles& T, uint32_t numGroups, const uint32_t* blockBase, uint32_t* out,
                        uint2* scratch, LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    // the long list holds one entry per (tile, pixel) pair of the tile list: repeated or overlapping tiles list a pixel more than once
    if (lv_tiles_pixels(T) > 0xFFFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    const uint32_t longCap = uint32_t(lv_tiles_pixels(T));
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->mlabLong, size_t(longCap) * 8))) return rc;
    const uint32_t K = ctx->opt.mlabNumLayers;
    const uint32_t* frags = (const uint32_t*)ctx->ppllNodes.ptr;
    const uint32_t* so = (const uint32_t*)ctx->ppllStart.ptr;
    const uint32_t* cnt = (const uint32_t*)ctx->ppllCount.ptr;
    uint2* const longList = (uint2*)ctx->mlabLong.ptr;
    const uint32_t longGrid = uint32_t(ctx->numCUs) * 2u;
#define LV_LAUNCH_MLAB(C)                                                                                                     \
    do {                                                                                                                       \
        k_mlab_resolve<C><<<numGroups, LV_WAVE, 0, st>>>(U, T, frags, so, blockBase, cnt, out, numGroups, K, longList, longCap, dc); \
        k_mlab_resolve_long<C><<<longGrid, LV_MLAB_LONG_BLOCK, 0, st>>>(U, frags, so, blockBase, cnt, out, K, longList, longCap,   \
                                                                        scratch, dc);                                           \
    } while (0)
    if (K <= 8u) LV_LAUNCH_MLAB(8);
    else if (K <= 16u) LV_LAUNCH_MLAB(16);
    else if (K <= 32u) LV_LAUNCH_MLAB(32);
    else LV_LAUNCH_MLAB(64);
#undef LV_LAUNCH_MLAB
    return LV_OK;
}

// log(x) of mode 6's depth range on the host: lv_log_det of the device (lv_log2_det x ln 2), so that the range is the same float32
// bits wherever the library runs (the reference calls std::log)
static float lv_log_det_host(float x) {
    uint32_t bits;
    memcpy(&bits, &x, 4);
    int e = int((bits >> 23) & 0xFFu) - 127;
    const uint32_t mb = (bits & 0x007FFFFFu) | 0x3F800000u;
    float m;
    memcpy(&m, &mb, 4);
    if (m > 1.41421356f) { m = m * 0.5f; e = e + 1; }
    const float f = m - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float P = 0.333333333f + z * (0.2f + z * (0.142857143f + z * 0.111111111f));
    const float ln = 2.0f * s + (2.0f * s) * (z * P);
    return (float(e) + ln * 1.44269504f) * 0.693147181f;
}

// MBOITRenderer::computeDepthRange (MBOITRenderer.cpp:484-503) + the moment uniforms: boxOrd = k_mboit_points_box's six values.
// The eight corners of the points' box through row z of the view matrix (lv_view_depth's order), -max z - 0.1 / -min z + 0.1,
// clamped to near / far in the reference's four steps.
static LvMboitParams lv_mboit_params(const lv_ctx* ctx, const LvUniforms& U, const uint32_t* boxOrd, bool stats) {
    auto ord2f = [](uint32_t u) {
        const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
        float f;
        memcpy(&f, &b, 4);
        return f;
    };
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
    if (ctx->numPoints)
        for (int k = 0; k < 3; k++) { lo[k] = -ord2f(boxOrd[k]); hi[k] = ord2f(boxOrd[3 + k]); }
    float zMin = 0.0f, zMax = 0.0f;
    for (int k = 0; k < 8; k++) {
        const float x = (k & 1) ? hi[0] : lo[0], y = (k & 2) ? hi[1] : lo[1], z = (k & 4) ? hi[2] : lo[2];
        const float vz = ((U.view[2] * x + U.view[6] * y) + U.view[10] * z) + U.view[14];
        zMin = k ? std::min(zMin, vz) : vz;
        zMax = k ? std::max(zMax, vz) : vz;
    }
    float minViewZ = -zMax - 0.1f, maxViewZ = -zMin + 0.1f;
    minViewZ = std::max(minViewZ, U.nearDist);
    maxViewZ = std::min(maxViewZ, U.farDist);
    minViewZ = std::min(minViewZ, U.farDist);
    maxViewZ = std::max(maxViewZ, U.nearDist);
    LvMboitParams M;
    M.logDepthMin = lv_log_det_host(minViewZ);
    M.logDepthMax = lv_log_det_host(maxViewZ);
    M.overestimation = ctx->opt.mboitOverestimation;
    // moment_bias of MBOITRenderer.cpp:136-145 unless mboit_moment_bias overrides it
    const uint32_t N = ctx->opt.mboitNumMoments;
    M.momentBias = ctx->opt.mboitMomentBias > 0.0f ? ctx->opt.mboitMomentBias : (N == 4u ? 5e-7f : N == 6u ? 5e-6f : 5e-5f);
    M.stats = stats ? 1u : 0u;
    return M;
}

// Mode 6, first frame on these line points: their box for the log depth range.  Queues k_mboit_points_box and the copy of its six
// values into words 2 ... 7 of the pinned block; lv_mboit_box_adopt takes them over once the caller has synchronised the stream.
static int lv_mboit_box_queue(lv_ctx* ctx, const LvSceneDev& S, LvDevCounters* dc) {
    if (!ctx->pinned) LV_HIP(ctx, hipHostMalloc((void**)&ctx->pinned, 64, hipHostMallocDefault));
    if (ctx->numPoints)
        k_mboit_points_box<<<std::min(nblocks(ctx->numPoints), 256u), LV_BLOCK, 0, ctx->stream>>>(S.points, ctx->numPoints, dc);
    LV_HIP(ctx, hipMemcpyAsync((void*)(ctx->pinned + 2), dc->mboitBoxOrd, 24, hipMemcpyDeviceToHost, ctx->stream));
    return LV_OK;
}
static void lv_mboit_box_adopt(lv_ctx* ctx) {
    for (int k = 0; k < 6; k++) ctx->mboitBoxOrd[k] = ctx->pinned[2 + k];
    ctx->mboitBoxValid = true;
}

// clear(): LinkedListClear.glsl:46-55 + fragmentCounterBuffer->fill(0); allRequested: every pixel is marked as requested right away
static void lv_ppll_clear(lv_ctx* ctx, const LvUniforms& U, size_t padded4, bool allRequested, bool stats, LvDevCounters* dc) {
    k_ppll_clear<<<uint32_t((padded4 + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, ctx->stream>>>(
            (uint4*)ctx->ppllStart.ptr, (uint4*)ctx->ppllCount.ptr, padded4, dc, allRequested ? 0u : 0xFFFFFFFFu,
            (allRequested && stats) ? (unsigned long long)U.width * U.height : 0ull);
}

// shading_numerics = fast in the prism fragment stage: the plain tubes with the raster colour (the only variant whose alpha cannot
// follow the halo coordinate); every other variant keeps the exact arithmetic
static bool lv_prism_fast_shade(const lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, bool stats) {
    return ctx->opt.fastShading && !stats && !S.prism.bands && !U.useHelicityBands && U.ppllRasterColour;
}

// The two sweeps of mode 6 over the runs in ctx->ppllNodes (colours, then the view depths depthBase entries in) / ppllStart
// (+ blockBase) / ppllCount: k_mboit_resolve, then the listed long runs
static int lv_mboit_resolve(lv_ctx* ctx, const LvUniforms& U, const LvTiles& T, const LvMboitParams& M, uint32_t numGroups,
                            uint32_t depthBase, const uint32_t* blockBase, uint32_t* out, float* moments, LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    if (lv_tiles_pixels(T) > 0xFFFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    const uint32_t longCap = uint32_t(lv_tiles_pixels(T));   // one entry per (tile, pixel) pair, as lv_mlab_fold
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->mlabLong, size_t(longCap) * 8))) return rc;
    const uint4* rgba = (const uint4*)ctx->ppllNodes.ptr;
    const uint32_t* zbits = (const uint32_t*)ctx->ppllNodes.ptr + 4 * size_t(depthBase);
    const uint32_t* so = (const uint32_t*)ctx->ppllStart.ptr;
    const uint32_t* cnt = (const uint32_t*)ctx->ppllCount.ptr;
    uint2* const longList = (uint2*)ctx->mlabLong.ptr;
    const uint32_t longGrid = uint32_t(ctx->numCUs) * 16u;
#define LV_LAUNCH_MBOIT(N)                                                                                                      \
    do {                                                                                                                        \
        k_mboit_resolve<N><<<numGroups, LV_WAVE, 0, st>>>(U, T, M, rgba, zbits, so, blockBase, cnt, out, numGroups, longList,    \
                                                          longCap, moments, dc);                                                \
        k_mboit_resolve_long<N><<<longGrid, LV_WAVE, 0, st>>>(U, M, rgba, zbits, so, blockBase, cnt, out, longList, longCap,     \
                                                              moments, dc);                                                     \
    } while (0)
    if (ctx->opt.mboitNumMoments == 4u) LV_LAUNCH_MBOIT(4);
    else if (ctx->opt.mboitNumMoments == 6u) LV_LAUNCH_MBOIT(6);
    else LV_LAUNCH_MBOIT(8);
#undef LV_LAUNCH_MBOIT
    return LV_OK;
}

// What the segment rasteriser's frame runs in front of it, for k_ppll_raster_prism and k_mboit_stream_pass alike: the opening event
// of LV_KERNEL_PPLL_RASTER and -- a frame that leaves tiles out -- the coarse grid, the requested pixels (k_ppll_mark_tiles) and the
// list of the segments that can touch them (k_ppll_cull_segments; k_ppll_clear zeroed the list's counter).  LV_KERNEL_PPLL_RASTER
// times the rasteriser WITH these: a rank's rasteriser cost is the three together.  leafList: the list, or nullptr =
// every segment
static int lv_segment_raster_front(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats,
                                   bool allRequested, LvDevCounters* dc, uint32_t*& leafList) {
    hipStream_t st = ctx->stream;
    int rc;
    uint32_t* coarse = nullptr;
    if (!allRequested) {
        const size_t cells = size_t((U.width + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE) * ((U.height + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE);
        if ((rc = lv_buf_reserve(ctx, ctx->ppllCoarse, cells * 4))) return rc;
        coarse = (uint32_t*)ctx->ppllCoarse.ptr;
        LV_HIP(ctx, hipMemsetAsync(coarse, 0, cells * 4, st));
    }
    leafList = nullptr;
    if ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RASTER) & 1u) LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RASTER, 0), st));
    if (allRequested) {}   // (k_ppll_clear marked every pixel)
    else if (stats) k_ppll_mark_tiles<true><<<gridTiles, LV_BLOCK, 0, st>>>(U, T, (uint32_t*)ctx->ppllStart.ptr, coarse, dc);
    else k_ppll_mark_tiles<false><<<gridTiles, LV_BLOCK, 0, st>>>(U, T, (uint32_t*)ctx->ppllStart.ptr, coarse, dc);
    if (!allRequested && S.numSegs != 0) {
        if ((rc = lv_buf_reserve(ctx, ctx->prismLeafList, size_t(S.numSegs) * 4))) return rc;
        leafList = (uint32_t*)ctx->prismLeafList.ptr;
        const uint32_t cullGrid = (S.numSegs + LV_CULL_PER_BLOCK - 1u) / LV_CULL_PER_BLOCK;
        k_ppll_cull_segments<<<cullGrid, LV_BLOCK, 0, st>>>(U, S, coarse, leafList, dc);
    }
    return LV_OK;
}

// ---- The host side that the frames without a fragment pool share: streamed mode 6, modes 8 and 10, modes 5 and 9 ----
struct LvStreamedOpen {
    size_t pixels;       // padded pixels (whole uint4s, k_ppll_clear): what ppllStart, ppllCount and the mode's buffer hold
    bool allRequested;   // the tile list covers the viewport: every pixel is requested
};
// The opening: the restrictions of these modes (`name` in the messages), the prism's constants, ppllStart, ppllCount and the mode's
// own buffer (modeBytes per padded pixel; nullptr: none) reserved, clear().
// (use_ribbons with rotating_helicity_bands never gets here: lv_frame_check refuses that pair for every mode)
static int lv_streamed_open(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, bool stats, LvDevCounters* dc, const char* name,
                            LvDeviceBuffer* modeBuf, size_t modeBytes, LvStreamedOpen& F) {
    int rc;
    if (!lv_ppll_prism_source(ctx))
        return lv_fail(ctx, LV_E_INVALID, "%s works on the fragments of the rasterised prism, which this line data does not have", name);
    if (ctx->opt.ppllPrismLbvhWalk)
        return lv_fail(ctx, LV_E_INVALID, "%s runs the segment rasteriser: ppll_prism_rasteriser = lbvh is not supported", name);
    lv_fill_prism(ctx, U, S.prism);
    const size_t padded4 = (size_t(U.ppllPaddedW) * U.ppllPaddedH + 3) / 4; // cleared as whole uint4s (k_ppll_clear)
    F.pixels = padded4 * 4;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllStart, padded4 * 16))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllCount, padded4 * 16))) return rc;
    if (modeBuf && (rc = lv_buf_reserve(ctx, *modeBuf, F.pixels * modeBytes))) return rc;
    ctx->ppllPoolNodes = 0;
    ctx->ppllPaddedW = U.ppllPaddedW;
    ctx->ppllPaddedH = U.ppllPaddedH;
    F.allRequested = ctx->tilesCoverViewport;
    lv_ppll_clear(ctx, U, padded4, F.allRequested, stats, dc);
    return LV_OK;
}
// The closing event of LV_KERNEL_PPLL_RASTER (lv_segment_raster_front recorded the opening one) and its launch count
static int lv_segment_raster_end(lv_ctx* ctx) {
    if ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RASTER) & 1u) {
        LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RASTER, 1), ctx->stream));
        ctx->kernelLaunches[LV_KERNEL_PPLL_RASTER]++;
    }
    return LV_OK;
}
// The close in front of the frame's resolve: the phase mark and the resolve's grid, one wave per 8 x 8-pixel cell
static int lv_streamed_close(lv_ctx* ctx, const LvTiles& T, uint32_t& numGroups) {
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[13], ctx->stream));
    if (lv_tiles_cells(T) > 0xFFFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    numGroups = uint32_t(lv_tiles_cells(T));
    return LV_OK;
}
// ctx->streamed: set at the end of the frame function of `mode` (param: N of mode 6, K of mode 10); what every *_get_* call asks of
// it -- the last frame was a `mode` frame over the whole viewport, and the viewport is still that one
static void lv_streamed_done(lv_ctx* ctx, const LvUniforms& U, int mode, uint32_t param = 0u) {
    ctx->streamed = {mode, ctx->tilesCoverViewport, U.width, U.height, {U.ppllTileW, U.ppllTileH}, param};
    ctx->streamed.quads = ctx->opt.lineQuads && (mode == LV_RENDERING_MODE_DEPTH_COMPLEXITY || mode == LV_RENDERING_MODE_WBOIT ||
                                                 mode == LV_RENDERING_MODE_ATOMIC_LOOP_64);
    ctx->streamed.quadsSegs = ctx->numSegs;
    ctx->streamed.quadsAo = U.useAmbientOcclusion && !U.aoPrebaked;
}
static bool lv_streamed_is(const lv_ctx* ctx, int mode) {
    const lv_ctx::StreamedFrame& r = ctx->streamed;
    return r.mode == mode && r.full && r.w == ctx->width && r.h == ctx->height;
}
// The instance of a streamed pass for the frame: LAUNCH(NT, SHADE, FAST) with NT = 6 for the six-sided prism (0: any n), then the
// variants lv_pool_frame selects for the pooled fragment stage -- fast (lv_prism_fast_shade), bands, helicity bands, plain
#define LV_SELECT_STREAM_PASS_NT(LAUNCH, NT)                                         \
    do {                                                                             \
        if (fastShade) LAUNCH(NT, LV_SHADE_PLAIN, 2);                                \
        else if (S.prism.bands) LAUNCH(NT, LV_SHADE_BANDS, 0);                       \
        else if (U.useHelicityBands) LAUNCH(NT, LV_SHADE_HELICITY, 0);               \
        else LAUNCH(NT, LV_SHADE_PLAIN, 0);                                          \
    } while (0)
#define LV_SELECT_STREAM_PASS(LAUNCH)                                                \
    do {                                                                             \
        const bool fastShade = lv_prism_fast_shade(ctx, U, S, stats);                \
        if (S.prism.n == 6u) LV_SELECT_STREAM_PASS_NT(LAUNCH, 6); else LV_SELECT_STREAM_PASS_NT(LAUNCH, 0); \
    } while (0)

// A mode-6 frame with mboit_fragment_storage = streamed: clear, the two launches of k_mboit_stream_pass, the blend.  No record pool,
// no fragment pool, no scan, no regrowth; the only host synchronisation is the read-back of the line points' box, once per
// acceleration-structure build.  The blend's overflow flag stays in the frame's counters (lv_mboit_stream_overflow reads it).
#ifndef LV_MBOIT_STREAM_BLOCKS_PER_CU
#define LV_MBOIT_STREAM_BLOCKS_PER_CU 2   // four waves per workgroup, LV_MBOIT_STREAM_MIN_WAVES per SIMD
#endif
static int lv_mboit_stream_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats,
                                 uint32_t* out, LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    int rc;
    if (!lv_ppll_prism_source(ctx) || (ctx->opt.useRibbons && ctx->opt.helicityBands))
        return lv_fail(ctx, LV_E_INVALID, "mboit_fragment_storage = streamed: band data with rotating helicity bands has no prism fragment stage");
    if (!ctx->mboitBoxValid) {   // (in front of the opening: the box kernel runs before clear())
        if ((rc = lv_mboit_box_queue(ctx, S, dc))) return rc;
        LV_HIP(ctx, hipStreamSynchronize(st));
        lv_mboit_box_adopt(ctx);
    }
    const uint32_t N = ctx->opt.mboitNumMoments;
    LvStreamedOpen F;
    if ((rc = lv_streamed_open(ctx, U, S, stats, dc, "mboit_fragment_storage = streamed", &ctx->mboitAccum, size_t(1u + N + 4u) * 8, F))) return rc;
    const LvMboitParams M = lv_mboit_params(ctx, U, ctx->mboitBoxOrd, stats);
    LV_HIP(ctx, hipMemsetAsync(ctx->mboitAccum.ptr, 0, F.pixels * size_t(1u + N + 4u) * 8, st));
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[11], st));
    // LV_KERNEL_PPLL_RASTER: one launch per pass, the first with what a sharded frame runs in front of it (as in pooled storage)
    const bool rasterTimed = ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RASTER) & 1u) != 0u;
    uint32_t* leafList;
    if ((rc = lv_segment_raster_front(ctx, U, S, T, gridTiles, stats, F.allRequested, dc, leafList))) return rc;
    const uint32_t passGrid = uint32_t(ctx->numCUs) * LV_MBOIT_STREAM_BLOCKS_PER_CU;
#define LV_LAUNCH_STREAM(NT, SH, FA)                                                                                            \
    k_mboit_stream_pass<NT, SH, FA><<<passGrid, LV_BLOCK, 0, st>>>(U, S, M, (const uint32_t*)ctx->ppllStart.ptr,               \
            (uint32_t*)ctx->ppllCount.ptr, (unsigned long long*)ctx->mboitAccum.ptr, dc, F.allRequested ? 1u : 0u, leafList, N, pass)
    for (uint32_t pass = 0u; pass < 2u; pass++) {
        if (rasterTimed && pass) LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RASTER, 0), st));
        if (S.numSegs != 0) LV_SELECT_STREAM_PASS(LV_LAUNCH_STREAM);
        if ((rc = lv_segment_raster_end(ctx))) return rc;
    }
#undef LV_LAUNCH_STREAM
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_mboit_stream_blend<<<numGroups, LV_WAVE, 0, st>>>(
            U, T, M, (const unsigned long long*)ctx->mboitAccum.ptr, (const uint32_t*)ctx->ppllCount.ptr, out, numGroups, N, dc)));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_MBOIT, N);
    return LV_OK;
}

// the overflow flag of the last frame when that was a streamed mode-6 frame, a mode-8 or a mode-10 frame (host-synchronous)
int lv_mboit_stream_overflow(lv_ctx* ctx) {
    const int mode = ctx->streamed.mode;
    if ((mode != LV_RENDERING_MODE_MBOIT && mode != LV_RENDERING_MODE_WBOIT && mode != LV_RENDERING_MODE_ATOMIC_LOOP_64) || !ctx->counters.ptr)
        return LV_OK;
    uint32_t flag = 0u;
    LV_HIP(ctx, hipMemcpy(&flag, &((const LvDevCounters*)ctx->counters.ptr)->mboitOverflow, 4, hipMemcpyDeviceToHost));
    if (flag)
        return lv_fail(ctx, LV_E_CAPACITY, "%s: a pixel is covered by more than %u kept fragments (the 64-bit sums are "
                                           "exact up to that count)", mode == LV_RENDERING_MODE_WBOIT ? "WBOIT" : mode == LV_RENDERING_MODE_ATOMIC_LOOP_64 ? "Atomic Loop 64" : "MBOIT (streamed)",
                       LV_MBOIT_STREAM_MAX_COUNT);
    return LV_OK;
}

// What every *_get_* call (`fn`) of the pool-free modes asks first: lv_streamed_is(mode) and `buf` of that frame exists, else
// LV_E_STATE (`frame`: how the message names the frame)
static int lv_streamed_require(lv_ctx* ctx, int mode, const char* frame, const LvDeviceBuffer& buf, const char* fn) {
    if (lv_streamed_is(ctx, mode) && buf.ptr) return LV_OK;
    return lv_fail(ctx, LV_E_STATE, "%s: the last frame was not a %s over the whole viewport", fn, frame);
}
// The opening of the calls that read per-pixel words back: lv_streamed_require; the caller's arrays hold `capacity` `unit`, `perPixel`
// per pixel, else LV_E_INVALID; the frame has finished and kept every fragment (lv_mboit_stream_overflow); ctx->scratchRays has room
// for scratchPerPixel bytes per pixel, where the mode's read kernel lays the words out in row-major order
static int lv_read_back_open(lv_ctx* ctx, int mode, const char* frame, const LvDeviceBuffer& buf, const char* fn, uint64_t capacity,
                             uint32_t perPixel, const char* unit, size_t scratchPerPixel, uint64_t& pixels) {
    int rc;
    if ((rc = lv_streamed_require(ctx, mode, frame, buf, fn))) return rc;
    pixels = uint64_t(ctx->streamed.w) * ctx->streamed.h;
    if (capacity < pixels * perPixel)
        return lv_fail(ctx, LV_E_INVALID, "%s: out holds %llu %s, need %llu", fn, (unsigned long long)capacity, unit,
                       (unsigned long long)(pixels * perPixel));
    LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = lv_mboit_stream_overflow(ctx))) return rc;
    return lv_buf_reserve(ctx, ctx->scratchRays, size_t(pixels) * scratchPerPixel);
}
// ... and what it, and every *_resolve_buffers call, ends with: the launches went through, the copies to the caller's arrays (dst
// null: not asked for), the synchronisation (also: host arrays of the call were sources of asynchronous uploads)
struct LvCopyBack { void* dst; const void* src; size_t bytes; };
static int lv_read_back(lv_ctx* ctx, std::initializer_list<LvCopyBack> copies) {
    LV_HIP(ctx, hipGetLastError());
    for (const LvCopyBack& c : copies)
        if (c.dst) LV_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
    LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LV_OK;
}

// lv_mboit_get_moments (capacity in floats)
int lv_frame_mboit_stream_moments(lv_ctx* ctx, float* out, uint64_t capacityFloats) {
    const uint32_t perPixel = 1u + ctx->streamed.param;
    uint64_t pixels;
    int rc;
    if ((rc = lv_read_back_open(ctx, LV_RENDERING_MODE_MBOIT, "mode-6 frame with mboit_fragment_storage = streamed", ctx->mboitAccum,
                                "lv_mboit_get_moments", capacityFloats, perPixel, "floats", size_t(perPixel) * 4, pixels)))
        return rc;
    k_mboit_stream_moments<<<uint32_t((pixels + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, ctx->stream>>>(
            (const unsigned long long*)ctx->mboitAccum.ptr, ctx->streamed.w, ctx->streamed.h, ctx->ppllPaddedW, ctx->streamed.tile[0],
            ctx->streamed.tile[1], ctx->streamed.param, (float*)ctx->scratchRays.ptr);
    return lv_read_back(ctx, {{out, ctx->scratchRays.ptr, size_t(pixels) * perPixel * 4}});
}

// ---- The simulation-mesh hull (lv_hull.h): one more launch between a mode's line pass and its resolve ----
static LvHullDev lv_hull_dev(const lv_ctx* ctx) {
    LvHullDev H;
    H.idx = (const uint32_t*)ctx->hullIdx.ptr;
    H.verts = (const lv_hull_vertex*)ctx->hullVerts.ptr;
    H.numTris = ctx->hullNumTris;
    for (int k = 0; k < 3; k++) H.color[k] = ctx->opt.hullColor[k];
    H.opacity = ctx->opt.hullOpacity;
    H.useShading = ctx->opt.hullUseShading ? 1u : 0u;
    return H;
}
// The hull pass of a mode-5, mode-8 or mode-10 frame, if a hull is drawn: ONE launch of k_hull_pass<store> on the frame's requested-pixel
// mask, ppllCount and the mode's buffer, timed as LV_KERNEL_HULL.  No memory beyond the mesh, no host synchronisation.
static int lv_hull_pass(lv_ctx* ctx, int store, const LvUniforms& U, const LvSceneDev& S, bool allRequested, bool stats, LvDevCounters* dc,
                        unsigned long long* buf, uint32_t arg) {
    if (!lv_hull_drawn(ctx)) return LV_OK;
    const LvHullList none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0ull};
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_HULL, lv_hull_launch(ctx->stream, store, uint32_t(ctx->numCUs), U, S.prism, lv_hull_dev(ctx),
                                                        allRequested ? nullptr : (const uint32_t*)ctx->ppllStart.ptr,
                                                        (uint32_t*)ctx->ppllCount.ptr, buf, arg, dc, stats, none));
    return LV_OK;
}

// lv_hull_get_fragments: the LIST store over the whole viewport, twice -- the count, then (when the caller's capacity holds it) the
// fragments into ctx->scratchRays, which no *_get_* call of the last frame keeps anything in
int lv_frame_hull_fragments(lv_ctx* ctx, uint32_t* outPixel, uint32_t* outTriangle, float* outDepth, float* outRgba, uint64_t capacity,
                            uint64_t* outCount) {
    hipStream_t st = ctx->stream;
    int rc;
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    LvPrismDev R;
    lv_fill_prism(ctx, U, R);
    const LvHullDev H = lv_hull_dev(ctx);
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 8))) return rc;
    LvHullList L = {(unsigned long long*)ctx->scratchRays.ptr, nullptr, nullptr, nullptr, nullptr, 0ull};
    unsigned long long count = 0ull;
    LV_HIP(ctx, hipMemsetAsync(L.counter, 0, 8, st));
    lv_hull_launch(st, LV_HULL_STORE_LIST, uint32_t(ctx->numCUs), U, R, H, nullptr, nullptr, nullptr, 0u, nullptr, false, L);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(&count, L.counter, 8, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    *outCount = count;
    if (capacity < count)
        return lv_fail(ctx, LV_E_CAPACITY, "lv_hull_get_fragments: %llu fragments, capacity %llu", count, (unsigned long long)capacity);
    if (count == 0ull || (!outPixel && !outTriangle && !outDepth && !outRgba)) return LV_OK;
    // {counter, pad}, rgba (16 B), pixel, triangle, depth (4 B each) per fragment
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 16 + size_t(count) * 28))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    L.counter = (unsigned long long*)base;
    L.rgba = (float4*)(base + 16);
    L.pixel = (uint32_t*)(base + 16 + size_t(count) * 16);
    L.triangle = L.pixel + size_t(count);
    L.depth = (float*)(L.triangle + size_t(count));
    L.capacity = count;
    LV_HIP(ctx, hipMemsetAsync(L.counter, 0, 8, st));
    lv_hull_launch(st, LV_HULL_STORE_LIST, uint32_t(ctx->numCUs), U, R, H, nullptr, nullptr, nullptr, 0u, nullptr, false, L);
    LV_HIP(ctx, hipGetLastError());
    if (outRgba) LV_HIP(ctx, hipMemcpyAsync(outRgba, L.rgba, size_t(count) * 16, hipMemcpyDeviceToHost, st));
    if (outPixel) LV_HIP(ctx, hipMemcpyAsync(outPixel, L.pixel, size_t(count) * 4, hipMemcpyDeviceToHost, st));
    if (outTriangle) LV_HIP(ctx, hipMemcpyAsync(outTriangle, L.triangle, size_t(count) * 4, hipMemcpyDeviceToHost, st));
    if (outDepth) LV_HIP(ctx, hipMemcpyAsync(outDepth, L.depth, size_t(count) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// ---- Line quads (lv_linequad.h): line_primitive_mode = "Quads (Programmable Pull)" replaces the prism pass of modes 5, 8 and 10 ----
static LvLineQuadList lv_linequad_no_list() { return {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0ull}; }

// lv_line_quads_get_fragments: the LIST store over the whole viewport, twice -- the count, then (when the caller's capacity holds it) the
// fragments into ctx->scratchRays, as lv_frame_hull_fragments.  The pass reads what the frame read: the leaf-ordered segments, the AO
// image and the depth range the frame left in the context, under the current camera and options
int lv_frame_line_quads_fragments(lv_ctx* ctx, uint32_t* outPixel, uint32_t* outSegment, uint32_t* outTriangle, float* outDepth, float* outRgba,
                                  uint64_t capacity, uint64_t* outCount) {
    const lv_ctx::StreamedFrame& r = ctx->streamed;
    if (!r.quads || !r.full)   // (lv_streamed_done; a tile-list frame filled the AO image for its tiles only)
        return lv_fail(ctx, LV_E_STATE, "lv_line_quads_get_fragments: the last frame was not a mode-5, mode-8 or mode-10 frame over the whole "
                                        "viewport drawn with line_primitive_mode = \"Quads (Programmable Pull)\"");
    // The pass runs again on what the frame read, which has to be the frame's still: the viewport (the AO image has its size), the
    // leaf-ordered segment records (lv_set_lines / lv_set_trajectories / a line-width or band switch end their validity) and the AO image
    // (an AO mode switched on since would read an image no frame wrote).  Anything else -- camera pose, colours, strengths -- only
    // changes the answer
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    U.aoProjectLookup = 0u;
    const bool aoNow = U.useAmbientOcclusion && !U.aoPrebaked;
    if (r.w != ctx->width || r.h != ctx->height || !ctx->accelValid || ctx->accelLineWidth != lv_accel_width(ctx) ||
        r.quadsSegs != ctx->numSegs || !ctx->segs.ptr || !ctx->prismFrames.ptr || !ctx->leafSeg.ptr || aoNow != r.quadsAo ||
        (aoNow && (ctx->aoW != ctx->width || ctx->aoH != ctx->height || !(ctx->aoResult || ctx->ao.ptr))) || U.aoPrebaked ||
        ctx->opt.useRibbons || ctx->opt.helicityBands)
        return lv_fail(ctx, LV_E_STATE, "lv_line_quads_get_fragments: the viewport, the line data or the ambient occlusion mode changed since "
                                        "the frame: render it again");
    hipStream_t st = ctx->stream;
    int rc;
    LvSceneDev S = sceneDev(ctx);
    lv_fill_prism(ctx, U, S.prism);
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 8))) return rc;
    LvLineQuadList L = lv_linequad_no_list();
    L.counter = (unsigned long long*)ctx->scratchRays.ptr;
    unsigned long long count = 0ull;
    LV_HIP(ctx, hipMemsetAsync(L.counter, 0, 8, st));
    lv_linequad_launch(st, LV_LINEQUAD_STORE_LIST, U, S, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, false, L);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(&count, L.counter, 8, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    *outCount = count;
    if (capacity < count)
        return lv_fail(ctx, LV_E_CAPACITY, "lv_line_quads_get_fragments: %llu fragments, capacity %llu", count, (unsigned long long)capacity);
    if (count == 0ull || (!outPixel && !outSegment && !outTriangle && !outDepth && !outRgba)) return LV_OK;
    // {counter, pad}, rgba (16 B), pixel, segment, triangle, depth (4 B each) per fragment
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 16 + size_t(count) * 32))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    L.counter = (unsigned long long*)base;
    L.rgba = (float4*)(base + 16);
    L.pixel = (uint32_t*)(base + 16 + size_t(count) * 16);
    L.segment = L.pixel + size_t(count);
    L.triangle = L.segment + size_t(count);
    L.depth = (float*)(L.triangle + size_t(count));
    L.capacity = count;
    LV_HIP(ctx, hipMemsetAsync(L.counter, 0, 8, st));
    lv_linequad_launch(st, LV_LINEQUAD_STORE_LIST, U, S, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, false, L);
    return lv_read_back(ctx, {{outRgba, L.rgba, size_t(count) * 16}, {outPixel, L.pixel, size_t(count) * 4},
                              {outSegment, L.segment, size_t(count) * 4}, {outTriangle, L.triangle, size_t(count) * 4},
                              {outDepth, L.depth, size_t(count) * 4}});
}

// The middle of a mode-8 or mode-10 frame, between the clear of the mode's buffer and the close: the phase mark and ONE launch of
// k_stream_pass<MODE> on `buf` and `arg`.  LV_KERNEL_PPLL_RASTER: the pass with what a sharded frame runs in front of it (as in
// modes 2, 3 and 6)
template <int MODE>
static int lv_stream_pass(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats,
                          const LvStreamedOpen& F, LvDevCounters* dc, unsigned long long* buf, uint32_t arg) {
    hipStream_t st = ctx->stream;
    int rc;
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[11], st));
    uint32_t* leafList;
    if ((rc = lv_segment_raster_front(ctx, U, S, T, gridTiles, stats, F.allRequested, dc, leafList))) return rc;
    const uint32_t passGrid = uint32_t(ctx->numCUs) * LV_MBOIT_STREAM_BLOCKS_PER_CU;
#define LV_LAUNCH_STREAM(NT, SH, FA)                                                                                            \
    k_stream_pass<MODE, NT, SH, FA><<<passGrid, LV_BLOCK, 0, st>>>(U, S, (const uint32_t*)ctx->ppllStart.ptr,                   \
            (uint32_t*)ctx->ppllCount.ptr, buf, dc, F.allRequested ? 1u : 0u, leafList, arg, stats ? 1u : 0u)
    if (ctx->opt.lineQuads)   // line_primitive_mode = "Quads (Programmable Pull)": the pass of lv_linequad.hip on the same buffers
        lv_linequad_launch(st, MODE == LV_RENDERING_MODE_WBOIT ? LV_LINEQUAD_STORE_WBOIT : LV_LINEQUAD_STORE_AL64, U, S, leafList,
                           F.allRequested ? nullptr : (const uint32_t*)ctx->ppllStart.ptr, (uint32_t*)ctx->ppllCount.ptr, buf, arg, dc, stats,
                           lv_linequad_no_list());
    else if (S.numSegs != 0) LV_SELECT_STREAM_PASS(LV_LAUNCH_STREAM);
#undef LV_LAUNCH_STREAM
    return lv_segment_raster_end(ctx);
}

// A mode-10 frame (Atomic Loop 64): clear, ONE launch of k_stream_pass, the resolve.  No pool, no scan, no regrowth and no host
// synchronisation; the resolve's overflow flag stays in the frame's counters (lv_mboit_stream_overflow reads it).
static void lv_al64_clear(lv_ctx* ctx, size_t numWords, uint32_t K) {
    const size_t blocks = (numWords + LV_BLOCK - 1) / LV_BLOCK, maxBlocks = size_t(ctx->numCUs) * 32u;
    k_al64_clear<<<uint32_t(std::max<size_t>(1, std::min(blocks, maxBlocks))), LV_BLOCK, 0, ctx->stream>>>(
            (unsigned long long*)ctx->al64Buf.ptr, numWords, K);
}
static int lv_al64_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                         LvDevCounters* dc) {
    int rc;
    const uint32_t K = ctx->opt.al64NumLayers;
    LvStreamedOpen F;
    if ((rc = lv_streamed_open(ctx, U, S, stats, dc, "mode 10 (Atomic Loop 64)", &ctx->al64Buf, size_t(K + LV_AL64_TAIL) * 8, F))) return rc;
    lv_al64_clear(ctx, F.pixels * size_t(K + LV_AL64_TAIL), K);
    if ((rc = lv_stream_pass<LV_RENDERING_MODE_ATOMIC_LOOP_64>(ctx, U, S, T, gridTiles, stats, F, dc, (unsigned long long*)ctx->al64Buf.ptr, K)))
        return rc;
    if ((rc = lv_hull_pass(ctx, LV_HULL_STORE_AL64, U, S, F.allRequested, stats, dc, (unsigned long long*)ctx->al64Buf.ptr, K))) return rc;
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_al64_resolve<<<numGroups, LV_WAVE, 0, ctx->stream>>>(
            U, T, (const unsigned long long*)ctx->al64Buf.ptr, (const uint32_t*)ctx->ppllCount.ptr, out, numGroups, K, dc)));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_ATOMIC_LOOP_64, K);
    return LV_OK;
}

// lv_atomic_loop_get_num_layers: K of the last frame when that was a mode-10 frame (what lv_atomic_loop_get_buffers returns per pixel)
int lv_frame_al64_num_layers(lv_ctx* ctx, uint32_t* out) {
    if (ctx->streamed.mode != LV_RENDERING_MODE_ATOMIC_LOOP_64) return lv_fail(ctx, LV_E_STATE, "lv_atomic_loop_get_num_layers: the last frame was not a mode-10 frame");
    *out = ctx->streamed.param;
    return LV_OK;
}

// lv_atomic_loop_get_buffers
int lv_frame_al64_buffers(lv_ctx* ctx, uint64_t* outSlots, uint64_t* outTail, uint64_t capacityPixels) {
    const uint32_t K = ctx->streamed.param;
    uint64_t pixels;
    int rc;
    if ((rc = lv_read_back_open(ctx, LV_RENDERING_MODE_ATOMIC_LOOP_64, "mode-10 frame", ctx->al64Buf, "lv_atomic_loop_get_buffers",
                                capacityPixels, 1u, "pixels", size_t(K + LV_AL64_TAIL) * 8, pixels)))
        return rc;
    unsigned long long* dSlots = (unsigned long long*)ctx->scratchRays.ptr;
    unsigned long long* dTail = dSlots + size_t(pixels) * K;
    k_al64_read<<<uint32_t((pixels + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, ctx->stream>>>(
            (const unsigned long long*)ctx->al64Buf.ptr, ctx->streamed.w, ctx->streamed.h, ctx->ppllPaddedW, ctx->streamed.tile[0], ctx->streamed.tile[1], K,
            dSlots, dTail);
    return lv_read_back(ctx, {{outSlots, dSlots, size_t(pixels) * K * 8}, {outTail, dTail, size_t(pixels) * LV_AL64_TAIL * 8}});
}

// A mode-8 frame (Weighted Blended OIT): the sums zeroed, ONE launch of k_stream_pass, the resolve.  No pool, no scan, no
// regrowth and no host synchronisation; the resolve's overflow flag stays in the frame's counters (lv_mboit_stream_overflow reads it).
static int lv_wboit_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                          LvDevCounters* dc) {
    int rc;
    LvStreamedOpen F;
    if ((rc = lv_streamed_open(ctx, U, S, stats, dc, "mode 8 (WBOIT)", &ctx->wboitBuf, size_t(LV_WBOIT_SUMS) * 8, F))) return rc;
    LV_HIP(ctx, hipMemsetAsync(ctx->wboitBuf.ptr, 0, F.pixels * size_t(LV_WBOIT_SUMS) * 8, ctx->stream));
    const uint32_t weightMode = ctx->opt.wboitOpenglWeight ? LV_WBOIT_WEIGHT_OPENGL : LV_WBOIT_WEIGHT_REFERENCE;
    if ((rc = lv_stream_pass<LV_RENDERING_MODE_WBOIT>(ctx, U, S, T, gridTiles, stats, F, dc, (unsigned long long*)ctx->wboitBuf.ptr, weightMode)))
        return rc;
    if ((rc = lv_hull_pass(ctx, LV_HULL_STORE_WBOIT, U, S, F.allRequested, stats, dc, (unsigned long long*)ctx->wboitBuf.ptr, weightMode)))
        return rc;
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_wboit_resolve<<<numGroups, LV_WAVE, 0, ctx->stream>>>(
            U, T, (const unsigned long long*)ctx->wboitBuf.ptr, (const uint32_t*)ctx->ppllCount.ptr, out, numGroups, dc)));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_WBOIT);
    return LV_OK;
}

// lv_wboit_get_buffers
int lv_frame_wboit_buffers(lv_ctx* ctx, int64_t* outSums, uint32_t* outCounts, uint64_t capacityPixels) {
    uint64_t pixels;
    int rc;
    if ((rc = lv_read_back_open(ctx, LV_RENDERING_MODE_WBOIT, "mode-8 frame", ctx->wboitBuf, "lv_wboit_get_buffers", capacityPixels, 1u,
                                "pixels", size_t(LV_WBOIT_SUMS) * 8 + 4, pixels)))
        return rc;
    unsigned long long* dSums = (unsigned long long*)ctx->scratchRays.ptr;
    uint32_t* dCounts = (uint32_t*)(dSums + size_t(pixels) * LV_WBOIT_SUMS);
    k_wboit_read<<<uint32_t((pixels + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, ctx->stream>>>(
            (const unsigned long long*)ctx->wboitBuf.ptr, (const uint32_t*)ctx->ppllCount.ptr, ctx->streamed.w, ctx->streamed.h, ctx->ppllPaddedW,
            ctx->streamed.tile[0], ctx->streamed.tile[1], dSums, dCounts);
    return lv_read_back(ctx, {{outSums, dSums, size_t(pixels) * LV_WBOIT_SUMS * 8}, {outCounts, dCounts, size_t(pixels) * 4}});
}

// the per-pixel words of mode 9 behind ctx->peelBuf for n pixels: 16 B accumulator, 8 B slot, 4 B prevZ, 4 B layer count
static LvPeelBuffers lv_peel_buffers(const lv_ctx* ctx, size_t n) {
    LvPeelBuffers B;
    char* base = (char*)ctx->peelBuf.ptr;
    B.accum = (float4*)base;
    B.slot = (unsigned long long*)(base + n * 16);
    B.prevZ = (uint32_t*)(base + n * 24);
    B.layers = (uint32_t*)(base + n * 28);
    return B;
}
#define LV_PEEL_BYTES_PER_PIXEL 32u

// What modes 5 and 9 share: the restrictions of the streamed modes, clear, the front of the segment rasteriser, ONE launch of
// k_dc_count_pass and k_dc_reduce.  LV_KERNEL_PPLL_RASTER times the count pass (with the tile marking and segment culling of a sharded
// frame), LV_KERNEL_PPLL_GATHER the reduce.  peel: the words of mode 9 are reserved and cleared too.
static int lv_dc_count(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, LvDevCounters* dc,
                       bool peel, const char* name, uint32_t*& leafList) {
    hipStream_t st = ctx->stream;
    int rc;
    LvStreamedOpen F;
    if ((rc = lv_streamed_open(ctx, U, S, stats, dc, name, peel ? &ctx->peelBuf : nullptr, LV_PEEL_BYTES_PER_PIXEL, F))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->dcStatsDev, sizeof(LvDcStats)))) return rc;
    const size_t n = F.pixels;
    const bool allRequested = F.allRequested;
    LvPeelBuffers B = {nullptr, nullptr, nullptr, nullptr};
    if (peel) B = lv_peel_buffers(ctx, n);
    k_peel_clear<<<uint32_t(peel ? (n + LV_BLOCK - 1) / LV_BLOCK : 1), LV_BLOCK, 0, st>>>(B, n, (LvDcStats*)ctx->dcStatsDev.ptr);
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[11], st));
    if ((rc = lv_segment_raster_front(ctx, U, S, T, gridTiles, stats, allRequested, dc, leafList))) return rc;
    const uint32_t passGrid = uint32_t(ctx->numCUs) * LV_PRISM_RASTER_BLOCKS_PER_CU;
    if (!peel && ctx->opt.lineQuads) {   // line_primitive_mode = "Quads (Programmable Pull)" (mode 9 with quads: lv_frame_check)
        lv_linequad_launch(st, LV_LINEQUAD_STORE_COUNT, U, S, leafList, allRequested ? nullptr : (const uint32_t*)ctx->ppllStart.ptr,
                           (uint32_t*)ctx->ppllCount.ptr, nullptr, 0u, dc, stats, lv_linequad_no_list());
    } else if (S.numSegs != 0) {
        if (S.prism.n == 6u)
            k_dc_count_pass<6><<<passGrid, LV_BLOCK, 0, st>>>(U, S, (const uint32_t*)ctx->ppllStart.ptr, (uint32_t*)ctx->ppllCount.ptr, dc,
                                                             allRequested ? 1u : 0u, leafList, stats ? 1u : 0u);
        else
            k_dc_count_pass<0><<<passGrid, LV_BLOCK, 0, st>>>(U, S, (const uint32_t*)ctx->ppllStart.ptr, (uint32_t*)ctx->ppllCount.ptr, dc,
                                                             allRequested ? 1u : 0u, leafList, stats ? 1u : 0u);
    }
    if ((rc = lv_segment_raster_end(ctx))) return rc;
    // the hull's fragments are counted in front of the reduce: mode 5's maximum and statistics include them.  Mode 9 draws no hull
    // (DepthPeelingRenderer.cpp:86)
    if (!peel && (rc = lv_hull_pass(ctx, LV_HULL_STORE_COUNT, U, S, allRequested, stats, dc, nullptr, 0u))) return rc;
    const uint32_t pixels = U.width * U.height;
    const uint32_t reduceGrid = std::min<uint32_t>((pixels + LV_BLOCK - 1) / LV_BLOCK, uint32_t(ctx->numCUs) * 4u);
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_GATHER, (k_dc_reduce<<<reduceGrid, LV_BLOCK, 0, st>>>(
            U, (const uint32_t*)ctx->ppllStart.ptr, (const uint32_t*)ctx->ppllCount.ptr, allRequested ? 1u : 0u,
            (LvDcStats*)ctx->dcStatsDev.ptr, dc)));
    return LV_OK;
}

// A mode-5 frame (depth complexity): count, reduce, resolve.  No host synchronisation: the resolve reads the maximum from device memory.
static int lv_dc_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                       LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    int rc;
    uint32_t* leafList;
    if ((rc = lv_dc_count(ctx, U, S, T, gridTiles, stats, dc, false, "mode 5 (depth complexity)", leafList))) return rc;
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_dc_resolve<<<numGroups, LV_WAVE, 0, st>>>(
            U, T, (const uint32_t*)ctx->ppllCount.ptr, (const LvDcStats*)ctx->dcStatsDev.ptr, ctx->opt.dcMaxColour, out, numGroups)));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_DEPTH_COMPLEXITY);
    return LV_OK;
}

// A mode-9 frame (depth peeling): count and reduce as mode 5, the read-back of the maximum -- the frame's ONE host synchronisation, the
// reference's syncWithCpu --, then min(maximum, depth_peeling_max_layers) times k_peel_pass + k_peel_layer, the blit.
// LV_KERNEL_PPLL_RASTER: the count pass, then the peel passes; LV_KERNEL_PPLL_SHADE: the layer launches; LV_KERNEL_PPLL_RESOLVE: the blit.
static int lv_peel_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                         LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    int rc;
    uint32_t* leafList;
    if ((rc = lv_dc_count(ctx, U, S, T, gridTiles, stats, dc, true, "mode 9 (depth peeling)", leafList))) return rc;
    LvDcStats hs;
    LV_HIP(ctx, hipMemcpyAsync(&hs, ctx->dcStatsDev.ptr, sizeof(hs), hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t passes = std::min(hs.maxCount, ctx->opt.peelMaxLayers);
    const bool allRequested = ctx->tilesCoverViewport;
    const size_t n = ((size_t(U.ppllPaddedW) * U.ppllPaddedH + 3) / 4) * 4;
    const LvPeelBuffers B = lv_peel_buffers(ctx, n);
    uint32_t* const startOffset = (uint32_t*)ctx->ppllStart.ptr;
    const uint32_t passGrid = uint32_t(ctx->numCUs) * LV_PRISM_RASTER_BLOCKS_PER_CU;
    const uint32_t layerGrid = (((U.width + 7u) / 8u) * ((U.height + 7u) / 8u) + LV_BLOCK / LV_WAVE - 1u) / (LV_BLOCK / LV_WAVE);
    // the instances and the selection of the pooled fragment stage
    const bool fastShade = lv_prism_fast_shade(ctx, U, S, stats);
    const int layerShade = fastShade ? LV_SHADE_PLAIN : S.prism.bands ? LV_SHADE_BANDS : U.useHelicityBands ? LV_SHADE_HELICITY : LV_SHADE_PLAIN;
    const int layerFast = fastShade ? 2 : 0;
    for (uint32_t i = 0; i < passes && S.numSegs != 0; i++) {
        // (LV_PEEL_MASK_DONE: the finished pixels have left the requested-pixel mask, stage A has to look)
        const uint32_t allReq = (allRequested && (i == 0u || !LV_PEEL_MASK_DONE)) ? 1u : 0u;
        if (S.prism.n == 6u)
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RASTER, (k_peel_pass<6><<<passGrid, LV_BLOCK, 0, st>>>(U, S, startOffset, B.slot, B.prevZ, dc,
                                                                                                    allReq, leafList, i == 0u ? 1u : 0u)));
        else
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RASTER, (k_peel_pass<0><<<passGrid, LV_BLOCK, 0, st>>>(U, S, startOffset, B.slot, B.prevZ, dc,
                                                                                                    allReq, leafList, i == 0u ? 1u : 0u)));
        LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_SHADE, lv_peel_launch_layer(st, layerGrid, layerShade, layerFast, U, S, startOffset, B));
    }
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_peel_blit<<<numGroups, LV_WAVE, 0, st>>>(U, T, B.accum, out, numGroups)));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_DEPTH_PEELING);
    return LV_OK;
}

// lv_depth_complexity_get_buffers (accum = layers = null) and lv_depth_peeling_get_buffers
int lv_frame_peel_buffers(lv_ctx* ctx, int mode, float* outAccum, uint32_t* outLayers, uint32_t* outCounts, uint64_t capacityPixels) {
    const bool peel = mode == LV_RENDERING_MODE_DEPTH_PEELING;
    uint64_t pixels;
    int rc;
    if ((rc = lv_read_back_open(ctx, mode, peel ? "mode-9 frame" : "mode-5 frame", ctx->ppllCount,
                                peel ? "lv_depth_peeling_get_buffers" : "lv_depth_complexity_get_buffers", capacityPixels, 1u, "pixels",
                                peel ? 24 : 8, pixels)))
        return rc;
    const size_t accBytes = peel ? size_t(pixels) * 16 : 0, wordBytes = size_t(pixels) * 4;
    float4* dAccum = (float4*)ctx->scratchRays.ptr;
    uint32_t* dLayers = (uint32_t*)((char*)ctx->scratchRays.ptr + accBytes);
    uint32_t* dCounts = dLayers + size_t(pixels);
    LvPeelBuffers B = {nullptr, nullptr, nullptr, nullptr};
    if (peel) B = lv_peel_buffers(ctx, ((size_t(ctx->ppllPaddedW) * ctx->ppllPaddedH + 3) / 4) * 4);
    k_peel_read<<<uint32_t((pixels + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, ctx->stream>>>(
            B, (const uint32_t*)ctx->ppllCount.ptr, ctx->streamed.w, ctx->streamed.h, ctx->ppllPaddedW, ctx->streamed.tile[0], ctx->streamed.tile[1],
            peel ? dAccum : nullptr, peel ? dLayers : nullptr, dCounts);
    return lv_read_back(ctx, {{outAccum, dAccum, accBytes}, {outLayers, dLayers, wordBytes}, {outCounts, dCounts, wordBytes}});
}

// lv_depth_complexity_get_stats: the words of k_dc_reduce
int lv_frame_dc_stats(lv_ctx* ctx, uint64_t out[5]) {
    int rc;
    if ((rc = lv_streamed_require(ctx, LV_RENDERING_MODE_DEPTH_COMPLEXITY, "mode-5 frame", ctx->dcStatsDev, "lv_depth_complexity_get_stats")))
        return rc;
    LvDcStats hs;
    LV_HIP(ctx, hipMemcpyAsync(&hs, ctx->dcStatsDev.ptr, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = hs.total; out[1] = hs.used; out[2] = hs.maxCount; out[3] = hs.minCount == 0xFFFFFFFFu ? 0u : hs.minCount;
    out[4] = uint64_t(ctx->streamed.w) * ctx->streamed.h;
    return LV_OK;
}

// The scene view and the uniforms of mode 1's shading pass: the triangle view with the transfer function's alpha forced to 1
// (fragmentColor.a = 1.0, RayHitCommon.glsl:130-132: ctx->deferredTf, rewritten per call), the pixel's own AO texel
static int lv_deferred_scene(lv_ctx* ctx, LvSceneDev& SD) {
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->deferredTf, size_t(ctx->tfN) * 16))) return rc;
    lv_deferred_launch_tf(ctx->stream, (const float4*)ctx->tf.ptr, ctx->tfN, (float4*)ctx->deferredTf.ptr);
    SD = sceneDevTriangles(ctx);
    SD.tf = (const float4*)ctx->deferredTf.ptr;
    return LV_OK;
}
// The variant of the shading pass, as lv_rt_frame selects the triangle closest-hit shading's
static int lv_deferred_bands(const LvUniforms& U) {
    return U.useHelicityBands ? LV_SHADE_HELICITY : U.useBands ? LV_SHADE_BANDS : LV_SHADE_PLAIN;
}
// What the shading pass of mode 1 is not built for: its AO texel is the pixel's own
static int lv_deferred_check(lv_ctx* ctx, const char* what) {
    if (ctx->opt.useAmbientOcclusion && ctx->opt.aoPrebaked)
        return lv_fail(ctx, LV_E_INVALID, "%s: the prebaked AO table is not built for deferred shading (RTAO (Screen Space) is)", what);
    return LV_OK;
}

// A mode-1 frame (deferred shading on a visibility buffer, lv_deferred.h): clear, k_vis_raster over the tube triangle mesh, the count of
// the winners, k_deferred_shade.  No pool and no host synchronisation; 8 B per padded pixel.  LV_KERNEL_PPLL_RASTER: the visibility
// pass with its clear and the tile marking of a sharded frame; LV_KERNEL_PPLL_RESOLVE: the shading pass.
static int lv_deferred_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool /*stats*/, uint32_t* out,
                             LvDevCounters* dc) {
    hipStream_t st = ctx->stream;
    int rc;
    lv_fill_prism(ctx, U, S.prism);   // the coverage direction's constants
    const size_t padded4 = (size_t(U.ppllPaddedW) * U.ppllPaddedH + 3) / 4, pixels = padded4 * 4;
    if ((rc = lv_buf_reserve(ctx, ctx->visBuf, pixels * 8))) return rc;
    ctx->ppllPoolNodes = 0;
    ctx->ppllPaddedW = U.ppllPaddedW;
    ctx->ppllPaddedH = U.ppllPaddedH;
    const bool allRequested = ctx->tilesCoverViewport;
    LvSceneDev SD;
    if ((rc = lv_deferred_scene(ctx, SD))) return rc;
    SD.prism = S.prism;
    unsigned long long* words = (unsigned long long*)ctx->visBuf.ptr;
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[11], st));
    if ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RASTER) & 1u) LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RASTER, 0), st));
    if (!allRequested) {   // the requested-pixel mask of the other modes (ppllStart: 0 = requested; k_ppll_clear clears ppllCount with it)
        if ((rc = lv_buf_reserve(ctx, ctx->ppllStart, padded4 * 16))) return rc;
        if ((rc = lv_buf_reserve(ctx, ctx->ppllCount, padded4 * 16))) return rc;
        if ((rc = lv_buf_reserve(ctx, ctx->ppllCoarse, size_t((U.width + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE) *
                                                       ((U.height + LV_PRISM_COARSE - 1u) / LV_PRISM_COARSE) * 4))) return rc;
        lv_ppll_clear(ctx, U, padded4, false, false, dc);
        k_ppll_mark_tiles<false><<<gridTiles, LV_BLOCK, 0, st>>>(U, T, (uint32_t*)ctx->ppllStart.ptr, (uint32_t*)ctx->ppllCoarse.ptr, dc);
    }
    const uint32_t* requested = allRequested ? nullptr : (const uint32_t*)ctx->ppllStart.ptr;
    lv_vis_launch_clear(st, words, pixels);
    lv_vis_launch_raster(st, U, SD, ctx->numTris, ctx->opt.useCappedTubes, requested, words);
    if ((rc = lv_segment_raster_end(ctx))) return rc;
    const uint32_t countGrid = std::min<uint32_t>(nblocks(uint64_t(U.width) * U.height), uint32_t(ctx->numCUs) * 4u);
    lv_vis_launch_count(st, countGrid, U, requested, words, dc);
    uint32_t numGroups;
    if ((rc = lv_streamed_close(ctx, T, numGroups))) return rc;
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, lv_deferred_launch_shade(st, numGroups, lv_deferred_bands(U), U, SD, T, words, out));
    lv_streamed_done(ctx, U, LV_RENDERING_MODE_DEFERRED_SHADING);
    return LV_OK;
}

// lv_deferred_get_buffers
int lv_frame_deferred_buffers(lv_ctx* ctx, uint32_t* outPrimitive, float* outDepth, uint64_t capacityPixels) {
    uint64_t pixels;
    int rc;
    if ((rc = lv_read_back_open(ctx, LV_RENDERING_MODE_DEFERRED_SHADING, "mode-1 frame", ctx->visBuf, "lv_deferred_get_buffers", capacityPixels,
                                1u, "pixels", 8, pixels)))
        return rc;
    uint32_t* dPrimitive = (uint32_t*)ctx->scratchRays.ptr;
    float* dDepth = (float*)(dPrimitive + size_t(pixels));
    lv_vis_launch_read(ctx->stream, (const unsigned long long*)ctx->visBuf.ptr, ctx->streamed.w, ctx->streamed.h, ctx->ppllPaddedW,
                       ctx->streamed.tile[0], ctx->streamed.tile[1], dPrimitive, dDepth);
    return lv_read_back(ctx, {{outPrimitive, dPrimitive, size_t(pixels) * 4}, {outDepth, dDepth, size_t(pixels) * 4}});
}

// ---- lv_frame_render: its refusals, its tile list, the two oldest frame functions (mode 11; modes 2, 3 and pooled 6), the frame ----

// How the messages of the modes that work on the prism's fragments alone name them (modes 3, 5, 6, 8, 9 and 10)
static const char* lv_prism_mode_name(int mode) {
    return mode == LV_RENDERING_MODE_DEPTH_COMPLEXITY ? "depth complexity" : mode == LV_RENDERING_MODE_DEPTH_PEELING ? "depth peeling"
         : mode == LV_RENDERING_MODE_WBOIT ? "WBOIT" : mode == LV_RENDERING_MODE_ATOMIC_LOOP_64 ? "Atomic Loop 64"
         : mode == LV_RENDERING_MODE_MBOIT ? "MBOIT" : "MLAB";
}

// a mode-2 or mode-3 frame draws the hull into its fragment pool (lv_hull_pool.h): hull_fragment_pool = on while a hull is drawn
static bool lv_hull_pooled(const lv_ctx* ctx, int mode) {
    return ctx->opt.hullFragmentPool && lv_hull_drawn(ctx) &&
           (mode == LV_RENDERING_MODE_PER_PIXEL_LINKED_LIST || mode == LV_RENDERING_MODE_MLAB);
}

// What a frame call is refused for before anything is built or enqueued: the mode, the options that exclude each other, the state
// the caller has not set.  A call of a supported mode ends the record of the last frame (ctx->streamed: set again at the end of a
// streamed mode-6, a mode-5, 8, 9 or 10 frame, lv_streamed_done), refused or not.
static int lv_frame_check(lv_ctx* ctx, int mode) {
    if (mode != LV_RENDERING_MODE_VULKAN_RAY_TRACER && mode != LV_RENDERING_MODE_PER_PIXEL_LINKED_LIST && mode != LV_RENDERING_MODE_MLAB &&
        mode != LV_RENDERING_MODE_MBOIT && mode != LV_RENDERING_MODE_WBOIT && mode != LV_RENDERING_MODE_ATOMIC_LOOP_64 &&
        mode != LV_RENDERING_MODE_DEPTH_COMPLEXITY && mode != LV_RENDERING_MODE_DEPTH_PEELING && mode != LV_RENDERING_MODE_DEFERRED_SHADING)
        return lv_fail(ctx, LV_E_INVALID, "unsupported rendering mode %d (11 = ray tracer, 1 = deferred shading, 2 = PPLL, 3 = MLAB, "
                                          "5 = depth complexity, 6 = MBOIT, 8 = WBOIT, 9 = depth peeling, 10 = Atomic Loop 64)", mode);
    ctx->streamed = {};
    ctx->rtHitsValid = false;   // (likewise the records of rt_record_hits: set again by a recording frame, lv_rt_frame)
    int rc;
    // the modes whose colour pass works on fragments (mode 1 works on the tube triangle mesh)
    const bool fragments = mode != LV_RENDERING_MODE_VULKAN_RAY_TRACER && mode != LV_RENDERING_MODE_DEFERRED_SHADING;
    if (fragments && mode != LV_RENDERING_MODE_PER_PIXEL_LINKED_LIST && ctx->opt.ppllFragmentSource == 1)
        return lv_fail(ctx, LV_E_INVALID, "mode %d (%s) works on the fragments of the rasterised prism: ppll_fragment_source = "
                                          "capsule_entry is not supported", mode, lv_prism_mode_name(mode));
    if (mode == LV_RENDERING_MODE_DEFERRED_SHADING && (rc = lv_deferred_check(ctx, "mode 1"))) return rc;
    if (!ctx->cameraSet) return lv_fail(ctx, LV_E_STATE, "lv_set_camera has not been called");
    if (!ctx->tf.ptr || ctx->tfN == 0) return lv_fail(ctx, LV_E_STATE, "lv_set_transfer_function has not been called");
    if (!ctx->points.ptr && ctx->numSegs) return lv_fail(ctx, LV_E_STATE, "lv_set_lines has not been called");
    if (ctx->opt.useRibbons) {
        // band data: the closest-hit paths of the ray tracer (analytic geometry modes, or "Triangle Mesh" on the elliptic triangle
        // tubes the host layer tessellates for the data set); RTAO over the analytic tubelets / capsules or over those triangle
        // tubes (rtao_geometry = triangle_tubes); MLAT over the same geometries; the PPLL gather over the analytic tubelets /
        // capsules.  The static prebaker bakes band data on the elliptic cross-section against the elliptic triangle tubes the caller
        // passed (VulkanAmbientOcclusionBaker.glsl:200-257) and is looked up with the band's own angle (phiLine of the tubelets).
        if (fragments && (ctx->opt.rtTriangleMesh || ctx->opt.rtLss))
            return lv_fail(ctx, LV_E_INVALID, "use_ribbons: the PPLL gather of band data runs over the analytic tubelets / capsules "
                                              "(geometry_mode \"AABBs\")");
        if (ctx->opt.rtTriangleMesh && ctx->opt.ellipticTubes)
            return lv_fail(ctx, LV_E_INVALID, "Elliptic Tubes belong to the AABB geometry mode (VulkanRayTracer.cpp:198), not to Triangle Mesh");
    } else if (ctx->opt.ellipticTubes) {
        return lv_fail(ctx, LV_E_INVALID, "use_analytic_elliptic_tubes needs band data (use_ribbons)");
    }
    if (ctx->opt.helicityBands && ctx->opt.useRibbons)
        return lv_fail(ctx, LV_E_INVALID, "rotating_helicity_bands and use_ribbons exclude each other (LineDataFlow.cpp:470,601-604)");
    if (ctx->opt.rtLss && ctx->opt.useRibbons && ctx->opt.ellipticTubes)
        return lv_fail(ctx, LV_E_INVALID, "Elliptic Tubes belong to the AABB geometry mode (VulkanRayTracer.cpp:198), not to Linear Swept Spheres");
    // the simulation-mesh hull: modes 6 and 9 draw none (as the reference); mode 11 ray-traces it under hull_ray_tracing = on
    // (lv_hull_rt.h), closest hits only; the others are not built for it yet
    const bool hullRayTraced = mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER && ctx->opt.hullRayTracing;
    if (mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER && lv_rt_hull_kernel(ctx)) {
        // k_render_rt_hull has no variant for the approximate lighting, and a record holds the step in 16 bits
        if (ctx->opt.fastShading)
            return lv_fail(ctx, LV_E_INVALID, "shading_numerics = fast is not built for the ray-traced hull and for rt_record_hits: set "
                                              "shading_numerics = exact, or hull_ray_tracing = off and rt_record_hits = false");
        if (ctx->opt.rtRecordHits && ctx->opt.maxDepthComplexity > 65536u)
            return lv_fail(ctx, LV_E_INVALID, "rt_record_hits: a record numbers the steps of a loop in 16 bits, max_depth_complexity = %u "
                                              "is more than 65536", ctx->opt.maxDepthComplexity);
    }
    if (lv_hull_drawn(ctx) && hullRayTraced && ctx->opt.useMlat)
        return lv_fail(ctx, LV_E_INVALID, "hull_ray_tracing = on: use_mlat does not draw the simulation-mesh hull (the any-hit variant is not "
                                          "built); set use_mlat = false, hull_opacity = 0 or remove the mesh");
    if (lv_hull_pooled(ctx, mode)) {
        // hull_fragment_pool = on (lv_hull_pool.h): the hull store fills the segment rasteriser's record pool only
        if (ctx->opt.lineQuads)
            return lv_fail(ctx, LV_E_INVALID, "hull_fragment_pool = on: mode %d stores the simulation-mesh hull in the segment rasteriser's "
                                              "record pool, which line_primitive_mode = \"Quads (Programmable Pull)\" does not fill; set it back "
                                              "to \"Tube (Programmable Pull)\", hull_opacity = 0 or remove the mesh", mode);
        if (!lv_ppll_prism_source(ctx))
            return lv_fail(ctx, LV_E_INVALID, "hull_fragment_pool = on: mode %d stores the simulation-mesh hull in the segment rasteriser's "
                                              "record pool, which ppll_fragment_source = capsule_entry does not fill; set it to auto or raster_prism, "
                                              "hull_opacity = 0 or remove the mesh", mode);
        if (ctx->opt.ppllPrismLbvhWalk)
            return lv_fail(ctx, LV_E_INVALID, "hull_fragment_pool = on: mode %d stores the simulation-mesh hull in the segment rasteriser's "
                                              "record pool, which ppll_prism_rasteriser = lbvh does not fill; set it to segments, hull_opacity "
                                              "= 0 or remove the mesh", mode);
        if (mode == LV_RENDERING_MODE_MLAB && !lv_hull_pool_keys_fit(ctx->numSegs, ctx->hullNumTris))
            return lv_fail(ctx, LV_E_INVALID, "hull_fragment_pool = on: mode 3 keys a hull fragment (segments << 6) + triangle; %llu segments "
                                              "and %u hull triangles do not fit 32 bits", (unsigned long long)ctx->numSegs, ctx->hullNumTris);
    }
    if (lv_hull_drawn(ctx) && !hullRayTraced && !lv_hull_pooled(ctx, mode) &&
                              (mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER || mode == LV_RENDERING_MODE_DEFERRED_SHADING ||
                               mode == LV_RENDERING_MODE_PER_PIXEL_LINKED_LIST || mode == LV_RENDERING_MODE_MLAB))
        return lv_fail(ctx, LV_E_INVALID, "mode %d does not draw the simulation-mesh hull yet: modes 5 (depth complexity), 8 (WBOIT) and 10 "
                                          "(Atomic Loop 64) do; set hull_opacity = 0 or remove the mesh (lv_set_hull_mesh with 0 triangles)", mode);
    // line_primitive_mode = "Quads (Programmable Pull)": drawn by modes 5, 8 and 10; modes 1 and 11 never read the primitive mode (as the
    // reference); the others are not built for it, nor are the line data variants below (lv_linequad.h)
    if (ctx->opt.lineQuads && fragments) {
        if (mode != LV_RENDERING_MODE_DEPTH_COMPLEXITY && mode != LV_RENDERING_MODE_WBOIT && mode != LV_RENDERING_MODE_ATOMIC_LOOP_64)
            return lv_fail(ctx, LV_E_INVALID, "mode %d does not draw line_primitive_mode = \"Quads (Programmable Pull)\": modes 5 (depth "
                                              "complexity), 8 (WBOIT) and 10 (Atomic Loop 64) do; set it back to \"Tube (Programmable Pull)\"", mode);
        if (ctx->opt.useRibbons)
            return lv_fail(ctx, LV_E_INVALID, "line quads: use_ribbons (ribbon quads) is not built");
        if (ctx->opt.helicityBands)
            return lv_fail(ctx, LV_E_INVALID, "line quads: rotating_helicity_bands is not built");
        if (ctx->opt.aoPrebaked)
            return lv_fail(ctx, LV_E_INVALID, "line quads: ambient_occlusion_mode = \"RTAO (Prebaker)\" is not built (its lookup needs "
                                              "phi = asin(x)); \"RTAO (Screen Space)\" is");
        if (ctx->opt.ppllPrismLbvhWalk)
            return lv_fail(ctx, LV_E_INVALID, "line quads: ppll_prism_rasteriser = lbvh is not supported");
    }
    return LV_OK;
}

// Do the tiles cover every pixel of the viewport?  (sufficient test: grid-aligned tiles, every grid cell present)
static bool lv_tiles_cover(uint32_t width, uint32_t height, uint32_t tileW, uint32_t tileH, const uint32_t* tiles, uint32_t numTiles) {
    const uint32_t gx = (width + tileW - 1u) / tileW, gy = (height + tileH - 1u) / tileH;
    if (uint64_t(gx) * gy > uint64_t(numTiles)) return false;
    std::vector<uint8_t> cell(size_t(gx) * gy, 0);
    size_t present = 0;
    for (uint32_t t = 0; t < numTiles; t++) {
        const uint32_t tx = tiles[2 * t], ty = tiles[2 * t + 1];
        if (tx % tileW || ty % tileH || tx / tileW >= gx || ty / tileH >= gy) continue;
        uint8_t& c = cell[size_t(ty / tileH) * gx + tx / tileW];
        if (!c) { c = 1; present++; }
    }
    return present == size_t(gx) * gy;
}

// Do two tiles of the list share a pixel (a tile listed twice, tiles off the grid)?  Equal-sized tiles overlap iff |dx| < tileW and
// |dy| < tileH; the grid cells of their origins are then the same or neighbours, and no cell holds the origins of two disjoint tiles.
static bool lv_tiles_overlap(uint32_t tileW, uint32_t tileH, const uint32_t* tiles, uint32_t numTiles) {
    std::unordered_map<uint64_t, uint32_t> cells;   // grid cell of an origin -> its tile
    cells.reserve(numTiles);
    for (uint32_t t = 0; t < numTiles; t++) {
        const uint64_t tx = tiles[2 * t], ty = tiles[2 * t + 1], cx = tx / tileW, cy = ty / tileH;
        for (uint64_t ny = cy ? cy - 1u : 0u; ny <= cy + 1u; ny++)
            for (uint64_t nx = cx ? cx - 1u : 0u; nx <= cx + 1u; nx++) {
                const auto it = cells.find(ny << 32 | nx);
                if (it == cells.end()) continue;
                const uint64_t ox = tiles[2 * it->second], oy = tiles[2 * it->second + 1];
                if ((ox > tx ? ox - tx : tx - ox) < tileW && (oy > ty ? oy - ty : ty - oy) < tileH) return true;
            }
        cells[cy << 32 | cx] = t;
    }
    return false;
}

// The frame's tile list on the device (ctx->tilesDev, reserved by the caller), ctx->tilesCoverViewport and ctx->tilesOverlap.
// The tile list is usually the same from frame to frame (a rank keeps its tiles): it is uploaded only when it changes, so that consecutive frames need no host
// synchronisation and the CPU can enqueue frame k+1 while frame k runs.  The cover test runs again when the list, the viewport or the
// tile size changed (ctx->tilesCoverKey).
static int lv_frame_tiles(lv_ctx* ctx, const uint32_t* tilesXYHost, uint32_t numTiles, uint32_t tileW, uint32_t tileH) {
    hipStream_t st = ctx->stream;
    const bool sameTiles = ctx->tilesUploaded && ctx->tilesHost.size() == 2 * size_t(numTiles) &&
                           memcmp(ctx->tilesHost.data(), tilesXYHost, size_t(numTiles) * 8) == 0;
    if (!sameTiles) {
        if (!ctx->tilesHost.empty()) LV_HIP(ctx, hipStreamSynchronize(st)); // previous staging copy may still be in flight
        ctx->tilesHost.assign(tilesXYHost, tilesXYHost + 2 * size_t(numTiles));
        LV_HIP(ctx, hipMemcpyAsync(ctx->tilesDev.ptr, ctx->tilesHost.data(), size_t(numTiles) * 8, hipMemcpyHostToDevice, st));
        ctx->tilesUploaded = true;
        ctx->tilesHaloUploaded = false;
        ctx->tilesGeneration++;
        ctx->tilesCoverKey[0] = 0u;   // (tilesCoverViewport is recomputed below)
    }
    if (ctx->tilesCoverKey[0] != ctx->width || ctx->tilesCoverKey[1] != ctx->height || ctx->tilesCoverKey[2] != tileW ||
        ctx->tilesCoverKey[3] != tileH) {
        ctx->tilesCoverViewport = lv_tiles_cover(ctx->width, ctx->height, tileW, tileH, tilesXYHost, numTiles);
        ctx->tilesOverlap = numTiles > 1u && lv_tiles_overlap(tileW, tileH, tilesXYHost, numTiles);
        ctx->tilesCoverKey[0] = ctx->width; ctx->tilesCoverKey[1] = ctx->height; ctx->tilesCoverKey[2] = tileW; ctx->tilesCoverKey[3] = tileH;
    }
    return LV_OK;
}

// A mode-11 frame's colour pass: the accumulation image of progressive frames, then use_mlat's single pass (lv_mlat.hip) or ONE launch
// of k_render_rt -- on the hits k_primary_pair traced in the RTAO pass (firstHitsTraced; maxPixels of them per slot of ctx->firstHit),
// or tracing its own first rays.
static int lv_rt_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                       LvDevCounters* dc, bool firstHitsTraced, uint64_t maxPixels) {
    hipStream_t st = ctx->stream;
    int rc;
    if (ctx->opt.numAccumulatedFrames > 1u) {
        // the running mean lives in a full-viewport rgba8 image: a resize restarts it (onResolutionChanged resets
        // accumulatedFramesCounter, VulkanRayTracer.cpp:119-129)
        if (U.frameNumber != 0u && (ctx->accumW != ctx->width || ctx->accumH != ctx->height))
            return lv_fail(ctx, LV_E_STATE, "the viewport changed (%ux%u -> %ux%u): restart the accumulation with frame_number = 0",
                           ctx->accumW, ctx->accumH, ctx->width, ctx->height);
        if ((rc = lv_buf_reserve(ctx, ctx->accum, size_t(ctx->width) * ctx->height * 4))) return rc;
        ctx->accumW = ctx->width;
        ctx->accumH = ctx->height;
        S.accum = (uint32_t*)ctx->accum.ptr;
    }
    // geometry_mode (VulkanRayTracer.cpp:226-250): analytic capsules, or the triangle tubes with their own LBVH
    const bool tri = ctx->opt.rtTriangleMesh;
    LvSceneDev SC = tri ? sceneDevTriangles(ctx) : S;
    SC.accum = S.accum;
    if (U.lssGeometry) SC.literalIntersection = 0u; // the hardware primitive has no intersection shader
    if (ctx->opt.useMlat) { // use_mlat: single-pass approximate transparency (lv_mlat.hip)
        if (tri && (rc = lv_prepare_overflow(ctx, SC, "MLAT pass", gridTiles, LV_STACK_LDS, true))) return rc;
        return lv_mlat_render(ctx, U, SC, T, gridTiles, out, dc, tri);
    }
    if (tri && (rc = lv_prepare_overflow(ctx, SC, "colour pass (triangle mesh)", gridTiles, LV_STACK_LDS, true))) return rc;
    if (lv_rt_hull_kernel(ctx)) {
        // hull_ray_tracing = on with a drawn hull, or a recording frame: k_render_rt_hull (lv_hull_rt.hip).  Its two walks share one
        // stack, so the launch gets the slab if either tree needs it (the frame reserved for the deeper one)
        LvHullRtDev R;
        R.nodes = (const float4*)ctx->hullNodes.ptr;
        R.tris = (const float4*)ctx->hullTris.ptr;
        R.pad = ctx->hullPad;
        R.mesh = lv_hull_dev(ctx);
        if (!lv_hull_drawn(ctx)) R.mesh.numTris = 0u;
        else {
            LvSceneDev SH = SC;
            if ((rc = lv_prepare_overflow(ctx, SH, "colour pass (hull)", gridTiles, LV_STACK_LDS, LV_TREE_HULL))) return rc;
            if (SH.stackOverflow) SC.stackOverflow = SH.stackOverflow;
        }
        uint32_t* rec = nullptr;
        if (ctx->opt.rtRecordHits) {
            if ((rc = lv_buf_reserve(ctx, ctx->rtHits, size_t(ctx->opt.rtHitsCapacity) * LV_RT_HIT_WORDS * 4))) return rc;
            rec = (uint32_t*)ctx->rtHits.ptr;
            ctx->rtHitsValid = ctx->tilesCoverViewport && !ctx->tilesOverlap;   // every pixel's loop exactly once
            ctx->rtHitsFrameCapacity = ctx->opt.rtHitsCapacity;
        }
        return lv_hull_rt_render(ctx, U, SC, R, T, gridTiles, out, dc, tri, rec, ctx->opt.rtHitsCapacity);
    }
#define LV_LAUNCH_RT(ST, PR, BA) \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_RENDER_RT, (k_render_rt<ST, PR, BA><<<gridTiles, LV_BLOCK, 0, st>>>(U, SC, T, out, dc)))
#define LV_LAUNCH_RT_PRE(ST, BA) \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_RENDER_RT, (k_render_rt<ST, LV_PRIM_CAPSULE, BA, true><<<gridTiles, LV_BLOCK, 0, st>>>( \
            U, SC, T, out, dc, (const uint2*)ctx->firstHit.ptr, size_t(maxPixels))))
#define LV_LAUNCH_RT2(ST)                                                        \
    do {                                                                         \
        if (fastPlain && firstHitsTraced)                                        \
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_RENDER_RT, (k_render_rt<false, LV_PRIM_CAPSULE, LV_SHADE_PLAIN, true, 1><<<gridTiles, LV_BLOCK, 0, st>>>( \
                    U, SC, T, out, dc, (const uint2*)ctx->firstHit.ptr, size_t(maxPixels)))); \
        else if (fastPlain)                                                      \
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_RENDER_RT, (k_render_rt<false, LV_PRIM_CAPSULE, LV_SHADE_PLAIN, false, 1><<<gridTiles, LV_BLOCK, 0, st>>>( \
                    U, SC, T, out, dc)));                                        \
        else if (firstHitsTraced && U.useHelicityBands) LV_LAUNCH_RT_PRE(ST, LV_SHADE_HELICITY); \
        else if (firstHitsTraced && U.useBands) LV_LAUNCH_RT_PRE(ST, LV_SHADE_BANDS); \
        else if (firstHitsTraced) LV_LAUNCH_RT_PRE(ST, LV_SHADE_PLAIN);          \
        else if (tri && U.useHelicityBands) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_HELICITY); \
        else if (tri && U.useBands) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_BANDS); \
        else if (tri) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_PLAIN);        \
        else if (U.useHelicityBands) LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_HELICITY); \
        else if (U.useEllipticTubes) LV_LAUNCH_RT(ST, LV_PRIM_ELLIPTIC, LV_SHADE_BANDS); \
        else if (U.useBands) LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_BANDS);  \
        else LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_PLAIN);                  \
    } while (0)
    // shading_numerics = fast: the capsule colour pass of plain flow lines (lighting through the approximate operations, FAST = 1)
    const bool fastPlain = ctx->opt.fastShading && !stats && !tri && !U.useHelicityBands && !U.useEllipticTubes && !U.useBands;
    if (stats) LV_LAUNCH_RT2(true); else LV_LAUNCH_RT2(false);
#undef LV_LAUNCH_RT2
#undef LV_LAUNCH_RT_PRE
#undef LV_LAUNCH_RT
    return LV_OK;
}

// The front end of a frame with a fragment pool (modes 2, 3 and pooled 6) on pools of poolSlots entries: the pools reserved, clear(),
// then gather() -- the fragments of the rasterised programmable-pull prism (the reference's geometry, default) or capsule entry hits.
// Modes 3 and 6 drop no fragment and never return a silently wrong frame: they read back what the rasteriser reserved and whether a
// pixel's 16-bit record count saturated -- one host synchronisation per frame.  need: the slots the frame asked for (mode 2 drops
// what does not fit: 0).
static int lv_pool_front(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats,
                         LvDevCounters* dc, int mode, uint32_t poolSlots, uint32_t& need) {
    hipStream_t st = ctx->stream;
    int rc;
    const bool mboit = mode == LV_RENDERING_MODE_MBOIT, mlab = mode == LV_RENDERING_MODE_MLAB || mboit;
    const char* const poolName = lv_prism_mode_name(mode);
    const bool prismSource = lv_ppll_prism_source(ctx);
    const uint32_t numSlices = prismSource ? 1u : LV_PPLL_SLICES; // (the prism's coverage kernel has no depth: one slice)
    // ppll_prism_rasteriser: "segments" (default) = one lane per segment over its screen rectangle, "lbvh" = the all-hits walk of
    // the viewing rays (k_ppll_gather<LV_PRIM_PRISM>); same coverage test, same fragments
    const bool segmentRaster = prismSource && !ctx->opt.ppllPrismLbvhWalk;
    const uint32_t rasterGrid = uint32_t(ctx->numCUs) * LV_PRISM_RASTER_BLOCKS_PER_CU;
    need = 0u;
    // (mode 6: 16-B colours + 4-B view depths per entry)
    if ((rc = lv_buf_reserve(ctx, ctx->ppllNodes, size_t(poolSlots) * (mboit ? 20 : 12))))
        return mlab ? lv_fail(ctx, LV_E_CAPACITY, "%s: cannot allocate a fragment pool of %u entries", poolName, poolSlots) : rc;
    // raster_prism: the coverage kernel writes 12-B records {pixel, leaf | triangle, rank} into a pool of their own; ppllNodes then
    // holds the fragment array (8-B {colour, depth} entries, one contiguous run per pixel -- 12-B {colour, window depth, key} in
    // mode 3), ppllStart the runs' offsets
    if (prismSource && (rc = lv_buf_reserve(ctx, ctx->prismRecords, size_t(poolSlots) * 12)))
        return mlab ? lv_fail(ctx, LV_E_CAPACITY, "%s: cannot allocate a record pool of %u entries", poolName, poolSlots) : rc;
    ctx->ppllArrays = prismSource;
    uint32_t* gatherPool = prismSource ? (uint32_t*)ctx->prismRecords.ptr : (uint32_t*)ctx->ppllNodes.ptr;
    const size_t padded4 = (size_t(U.ppllPaddedW) * U.ppllPaddedH + 3) / 4; // cleared as whole uint4s (k_ppll_clear)
    if ((rc = lv_buf_reserve(ctx, ctx->ppllStart, padded4 * 16))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllCount, padded4 * 16))) return rc;
    ctx->ppllPoolNodes = poolSlots;
    ctx->ppllPaddedW = U.ppllPaddedW;
    ctx->ppllPaddedH = U.ppllPaddedH;
    const bool allRequested = segmentRaster && ctx->tilesCoverViewport;
    lv_ppll_clear(ctx, U, padded4, allRequested, stats, dc);
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[11], st));
    if (segmentRaster) {
        // the segment rasteriser (k_ppll_raster_prism): requested pixels marked, then one lane per segment
#define LV_LAUNCH_RASTER(ST, NT)                                                                                              \
    k_ppll_raster_prism<ST, NT><<<rasterGrid, LV_BLOCK, 0, st>>>(                                                             \
            U, S, gatherPool, (const uint32_t*)ctx->ppllStart.ptr, (uint32_t*)ctx->ppllCount.ptr, dc, poolSlots,                \
            allRequested ? 1u : 0u, leafList)
        uint32_t* leafList;
        if ((rc = lv_segment_raster_front(ctx, U, S, T, gridTiles, stats, allRequested, dc, leafList))) return rc;
        if (lv_hull_pooled(ctx, mode)) {
            // the hull's records (lv_hull_pool.h), BEFORE the lines': the hull then holds ranks [0, h) of every pixel's run, which
            // its fragment stage hands out again from the counters zeroed here
            if ((rc = lv_buf_reserve(ctx, ctx->hullRanks, padded4 * 16))) return rc;
            LV_HIP(ctx, hipMemsetAsync(ctx->hullRanks.ptr, 0, padded4 * 16, st));
            const LvHullList none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0ull};
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_HULL, lv_hull_launch(st, LV_HULL_STORE_RECORD, uint32_t(ctx->numCUs), U, S.prism, lv_hull_dev(ctx),
                                                                allRequested ? nullptr : (const uint32_t*)ctx->ppllStart.ptr,
                                                                (uint32_t*)ctx->ppllCount.ptr, (unsigned long long*)gatherPool, poolSlots,
                                                                dc, stats, none));
        }
        if (S.numSegs != 0) {
            if (S.prism.n == 6u) { if (stats) LV_LAUNCH_RASTER(true, 6); else LV_LAUNCH_RASTER(false, 6); }
            else { if (stats) LV_LAUNCH_RASTER(true, 0); else LV_LAUNCH_RASTER(false, 0); }
        }
        if ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RASTER) & 1u) {
            LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RASTER, 1), st));
            ctx->kernelLaunches[LV_KERNEL_PPLL_RASTER]++;
        }
#undef LV_LAUNCH_RASTER
    } else {
#define LV_LAUNCH_GATHER(ST, PR, BA)                                                                             \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_GATHER, (k_ppll_gather<ST, PR, BA><<<gridTiles * numSlices, LV_BLOCK, 0, st>>>( \
            U, S, T, gatherPool, (uint32_t*)ctx->ppllStart.ptr,                                                  \
            (uint32_t*)ctx->ppllCount.ptr, dc, numSlices, poolSlots)))
#define LV_LAUNCH_GATHER2(ST)                                                          \
    do {                                                                               \
        if (prismSource) LV_LAUNCH_GATHER(ST, LV_PRIM_PRISM, LV_SHADE_PLAIN);          \
        else if (U.useHelicityBands) LV_LAUNCH_GATHER(ST, LV_PRIM_CAPSULE, LV_SHADE_HELICITY); \
        else if (U.useBands && U.useEllipticTubes) LV_LAUNCH_GATHER(ST, LV_PRIM_ELLIPTIC, LV_SHADE_BANDS); \
        else if (U.useBands) LV_LAUNCH_GATHER(ST, LV_PRIM_CAPSULE, LV_SHADE_BANDS);    \
        else LV_LAUNCH_GATHER(ST, LV_PRIM_CAPSULE, LV_SHADE_PLAIN);                    \
    } while (0)
        if (stats) LV_LAUNCH_GATHER2(true); else LV_LAUNCH_GATHER2(false);
#undef LV_LAUNCH_GATHER2
#undef LV_LAUNCH_GATHER
    }
    if (!mlab) return LV_OK;
    k_mlab_check_counts<<<uint32_t((padded4 + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>((const uint4*)ctx->ppllCount.ptr, padded4, dc);
    if (!ctx->pinned) LV_HIP(ctx, hipHostMalloc((void**)&ctx->pinned, 64, hipHostMallocDefault));
    volatile uint32_t* pin = ctx->pinned + 14;   // (words 14, 15 of the pinned block)
    LV_HIP(ctx, hipMemcpyAsync((void*)pin, &dc->fragAlloc, 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync((void*)(pin + 1), &dc->mlabSaturated, 4, hipMemcpyDeviceToHost, st));
    const bool readBox = mboit && !ctx->mboitBoxValid;
    if (readBox && (rc = lv_mboit_box_queue(ctx, S, dc))) return rc;   // read back with the same synchronisation
    LV_HIP(ctx, hipStreamSynchronize(st));
    if (readBox) lv_mboit_box_adopt(ctx);
    need = pin[0];
    if (pin[1])
        return lv_fail(ctx, LV_E_CAPACITY, "%s: a pixel is covered by more than 65534 fragments (16-bit per-pixel count)", poolName);
    return LV_OK;
}

// A mode-2, mode-3 or pooled mode-6 frame (reallocateFragmentBuffer, PerPixelLinkedListLineRenderer.cpp:251-357): the front end --
// again, ONCE, on a grown pool when a mode-3 or mode-6 frame needed more slots than the pool held --, then for the prism's records the
// scan of the per-pixel counts, the fragment stage and mode 2's selection of the nearest fragments, then resolve().
static int lv_pool_frame(lv_ctx* ctx, LvUniforms& U, LvSceneDev& S, const LvTiles& T, uint32_t gridTiles, bool stats, uint32_t* out,
                         LvDevCounters* dc, int mode) {
    hipStream_t st = ctx->stream;
    int rc;
    // modes 3 and 6 share the front end and the pool that drops nothing (`mlab`); `mboit` picks the entry format and the resolve
    const bool mboit = mode == LV_RENDERING_MODE_MBOIT, mlab = mode == LV_RENDERING_MODE_MLAB || mboit;
    const bool prismSource = lv_ppll_prism_source(ctx);
    if (prismSource && ctx->opt.useRibbons && ctx->opt.helicityBands)
        return lv_fail(ctx, LV_E_INVALID, "ppll_fragment_source = raster_prism: band data with rotating helicity bands has no prism "
                                          "fragment stage (use auto or capsule_entry)");
    if (prismSource && ctx->opt.useRibbons && ctx->opt.ppllPrismLbvhWalk)
        return lv_fail(ctx, LV_E_INVALID, "ppll_prism_rasteriser = lbvh: the segment boxes do not enclose the band prism "
                                          "(band_width / 2); band data uses the segment rasteriser");
    if (prismSource) lv_fill_prism(ctx, U, S.prism);
    const uint32_t numSlices = prismSource ? 1u : LV_PPLL_SLICES;   // (as lv_pool_front launches the gather)
    if (uint64_t(gridTiles) * numSlices > 0x7FFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    // physical pool = the reference's linkedListSize + the tail every wave of the gather may leave unused in its last
    // chunk of node slots (k_ppll_gather / k_ppll_raster_prism), so that the effective capacity is never below the reference's
    const bool segmentRaster = prismSource && !ctx->opt.ppllPrismLbvhWalk;
    uint64_t chunkSlack = segmentRaster ? uint64_t(ctx->numCUs) * LV_PRISM_RASTER_BLOCKS_PER_CU * (LV_BLOCK / LV_WAVE) * LV_PRISM_RASTER_CHUNK
                                              : uint64_t(gridTiles) * numSlices * (LV_BLOCK / LV_WAVE) * LV_PPLL_CHUNK;
    // (+ the tails of the hull launch's waves when, and only when, the hull is drawn into the pool)
    const bool hullPooled = lv_hull_pooled(ctx, mode);
    if (hullPooled) chunkSlack += uint64_t(lv_hull_launch_waves(uint32_t(ctx->numCUs), ctx->hullNumTris, U.height)) * LV_HULL_CHUNK;
    uint64_t poolSlots64 = uint64_t(U.ppllLinkedListSize) + chunkSlack;
    // MLAB drops no fragment (the reference's MLAB has no pool): it starts from the linkedListSize of the options (no chunk slack:
    // a frame that needs more slots grows the pool below) or from what the largest mode-3 frame so far needed
    if (mlab) poolSlots64 = std::max<uint64_t>(U.ppllLinkedListSize, ctx->mlabPoolSlots);
    if (poolSlots64 > 0xFFFFFFF0ull) poolSlots64 = 0xFFFFFFF0ull; // node indices are 32 bit
    uint32_t poolSlots = uint32_t(poolSlots64);
    // a regrown mode-3 frame runs its front end twice: the statistics it adds (rays, nodes, prims, hits; k_ppll_clear resets the
    // fragment counters) are restored from this copy before the second run.  (The per-kernel timers keep both runs' launches.)
    const bool mlabStatsSnap = mlab && stats;
    if (mlabStatsSnap) {
        if ((rc = lv_buf_reserve(ctx, ctx->mlabStatsSnap, 4 * sizeof(unsigned long long)))) return rc;
        LV_HIP(ctx, hipMemcpyAsync(ctx->mlabStatsSnap.ptr, &dc->rays, 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    }
    for (int round = 0;; round++) {
        uint32_t need;
        if ((rc = lv_pool_front(ctx, U, S, T, gridTiles, stats, dc, mode, poolSlots, need))) return rc;
        if (need <= poolSlots) break;
        // (modes 3 and 6: the rasteriser needed more record slots than the pool held -- grown, and the front end runs again)
        const uint64_t grown = uint64_t(need) + chunkSlack;
        if (round || grown > 0xFFFFFFF0ull)
            return lv_fail(ctx, LV_E_CAPACITY, "%s: the frame needs %llu fragment slots (pool: %u)", lv_prism_mode_name(mode),
                           (unsigned long long)grown, poolSlots);
        poolSlots = uint32_t(grown);
        ctx->mlabPoolSlots = poolSlots;
        if (mlabStatsSnap)
            LV_HIP(ctx, hipMemcpyAsync(&dc->rays, ctx->mlabStatsSnap.ptr, 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    }
    uint32_t* blockBase = nullptr;
    if (prismSource) {
        // per-pixel counts -> offsets of the pixels' runs + the list of the pixels with more records than the sort arrays hold
        const size_t padded4 = (size_t(U.ppllPaddedW) * U.ppllPaddedH + 3) / 4;   // (whole uint4s, as lv_pool_front reserved them)
        const uint32_t numAddr = uint32_t(padded4 * 4);
        const uint32_t scanBlocks = (numAddr + LV_SCAN_ITEMS - 1u) / LV_SCAN_ITEMS;
        if ((rc = lv_buf_reserve(ctx, ctx->ppllOverflow, padded4 * 16))) return rc;
        if ((rc = lv_buf_reserve(ctx, ctx->scanTemp, (2 * size_t(scanBlocks) + 1) * 4))) return rc;
        uint32_t* blockTotals = (uint32_t*)ctx->scanTemp.ptr;
        blockBase = blockTotals + scanBlocks;
        // (mode 3 keeps every fragment: no pixel goes on the list)
        k_ppll_scan<<<scanBlocks, LV_BLOCK, 0, st>>>((const uint32_t*)ctx->ppllCount.ptr, (uint32_t*)ctx->ppllStart.ptr, numAddr,
                                                    blockTotals, mlab ? 0xFFFFFFFFu : U.ppllMaxNumFrags,
                                                    (uint32_t*)ctx->ppllOverflow.ptr, dc);
        k_ppll_scan_bases<<<1, LV_BLOCK, 0, st>>>(blockTotals, blockBase, scanBlocks);
        ctx->ppllScanBlocks = scanBlocks;
        const uint32_t shadeGrid = uint32_t(ctx->numCUs) * LV_PRISM_SHADE_BLOCKS_PER_CU;
#define LV_LAUNCH_SHADE(ST, BA, FA, ML)                                                                                         \
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_SHADE, (k_ppll_shade_prism<ST, BA, FA, ML><<<shadeGrid, LV_BLOCK, 0, st>>>(             \
            U, S, (const uint32_t*)ctx->prismRecords.ptr, (uint2*)ctx->ppllNodes.ptr, (const uint32_t*)ctx->ppllStart.ptr,      \
            blockBase, (uint32_t*)ctx->ppllCount.ptr, dc, poolSlots)))
#define LV_LAUNCH_SHADE2(ST, ML)                                                     \
    do {                                                                             \
        if (fastShade) LV_LAUNCH_SHADE(false, LV_SHADE_PLAIN, 2, ML);                \
        else if (S.prism.bands) LV_LAUNCH_SHADE(ST, LV_SHADE_BANDS, 0, ML);          \
        else if (U.useHelicityBands) LV_LAUNCH_SHADE(ST, LV_SHADE_HELICITY, 0, ML);  \
        else LV_LAUNCH_SHADE(ST, LV_SHADE_PLAIN, 0, ML);                             \
    } while (0)
#define LV_LAUNCH_SHADE3(ML) do { if (stats) LV_LAUNCH_SHADE2(true, ML); else LV_LAUNCH_SHADE2(false, ML); } while (0)
        const bool fastShade = lv_prism_fast_shade(ctx, U, S, stats);
        if (mboit) LV_LAUNCH_SHADE3(LV_ENTRY_MBOIT);
        else if (mlab) LV_LAUNCH_SHADE3(LV_ENTRY_MLAB);
        else LV_LAUNCH_SHADE3(LV_ENTRY_PPLL);
#undef LV_LAUNCH_SHADE3
#undef LV_LAUNCH_SHADE2
#undef LV_LAUNCH_SHADE
        // the fragment stage of the hull's records (lv_hull_pool.h): other slots of the pool, other entries of the runs
        if (hullPooled)
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_HULL, lv_hull_shade_launch(st, mlab ? LV_ENTRY_MLAB : LV_ENTRY_PPLL, uint32_t(ctx->numCUs), U, S.prism,
                                                                      lv_hull_dev(ctx), (const uint32_t*)ctx->prismRecords.ptr,
                                                                      (uint32_t*)ctx->ppllNodes.ptr, (const uint32_t*)ctx->ppllStart.ptr,
                                                                      blockBase, (uint32_t*)ctx->ppllCount.ptr, (uint32_t*)ctx->hullRanks.ptr,
                                                                      dc, poolSlots, ctx->numSegs << 6));   // (lv_frame_check: the keys fit 32 bits)
        // the listed pixels: their nearest ppllMaxNumFrags fragments to the front of the run
        if (!mlab) k_ppll_select_nearest<<<uint32_t(ctx->numCUs) * 16u, LV_WAVE, 0, st>>>(
                U, (uint2*)ctx->ppllNodes.ptr, (uint2*)ctx->prismRecords.ptr, (const uint32_t*)ctx->ppllStart.ptr, blockBase,
                (const uint32_t*)ctx->ppllCount.ptr, (const uint32_t*)ctx->ppllOverflow.ptr, dc);
    }
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[13], st));
    // resolve()
    if (lv_tiles_cells(T) > 0xFFFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    const uint32_t numGroups = uint32_t(lv_tiles_cells(T));
    if (mlab) {
        // the fold: k_mlab_resolve, then the pixels with long runs (k_mlab_resolve_long); both in the LV_KERNEL_PPLL_RESOLVE slot
        const bool timed = ((ctx->opt.timerMask >> LV_KERNEL_PPLL_RESOLVE) & 1u) != 0u;
        if (timed) LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RESOLVE, 0), st));
        if (mboit) {
            const LvMboitParams M = lv_mboit_params(ctx, U, ctx->mboitBoxOrd, stats);
            if ((rc = lv_mboit_resolve(ctx, U, T, M, numGroups, poolSlots, blockBase, out, nullptr, dc))) return rc;
        } else if ((rc = lv_mlab_fold(ctx, U, T, numGroups, blockBase, out, (uint2*)ctx->prismRecords.ptr, dc))) return rc;
        if (timed) {
            LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, LV_KERNEL_PPLL_RESOLVE, 1), st));
            ctx->kernelLaunches[LV_KERNEL_PPLL_RESOLVE]++;
        }
        return LV_OK;
    }
    const uint32_t* prismCount = prismSource ? (const uint32_t*)ctx->ppllCount.ptr : nullptr; // (kept fragments per pixel -> max depth complexity)
    const size_t ldsBytes = size_t(U.ppllMaxNumFrags) * LV_WAVE * 8;
#define LV_LAUNCH_RESOLVE(LDS, PQ, GRID, BYTES, SCRATCH)                                                                        \
    do {                                                                                                                       \
        if (prismSource)                                                                                                       \
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_ppll_resolve<LDS, PQ, true><<<GRID, LV_WAVE, BYTES, st>>>(        \
                    U, T, (const uint32_t*)ctx->ppllNodes.ptr, (const uint32_t*)ctx->ppllStart.ptr, out, SCRATCH, numGroups,   \
                    prismCount, dc, blockBase)));                                                                              \
        else                                                                                                                   \
            LV_TIMED_LAUNCH(ctx, LV_KERNEL_PPLL_RESOLVE, (k_ppll_resolve<LDS, PQ, false><<<GRID, LV_WAVE, BYTES, st>>>(       \
                    U, T, (const uint32_t*)ctx->ppllNodes.ptr, (const uint32_t*)ctx->ppllStart.ptr, out, SCRATCH, numGroups,   \
                    nullptr, dc, nullptr)));                                                                                   \
    } while (0)
    if (ldsBytes <= LV_RESOLVE_LDS_MAX) {
        if (U.ppllSortingMode == 0u) LV_LAUNCH_RESOLVE(true, true, numGroups, ldsBytes, nullptr);
        else LV_LAUNCH_RESOLVE(true, false, numGroups, ldsBytes, nullptr);
    } else {
        const uint32_t grid = numGroups < LV_RESOLVE_SLAB_GRID ? numGroups : LV_RESOLVE_SLAB_GRID;
        if ((rc = lv_buf_reserve(ctx, ctx->ppllScratch, size_t(grid) * ldsBytes))) return rc;
        if (U.ppllSortingMode == 0u) LV_LAUNCH_RESOLVE(false, true, grid, 0, (uint32_t*)ctx->ppllScratch.ptr);
        else LV_LAUNCH_RESOLVE(false, false, grid, 0, (uint32_t*)ctx->ppllScratch.ptr);
    }
#undef LV_LAUNCH_RESOLVE
    return LV_OK;
}

// A frame: the checks, what the frame reads brought up to date (line points, acceleration structures, uniforms, tiles), the depth
// range, the RTAO pass or the prebaked table, then the mode's frame function between the phase marks.
int lv_frame_render(lv_ctx* ctx, int mode, const uint32_t* tilesXYHost, uint32_t numTiles, uint32_t tileW,
                    uint32_t tileH, void* outDevice) {
    int rc;
    if ((rc = lv_frame_check(ctx, mode))) return rc;
    if (numTiles == 0 || tileW == 0 || tileH == 0) return lv_fail(ctx, LV_E_INVALID, "empty tile list");
    const bool rayTracer = mode == LV_RENDERING_MODE_VULKAN_RAY_TRACER;
    if ((rc = lv_ensure_line_points(ctx))) return rc;   // lv_set_trajectories' records follow the band / helicity switches
    if (!ctx->accelValid || ctx->accelLineWidth != lv_accel_width(ctx))
        if ((rc = lv_bvh_build(ctx))) return rc;
    const bool needTriangles = (ctx->opt.useAmbientOcclusion && ctx->opt.aoPrebaked) ||
                               (ctx->opt.useAmbientOcclusion && lv_ao_triangle_tubes(ctx)) || (ctx->opt.rtTriangleMesh && rayTracer);
    if (needTriangles) {
        if ((rc = lv_ensure_tube_mesh(ctx))) return rc;
        if (!ctx->triMeshSet)
            return lv_fail(ctx, LV_E_STATE, "rtao_geometry = triangle_tubes / geometry_mode = Triangle Mesh / the RTAO "
                                            "prebaker need lv_set_tube_triangle_mesh");
        if (!ctx->triAccelValid || ctx->triAccelLineWidth != ctx->opt.lineWidth)
            if ((rc = lv_bvh_build_triangles(ctx))) return rc;
    }
    // hull_ray_tracing / rt_record_hits: the colour pass is k_render_rt_hull; the hull's LBVH is built by the first frame that walks it
    const bool hullKernel = rayTracer && lv_rt_hull_kernel(ctx);
    if (hullKernel && lv_hull_drawn(ctx) && !ctx->hullAccelValid && (rc = lv_bvh_build_hull(ctx))) return rc;
    if (mode == LV_RENDERING_MODE_DEFERRED_SHADING) {   // the mesh itself, no LBVH over it
        if ((rc = lv_ensure_tube_mesh(ctx))) return rc;
        if (!ctx->triMeshSet || ctx->numTris == 0u)
            return lv_fail(ctx, LV_E_STATE, "mode 1 (deferred shading) rasterises the tube triangle mesh: lv_set_tube_triangle_mesh or "
                                            "lv_set_trajectories has not been called");
    }

    hipStream_t st = ctx->stream;
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    // AO lookup of the colour pass: literal projection + bilinear sample for jittered primary rays (ray tracer only; the PPLL
    // fragments sit at pixel centres), the pixel's own texel otherwise
    U.aoProjectLookup = (rayTracer && U.useJitteredRays && U.useAmbientOcclusion && !U.aoPrebaked) ? 1u : 0u;
    if ((rc = lv_buf_reserve(ctx, ctx->counters, sizeof(LvDevCounters)))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->depthMinMax, 16))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->tilesDev, size_t(numTiles) * 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ao, size_t(ctx->width) * ctx->height * 4))) return rc;
    if (ctx->aoW != ctx->width || ctx->aoH != ctx->height) ctx->aoResult = nullptr; // images of another viewport size
    ctx->aoW = ctx->width;
    ctx->aoH = ctx->height;
    LvDevCounters* dc = (LvDevCounters*)ctx->counters.ptr;

    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[2], st));
    if ((rc = lv_frame_tiles(ctx, tilesXYHost, numTiles, tileW, tileH))) return rc;
    LV_HIP(ctx, hipMemsetAsync(dc, 0, sizeof(LvDevCounters), st));

    LvTiles T = lv_tiles((const uint32_t*)ctx->tilesDev.ptr, numTiles, tileW, tileH);
    if (lv_tiles_blocks(T) > 0x7FFFFFF0ull) return lv_fail(ctx, LV_E_INVALID, "tile list too large");
    ctx->groupOrderSorted = false;
    ctx->groupOrder[1].active = false;
    if ((rc = lv_group_order_prepare(ctx, T, 0))) return rc;
    const uint32_t gridTiles = uint32_t(lv_tiles_grid(T));
    const uint64_t maxPixels = lv_tiles_pixels(T);
    const bool stats = ctx->opt.collectStats;
    // overlap_primary_passes (default on): the colour pass' first-hit trace rides along with the RTAO primaries (k_primary_pair) and the
    // colour kernel after the RTAO pass only shades.  Where it applies: the ray tracer on the analytic capsules, one sample per pixel
    // (the first ray of a pixel is then its only first ray), the per-frame RTAO pass on the caller's tiles (SVGF covers the viewport).
    // "auto": while the colour pass' tile kernel is at most four rounds of workgroups (16 per CU; half a 1920 x 1080 frame) -- a frame
    // that fills the GPU several times over is throughput-bound in both passes and only pays the second shading (measured, EXPERIMENTS 13.2)
    const bool pairWanted = ctx->opt.overlapPrimaryPasses == 1 || (ctx->opt.overlapPrimaryPasses == 2 && gridTiles <= 16u * uint32_t(ctx->numCUs));
    // (k_render_rt_hull traces every step itself: a frame does not depend on the option either way)
    const bool pairPrimaries = pairWanted && rayTracer && !hullKernel && U.useAmbientOcclusion &&
                               !U.aoPrebaked && !ctx->opt.useMlat && !ctx->opt.rtTriangleMesh && !U.useEllipticTubes &&
                               !ctx->opt.svgfEnabled && !ctx->opt.shEnabled && (U.useJitteredRays ? U.numSamplesPerFrame : 1u) == 1u && ctx->numSegs > 0u &&
                               (ctx->opt.numAccumulatedFrames <= 1u || ctx->opt.frameNumber < ctx->opt.aoIterations);
    // one reservation for every launch of this frame: no view built below can move the slab
    const size_t need = lv_frame_overflow_bytes(ctx, U, T, mode, pairPrimaries);
    if (need && (rc = lv_buf_reserve(ctx, ctx->stackOverflow, need))) return rc;
    LvSceneDev S = sceneDev(ctx);
    if ((rc = lv_prepare_overflow(ctx, S, "colour pass", gridTiles))) return rc;

    // LineRenderer::renderBase: depth range, LineRenderer.cpp:248-256
    if (U.useDepthCues) {
        k_depth_init<<<1, 64, 0, st>>>(U, dc);
        if (ctx->numPoints)
            k_depth_minmax<<<nblocks(ctx->numPoints), LV_BLOCK, 0, st>>>(U, S.points, ctx->numPoints, dc);
        k_depth_finalize<<<1, 64, 0, st>>>(dc, (float*)ctx->depthMinMax.ptr);
    }
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[5], st));

    // ambientOcclusionBaker->updateIterative(), LineRenderer.cpp:257-264
    ctx->aoNumGroups = 0;
    bool firstHitsTraced = false;
    if (U.useAmbientOcclusion && !U.aoPrebaked) {
        LvSceneDev SP = S;
        if (pairPrimaries) {
            if (U.lssGeometry) SP.literalIntersection = 0u; // as the colour pass (lv_rt_frame)
            if ((rc = lv_buf_reserve(ctx, ctx->firstHit, size_t(maxPixels) * 8 * LV_PRE_HITS))) return rc;
        }
        if ((rc = lv_run_ao(ctx, U, S, T, pairPrimaries ? &SP : nullptr, &firstHitsTraced))) return rc;
    }
    if (U.aoPrebaked && !ctx->bakeValid && ctx->bakeAsyncPending) {
        // a bake is running on the second stream (lv_bake_ao_start): adopt its table if it has finished; otherwise this frame is
        // rendered without ambient occlusion -- "display the AO once baking has finished" (AmbientOcclusionBaker.hpp:66-70)
        if ((rc = lv_bake_poll(ctx, false))) return rc;
        if (!ctx->bakeValid && ctx->bakeAsyncPending) { U.aoPrebaked = 0u; U.useAmbientOcclusion = 0u; }
    }
    if (U.aoPrebaked) {
        // static prebaker: view independent, (re)baked only when geometry or baking settings changed
        if (!ctx->bakeValid) {
            if ((rc = lv_bake_ambient_occlusion(ctx, false, true))) return rc;
        }
        S.bakedAo = (const float*)ctx->bakedAo.ptr;
        S.bakedBlendingWeights = (const float*)ctx->bakeBlendingWeights.ptr;
    }
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[7], st));
    // The colour pass of a raster_prism frame with the segment rasteriser has no tile kernel: only its resolve pass could use the
    // dispatch order, and measured it does not (config 4: 0.134 ms as numbered, 0.145 ms heaviest first + 11 us for k_group_order)
    if (!rayTracer && lv_ppll_prism_source(ctx) && !ctx->opt.ppllPrismLbvhWalk && !ctx->groupOrderSorted) {
        T.groupOrder = nullptr;
        T.groupCost = nullptr;
        ctx->groupOrder[0].active = false;
    }
    if ((rc = lv_group_order_sort(ctx))) return rc; // (queued by the RTAO pass already when that ran)

    uint32_t* out = (uint32_t*)outDevice;
    switch (mode) {
    case LV_RENDERING_MODE_VULKAN_RAY_TRACER: rc = lv_rt_frame(ctx, U, S, T, gridTiles, stats, out, dc, firstHitsTraced, maxPixels); break;
    case LV_RENDERING_MODE_MBOIT:
        rc = ctx->opt.mboitStreamed ? lv_mboit_stream_frame(ctx, U, S, T, gridTiles, stats, out, dc)
                                    : lv_pool_frame(ctx, U, S, T, gridTiles, stats, out, dc, mode);
        break;
    case LV_RENDERING_MODE_WBOIT: rc = lv_wboit_frame(ctx, U, S, T, gridTiles, stats, out, dc); break;
    case LV_RENDERING_MODE_DEPTH_COMPLEXITY: rc = lv_dc_frame(ctx, U, S, T, gridTiles, stats, out, dc); break;
    case LV_RENDERING_MODE_DEPTH_PEELING: rc = lv_peel_frame(ctx, U, S, T, gridTiles, stats, out, dc); break;
    case LV_RENDERING_MODE_ATOMIC_LOOP_64: rc = lv_al64_frame(ctx, U, S, T, gridTiles, stats, out, dc); break;
    case LV_RENDERING_MODE_DEFERRED_SHADING: rc = lv_deferred_frame(ctx, U, S, T, gridTiles, stats, out, dc); break;
    default: rc = lv_pool_frame(ctx, U, S, T, gridTiles, stats, out, dc, mode); break;   // modes 2 and 3
    }
    if (rc) return rc;
    LV_HIP(ctx, hipGetLastError());
    if (ctx->opt.timerMask >> 31) LV_HIP(ctx, hipEventRecord(ctx->ev[3], st));
    ctx->evFrameValid = true;
    ctx->evPhaseRecorded = (ctx->opt.timerMask >> 31) != 0u;
    ctx->lastMode = mode;
    return LV_OK;
}

int lv_frame_trace_rays(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n, float* outT,
                        uint32_t* outSeg, uint32_t* outKind) {
    int rc;
    if ((rc = lv_ensure_line_points(ctx))) return rc;
    if (!ctx->accelValid || ctx->accelLineWidth != lv_accel_width(ctx))
        if ((rc = lv_bvh_build(ctx))) return rc;
    if (n == 0) return LV_OK;
    hipStream_t st = ctx->stream;
    const size_t rb = size_t(n) * 12;
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 2 * rb + size_t(n) * 12))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    float* dO = (float*)base;
    float* dD = (float*)(base + rb);
    float* dT = (float*)(base + 2 * rb);
    uint32_t* dS = (uint32_t*)(base + 2 * rb + size_t(n) * 4);
    uint32_t* dK = (uint32_t*)(base + 2 * rb + size_t(n) * 8);
    LV_HIP(ctx, hipMemcpyAsync(dO, o, rb, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(dD, d, rb, hipMemcpyHostToDevice, st));
    LvSceneDev S = sceneDev(ctx);
    if ((rc = lv_reserve_overflow(ctx, S, "lv_trace_rays", nblocks(n)))) return rc;
    if (ctx->opt.useRibbons && ctx->opt.ellipticTubes) // the elliptic tubelets of the band data (kind = 0)
        k_trace_rays<LV_PRIM_ELLIPTIC><<<nblocks(n), LV_BLOCK, 0, st>>>(S, ctx->opt.lineWidth * 0.5f, ctx->opt.useCappedTubes, dO,
                                                                        dD, tMin, tMax, n, dT, dS, dK);
    else if (ctx->opt.traceRaysHardwareInv) // traversal_reciprocal = hardware: the node steps' reciprocals as in k_ao_rays (lv_traversal_inv)
        k_trace_rays<LV_PRIM_CAPSULE, true><<<nblocks(n), LV_BLOCK, 0, st>>>(S, ctx->opt.lineWidth * 0.5f, ctx->opt.useCappedTubes, dO,
                                                                             dD, tMin, tMax, n, dT, dS, dK);
    else
        k_trace_rays<LV_PRIM_CAPSULE><<<nblocks(n), LV_BLOCK, 0, st>>>(S, ctx->opt.lineWidth * 0.5f, ctx->opt.useCappedTubes, dO,
                                                                       dD, tMin, tMax, n, dT, dS, dK);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(outT, dT, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(outSeg, dS, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(outKind, dK, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// ---------------------------------------------------------------- the *_resolve_only entry points: the caller's runs through a resolve
// The one tile (txy, w x h) they resolve, uploaded into ctx->tilesDev (reserved by the caller; txy outlives the call's last
// synchronisation), and the grid of its resolve
static int lv_single_tile(lv_ctx* ctx, const uint32_t* txy, uint32_t w, uint32_t h, LvTiles& T, uint32_t& numGroups) {
    ctx->tilesUploaded = false; // tilesDev is overwritten below
    LV_HIP(ctx, hipMemcpyAsync(ctx->tilesDev.ptr, txy, 8, hipMemcpyHostToDevice, ctx->stream));
    T = lv_tiles((const uint32_t*)ctx->tilesDev.ptr, 1, w, h);
    numGroups = uint32_t(lv_tiles_cells(T));
    return LV_OK;
}
// ... and the resolved rectangle (ctx->outDev) back to the caller, with the call's other arrays (`more`; dst null: not asked for)
static int lv_resolve_read_back(lv_ctx* ctx, uint8_t* out, size_t numPixels, LvCopyBack more0 = {}, LvCopyBack more1 = {}) {
    return lv_read_back(ctx, {{out, ctx->outDev.ptr, numPixels * 4}, more0, more1});
}
// row-major addressing of a w x h rectangle: one 1 x 1-pixel tiling, address = y * w + x
static void lv_row_major_uniforms(lv_ctx* ctx, LvUniforms& U, uint32_t w, uint32_t h) {
    lv_fill_uniforms(ctx, U);
    U.width = w; U.height = h;
    U.ppllTileW = 1u; U.ppllTileH = 1u; U.ppllPaddedW = w; U.ppllPaddedH = h;
}

// Given lists (modes 3, 6, 8, 9 and 10): pixel p of the w x h rectangle owns entries [offsets[p], offsets[p + 1]), in any order.
// What a mode admits: fewer than maxEntries `noun` and at most maxPixels pixels (the 32-bit indices of its kernels), at most maxCount
// of them in a pixel (0xFFFFFFFF: no maximum of its own -- a run is shorter than maxEntries)
struct LvRunLimits { const char* noun; uint64_t maxEntries, maxPixels; uint32_t maxCount; };
// The check every such call starts with, in this order: the sizes, else LV_E_CAPACITY; the offsets, else LV_E_INVALID.  The mode's
// checks of reserved values follow it, and nothing of the context is touched before all of them have passed.  longest: the longest run
static int lv_runs_from_offsets(lv_ctx* ctx, const LvRunLimits& lim, const uint64_t* offsets, uint64_t numPixels, uint64_t numEntries,
                                uint64_t* longest = nullptr) {
    if (numEntries >= lim.maxEntries || numPixels > lim.maxPixels) return lv_fail(ctx, LV_E_CAPACITY, "too many %s or pixels", lim.noun);
    if (offsets[0] != 0 || offsets[numPixels] != numEntries)
        return lv_fail(ctx, LV_E_INVALID, "offsets must run from 0 to the number of %s", lim.noun);
    uint64_t most = 0;
    for (uint64_t p = 0; p < numPixels; p++) {
        if (offsets[p + 1] < offsets[p] || offsets[p + 1] - offsets[p] > lim.maxCount)
            return lv_fail(ctx, LV_E_INVALID, "pixel %llu: offsets must ascend, at most %u %s per pixel", (unsigned long long)p,
                           lim.maxCount, lim.noun);
        most = std::max(most, offsets[p + 1] - offsets[p]);
    }
    if (longest) *longest = most;
    return LV_OK;
}
// What such a call does to the context around its own kernels: row-major uniforms; the buffers it takes over -- ppllNodes for the
// entries (entrySize bytes each), counters, tilesDev, outDev, and those of the runs' shape (below) --, after which no *_get_* call
// finds a frame; the entries uploaded, the counters zeroed, the tile at the origin and the grid of its resolve
struct LvGivenLists {
    LvUniforms U;
    LvTiles T;
    uint32_t numGroups;
    std::vector<uint32_t> runs;   // lv_upload_start_count: the host arrays, sources of uploads until the call's last synchronisation
};
static int lv_upload_runs(lv_ctx* ctx, const void* entries, uint64_t numEntries, size_t entrySize, uint32_t w, uint32_t h, LvGivenLists& G) {
    static const uint32_t txy[2] = {0u, 0u};
    hipStream_t st = ctx->stream;
    int rc;
    lv_row_major_uniforms(ctx, G.U, w, h);
    if ((rc = lv_buf_reserve(ctx, ctx->ppllNodes, size_t(numEntries ? numEntries : 1) * entrySize))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->counters, sizeof(LvDevCounters)))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->tilesDev, 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->outDev, size_t(w) * h * 4))) return rc;
    ctx->streamed = {};   // (ppllCount, the mode's buffer and the padded size no longer belong to a frame)
    if (numEntries) LV_HIP(ctx, hipMemcpyAsync(ctx->ppllNodes.ptr, entries, size_t(numEntries) * entrySize, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemsetAsync(ctx->counters.ptr, 0, sizeof(LvDevCounters), st));
    return lv_single_tile(ctx, txy, w, h, G.T, G.numGroups);
}
// The runs as modes 3 and 6 take them, whose resolves are the frame's own: 32-bit starts and counts in ppllStart and ppllCount
static int lv_upload_start_count(lv_ctx* ctx, const uint64_t* offsets, size_t numPixels, std::vector<uint32_t>& runs) {
    runs.resize(2 * numPixels);
    for (size_t p = 0; p < numPixels; p++) {
        runs[p] = uint32_t(offsets[p]);
        runs[numPixels + p] = uint32_t(offsets[p + 1] - offsets[p]);
    }
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllStart, numPixels * 4))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllCount, numPixels * 4))) return rc;
    LV_HIP(ctx, hipMemcpyAsync(ctx->ppllStart.ptr, runs.data(), numPixels * 4, hipMemcpyHostToDevice, ctx->stream));
    LV_HIP(ctx, hipMemcpyAsync(ctx->ppllCount.ptr, runs.data() + numPixels, numPixels * 4, hipMemcpyHostToDevice, ctx->stream));
    return LV_OK;
}
// The runs as modes 8, 9 and 10 take them, whose *_given kernels look a lane's pixel up: the 64-bit offsets in ppllScratch, and the
// per-pixel counts those kernels add to (ppllCount) zeroed
static int lv_upload_offsets(lv_ctx* ctx, const uint64_t* offsets, size_t numPixels) {
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllScratch, (numPixels + 1) * 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllCount, numPixels * 4))) return rc;
    LV_HIP(ctx, hipMemcpyAsync(ctx->ppllScratch.ptr, offsets, (numPixels + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    LV_HIP(ctx, hipMemsetAsync(ctx->ppllCount.ptr, 0, numPixels * 4, ctx->stream));
    return LV_OK;
}

int lv_frame_ppll_resolve_only(lv_ctx* ctx, const uint32_t* nodes, uint64_t numNodes, const uint32_t* start,
                               uint64_t numPixels, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint8_t* out) {
    if (!ctx->cameraSet) return lv_fail(ctx, LV_E_STATE, "lv_set_camera has not been called");
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    if (numPixels != uint64_t(U.ppllPaddedW) * U.ppllPaddedH)
        return lv_fail(ctx, LV_E_INVALID, "start_offset must hold padded_w * padded_h = %llu entries",
                       (unsigned long long)(uint64_t(U.ppllPaddedW) * U.ppllPaddedH));
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllNodes, size_t(numNodes ? numNodes : 1) * 12))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllStart, size_t(numPixels) * 4))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->tilesDev, 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->outDev, size_t(w) * h * 4))) return rc;
    if (numNodes) LV_HIP(ctx, hipMemcpyAsync(ctx->ppllNodes.ptr, nodes, size_t(numNodes) * 12, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(ctx->ppllStart.ptr, start, size_t(numPixels) * 4, hipMemcpyHostToDevice, st));
    const uint32_t txy[2] = {x0, y0};
    LvTiles T;
    uint32_t numGroups;
    if ((rc = lv_single_tile(ctx, txy, w, h, T, numGroups))) return rc;
    LV_HIP(ctx, hipStreamSynchronize(st));
    const size_t ldsBytes = size_t(U.ppllMaxNumFrags) * LV_WAVE * 8;
    const uint32_t* nd = (const uint32_t*)ctx->ppllNodes.ptr;
    const uint32_t* so = (const uint32_t*)ctx->ppllStart.ptr;
    uint32_t* od = (uint32_t*)ctx->outDev.ptr;
    const bool pq = U.ppllSortingMode == 0u;
    if (ldsBytes <= LV_RESOLVE_LDS_MAX) {
        if (pq) k_ppll_resolve<true, true><<<numGroups, LV_WAVE, ldsBytes, st>>>(U, T, nd, so, od, nullptr, numGroups, nullptr, nullptr, nullptr);
        else k_ppll_resolve<true, false><<<numGroups, LV_WAVE, ldsBytes, st>>>(U, T, nd, so, od, nullptr, numGroups, nullptr, nullptr, nullptr);
    } else {
        const uint32_t grid = numGroups < LV_RESOLVE_SLAB_GRID ? numGroups : LV_RESOLVE_SLAB_GRID;
        if ((rc = lv_buf_reserve(ctx, ctx->ppllScratch, size_t(grid) * ldsBytes))) return rc;
        uint32_t* sc = (uint32_t*)ctx->ppllScratch.ptr;
        if (pq) k_ppll_resolve<false, true><<<grid, LV_WAVE, 0, st>>>(U, T, nd, so, od, sc, numGroups, nullptr, nullptr, nullptr);
        else k_ppll_resolve<false, false><<<grid, LV_WAVE, 0, st>>>(U, T, nd, so, od, sc, numGroups, nullptr, nullptr, nullptr);
    }
    return lv_resolve_read_back(ctx, out, size_t(w) * h);
}

// lv_mlab_resolve_buffers: the caller's runs (pixel p of the w x h rectangle owns entries [offsets[p], offsets[p + 1])) through the
// fold of mode 3 -- k_mlab_resolve with row-major addressing (one 1 x 1-pixel tiling, absolute run starts) and k_mlab_resolve_long
int lv_frame_mlab_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w,
                               uint32_t h, uint8_t* out) {
    const uint64_t numPixels = uint64_t(w) * h;
    const LvRunLimits lim = {"entries", 0xFFFFFFF0ull, 0x7FFFFFF0ull, 0xFFFFu};
    int rc;
    if ((rc = lv_runs_from_offsets(ctx, lim, offsets, numPixels, numEntries))) return rc;
    for (uint64_t i = 0; i < numEntries; i++)
        if (entries[3 * i + 2] == LV_MLAB_NO_KEY) return lv_fail(ctx, LV_E_INVALID, "entry %llu: key 0xFFFFFFFF is reserved", (unsigned long long)i);
    {   // keys unique within a pixel: the ordering ranks by key (a repeated key would leave a rank unwritten)
        std::vector<uint32_t> keys;
        for (uint64_t p = 0; p < numPixels; p++) {
            keys.clear();
            for (uint64_t i = offsets[p]; i < offsets[p + 1]; i++) keys.push_back(entries[3 * i + 2]);
            std::sort(keys.begin(), keys.end());
            if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
                return lv_fail(ctx, LV_E_INVALID, "pixel %llu: keys must be unique within a pixel", (unsigned long long)p);
        }
    }
    LvGivenLists G;
    if ((rc = lv_upload_runs(ctx, entries, numEntries, 12, w, h, G))) return rc;
    if ((rc = lv_upload_start_count(ctx, offsets, size_t(numPixels), G.runs))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->ppllScratch, size_t(numEntries ? numEntries : 1) * 8))) return rc;
    if ((rc = lv_mlab_fold(ctx, G.U, G.T, G.numGroups, nullptr, (uint32_t*)ctx->outDev.ptr, (uint2*)ctx->ppllScratch.ptr,
                           (LvDevCounters*)ctx->counters.ptr)))
        return rc;
    return lv_resolve_read_back(ctx, out, size_t(numPixels));
}

// lv_mboit_resolve_buffers: the caller's runs through the two sweeps of mode 6 (row-major addressing, absolute run starts, as
// lv_frame_mlab_resolve_only); entries = 5 words {r, g, b, a, view depth}, split into the colour and the depth array on upload
int lv_frame_mboit_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w,
                                uint32_t h, float logDepthMin, float logDepthMax, float* outMoments, uint8_t* out) {
    const uint64_t numPixels = uint64_t(w) * h;
    const uint32_t N = ctx->opt.mboitNumMoments;
    const LvRunLimits lim = {"entries", 0xFFFFFFF0ull / 5, 0x7FFFFFF0ull / (1 + N), 0xFFFEu};
    int rc;
    if ((rc = lv_runs_from_offsets(ctx, lim, offsets, numPixels, numEntries))) return rc;
    const size_t cap = size_t(numEntries ? numEntries : 1);
    std::vector<uint32_t> split(cap * 5);
    for (uint64_t i = 0; i < numEntries; i++) {
        if (entries[5 * i + 4] == LV_PPLL_DEAD) return lv_fail(ctx, LV_E_INVALID, "entry %llu: depth bits 0xFFFFFFFF are reserved", (unsigned long long)i);
        for (int k = 0; k < 4; k++) split[4 * i + k] = entries[5 * i + k];
        split[4 * cap + i] = entries[5 * i + 4];
    }
    LvGivenLists G;
    if ((rc = lv_upload_runs(ctx, split.data(), numEntries, 20, w, h, G))) return rc;
    if ((rc = lv_upload_start_count(ctx, offsets, size_t(numPixels), G.runs))) return rc;
    const size_t momBytes = size_t(numPixels) * (1 + N) * 4;
    if (outMoments && (rc = lv_buf_reserve(ctx, ctx->ppllScratch, momBytes))) return rc;
    const uint32_t noBox[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    LvMboitParams M = lv_mboit_params(ctx, G.U, noBox, ctx->opt.collectStats);
    M.logDepthMin = logDepthMin;
    M.logDepthMax = logDepthMax;
    if ((rc = lv_mboit_resolve(ctx, G.U, G.T, M, G.numGroups, uint32_t(cap), nullptr, (uint32_t*)ctx->outDev.ptr,
                               outMoments ? (float*)ctx->ppllScratch.ptr : nullptr, (LvDevCounters*)ctx->counters.ptr)))
        return rc;
    return lv_resolve_read_back(ctx, out, size_t(numPixels), {outMoments, ctx->ppllScratch.ptr, momBytes});
}

// lv_atomic_loop_resolve_buffers: the caller's keys (pixel p of the w x h rectangle owns keys [offsets[p], offsets[p + 1])) inserted
// by k_al64_insert_given, one lane per key with all lanes racing, then k_al64_resolve with row-major addressing
int lv_frame_al64_resolve_only(lv_ctx* ctx, const uint64_t* keys, uint64_t numKeys, const uint64_t* offsets, uint32_t w, uint32_t h,
                               uint8_t* out, uint64_t* outSlots, uint64_t* outTail) {
    const uint64_t numPixels = uint64_t(w) * h;
    const uint32_t K = ctx->opt.al64NumLayers;
    const LvRunLimits lim = {"keys", 0xFFFFFFF0ull, 0x7FFFFFF0ull / (K + LV_AL64_TAIL), LV_AL64_MAX_COUNT};
    int rc;
    if ((rc = lv_runs_from_offsets(ctx, lim, offsets, numPixels, numKeys))) return rc;
    for (uint64_t i = 0; i < numKeys; i++)
        if (keys[i] == LV_AL64_EMPTY) return lv_fail(ctx, LV_E_INVALID, "key %llu: 0xFFFFFFFFFFFFFFFF is the empty slot", (unsigned long long)i);
    hipStream_t st = ctx->stream;
    LvGivenLists G;
    if ((rc = lv_upload_runs(ctx, keys, numKeys, 8, w, h, G))) return rc;
    if ((rc = lv_upload_offsets(ctx, offsets, size_t(numPixels)))) return rc;
    const size_t numWords = size_t(numPixels) * (K + LV_AL64_TAIL);
    if ((rc = lv_buf_reserve(ctx, ctx->al64Buf, numWords * 8))) return rc;
    lv_al64_clear(ctx, numWords, K);
    if (numKeys)
        k_al64_insert_given<<<uint32_t((numKeys + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(
                (const unsigned long long*)ctx->ppllNodes.ptr, numKeys, (const unsigned long long*)ctx->ppllScratch.ptr, uint32_t(numPixels),
                (unsigned long long*)ctx->al64Buf.ptr, (uint32_t*)ctx->ppllCount.ptr, K);
    k_al64_resolve<<<G.numGroups, LV_WAVE, 0, st>>>(G.U, G.T, (const unsigned long long*)ctx->al64Buf.ptr, (const uint32_t*)ctx->ppllCount.ptr,
                                                    (uint32_t*)ctx->outDev.ptr, G.numGroups, K, (LvDevCounters*)ctx->counters.ptr);
    unsigned long long *dSlots = nullptr, *dTail = nullptr;
    if (outSlots || outTail) {
        if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, numWords * 8))) return rc;
        dSlots = (unsigned long long*)ctx->scratchRays.ptr;
        dTail = dSlots + size_t(numPixels) * K;
        k_al64_read<<<uint32_t((numPixels + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(
                (const unsigned long long*)ctx->al64Buf.ptr, w, h, w, 1u, 1u, K, dSlots, dTail);
    }
    return lv_resolve_read_back(ctx, out, size_t(numPixels), {outSlots, dSlots, size_t(numPixels) * K * 8},
                                {outTail, dTail, size_t(numPixels) * LV_AL64_TAIL * 8});
}

// lv_wboit_resolve_buffers: the caller's fragments (pixel p of the w x h rectangle owns entries [offsets[p], offsets[p + 1])) added
// by k_wboit_add_given, one lane per fragment with all lanes racing, then k_wboit_resolve with row-major addressing.  A pixel with
// more than LV_WBOIT_MAX_COUNT fragments is found where a frame finds it: by the resolve's overflow flag.
int lv_frame_wboit_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w, uint32_t h,
                                uint8_t* out, int64_t* outSums) {
    const uint64_t numPixels = uint64_t(w) * h;
    const LvRunLimits lim = {"entries", 0xFFFFFFF0ull / 5u, 0x7FFFFFF0ull / LV_WBOIT_SUMS, 0xFFFFFFFFu};
    int rc;
    if ((rc = lv_runs_from_offsets(ctx, lim, offsets, numPixels, numEntries))) return rc;
    hipStream_t st = ctx->stream;
    LvGivenLists G;
    if ((rc = lv_upload_runs(ctx, entries, numEntries, 20, w, h, G))) return rc;
    if ((rc = lv_upload_offsets(ctx, offsets, size_t(numPixels)))) return rc;
    const size_t sumBytes = size_t(numPixels) * LV_WBOIT_SUMS * 8;
    if ((rc = lv_buf_reserve(ctx, ctx->wboitBuf, sumBytes))) return rc;
    LV_HIP(ctx, hipMemsetAsync(ctx->wboitBuf.ptr, 0, sumBytes, st));
    if (numEntries)
        k_wboit_add_given<<<uint32_t((numEntries + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(
                (const float*)ctx->ppllNodes.ptr, numEntries, (const unsigned long long*)ctx->ppllScratch.ptr, uint32_t(numPixels),
                (unsigned long long*)ctx->wboitBuf.ptr, (uint32_t*)ctx->ppllCount.ptr,
                ctx->opt.wboitOpenglWeight ? LV_WBOIT_WEIGHT_OPENGL : LV_WBOIT_WEIGHT_REFERENCE);
    k_wboit_resolve<<<G.numGroups, LV_WAVE, 0, st>>>(G.U, G.T, (const unsigned long long*)ctx->wboitBuf.ptr, (const uint32_t*)ctx->ppllCount.ptr,
                                                     (uint32_t*)ctx->outDev.ptr, G.numGroups, (LvDevCounters*)ctx->counters.ptr);
    // (row-major addressing: the sums lie as the caller's array does)
    if ((rc = lv_resolve_read_back(ctx, out, size_t(numPixels), {outSums, ctx->wboitBuf.ptr, sumBytes}))) return rc;
    uint32_t flag = 0u;
    LV_HIP(ctx, hipMemcpy(&flag, &((const LvDevCounters*)ctx->counters.ptr)->mboitOverflow, 4, hipMemcpyDeviceToHost));
    if (flag)
        return lv_fail(ctx, LV_E_CAPACITY, "WBOIT: a pixel holds more than %u fragments (the 64-bit sums are exact up to that count)",
                       LV_WBOIT_MAX_COUNT);
    return LV_OK;
}

// lv_depth_peeling_resolve_buffers: the caller's fragments (pixel p of the w x h rectangle owns entries [offsets[p], offsets[p + 1]))
// peeled by min(longest run, depth_peeling_max_layers) times k_peel_given + k_peel_layer_given, then k_peel_blit, row-major addressing
int lv_frame_peel_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w, uint32_t h,
                               uint8_t* out, float* outAccum, uint32_t* outLayers) {
    const uint64_t numPixels = uint64_t(w) * h;
    const LvRunLimits lim = {"entries", 0xFFFFFFF0ull / 6u, 0x7FFFFFF0ull / 8u, 0xFFFFFFFFu};
    uint64_t longest = 0;
    int rc;
    if ((rc = lv_runs_from_offsets(ctx, lim, offsets, numPixels, numEntries, &longest))) return rc;
    hipStream_t st = ctx->stream;
    LvGivenLists G;
    if ((rc = lv_upload_runs(ctx, entries, numEntries, 24, w, h, G))) return rc;
    if ((rc = lv_upload_offsets(ctx, offsets, size_t(numPixels)))) return rc;
    const size_t n = size_t(numPixels);
    if ((rc = lv_buf_reserve(ctx, ctx->peelBuf, n * LV_PEEL_BYTES_PER_PIXEL))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->dcStatsDev, sizeof(LvDcStats)))) return rc;
    const LvPeelBuffers B = lv_peel_buffers(ctx, n);
    k_peel_clear<<<uint32_t((n + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(B, n, (LvDcStats*)ctx->dcStatsDev.ptr);
    const uint32_t passes = uint32_t(std::min<uint64_t>(longest, ctx->opt.peelMaxLayers));
    for (uint32_t i = 0; i < passes; i++) {
        k_peel_given<<<uint32_t((numEntries + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(
                (const uint32_t*)ctx->ppllNodes.ptr, numEntries, (const unsigned long long*)ctx->ppllScratch.ptr, uint32_t(numPixels), B,
                i == 0u ? 1u : 0u);
        k_peel_layer_given<<<uint32_t((n + LV_BLOCK - 1) / LV_BLOCK), LV_BLOCK, 0, st>>>(
                (const uint32_t*)ctx->ppllNodes.ptr, (const unsigned long long*)ctx->ppllScratch.ptr, uint32_t(numPixels), B);
    }
    k_peel_blit<<<G.numGroups, LV_WAVE, 0, st>>>(G.U, G.T, B.accum, (uint32_t*)ctx->outDev.ptr, G.numGroups);
    // (row-major addressing: the words lie as the caller's arrays do)
    return lv_resolve_read_back(ctx, out, n, {outAccum, B.accum, n * 16}, {outLayers, B.layers, n * 4});
}

// lv_deferred_shade_buffers: the caller's visibility buffer (row-major, w x h = the viewport size of the shading) packed into words by
// k_vis_pack, then k_deferred_shade with row-major addressing over the one tile at the origin.  The checks come first -- state, sizes,
// index range, the images the shading would read --, behind lv_ensure_tube_mesh only (the index check needs the mesh's triangle count; a
// tessellation touches no buffer of a frame); after them the call takes over visBuf, scratchRays, tilesDev and outDev, and no *_get_*
// call finds a frame.
int lv_frame_deferred_shade_only(lv_ctx* ctx, const uint32_t* primitive, const float* depth, uint32_t w, uint32_t h, uint32_t* out) {
    static const uint32_t txy[2] = {0u, 0u};
    const uint64_t numPixels = uint64_t(w) * h;
    int rc;
    if (numPixels > 0x7FFFFFF0ull / 8u) return lv_fail(ctx, LV_E_CAPACITY, "too many pixels");
    if (!ctx->cameraSet) return lv_fail(ctx, LV_E_STATE, "lv_set_camera has not been called");
    if (!ctx->tf.ptr || ctx->tfN == 0) return lv_fail(ctx, LV_E_STATE, "lv_set_transfer_function has not been called");
    if ((rc = lv_ensure_tube_mesh(ctx))) return rc;
    if (!ctx->triMeshSet || ctx->numTris == 0u)
        return lv_fail(ctx, LV_E_STATE, "lv_deferred_shade_buffers shades the tube triangle mesh: lv_set_tube_triangle_mesh or "
                                        "lv_set_trajectories has not been called");
    for (uint64_t p = 0; p < numPixels; p++)
        if (primitive[p] != LV_VIS_NO_PRIMITIVE && primitive[p] >= ctx->numTris)
            return lv_fail(ctx, LV_E_INVALID, "pixel %llu: primitive index %u, the mesh has %u triangles", (unsigned long long)p, primitive[p],
                           ctx->numTris);
    if ((rc = lv_deferred_check(ctx, "lv_deferred_shade_buffers"))) return rc;
    LvGivenLists G;
    lv_row_major_uniforms(ctx, G.U, w, h);
    if (G.U.useAmbientOcclusion && (!ctx->ao.ptr || ctx->aoW != w || ctx->aoH != h))
        return lv_fail(ctx, LV_E_INVALID, "the screen-space RTAO image is %u x %u, the visibility buffer %u x %u", ctx->aoW, ctx->aoH, w, h);
    if (G.U.useDepthCues && !ctx->depthMinMax.ptr) return lv_fail(ctx, LV_E_STATE, "depth cues need the depth range of a frame: render one first");
    hipStream_t st = ctx->stream;
    const size_t n = size_t(numPixels);
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, n * 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->visBuf, n * 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->tilesDev, 8))) return rc;
    if ((rc = lv_buf_reserve(ctx, ctx->outDev, n * 4))) return rc;
    ctx->streamed = {};   // (visBuf no longer belongs to a frame)
    uint32_t* dPrimitive = (uint32_t*)ctx->scratchRays.ptr;
    float* dDepth = (float*)(dPrimitive + n);
    LV_HIP(ctx, hipMemcpyAsync(dPrimitive, primitive, n * 4, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(dDepth, depth, n * 4, hipMemcpyHostToDevice, st));
    lv_vis_launch_pack(st, dPrimitive, dDepth, n, (unsigned long long*)ctx->visBuf.ptr);
    LvSceneDev SD;
    if ((rc = lv_deferred_scene(ctx, SD))) return rc;
    if ((rc = lv_single_tile(ctx, txy, w, h, G.T, G.numGroups))) return rc;
    lv_deferred_launch_shade(st, G.numGroups, lv_deferred_bands(G.U), G.U, SD, G.T, (const unsigned long long*)ctx->visBuf.ptr,
                             (uint32_t*)ctx->outDev.ptr);
    return lv_resolve_read_back(ctx, (uint8_t*)out, n);
}

int lv_frame_trace_rays_triangles(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n,
                                  float* outT, uint32_t* outTri, float* outUV) {
    int rc;
    if ((rc = lv_ensure_tube_mesh(ctx))) return rc;
    if (!ctx->triMeshSet) return lv_fail(ctx, LV_E_STATE, "lv_set_tube_triangle_mesh has not been called");
    if (!ctx->triAccelValid || ctx->triAccelLineWidth != ctx->opt.lineWidth)
        if ((rc = lv_bvh_build_triangles(ctx))) return rc;
    if (n == 0) return LV_OK;
    hipStream_t st = ctx->stream;
    const size_t rb = size_t(n) * 12;
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 2 * rb + size_t(n) * 16))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    float* dO = (float*)base;
    float* dD = (float*)(base + rb);
    float* dT = (float*)(base + 2 * rb);
    uint32_t* dS = (uint32_t*)(base + 2 * rb + size_t(n) * 4);
    float* dUV = (float*)(base + 2 * rb + size_t(n) * 8);
    LV_HIP(ctx, hipMemcpyAsync(dO, o, rb, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(dD, d, rb, hipMemcpyHostToDevice, st));
    LvSceneDev S = sceneDevTriangles(ctx);
    if ((rc = lv_reserve_overflow(ctx, S, "lv_trace_rays_triangles", nblocks(n), LV_STACK_LDS, true))) return rc;
    if (ctx->opt.traceRaysHardwareInv) k_trace_rays_tri<true><<<nblocks(n), LV_BLOCK, 0, st>>>(S, dO, dD, tMin, tMax, n, dT, dS, dUV);
    else k_trace_rays_tri<false><<<nblocks(n), LV_BLOCK, 0, st>>>(S, dO, dD, tMin, tMax, n, dT, dS, dUV);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(outT, dT, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(outTri, dS, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    if (outUV) LV_HIP(ctx, hipMemcpyAsync(outUV, dUV, size_t(n) * 8, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// lv_trace_rays_hull: the closest hull hit of arbitrary rays (H of lv_hull_rt.h), whatever hull_ray_tracing says
int lv_frame_trace_rays_hull(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n, float* outT, uint32_t* outTri,
                             float* outUV) {
    int rc;
    if (ctx->hullNumTris == 0u) return lv_fail(ctx, LV_E_STATE, "lv_trace_rays_hull: lv_set_hull_mesh has not been called");
    if (!ctx->hullAccelValid && (rc = lv_bvh_build_hull(ctx))) return rc;
    if (n == 0) return LV_OK;
    hipStream_t st = ctx->stream;
    const size_t rb = size_t(n) * 12;
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, 2 * rb + size_t(n) * 16))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    float* dO = (float*)base;
    float* dD = (float*)(base + rb);
    float* dT = (float*)(base + 2 * rb);
    uint32_t* dS = (uint32_t*)(base + 2 * rb + size_t(n) * 4);
    float* dUV = (float*)(base + 2 * rb + size_t(n) * 8);
    LV_HIP(ctx, hipMemcpyAsync(dO, o, rb, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(dD, d, rb, hipMemcpyHostToDevice, st));
    LvSceneDev S = sceneDev(ctx);
    if ((rc = lv_reserve_overflow(ctx, S, "lv_trace_rays_hull", nblocks(n), LV_STACK_LDS, LV_TREE_HULL))) return rc;
    LvHullRtDev R;
    R.nodes = (const float4*)ctx->hullNodes.ptr;
    R.tris = (const float4*)ctx->hullTris.ptr;
    R.pad = ctx->hullPad;
    R.mesh = lv_hull_dev(ctx);
    lv_hull_rt_trace_rays(st, S, R, dO, dD, tMin, tMax, n, dT, dS, dUV);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(outT, dT, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(outTri, dS, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    if (outUV) LV_HIP(ctx, hipMemcpyAsync(outUV, dUV, size_t(n) * 8, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// ---------------------------------------------------------------- lv_selftest_stack: the traversal stack on scripts
// One workgroup, every thread runs its own script on the stack type of the kernels (same members, same window and stride).
template <int NLDS>
__global__ __launch_bounds__(LV_BLOCK) void k_selftest_stack(unsigned* slab, const uint32_t* __restrict__ ops, uint32_t opsPerThread,
                                                             uint32_t* __restrict__ outWords, uint32_t* __restrict__ outCounts) {
    __shared__ unsigned s_stack[NLDS * LV_BLOCK];
    LvStackT<NLDS, LV_BLOCK, true> st;
    st.init(s_stack, slab);
    const uint32_t* my = ops + size_t(threadIdx.x) * opsPerThread * 4;
    uint32_t* out = outWords + size_t(threadIdx.x) * opsPerThread;
    uint32_t pops = 0;
    for (uint32_t i = 0; i < opsPerThread; i++) {
        const uint32_t op = my[4 * i];
        if ((op & 0xFFu) == LV_STACK_OP_PUSH3) st.push3(my[4 * i + 1], (op & 0x100u) != 0, my[4 * i + 2], (op & 0x200u) != 0, my[4 * i + 3], (op & 0x400u) != 0);
        else if ((op & 0xFFu) == LV_STACK_OP_POP) out[pops++] = lv_pop_or_done(st);
        else if ((op & 0xFFu) == LV_STACK_OP_CLEAR) st.clear();
    }
    outCounts[3 * threadIdx.x] = pops;
    outCounts[3 * threadIdx.x + 1] = st.spills;
    outCounts[3 * threadIdx.x + 2] = st.refills;
}

int lv_selftest_stack(lv_ctx* ctx, uint32_t instantiation, uint32_t wide_levels, const uint32_t* ops, uint32_t ops_per_thread,
                      uint32_t* out_words, uint32_t* out_counts, uint64_t* out_info) {
    if (!ctx) return LV_E_INVALID;
    if (instantiation > LV_STACK_INST_TILE) return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: unknown instantiation %u", instantiation);
    (void)hipSetDevice(ctx->device);
    const uint32_t slots = instantiation == LV_STACK_INST_AO ? LV_AO_STACK_LDS : LV_STACK_LDS;
    const uint64_t maxEntries = 3ull * wide_levels + 2, column = lv_overflow_entries(wide_levels, slots);
    if (out_info) {
        out_info[0] = slots - 1u;
        out_info[1] = LV_STACK_SPILL_BLOCK;
        out_info[2] = column;
        out_info[3] = ctx->stackOverflow.bytes;   // what the context's launches have reserved so far
        out_info[4] = ctx->wideDepth;
        out_info[5] = ctx->triWideDepth;
    }
    if (ops_per_thread == 0) return LV_OK;
    if (!ops || !out_words || !out_counts) return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: null array");
    if (wide_levels > 4096u || ops_per_thread > 65536u) return lv_fail(ctx, LV_E_CAPACITY, "lv_selftest_stack: script or depth too large");
    // A script is run only if it stays inside what the slab bound covers: never more than 3 * wide_levels + 2 entries, no spill without
    // a slab, no reference that reads as a marker or as "finished", nothing but clear after the pop that found the stack empty.
    for (uint32_t t = 0; t < LV_BLOCK; t++) {
        uint64_t depth = 0;
        bool finished = false;
        for (uint32_t i = 0; i < ops_per_thread; i++) {
            const uint32_t* op = ops + (size_t(t) * ops_per_thread + i) * 4;
            const uint32_t code = op[0] & 0xFFu;
            if (code == LV_STACK_OP_END) continue;
            if (code == LV_STACK_OP_CLEAR) { depth = 0; finished = false; continue; }
            if (finished) return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: thread %u op %u follows a pop of the empty stack without clear", t, i);
            if (code == LV_STACK_OP_POP) {
                if (depth == 0) finished = true; else depth--;
            } else if (code == LV_STACK_OP_PUSH3) {
                if (column == 0 && depth + 3 > slots - 1u)
                    return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: thread %u op %u would spill, but %u levels need no slab", t, i, wide_levels);
                for (int k = 0; k < 3; k++)
                    if (op[1 + k] == LV_INVALID || int32_t(op[1 + k]) >= int32_t(0x7C000000))
                        return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: thread %u op %u pushes a word that is no reference", t, i);
                depth += ((op[0] >> 8) & 1u) + ((op[0] >> 9) & 1u) + ((op[0] >> 10) & 1u);
                if (depth > maxEntries)
                    return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: thread %u op %u exceeds %llu entries", t, i, (unsigned long long)maxEntries);
            } else {
                return lv_fail(ctx, LV_E_INVALID, "lv_selftest_stack: thread %u op %u: unknown operation %u", t, i, code);
            }
        }
    }
    int rc;
    hipStream_t st = ctx->stream;
    const size_t opBytes = size_t(LV_BLOCK) * ops_per_thread * 16, wordBytes = size_t(LV_BLOCK) * ops_per_thread * 4, countBytes = size_t(LV_BLOCK) * 12;
    if ((rc = lv_buf_reserve(ctx, ctx->scratchRays, opBytes + wordBytes + countBytes))) return rc;
    const size_t slabBytes = size_t(LV_BLOCK) * column * 4;   // one workgroup: lv_overflow_bytes with gridBlocks = 1
    if (slabBytes && (rc = lv_buf_reserve(ctx, ctx->stackOverflow, slabBytes))) return rc;
    char* base = (char*)ctx->scratchRays.ptr;
    uint32_t* dOps = (uint32_t*)base;
    uint32_t* dWords = (uint32_t*)(base + opBytes);
    uint32_t* dCounts = (uint32_t*)(base + opBytes + wordBytes);
    unsigned* slab = slabBytes ? (unsigned*)ctx->stackOverflow.ptr : nullptr;
    LV_HIP(ctx, hipMemcpyAsync(dOps, ops, opBytes, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemsetAsync(dWords, 0, wordBytes + countBytes, st));
    if (instantiation == LV_STACK_INST_AO) k_selftest_stack<LV_AO_STACK_LDS><<<1, LV_BLOCK, 0, st>>>(slab, dOps, ops_per_thread, dWords, dCounts);
    else k_selftest_stack<LV_STACK_LDS><<<1, LV_BLOCK, 0, st>>>(slab, dOps, ops_per_thread, dWords, dCounts);
    LV_HIP(ctx, hipGetLastError());
    LV_HIP(ctx, hipMemcpyAsync(out_words, dWords, wordBytes, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(out_counts, dCounts, countBytes, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// VulkanAmbientOcclusionBaker::bakeAoTexture (VulkanAmbientOcclusionBaker.cpp:193-262): maxNumIterations passes of the
// baking shader, each averaging numAmbientOcclusionSamplesPerFrame rays per (parametrisation vertex, tube subdivision),
// accumulated as a running mean.  Rays hit the triangle tubes (the reference binds the triangle TLAS, cpp:480) and run
// through the same persistent work-queue kernel as the screen-space pass.
// async == false: on the context's stream with the frame's scratch buffers; the table is valid when the call returns (to the stream).
// async == true (lv_bake_ao_start; the reference's BakingMode::MULTI_THREADED, VulkanAmbientOcclusionBaker.cpp:266-346): on a second
// stream, into a second table, with scratch buffers and counters of its own -- frames keep rendering on the context's stream (without
// AO, or with the previous table's AO while that is still valid) until lv_bake_poll finds the stream finished and swaps the tables.
int lv_bake_ambient_occlusion(lv_ctx* ctx, bool async, bool inFrame) {
    const LvOptions& o = ctx->opt;
    {
        const int rcMesh = lv_ensure_tube_mesh(ctx);
        if (rcMesh) return rcMesh;
    }
    if (!ctx->triMeshSet) return lv_fail(ctx, LV_E_STATE, "the RTAO prebaker needs lv_set_tube_triangle_mesh");
    if (!ctx->bakeParamSet) return lv_fail(ctx, LV_E_STATE, "the RTAO prebaker needs lv_set_ao_parametrization");
    if (ctx->bakeNumLineVertices != ctx->numTriPoints)
        return lv_fail(ctx, LV_E_INVALID, "blending weights (%u) must match the mesh's line points (%u)",
                       ctx->bakeNumLineVertices, ctx->numTriPoints);
    int rc;
    if (!ctx->triAccelValid || ctx->triAccelLineWidth != o.lineWidth)
        if ((rc = lv_bvh_build_triangles(ctx))) return rc;
    if (async && !ctx->bakeStream) {
        LV_HIP(ctx, hipStreamCreateWithFlags(&ctx->bakeStream, hipStreamNonBlocking));
        LV_HIP(ctx, hipEventCreateWithFlags(&ctx->evBakePrereq, hipEventDisableTiming));
        LV_HIP(ctx, hipEventCreateWithFlags(&ctx->evBakeDone, hipEventDisableTiming));
    }
    hipStream_t st = async ? ctx->bakeStream : ctx->stream;
    const uint32_t N = o.bakeNumTubeSubdivisions, spp = o.bakeSamplesPerFrame, M = ctx->bakeNumParametrizationVertices;
    const uint64_t slots = uint64_t(M) * N;
    if (slots > 0x7FFFFFFFull) return lv_fail(ctx, LV_E_CAPACITY, "too many AO bake entries");
    LvDeviceBuffer& counters = async ? ctx->bakeCounters : ctx->counters;
    LvDeviceBuffer& gbuf = async ? ctx->bakeGbuf : ctx->aoGbuf;
    LvDeviceBuffer& samples = async ? ctx->bakeSamples : ctx->aoSamples;
    LvDeviceBuffer& table = async ? ctx->bakedAoPending : ctx->bakedAo;
    if (slots == 0) {
        if (async) { ctx->bakeAsyncPending = false; }
        ctx->bakeValid = true;
        return LV_OK;
    }
    if ((rc = lv_buf_reserve(ctx, counters, sizeof(LvDevCounters)))) return rc;
    if ((rc = lv_buf_reserve(ctx, table, size_t(slots) * 4))) return rc;
    if ((rc = lv_buf_reserve(ctx, gbuf, size_t(slots) * 48))) return rc;
    if ((rc = lv_buf_reserve(ctx, samples, size_t(slots) * spp * 4))) return rc;
    // LCG skip-ahead table: state after j steps = A_j * s + C_j (a = 1664525, c = 1013904223, RayTracingUtilities.glsl:169-175)
    std::vector<uint32_t>& skip = ctx->bakeSkipHost;   // (kept in the context: source of an asynchronous upload)
    if (ctx->bakeAsyncPending) LV_HIP(ctx, hipEventSynchronize(ctx->evBakeDone));   // the previous upload may still read it
    skip.assign(size_t(4) * N * spp, 0u);
    {
        uint32_t A = 1u, C = 0u;
        for (size_t j = 0; j < size_t(2) * N * spp; j++) {
            skip[2 * j] = A; skip[2 * j + 1] = C;
            A = 1664525u * A;
            C = 1664525u * C + 1013904223u;
        }
    }
    if ((rc = lv_buf_reserve(ctx, ctx->bakeLcgSkip, skip.size() * 4))) return rc;
    LvUniforms U;
    lv_fill_uniforms(ctx, U);
    U.aoSamplesPerFrame = spp;
    LvSceneDev SA = sceneDevTriangles(ctx);
    const uint64_t gridRays = lv_ao_grid(ctx, slots * spp);
    if (async) {
        // stack overflow slab of its own (the frames' slab is in use on the other stream)
        SA.stackOverflow = nullptr;
        const size_t bytes = lv_overflow_bytes(ctx, gridRays, LV_AO_STACK_LDS, true);
        if (bytes > LV_OVERFLOW_MAX_BYTES)
            return lv_fail(ctx, LV_E_CAPACITY, "RTAO prebaker: the traversal stacks would need %llu bytes; a launch addresses at most 4 GiB of them",
                           (unsigned long long)bytes);
        if (bytes) {
            if ((rc = lv_buf_reserve(ctx, ctx->bakeOverflow, bytes))) return rc;
            SA.stackOverflow = (unsigned*)ctx->bakeOverflow.ptr;
        }
        // everything queued on the context's stream so far (mesh upload, triangle LBVH) comes first
        LV_HIP(ctx, hipEventRecord(ctx->evBakePrereq, ctx->stream));
        LV_HIP(ctx, hipStreamWaitEvent(st, ctx->evBakePrereq, 0));
    } else if ((rc = inFrame ? lv_prepare_overflow(ctx, SA, "RTAO prebaker", gridRays, LV_AO_STACK_LDS, true)
                             : lv_reserve_overflow(ctx, SA, "RTAO prebaker", gridRays, LV_AO_STACK_LDS, true))) {
        return rc;
    }
    LV_HIP(ctx, hipMemcpyAsync(ctx->bakeLcgSkip.ptr, skip.data(), skip.size() * 4, hipMemcpyHostToDevice, st));
    LvDevCounters* dc = (LvDevCounters*)counters.ptr;
    float4* g = (float4*)gbuf.ptr;
    float* smp = (float*)samples.ptr;
    float* out = (float*)table.ptr;
    k_bake_setup<<<nblocks(slots), LV_BLOCK, 0, st>>>((const lv_line_point*)ctx->triPoints.ptr, ctx->numTriPoints,
                                                      (const float*)ctx->bakeSamplingLocations.ptr, M, N,
                                                      o.lineWidth * 0.5f, g, o.useRibbons ? 1u : 0u, o.bandWidth * 0.5f,
                                                      o.minBandThickness);
    ctx->bakeSlotsHost = uint32_t(slots);
    LV_HIP(ctx, hipMemcpyAsync(&dc->aoCount, &ctx->bakeSlotsHost, 4, hipMemcpyHostToDevice, st));
    for (uint32_t iter = 0; iter < o.bakeIterations; iter++) {
        U.aoFrameNumber = iter;
        LV_HIP(ctx, hipMemsetAsync(&dc->aoQueueHead, 0, 8, st));
        if (U.aoUseDistance)
            k_ao_rays<false, false, LV_PRIM_TRIANGLE, true><<<uint32_t(gridRays), LV_AO_BLOCK, 0, st>>>(
                    U, SA, g, smp, dc, nullptr, 0u, LvAoLayout{0u, 0u, 1u, 1u}, (const uint2*)ctx->bakeLcgSkip.ptr);
        else
            k_ao_rays<false, true, LV_PRIM_TRIANGLE, true><<<uint32_t(gridRays), LV_AO_BLOCK, 0, st>>>(
                    U, SA, g, smp, dc, nullptr, 0u, LvAoLayout{0u, 0u, 1u, 1u}, (const uint2*)ctx->bakeLcgSkip.ptr);
        k_ao_reduce<true><<<nblocks(slots), LV_BLOCK, 0, st>>>(U, g, smp, out, out, dc, nullptr, 0u, LvAoLayout{0u, 0u, 1u, 1u});
    }
    LV_HIP(ctx, hipGetLastError());
    if (async) {
        LV_HIP(ctx, hipEventRecord(ctx->evBakeDone, st));
        ctx->bakeAsyncPending = true;
        ctx->bakePendingGeneration = ctx->bakeGeneration;
    } else {
        ctx->bakeValid = true;
    }
    return LV_OK;
}

// Adopts the table of a finished asynchronous bake (wait == true: blocks until it has finished).  A table whose inputs changed while
// it was being computed (lv_invalidate_bake) is dropped.
int lv_bake_poll(lv_ctx* ctx, bool wait) {
    if (!ctx->bakeAsyncPending) return LV_OK;
    if (wait) {
        LV_HIP(ctx, hipEventSynchronize(ctx->evBakeDone));
    } else {
        const hipError_t e = hipEventQuery(ctx->evBakeDone);
        if (e == hipErrorNotReady) return LV_OK;
        if (e != hipSuccess) return lv_fail(ctx, LV_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
    }
    ctx->bakeAsyncPending = false;
    if (ctx->bakePendingGeneration == ctx->bakeGeneration) {
        // the context's stream may still shade a frame with the old table: order the swap behind it
        LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::swap(ctx->bakedAo, ctx->bakedAoPending);
        ctx->bakeValid = true;
    }
    return LV_OK;
}
