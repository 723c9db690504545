// Deferred shading on a visibility buffer (rendering mode 1: DeferredRenderer with deferredRenderingMode = "Draw Indexed" and
// drawIndexedGeometryMode = "Precomputed Triangles", DeferredRenderer.hpp:297-300) under the numerics contract of DESIGN.md 4
// (float32, one operation at a time, left to right, no contraction): every rule of the mode, stated once.
// tests/test_deferred_restatement.py states the same on the CPU, bit for bit.
//
// The visibility buffer.  The reference draws the tube triangle mesh once into a primitive-index attachment (clear 0xFFFFFFFF) and
// a depth attachment (clear 1.0, LESS; VisibilityBufferDrawIndexed.glsl, VisibilityBufferDrawIndexedPass.cpp:70-92).  Here both are
// ONE 64-bit word per pixel, (bits(z) << 32) | primitive index, and a fragment is ONE atomicMin on it (lv_peel_key): the smallest z,
// the first primitive in index-buffer order among equal depths.  The bit patterns order as the floats do because a kept fragment
// has 0 <= z < 1 (lv_peel_candidate with first = true: a z with the sign bit set, a z >= 1 and a NaN are refused -- the depth clip
// of the pipeline).  The empty word is (bits(1.0) << 32) | 0xFFFFFFFF: both clear values at once.
//
// Coverage is the build's own (the driver's rule is implementation-defined), stated as lv_prism.h states the prism's:
//   viewing ray     the pixel-centre coverage direction D of lv_prism_cov_dir, its basis P = cross(R, D), Q = cross(D, P)
//   vertex          A = V - cameraPosition; (x, y) = (A . P, A . Q), unfused dot products: a pure function of (vertex, pixel), so both
//                   triangles at an edge see the same bits
//   edge function   lv_prism_edge, UNFUSED: E(V, U) == -E(U, V) bit for bit
//   facing          det = A0 . cross(A1 - A0, A2 - A0), once per triangle: det < 0 is FRONT -- the sense in which the tessellator's
//                   outward triangles (host/Tubes.cpp, lv_lines.hip) are front, and the one in which e0, e1, e2 > 0 inside.  det == 0
//                   (edge-on, degenerate) covers nothing.  Back faces are culled iff use_capped_tubes
//                   (VisibilityBufferDrawIndexedPass.cpp:77-81); drawn back faces are covered where -e0, -e1, -e2 > 0
//   coverage        e0 = E(V1, V2), e1 = E(V2, V0), e2 = E(V0, V1) all > 0, an edge with e == 0 counting as inside iff the triangle
//                   runs through it with ASCENDING vertex index (the neighbour runs through it the other way: exactly one of the two
//                   owns it; a drawn back face runs through its edges the other way round), and (e0 + e1) + e2 > 0
//   near plane      no clipping: the facing is the triangle's, so a ray meets it in front of the camera or not at all, and the
//                   depth rule drops what lies in front of the near plane
//   z               lv_window_depth's arithmetic (lv_vis_window_depth) of the perspective-correct position (b0 V0 + b1 V1) + b2 V2,
//                   b_i = e_i * (1 / ((e0 + e1) + e2))
// The pixel rectangle of a triangle (projected vertices +- LV_VIS_BBOX_MARGIN, the whole viewport when a vertex has clip w <= 0)
// only has to be conservative; a triangle whose three vertices all have clip w <= 0 or clip z < 0 is dropped before it.
//
// Shading runs once per pixel (DeferredShading.glsl:90-134): position from the depth, barycentrics from area ratios,
// LineAttributesBarycentric.glsl, computeFragmentColor with fragmentColor.a = 1 (RayHitCommon.glsl:130-132).
// Not built: the prebaked AO table in the shading pass; "Programmable Pulling" geometry, the
// Draw Indirect, BVH and mesh-shader modes, HZB culling, meshlets, supersampling and upscalers, motion vectors, the hull pass,
// stress-line data, per-rank triangle culling of sharded frames.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_peel.h"

#define LV_VIS_NO_PRIMITIVE 0xFFFFFFFFu                                  // DeferredShading.glsl:73: the primitive index's clear value
#define LV_VIS_EMPTY ((0x3F800000ull << 32) | 0xFFFFFFFFull)              // depth clear 1.0, primitive clear
#define LV_VIS_BBOX_MARGIN 0.015625f   // 1/64 pixel, as LV_PRISM_BBOX_MARGIN
// Measured knobs (tools/probe_deferred.py, profiles/deferred_c2.json): the 1M-segment tornado scene (12.06 M triangles),
// config 2's settings, mode-1 frame, median of 5 frames per process, three processes each, interleaved, at 1920 x 1080 / 3840 x 2160:
// LV_VIS_SMALL 4: 0.939 ... 0.953 / 4.126 ... 4.136 ms; 16: 0.466 ... 0.486 / 1.519 ... 1.535 ms; 64: 0.473 ... 0.479 / 1.014 ... 1.039 ms;
// 256: 0.479 ... 0.483 / 1.034 ... 1.047 ms -> 64 (at 3840 x 2160 a third less than 16, far outside the spread; nothing more beyond it).
// LV_VIS_PRELOAD (with 64): 0.486 ... 0.491 / 1.064 ... 1.073 ms: slower at both resolutions -> off.
#ifndef LV_VIS_SMALL
#define LV_VIS_SMALL 64u        // a lane walks a pixel rectangle of at most this many pixels itself; larger ones are covered by the wave
#endif
#ifndef LV_VIS_PRELOAD
#define LV_VIS_PRELOAD 0        // 1: a relaxed load of the word first; the atomic is skipped when the key is not below it
#endif

// rows z and w of proj * view, as lv_window_depth (lv_render.hip) builds them
struct LvVisRows { float mz[4], mw[4]; };
__device__ __forceinline__ LvVisRows lv_vis_rows(const LvUniforms& U) {
    LvVisRows Z;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        Z.mz[c] = 0.0f; Z.mw[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {   // column-major 4 x 4
            Z.mz[c] += U.proj[4 * k + 2] * U.view[4 * c + k];
            Z.mw[c] += U.proj[4 * k + 3] * U.view[4 * c + k];
        }
    }
    return Z;
}
// window depth gl_FragCoord.z = clip.z / clip.w of a world position: the arithmetic of lv_window_depth
__device__ __forceinline__ float lv_vis_window_depth(const LvVisRows& Z, f3 p) {
    const float cz = ((Z.mz[0] * p.x + Z.mz[1] * p.y) + Z.mz[2] * p.z) + Z.mz[3];
    const float cw = ((Z.mw[0] * p.x + Z.mw[1] * p.y) + Z.mw[2] * p.z) + Z.mw[3];
    return cz / cw;
}

// one triangle as the rasteriser sees it
struct LvVisTri {
    f3 V[3], A[3];        // world positions; relative to the camera
    bool own[3];          // edge i (opposite vertex i) counts as inside at e_i == 0
    bool flip;            // a drawn back face: the edge functions change sign
    int x0, y0, x1, y1;   // the pixel rectangle, inclusive, inside the viewport
};
// false: the triangle covers nothing (header: facing, the early rejections, an empty rectangle)
__device__ __forceinline__ bool lv_vis_setup(const LvUniforms& U, const LvSceneDev& S, uint32_t tri, bool cull, LvVisTri& T) {
    const uint32_t id[3] = {S.triIdx[3 * size_t(tri)], S.triIdx[3 * size_t(tri) + 1], S.triIdx[3 * size_t(tri) + 2]};
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    bool allBehind = true, anyBehindCamera = false;
    float sxMin = __builtin_inff(), sxMax = -__builtin_inff(), syMin = __builtin_inff(), syMax = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float* p = S.triVerts[id[i]].vertexPosition;
        T.V[i] = mk3(p[0], p[1], p[2]);
        T.A[i] = T.V[i] - o;
        const f4 v = mulM4(U.view, p[0], p[1], p[2], 1.0f);
        const f4 c = mulM4(U.proj, v.x, v.y, v.z, v.w);
        const bool behindCamera = !(c.w > 0.0f);
        anyBehindCamera = anyBehindCamera || behindCamera;
        allBehind = allBehind && (behindCamera || c.z < 0.0f);
        const float sx = ((c.x / c.w) * 0.5f + 0.5f) * float(U.width), sy = ((c.y / c.w) * 0.5f + 0.5f) * float(U.height);
        sxMin = fminf(sxMin, sx); sxMax = fmaxf(sxMax, sx);
        syMin = fminf(syMin, sy); syMax = fmaxf(syMax, sy);
    }
    if (allBehind) return false;
    const float det = dot3(T.A[0], cross3(T.A[1] - T.A[0], T.A[2] - T.A[0]));
    if (det == 0.0f) return false;
    T.flip = det > 0.0f;
    if (T.flip && cull) return false;
    T.own[0] = T.flip ? id[2] < id[1] : id[1] < id[2];
    T.own[1] = T.flip ? id[0] < id[2] : id[2] < id[0];
    T.own[2] = T.flip ? id[1] < id[0] : id[0] < id[1];
    const float W = float(U.width), H = float(U.height);
    if (anyBehindCamera) {
        T.x0 = 0; T.y0 = 0; T.x1 = int(U.width) - 1; T.y1 = int(U.height) - 1;
    } else {
        // pixel centres x + 0.5 inside [min - margin, max + margin]; clamped while still float (infinities of a tiny clip w)
        T.x0 = int(fminf(fmaxf(ceilf((sxMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), W));
        T.x1 = int(fminf(fmaxf(floorf((sxMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), W - 1.0f));
        T.y0 = int(fminf(fmaxf(ceilf((syMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), H));
        T.y1 = int(fminf(fmaxf(floorf((syMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), H - 1.0f));
    }
    return T.x0 <= T.x1 && T.y0 <= T.y1;
}
// does the triangle cover pixel (x, y)?  e: the edge functions as the weights take them (a drawn back face's negated)
__device__ __forceinline__ bool lv_vis_cover(const LvPrismDev& R, const LvVisTri& T, uint32_t x, uint32_t y, float e[3]) {
    const f3 D = lv_prism_cov_dir(R, x, y);
    f3 P, Q;
    lv_prism_basis(R, D, P, Q);
    float X[3], Y[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { X[i] = dot3(T.A[i], P); Y[i] = dot3(T.A[i], Q); }
    e[0] = lv_prism_edge(X[1], Y[1], X[2], Y[2]);
    e[1] = lv_prism_edge(X[2], Y[2], X[0], Y[0]);
    e[2] = lv_prism_edge(X[0], Y[0], X[1], Y[1]);
    if (T.flip) { e[0] = -e[0]; e[1] = -e[1]; e[2] = -e[2]; }
    return lv_prism_inside(e[0], T.own[0]) && lv_prism_inside(e[1], T.own[1]) && lv_prism_inside(e[2], T.own[2]) &&
           (e[0] + e[1]) + e[2] > 0.0f;
}
// the covered fragment's depth bits
__device__ __forceinline__ uint32_t lv_vis_depth_bits(const LvVisRows& Z, const LvVisTri& T, const float e[3]) {
    float b[3];
    lv_prism_weights(e, b);
    return __float_as_uint(lv_vis_window_depth(Z, lv_prism_mix3(b, T.V[0], T.V[1], T.V[2])));
}
// the fragment's store
__device__ __forceinline__ void lv_vis_offer(unsigned long long* word, unsigned long long key) {
#if LV_VIS_PRELOAD
    // words only decrease within a frame: a stale value can only skip less
    if (key >= __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
#endif
    atomicMin(word, key);
}

// DeferredShading.glsl:103-124: the fragment's position from the pixel centre and the depth, the barycentrics from area ratios
struct LvDeferredFrag { f3 pos; float u, v, w; };
__device__ __forceinline__ LvDeferredFrag lv_deferred_fragment(const LvUniforms& U, const LvSceneDev& S, uint32_t x, uint32_t y,
                                                               float fragmentDepth, uint32_t tri) {
    const float fx = float(x) + 0.5f, fy = float(y) + 0.5f;   // gl_FragCoord.xy
    const float nx = 2.0f * fx / float(U.width) - 1.0f, ny = 2.0f * fy / float(U.height) - 1.0f;
    const f4 fragPosView = mulM4(U.invProj, nx, ny, fragmentDepth, 1.0f);
    const f4 fragPosWorld = mulM4(U.invView, fragPosView.x, fragPosView.y, fragPosView.z, fragPosView.w);
    LvDeferredFrag F;
    F.pos = mk3(fragPosWorld.x / fragPosWorld.w, fragPosWorld.y / fragPosWorld.w, fragPosWorld.z / fragPosWorld.w);
    const float* a = S.triVerts[S.triIdx[3 * size_t(tri)]].vertexPosition;
    const float* b = S.triVerts[S.triIdx[3 * size_t(tri) + 1]].vertexPosition;
    const float* c = S.triVerts[S.triIdx[3 * size_t(tri) + 2]].vertexPosition;
    const f3 p0 = mk3(a[0], a[1], a[2]), p1 = mk3(b[0], b[1], b[2]), p2 = mk3(c[0], c[1], c[2]);
    const f3 d20 = p2 - p0, d21 = p2 - p1;
    const float totalArea = len3(cross3(d20, d21));
    F.u = len3(cross3(d21, F.pos - p1)) / totalArea;
    F.v = len3(cross3(F.pos - p0, d20)) / totalArea;
    F.w = (1.0f - F.u) - F.v;
    return F;
}

// LineAttributesBarycentric.glsl with barycentricCoordinates = (w0, w1, w2) for the vertices 0, 1, 2 and the given position, then
// computeFragmentColor: lv_shade_hit_triangle's sibling for a caller that brings its own barycentrics and position (the deferred pass:
// (u, v, 1 - u - v) of DeferredShading.glsl:124), in the same three variants.  S.tf: the caller passes the transfer function with
// alpha 1 (fragmentColor.a = 1.0, RayHitCommon.glsl:130-132; the alpha of the transfer function reaches nothing but the result's
// alpha).  The depth cue takes (viewMatrix * position).xyz, as computeFragmentColor itself does (RayHitCommon.glsl:390: the function's
// own screenSpacePosition hides the one DeferredShading.glsl:110 computes).  The AO texel is the pixel's own: the prebaked AO table
// is not built for this pass (lv_frame_check refuses it for mode 1).
template <int BANDS = LV_SHADE_PLAIN>
__device__ __forceinline__ f4 lv_shade_triangle_barycentric(const LvSceneDev& S, const LvUniforms& U, float aoTexel, uint32_t tri, float w0,
                                                            float w1, float w2, f3 fragPos, float& payloadHitT) {
    const uint32_t i0 = S.triIdx[3 * size_t(tri)], i1 = S.triIdx[3 * size_t(tri) + 1], i2 = S.triIdx[3 * size_t(tri) + 2];
    const lv_tube_vertex& vd0 = S.triVerts[i0];
    const lv_tube_vertex& vd1 = S.triVerts[i1];
    const lv_tube_vertex& vd2 = S.triVerts[i2];
    const lv_line_point& lp0 = S.triPoints[vd0.vertexLinePointIndex & 0x7FFFFFFFu];
    const lv_line_point& lp1 = S.triPoints[vd1.vertexLinePointIndex & 0x7FFFFFFFu];
    const lv_line_point& lp2 = S.triPoints[vd2.vertexLinePointIndex & 0x7FFFFFFFu];
    auto lerp3 = [&](const float* a, const float* b, const float* c) {
        return (mk3(a[0], a[1], a[2]) * w0 + mk3(b[0], b[1], b[2]) * w1) + mk3(c[0], c[1], c[2]) * w2;
    };
    const bool isCap = U.useCappedTubes &&
            (((vd0.vertexLinePointIndex | vd1.vertexLinePointIndex | vd2.vertexLinePointIndex) >> 31) != 0u);
    const f3 fragmentNormal = norm3(lerp3(vd0.vertexNormal, vd1.vertexNormal, vd2.vertexNormal));
    const f3 fragmentTangent = norm3(lerp3(lp0.lineTangent, lp1.lineTangent, lp2.lineTangent));
    const float fragmentAttribute = (lp0.lineAttribute * w0 + lp1.lineAttribute * w1) + lp2.lineAttribute * w2;
    if (BANDS == LV_SHADE_PLAIN)
        return lv_compute_fragment_color(S, U, aoTexel, fragPos, fragmentNormal, fragmentTangent, isCap, fragmentAttribute, payloadHitT);
    // interpolateAngle, BarycentricInterpolation.glsl:43-55
    const float PI = 3.14159265358979323846f;
    float a0 = vd0.phi, a1 = vd1.phi, a2 = vd2.phi;
    if (a1 - a0 > PI || a2 - a0 > PI) a0 += 2.0f * PI;
    if (a0 - a1 > PI || a2 - a1 > PI) a1 += 2.0f * PI;
    if (a0 - a2 > PI || a1 - a2 > PI) a2 += 2.0f * PI;
    LvBandArgs b;
    b.phi = (a0 * w0 + a1 * w1) + a2 * w2;
    b.rotation = 0.0f; b.separatorScale = 1.0f; b.rasterEpsWhite = -1.0f;
    if (BANDS == LV_SHADE_BANDS) {   // USE_BANDS, LineAttributesBarycentric.glsl:53-58; useBand = true (RayHitCommon.glsl:164-172)
        b.useBand = true;
        b.linePosition = lerp3(lp0.linePosition, lp1.linePosition, lp2.linePosition);
        b.lineNormal = lerp3(lp0.lineNormal, lp1.lineNormal, lp2.lineNormal);
        return lv_compute_fragment_color_t<LV_SHADE_BANDS>(S, U, aoTexel, fragPos, fragmentNormal, fragmentTangent, isCap, fragmentAttribute,
                                                           payloadHitT, b);
    }
    // USE_ROTATING_HELICITY_BANDS, LineAttributesBarycentric.glsl:60-111
    b.useBand = false;
    b.linePosition = mk3(0.0f, 0.0f, 0.0f);
    b.lineNormal = mk3(0.0f, 0.0f, 0.0f);
    const float f = U.helicityRotationFactor;
    b.rotation = ((lp0.lineRotation * f) * w0 + (lp1.lineRotation * f) * w1) + (lp2.lineRotation * f) * w2;
    const uint32_t li0 = vd0.vertexLinePointIndex & 0x7FFFFFFFu;
    const f3 c0 = mk3(lp0.linePosition[0], lp0.linePosition[1], lp0.linePosition[2]);
    // the neighbour of the first vertex's line point on its line: the previous point, or the next one at a line's start
    const bool hasPrevious = li0 != 0u && S.triPoints[li0 - 1u].lineStartIndex == lp0.lineStartIndex;
    const lv_line_point& other = S.triPoints[hasPrevious ? li0 - 1u : li0 + 1u];
    const f3 co = mk3(other.linePosition[0], other.linePosition[1], other.linePosition[2]);
    if (isCap) {   // the rotation continued linearly along the line
        const float fragmentRotationDelta = (lp0.lineRotation - other.lineRotation) * f;
        f3 planeNormal = c0 - co;
        const float segmentLength = len3(planeNormal);
        planeNormal = mk3(planeNormal.x / segmentLength, planeNormal.y / segmentLength, planeNormal.z / segmentLength);
        const float planeDist = -dot3(planeNormal, c0);
        const float distToPlane = dot3(planeNormal, fragPos) + planeDist;
        b.rotation += fragmentRotationDelta * distToPlane / segmentLength;
    }
    if (U.uniformHelicityBandWidth) {   // UNIFORM_HELICITY_BAND_WIDTH, :94-111
        const float rotDy = hasPrevious ? (lp0.lineRotation - other.lineRotation) * f : (other.lineRotation - lp0.lineRotation) * f;
        const float rotDx = len3(c0 - co);
        float sn, cs;
        lv_sincos_rad(lv_atan2_det(rotDy * 0.5f * U.lineWidth, rotDx), sn, cs);
        b.separatorScale = cs;
    }
    return lv_compute_fragment_color_t<LV_SHADE_HELICITY>(S, U, aoTexel, fragPos, fragmentNormal, fragmentTangent, isCap,
                                                          fragmentAttribute, payloadHitT, b);
}

// lv_deferred.hip: the launches of a mode-1 frame.  S: the triangle scene view (triIdx, triVerts, triPoints)
// the words of n pixels set to LV_VIS_EMPTY
void lv_vis_launch_clear(hipStream_t st, unsigned long long* words, size_t n);
// k_vis_raster, one lane per triangle.  requested: the requested-pixel mask (0 = requested, addressed like the words), or null = every pixel
void lv_vis_launch_raster(hipStream_t st, const LvUniforms& U, const LvSceneDev& S, uint32_t numTris, bool cull, const uint32_t* requested,
                          unsigned long long* words);
// the requested viewport pixels with a winner added to dc->fragCounter
void lv_vis_launch_count(hipStream_t st, uint32_t grid, const LvUniforms& U, const uint32_t* requested, const unsigned long long* words,
                         LvDevCounters* dc);
// k_deferred_shade<bands> (LV_SHADE_*): the cells and groups of k_wboit_resolve over the tile list.  S.tf: the transfer function with alpha 1
void lv_deferred_launch_shade(hipStream_t st, uint32_t numGroups, int bands, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T,
                              const unsigned long long* words, uint32_t* out);
// tfOpaque[i] = {tf[i].rgb, 1}
void lv_deferred_launch_tf(hipStream_t st, const float4* tf, uint32_t n, float4* tfOpaque);
// the words of the w x h viewport, row-major, taken apart (lv_deferred_get_buffers) / put together (lv_deferred_shade_buffers)
void lv_vis_launch_read(hipStream_t st, const unsigned long long* words, uint32_t w, uint32_t h, uint32_t paddedW, uint32_t tileW,
                        uint32_t tileH, uint32_t* outPrimitive, float* outDepth);
void lv_vis_launch_pack(hipStream_t st, const uint32_t* primitive, const float* depth, size_t n, unsigned long long* words);
