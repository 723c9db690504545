// The simulation-mesh hull (LineRenderer::renderHull, LineRenderer.cpp:732; HullRasterPass.cpp; MeshHull.glsl) in rendering modes 5, 8
// and 10 under the numerics contract of DESIGN.md 4 (float32, one operation at a time, left to right, no contraction): every rule of
// the hull fragment, stated once.  tests/test_hull_restatement.py states the same on the CPU, bit for bit.
//
// The hull is the translucent boundary surface of the domain the lines were traced in: an indexed triangle mesh of 32-byte
// HullTriangleVertexData records {position, pad, normal, pad} (LineRenderData.hpp:186-191), drawn between a mode's line pass and its
// resolve with culling off (HullRasterPass.cpp:108, CULL_NONE).
//
// Coverage and depth are mode 1's rules (lv_deferred.h) on this mesh: the coverage direction of lv_prism_cov_dir and its basis, unfused
// edge functions, the facing from det = A0 . cross(A1 - A0, A2 - A0) (the triangle's own; det == 0 covers nothing), the ascending-index
// fill rule with a back face running through its edges the other way round, (e0 + e1) + e2 > 0, no near-plane clipping, a
// conservative rectangle that is the whole viewport when a vertex has clip w <= 0, z = lv_vis_window_depth of the perspective-correct
// position (b0 V0 + b1 V1) + b2 V2, kept iff 0 <= z < 1.  lv_hull_setup is lv_vis_setup's sibling for the hull's vertex layout;
// lv_vis_cover, lv_vis_rows and lv_vis_window_depth are mode 1's own.
//
// Shading (MeshHull.glsl:77-90): the normal is (b0 N0 + b1 N1) + b2 N2, NOT normalised by the raster shader; with hull_use_shading
// the colour is blinnPhongShading(hullColor, normal) as Lighting.glsl:45-92 reads under MESH_HULL -- no depth cue, no AO,
// n = normalize(normal), l = v = normalize(camera - position), h = normalize(v + l), kA, kD, kS, s of the branch the frame's USE_BANDS
// selects --, else hullColor; alpha = hullOpacity * (1 - |dot(normal, v)|) with the un-normalised normal.
//
// The gather is the mode's own, as for a line fragment: mode 10 discards alpha < 0.001 (AtomicLoop64Gather.glsl:56-59) and inserts
// (bits(z) << 32) | packUnorm4x8(colour); mode 8 discards nothing and adds lv_wboit_add's terms under lv_wboit_weight(alpha, z); mode 5
// counts.  Every store adds 1 to the pixel's count and to the frame's fragment counter.
// Modes 2 and 3 store it in their fragment pool behind hull_fragment_pool = on (lv_hull_pool.h: the RECORD store of k_hull_pass and a
// fragment stage of its own), mode 11 ray-traces it behind hull_ray_tracing = on (lv_hull_rt.h); by default both refuse a frame while a
// hull would be drawn.  Not built: the hull in mode 1; modes 6 and 9 draw none in the reference.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_peel.h"
#include "lv_deferred.h"
#include "lv_al64.h"
#include "lv_wboit.h"

#define LV_HULL_STORE_COUNT 0   // mode 5: the per-pixel count
#define LV_HULL_STORE_WBOIT 1   // mode 8: lv_wboit_add
#define LV_HULL_STORE_AL64 2    // mode 10: lv_al64_insert
#define LV_HULL_STORE_LIST 3    // lv_hull_get_fragments: the fragment appended to a list
// (4: LV_HULL_STORE_RECORD of lv_hull_pool.h, modes 2 and 3)
#ifndef LV_HULL_SMALL
#define LV_HULL_SMALL 64u       // as LV_VIS_SMALL: a lane walks a pixel rectangle of at most this many pixels itself
#endif
#ifndef LV_HULL_WAVES_PER_CU
#define LV_HULL_WAVES_PER_CU 16u   // the launch splits the viewport into row bands until it has about this many waves per CU
#endif

// the mesh and the three options as the kernel reads them
struct LvHullDev {
    const uint32_t* idx;            // 3 per triangle
    const lv_hull_vertex* verts;    // HullTriangleVertexData
    uint32_t numTris;
    float color[3], opacity;        // hullColor = {hull_color, hull_opacity} (LineData.cpp:1310)
    uint32_t useShading;
};
// the list of LV_HULL_STORE_LIST: entry i of a fragment whose slot i = atomicAdd(counter, 1) is below capacity
struct LvHullList {
    unsigned long long* counter;
    uint32_t* pixel;                // y * width + x
    uint32_t* triangle;
    float* depth;
    float4* rgba;                   // straight colour
    unsigned long long capacity;
};

// lv_vis_setup for the hull's vertex layout, culling off; N: the vertex normals as given.  false: the triangle covers nothing
__device__ __forceinline__ bool lv_hull_setup(const LvUniforms& U, const LvHullDev& H, uint32_t tri, LvVisTri& T, f3 N[3]) {
    const uint32_t id[3] = {H.idx[3 * size_t(tri)], H.idx[3 * size_t(tri) + 1], H.idx[3 * size_t(tri) + 2]};
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    bool allBehind = true, anyBehindCamera = false;
    float sxMin = __builtin_inff(), sxMax = -__builtin_inff(), syMin = __builtin_inff(), syMax = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float* p = H.verts[id[i]].vertexPosition;
        const float* n = H.verts[id[i]].vertexNormal;
        T.V[i] = mk3(p[0], p[1], p[2]);
        N[i] = mk3(n[0], n[1], n[2]);
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
    T.own[0] = T.flip ? id[2] < id[1] : id[1] < id[2];
    T.own[1] = T.flip ? id[0] < id[2] : id[2] < id[0];
    T.own[2] = T.flip ? id[1] < id[0] : id[0] < id[1];
    const float W = float(U.width), Hh = float(U.height);
    if (anyBehindCamera) {
        T.x0 = 0; T.y0 = 0; T.x1 = int(U.width) - 1; T.y1 = int(U.height) - 1;
    } else {
        T.x0 = int(fminf(fmaxf(ceilf((sxMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), W));
        T.x1 = int(fminf(fmaxf(floorf((sxMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), W - 1.0f));
        T.y0 = int(fminf(fmaxf(ceilf((syMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), Hh));
        T.y1 = int(fminf(fmaxf(floorf((syMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), Hh - 1.0f));
    }
    return T.x0 <= T.x1 && T.y0 <= T.y1;
}

// MeshHull.glsl:77-90 on the interpolated position and the interpolated, un-normalised normal: the fragment's straight colour
__device__ __forceinline__ f4 lv_hull_shade(const LvUniforms& U, const LvHullDev& H, f3 pos, f3 nrm) {
    const f3 v = norm3s(mk3(U.camPos[0], U.camPos[1], U.camPos[2]) - pos);
    f4 c;
    c.x = H.color[0]; c.y = H.color[1]; c.z = H.color[2];
    if (H.useShading) {   // blinnPhongShading, Lighting.glsl:45-92 under MESH_HULL
        const float kA = 0.1f, kD = U.useBands ? 0.9f : 1.0f, kS = 0.3f, s = U.useBands ? 30.0f : 50.0f;
        const f3 n = norm3s(nrm);
        const f3 l = v;
        const f3 h = norm3s(v + l);
        const float diffuse = kD * clampf(fabsf(dot3(n, l)), 0.0f, 1.0f);
        const float Is = (kS * lv_pow_det(clampf(fabsf(dot3(n, h)), 0.0f, 1.0f), s)) * 1.0f;
        c.x = (kA * H.color[0] + diffuse * H.color[0]) + Is;
        c.y = (kA * H.color[1] + diffuse * H.color[1]) + Is;
        c.z = (kA * H.color[2] + diffuse * H.color[2]) + Is;
    }
    float cosAngle = dot3(nrm, v);
    if (cosAngle < 0.0f) cosAngle = cosAngle * -1.0f;
    c.w = H.opacity * (1.0f - cosAngle);
    return c;
}

// the covered fragment from its edge functions: the depth rule (false: not kept), then -- SHADE -- the colour
template <bool SHADE>
__device__ __forceinline__ bool lv_hull_fragment(const LvUniforms& U, const LvHullDev& H, const LvVisRows& Z, const LvVisTri& T,
                                                 const f3 N[3], const float e[3], uint32_t& zbits, f4& color) {
    float b[3];
    lv_prism_weights(e, b);
    const f3 pos = lv_prism_mix3(b, T.V[0], T.V[1], T.V[2]);
    zbits = __float_as_uint(lv_vis_window_depth(Z, pos));
    if (!lv_peel_candidate(zbits, 0u, true)) return false;   // 0 <= z < 1
    if (SHADE) color = lv_hull_shade(U, H, pos, lv_prism_mix3(b, N[0], N[1], N[2]));
    return true;
}

// lv_hull.hip: ONE launch of k_hull_pass<store>.  R: the coverage direction's constants (lv_fill_prism); requested: the requested-pixel
// mask (0 = requested, addressed like fragCount), or null = every pixel; fragCount, buf, arg: ppllCount and the mode's buffer and
// argument as k_stream_pass takes them (LIST: unused); L: the list (LIST only)
void lv_hull_launch(hipStream_t st, int store, uint32_t numCUs, const LvUniforms& U, const LvPrismDev& R, const LvHullDev& H,
                    const uint32_t* requested, uint32_t* fragCount, unsigned long long* buf, uint32_t arg, LvDevCounters* dc, bool stats,
                    const LvHullList& L);
