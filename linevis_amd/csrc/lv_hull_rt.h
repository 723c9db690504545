// The simulation-mesh hull in the ray tracer (rendering mode 11, hull_ray_tracing = on): the semantics, stated once.
// tests/test_hull_rt_restatement.py states the same in float32 numpy, bit for bit.
//
// The reference puts a hull triangle BLAS into every TLAS the ray tracer uses (getRayTracingTube*AndHullTopLevelAS, LineData.cpp:949-1162)
// and shades its hits in ClosestHitHull (TubeRayTracing.glsl:359-431) inside the transparency loop of the lines (traceRayTransparent,
// :61-82).  Here, under the numerics contract of DESIGN.md 4 (float32, one operation at a time, no contraction), one step of that loop
// with the ray (o, d), tMin and tMax = 1000 is:
//
//   L   the closest line hit, exactly as k_render_rt finds it (lv_trace_closest on the frame's line primitive).
//   H   the closest hull hit: the least t over the triangles lv_ray_triangle accepts with pad = hullPad, no culling, t inside the closed
//       interval [tMin, tMax] as lv_trace_rays_triangles has it; ties go to the lowest triangle index.
//       hullPad = maxAbs * 1e-5f + 1e-6f with maxAbs the largest absolute vertex coordinate of the mesh: it depends on the mesh alone,
//       never on the line width, so the hull LBVH (lv_bvh_build_hull) is rebuilt by lv_set_hull_mesh and by nothing else.
//   the hull wins iff H is found and (L is not found or tH < tL); a tie goes to the line.  The hull walk therefore runs on [tMin, tL].
//   a hull hit is shaded as ClosestHitHull (lv_hull_rt_hit): (t, u, v) of lv_ray_triangle on the triangle's own vertices,
//       b = ((1 - u) - v, u, v), position and normal (b0 a0 + b1 a1) + b2 a2 (interpolateVec3's order), the normal then normalised --
//       unlike the raster shader of lv_hull.h --, colour = blinnPhongShading without depth cue and AO (lv_hull_shade) or the plain
//       hull_color, alpha = hull_opacity * (1 - |n . v|) with the normalised normal, payload.hitT = length(position - cameraPosition).
//   tMin update, blend, termination and miss are k_render_rt's.
//
// k_render_rt_hull (lv_hull_rt.hip) is k_render_rt with that step; with rt_record_hits it appends one record per step that hit
// (LV_RT_HIT_WORDS words, lv_rt_get_hits).  k_trace_rays_hull is H alone for arbitrary rays (lv_trace_rays_hull).
// Not built: the hull under use_mlat (AnyHitHull) and in modes 1, 2 and 3.
#pragma once
#include "lv_hull.h"

#define LV_RT_HIT_WORDS 9u      // {pixel, sampleIdx << 16 | hitIdx, primitive, t, payload.hitT, r, g, b, a}
#define LV_RT_HIT_HULL 0x80000000u

// the hull as the ray tracer reads it: its LBVH (48-B records, one triangle per leaf) and the mesh with the three options
struct LvHullRtDev {
    const float4* nodes;
    const float4* tris;
    float pad;                  // hullPad
    LvHullDev mesh;             // numTris == 0: no hull is drawn (a recording frame without one)
};

// the scene view lv_trace_closest<.., LV_PRIM_TRIANGLE> walks the hull LBVH through; slab: the launch's traversal-stack slab
__device__ __forceinline__ LvSceneDev lv_hull_rt_view(const LvSceneDev& S, const LvHullRtDev& R) {
    LvSceneDev V = S;
    V.nodes = R.nodes;
    V.numSegs = R.mesh.numTris;
    V.tris = R.tris;
    V.triPad = R.pad;
    V.triLeafSize = 1u;
    V.triPairs = 0u;
    return V;
}

// (t, u, v) of hull triangle `tri` on the ray: the operands and operations of the leaf test, so the same bits
__device__ __forceinline__ bool lv_hull_rt_tuv(const LvHullRtDev& R, uint32_t tri, f3 o, f3 d, float& t, float& u, float& v) {
    const uint32_t* ti = R.mesh.idx + 3 * size_t(tri);
    const float* a = R.mesh.verts[ti[0]].vertexPosition;
    const float* b = R.mesh.verts[ti[1]].vertexPosition;
    const float* c = R.mesh.verts[ti[2]].vertexPosition;
    return lv_ray_triangle(o, d, mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]),
                           R.pad, t, u, v);
}

// ClosestHitHull, TubeRayTracing.glsl:397-431: the straight colour of the hit and payload.hitT
__device__ __forceinline__ f4 lv_hull_rt_hit(const LvUniforms& U, const LvHullRtDev& R, uint32_t tri, f3 o, f3 d, float& payloadHitT) {
    float t = 0.0f, u = 0.0f, v = 0.0f;
    lv_hull_rt_tuv(R, tri, o, d, t, u, v);
    const float b[3] = {(1.0f - u) - v, u, v};
    const uint32_t* ti = R.mesh.idx + 3 * size_t(tri);
    f3 P[3], N[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float* p = R.mesh.verts[ti[i]].vertexPosition;
        const float* n = R.mesh.verts[ti[i]].vertexNormal;
        P[i] = mk3(p[0], p[1], p[2]);
        N[i] = mk3(n[0], n[1], n[2]);
    }
    const f3 pos = lv_prism_mix3(b, P[0], P[1], P[2]);
    const f3 nrm = lv_prism_mix3(b, N[0], N[1], N[2]);
    const f3 cam = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    f4 c = lv_hull_shade(U, R.mesh, pos, nrm);
    // the alpha takes the NORMALISED normal here (fragmentNormal = normalize(fragmentNormal), :409)
    float cosAngle = dot3(norm3s(nrm), norm3s(cam - pos));
    if (cosAngle < 0.0f) cosAngle = cosAngle * -1.0f;
    c.w = R.mesh.opacity * (1.0f - cosAngle);
    payloadHitT = len3(pos - cam);
    return c;
}

// lv_hull_rt.hip
struct lv_ctx;
// ONE launch of k_render_rt_hull for the frame's line primitive and shading variant; rec: the record array of rt_record_hits or null
int lv_hull_rt_render(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvHullRtDev& R, const LvTiles& T, uint32_t gridTiles,
                      uint32_t* out, LvDevCounters* dc, bool triangles, uint32_t* rec, uint32_t recCap);
// k_trace_rays_hull over n rays; S: any scene view whose stackOverflow is the launch's slab
void lv_hull_rt_trace_rays(hipStream_t st, const LvSceneDev& S, const LvHullRtDev& R, const float* org, const float* dir, float tMin, float tMax,
                           uint32_t n, float* outT, uint32_t* outTri, float* outUV);
