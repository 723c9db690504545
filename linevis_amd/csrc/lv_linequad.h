// lv_linequad.h -- the second line primitive: view-aligned line quads, the reference's "Quads (Programmable Pull)"
// (line_primitive_mode; LineData::LinePrimitiveMode begins with it), in rendering modes 5, 8 and 10 under the numerics contract of
// DESIGN.md 4 (float32, one operation at a time, left to right, fused multiply-adds exactly where lv_prism.h writes them).  Every rule of
// the quad fragment, stated once; tests/test_line_quads_restatement.py states the same on the CPU, bit for bit.
// (LvRasterQuad is something else: the 2 x 2 PIXEL quad of the helper lanes.)
//
//   vertex stage   Data/Shaders/Renderers/GeometryPass/LinePassQuads.glsl:73-113 (mMatrix = identity): line point i yields vertex 2 i
//                  with shiftSign -1 and vertex 2 i + 1 with shiftSign +1,
//                      tangent         = normalize(vertexTangent)
//                      viewDirection   = normalize(cameraPosition - linePoint)
//                      offsetDirection = normalize(cross(viewDirection, tangent))
//                      position        = linePoint + ((shiftSign * lineWidth) * 0.5) * offsetDirection
//                      normal0         = normalize(cross(tangent, offsetDirection)),  normal1 = offsetDirection
//                      fragmentNormalFloat = shiftSign,  fragmentTangent = vertexTangent (as stored),  fragmentAttribute
//                  with the shading code's normalize (norm3s).  A vertex is a pure function of (line point, side, camera): both segments
//                  at a point see the same bits.
//   line points    src/LineData/LineDataFlow.cpp:1047-1122 takes points, tangents and segment index pairs from
//                  createLineTubesRenderDataCPU, the call the prism's accessor makes on the same input (:1850): S.segs and S.prismFrames
//                  hold every input of a quad already -- position, attribute, tangent, point index.  No geometry buffer, no upload; a
//                  line-width change costs nothing.
//   index pattern  per segment (a, b): (2a, 2b, 2b + 1), (2a, 2b + 1, 2a + 1) (:1087-1097).  With v0 = 2a, v1 = 2a + 1, v2 = 2b,
//                  v3 = 2b + 1 the five distinct edge functions are E(v2, v3), E(v3, v0), E(v0, v2), E(v3, v1), E(v1, v0); the diagonal
//                  v0 v3 serves both triangles with opposite sign.
//   coverage       the prism's, unchanged (lv_prism.h): the vertices projected into the plane perpendicular to the pixel's coverage
//                  direction (lv_prism_cov_dir, lv_prism_basis, fused dot products of V - o), the unfused lv_prism_edge, an edge with
//                  e == 0 inside iff the triangle owns it (directed edge U -> V owned iff gl_VertexIndex(U) < gl_VertexIndex(V)), and
//                  (e0 + e1) + e2 > 0.
//   culling        LineRasterPass.cpp:86-90 culls back faces for every transparent renderer, and the pipeline is the prism's, so front
//                  is det[V0 - o, V1 - o, V2 - o] < 0 = "all e >= 0".  For this index pattern that is the side facing the camera:
//                  (B - A) x (C - A) is parallel to t x (v x t) = v - t (t . v) (t the tangent, v the view direction), whose component
//                  along v is 1 - (t . v)^2 >= 0.  A quad is front-facing by construction; only the flipped triangle of a bow-tie --
//                  the offset directions of its two points cross -- has all e < 0 and is dropped.  Nothing is tested for it.
//   weights        lv_prism_planes / lv_prism_interpolate: perspective-correct weights of the pixel's generator ray; position, attribute,
//                  tangent, normal0 through them, normal1 and fragmentNormalFloat (x) with the same weights by lv_prism_mix3's order.
//   kept iff       lv_prism_accept's three rules on the interpolated position: the ray interval, the own-box rule (every quad vertex lies
//                  within r of its line point, as a ring vertex does), depth clipping.
//   depth          what stage C of the mode's prism pass stores: the window depth (modes 8 and 10), nothing (mode 5).
//   degenerate     a point whose tangent is parallel to its view direction has cross(viewDirection, tangent) = 0.  GLSL's normalize
//                  makes NaN vertices of that; the shading code's normalize clamps the squared length at 2^-60, so here the offset
//                  direction is the zero vector and both vertices of the point coincide: E(v, v) = 0 and a triangle with two equal
//                  vertices has (e0 + e1) + e2 = 0 exactly, it covers nothing; a segment between one such point and an ordinary one
//                  tapers to it.  Non-finite line data gives NaN vertices: NaN edge values fail every comparison, the rectangle of
//                  a NaN projection is empty.  No special case for either.
//   fragment stage LinePassQuads.glsl:392-445.  Build-owned where GLSL leaves asin / sin / cos to the driver (asin is NaN one ulp
//                  outside [-1, 1]; sin(asin x) = x, cos(asin x) = sqrt(1 - x^2)):
//                      xc             = clamp(x, -1, 1)
//                      fragmentNormal = sqrt(fma(-xc, xc, 1)) * normalize(normal0) + xc * normalize(normal1)
//                  fragmentColor = blinnPhongShadingTube(transferFunction(attribute), fragmentNormal, fragmentTangent): the lighting of
//                  lv_compute_fragment_color_t<LV_SHADE_PLAIN> with the screen-space AO texel of the pixel and the depth cues, reached
//                  by calling that function with the halo switched off -- its outline then blends with weight 0 and coverage 1, what
//                  comes back is the lit colour and the transfer function's alpha.  (The screen-space position is the view matrix
//                  applied to the interpolated world position, as for every other fragment of this build.)  Then
//                      absCoords     = |x|                                        (un-clamped, as the shader)
//                      fragmentDepth = length(fragmentPositionWorld - cameraPosition)
//                      EPSILON       = clamp(((fragmentDepth / lineWidth) * 2) / viewportSize.y * fieldOfViewY, 0, 0.49)
//                      EPSILON_WHITE = fwidth(absCoords) = |fx - f0| + |fy - f0|: the same triangle's planes at the rays rq.dX, rq.dY of
//                                      the 2 x 2 partners (LvRasterQuad), as lv_shade_prism does for its halo coordinate
//                      rgb           = mix(fragmentColor.rgb, foregroundColor.rgb, smoothstep(0.7 - EPSILON_WHITE, 0.7 + EPSILON_WHITE, absCoords))
//                      alpha         = fragmentColor.a * (1 - smoothstep(1 - EPSILON, 1, absCoords))
//                  shading_numerics = fast: quads are shaded by the exact path.
//   gather         the mode's own, as for a prism fragment: mode 10 discards alpha < 0.001 and inserts (bits(z) << 32) |
//                  packUnorm4x8(colour); mode 8 discards nothing and adds lv_wboit_add's terms; mode 5 counts every kept fragment.
// Not built: quads in modes 2, 3, 6 and 9; the geometry-shader variant (the same picture); ribbon quads; band and helicity data on
// quads; the prebaked AO table on quads (its lookup needs phi = asin(x)); stress-line defines; VISUALIZE_SEEDING_PROCESS.
#pragma once
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_peel.h"
#include "lv_deferred.h"
#include "lv_al64.h"
#include "lv_wboit.h"

#define LV_LINEQUAD_STORE_COUNT 0   // mode 5: the per-pixel count
#define LV_LINEQUAD_STORE_WBOIT 1   // mode 8: lv_wboit_add
#define LV_LINEQUAD_STORE_AL64 2    // mode 10: lv_al64_insert
#define LV_LINEQUAD_STORE_LIST 3    // lv_line_quads_get_fragments: the fragment appended to a list
#ifndef LV_LINEQUAD_SMALL
#define LV_LINEQUAD_SMALL 64u       // as LV_HULL_SMALL: a lane walks a pixel rectangle of at most this many pixels itself
#endif

// the list of LV_LINEQUAD_STORE_LIST: entry i of a fragment whose slot i = atomicAdd(counter, 1) is below capacity
struct LvLineQuadList {
    unsigned long long* counter;
    uint32_t* pixel;                // y * width + x
    uint32_t* segment;              // index of the segment in the caller's order (S.leafSeg)
    uint32_t* triangle;             // 0: (2a, 2b, 2b + 1), 1: (2a, 2b + 1, 2a + 1)
    float* depth;                   // window depth
    float4* rgba;                   // straight colour
    unsigned long long capacity;
};

// one segment's quad: vertex v = 2 * point + side (point 0 = a, 1 = b; side 0: shiftSign -1, 1: +1)
struct LvLineQuad {
    f3 V[4];                        // world positions
    f3 normal0[2], normal1[2], tangent[2], centre[2];   // per point
    float attr[2];
    uint32_t id[4];                 // gl_VertexIndex
    int x0, y0, x1, y1;             // the pixel rectangle, inclusive, inside the viewport
};

// the vertex stage for one line point: positions of both sides, normal0, normal1
__device__ __forceinline__ void lv_linequad_point(f3 cam, f3 linePoint, f3 vertexTangent, float lineWidth, f3& posMinus, f3& posPlus,
                                                  f3& normal0, f3& normal1) {
    const f3 tangent = norm3s(vertexTangent);
    const f3 viewDirection = norm3s(cam - linePoint);
    const f3 offsetDirection = norm3s(cross3(viewDirection, tangent));
    posMinus = linePoint + ((-1.0f * lineWidth) * 0.5f) * offsetDirection;
    posPlus = linePoint + ((1.0f * lineWidth) * 0.5f) * offsetDirection;
    normal0 = norm3s(cross3(tangent, offsetDirection));
    normal1 = offsetDirection;
}

// The quad of the leaf's segment and its conservative pixel rectangle (lv_hull_setup's: projected vertices +- LV_VIS_BBOX_MARGIN, the
// whole viewport when a vertex has clip w <= 0).  false: it covers nothing (every vertex behind the camera or in front of the near
// plane, or an empty rectangle -- NaN vertices give one)
__device__ __forceinline__ bool lv_linequad_setup(const LvUniforms& U, const LvSceneDev& S, uint32_t leaf, LvLineQuad& Q) {
    const float4 pa = S.segs[2 * size_t(leaf)], pb = S.segs[2 * size_t(leaf) + 1];
    uint32_t pi[2];
    LvPrismPoint pt[2];
    lv_prism_frames(S, leaf, pa, pb, pt, pi);
    const f3 cam = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
#pragma unroll
    for (int p = 0; p < 2; p++) {
        Q.centre[p] = pt[p].centre; Q.tangent[p] = pt[p].tangent; Q.attr[p] = pt[p].attr;
        lv_linequad_point(cam, pt[p].centre, pt[p].tangent, U.lineWidth, Q.V[2 * p], Q.V[2 * p + 1], Q.normal0[p], Q.normal1[p]);
        Q.id[2 * p] = 2u * pi[p]; Q.id[2 * p + 1] = 2u * pi[p] + 1u;
    }
    bool allBehind = true, anyBehindCamera = false;
    float sxMin = __builtin_inff(), sxMax = -__builtin_inff(), syMin = __builtin_inff(), syMax = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f4 v = mulM4(U.view, Q.V[i].x, Q.V[i].y, Q.V[i].z, 1.0f);
        const f4 c = mulM4(U.proj, v.x, v.y, v.z, v.w);
        const bool behindCamera = !(c.w > 0.0f);
        anyBehindCamera = anyBehindCamera || behindCamera;
        allBehind = allBehind && (behindCamera || c.z < 0.0f);
        const float sx = ((c.x / c.w) * 0.5f + 0.5f) * float(U.width), sy = ((c.y / c.w) * 0.5f + 0.5f) * float(U.height);
        sxMin = fminf(sxMin, sx); sxMax = fmaxf(sxMax, sx);
        syMin = fminf(syMin, sy); syMax = fmaxf(syMax, sy);
    }
    if (allBehind) return false;
    const float W = float(U.width), H = float(U.height);
    if (anyBehindCamera) {
        Q.x0 = 0; Q.y0 = 0; Q.x1 = int(U.width) - 1; Q.y1 = int(U.height) - 1;
    } else {
        Q.x0 = int(fminf(fmaxf(ceilf((sxMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), W));
        Q.x1 = int(fminf(fmaxf(floorf((sxMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), W - 1.0f));
        Q.y0 = int(fminf(fmaxf(ceilf((syMin - LV_VIS_BBOX_MARGIN) - 0.5f), 0.0f), H));
        Q.y1 = int(fminf(fmaxf(floorf((syMax + LV_VIS_BBOX_MARGIN) - 0.5f), -1.0f), H - 1.0f));
    }
    return Q.x0 <= Q.x1 && Q.y0 <= Q.y1;
}

// Coverage of pixel (x, y) by the quad's two triangles: bit t of the result = triangle t covers the pixel (front face, fill rule)
__device__ __forceinline__ unsigned lv_linequad_coverage(const LvPrismDev& R, const LvLineQuad& Q, f3 o, uint32_t x, uint32_t y) {
    f3 P, Qb;
    lv_prism_basis(R, lv_prism_cov_dir(R, x, y), P, Qb);
    float X[4], Y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f3 A = Q.V[i] - o;
        X[i] = lv_prism_dot(A, P); Y[i] = lv_prism_dot(A, Qb);
    }
    const float e23 = lv_prism_edge(X[2], Y[2], X[3], Y[3]);   // E(v2, v3)
    const float e30 = lv_prism_edge(X[3], Y[3], X[0], Y[0]);   // E(v3, v0): the diagonal
    const float e02 = lv_prism_edge(X[0], Y[0], X[2], Y[2]);   // E(v0, v2)
    const float e31 = lv_prism_edge(X[3], Y[3], X[1], Y[1]);   // E(v3, v1)
    const float e10 = lv_prism_edge(X[1], Y[1], X[0], Y[0]);   // E(v1, v0)
    const float e03 = -e30;                                    // E(v0, v3)
    unsigned mask = 0u;
    // (v0, v2, v3): e0 = E(v2, v3), e1 = E(v3, v0), e2 = E(v0, v2)
    if (lv_prism_inside(e23, Q.id[2] < Q.id[3]) && lv_prism_inside(e30, Q.id[3] < Q.id[0]) && lv_prism_inside(e02, Q.id[0] < Q.id[2]) &&
        (e23 + e30) + e02 > 0.0f)
        mask |= 1u;
    // (v0, v3, v1): e0 = E(v3, v1), e1 = E(v1, v0), e2 = E(v0, v3)
    if (lv_prism_inside(e31, Q.id[3] < Q.id[1]) && lv_prism_inside(e10, Q.id[1] < Q.id[0]) && lv_prism_inside(e03, Q.id[0] < Q.id[3]) &&
        (e31 + e10) + e03 > 0.0f)
        mask |= 2u;
    return mask;
}

// the three vertices of triangle t as lv_prism_planes / lv_prism_interpolate take them, with the quad's own varyings beside them
struct LvLineQuadTri { LvPrismTri T; f3 normal0[3], normal1[3]; float x[3]; };
__device__ __forceinline__ LvLineQuadTri lv_linequad_triangle(const LvLineQuad& Q, uint32_t t) {
    const int v[3] = {0, t == 0u ? 2 : 3, t == 0u ? 3 : 1};
    LvLineQuadTri G;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int p = v[i] >> 1;
        G.T.pos[i] = Q.V[v[i]];
        G.T.tan[i] = Q.tangent[p];
        G.T.attr[i] = Q.attr[p];
        G.normal0[i] = Q.normal0[p];
        G.normal1[i] = Q.normal1[p];
        G.x[i] = (v[i] & 1) ? 1.0f : -1.0f;
    }
    return G;
}

// The fragment of triangle t at pixel (x, y): kept (lv_prism_accept) or not; its window depth; -- SHADE -- its straight colour
template <bool SHADE>
__device__ __forceinline__ bool lv_linequad_fragment(const LvUniforms& U, const LvSceneDev& S, const LvVisRows& Z, const LvLineQuad& Q,
                                                     uint32_t t, uint32_t x, uint32_t y, uint32_t& zbits, f4& color) {
    const LvPrismDev& R = S.prism;
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u);   // the ray interval of the prism passes
    f3 o, d;
    lv_primary_ray(U, x, y, 0.5f, 0.5f, o, d);
    const LvLineQuadTri G = lv_linequad_triangle(Q, t);
    const LvPrismPlanes pl = lv_prism_planes(R, G.T, o, d);
    const LvPrismInputs I = lv_prism_interpolate(G.T, G.normal0, pl, d);
    LvPrismPoint pt[2];
    pt[0].centre = Q.centre[0]; pt[1].centre = Q.centre[1];
    if (!lv_prism_accept(R, pt, R.radius, o, d, I.pos, len3(I.pos - o), tLo, tHi)) return false;
    zbits = __float_as_uint(lv_vis_window_depth(Z, I.pos));
    if (!SHADE) return true;
    const f3 n1 = lv_prism_mix3(I.b, G.normal1[0], G.normal1[1], G.normal1[2]);
    const float xf = (I.b[0] * G.x[0] + I.b[1] * G.x[1]) + I.b[2] * G.x[2];
    // fwidth(absCoords) from the helper lanes: the same planes at the quad partners' rays
    const LvRasterQuad rq = lv_make_raster_quad(U, x, y);
    const LvPrismInputs Ix = lv_prism_interpolate(G.T, G.normal0, pl, rq.dX), Iy = lv_prism_interpolate(G.T, G.normal0, pl, rq.dY);
    const float f0 = fabsf(xf);
    const float fx = fabsf((Ix.b[0] * G.x[0] + Ix.b[1] * G.x[1]) + Ix.b[2] * G.x[2]);
    const float fy = fabsf((Iy.b[0] * G.x[0] + Iy.b[1] * G.x[1]) + Iy.b[2] * G.x[2]);
    const float EPSILON_WHITE = fabsf(fx - f0) + fabsf(fy - f0);
    // the build-owned normal
    const float xc = clampf(xf, -1.0f, 1.0f);
    const float cs = sqrtf(__builtin_fmaf(-xc, xc, 1.0f));
    const f3 fragmentNormal = cs * norm3s(I.nrm) + xc * norm3s(n1);
    // blinnPhongShadingTube(transferFunction(attribute), fragmentNormal, fragmentTangent) with AO and depth cues: the halo off
    LvUniforms UL = U;
    UL.useHalos = 0u;
    LvBandArgs none;
    none.useBand = false; none.phi = 0.0f; none.linePosition = mk3(0.0f, 0.0f, 0.0f); none.lineNormal = mk3(0.0f, 0.0f, 0.0f);
    none.rotation = 0.0f; none.separatorScale = 1.0f; none.rasterEpsWhite = 0.0f;
    const float aoTexel = (U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(y) * U.width + x] : 1.0f;
    float fragmentDepth;
    const f4 lit = lv_compute_fragment_color_t<LV_SHADE_PLAIN, 0>(S, UL, aoTexel, I.pos, fragmentNormal, I.tan, false, I.attr, fragmentDepth,
                                                                  none);
    const float EPSILON = clampf(((fragmentDepth / U.lineWidth) * 2.0f) / float(U.height) * U.fovY, 0.0f, 0.49f);
    const float w = smoothstepf(0.7f - EPSILON_WHITE, 0.7f + EPSILON_WHITE, f0);
    color.x = mixf(lit.x, U.foreground[0], w);
    color.y = mixf(lit.y, U.foreground[1], w);
    color.z = mixf(lit.z, U.foreground[2], w);
    color.w = lit.w * (1.0f - smoothstepf(1.0f - EPSILON, 1.0f, f0));
    return true;
}

// lv_linequad.hip: ONE launch of k_linequad_pass<store> over the leaves (leafList: the segments k_ppll_cull_segments kept, their
// number in dc->prismListCount; null: every segment).  requested: the requested-pixel mask (0 = requested, addressed like fragCount),
// or null = every pixel; fragCount, buf, arg: ppllCount and the mode's buffer and argument as k_stream_pass takes them (LIST:
// unused); L: the list (LIST only)
void lv_linequad_launch(hipStream_t st, int store, const LvUniforms& U, const LvSceneDev& S, const uint32_t* leafList,
                        const uint32_t* requested, uint32_t* fragCount, unsigned long long* buf, uint32_t arg, LvDevCounters* dc, bool stats,
                        const LvLineQuadList& L);
