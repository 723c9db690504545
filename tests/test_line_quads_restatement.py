"""The line-quad fragment (linevis_amd/csrc/lv_linequad.h; include/linevis_hip.h, line_primitive_mode = "Quads (Programmable Pull)")
restated in float32 numpy: one operation at a time, left to right, no contraction; a fused multiply-add exactly where the device
writes one (fmaf below rounds once).

quad_fragments() is the vectorised statement -- the vertex stage of every line point, the conservative rectangle of every segment,
the ray-space coverage of its two triangles with the prism's fill rule, the perspective-correct weights of lv_prism_planes /
lv_prism_interpolate, lv_prism_accept's three rules, the window depth, the build-owned normal, the tube lighting (the checker's
computeFragmentColor of tests/test_deferred_restatement.py with the halo off), the quad's own outline and coverage; quad_pair() is its
scalar transcription for one (segment, pixel).  frame_references() folds the fragments (with a hull's, if given) through wboit_fold,
al64_fold and depth_complexity_frame: the reference frames tests/test_gpu_line_quads.py compares the device with.

Here, without a GPU: the vectorised form against the scalar one; against an independent float64 screen-space rasteriser of the same
quads; a straight line seen side-on; the interpolated coordinate; a bow-tie; a line pointing at the camera; the clamp of the normal."""
import copy
import functools

import numpy as np

from common import Case, small_case
from linevis_amd import transfer_function as tfm
from oracle import lvo
from test_atomic_loop_restatement import al64_fold, al64_key
from test_deferred_restatement import (BBOX_MARGIN, F, View, clampf, compute_fragment_color, cross3, dot3, len3, mixf, mul_m4, norm_shade,
                                       pairs_of, smoothstepf)
from test_depth_peeling_restatement import depth_complexity_frame
from test_mlab_restatement import pack, window_depth
from test_wboit_restatement import wboit_fold

T_LO = F(0.0001)
T_HI = (np.array([1000.0], F).view(np.uint32) + np.uint32(1)).view(F)[0]     # the ray interval of the prism passes
# vertex v of a segment's quad: (point 0 = a | 1 = b, side 0 = shiftSign -1 | 1 = +1); triangle t: its three vertices
TRIANGLES = ((0, 2, 3), (0, 3, 1))


def fmaf(a, b, c):
    """fma(a, b, c) in float32, rounded once: the product of two float32 is exact in float64; the float64 sum is corrected to
    round-to-odd with the exact error of TwoSum, after which the rounding to float32 is the rounding of the exact value"""
    a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = np.atleast_1d(s).view(np.int64).copy()
        fix = np.atleast_1d((err != 0) & np.isfinite(s) & np.isfinite(err)) & ((bits & 1) == 0)
        up = np.atleast_1d((err > 0) == (s > 0))
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        out = bits.view(np.float64).astype(F)
    return out.reshape(np.shape(s)) if np.ndim(s) else out[0]


def prism_dot(a, b):
    """lv_prism_dot"""
    with np.errstate(all="ignore"):
        return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))


def sub3(a, b):
    return [a[k] - b[k] for k in range(3)]


def mix3(b, a0, a1, a2):
    """lv_prism_mix3"""
    return [(b[0] * a0[k] + b[1] * a1[k]) + b[2] * a2[k] for k in range(3)]


def columns(a):
    return [np.ascontiguousarray(a[:, k], dtype=F) for k in range(3)]


# ---------------------------------------------------------------- the vertex stage and the rectangle
def quad_points(points, V, line_width):
    """lv_linequad_point for every line point: dict of minus, plus (positions of the two sides), normal0, normal1, tangent (as stored),
    centre -- lists of three float32 arrays -- and attr"""
    with np.errstate(all="ignore"):
        lp, tan = columns(points["linePosition"]), columns(points["lineTangent"])
        cam = [V.cam[k] for k in range(3)]
        t = norm_shade(tan)
        view = norm_shade(sub3(cam, lp))
        od = norm_shade(cross3(view, t))
        hm, hp = (F(-1.0) * F(line_width)) * F(0.5), (F(1.0) * F(line_width)) * F(0.5)
        return dict(minus=[lp[k] + hm * od[k] for k in range(3)], plus=[lp[k] + hp * od[k] for k in range(3)],
                    normal0=norm_shade(cross3(t, od)), normal1=od, tangent=tan, centre=lp,
                    attr=np.ascontiguousarray(points["lineAttribute"], dtype=F))


def quad_vertex(Q, seg, v):
    """vertex v of the segments' quads (TRIANGLES' numbering): three float32 arrays"""
    idx = seg[:, v >> 1]
    return [Q["plus" if v & 1 else "minus"][k][idx] for k in range(3)]


def quad_setup(Q, seg, V):
    """lv_linequad_setup's rectangle per segment (x1 < x0: covers nothing)"""
    n = len(seg)
    W, H = F(V.w), F(V.h)
    all_behind, any_behind = np.ones(n, bool), np.zeros(n, bool)
    sx_min, sx_max = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    sy_min, sy_max = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    with np.errstate(all="ignore"):
        for v in range(4):
            p = quad_vertex(Q, seg, v)
            vv = mul_m4(V.view, p[0], p[1], p[2], F(1.0))
            c = mul_m4(V.proj, vv[0], vv[1], vv[2], vv[3])
            behind = ~(c[3] > 0)
            any_behind |= behind
            all_behind &= behind | (c[2] < 0)
            sx = ((c[0] / c[3]) * F(0.5) + F(0.5)) * W
            sy = ((c[1] / c[3]) * F(0.5) + F(0.5)) * H
            sx_min, sx_max = np.fmin(sx_min, sx), np.fmax(sx_max, sx)
            sy_min, sy_max = np.fmin(sy_min, sy), np.fmax(sy_max, sy)
        x0 = np.fmin(np.fmax(np.ceil((sx_min - BBOX_MARGIN) - F(0.5)), F(0.0)), W)
        x1 = np.fmin(np.fmax(np.floor((sx_max + BBOX_MARGIN) - F(0.5)), F(-1.0)), W - F(1.0))
        y0 = np.fmin(np.fmax(np.ceil((sy_min - BBOX_MARGIN) - F(0.5)), F(0.0)), H)
        y1 = np.fmin(np.fmax(np.floor((sy_max + BBOX_MARGIN) - F(0.5)), F(-1.0)), H - F(1.0))
    x0 = np.where(any_behind, 0, np.nan_to_num(x0)).astype(np.int64)
    y0 = np.where(any_behind, 0, np.nan_to_num(y0)).astype(np.int64)
    x1 = np.where(any_behind, V.w - 1, np.nan_to_num(x1)).astype(np.int64)
    y1 = np.where(any_behind, V.h - 1, np.nan_to_num(y1)).astype(np.int64)
    x1 = np.where(all_behind, x0 - 1, x1)
    return dict(x0=x0, y0=y0, x1=x1, y1=y1)


# ---------------------------------------------------------------- coverage
def inside(e, owned):
    """lv_prism_inside"""
    return (e > 0) | ((e == 0) & owned)


def quad_coverage(Q, seg, V, s, x, y):
    """lv_linequad_coverage for (segment, pixel) pairs: the covered flags of the two triangles and the five edge values"""
    with np.errstate(all="ignore"):
        D = [V.cov[y, x, k] for k in range(3)]
        P = cross3([V.right[k] for k in range(3)], D)
        Qb = cross3(D, P)
        X, Y = [], []
        for v in range(4):
            A = sub3([a[s] for a in quad_vertex(Q, seg, v)], [V.cam[k] for k in range(3)])
            X.append(prism_dot(A, P))
            Y.append(prism_dot(A, Qb))
        edge = lambda u, v: Y[u] * X[v] - X[u] * Y[v]
        e23, e30, e02, e31, e10 = edge(2, 3), edge(3, 0), edge(0, 2), edge(3, 1), edge(1, 0)
        e03 = -e30
        a, b = seg[s, 0].astype(np.int64), seg[s, 1].astype(np.int64)
        vid = [2 * a, 2 * a + 1, 2 * b, 2 * b + 1]
        t0 = inside(e23, vid[2] < vid[3]) & inside(e30, vid[3] < vid[0]) & inside(e02, vid[0] < vid[2]) & ((e23 + e30) + e02 > 0)
        t1 = inside(e31, vid[3] < vid[1]) & inside(e10, vid[1] < vid[0]) & inside(e03, vid[0] < vid[3]) & ((e31 + e10) + e03 > 0)
    return [t0, t1], dict(e23=e23, e30=e30, e02=e02, e31=e31, e10=e10)


# ---------------------------------------------------------------- the fragment
def raster_quad(V, x, y):
    """lv_make_raster_quad: the affine generator's rays of the pixel and of its 2 x 2 partners"""
    with np.errstate(all="ignore"):
        sxp, syp = F(2.0) / F(V.w), F(2.0) / F(V.h)
        ndcx = (x.astype(F) + F(0.5)) * sxp - F(1.0)
        ndcy = (y.astype(F) + F(0.5)) * syp - F(1.0)
        target = mul_m4(V.inv_proj, ndcx, ndcy, F(1.0), F(1.0))
        d = mul_m4(V.inv_view, target[0], target[1], target[2], F(0.0))
        gx = mul_m4(V.inv_proj, sxp, F(0.0), F(0.0), F(0.0))
        gy = mul_m4(V.inv_proj, F(0.0), syp, F(0.0), F(0.0))
        Gx = mul_m4(V.inv_view, gx[0], gx[1], gx[2], F(0.0))
        Gy = mul_m4(V.inv_view, gy[0], gy[1], gy[2], F(0.0))
        sx = np.where((x & 1) != 0, F(-1.0), F(1.0)).astype(F)
        sy = np.where((y & 1) != 0, F(-1.0), F(1.0)).astype(F)
        return [d[k] + sx * Gx[k] for k in range(3)], [d[k] + sy * Gy[k] for k in range(3)]


def own_box(o, d, p0, p1, radius, depth):
    """lv_prism_own_box"""
    with np.errstate(all="ignore"):
        lo, hi = [], []
        for k in range(3):
            inv = F(1.0) / d[k]
            t0 = ((np.fmin(p0[k], p1[k]) - radius) - o[k]) * inv
            t1 = ((np.fmax(p0[k], p1[k]) + radius) - o[k]) * inv
            lo.append(np.fmin(t0, t1))
            hi.append(np.fmax(t0, t1))
        tn = np.fmax(np.fmax(lo[0], lo[1]), lo[2])
        tf = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
        slack = radius / len3(d)
        return (tn <= tf) & (depth >= tn - slack) & (depth <= tf + slack)


@functools.lru_cache(maxsize=None)
def _case_params(case):
    sc = case.oracle_scene()
    return case.oracle_params(sc)


def shading_params(case, depth_range=None):
    """the checker's params of the case with the halo off (lv_linequad_fragment's call of computeFragmentColor)"""
    P = copy.copy(_case_params(case))
    P.useHalos = 0
    if depth_range is not None:
        P.minDepth, P.maxDepth = float(depth_range[0]), float(depth_range[1])
    return P


def quad_fragment(case, Q, seg, V, P, s, x, y, t, ao=None):
    """lv_linequad_fragment for (segment s, pixel, triangle t) rows: dict of kept, zbits, rgba (n, 4), pos, x (the interpolated
    fragmentNormalFloat), eps_white"""
    n = len(s)
    cam = [V.cam[k] for k in range(3)]
    vsel = np.asarray(TRIANGLES, np.int64)[t]                   # (n, 3) vertex numbers
    pt = vsel >> 1
    pidx = np.take_along_axis(seg[s].astype(np.int64), pt, 1)   # (n, 3) line points
    side = (vsel & 1).astype(bool)
    with np.errstate(all="ignore"):
        pos3 = [[np.where(side[:, i], Q["plus"][k][pidx[:, i]], Q["minus"][k][pidx[:, i]]) for k in range(3)] for i in range(3)]
        var3 = lambda name: [[Q[name][k][pidx[:, i]] for k in range(3)] for i in range(3)]
        n03, n13, tan3 = var3("normal0"), var3("normal1"), var3("tangent")
        attr3 = [Q["attr"][pidx[:, i]] for i in range(3)]
        x3 = [np.where(side[:, i], F(1.0), F(-1.0)).astype(F) for i in range(3)]
        # lv_prism_planes in the basis of the generator's normalised ray
        d = [V.ray[y, x, k] for k in range(3)]
        Pb = cross3([V.right[k] for k in range(3)], d)
        Qb = cross3(d, Pb)
        vv = []
        for i in range(3):
            A = sub3(pos3[i], cam)
            vv.append([prism_dot(A, Pb), prism_dot(A, Qb), prism_dot(A, d)])
        c = [cross3(vv[1], vv[2]), cross3(vv[2], vv[0]), cross3(vv[0], vv[1])]

        def weights(Dr):
            abg = [prism_dot(Dr, Pb), prism_dot(Dr, Qb), prism_dot(Dr, d)]
            e = [prism_dot(abg, c[i]) for i in range(3)]
            rs = F(1.0) / ((e[0] + e[1]) + e[2])
            return [a * rs for a in e]

        scalar = lambda b, a: (b[0] * a[0] + b[1] * a[1]) + b[2] * a[2]
        b = weights(d)
        pos = mix3(b, *pos3)
        nrm0, nrm1, tan = mix3(b, *n03), mix3(b, *n13), mix3(b, *tan3)
        attr, xf = scalar(b, attr3), scalar(b, x3)
        # lv_prism_accept
        depth = len3(sub3(pos, cam))
        c0, c1 = [Q["centre"][k][seg[s, 0]] for k in range(3)], [Q["centre"][k][seg[s, 1]] for k in range(3)]
        radius = F(case.line_width) * F(0.5)
        vz = ((V.view[2] * pos[0] + V.view[6] * pos[1]) + V.view[10] * pos[2]) + V.view[14] * F(1.0)
        kept = (depth >= T_LO) & (depth < T_HI) & own_box(cam, d, c0, c1, radius, depth) & (-vz >= F(case.near)) & (-vz <= F(case.far))
        zbits = window_depth(np.stack(pos, 1), V.view, V.proj).view(np.uint32)
        # fwidth(|x|) from the 2 x 2 partners' rays on the same planes
        dX, dY = raster_quad(V, x, y)
        f0, fx, fy = np.abs(xf), np.abs(scalar(weights(dX), x3)), np.abs(scalar(weights(dY), x3))
        eps_white = np.abs(fx - f0) + np.abs(fy - f0)
        # the build-owned normal
        xc = clampf(xf, -1.0, 1.0)
        cs = np.sqrt(fmaf(-xc, xc, F(1.0)))
        u0, u1 = norm_shade(nrm0), norm_shade(nrm1)
        normal = [cs * u0[k] + xc * u1[k] for k in range(3)]
        ao_texel = np.ascontiguousarray(ao[y, x], dtype=F) if (ao is not None and P.useAmbientOcclusion) else np.ones(n, F)
        lit = compute_fragment_color(case.tf, P, V, pos, normal, tan, np.zeros(n, bool), attr, ao_texel)
        eps = clampf(((depth / F(case.line_width)) * F(2.0)) / F(V.h) * F(case.fovy), 0.0, 0.49)
        w = smoothstepf(F(0.7) - eps_white, F(0.7) + eps_white, f0)
        fg = [F(1.0) - F(case.background[k]) for k in range(3)]
        rgba = [mixf(lit[k], fg[k], w) for k in range(3)] + [lit[3] * (F(1.0) - smoothstepf(F(1.0) - eps, F(1.0), f0))]
    return dict(kept=kept, zbits=zbits, rgba=np.stack(rgba, 1).astype(F) if n else np.zeros((0, 4), F),
                pos=np.stack(pos, 1) if n else np.zeros((0, 3), F), x=xf, eps_white=eps_white)


def quad_fragments(case, V=None, requested=None, ao=None, depth_range=None):
    """Every kept line-quad fragment of the viewport: dict of pixel (y * w + x), seg, tri, zbits (uint32), rgba (n, 4) float32, pos, x
    -- sorted by (pixel, segment, triangle).  ao, depth_range: the AO image (h, w) and the depth range the lighting reads (default: the
    checker's depth range, no AO image)"""
    V = V or View(case)
    seg = case.seg.astype(np.int64)
    Q = quad_points(case.points, V, case.line_width)
    P = shading_params(case, depth_range)
    s, x, y = pairs_of(quad_setup(Q, seg, V))
    cov, _ = quad_coverage(Q, seg, V, s, x, y)
    rows = [np.nonzero(cov[t])[0] for t in range(2)]
    t = np.concatenate([np.full(len(r), k, np.int64) for k, r in enumerate(rows)])
    r = np.concatenate(rows)
    s, x, y = s[r], x[r], y[r]
    fr = quad_fragment(case, Q, seg, V, P, s, x, y, t, ao)
    keep = fr["kept"]
    if requested is not None:
        keep = keep & requested[y, x]
    pixel = (y * V.w + x).astype(np.uint32)
    order = np.lexsort((t[keep], s[keep], pixel[keep]))
    pick = lambda a: a[keep][order]
    return dict(pixel=pick(pixel), seg=pick(s).astype(np.uint32), tri=pick(t).astype(np.uint32), zbits=pick(fr["zbits"]),
                rgba=pick(fr["rgba"]), pos=pick(fr["pos"]), x=pick(fr["x"]), eps_white=pick(fr["eps_white"]))


# ---------------------------------------------------------------- the scalar transcription
def quad_pair(case, V, s, x, y, ao=None, depth_range=None):
    """ONE (segment, pixel), step by step on float32 scalars with the device's control flow: the list of (triangle, zbits, [r, g, b, a])
    of its kept fragments.  The lighting is the checker's computeFragmentColor on one-element arrays."""
    f = lambda v: F(v)
    mul, add, sub = (lambda a, b: F(f(a) * f(b))), (lambda a, b: F(f(a) + f(b))), (lambda a, b: F(f(a) - f(b)))
    dot = lambda a, b: add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))
    pdot = lambda a, b: fmaf(a[2], b[2], fmaf(a[1], b[1], mul(a[0], b[0])))
    crs = lambda a, b: [sub(mul(a[1], b[2]), mul(b[1], a[2])), sub(mul(a[2], b[0]), mul(b[2], a[0])), sub(mul(a[0], b[1]), mul(b[0], a[1]))]

    def normalize(a):
        r = F(F(1.0) / F(np.sqrt(F(np.fmin(np.fmax(dot(a, a), F(2.0 ** -60)), F(2.0 ** 60))))))
        return [mul(c, r) for c in a]

    def m4(m, v):
        return [add(add(add(mul(m[i], v[0]), mul(m[4 + i], v[1])), mul(m[8 + i], v[2])), mul(m[12 + i], v[3])) for i in range(4)]

    with np.errstate(all="ignore"):
        cam = [f(c) for c in V.cam]
        lw = f(case.line_width)
        ids = [int(case.seg[s, 0]), int(case.seg[s, 1])]
        verts, n0s, n1s, tans, attrs, centres = [], [], [], [], [], []
        for i in ids:                                                  # the vertex stage
            lp = [f(c) for c in case.points["linePosition"][i]]
            tr = [f(c) for c in case.points["lineTangent"][i]]
            t = normalize(tr)
            view = normalize([sub(cam[k], lp[k]) for k in range(3)])
            od = normalize(crs(view, t))
            for sign in (F(-1.0), F(1.0)):
                h = mul(mul(sign, lw), F(0.5))
                verts.append([add(lp[k], mul(h, od[k])) for k in range(3)])
            n0s.append(normalize(crs(t, od)))
            n1s.append(od)
            tans.append(tr)
            attrs.append(f(case.points["lineAttribute"][i]))
            centres.append(lp)
        vid = [2 * ids[0], 2 * ids[0] + 1, 2 * ids[1], 2 * ids[1] + 1]
        # coverage
        D = [f(c) for c in V.cov[y, x]]
        right = [f(c) for c in V.right]
        P = crs(right, D)
        Qb = crs(D, P)
        X, Y = [], []
        for v in range(4):
            A = [sub(verts[v][k], cam[k]) for k in range(3)]
            X.append(pdot(A, P))
            Y.append(pdot(A, Qb))
        edge = lambda u, v: sub(mul(Y[u], X[v]), mul(X[u], Y[v]))
        ins = lambda e, owned: bool(e > 0 or (e == 0 and owned))
        e23, e30, e02, e31, e10 = edge(2, 3), edge(3, 0), edge(0, 2), edge(3, 1), edge(1, 0)
        e03 = F(-e30)
        covered = [ins(e23, vid[2] < vid[3]) and ins(e30, vid[3] < vid[0]) and ins(e02, vid[0] < vid[2]) and add(add(e23, e30), e02) > 0,
                   ins(e31, vid[3] < vid[1]) and ins(e10, vid[1] < vid[0]) and ins(e03, vid[0] < vid[3]) and add(add(e31, e10), e03) > 0]
        out = []
        Pm = shading_params(case, depth_range)
        for t in range(2):
            if not covered[t]:
                continue
            tri = TRIANGLES[t]
            d = [f(c) for c in V.ray[y, x]]
            Pb = crs(right, d)
            Qd = crs(d, Pb)
            vv = []
            for v in tri:
                A = [sub(verts[v][k], cam[k]) for k in range(3)]
                vv.append([pdot(A, Pb), pdot(A, Qd), pdot(A, d)])
            c = [crs(vv[1], vv[2]), crs(vv[2], vv[0]), crs(vv[0], vv[1])]

            def weights(Dr):
                abg = [pdot(Dr, Pb), pdot(Dr, Qd), pdot(Dr, d)]
                e = [pdot(abg, c[i]) for i in range(3)]
                rs = F(F(1.0) / add(add(e[0], e[1]), e[2]))
                return [mul(a, rs) for a in e]

            scalar = lambda b, a: add(add(mul(b[0], a[0]), mul(b[1], a[1])), mul(b[2], a[2]))
            vec = lambda b, a: [scalar(b, [a[0][k], a[1][k], a[2][k]]) for k in range(3)]
            b = weights(d)
            pos = vec(b, [verts[v] for v in tri])
            nrm0, nrm1 = vec(b, [n0s[v >> 1] for v in tri]), vec(b, [n1s[v >> 1] for v in tri])
            tan = vec(b, [tans[v >> 1] for v in tri])
            attr = scalar(b, [attrs[v >> 1] for v in tri])
            x3 = [F(1.0) if v & 1 else F(-1.0) for v in tri]
            xf = scalar(b, x3)
            rel = [sub(pos[k], cam[k]) for k in range(3)]
            depth = F(np.sqrt(dot(rel, rel)))
            if not (depth >= T_LO and depth < T_HI):
                continue
            radius = mul(lw, F(0.5))
            lo, hi = [], []
            for k in range(3):
                inv = F(F(1.0) / d[k])
                t0 = mul(sub(sub(F(np.fmin(centres[0][k], centres[1][k])), radius), cam[k]), inv)
                t1 = mul(sub(add(F(np.fmax(centres[0][k], centres[1][k])), radius), cam[k]), inv)
                lo.append(F(np.fmin(t0, t1)))
                hi.append(F(np.fmax(t0, t1)))
            tn = F(np.fmax(np.fmax(lo[0], lo[1]), lo[2]))
            tf = F(np.fmin(np.fmin(hi[0], hi[1]), hi[2]))
            slack = F(radius / F(np.sqrt(dot(d, d))))
            if not (tn <= tf and depth >= sub(tn, slack) and depth <= add(tf, slack)):
                continue
            vz = add(add(add(mul(V.view[2], pos[0]), mul(V.view[6], pos[1])), mul(V.view[10], pos[2])), mul(V.view[14], F(1.0)))
            if not (F(-vz) >= F(case.near) and F(-vz) <= F(case.far)):
                continue
            zbits = int(window_depth(np.array([pos], dtype=F), V.view, V.proj).view(np.uint32)[0])
            # the helper lanes
            sxp, syp = F(F(2.0) / F(V.w)), F(F(2.0) / F(V.h))
            ndc = [sub(mul(add(F(x), F(0.5)), sxp), F(1.0)), sub(mul(add(F(y), F(0.5)), syp), F(1.0))]
            target = m4(V.inv_proj, [ndc[0], ndc[1], F(1.0), F(1.0)])
            dd = m4(V.inv_view, [target[0], target[1], target[2], F(0.0)])
            gx, gy = m4(V.inv_proj, [sxp, F(0.0), F(0.0), F(0.0)]), m4(V.inv_proj, [F(0.0), syp, F(0.0), F(0.0)])
            Gx, Gy = m4(V.inv_view, gx[:3] + [F(0.0)]), m4(V.inv_view, gy[:3] + [F(0.0)])
            sx, sy = (F(-1.0) if x & 1 else F(1.0)), (F(-1.0) if y & 1 else F(1.0))
            dX = [add(dd[k], mul(sx, Gx[k])) for k in range(3)]
            dY = [add(dd[k], mul(sy, Gy[k])) for k in range(3)]
            f0, fx, fy = F(abs(xf)), F(abs(scalar(weights(dX), x3))), F(abs(scalar(weights(dY), x3)))
            eps_white = add(F(abs(sub(fx, f0))), F(abs(sub(fy, f0))))
            xc = F(np.fmin(np.fmax(xf, F(-1.0)), F(1.0)))
            cs = F(np.sqrt(fmaf(F(-xc), xc, F(1.0))))
            u0, u1 = normalize(nrm0), normalize(nrm1)
            normal = [add(mul(cs, u0[k]), mul(xc, u1[k])) for k in range(3)]
            one = lambda a: np.array([a], dtype=F)
            texel = one(ao[y, x]) if (ao is not None and Pm.useAmbientOcclusion) else one(1.0)
            lit = [F(a[0]) for a in compute_fragment_color(case.tf, Pm, V, [one(a) for a in pos], [one(a) for a in normal],
                                                           [one(a) for a in tan], np.zeros(1, bool), one(attr), texel)]
            eps = F(np.fmin(np.fmax(mul(F(mul(F(depth / lw), F(2.0)) / F(V.h)), F(case.fovy)), F(0.0)), F(0.49)))

            def smooth(e0, e1, v):
                tt = F(np.fmin(np.fmax(F(sub(v, e0) / sub(e1, e0)), F(0.0)), F(1.0)))
                return mul(mul(tt, tt), sub(F(3.0), mul(F(2.0), tt)))

            mix = lambda a, bb, w: add(mul(a, sub(F(1.0), w)), mul(bb, w))
            w = smooth(sub(F(0.7), eps_white), add(F(0.7), eps_white), f0)
            fg = [sub(F(1.0), F(case.background[k])) for k in range(3)]
            rgba = [mix(lit[k], fg[k], w) for k in range(3)] + [mul(lit[3], sub(F(1.0), smooth(sub(F(1.0), eps), F(1.0), f0)))]
            out.append((t, zbits, rgba))
    return out


# ---------------------------------------------------------------- the fixtures
LW = 0.02


@functools.lru_cache(maxsize=None)
def quad_case(kind="plain"):
    """(case, View) of the comparisons, computed once:
    plain   small_case's 30 lines x 30 points at 70 x 45, line width 0.02, the transparent transfer function
    odd     the same at 97 x 61
    wide    line width 0.06
    thin    line width 0.004
    cues    plain with RTAO (Screen Space) and depth cues"""
    w, h = (97, 61) if kind == "odd" else (70, 45)
    lw = {"wide": 0.06, "thin": 0.004}.get(kind, LW)
    settings = {}
    if kind == "cues":
        settings = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=0.6, ambient_occlusion_gamma=1.5,
                        ambient_occlusion_iterations=2, ambient_occlusion_samples_per_frame=2, depth_cue_strength=0.7)
    c = small_case(width=w, height=h, line_width=lw, transparent=True, camera_pos=(0.21, 0.13, 0.8), **settings)
    return c, View(c)


@functools.lru_cache(maxsize=None)
def reference_fragments(kind="plain"):
    c, V = quad_case(kind)
    ao = None
    if kind == "cues":
        sc = c.oracle_scene()
        ao = c.oracle_ao(sc, c.oracle_params(sc), mode=2)
    return quad_fragments(c, V, ao=ao)


def hand_case(positions, width=70, height=45, line_width=0.05, camera_pos=(0.0, 0.0, 0.8), tangents=None, attributes=None):
    """one polyline as a Case: tangents default to the normalised central differences createLineTubesRenderDataCPU would give a
    straight or gently bent line"""
    pos = np.asarray(positions, dtype=F)
    n = len(pos)
    pts = np.zeros(n, dtype=lvo.LINE_POINT_DTYPE)
    pts["linePosition"] = pos
    pts["lineAttribute"] = np.linspace(0.2, 0.8, n).astype(F) if attributes is None else attributes
    if tangents is None:
        d = np.gradient(pos.astype(np.float64), axis=0)
        tangents = d / np.linalg.norm(d, axis=1)[:, None]
    pts["lineTangent"] = np.asarray(tangents, dtype=F)
    pts["lineNormal"] = (0.0, 0.0, 1.0)
    seg = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.uint32)
    return Case(pts, seg, tfm.standard_transparent(), width, height, line_width, camera_pos=camera_pos)


def runs_of(pixel, num_pixels):
    """offsets per pixel of fragments sorted by pixel"""
    off = np.zeros(num_pixels + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(pixel, minlength=num_pixels))
    return off


def al64_keys(rgba, z):
    return al64_key(z, pack([rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]]))


def frame_references(case, fr, K=8, weight="reference", hull=None, max_colour=0):
    """The frames of modes 8, 10 and 5 drawn with quads: dict of wboit (frame, sums, counts), al64 (frame, slots, tail, counts past
    the discard), dc (frame, counts).  fr: quad_fragments(); hull: the hull's fragments (hull_fragments() of
    tests/test_hull_restatement.py) drawn after them, or None"""
    num = case.width * case.height
    off = runs_of(fr["pixel"], num)
    rgba, z = np.asarray(fr["rgba"], dtype=F), fr["zbits"].view(F)
    key, keep = al64_keys(rgba, z), rgba[:, 3] >= F(0.001)
    if hull is not None:
        hoff = runs_of(hull["pixel"], num)
        hrgba, hz = np.asarray(hull["rgba"], dtype=F), hull["zbits"].view(F)
        hkey, hkeep = al64_keys(hrgba, hz), hrgba[:, 3] >= F(0.001)
    wb, al = [], []
    for p in range(num):
        a, b = off[p], off[p + 1]
        if hull is None:
            wb.append((rgba[a:b], z[a:b]))
            al.append(key[a:b][keep[a:b]])
        else:
            ha, hb = hoff[p], hoff[p + 1]
            wb.append((np.concatenate([rgba[a:b], hrgba[ha:hb]]), np.concatenate([z[a:b], hz[ha:hb]])))
            al.append(np.concatenate([key[a:b][keep[a:b]], hkey[ha:hb][hkeep[ha:hb]]]))
    counts = np.array([len(r[1]) for r in wb], np.uint32)
    shape = (case.height, case.width)
    wf, ws = wboit_fold(wb, case.background, weight, details=True)
    af, slots, tail = al64_fold(al, K, case.background)
    return dict(wboit=(wf.reshape(shape + (4,)), ws.reshape(shape + (5,)), counts.reshape(shape)),
                al64=(af.reshape(shape + (4,)), slots.reshape(shape + (K,)), tail.reshape(shape + (5,)),
                      np.array([len(r) for r in al], np.uint32).reshape(shape)),
                dc=(depth_complexity_frame(counts, case.background, max_colour).reshape(shape + (4,)), counts.reshape(shape)))


# ---------------------------------------------------------------- an independent float64 screen-space rasteriser of the same quads
def rasterise64(case, margin=1e-4):
    """The quads in float64 screen space: the vertices of the float64 vertex stage projected with the view-projection matrix, ordinary
    2-D edge functions at the pixel centres, counter-clockwise triangles only (the front faces of this index pattern).  Returns the
    set of (pixel, segment, triangle) and `near`: the (pixel, segment, triangle) whose float64 edge value lies within `margin` pixels of
    zero (the rule of tests/test_prism_raster.py), which a float32 rasteriser may decide either way."""
    W, H = case.width, case.height
    view = np.asarray(case.view, np.float64).reshape(4, 4).T
    proj = np.asarray(case.proj, np.float64).reshape(4, 4).T
    cam = np.linalg.inv(view)[:3, 3]
    lp = case.points["linePosition"].astype(np.float64)
    tan = case.points["lineTangent"].astype(np.float64)
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None]
    with np.errstate(all="ignore"):
        od = unit(np.cross(unit(cam - lp), unit(tan)))
    half = 0.5 * float(case.line_width)
    vert = np.stack([lp - half * od, lp + half * od], 1)          # (points, side, 3)
    clip = np.concatenate([vert, np.ones(vert.shape[:2] + (1,))], 2) @ (proj @ view).T
    with np.errstate(all="ignore"):
        win = np.stack([(clip[..., 0] / clip[..., 3] + 1.0) * 0.5 * W, (clip[..., 1] / clip[..., 3] + 1.0) * 0.5 * H], 2)
    seg = case.seg.astype(np.int64)
    inside, near = set(), set()
    orient = 1.0 if proj[0, 0] * proj[1, 1] > 0 else -1.0
    for s, (a, b) in enumerate(seg):
        quad = [win[a, 0], win[a, 1], win[b, 0], win[b, 1]]
        if not np.isfinite(np.asarray(quad)).all() or (clip[[a, b], :, 3] <= 0).any():
            continue
        for t, tri in enumerate(TRIANGLES):
            p = [quad[v] for v in tri]
            xs, ys = [q[0] for q in p], [q[1] for q in p]
            x0, x1 = max(int(np.floor(min(xs) - 0.5)) - 1, 0), min(int(np.ceil(max(xs) - 0.5)) + 1, W - 1)
            y0, y1 = max(int(np.floor(min(ys) - 0.5)) - 1, 0), min(int(np.ceil(max(ys) - 0.5)) + 1, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            gx, gy = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
            area = lambda u, v: (v[0] - u[0]) * (gy - u[1]) - (v[1] - u[1]) * (gx - u[0])
            es = [area(p[1], p[2]), area(p[2], p[0]), area(p[0], p[1])]
            ln = [np.hypot(*(p[2] - p[1])), np.hypot(*(p[0] - p[2])), np.hypot(*(p[1] - p[0]))]
            # front faces: counter-clockwise in normalised device coordinates (E(U, V) of lv_prism.h is the 2-D cross product there),
            # which the window inherits unless the projection mirrors one axis
            es = [e * orient for e in es]
            ins = (es[0] >= 0) & (es[1] >= 0) & (es[2] >= 0) & ((es[0] + es[1] + es[2]) > 0)
            # an edge value within the margin of zero decides nothing where the other two edges let the pixel in
            with np.errstate(all="ignore"):
                dist = [np.abs(e) / l for e, l in zip(es, ln)]
                ok = [(es[i] >= 0) | ~(dist[i] >= margin) for i in range(3)]
                close = np.zeros_like(ins)
                for i in range(3):
                    close |= ~(dist[i] >= margin) & ok[(i + 1) % 3] & ok[(i + 2) % 3]
            for yy, xx in zip(*np.nonzero(ins)):
                inside.add(((y0 + yy) * W + (x0 + xx), s, t))
            for yy, xx in zip(*np.nonzero(close)):
                near.add(((y0 + yy) * W + (x0 + xx), s, t))
    return inside, near


# ---------------------------------------------------------------- the checks
def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def test_fmaf_rounds_once():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(20000).astype(F), rng.standard_normal(20000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.standard_normal(20000) * 1e-7)).astype(F)   # cancellation
    from fractions import Fraction
    got = fmaf(a, b, c)
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], F(-np.inf)).astype(np.float64)
        hi = np.nextafter(got[i], F(np.inf)).astype(np.float64)
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    # rounding the float64 sum first would round twice: (2^-12 - 2^-30) (2^-12 + 2^-30) = 2^-24 - 2^-60 puts the exact sum just below the
    # tie between c and its successor; the float64 sum lands on the tie and would go to the even neighbour above
    a0, b0, c0 = F(2.0 ** -12 - 2.0 ** -30), F(2.0 ** -12 + 2.0 ** -30), F(1.0 + 2.0 ** -23)
    assert F(np.float64(a0) * np.float64(b0) + np.float64(c0)) == F(1.0 + 2.0 ** -22)
    assert fmaf(a0, b0, c0) == c0
    assert fmaf(F(3.0), F(4.0), F(5.0)) == F(17.0)


def test_vectorised_statement_against_the_scalar_transcription():
    for kind in ("plain", "wide", "cues"):
        c, V = quad_case(kind)
        fr = reference_fragments(kind)
        ao = None
        if kind == "cues":
            sc = c.oracle_scene()
            ao = c.oracle_ao(sc, c.oracle_params(sc), mode=2)
        assert len(fr["pixel"]) > (1500 if kind == "wide" else 400), (kind, len(fr["pixel"]))
        rng = np.random.default_rng(11)
        have = {}
        for j in range(len(fr["pixel"])):
            have.setdefault((int(fr["pixel"][j]), int(fr["seg"][j])), []).append(j)
        keys = list(have)
        for k in rng.choice(len(keys), 60, replace=False):
            p, s = keys[k]
            got = quad_pair(c, V, s, p % V.w, p // V.w, ao=ao)
            rows = have[(p, s)]
            assert [g[0] for g in got] == [int(fr["tri"][j]) for j in rows], (kind, p, s)
            for g, j in zip(got, rows):
                assert g[1] == int(fr["zbits"][j]), (kind, p, s)
                assert [int(_bits(a)) for a in g[2]] == [int(a) for a in _bits(fr["rgba"][j])], (kind, p, s)
        misses = 0
        for _ in range(120):
            s, x, y = int(rng.integers(len(c.seg))), int(rng.integers(V.w)), int(rng.integers(V.h))
            if (y * V.w + x, s) not in have:
                assert quad_pair(c, V, s, x, y, ao=ao) == []
                misses += 1
        assert misses > 50


def test_against_the_independent_float64_rasteriser():
    for kind in ("plain", "odd", "wide", "thin"):
        c, V = quad_case(kind)
        fr = reference_fragments(kind)
        # the float32 statement before the kept rules, which the float64 rasteriser does not restate: every covered triangle
        seg = c.seg.astype(np.int64)
        Q = quad_points(c.points, V, c.line_width)
        s, x, y = pairs_of(quad_setup(Q, seg, V))
        cov, _ = quad_coverage(Q, seg, V, s, x, y)
        got = set()
        for t in range(2):
            r = np.nonzero(cov[t])[0]
            got |= set(zip((y[r] * V.w + x[r]).tolist(), s[r].tolist(), [t] * len(r)))
        want, near = rasterise64(c)
        total = len(got | want)
        assert total > (100 if kind == "thin" else 400), (kind, total)
        # the scenes keep the float64 rasteriser itself inside the cap
        assert len(near) <= 0.01 * total, (kind, len(near), total)
        assert (got ^ want) <= near, (kind, sorted((got ^ want) - near)[:5])
        # and the kept rules drop nothing in these scenes: the fragments are the covered triangles
        assert set(zip(fr["pixel"].tolist(), fr["seg"].tolist(), fr["tri"].tolist())) == got


def _straight(width=70, height=45, **kw):
    # a straight line across the view, off the pixel grid's axes, seen side-on
    t = np.linspace(-1.0, 1.0, 7)[:, None]
    return hand_case(np.array([0.013, 0.021, 0.0]) + t * np.array([0.23, 0.071, 0.0]), width, height, **kw)


def test_straight_line_side_on_gives_one_fragment_per_covered_pixel():
    c = _straight()
    V = View(c)
    fr = quad_fragments(c, V)
    counts = np.bincount(fr["pixel"], minlength=V.w * V.h)
    assert (counts > 0).sum() > 60 and set(np.unique(counts)) == {0, 1}       # no double hit on the diagonal or at a joint
    assert len(np.unique(fr["seg"])) == 6 and set(np.unique(fr["tri"])) == {0, 1}
    # pixels on both sides of every joint are covered: no gap either (the covered set is that of the float64 rasteriser)
    want, near = rasterise64(c)
    assert (set(zip(fr["pixel"].tolist(), fr["seg"].tolist(), fr["tri"].tolist())) ^ want) <= near


def test_coordinate_runs_from_minus_one_to_plus_one():
    c = _straight(width=140, height=90, line_width=0.08)
    V = View(c)
    fr = quad_fragments(c, V)
    x = fr["x"].astype(np.float64)
    assert x.min() < -0.9 and x.max() > 0.9 and np.abs(x).max() <= 1.0 + 1e-5
    # x is the signed distance from the axis over the radius, in float64 from the fragment's position
    lp = c.points["linePosition"].astype(np.float64)
    axis = (lp[-1] - lp[0]) / np.linalg.norm(lp[-1] - lp[0])
    rel = fr["pos"].astype(np.float64) - lp[0]
    across = rel - (rel @ axis)[:, None] * axis
    assert np.abs(np.linalg.norm(across, axis=1) / (0.5 * c.line_width) - np.abs(x)).max() < 2e-3
    # the rim: the fragments nearest the outline have absCoords close to 1, and their alpha falls off there
    rim = np.abs(x) > 0.97
    assert rim.sum() > 10 and (fr["rgba"][rim, 3] < fr["rgba"][np.abs(x) < 0.5, 3].min()).any()
    assert np.isfinite(fr["rgba"]).all()


def test_bow_tie_loses_exactly_its_flipped_triangle():
    # the second point's tangent is reversed: its offset direction crosses the first point's
    pos = np.array([(-0.15, 0.011, 0.0), (0.15, 0.023, 0.0)], dtype=F)
    d = (pos[1] - pos[0]) / np.linalg.norm(pos[1] - pos[0])
    straight = hand_case(pos, tangents=[d, d], line_width=0.12)
    tie = hand_case(pos, tangents=[d, -d], line_width=0.12)
    Vs, Vt = View(straight), View(tie)
    fs, ft = quad_fragments(straight, Vs), quad_fragments(tie, Vt)
    assert set(np.unique(fs["tri"])) == {0, 1} and len(fs["pixel"]) > 100
    # of the bow-tie's two triangles one keeps its winding and one is flipped: every fragment belongs to the kept one
    assert len(np.unique(ft["tri"])) == 1 and len(ft["pixel"]) > 30
    kept = int(ft["tri"][0])
    seg = tie.seg.astype(np.int64)
    Q = quad_points(tie.points, Vt, tie.line_width)
    s, x, y = pairs_of(quad_setup(Q, seg, Vt))
    cov, e = quad_coverage(Q, seg, Vt, s, x, y)
    assert cov[kept].sum() == len(ft["pixel"]) and cov[1 - kept].sum() == 0
    # the flipped one has every edge value negative somewhere inside it: it was culled, not missed
    flipped = [e["e23"], e["e30"], e["e02"]] if kept == 1 else [e["e31"], e["e10"], -e["e30"]]
    assert ((flipped[0] < 0) & (flipped[1] < 0) & (flipped[2] < 0)).sum() > 30


def test_line_pointing_at_the_camera_draws_nothing():
    """Every point on the camera's axis with its tangent along the view direction: cross(view, tangent) = 0.  The shading code's
    normalize clamps the squared length at 2^-60, so the offset direction is the zero vector, not NaN: both vertices of a point
    coincide, E(v, v) = 0 and the other two edge values cancel exactly -- (e0 + e1) + e2 > 0 fails, the quad draws nothing."""
    pos = np.array([(0.0, 0.0, z) for z in (-0.3, -0.1, 0.1, 0.3)], dtype=F)
    c = hand_case(pos, tangents=np.tile([0.0, 0.0, 1.0], (4, 1)))
    V = View(c)
    Q = quad_points(c.points, V, c.line_width)
    assert all(np.array_equal(Q["minus"][k], Q["plus"][k]) and np.isfinite(Q["plus"][k]).all() for k in range(3))
    fr = quad_fragments(c, V)
    assert len(fr["pixel"]) == 0 and quad_pair(c, V, 1, V.w // 2, V.h // 2) == []
    # the same line a little off the axis, seen almost end-on: whatever it draws is finite
    c = hand_case(pos + np.array([1e-4, 2e-4, 0.0], F), tangents=np.tile([0.0, 0.0, 1.0], (4, 1)))
    assert np.isfinite(quad_fragments(c, View(c))["rgba"]).all()
    # one such point in an otherwise ordinary line: its two segments taper to it (one triangle each is degenerate), the colours are finite
    pos = np.array([(-0.2, 0.01, 0.0), (-0.1, 0.0, 0.0), (0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.2, 0.01, 0.0)], dtype=F)
    tang = np.tile([1.0, 0.0, 0.0], (5, 1))
    tang[2] = (0.0, 0.0, 1.0)
    c = hand_case(pos, tangents=tang)
    fr = quad_fragments(c, View(c))
    assert set(np.unique(fr["seg"])) == {0, 1, 2, 3} and np.isfinite(fr["rgba"]).all()
    assert set(np.unique(fr["tri"][fr["seg"] == 1])) == {1} and set(np.unique(fr["tri"][fr["seg"] == 2])) == {0}
    # genuinely non-finite input (a NaN tangent) draws nothing either: NaN edge values fail every comparison
    tang[2] = (np.nan, 0.0, 0.0)
    c = hand_case(pos, tangents=tang)
    fr = quad_fragments(c, View(c))
    assert set(np.unique(fr["seg"])) == {0, 3} and np.isfinite(fr["rgba"]).all()


def test_the_clamp_keeps_the_normal_finite():
    """|x| > 1 by rounding.  A straight line along x in the plane z = 0, seen from (0, 0, 0.8): its quad lies in that plane, and this
    line width (three float32 steps below twice the height of a pixel row at z = 0) puts the rim on the centres of the pixel rows next
    to the axis'.  There the weights of the rim's two vertices sum to 1 + an ulp or two and the third weight is 0 or tiny: the
    interpolated coordinate overshoots.  asin is NaN there, and so is sqrt(1 - x^2) without the clamp."""
    pos = np.array([(-0.2, 0.0, 0.0), (0.0, 0.0, 0.0), (0.2, 0.0, 0.0)], dtype=F)
    c = hand_case(pos, line_width=0.03555554151535034, tangents=np.tile([1.0, 0.0, 0.0], (3, 1)))
    V = View(c)
    fr = quad_fragments(c, V)
    over = np.abs(fr["x"]) > F(1.0)
    assert over.sum() >= 10 and len(fr["pixel"]) > 40
    assert np.isfinite(fr["rgba"]).all() and (fr["rgba"][over, 3] == 0).all()      # (coverage 0 on the rim itself)
    x = fr["x"][over]
    with np.errstate(all="ignore"):
        assert np.isnan(np.sqrt(fmaf(-x, x, F(1.0)))).all() and np.isnan(np.arcsin(x)).all()
    # the scalar transcription takes the same path
    j = int(np.nonzero(over)[0][0])
    p, s = int(fr["pixel"][j]), int(fr["seg"][j])
    got = [g for g in quad_pair(c, V, s, p % V.w, p // V.w) if g[0] == int(fr["tri"][j])]
    assert len(got) == 1 and [int(_bits(a)) for a in got[0][2]] == [int(a) for a in _bits(fr["rgba"][j])]
