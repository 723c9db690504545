"""Rendering mode 1, the deferred visibility-buffer renderer (linevis_amd/csrc/lv_deferred.h; include/linevis_hip.h,
deferred_rendering_mode), restated in float32 numpy: one operation at a time, left to right, no contraction.

deferred_visibility() restates the visibility pass -- the rectangle, the facing, the ray-space coverage with its fill rule, the
window depth of the perspective-correct position, the 64-bit atomicMin -- vectorised over (triangle, pixel) pairs; visibility_pair()
is its scalar transcription.  deferred_shade() restates the shading pass: the position from the depth, the barycentrics from area
ratios, LineAttributesBarycentric.glsl, then computeFragmentColor (the checker's own restatement, Scene.compute_fragment_color) with
the transfer function's alpha forced to 1.  tests/test_gpu_deferred.py compares the device with both, bit for bit / within 2 LSB.

Here, without a GPU: the vectorised form against the scalar one; the visibility buffer against an independent float64 screen-space
rasteriser and against the brute-force closest hits of the pixel-centre rays; the edge cases of the rules."""
import numpy as np

from common import small_case
from linevis_amd import camera, scenes
from oracle import lvo
from test_mlab_restatement import window_depth

F = np.float32
NO_PRIMITIVE = np.uint32(0xFFFFFFFF)
Z_ONE = np.uint32(0x3F800000)
EMPTY = (np.uint64(0x3F800000) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
BBOX_MARGIN = F(0.015625)


def cross3(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def len3(a):
    return np.sqrt(dot3(a, a))


def mul_m4(m, x, y, z, w):
    """column-major mat4 * vec4, columns summed left to right (mulM4)"""
    return [((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i] * w for i in range(4)]


class View:
    """The frame constants both passes read: the matrices and their float32 inverses, the camera position, the right axis, the
    coverage direction (lv_prism_cov_dir) and the generator's ray of every pixel centre -- those two from the checker, which the device
    equals bit for bit (tests/test_prism_raster.py)."""

    def __init__(self, case):
        self.w, self.h = case.width, case.height
        self.view = np.asarray(case.view, dtype=F).reshape(16)
        self.proj = np.asarray(case.proj, dtype=F).reshape(16)
        self.inv_view = np.asarray(lvo.mat4_inverse(self.view), dtype=F).reshape(16)
        self.inv_proj = np.asarray(lvo.mat4_inverse(self.proj), dtype=F).reshape(16)
        self.cam = self.inv_view[12:15].copy()
        self.right = self.inv_view[0:3].copy()
        P = lvo.make_params(self.view, self.proj, self.w, self.h)
        self.cov = np.zeros((self.h, self.w, 3), dtype=F)
        self.ray = np.zeros((self.h, self.w, 3), dtype=F)
        for y in range(self.h):
            for x in range(self.w):
                self.cov[y, x], self.ray[y, x] = lvo.prism_coverage_dir(P, x, y)


def triangle_setup(mesh, V, cull):
    """lv_vis_setup for every triangle: world positions, positions relative to the camera, the owned edges, the facing, the pixel
    rectangle (x1 < x0: covers nothing)."""
    idx, verts, _ = mesh
    idx = np.asarray(idx, dtype=np.uint32).reshape(-1, 3)
    W, H = F(V.w), F(V.h)
    pos = [np.ascontiguousarray(verts["vertexPosition"][idx[:, i]], dtype=F) for i in range(3)]
    A = [[p[:, k] - V.cam[k] for k in range(3)] for p in pos]
    n = len(idx)
    all_behind, any_behind = np.ones(n, bool), np.zeros(n, bool)
    sx_min, sx_max = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    sy_min, sy_max = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    with np.errstate(all="ignore"):
        for p in pos:
            v = mul_m4(V.view, p[:, 0], p[:, 1], p[:, 2], F(1.0))
            c = mul_m4(V.proj, v[0], v[1], v[2], v[3])
            behind = ~(c[3] > 0)
            any_behind |= behind
            all_behind &= behind | (c[2] < 0)
            sx = ((c[0] / c[3]) * F(0.5) + F(0.5)) * W
            sy = ((c[1] / c[3]) * F(0.5) + F(0.5)) * H
            sx_min, sx_max = np.fmin(sx_min, sx), np.fmax(sx_max, sx)
            sy_min, sy_max = np.fmin(sy_min, sy), np.fmax(sy_max, sy)
        d10 = [A[1][k] - A[0][k] for k in range(3)]
        d20 = [A[2][k] - A[0][k] for k in range(3)]
        det = dot3(A[0], cross3(d10, d20))
        x0 = np.fmin(np.fmax(np.ceil((sx_min - BBOX_MARGIN) - F(0.5)), F(0.0)), W)
        x1 = np.fmin(np.fmax(np.floor((sx_max + BBOX_MARGIN) - F(0.5)), F(-1.0)), W - F(1.0))
        y0 = np.fmin(np.fmax(np.ceil((sy_min - BBOX_MARGIN) - F(0.5)), F(0.0)), H)
        y1 = np.fmin(np.fmax(np.floor((sy_max + BBOX_MARGIN) - F(0.5)), F(-1.0)), H - F(1.0))
    flip = det > 0
    ok = ~all_behind & (det != 0) & ~(flip & bool(cull))
    x0 = np.where(any_behind, 0, np.nan_to_num(x0)).astype(np.int64)
    y0 = np.where(any_behind, 0, np.nan_to_num(y0)).astype(np.int64)
    x1 = np.where(any_behind, V.w - 1, np.nan_to_num(x1)).astype(np.int64)
    y1 = np.where(any_behind, V.h - 1, np.nan_to_num(y1)).astype(np.int64)
    x1 = np.where(ok, x1, x0 - 1)
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    own = [np.where(flip, i2 < i1, i1 < i2), np.where(flip, i0 < i2, i2 < i0), np.where(flip, i1 < i0, i0 < i1)]
    return dict(pos=pos, A=A, own=own, flip=flip, x0=x0, y0=y0, x1=x1, y1=y1, det=det, ok=ok, any_behind=any_behind)


def pairs_of(S):
    """every (triangle, x, y) of the rectangles"""
    nx = np.maximum(S["x1"] - S["x0"] + 1, 0)
    ny = np.maximum(S["y1"] - S["y0"] + 1, 0)
    cnt = nx * ny
    tri = np.repeat(np.arange(len(cnt)), cnt)
    first = np.cumsum(cnt) - cnt
    k = np.arange(int(cnt.sum())) - np.repeat(first, cnt)
    nxr = np.repeat(nx, cnt)
    return tri, S["x0"][tri] + k % np.maximum(nxr, 1), S["y0"][tri] + k // np.maximum(nxr, 1)


def coverage(V, S, tri, x, y):
    """lv_vis_cover for pairs: (covered, e0, e1, e2)"""
    D = [V.cov[y, x, k] for k in range(3)]
    Pb = cross3(list(V.right), D)
    Qb = cross3(D, Pb)
    X = [dot3([S["A"][i][k][tri] for k in range(3)], Pb) for i in range(3)]
    Y = [dot3([S["A"][i][k][tri] for k in range(3)], Qb) for i in range(3)]
    edge = lambda u, v: Y[u] * X[v] - X[u] * Y[v]
    e = [edge(1, 2), edge(2, 0), edge(0, 1)]
    flip = S["flip"][tri]
    e = [np.where(flip, -a, a) for a in e]
    inside = [(e[i] > 0) | ((e[i] == 0) & S["own"][i][tri]) for i in range(3)]
    return inside[0] & inside[1] & inside[2] & ((e[0] + e[1]) + e[2] > 0), e


def depth_bits(V, S, tri, e):
    """lv_vis_depth_bits"""
    with np.errstate(all="ignore"):
        rs = F(1.0) / ((e[0] + e[1]) + e[2])
        b = [a * rs for a in e]
        pos = np.stack([(b[0] * S["pos"][0][tri, k] + b[1] * S["pos"][1][tri, k]) + b[2] * S["pos"][2][tri, k] for k in range(3)], 1)
        return window_depth(pos, V.view, V.proj).view(np.uint32)


def deferred_visibility(mesh, V, cull=True, requested=None):
    """The words of a mode-1 frame, (h, w) uint64: (bits(z) << 32) | primitive index, EMPTY where nothing is kept."""
    S = triangle_setup(mesh, V, cull)
    tri, x, y = pairs_of(S)
    cov, e = coverage(V, S, tri, x, y)
    tri, x, y, e = tri[cov], x[cov], y[cov], [a[cov] for a in e]
    zb = depth_bits(V, S, tri, e)
    keep = zb < Z_ONE                                # 0 <= z < 1: the sign bit, z >= 1 and NaN are refused
    if requested is not None:
        keep &= requested[y, x]
    words = np.full(V.w * V.h, EMPTY, dtype=np.uint64)
    key = (zb[keep].astype(np.uint64) << np.uint64(32)) | tri[keep].astype(np.uint64)
    np.minimum.at(words, (y[keep] * V.w + x[keep]), key)
    return words.reshape(V.h, V.w)


def split(words):
    return (words & np.uint64(0xFFFFFFFF)).astype(np.uint32), (words >> np.uint64(32)).astype(np.uint32).view(F)


def visibility_pair(mesh, V, tri, x, y, cull=True):
    """The scalar transcription of lv_vis_setup + lv_vis_cover + lv_vis_depth_bits for ONE (triangle, pixel): the key, or None."""
    idx, verts, _ = mesh
    ids = [int(i) for i in np.asarray(idx).reshape(-1, 3)[tri]]
    Vw = [[F(c) for c in verts["vertexPosition"][i]] for i in ids]
    A = [[F(p[k] - V.cam[k]) for k in range(3)] for p in Vw]
    all_behind, any_behind = True, False
    sxs, sys_ = [], []
    with np.errstate(all="ignore"):
        for p in Vw:
            v = mul_m4(V.view, p[0], p[1], p[2], F(1.0))
            c = mul_m4(V.proj, v[0], v[1], v[2], v[3])
            behind = not (c[3] > 0)
            any_behind = any_behind or behind
            all_behind = all_behind and (behind or c[2] < 0)
            sxs.append(F(F(F(c[0] / c[3]) * F(0.5) + F(0.5)) * F(V.w)))
            sys_.append(F(F(F(c[1] / c[3]) * F(0.5) + F(0.5)) * F(V.h)))
        if all_behind:
            return None
        det = dot3(A[0], cross3([A[1][k] - A[0][k] for k in range(3)], [A[2][k] - A[0][k] for k in range(3)]))
        if det == 0:
            return None
        flip = bool(det > 0)
        if flip and cull:
            return None
        if not any_behind:
            x0 = min(max(np.ceil(F(F(np.fmin.reduce(sxs) - BBOX_MARGIN) - F(0.5))), 0.0), V.w)
            x1 = min(max(np.floor(F(F(np.fmax.reduce(sxs) + BBOX_MARGIN) - F(0.5))), -1.0), V.w - 1.0)
            y0 = min(max(np.ceil(F(F(np.fmin.reduce(sys_) - BBOX_MARGIN) - F(0.5))), 0.0), V.h)
            y1 = min(max(np.floor(F(F(np.fmax.reduce(sys_) + BBOX_MARGIN) - F(0.5))), -1.0), V.h - 1.0)
            if not (x0 <= x <= x1 and y0 <= y <= y1):
                return None
        own = [ids[2] < ids[1], ids[0] < ids[2], ids[1] < ids[0]] if flip else [ids[1] < ids[2], ids[2] < ids[0], ids[0] < ids[1]]
        D = [F(c) for c in V.cov[y, x]]
        Pb = cross3([F(c) for c in V.right], D)
        Qb = cross3(D, Pb)
        X = [dot3(a, Pb) for a in A]
        Y = [dot3(a, Qb) for a in A]
        e = [F(Y[1] * X[2] - X[1] * Y[2]), F(Y[2] * X[0] - X[2] * Y[0]), F(Y[0] * X[1] - X[0] * Y[1])]
        if flip:
            e = [F(-a) for a in e]
        if not all(a > 0 or (a == 0 and o) for a, o in zip(e, own)):
            return None
        s = F(F(e[0] + e[1]) + e[2])
        if not s > 0:
            return None
        rs = F(F(1.0) / s)
        b = [F(a * rs) for a in e]
        pos = [F(F(F(b[0] * Vw[0][k]) + F(b[1] * Vw[1][k])) + F(b[2] * Vw[2][k])) for k in range(3)]
        zb = int(window_depth(np.array([pos], dtype=F), V.view, V.proj).view(np.uint32)[0])
    if not zb < int(Z_ONE):
        return None
    return (zb << 32) | tri


def unorm8(c):
    return np.floor(np.fmin(np.fmax(c, F(0.0)), F(1.0)) * F(255.0) + F(0.5)).astype(np.uint8)


# ---------------------------------------------------------------- computeFragmentColor in float32, the three variants
PLAIN, BANDS, HELICITY = 0, 1, 2
PI = F(3.14159265358979323846)
RSQRT_LO, RSQRT_HI = F(2.0 ** -60), F(2.0 ** 60)


def _eval(name, *args):
    """a build-owned scalar function of the checker (sincos_rad, atan2_det) on float32 arrays"""
    w = np.stack([np.ascontiguousarray(a, dtype=F).view(np.uint32) for a in np.broadcast_arrays(*args)], 1)
    out = lvo.eval_words(name, w)
    return [np.ascontiguousarray(out[:, k]).view(F) for k in range(out.shape[1])]


def norm3(a):
    ln = len3(a)
    return [c / ln for c in a]


def norm_shade(a):
    """normalize() of the shading code: v * (1 / sqrt(clamp(v . v, 2^-60, 2^60))) (lv_rsqrt_shade is that value, correctly rounded)"""
    r = F(1.0) / np.sqrt(np.fmin(np.fmax(dot3(a, a), RSQRT_LO), RSQRT_HI))
    return [c * r for c in a]


def clampf(x, lo, hi):
    return np.fmin(np.fmax(x, F(lo)), F(hi))


def mixf(a, b, w):
    return a * (F(1.0) - w) + b * w


def smoothstepf(e0, e1, x):
    t = clampf((x - e0) / (e1 - e0), 0.0, 1.0)
    return t * t * (F(3.0) - F(2.0) * t)


def transfer_function(tf, attr, attr_min, attr_max):
    n = len(tf)
    pos = clampf((attr - F(attr_min)) / (F(attr_max) - F(attr_min)), 0.0, 1.0)
    u = pos * F(n) - F(0.5)
    fl = np.floor(u)
    f = u - fl
    i0 = np.clip(fl.astype(np.int64), 0, n - 1)
    i1 = np.clip(fl.astype(np.int64) + 1, 0, n - 1)
    return [tf[i0, k] * (F(1.0) - f) + tf[i1, k] * f for k in range(4)]


def bands_ribbon_of_point(cam, line_position, line_normal, fragment_tangent, t, pH, line_radius, thickness):
    """lv_bands_ribbon_of_point (RayHitCommon.glsl:232-351); l.z is -1, so the first of its three cases is the one that runs"""
    lineN = norm3(line_normal)
    lineB = cross3(t, lineN)
    cN = [cam[k] - line_position[k] for k in range(3)]
    dist = dot3(cN, fragment_tangent)
    wv = [cN[k] - dist * fragment_tangent[k] for k in range(3)]
    c = [dot3(lineN, wv) / line_radius, dot3(lineB, wv) / line_radius, F(1.0)]
    a = F(1.0) / (thickness * thickness)
    l = [a * c[0], c[1], F(-1.0)]
    zero = np.zeros_like(l[0])
    Ml = [[zero, -l[2], l[1]], [l[2], zero, -l[0]], [-l[1], l[0], zero]]
    B = [[l[2] * l[2] - l[1] * l[1], l[0] * l[1], -l[0] * l[2]],
         [l[0] * l[1], a * l[2] * l[2] - l[0] * l[0], -a * l[1] * l[2]],
         [-l[0] * l[2], -a * l[1] * l[2], a * l[1] * l[1] + l[0] * l[0]]]
    discr = -B[0][0] * B[1][1] + B[0][1] * B[1][0]
    alpha = np.sqrt(discr) / l[2]
    Cm = [[B[i][j] + alpha * Ml[i][j] for j in range(3)] for i in range(3)]
    pm0x = pm0y = pm1x = pm1y = zero
    for i in range(2):
        on = np.abs(Cm[i][i]) > F(1e-4)
        pm0x, pm0y = np.where(on, Cm[i][0] / Cm[i][2], pm0x), np.where(on, Cm[i][1] / Cm[i][2], pm0y)
        pm1x, pm1y = np.where(on, Cm[0][i] / Cm[2][i], pm1x), np.where(on, Cm[1][i] / Cm[2][i], pm1y)
    pl = cross3(l, cross3(c, pH))
    plx, ply = pl[0] / pl[2], pl[1] / pl[2]
    num = np.sqrt((plx - pm0x) * (plx - pm0x) + (ply - pm0y) * (ply - pm0y))
    den = np.sqrt((pm1x - pm0x) * (pm1x - pm0x) + (pm1y - pm0y) * (pm1y - pm0y))
    return num / den * F(2.0) - F(1.0)


def compute_fragment_color(tf, P, V, pos, nrm, tan, is_cap, attr, ao_texel, variant=PLAIN, bands=None):
    """lv_compute_fragment_color_t<variant> (computeFragmentColor + blinnPhongShadingTube) on lists of three float32 arrays; bands:
    phi, and linePosition / lineNormal (BANDS) or rotation / separatorScale (HELICITY).  Returns four float32 arrays."""
    with np.errstate(all="ignore"):
        cam = [V.cam[k] for k in range(3)]
        fc = transfer_function(np.asarray(tf, dtype=F).reshape(-1, 4), attr, P.attrMin, P.attrMax)
        n = norm_shade(nrm)
        vv = norm_shade([cam[k] - pos[k] for k in range(3)])
        t = norm_shade(tan)
        helper = norm_shade(cross3(t, vv))
        newV = norm_shade(cross3(helper, t))
        rp = np.zeros_like(attr)
        if P.useHalos:
            c2 = cross3(newV, n)
            tube = len3(c2)
            tube = clampf(np.where(dot3(t, c2) < 0, -tube, tube), -1.0, 1.0)
            if variant == BANDS:
                thickness = F(P.minThickness)
                sp, cp = _eval("sincos_rad", bands["phi"])
                tube = bands_ribbon_of_point(cam, bands["linePosition"], bands["lineNormal"], tan, t, [thickness * cp, sp, F(1.0)],
                                             F(P.bandWidth) * F(0.5), thickness)
            cv = cross3(vv, n)
            neg = dot3(t, cv) < 0
            r1 = len3(cv)
            r2 = len3(c2)
            r2 = clampf(np.where(neg, -r2, r2), -1.0, 1.0)
            r1 = np.where(neg, -r1, r1)
            cap = np.where(np.abs(r2) < np.abs(r1), r2, r1)
            rp = np.where(is_cap & bool(P.useCappedTubes), cap, tube)
        aoF = F(1.0)
        if P.useAmbientOcclusion:
            aoF = np.fmax(F(0.0), (F(1.0) - F(P.aoStrength)) + F(P.aoStrength) * lvo.pow_det(ao_texel, F(P.aoGamma)))
            kA, kD = F(0.2) + (F(1.0) - aoF) * F(0.5), F(0.9) * aoF
        else:
            kA, kD = F(0.1), F(0.9)
        nB, tB = norm_shade(n), norm_shade(t)
        hh = norm_shade([vv[k] + vv[k] for k in range(3)])
        newL = norm_shade(cross3(norm_shade(cross3(tB, vv)), tB))
        exponent = F(1.0) if variant == BANDS else F(1.7)
        cos1 = lvo.pow_det(clampf(np.abs(dot3(nB, vv)), 0.0, 1.0), exponent)
        cos2 = lvo.pow_det(clampf(np.abs(dot3(nB, newL)), 0.0, 1.0), exponent)
        comb = F(0.3) * cos1 + F(0.7) * cos2
        spec = F(0.3) * lvo.pow_det(clampf(np.abs(dot3(nB, hh)), 0.0, 1.0), F(30.0))
        phong = [(kA * fc[k] + (kD * comb) * fc[k]) + spec * F(1.0) for k in range(3)]
        if P.useAmbientOcclusion:
            phong = [c * aoF for c in phong]
        if P.useDepthCues:
            s4 = mul_m4(V.view, pos[0], pos[1], pos[2], F(1.0))
            dcf = clampf((-s4[2] - F(P.minDepth)) / (F(P.maxDepth) - F(P.minDepth)), 0.0, 1.0)
            dcf = (dcf * dcf) * F(P.depthCueStrength)
            phong = [mixf(c, F(0.5), dcf) for c in phong]
        abs_coords = np.abs(rp) if P.useHalos else np.zeros_like(rp)
        depth = len3([pos[k] - cam[k] for k in range(3)])
        H = F(P.height)
        aaO = ((depth / F(P.lineWidth)) * F(0.05)) / H * F(P.fovY)
        aaW = ((depth / F(P.lineWidth)) * F(2.0)) / H * F(P.fovY)
        if variant == BANDS:
            aaO = aaW = ((depth / F(P.bandWidth)) * F(0.25)) / H * F(P.fovY)
        eps_outline, eps_white, threshold = clampf(aaO, 0.0, 0.49), clampf(aaW, 0.0, 0.49), F(0.7)
        if variant == HELICITY:      # drawSeparatorStripe, RayHitCommon.glsl:455-486
            sep = F(P.separatorBaseWidth) / bands["separatorScale"]
            period = F(2.0) / F(P.numSubdivisionsBands) * PI
            x = bands["phi"] + bands["rotation"] + sep * F(0.5)
            frac = x - period * np.floor(x / period)
            aaf = eps_outline * F(10.0)
            m = np.fmax(smoothstepf(aaf, F(0.0), frac), smoothstepf(sep - aaf * F(0.5), sep + aaf * F(0.5), frac))
            phong = [c * m for c in phong]
            threshold = F(0.8)
        coverage = F(1.0) - smoothstepf(F(1.0) - eps_outline, F(1.0), abs_coords) if P.useHalos else np.ones_like(rp)
        if variant == BANDS and P.useEllipticTubes:
            coverage = np.ones_like(rp)
        w = smoothstepf(threshold - eps_white, threshold + eps_white, abs_coords)
        fg = [F(1.0) - F(P.background[k]) for k in range(3)]
        return [mixf(phong[k], fg[k], w) for k in range(3)] + [fc[3] * coverage]


def deferred_fragment(V, w, h, xs, ys, zz, p):
    """lv_deferred_fragment (DeferredShading.glsl:103-124): the position from the pixel centre and the depth through the inverse
    matrices, (u, v, 1 - u - v) from cross-product areas.  p: the triangle's three positions, lists of three arrays"""
    with np.errstate(all="ignore"):
        fx, fy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
        nx, ny = F(2.0) * fx / F(w) - F(1.0), F(2.0) * fy / F(h) - F(1.0)
        pv = mul_m4(V.inv_proj, nx, ny, zz, F(1.0))
        pw = mul_m4(V.inv_view, pv[0], pv[1], pv[2], pv[3])
        pos = [pw[k] / pw[3] for k in range(3)]
        d20 = [p[2][k] - p[0][k] for k in range(3)]
        d21 = [p[2][k] - p[1][k] for k in range(3)]
        total = len3(cross3(d20, d21))
        u = len3(cross3(d21, [pos[k] - p[1][k] for k in range(3)])) / total
        v = len3(cross3([pos[k] - p[0][k] for k in range(3)], d20)) / total
        return pos, [u, v, (F(1.0) - u) - v]


def deferred_fragment_scalar(V, w, h, x, y, z, p):
    """the scalar transcription of deferred_fragment for ONE pixel; p: three positions of three float32"""
    with np.errstate(all="ignore"):
        fx, fy = F(F(x) + F(0.5)), F(F(y) + F(0.5))
        nx, ny = F(F(F(2.0) * fx) / F(w)) - F(1.0), F(F(F(2.0) * fy) / F(h)) - F(1.0)
        pv = [F(F(F(F(V.inv_proj[i] * nx) + F(V.inv_proj[4 + i] * ny)) + F(V.inv_proj[8 + i] * F(z))) + F(V.inv_proj[12 + i] * F(1.0)))
              for i in range(4)]
        pw = [F(F(F(F(V.inv_view[i] * pv[0]) + F(V.inv_view[4 + i] * pv[1])) + F(V.inv_view[8 + i] * pv[2])) + F(V.inv_view[12 + i] * pv[3]))
              for i in range(4)]
        pos = [F(pw[k] / pw[3]) for k in range(3)]
        sub = lambda a, b: [F(a[k] - b[k]) for k in range(3)]
        crs = lambda a, b: [F(F(a[1] * b[2]) - F(b[1] * a[2])), F(F(a[2] * b[0]) - F(b[2] * a[0])), F(F(a[0] * b[1]) - F(b[0] * a[1]))]
        ln = lambda a: F(np.sqrt(F(F(F(a[0] * a[0]) + F(a[1] * a[1])) + F(a[2] * a[2]))))
        d20, d21 = sub(p[2], p[0]), sub(p[2], p[1])
        total = ln(crs(d20, d21))
        u = F(ln(crs(d21, sub(pos, p[1]))) / total)
        v = F(ln(crs(sub(pos, p[0]), d20)) / total)
        return pos, [u, v, F(F(F(1.0) - u) - v)]


def shade_variant(P):
    return HELICITY if P.useHelicityBands else BANDS if P.useBands else PLAIN


def deferred_shade(words, mesh, V, case, P, ao=None):
    """The shading pass on the words (h, w): (h, w, 4) uint8 -- lv_deferred_fragment, LineAttributesBarycentric.glsl with the weights
    (u, v, 1 - u - v) (isCap, interpolateAngle, the helicity cap continuation, UNIFORM_HELICITY_BAND_WIDTH), computeFragmentColor on the
    transfer function with alpha 1, in the variant the settings select as the library does."""
    idx, verts, lpts = mesh
    idx = np.asarray(idx, dtype=np.uint32).reshape(-1, 3)
    h, w = words.shape
    prim, z = split(words)
    out = np.empty((h, w, 4), dtype=np.uint8)
    out[:] = unorm8(np.asarray(case.background, dtype=F))
    ys, xs = np.nonzero(prim != NO_PRIMITIVE)
    if len(ys) == 0:
        return out
    variant = shade_variant(P)
    tri = idx[prim[ys, xs]]
    fld = lambda arr, name, i: [np.ascontiguousarray(arr[name][i][:, k], dtype=F) for k in range(3)]
    p = [fld(verts, "vertexPosition", tri[:, i]) for i in range(3)]
    pos, wt = deferred_fragment(V, w, h, xs, ys, z[ys, xs], p)
    with np.errstate(all="ignore"):
        lerp3 = lambda a: [(a[0][k] * wt[0] + a[1][k] * wt[1]) + a[2][k] * wt[2] for k in range(3)]
        lerp1 = lambda a: (a[0] * wt[0] + a[1] * wt[1]) + a[2] * wt[2]
        li = verts["vertexLinePointIndex"][tri]
        lpi = (li & np.uint32(0x7FFFFFFF)).astype(np.int64)
        is_cap = (((li[:, 0] | li[:, 1] | li[:, 2]) >> np.uint32(31)) != 0) & bool(P.useCappedTubes)
        nrm = norm3(lerp3([fld(verts, "vertexNormal", tri[:, i]) for i in range(3)]))
        tan = norm3(lerp3([fld(lpts, "lineTangent", lpi[:, i]) for i in range(3)]))
        attr = lerp1([np.ascontiguousarray(lpts["lineAttribute"][lpi[:, i]], dtype=F) for i in range(3)])
        bands = None
        if variant != PLAIN:
            a = [np.ascontiguousarray(verts["phi"][tri[:, i]], dtype=F).copy() for i in range(3)]     # interpolateAngle
            a[0] = np.where((a[1] - a[0] > PI) | (a[2] - a[0] > PI), a[0] + F(2.0) * PI, a[0])
            a[1] = np.where((a[0] - a[1] > PI) | (a[2] - a[1] > PI), a[1] + F(2.0) * PI, a[1])
            a[2] = np.where((a[0] - a[2] > PI) | (a[1] - a[2] > PI), a[2] + F(2.0) * PI, a[2])
            bands = {"phi": lerp1(a)}
        if variant == BANDS:
            bands["linePosition"] = lerp3([fld(lpts, "linePosition", lpi[:, i]) for i in range(3)])
            bands["lineNormal"] = lerp3([fld(lpts, "lineNormal", lpi[:, i]) for i in range(3)])
        if variant == HELICITY:
            f = F(P.helicityRotationFactor)
            rot = [np.ascontiguousarray(lpts["lineRotation"][lpi[:, i]], dtype=F) for i in range(3)]
            rotation = lerp1([r * f for r in rot])
            l0 = lpi[:, 0]
            prev = np.maximum(l0 - 1, 0)
            has_prev = (l0 != 0) & (lpts["lineStartIndex"][prev] == lpts["lineStartIndex"][l0])
            other = np.where(has_prev, l0 - 1, np.minimum(l0 + 1, len(lpts) - 1))
            c0, co = fld(lpts, "linePosition", l0), fld(lpts, "linePosition", other)
            rot_o = np.ascontiguousarray(lpts["lineRotation"][other], dtype=F)
            d = [c0[k] - co[k] for k in range(3)]
            seg_len = len3(d)
            pn = [c / seg_len for c in d]
            dist = dot3(pn, pos) + (-dot3(pn, c0))
            rotation = np.where(is_cap, rotation + ((rot[0] - rot_o) * f) * dist / seg_len, rotation)
            scale = np.ones_like(rotation)
            if P.uniformHelicityBandWidth:
                rot_dy = np.where(has_prev, (rot[0] - rot_o) * f, (rot_o - rot[0]) * f)
                ang = _eval("atan2_det", rot_dy * F(0.5) * F(P.lineWidth), seg_len)[0]
                scale = _eval("sincos_rad", ang)[1]
            bands.update(rotation=rotation, separatorScale=scale)
    tf = np.array(case.tf, dtype=F).reshape(-1, 4)
    tf[:, 3] = 1.0                                   # fragmentColor.a = 1.0, RayHitCommon.glsl:130-132
    ao_texel = np.ascontiguousarray(ao[ys, xs], dtype=F) if ao is not None else np.ones(len(ys), F)
    col = compute_fragment_color(tf, P, V, pos, nrm, tan, is_cap, attr, ao_texel, variant, bands)
    out[ys, xs] = np.stack([unorm8(c) for c in col], 1)
    return out


# ---------------------------------------------------------------- an independent float64 screen-space rasteriser
def rasterise64(mesh, case, cull=True):
    """Closest front-facing triangle per pixel centre in float64 screen space (triangles with a vertex at clip w <= 0 are left out:
    the scenes of these tests stay in front of the camera).  Returns (primitive (h, w) int64, -1 = none; z (h, w); unsure (h, w) bool:
    the centre lies within 1e-4 px of a projected edge of a candidate triangle, or the two nearest depths tie)."""
    idx, verts, _ = mesh
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    W, H = case.width, case.height
    view = np.asarray(case.view, np.float64).reshape(4, 4).T
    proj = np.asarray(case.proj, np.float64).reshape(4, 4).T
    cam = np.linalg.inv(view)[:3, 3]
    vp = verts["vertexPosition"].astype(np.float64)
    clip = np.concatenate([vp, np.ones((len(vp), 1))], 1) @ (proj @ view).T
    win = np.stack([(clip[:, 0] / clip[:, 3] + 1.0) * 0.5 * W, (clip[:, 1] / clip[:, 3] + 1.0) * 0.5 * H, clip[:, 2] / clip[:, 3]], 1)
    S = win[idx]                                      # (T, 3, 3)
    g = np.cross(vp[idx[:, 1]] - vp[idx[:, 0]], vp[idx[:, 2]] - vp[idx[:, 0]])
    front = (g * (cam - vp[idx[:, 0]])).sum(1) > 0
    ok = (clip[idx, 3] > 0).all(1) & ((front | (not cull)))
    lo = np.floor(S[:, :, :2].min(1) - 0.5).astype(np.int64) - 1      # one pixel more on every side: the candidates of the margin
    hi = np.ceil(S[:, :, :2].max(1) - 0.5).astype(np.int64) + 1
    x0, y0 = np.clip(lo[:, 0], 0, W), np.clip(lo[:, 1], 0, H)
    x1, y1 = np.clip(hi[:, 0], -1, W - 1), np.clip(hi[:, 1], -1, H - 1)
    x1 = np.where(ok, x1, x0 - 1)
    tri, x, y = pairs_of(dict(x0=x0, y0=y0, x1=x1, y1=y1))
    px, py = x + 0.5, y + 0.5
    T = S[tri]
    area = lambda a, b: (b[:, 0] - a[:, 0]) * (py - a[:, 1]) - (b[:, 1] - a[:, 1]) * (px - a[:, 0])
    a = np.stack([area(T[:, 1], T[:, 2]), area(T[:, 2], T[:, 0]), area(T[:, 0], T[:, 1])], 1)
    elen = np.stack([np.linalg.norm(T[:, 2, :2] - T[:, 1, :2], axis=1), np.linalg.norm(T[:, 0, :2] - T[:, 2, :2], axis=1),
                     np.linalg.norm(T[:, 1, :2] - T[:, 0, :2], axis=1)], 1)
    with np.errstate(all="ignore"):
        dist = np.abs(a) / elen                       # distance of the centre from the edges' lines, in pixels
    A = a.sum(1)
    sgn = np.where(A >= 0, 1.0, -1.0)
    inside = ((a * sgn[:, None]) >= 0).all(1) & (A != 0)
    near_edge = (dist < 1e-4).any(1) | ~np.isfinite(dist).all(1)
    unsure = np.zeros(W * H, bool)
    unsure[(y * W + x)[near_edge]] = True
    with np.errstate(all="ignore"):
        z = (a * T[:, :, 2]).sum(1) / A
    keep = inside & (z >= 0) & (z < 1)
    pix = (y * W + x)[keep]
    zk, tk = z[keep], tri[keep]
    order = np.lexsort((tk, zk, pix))
    pix, zk, tk = pix[order], zk[order], tk[order]
    first = np.r_[True, pix[1:] != pix[:-1]]
    prim = np.full(W * H, -1, np.int64)
    zbuf = np.ones(W * H)
    prim[pix[first]] = tk[first]
    zbuf[pix[first]] = zk[first]
    second = np.r_[False, (pix[1:] == pix[:-1]) & first[:-1]]
    tie = second & (np.abs(zk - np.r_[0.0, zk[:-1]]) <= 1e-6)
    unsure[pix[tie]] = True
    return prim.reshape(H, W), zbuf.reshape(H, W), unsure.reshape(H, W)


# ---------------------------------------------------------------- the shared scene of the comparisons
LW = 0.02
_CACHE = {}


def reference_case(width=120, height=80, capped=True, **kw):
    """small_case with its tube mesh (capped = False: use_capped_tubes off and the cap triangles left out), the frame constants and
    the restated words, computed once"""
    key = (width, height, capped, tuple(sorted(kw.items())))
    if key not in _CACHE:
        case = small_case(width=width, height=height, line_width=LW, use_capped_tubes=capped, **kw)
        tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
        mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)
        if not capped:       # open tubes: without the cap triangles the inside of a tube shows at its ends
            idx, verts, lpts = mesh
            mesh = (idx[~((verts["vertexLinePointIndex"][idx] >> 31) != 0).any(axis=1)], verts, lpts)
        V = View(case)
        _CACHE[key] = (case, mesh, V, deferred_visibility(mesh, V, cull=capped))
    return _CACHE[key]


def test_vectorised_visibility_against_the_scalar_transcription():
    case, mesh, V, words = reference_case()
    S = triangle_setup(mesh, V, True)
    tri, x, y = pairs_of(S)
    cov, e = coverage(V, S, tri, x, y)
    zb = depth_bits(V, S, tri, e)
    rng = np.random.default_rng(3)
    covered = np.nonzero(cov)[0]
    sample = np.concatenate([rng.choice(len(tri), 300, replace=False), rng.choice(covered, 300, replace=False)])
    hits = 0
    for j in sample:
        want = visibility_pair(mesh, V, int(tri[j]), int(x[j]), int(y[j]))
        got = ((int(zb[j]) << 32) | int(tri[j])) if (cov[j] and zb[j] < Z_ONE) else None
        assert got == want, (j, got, want)
        hits += want is not None
    assert hits >= 300
    # a pair outside a triangle's rectangle is nothing in the scalar form either, and the winner of a pixel is the smallest key
    ys, xs = np.nonzero(split(words)[0] != NO_PRIMITIVE)
    for k in rng.choice(len(ys), 40, replace=False):
        px, py = int(xs[k]), int(ys[k])
        cand = [visibility_pair(mesh, V, int(t), px, py) for t in tri[(x == px) & (y == py)]]
        assert min(c for c in cand if c is not None) == int(words[py, px])


def test_fragment_reconstruction_against_its_scalar_transcription_and_float64():
    """the position and the barycentrics of the shading pass: vectorised = scalar; in float64 the position is the point where the
    pixel-centre ray meets the winner's plane, and (u, v, 1 - u - v) are its barycentrics there"""
    case, mesh, V, words = reference_case()
    idx, verts, _ = mesh
    prim, z = split(words)
    ys, xs = np.nonzero(prim != NO_PRIMITIVE)
    tri = np.asarray(idx).reshape(-1, 3)[prim[ys, xs]]
    p = [[np.ascontiguousarray(verts["vertexPosition"][tri[:, i], k], dtype=F) for k in range(3)] for i in range(3)]
    pos, wt = deferred_fragment(V, V.w, V.h, xs, ys, z[ys, xs], p)
    rng = np.random.default_rng(5)
    for j in rng.choice(len(ys), 200, replace=False):
        sp, sw = deferred_fragment_scalar(V, V.w, V.h, int(xs[j]), int(ys[j]), z[ys[j], xs[j]], [[c[j] for c in q] for q in p])
        assert all(a.view(np.uint32) == b[j].view(np.uint32) for a, b in zip(sp + sw, pos + wt)), j
    P3 = np.stack([np.stack(q, 1) for q in p], 1).astype(np.float64)              # (n, 3 vertices, 3)
    n = np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0])
    cam, d = V.cam.astype(np.float64), V.ray[ys, xs].astype(np.float64)
    t = ((P3[:, 0] - cam) * n).sum(1) / (d * n).sum(1)
    q = cam + t[:, None] * d
    assert np.abs(np.stack(pos, 1) - q).max() < 2e-4        # (the depth buffer's float32 z near 1 carries the error)
    bary = np.stack([(np.cross(P3[:, (i + 1) % 3] - q, P3[:, (i + 2) % 3] - q) * n).sum(1) for i in range(3)], 1) / (n * n).sum(1)[:, None]
    area = np.linalg.norm(n, axis=1)
    good = area > np.percentile(area, 20)                    # (slivers: the position's error is large against the triangle)
    assert np.abs(np.stack(wt, 1) - bary)[good].max() < 0.08 and np.median(np.abs(np.stack(wt, 1) - bary)) < 2e-3


def test_fragment_colour_restatement_against_the_checkers():
    """compute_fragment_color (plain variant) equals the checker's float32 computeFragmentColor bit for bit, with halos, caps, the AO
    mapping and depth cues; deferred_shade of the reference frame is a picture"""
    case, mesh, V, words = reference_case(depth_cue_strength=0.7, ambient_occlusion_mode="RTAO (Screen Space)",
                                          ambient_occlusion_strength=0.8, ambient_occlusion_gamma=1.5)
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    rng = np.random.default_rng(6)
    n = 4000
    pos = rng.uniform(-0.3, 0.3, (n, 3)).astype(F)
    nrm = rng.normal(size=(n, 3)).astype(F)
    tan = rng.normal(size=(n, 3)).astype(F)
    cap = rng.random(n) < 0.3
    attr = rng.uniform(-0.1, 1.1, n).astype(F)
    ao = rng.uniform(0, 1, n).astype(F)
    want, _ = sc.compute_fragment_color(P, pos, nrm, tan, cap, attr, ao)
    got = compute_fragment_color(case.tf, P, V, [pos[:, k] for k in range(3)], [nrm[:, k] for k in range(3)], [tan[:, k] for k in range(3)],
                                 cap, attr, ao)
    assert np.array_equal(np.stack(got, 1).view(np.uint32), want.view(np.uint32))
    img = deferred_shade(words, mesh, V, case, P, ao=np.full((V.h, V.w), 0.6, F))
    assert (img[..., 3] == 255).sum() > 500 and len(np.unique(img.reshape(-1, 4), axis=0)) > 200


def test_rectangles_are_conservative():
    """the coverage rule over the WHOLE viewport for every 10th triangle that is drawn: nothing is covered outside its rectangle (an
    empty rectangle: nothing at all)"""
    case, mesh, V, _ = reference_case()
    S = triangle_setup(mesh, V, True)
    ys, xs = np.mgrid[0:V.h, 0:V.w]
    checked = 0
    for t in np.nonzero(S["ok"])[0][::10]:
        cov, _ = coverage(V, S, np.full(xs.size, t), xs.ravel(), ys.ravel())
        cy, cx = ys.ravel()[cov], xs.ravel()[cov]
        assert np.all((cx >= S["x0"][t]) & (cx <= S["x1"][t]) & (cy >= S["y0"][t]) & (cy <= S["y1"][t])), t
        checked += int(cov.sum())
    assert checked > 200


def test_visibility_against_the_independent_float64_rasteriser():
    case, mesh, V, words = reference_case()
    prim, z = split(words)
    p64, z64, unsure = rasterise64(mesh, case)
    covered = p64 >= 0
    assert covered.sum() > 1500 and unsure.sum() < 0.02 * covered.sum()
    sure = ~unsure
    assert np.array_equal(np.where(prim == NO_PRIMITIVE, -1, prim.astype(np.int64))[sure], p64[sure])
    assert np.abs(z[sure & covered].astype(np.float64) - z64[sure & covered]).max() < 2e-6


def brute_force_primitives(mesh, V, trace):
    """closest hits of the pixel-centre rays: trace(o, d) -> (t, triangle, uv)"""
    o = np.tile(V.cam, (V.w * V.h, 1))
    return trace(o, V.ray.reshape(-1, 3))[1].reshape(V.h, V.w)


def compare_with_rays(words, hit_tri, unsure):
    """the share of covered pixels left out (edge margin, depth ties) and the disagreements among the others"""
    prim, _ = split(words)
    covered = (prim != NO_PRIMITIVE) | (hit_tri != NO_PRIMITIVE)
    sure = covered & ~unsure
    return float((covered & unsure).sum()) / float(covered.sum()), int((prim[sure] != hit_tri[sure]).sum()), int(covered.sum())


def test_visibility_against_brute_force_closest_hits():
    case, mesh, V, words = reference_case()
    ts = lvo.TriScene(*mesh, LW)
    hit = brute_force_primitives(mesh, V, lambda o, d: ts.trace_rays(o, d, 0.0, 1000.0, use_bvh=False))
    _, _, unsure = rasterise64(mesh, case)
    share, wrong, covered = compare_with_rays(words, hit, unsure)
    assert covered > 1500
    assert share <= 0.01, share          # the cap of the excluded pixels
    assert wrong == 0


# ---------------------------------------------------------------- edge cases on hand-made meshes
def hand_mesh(positions, triangles):
    verts = np.zeros(len(positions), dtype=lvo.TUBE_VERTEX_DTYPE)
    verts["vertexPosition"] = np.asarray(positions, dtype=F)
    verts["vertexNormal"][:, 2] = 1.0
    lp = np.zeros(1, dtype=lvo.LINE_POINT_DTYPE)
    lp["lineTangent"][:, 1] = 1.0
    return np.asarray(triangles, dtype=np.uint32).reshape(-1, 3), verts, lp


def hand_case(w=33, h=33, eye=(0.0, 0.0, 1.0)):
    c = small_case(width=w, height=h, n_lines=2, pts_per_line=4)
    c.view, c.proj = camera.look_at(eye, (0.0, 0.0, 0.0)), camera.perspective(c.fovy, float(w) / float(h), c.near, c.far)
    return c


class RuleView:
    """Frame constants in which the rules' arithmetic is exact: camera at the origin, right axis x, coverage direction of pixel (x, y) =
    ((x - 16) / 64, (y - 16) / 64, -1).  With vertices on the grid of 1 / 128 at z = -1 every product and sum of the coverage test
    is exact in float32, so an edge function is 0.0 exactly where the pixel's ray meets the edge."""

    def __init__(self, w=33, h=33):
        self.w, self.h = w, h
        self.cam = np.zeros(3, F)
        self.right = np.array([1.0, 0.0, 0.0], F)
        ys, xs = np.mgrid[0:h, 0:w]
        self.cov = np.stack([(xs - 16) / 64.0, (ys - 16) / 64.0, -np.ones((h, w))], -1).astype(F)
        self.view = np.eye(4, dtype=F).reshape(16)
        self.proj = np.diag([1.0, 1.0, -0.5, 1.0]).astype(F).reshape(16)      # clip w = 1, clip z = 0.5: in front, between the planes


def rule_coverage(positions, triangles, cull):
    """coverage counts (h, w), pixels with an edge function of exactly 0, and the facing of the triangles over the whole RuleView"""
    V = RuleView()
    mesh = hand_mesh(positions, triangles)
    S = triangle_setup(mesh, V, cull)
    for k, v in (("x0", 0), ("y0", 0), ("y1", V.h - 1)):
        S[k][:] = v
    S["x1"] = np.where(S["ok"], V.w - 1, -1)
    tri, x, y = pairs_of(S)
    cov, e = coverage(V, S, tri, x, y)
    count = np.zeros((V.h, V.w), int)
    np.add.at(count, (y[cov], x[cov]), 1)
    on_edge = np.zeros((V.h, V.w), bool)
    on_edge[y[cov], x[cov]] |= np.stack(e, 1)[cov].min(1) == 0
    return count, on_edge, S["flip"]


def test_watertight_fan_through_pixel_centres():
    """A fan around a hub between four pixel centres whose spokes run along the diagonals, exactly through the centres of the pixels
    (16 + k, 16 + k), (16 - k, 17 + k), ...: every pixel of the fan is covered exactly once, those on the spokes too -- by the triangle
    that runs through the spoke with ascending vertex index -- and `>=` on every edge would count them twice, `>` never."""
    g = lambda x, y: (x / 64.0, y / 64.0, -1.0)
    pos = [g(0.5, 0.5), g(8.5, 8.5), g(-7.5, 8.5), g(-7.5, -7.5), g(8.5, -7.5)]
    tris = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1)]
    for winding in (tris, [t[::-1] for t in tris]):
        count, on_edge, flip = rule_coverage(pos, winding, cull=False)
        assert flip.all() or not flip.any()
        spoke = np.zeros((33, 33), bool)
        for k in range(1, 8):
            spoke[16 + k, 16 + k] = spoke[17 + k - 1, 16 - k + 1] = spoke[16 - k + 1, 16 - k + 1] = spoke[16 - k + 1, 17 + k - 1] = True
        inside = np.zeros((33, 33), bool)
        inside[10:24, 10:24] = True                       # well inside the square (-7.5 ... 8.5) + 16
        assert np.all(count[inside] == 1)
        assert on_edge[spoke & inside].all() and (spoke & inside).sum() >= 20
        assert not on_edge[inside & ~spoke].any()
        assert set(np.unique(count)) <= {0, 1}
    # back faces are culled iff asked to: exactly one of the two windings is drawn
    drawn = [rule_coverage(pos, w, cull=True)[0].sum() for w in (tris, [t[::-1] for t in tris])]
    assert sorted(drawn)[0] == 0 and sorted(drawn)[1] > 100


def test_equal_depths_go_to_the_lower_primitive_index():
    case = hand_case()
    V = View(case)
    quad = [(-0.2, -0.2, 0), (0.2, -0.2, 0), (0.2, 0.2, 0), (-0.2, 0.2, 0)]
    mesh = hand_mesh(quad + quad, [(4, 5, 6), (0, 1, 2), (0, 2, 3), (4, 6, 7)])    # each triangle twice, at the same depth
    prim, _ = split(deferred_visibility(mesh, V))
    assert set(np.unique(prim)) == {0, 2, int(NO_PRIMITIVE)}


def test_depth_rule_keeps_zero_and_refuses_one_and_the_sign_bit():
    """the keep rule on the bits: +0 is kept, 1.0 and everything above, -0, negative values and NaN are refused"""
    zb = np.array([0.0, 1e-45, 0.5, np.nextafter(F(1.0), F(0.0)), 1.0, 2.0, np.inf, -0.0, -1e-3, np.nan], dtype=F).view(np.uint32)
    assert list(zb < Z_ONE) == [True, True, True, True, False, False, False, False, False, False]
    # and through the pass: a triangle in the near plane's neighbourhood / beyond the far plane
    case = hand_case()
    V = View(case)
    tri = lambda z: hand_mesh([(-0.05, -0.05, z), (0.05, -0.05, z), (0.0, 0.05, z)], [(0, 1, 2)])
    near_z, far_z = 1.0 - case.near, 1.0 - case.far
    assert (split(deferred_visibility(tri(near_z - 0.05), V))[0] != NO_PRIMITIVE).any()
    assert (split(deferred_visibility(tri(near_z + 0.005), V))[0] == NO_PRIMITIVE).all()     # in front of the near plane: z < 0
    assert (split(deferred_visibility(tri(far_z - 1.0), V))[0] == NO_PRIMITIVE).all()        # beyond the far plane: z >= 1


def test_triangle_across_the_near_plane_covers_only_its_part_beyond_it():
    """A long triangle from in front of the camera to behind it (a vertex at clip w < 0: the rectangle is the viewport): the pixels it
    wins are those of the float64 statement -- the ray meets the triangle's plane inside it and between the planes."""
    case = hand_case(w=41, h=31)
    V = View(case)
    pos = [(-0.3, -0.25, -0.5), (0.3, -0.25, -0.5), (0.0, -0.05, 1.5)]      # the camera sits at z = 1
    mesh = hand_mesh(pos, [(0, 1, 2)])
    S = triangle_setup(mesh, V, False)
    assert S["x0"][0] == 0 and S["x1"][0] == 40 and S["y0"][0] == 0 and S["y1"][0] == 30
    prim, z = split(deferred_visibility(mesh, V, cull=False))
    got = prim != NO_PRIMITIVE
    P3 = np.asarray(pos, np.float64)
    n = np.cross(P3[1] - P3[0], P3[2] - P3[0])
    cam = V.cam.astype(np.float64)
    view = np.asarray(case.view, np.float64).reshape(4, 4).T
    proj = np.asarray(case.proj, np.float64).reshape(4, 4).T
    want = np.zeros_like(got)
    margin = np.zeros_like(got)
    for yy in range(31):
        for xx in range(41):
            d = V.ray[yy, xx].astype(np.float64)
            t = ((P3[0] - cam) @ n) / (d @ n)
            q = cam + t * d
            b = np.array([np.cross(P3[(i + 1) % 3] - q, P3[(i + 2) % 3] - q) @ n for i in range(3)]) / (n @ n)
            c = proj @ view @ np.r_[q, 1.0]
            zz = c[2] / c[3]
            want[yy, xx] = t > 0 and b.min() >= 0 and 0 <= zz < 1
            margin[yy, xx] = abs(b).min() < 1e-6 or abs(zz) < 1e-6
    assert want.sum() > 20 and (~want).sum() > 20
    assert np.array_equal(got[~margin], want[~margin])
    assert (z[got] >= 0).all() and (z[got] < 1).all()
