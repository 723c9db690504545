"""The simulation-mesh hull in the ray tracer (linevis_amd/csrc/lv_hull_rt.h; include/linevis_hip.h, hull_ray_tracing) restated in
float32 numpy: one operation at a time, left to right, no contraction.

ray_triangle() is lv_ray_triangle on broadcast arrays, closest_hull_hit() the brute force over a mesh (closed interval [tMin, tMax],
ties to the lowest triangle index, pad = hull_pad(mesh): maxAbs * 1e-5 + 1e-6, a property of the mesh alone), hull_hit_shade()
ClosestHitHull (TubeRayTracing.glsl:397-431) on hull_shade(..., normalised_alpha=True) of test_hull_restatement.py, primary_rays() the
ray generator with its jitter, fold_step() / hull_only_loop() traceRayTransparent (:61-82) where only the hull is hit.
tests/test_gpu_hull_rt.py compares the device with these.

Here, without a GPU: the per-triangle test against the oracle's lvo.intersect_triangle bit for bit; the brute force's interval and
tie rules; the shading against a scalar transcription and its geometry; the hull-only loop on the closed box; the defaults."""
import os
import re
import types

import numpy as np

from linevis_amd import scenes
from oracle import lvo
from test_deferred_restatement import F, View, cross3, dot3, len3, mul_m4, norm3
from test_hull_restatement import DEFAULT_COLOR, DEFAULT_OPACITY, bent_strip, hull_arrays, hull_case, hull_shade
from test_mlab_restatement import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MIN, T_MAX = F(0.0001), F(1000.0)
HIT_DISTANCE_EPSILON = F(1e-5)
MISS = np.uint32(0xFFFFFFFF)
HULL_FLAG = np.uint32(0x80000000)
BACKGROUND = (1.0, 1.0, 1.0, 1.0)


# ---------------------------------------------------------------- H: the closest hull hit
def hull_pad(hull):
    """hullPad: from the largest absolute coordinate of the mesh, never from the line width"""
    return F(F(np.abs(np.asarray(hull.positions, dtype=F)).max() * F(1e-5)) + F(1e-6))


def ray_triangle(o, d, v0, v1, v2, pad):
    """lv_ray_triangle (lv_trace.h) on lists of three broadcastable float32 arrays: (hit, t, u, v).  Moeller-Trumbore without culling, then
    t inside the ray interval of the triangle's own AABB padded by `pad`."""
    pad = F(pad)
    with np.errstate(all="ignore"):
        e1 = [v1[k] - v0[k] for k in range(3)]
        e2 = [v2[k] - v0[k] for k in range(3)]
        p = cross3(d, e2)
        det = dot3(e1, p)
        r = F(1.0) / det
        tv = [o[k] - v0[k] for k in range(3)]
        u = dot3(tv, p) * r
        q = cross3(tv, e1)
        v = dot3(d, q) * r
        t = dot3(e2, q) * r
        hit = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1)
        lo, hi = [], []
        for k in range(3):
            mn = np.fmin(np.fmin(v0[k], v1[k]), v2[k]) - pad
            mx = np.fmax(np.fmax(v0[k], v1[k]), v2[k]) + pad
            inv = F(1.0) / d[k]
            a, b = (mn - o[k]) * inv, (mx - o[k]) * inv
            lo.append(np.fmin(a, b))
            hi.append(np.fmax(a, b))
        tn = np.fmax(np.fmax(lo[0], lo[1]), lo[2])
        tf = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
        hit = hit & (t >= tn) & (t <= tf)
    return hit, t, u, v


def closest_hull_hit(hull, o, d, t_min, t_max, chunk=2048):
    """H of lv_hull_rt.h for n rays (o, d: (n, 3); t_min, t_max: scalars or (n,)): (t or t_max, triangle or 0xFFFFFFFF, uv (n, 2))"""
    idx, verts, _ = hull_arrays(hull)
    pad = hull_pad(hull)
    P = [np.ascontiguousarray(verts["vertexPosition"][idx[:, i]], dtype=F) for i in range(3)]
    o = np.asarray(o, dtype=F).reshape(-1, 3)
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    n = len(o)
    lo = np.broadcast_to(np.asarray(t_min, dtype=F), (n,))
    hi = np.broadcast_to(np.asarray(t_max, dtype=F), (n,))
    out_t, out_tri, out_uv = hi.copy(), np.full(n, MISS), np.zeros((n, 2), F)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        oo = [o[s:e, k, None] for k in range(3)]
        dd = [d[s:e, k, None] for k in range(3)]
        hit, t, u, v = ray_triangle(oo, dd, *[[p[None, :, k] for k in range(3)] for p in P], pad)
        hit = hit & (t >= lo[s:e, None]) & (t <= hi[s:e, None])
        key = np.where(hit, t, F(np.inf))
        best = key.argmin(1)                       # the first minimum: ties go to the lowest triangle index
        rows = np.arange(e - s)
        found = hit[rows, best]
        out_t[s:e] = np.where(found, t[rows, best], hi[s:e])
        out_tri[s:e] = np.where(found, best.astype(np.uint32), MISS)
        out_uv[s:e, 0] = np.where(found, u[rows, best], F(0.0))
        out_uv[s:e, 1] = np.where(found, v[rows, best], F(0.0))
    return out_t, out_tri, out_uv


# ---------------------------------------------------------------- ClosestHitHull
def hull_hit_shade(hull, cam, tri, uv, opacity=DEFAULT_OPACITY, color=DEFAULT_COLOR, use_shading=True, use_bands=False):
    """lv_hull_rt_hit for hits (tri (n,), uv (n, 2)): (rgba (n, 4) straight colour, payload.hitT (n,))"""
    idx, verts, _ = hull_arrays(hull)
    tri = np.asarray(tri, dtype=np.int64)
    u, v = np.asarray(uv, dtype=F)[:, 0], np.asarray(uv, dtype=F)[:, 1]
    b = [(F(1.0) - u) - v, u, v]
    mix = lambda field: [(b[0] * field[0][:, k] + b[1] * field[1][:, k]) + b[2] * field[2][:, k] for k in range(3)]
    pos = mix([np.ascontiguousarray(verts["vertexPosition"][idx[tri, i]], dtype=F) for i in range(3)])
    nrm = mix([np.ascontiguousarray(verts["vertexNormal"][idx[tri, i]], dtype=F) for i in range(3)])
    V = types.SimpleNamespace(cam=np.asarray(cam, dtype=F))
    rgba = hull_shade(V, pos, nrm, opacity=opacity, color=color, use_shading=use_shading, use_bands=use_bands, normalised_alpha=True)
    with np.errstate(all="ignore"):
        hit_t = len3([pos[k] - V.cam[k] for k in range(3)])
    return np.stack([np.broadcast_to(c, u.shape) for c in rgba], 1).astype(F), np.asarray(hit_t, dtype=F)


# ---------------------------------------------------------------- the ray generator and the loop
def primary_rays(V, xs, ys, frame_number=0, num_samples=1, sample=0, jittered=False):
    """lv_primary_ray for pixels (xs, ys): (origin (3,), directions (n, 3)); jittered: the per-pixel seed tea(x + y * w, frame * spp + s)"""
    xs, ys = np.asarray(xs, dtype=np.int64).ravel(), np.asarray(ys, dtype=np.int64).ravel()
    xi = np.full((len(xs), 2), 0.5, dtype=F)
    if jittered:
        for i, (x, y) in enumerate(zip(xs, ys)):
            xi[i] = lvo.rnd_sequence(lvo.tea(int(x + y * V.w), frame_number * num_samples + sample), 2)
    ndcx = F(2.0) * ((xs.astype(F) + xi[:, 0]) / F(V.w)) - F(1.0)
    ndcy = F(2.0) * ((ys.astype(F) + xi[:, 1]) / F(V.h)) - F(1.0)
    one = np.ones_like(ndcx)
    target = mul_m4(V.inv_proj, ndcx, ndcy, one, one)
    tn = norm3(target[:3])
    d = mul_m4(V.inv_view, tn[0], tn[1], tn[2], F(0.0) * one)
    return V.cam.copy(), np.stack(d[:3], 1).astype(F)


def next_t_min(hit_t):
    hit_t = np.asarray(hit_t, dtype=F)
    return hit_t + np.fmax(hit_t * HIT_DISTANCE_EPSILON, F(1e-7))


def fold_step(fc, rgba):
    """one blend of traceRayTransparent on (n, 4) arrays: the new (n, 4)"""
    a = (F(1.0) - fc[:, 3]) * rgba[:, 3]
    return np.stack([fc[:, 0] + a * rgba[:, 0], fc[:, 1] + a * rgba[:, 1], fc[:, 2] + a * rgba[:, 2], fc[:, 3] + a], 1).astype(F)


def fold_records(rec, num_pixels, background=BACKGROUND, max_depth=1024, num_samples=1, jittered=False, state=None):
    """the frame's float colours (num_pixels, 4) from (n, 9) hit records alone: per pixel and sample the recorded hits in hitIdx order,
    then the miss unless the loop ended on alpha > 0.99 or at max_depth; samples summed in order and divided when jittered.  Asserts
    that no step follows one that ended the loop.  state: a list that receives (missed (num_pixels,) bool, steps (num_pixels,)) per
    sample -- the rays whose loop ended with the miss shader"""
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 9)
    pix, sample, step = rec[:, 0].astype(np.int64), (rec[:, 1] >> 16).astype(np.int64), (rec[:, 1] & 0xFFFF).astype(np.int64)
    rgba = np.ascontiguousarray(rec[:, 5:9]).view(F)
    bg = np.asarray(background, dtype=F)
    acc = np.zeros((num_pixels, 4), F)
    for s in range(num_samples):
        fc = np.zeros((num_pixels, 4), F)
        count = np.zeros(num_pixels, np.int64)
        sel = sample == s
        for k in range(int(step[sel].max()) + 1 if sel.any() else 0):
            m = sel & (step == k)
            p = pix[m]
            assert len(np.unique(p)) == len(p) and (count[p] == k).all(), "a pixel's steps are numbered 0, 1, 2, ... without gaps"
            assert (fc[p, 3] <= F(0.99)).all() and k < max_depth, "a step after the loop's end"
            fc[p] = fold_step(fc[p], rgba[m])
            count[p] += 1
        miss = (fc[:, 3] <= F(0.99)) & (count < max_depth)
        fc[miss] = fold_step(fc[miss], np.broadcast_to(bg, (int(miss.sum()), 4)))
        if state is not None:
            state.append((miss, count))
        acc = acc + fc
    if jittered:
        acc = acc / F(num_samples)
    return acc


def frame_of(colours, w, h):
    """lv_store_color without accumulation: (h, w, 4) uint8"""
    return pack([colours[:, k] for k in range(4)]).view(np.uint8).reshape(h, w, 4)


def hull_only_loop(hull, V, background=BACKGROUND, max_depth=1024, **shade):
    """traceRayTransparent of every pixel-centre ray where the hull is the only geometry: (records (n, 9) uint32 sorted by (pixel, hitIdx),
    float colours (w * h, 4))"""
    ys, xs = np.mgrid[0:V.h, 0:V.w]
    o, d = primary_rays(V, xs, ys)
    n = V.w * V.h
    oo = np.broadcast_to(o, (n, 3))
    fc = np.zeros((n, 4), F)
    t_min = np.full(n, T_MIN)
    active = np.arange(n)
    records = []
    bg = np.asarray(background, dtype=F)
    for step in range(max_depth):
        if len(active) == 0:
            break
        t, tri, uv = closest_hull_hit(hull, oo[active], d[active], t_min[active], T_MAX)
        found = tri != MISS
        rgba = np.broadcast_to(bg, (len(active), 4)).astype(F).copy()
        hit_t = np.zeros(len(active), F)
        if found.any():
            rgba[found], hit_t[found] = hull_hit_shade(hull, V.cam, tri[found], uv[found], **shade)
            r = np.zeros((int(found.sum()), 9), np.uint32)
            r[:, 0], r[:, 1], r[:, 2] = active[found], step, HULL_FLAG | tri[found]
            r[:, 3], r[:, 4] = t[found].view(np.uint32), hit_t[found].view(np.uint32)
            r[:, 5:9] = rgba[found].view(np.uint32)
            records.append(r)
        t_min[active] = next_t_min(hit_t)
        fc[active] = fold_step(fc[active], rgba)
        active = active[found & (fc[active, 3] <= F(0.99))]
    rec = np.concatenate(records) if records else np.zeros((0, 9), np.uint32)
    return rec[np.lexsort((rec[:, 1], rec[:, 0]))], fc


def sort_records(rec):
    """records in (pixel, sample, hitIdx) order"""
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 9)
    return rec[np.lexsort((rec[:, 1], rec[:, 0]))]


# ---------------------------------------------------------------- the fixtures of the GPU comparison
def one_triangle():
    pos = np.array([(-0.3, -0.2, 0.1), (0.35, -0.25, -0.1), (0.05, 0.3, 0.0)], dtype=np.float32)
    idx = np.array([(0, 1, 2)], dtype=np.uint32)
    return scenes.HullMesh(idx, pos, scenes.compute_smooth_triangle_normals(idx, pos))


def two_triangles():
    """two triangles that share an edge and overlap along the viewing direction near it (a fold)"""
    pos = np.array([(-0.3, -0.2, 0.1), (0.35, -0.25, -0.1), (0.05, 0.3, 0.0), (0.1, -0.3, 0.25)], dtype=np.float32)
    idx = np.array([(0, 1, 2), (1, 0, 3)], dtype=np.uint32)
    return scenes.HullMesh(idx, pos, scenes.compute_smooth_triangle_normals(idx, pos))


def ray_triangle_pairs():
    """(o, d, v0, v1, v2), each (n, 3): seeded rays against seeded triangles, with rays aimed at vertices and edges (grazing), rays
    inside a triangle's plane, axis-parallel directions with +0 and -0 components and degenerate triangles among them"""
    rng = np.random.default_rng(0x48554C4C)
    n = 2400
    tri = rng.uniform(-0.5, 0.5, (n, 3, 3)).astype(F)
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    w = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
    target = np.einsum("ni,nik->nk", w, tri).astype(F)
    kind = np.arange(n) % 8
    target[kind == 1] = tri[kind == 1, 0]                                   # through a vertex
    target[kind == 2] = (F(0.5) * tri[kind == 2, 0] + F(0.5) * tri[kind == 2, 1]).astype(F)   # through an edge
    target[kind == 3] = rng.uniform(-0.6, 0.6, ((kind == 3).sum(), 3)).astype(F)              # anywhere: mostly misses
    d = (target - o).astype(F)
    ax = kind == 4                                                          # axis-parallel, +0 and -0 in the other components
    axis = rng.integers(0, 3, n)
    for i in np.nonzero(ax)[0]:
        o[i] = target[i]
        o[i, axis[i]] = F(1.5)
        d[i] = np.where(np.arange(3) == axis[i], F(-1.0), F(0.0) if i % 16 < 8 else F(-0.0))
    inplane = kind == 5                                                     # the origin in the triangle's plane
    o[inplane] = (tri[inplane, 0] + F(2.0) * (tri[inplane, 1] - tri[inplane, 0]) + F(1.5) * (tri[inplane, 2] - tri[inplane, 0])).astype(F)
    d[inplane] = (target[inplane] - o[inplane]).astype(F)
    tri[kind == 6, 2] = tri[kind == 6, 1]                                   # degenerate: det == 0
    return o, d, tri[:, 0].copy(), tri[:, 1].copy(), tri[:, 2].copy()


# ---------------------------------------------------------------- the tests
def test_ray_triangle_equals_the_oracle_bit_for_bit():
    o, d, v0, v1, v2 = ray_triangle_pairs()
    assert len(o) >= 2000
    hits = 0
    for pad in (F(1e-6), F(6e-6)):
        hit, t, u, v = ray_triangle(*[[a[:, k] for k in range(3)] for a in (o, d, v0, v1, v2)], pad)
        for i in range(len(o)):
            want = lvo.intersect_triangle(o[i], d[i], v0[i], v1[i], v2[i], float(pad))
            assert bool(hit[i]) == want[0], i
            if want[0]:
                got = np.array([t[i], u[i], v[i]], F).view(np.uint32)
                assert np.array_equal(got, np.array(want[1:], F).view(np.uint32)), i
        hits += int(hit.sum())
    kinds = np.arange(len(o)) % 8
    hit = ray_triangle(*[[a[:, k] for k in range(3)] for a in (o, d, v0, v1, v2)], F(1e-6))[0]
    assert hit[kinds == 0].mean() > 0.9 and hit[kinds == 4].sum() > 100 and not hit[kinds == 6].any() and hits > 2000


def test_closest_hit_interval_and_ties():
    # two coincident triangles and one behind them: the lowest index wins the tie; the interval is closed at both ends
    pos = np.array([(-1, -1, 0), (1, -1, 0), (0, 1, 0), (-1, -1, -0.5), (1, -1, -0.5), (0, 1, -0.5)], dtype=np.float32)
    idx = np.array([(3, 4, 5), (0, 1, 2), (0, 1, 2)], dtype=np.uint32)
    hull = scenes.HullMesh(idx, pos, scenes.compute_smooth_triangle_normals(idx, pos))
    o, d = np.array([[0.0, -0.2, 1.0]], F), np.array([[0.0, 0.0, -1.0]], F)
    t, tri, uv = closest_hull_hit(hull, o, d, T_MIN, T_MAX)
    assert (float(t[0]), int(tri[0])) == (1.0, 1)
    assert int(closest_hull_hit(hull, o, d, F(1.0), T_MAX)[1][0]) == 1            # t == tMin is inside
    assert int(closest_hull_hit(hull, o, d, T_MIN, F(1.0))[1][0]) == 1            # t == tMax is inside
    assert int(closest_hull_hit(hull, o, d, np.nextafter(F(1.0), F(2.0)), T_MAX)[1][0]) == 0
    t, tri, uv = closest_hull_hit(hull, o, d, T_MIN, F(0.5))
    assert (float(t[0]), tri[0]) == (0.5, MISS) and not uv.any()
    # the brute force equals the oracle's test triangle by triangle on a real mesh
    c, box, V = hull_case("outside")
    ys, xs = np.mgrid[7:V.h:13, 5:V.w:11]
    o, dirs = primary_rays(V, xs, ys)
    t, tri, uv = closest_hull_hit(box, np.broadcast_to(o, dirs.shape), dirs, T_MIN, T_MAX)
    idx, verts, _ = hull_arrays(box)
    pad = float(hull_pad(box))
    for i in range(len(dirs)):
        best = (None, MISS)
        for k in range(len(idx)):
            h = lvo.intersect_triangle(o, dirs[i], *[verts["vertexPosition"][idx[k, j]] for j in range(3)], pad)
            if h[0] and T_MIN <= F(h[1]) <= T_MAX and (best[0] is None or F(h[1]) < best[0]):
                best = (F(h[1]), np.uint32(k))
        assert best[1] == tri[i] and (best[0] is None or best[0] == t[i]), i
    assert (tri != MISS).sum() > 20


def test_pad_depends_on_the_mesh_alone():
    c, box, V = hull_case("outside")
    m = np.abs(np.asarray(box.positions, dtype=np.float64)).max()
    assert abs(float(hull_pad(box)) - (m * 1e-5 + 1e-6)) < 1e-9
    big = scenes.HullMesh(box.triangle_indices, box.positions * np.float32(100.0), box.normals)
    assert hull_pad(big) > F(50.0) * hull_pad(box)


def test_pixel_centre_rays_are_the_generators():
    c, box, V = hull_case("outside")
    ys, xs = np.mgrid[0:V.h, 0:V.w]
    o, d = primary_rays(V, xs, ys)
    assert np.array_equal(d.view(np.uint32), V.ray.reshape(-1, 3).view(np.uint32)) and np.array_equal(o, V.cam)
    oj, dj = primary_rays(V, xs[:3, :5], ys[:3, :5], num_samples=2, sample=1, jittered=True)
    assert (dj != d.reshape(V.h, V.w, 3)[:3, :5].reshape(-1, 3)).any(1).all()
    # a jittered ray stays inside its pixel's frustum: between the rays of the neighbouring pixel centres
    assert np.abs(dj - d.reshape(V.h, V.w, 3)[:3, :5].reshape(-1, 3)).max() < 2.5 * np.abs(np.diff(d.reshape(V.h, V.w, 3), axis=1)).max()


def test_shading_against_the_scalar_transcription():
    c, box, V = hull_case("outside")
    rng = np.random.default_rng(5)
    tri = rng.integers(0, len(box.triangle_indices), 64)
    uv = rng.dirichlet((1, 1, 1), 64)[:, :2].astype(F)
    idx, verts, _ = hull_arrays(box)
    mul, add, sub = (lambda a, b: F(F(a) * F(b))), (lambda a, b: F(F(a) + F(b))), (lambda a, b: F(F(a) - F(b)))
    dot = lambda a, b: add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))

    def normalize(a):
        r = F(F(1.0) / F(np.sqrt(F(min(max(dot(a, a), F(2.0 ** -60)), F(2.0 ** 60))))))
        return [mul(x, r) for x in a]

    for shading, bands in ((True, False), (True, True), (False, False)):
        rgba, hit_t = hull_hit_shade(box, V.cam, tri, uv, opacity=0.45, color=(0.8, 0.3, 0.1), use_shading=shading, use_bands=bands)
        for i in range(len(tri)):
            P = [[F(x) for x in verts["vertexPosition"][idx[tri[i], j]]] for j in range(3)]
            N = [[F(x) for x in verts["vertexNormal"][idx[tri[i], j]]] for j in range(3)]
            b = [sub(sub(F(1.0), uv[i, 0]), uv[i, 1]), uv[i, 0], uv[i, 1]]
            mixv = lambda a: [add(add(mul(b[0], a[0][k]), mul(b[1], a[1][k])), mul(b[2], a[2][k])) for k in range(3)]
            pos, nrm = mixv(P), mixv(N)
            cam = [F(x) for x in V.cam]
            v = normalize([sub(cam[k], pos[k]) for k in range(3)])
            n = normalize(nrm)
            rgb = [F(0.8), F(0.3), F(0.1)]
            if shading:
                kA, kD, kS, s = F(0.1), F(0.9 if bands else 1.0), F(0.3), F(30.0 if bands else 50.0)
                h = normalize([add(v[k], v[k]) for k in range(3)])
                clamp01 = lambda t: F(min(max(F(t), F(0.0)), F(1.0)))
                diffuse = mul(kD, clamp01(abs(dot(n, v))))
                Is = mul(mul(kS, lvo.pow_det(clamp01(abs(dot(n, h))), s)[0]), F(1.0))
                rgb = [add(add(mul(kA, x), mul(diffuse, x)), Is) for x in rgb]
            cos_angle = dot(n, v)
            if cos_angle < 0:
                cos_angle = mul(cos_angle, F(-1.0))
            want = rgb + [mul(F(0.45), sub(F(1.0), cos_angle))]
            dp = [sub(pos[k], cam[k]) for k in range(3)]
            want_t = F(np.sqrt(dot(dp, dp)))
            assert np.array_equal(rgba[i].view(np.uint32), np.array(want, F).view(np.uint32)), (shading, bands, i)
            assert hit_t[i] == want_t
    # geometry: the interpolated position lies on the ray of a real hit, and hitT is its distance from the camera
    ys, xs = np.mgrid[3:V.h:9, 2:V.w:7]
    o, d = primary_rays(V, xs, ys)
    t, tri, uv = closest_hull_hit(box, np.broadcast_to(o, d.shape), d, T_MIN, T_MAX)
    f = tri != MISS
    rgba, hit_t = hull_hit_shade(box, V.cam, tri[f], uv[f])
    along = t[f].astype(np.float64) * np.linalg.norm(d[f].astype(np.float64), axis=1)
    assert f.sum() > 30 and np.abs(along - hit_t).max() < 1e-5
    assert (rgba[:, 3] >= 0).all() and (rgba[:, 3] <= F(DEFAULT_OPACITY)).all()


def test_hull_only_loop_on_the_closed_box():
    c, box, V = hull_case("outside")
    rec, fc = hull_only_loop(box, V)
    per_pixel = np.bincount(rec[:, 0].astype(np.int64), minlength=V.w * V.h)
    assert set(np.unique(per_pixel)) <= {0, 2} and (per_pixel == 2).sum() > 5000        # a closed box: in and out
    t = rec[:, 3].view(F)
    first, second = rec[rec[:, 1] == 0], rec[rec[:, 1] == 1]
    assert np.array_equal(first[:, 0], second[:, 0]) and (first[:, 3].view(F) < second[:, 3].view(F)).all()
    assert (rec[:, 2] & HULL_FLAG).all() and (t > 0).all()
    # the second step starts behind the first hit
    assert (second[:, 3].view(F) >= next_t_min(first[:, 4].view(F))).all()
    # the fold of the records alone is the loop's colour; pixels without a hit are the background
    again = fold_records(rec, V.w * V.h)
    assert np.array_equal(again.view(np.uint32), fc.view(np.uint32))
    frame = frame_of(fc, V.w, V.h)
    assert (frame[(per_pixel == 0).reshape(V.h, V.w)] == 255).all() and (frame[(per_pixel == 2).reshape(V.h, V.w)][:, :3] < 255).any()
    # from inside the box every pixel has exactly one hit; the open strip has 0, 1 or 2
    ci, boxi, Vi = hull_case("inside")
    reci, _ = hull_only_loop(boxi, Vi)
    assert np.array_equal(np.bincount(reci[:, 0].astype(np.int64), minlength=Vi.w * Vi.h), np.ones(Vi.w * Vi.h, np.int64))
    cs, strip, Vs = hull_case("strip")
    recs, _ = hull_only_loop(strip, Vs)
    assert set(np.unique(np.bincount(recs[:, 0].astype(np.int64), minlength=Vs.w * Vs.h))) == {0, 1, 2}
    # hull_opacity 0.3 never ends a loop on alpha > 0.99: every ray reaches the opaque background, which is blended last
    assert np.isfinite(fc).all() and (fc[:, 3] > F(0.99)).all()


def test_default_state_and_interface():
    header = open(os.path.join(ROOT, "include", "linevis_hip.h")).read()
    assert re.search(r"\bint\s+lv_trace_rays_hull\s*\(", header) and re.search(r"\bint\s+lv_rt_get_hits\s*\(", header)
    assert re.search(r"hull_ray_tracing[^\n]*\"off\" \(default", header) and "rt_record_hits" in header
    from linevis_amd import capi
    assert callable(capi.Context.trace_rays_hull) and callable(capi.Context.rt_hits)
    assert "lv_trace_rays_hull" in capi.SYMBOLS and "lv_rt_get_hits" in capi.SYMBOLS
    internal = open(os.path.join(ROOT, "linevis_amd", "csrc", "lv_internal.h")).read()
    assert re.search(r"bool\s+hullRayTracing\s*=\s*false\s*;", internal) and re.search(r"bool\s+rtRecordHits\s*=\s*false\s*;", internal)
    api = open(os.path.join(ROOT, "linevis_amd", "csrc", "lv_api.hip")).read()
    assert '"hull_ray_tracing"' in api and '"rt_record_hits"' in api
    assert "lv_hull_rt.hip" in open(os.path.join(ROOT, "linevis_amd", "build.py")).read()
