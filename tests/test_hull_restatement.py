"""The simulation-mesh hull fragment (linevis_amd/csrc/lv_hull.h; include/linevis_hip.h, hull_opacity) restated in float32 numpy: one
operation at a time, left to right, no contraction.

Coverage and depth are mode 1's rules with culling off: triangle_setup, pairs_of, coverage and depth_bits of
test_deferred_restatement.py, called with cull=False on a structured array with a vertexPosition field.  hull_shade() restates
MeshHull.glsl:77-90 with blinnPhongShading of Lighting.glsl:45-92 under MESH_HULL on the host's build-owned functions (the shading
code's normalize, lvo.pow_det).  hull_fragments() is the vectorised statement, hull_pair() its scalar transcription.
frame_references() folds the hull fragments with the oracle's line fragments through wboit_fold, al64_fold and
depth_complexity_frame: the reference frames tests/test_gpu_hull.py compares the device with.

Here, without a GPU: the vectorised form against the scalar one; against an independent float64 screen-space rasteriser; the
closed box seen from outside (0 or 2 fragments per pixel) and from inside (exactly 1); a fan that is watertight across a front /
back pair; the alpha's un-normalised normal; the folds."""
import functools

import numpy as np

from common import small_case
from linevis_amd import camera, scenes
from oracle import lvo
from test_atomic_loop_restatement import al64_fold, al64_key
from test_deferred_restatement import (F, Z_ONE, View, clampf, coverage, cross3, depth_bits, dot3, norm_shade, pairs_of,
                                       triangle_setup, visibility_pair)
from test_depth_peeling_restatement import depth_complexity_frame
from test_mlab_restatement import pack, window_depth
from test_wboit_restatement import wboit_fold

# struct HullTriangleVertexData, LineRenderData.hpp:186-191 (lv_hull_vertex)
HULL_VERTEX_DTYPE = np.dtype([("vertexPosition", "<f4", 3), ("padding0", "<f4"), ("vertexNormal", "<f4", 3), ("padding1", "<f4")])
assert HULL_VERTEX_DTYPE.itemsize == 32
# the linear value of sRGB 0.5 by the standard piecewise formula, in double, as float32 (include/linevis_hip.h, hull_color)
DEFAULT_COLOR = (float(np.float32(((0.5 + 0.055) / 1.055) ** 2.4)),) * 3
DEFAULT_OPACITY = 0.3


def hull_arrays(hull):
    """the mesh as triangle_setup takes it: (indices, vertices with a vertexPosition field, nothing)"""
    verts = np.zeros(len(hull.positions), dtype=HULL_VERTEX_DTYPE)
    verts["vertexPosition"] = np.asarray(hull.positions, dtype=F)
    verts["vertexNormal"] = np.asarray(hull.normals, dtype=F)
    return np.asarray(hull.triangle_indices, dtype=np.uint32).reshape(-1, 3), verts, None


def hull_shade(V, pos, nrm, opacity=DEFAULT_OPACITY, color=DEFAULT_COLOR, use_shading=True, use_bands=False, normalised_alpha=False):
    """lv_hull_shade on lists of three float32 arrays: four float32 arrays.  normalised_alpha: the ray tracer's hit shader's alpha
    (it normalises the normal first) -- NOT what the raster shader and this build do; here for the test that tells them apart."""
    with np.errstate(all="ignore"):
        v = norm_shade([V.cam[k] - pos[k] for k in range(3)])
        col = [F(c) for c in color]
        rgb = [np.full_like(pos[0], c) for c in col]
        if use_shading:
            kA, kD, kS, s = F(0.1), F(0.9 if use_bands else 1.0), F(0.3), F(30.0 if use_bands else 50.0)
            n = norm_shade(nrm)
            h = norm_shade([v[k] + v[k] for k in range(3)])
            diffuse = kD * clampf(np.abs(dot3(n, v)), 0.0, 1.0)
            Is = (kS * lvo.pow_det(clampf(np.abs(dot3(n, h)), 0.0, 1.0), s)) * F(1.0)
            rgb = [(kA * c + diffuse * c) + Is for c in col]
        cos_angle = dot3(norm_shade(nrm) if normalised_alpha else nrm, v)
        cos_angle = np.where(cos_angle < 0, cos_angle * F(-1.0), cos_angle)
        return [np.asarray(c, dtype=F) for c in rgb] + [F(opacity) * (F(1.0) - cos_angle)]


def hull_fragments(hull, V, requested=None, **shade):
    """Every kept hull fragment of the viewport: dict of pixel (y * w + x), tri, zbits (uint32), rgba (n, 4) float32, pos, nrm -- sorted
    by (pixel, triangle)."""
    mesh = hull_arrays(hull)
    idx, verts, _ = mesh
    S = triangle_setup(mesh, V, False)
    tri, x, y = pairs_of(S)
    cov, e = coverage(V, S, tri, x, y)
    tri, x, y, e = tri[cov], x[cov], y[cov], [a[cov] for a in e]
    zb = depth_bits(V, S, tri, e)
    keep = zb < Z_ONE                                # 0 <= z < 1
    if requested is not None:
        keep &= requested[y, x]
    tri, x, y, e, zb = tri[keep], x[keep], y[keep], [a[keep] for a in e], zb[keep]
    with np.errstate(all="ignore"):
        rs = F(1.0) / ((e[0] + e[1]) + e[2])
        b = [a * rs for a in e]
        mix = lambda a: [(b[0] * a[0][:, k] + b[1] * a[1][:, k]) + b[2] * a[2][:, k] for k in range(3)]
        pos = mix([S["pos"][i][tri] for i in range(3)])
        nrm = mix([np.ascontiguousarray(verts["vertexNormal"][idx[tri, i]], dtype=F) for i in range(3)])
    rgba = np.stack(hull_shade(V, pos, nrm, **shade), 1).astype(F) if len(tri) else np.zeros((0, 4), F)
    pixel = (y * V.w + x).astype(np.uint32)
    order = np.lexsort((tri, pixel))
    return dict(pixel=pixel[order], tri=tri[order].astype(np.uint32), zbits=zb[order], rgba=rgba[order],
                pos=np.stack(pos, 1)[order] if len(tri) else np.zeros((0, 3), F),
                nrm=np.stack(nrm, 1)[order] if len(tri) else np.zeros((0, 3), F))


def hull_pair(hull, V, tri, x, y, opacity=DEFAULT_OPACITY, color=DEFAULT_COLOR, use_shading=True, use_bands=False):
    """The scalar transcription for ONE (triangle, pixel): (zbits, [r, g, b, a]) or None.  Coverage and depth: visibility_pair with
    culling off; then lv_hull_fragment's weights and lv_hull_shade, every operation rounded to float32 by hand."""
    mesh = hull_arrays(hull)
    idx, verts, _ = mesh
    key = visibility_pair(mesh, V, tri, x, y, cull=False)
    if key is None:
        return None
    ids = [int(i) for i in idx[tri]]
    P = [[F(c) for c in verts["vertexPosition"][i]] for i in ids]
    N = [[F(c) for c in verts["vertexNormal"][i]] for i in ids]
    mul, add, sub = (lambda a, b: F(F(a) * F(b))), (lambda a, b: F(F(a) + F(b))), (lambda a, b: F(F(a) - F(b)))
    dot = lambda a, b: add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))
    crs = lambda a, b: [sub(mul(a[1], b[2]), mul(b[1], a[2])), sub(mul(a[2], b[0]), mul(b[2], a[0])), sub(mul(a[0], b[1]), mul(b[0], a[1]))]
    cam = [F(c) for c in V.cam]
    A = [[sub(p[k], cam[k]) for k in range(3)] for p in P]
    D = [F(c) for c in V.cov[y, x]]
    Pb = crs([F(c) for c in V.right], D)
    Qb = crs(D, Pb)
    X, Y = [dot(a, Pb) for a in A], [dot(a, Qb) for a in A]
    e = [sub(mul(Y[1], X[2]), mul(X[1], Y[2])), sub(mul(Y[2], X[0]), mul(X[2], Y[0])), sub(mul(Y[0], X[1]), mul(X[0], Y[1]))]
    det = dot(A[0], crs([sub(A[1][k], A[0][k]) for k in range(3)], [sub(A[2][k], A[0][k]) for k in range(3)]))
    if det > 0:
        e = [F(-a) for a in e]
    with np.errstate(all="ignore"):
        rs = F(F(1.0) / add(add(e[0], e[1]), e[2]))
        b = [mul(a, rs) for a in e]
        mix = lambda a: [add(add(mul(b[0], a[0][k]), mul(b[1], a[1][k])), mul(b[2], a[2][k])) for k in range(3)]
        pos, nrm = mix(P), mix(N)

        def normalize(a):
            r = F(F(1.0) / F(np.sqrt(F(min(max(dot(a, a), F(2.0 ** -60)), F(2.0 ** 60))))))
            return [mul(c, r) for c in a]

        clamp01 = lambda t: F(min(max(F(t), F(0.0)), F(1.0)))
        v = normalize([sub(cam[k], pos[k]) for k in range(3)])
        rgb = [F(c) for c in color]
        if use_shading:
            kA, kD, kS, s = F(0.1), F(0.9 if use_bands else 1.0), F(0.3), F(30.0 if use_bands else 50.0)
            n = normalize(nrm)
            h = normalize([add(v[k], v[k]) for k in range(3)])
            diffuse = mul(kD, clamp01(abs(dot(n, v))))
            Is = mul(mul(kS, lvo.pow_det(clamp01(abs(dot(n, h))), s)[0]), F(1.0))
            rgb = [add(add(mul(kA, c), mul(diffuse, c)), Is) for c in rgb]
        cos_angle = dot(nrm, v)
        if cos_angle < 0:
            cos_angle = mul(cos_angle, F(-1.0))
        alpha = mul(F(opacity), sub(F(1.0), cos_angle))
    return key >> 32, rgb + [alpha]


# ---------------------------------------------------------------- the fixtures
LW = 0.02


def bent_strip():
    """an open strip of 8 triangles bent round the y axis: seen from +z one half shows its front, the other its back"""
    ang = np.radians([-80.0, -35.0, 0.0, 35.0, 80.0])
    # a "V"-like arc whose right half folds back towards the camera, so that its other side faces the viewer
    xs = 0.22 * np.sin(ang) - np.where(ang > 0, 0.3 * (1 - np.cos(ang)), 0.0)
    zs = 0.22 * np.cos(ang) - 0.1
    pos = np.array([(xs[i], yy, zs[i]) for i in range(5) for yy in (-0.17, 0.19)], dtype=np.float32)
    tris = []
    for i in range(4):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        tris += [(a, c, b), (b, c, d)]
    idx = np.asarray(tris, dtype=np.uint32)
    return scenes.HullMesh(idx, pos, scenes.compute_smooth_triangle_normals(idx, pos))


@functools.lru_cache(maxsize=None)
def hull_case(kind="outside"):
    """(case, hull, View) of the comparisons, computed once:
    outside   box_hull with n = 3 (108 triangles) around small_case's lines at 120 x 80, the camera outside the box
    odd       the same at 257 x 131
    inside    the camera inside the box at 96 x 64, in the manner of _closeup of tests/test_gpu_deferred.py: next to a wall and
              looking along it, so that triangles with vertices at clip w <= 0 occur and win pixels
    strip     the open, bent strip"""
    w, h = {"outside": (120, 80), "odd": (257, 131), "inside": (96, 64), "strip": (120, 80)}[kind]
    # (off the box's axes: seen head-on, the diagonals of the front face's quads run exactly through pixel centres, which the fill rule
    # decides but the float64 comparison has to leave out)
    c = small_case(width=w, height=h, line_width=LW, transparent=True, camera_pos=(0.21, 0.13, 0.8))
    pts = c.points["linePosition"]
    hull = bent_strip() if kind == "strip" else scenes.box_hull((pts.min(0), pts.max(0)), 3, 0.05)
    if kind == "inside":
        c.view = camera.look_at((0.28, 0.02, 0.05), (0.25, 0.0, -0.3))
    return c, hull, View(c)


@functools.lru_cache(maxsize=None)
def reference_fragments(kind="outside", use_shading=True):
    c, hull, V = hull_case(kind)
    return hull_fragments(hull, V, use_shading=use_shading)


def line_fragments(c):
    """the oracle's prism fragments of the case's lines: (offsets, rgba (n, 4), window depth (n,))"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P)
    off = fr["offsets"].astype(np.int64)
    n = int(off[-1])
    rgba = np.asarray(fr["rgba"], dtype=F).reshape(-1, 4)[:n]
    return off, rgba, window_depth(np.asarray(fr["pos"], dtype=F)[:n], c.view, c.proj)


def hull_runs(fr, num_pixels):
    """the hull fragments' offsets per pixel (they are sorted by pixel)"""
    off = np.zeros(num_pixels + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(fr["pixel"], minlength=num_pixels))
    return off


def al64_keys(rgba, z):
    return al64_key(z, pack([rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]]))


def union_runs(c, fr, hull_rgba=None):
    """per pixel: the line fragments, then the hull fragments -- (rgba, z) runs for wboit_fold, key runs past the 0.001 discard for
    al64_fold (hull_rgba: other colours for the hull's fragments, e.g. the device's own), the counts of mode 5"""
    num = c.width * c.height
    off, rgba, z = line_fragments(c)
    hoff = hull_runs(fr, num)
    hrgba = np.asarray(fr["rgba"] if hull_rgba is None else hull_rgba, dtype=F)
    hz = fr["zbits"].view(F)
    lkey, hkey = al64_keys(rgba, z), al64_keys(hrgba, hz)
    lkeep, hkeep = rgba[:, 3] >= F(0.001), hrgba[:, 3] >= F(0.001)
    wb, al = [], []
    for p in range(num):
        a, b, ha, hb = off[p], off[p + 1], hoff[p], hoff[p + 1]
        wb.append((np.concatenate([rgba[a:b], hrgba[ha:hb]]), np.concatenate([z[a:b], hz[ha:hb]])))
        al.append(np.concatenate([lkey[a:b][lkeep[a:b]], hkey[ha:hb][hkeep[ha:hb]]]))
    counts = (np.diff(off) + np.diff(hoff)).astype(np.uint32)
    return wb, al, counts


def frame_references(c, fr, K=8, weight="reference", hull_rgba=None):
    """The frames of modes 8, 10 and 5 with the hull: dict of wboit (frame, sums, counts), al64 (frame, slots, tail, counts past the
    discard), dc (frame, counts)"""
    wb, al, counts = union_runs(c, fr, hull_rgba)
    shape = (c.height, c.width)
    wf, ws = wboit_fold(wb, c.background, weight, details=True)
    af, slots, tail = al64_fold(al, K, c.background)
    return dict(wboit=(wf.reshape(shape + (4,)), ws.reshape(shape + (5,)), counts.reshape(shape)),
                al64=(af.reshape(shape + (4,)), slots.reshape(shape + (K,)), tail.reshape(shape + (5,)),
                      np.array([len(r) for r in al], np.uint32).reshape(shape)),
                dc=(depth_complexity_frame(counts, c.background).reshape(shape + (4,)), counts.reshape(shape)))


# ---------------------------------------------------------------- an independent float64 screen-space rasteriser, every fragment
def rasterise64_all(hull, case):
    """Every triangle covering every pixel centre in float64 screen space, both facings (triangles with a vertex at clip w <= 0 are left
    out: for cameras that keep the mesh in front of them).  Returns (pixel, tri, z) sorted by (pixel, tri) and unsure (h * w) bool:
    the centre lies within 1e-4 px of a projected edge of a candidate triangle (the rule of tests/test_prism_raster.py)."""
    idx = np.asarray(hull.triangle_indices, dtype=np.int64).reshape(-1, 3)
    W, H = case.width, case.height
    view = np.asarray(case.view, np.float64).reshape(4, 4).T
    proj = np.asarray(case.proj, np.float64).reshape(4, 4).T
    vp = np.asarray(hull.positions, np.float64)
    clip = np.concatenate([vp, np.ones((len(vp), 1))], 1) @ (proj @ view).T
    win = np.stack([(clip[:, 0] / clip[:, 3] + 1.0) * 0.5 * W, (clip[:, 1] / clip[:, 3] + 1.0) * 0.5 * H, clip[:, 2] / clip[:, 3]], 1)
    S = win[idx]
    ok = (clip[idx, 3] > 0).all(1)
    lo = np.floor(S[:, :, :2].min(1) - 0.5).astype(np.int64) - 1
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
        dist = np.abs(a) / elen
        A = a.sum(1)
        sgn = np.where(A >= 0, 1.0, -1.0)
        inside = ((a * sgn[:, None]) >= 0).all(1) & (A != 0)
        z = (a * T[:, :, 2]).sum(1) / A
    near_edge = (dist < 1e-4).any(1) | ~np.isfinite(dist).all(1)
    unsure = np.zeros(W * H, bool)
    unsure[(y * W + x)[near_edge]] = True
    keep = inside & (z >= 0) & (z < 1)
    pix, tk, zk = (y * W + x)[keep], tri[keep], z[keep]
    order = np.lexsort((tk, pix))
    return pix[order], tk[order], zk[order], unsure


# ---------------------------------------------------------------- the checks
def test_vectorised_statement_against_the_scalar_transcription():
    for kind, shading in (("outside", True), ("strip", False), ("inside", True)):
        c, hull, V = hull_case(kind)
        fr = reference_fragments(kind, shading)
        assert len(fr["pixel"]) > 1000
        rng = np.random.default_rng(11)
        for j in rng.choice(len(fr["pixel"]), 120, replace=False):
            p, t = int(fr["pixel"][j]), int(fr["tri"][j])
            got = hull_pair(hull, V, t, p % V.w, p // V.w, use_shading=shading)
            assert got is not None and got[0] == int(fr["zbits"][j]), (kind, j)
            assert [a.view(np.uint32) for a in got[1]] == [a.view(np.uint32) for a in fr["rgba"][j]], (kind, j)
        # pairs that are no fragment are none in the scalar form either
        have = set(zip(fr["pixel"].tolist(), fr["tri"].tolist()))
        misses = 0
        for _ in range(150):
            t, x, y = int(rng.integers(len(hull.triangle_indices))), int(rng.integers(V.w)), int(rng.integers(V.h))
            if (y * V.w + x, t) not in have:
                assert hull_pair(hull, V, t, x, y, use_shading=shading) is None
                misses += 1
        assert misses > 50
    # USE_BANDS selects the other constants
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    banded = hull_fragments(hull, V, use_bands=True)
    assert np.array_equal(banded["zbits"], fr["zbits"]) and not np.array_equal(banded["rgba"][:, :3], fr["rgba"][:, :3])
    assert np.array_equal(banded["rgba"][:, 3].view(np.uint32), fr["rgba"][:, 3].view(np.uint32))
    j = len(fr["pixel"]) // 2
    p, t = int(banded["pixel"][j]), int(banded["tri"][j])
    got = hull_pair(hull, V, t, p % V.w, p // V.w, use_bands=True)
    assert [a.view(np.uint32) for a in got[1]] == [a.view(np.uint32) for a in banded["rgba"][j]]


def test_against_the_independent_float64_rasteriser():
    for kind in ("outside", "odd", "strip"):
        c, hull, V = hull_case(kind)
        fr = reference_fragments(kind)
        pix, tri, z, unsure = rasterise64_all(hull, c)
        covered = np.zeros(V.w * V.h, bool)
        covered[pix] = True
        covered[fr["pixel"]] = True
        assert covered.sum() > (500 if kind == "strip" else 2000)
        share = float((covered & unsure).sum()) / float(covered.sum())
        assert share <= 0.01, (kind, share)           # the cap of the excluded pixels (tests/test_gpu_deferred.py)
        s32, s64 = ~unsure[fr["pixel"]], ~unsure[pix]
        assert np.array_equal(fr["pixel"][s32], pix[s64]) and np.array_equal(fr["tri"][s32], tri[s64]), kind
        assert np.abs(fr["zbits"].view(F)[s32].astype(np.float64) - z[s64]).max() < 2e-6
    # both facings are drawn: the strip shows front faces and back faces
    c, hull, V = hull_case("strip")
    S = triangle_setup(hull_arrays(hull), V, False)
    seen = np.unique(reference_fragments("strip")["tri"])
    assert S["flip"][seen].any() and (~S["flip"][seen]).any() and len(seen) == 8


def _counts_and_exact_edges(kind):
    """fragments per pixel, and the pixels with an edge function of exactly 0 in a triangle whose rectangle holds them"""
    c, hull, V = hull_case(kind)
    S = triangle_setup(hull_arrays(hull), V, False)
    tri, x, y = pairs_of(S)
    _, e = coverage(V, S, tri, x, y)
    on_edge = np.zeros(V.w * V.h, bool)
    on_edge[(y * V.w + x)[np.stack(e, 1).min(1) == 0] if len(tri) else []] = True
    on_edge[(y * V.w + x)[(np.stack(e, 1) == 0).any(1)]] = True
    return np.bincount(reference_fragments(kind)["pixel"], minlength=V.w * V.h), on_edge, S


def test_closed_box_from_outside_has_zero_or_two_fragments_per_pixel():
    for kind in ("outside", "odd"):
        counts, on_edge, S = _counts_and_exact_edges(kind)
        assert not S["any_behind"].any()
        assert set(np.unique(counts[~on_edge])) == {0, 2}
        assert (counts == 2).sum() > 2000
    # (the fill rule keeps that on the edges too: a shared edge belongs to exactly one of its two triangles)
        assert set(np.unique(counts)) <= {0, 2}


def test_closed_box_from_inside_has_exactly_one_fragment_per_pixel():
    counts, on_edge, S = _counts_and_exact_edges("inside")
    fr = reference_fragments("inside")
    behind = S["any_behind"]
    assert behind.sum() >= 4 and behind[np.unique(fr["tri"])].sum() >= 2      # vertices with clip w <= 0 occur, and win pixels
    assert np.all(counts[~on_edge] == 1) and (~on_edge).sum() > 0.99 * counts.size
    assert np.all(counts == 1)


def test_fan_is_watertight_across_a_front_back_pair():
    """The fan of test_deferred_restatement.py whose spokes run exactly through pixel centres, every other triangle wound the other
    way round: front faces and back faces alternate, and every pixel of the fan is still covered exactly once -- a drawn back face runs
    through its edges the other way round, so a spoke between a front and a back face has one owner."""
    from test_deferred_restatement import rule_coverage
    g = lambda x, y: (x / 64.0, y / 64.0, -1.0)
    pos = [g(0.5, 0.5), g(8.5, 8.5), g(-7.5, 8.5), g(-7.5, -7.5), g(8.5, -7.5)]
    for tris in ([(0, 1, 2), (0, 3, 2), (0, 3, 4), (0, 1, 4)], [(0, 2, 1), (0, 2, 3), (0, 4, 3), (0, 4, 1)]):
        count, on_edge, flip = rule_coverage(pos, tris, cull=False)
        assert flip.sum() == 2 and list(flip[::2]) != list(flip[1::2])
        inside = np.zeros((33, 33), bool)
        inside[10:24, 10:24] = True
        assert np.all(count[inside] == 1) and on_edge[inside].sum() >= 20
        assert set(np.unique(count)) <= {0, 1}


def test_edge_on_triangle_covers_nothing():
    """A hand mesh: a triangle in the plane y = 0 through the camera at (0, 0, 1) has det == 0 exactly and covers nothing; its
    neighbour is drawn"""
    from test_deferred_restatement import hand_case
    pos = np.array([(-0.125, 0.0, 0.0), (0.125, 0.0, 0.0), (0.0, 0.0, -0.5), (0.0, 0.125, 0.0)], dtype=np.float32)
    idx = np.array([(0, 1, 2), (0, 1, 3)], dtype=np.uint32)
    hull = scenes.HullMesh(idx, pos, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4, 1)))
    V = View(hand_case())
    S = triangle_setup(hull_arrays(hull), V, False)
    assert S["det"][0] == 0 and not S["ok"][0] and S["ok"][1]
    fr = hull_fragments(hull, V)
    assert len(fr["tri"]) > 10 and set(fr["tri"]) == {1}


def test_alpha_takes_the_unnormalised_normal():
    """The smooth normals of the box differ from vertex to vertex near its edges, so the interpolated normal is visibly shorter than
    1 there: alpha = opacity * (1 - |n . v|) with it is NOT the alpha of the normalised normal (the ray tracer's hit shader)."""
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    ln = np.linalg.norm(fr["nrm"].astype(np.float64), axis=1)
    short = ln < 0.9
    assert short.sum() > 500 and ln.max() <= 1.0 + 1e-6
    pos, nrm = [fr["pos"][:, k] for k in range(3)], [fr["nrm"][:, k] for k in range(3)]
    raster = hull_shade(V, pos, nrm)[3]
    tracer = hull_shade(V, pos, nrm, normalised_alpha=True)[3]
    assert np.array_equal(raster.view(np.uint32), fr["rgba"][:, 3].view(np.uint32))
    facing = short & (np.abs(1.0 - tracer / F(DEFAULT_OPACITY)) > 0.2)      # (where |n . v| is not small anyway)
    assert facing.sum() > 300
    assert np.all(raster[facing] - tracer[facing] > 1e-3)    # a shorter normal: a smaller cosine, a larger alpha
    # and the definition in float64
    v = V.cam.astype(np.float64) - fr["pos"].astype(np.float64)
    v /= np.linalg.norm(v, axis=1)[:, None]
    want = DEFAULT_OPACITY * (1.0 - np.abs((fr["nrm"].astype(np.float64) * v).sum(1)))
    assert np.abs(raster - want).max() < 1e-6


def test_default_colour_is_the_linear_value_of_srgb_half():
    assert np.float32(DEFAULT_COLOR[0]).view(np.uint32) == 0x3E5B2D9A and abs(DEFAULT_COLOR[0] - 0.21404114048223255) < 1e-8


def test_hull_fragments_fold_with_the_line_fragments():
    """the reference frames of the GPU tests: the union of the oracle's line fragments and the hull's through the three folds"""
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    with_hull = frame_references(c, fr, K=8)
    empty = {k: v[:0] for k, v in fr.items()}
    without = frame_references(c, empty, K=8)
    hull_counts = np.bincount(fr["pixel"], minlength=V.w * V.h).reshape(V.h, V.w)
    assert np.array_equal(with_hull["dc"][1] - without["dc"][1], hull_counts)
    assert np.array_equal(with_hull["wboit"][2], with_hull["dc"][1])
    # mode 10 keeps what passes the 0.001 discard; the hull's fragments are among the slots
    past = np.bincount(fr["pixel"][fr["rgba"][:, 3] >= F(0.001)], minlength=V.w * V.h).reshape(V.h, V.w)
    assert np.array_equal(with_hull["al64"][3] - without["al64"][3], past) and past.sum() > 2000
    for mode in ("wboit", "al64", "dc"):
        changed = (with_hull[mode][0] != without[mode][0]).any(axis=2)
        assert changed.sum() > 1500 and not changed[hull_counts == 0].any(), mode
    # with K = 2 hull fragments reach the tail
    deep = frame_references(c, fr, K=2)
    assert (deep["al64"][2][..., 0] != 0).sum() > 200
