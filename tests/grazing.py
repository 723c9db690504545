"""Grazing rays for the culling tests (test_culling_grazing.py, test_gpu_culling_grazing.py): rays that pass within a small
fraction of the radius of a face of a primitive's bounding box, where a slab test with too small a margin culls a box whose
primitive the ray hits.  A random ray almost never comes within 1e-5 of a box face; these all do.  Also the scenes and the
(translation, line width) configurations both test files run, and the box rule of the builders as a float32 statement.

A helper module, not a test.  Everything is generated in float64 and handed out as float32."""
import functools

import numpy as np

from common import scene_arrays
from linevis_amd import scenes, transfer_function as tfm
from oracle import lvo

T_MIN, T_MAX = 0.0, 1000.0
N_RAYS = 40000
MISS = 0xFFFFFFFF

# (name, float32 translation, scale about the origin, line width after the scale)
CONFIGS = [
    ("unit_w0.02", (0.0, 0.0, 0.0), 1.0, 0.02),              # control
    ("unit_w0.002", (0.0, 0.0, 0.0), 1.0, 0.002),            # control
    ("t30_w0.0004", (30.0, 30.0, -30.0), 1.0, 0.0004),
    ("t100_w0.002", (100.0, -100.0, 100.0), 1.0, 0.002),
    ("t1000_w0.02", (1000.0, 1000.0, -1000.0), 1.0, 0.02),
    ("x256_w5.12", (0.0, 0.0, 0.0), 256.0, 5.12),            # control: the pad grows with the radius
]
CONFIG_IDS = [c[0] for c in CONFIGS]


def _aim(rng, P, k, sigma, eps, distances):
    """Rays through P - sigma * eps * e_k: direction = a random unit vector of the plane perpendicular to e_k plus a k component
    of +-10^U(-7, -2), normalised; origin = target - D * direction, D drawn from `distances`."""
    n = len(P)
    i = np.arange(n)
    target = P.copy()
    target[i, k] -= sigma * eps
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    d = np.zeros((n, 3))
    d[i, (k + 1) % 3] = np.cos(phi)
    d[i, (k + 2) % 3] = np.sin(phi)
    d[i, k] = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7.0, -2.0, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    D = rng.choice(np.asarray(distances, dtype=np.float64), n)
    o = target - D[:, None] * d
    return o.astype(np.float32), d.astype(np.float32)


def grazing_rays(positions, seg, radius, n, seed, distances=(0.5, 8.0, 128.0)):
    """(o, d, target_segment): per ray a segment s, an axis k and a sign sigma, all uniform.  e = the endpoint of s with the larger
    sigma * x_k, P = e + sigma * radius * e_k = the capsule's extreme point on that face of its box; the ray is aimed
    eps = radius * 10^U(-6, -2) inside of P along the axis."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    s = rng.integers(0, len(seg), n)
    k = rng.integers(0, 3, n)
    sigma = rng.choice([-1.0, 1.0], n)
    i = np.arange(n)
    a, b = pos[seg[s, 0]], pos[seg[s, 1]]
    e = np.where((sigma * a[i, k] >= sigma * b[i, k])[:, None], a, b)
    P = e.copy()
    P[i, k] += sigma * radius
    eps = radius * 10.0 ** rng.uniform(-6.0, -2.0, n)
    o, d = _aim(rng, P, k, sigma, eps, distances)
    return o, d, s.astype(np.uint32)


def grazing_rays_at_vertices(vertices, radius, n, seed, distances=(0.5, 8.0, 128.0)):
    """(o, d, target_vertex): the same with P a mesh vertex (an extreme point of the boxes of its triangles) and eps measured inward
    along -sigma * e_k."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    s = rng.integers(0, len(v), n)
    k = rng.integers(0, 3, n)
    sigma = rng.choice([-1.0, 1.0], n)
    eps = radius * 10.0 ** rng.uniform(-6.0, -2.0, n)
    o, d = _aim(rng, v[s].copy(), k, sigma, eps, distances)
    return o, d, s.astype(np.uint32)


def _move(xyz, translation, scale):
    """float32: scale about the origin (a power of two: exact), then the translation (rounds every coordinate)."""
    return (xyz * np.float32(scale) + np.asarray(translation, dtype=np.float32)).astype(np.float32)


def _unit_width(scale, line_width):
    return float(np.float32(line_width) / np.float32(scale))


def capsule_scene(config, n_lines=30, points_per_line=30, seed=7):
    """(points, seg, line_width): the normalised random curves (30 x 30: 870 segments) through the a2 restatement, then moved."""
    _, translation, scale, line_width = config
    tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=points_per_line, seed=seed))
    pts, seg = scene_arrays(tr, _unit_width(scale, line_width))
    pts["linePosition"] = _move(pts["linePosition"], translation, scale)
    return pts, seg, float(np.float32(line_width))


def few_segments(config, n):
    """The first n segments of the first line of the capsule scene: n = 1 is the single-node build, n = 2 the smallest collapsed node."""
    pts, seg, line_width = capsule_scene(config)
    return pts[:n + 1].copy(), seg[:n].copy(), line_width


def triangle_scene(config, n_lines=10, points_per_line=12, subdiv=6, seed=7):
    """(mesh = (indices, vertices, line points), line_width): the 6-gon tubes of 10 x 12 points, tessellated in the unit box and moved."""
    _, translation, scale, line_width = config
    tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=points_per_line, seed=seed))
    idx, verts, pts = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets,
                                                          _unit_width(scale, line_width), subdiv)
    verts["vertexPosition"] = _move(verts["vertexPosition"], translation, scale)
    pts["linePosition"] = _move(pts["linePosition"], translation, scale)
    return (idx, verts, pts), float(np.float32(line_width))


def radius_in_ulps(xyz, radius):
    """radius / ulp(largest |coordinate|): the supported range of the numerics contract is >= 64."""
    return float(np.float32(radius) / np.spacing(np.abs(np.asarray(xyz, dtype=np.float32)).max()))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the box rule of the builders, float32
REL_PAD = np.float32(2.0 ** -21)


def pad_of(radius):
    return np.float32(np.float32(radius) * np.float32(1e-3) + np.float32(1e-6))


def widen(lo0, hi0, pad):
    """lo = lo0 - max(pad, |lo0| * 2^-21), hi = hi0 + max(pad, |hi0| * 2^-21): every operation rounds to float32."""
    lo0, hi0 = np.asarray(lo0, dtype=np.float32), np.asarray(hi0, dtype=np.float32)
    return (lo0 - np.maximum(pad, np.abs(lo0) * REL_PAD)).astype(np.float32), (hi0 + np.maximum(pad, np.abs(hi0) * REL_PAD)).astype(np.float32)


def segment_boxes(positions, seg, radius):
    """Rule boxes of the capsules: lo0 = min(p0, p1) - radius, hi0 = max(p0, p1) + radius, then widen()."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    a, b = p[seg[:, 0]], p[seg[:, 1]]
    r = np.float32(radius)
    return widen(np.minimum(a, b) - r, np.maximum(a, b) + r, pad_of(radius))


# ---------------------------------------------------------------- scenes, rays and brute-force hits, computed once per session
@functools.lru_cache(maxsize=None)
def capsule_case(name, n_segments=0, literal=True):
    """(scene, line width, rays, brute-force hits) of one configuration, computed once and shared; n_segments = 1 / 2: the small scenes.
    literal: the reference's textbook roots with the own-box rule (the library's default form) or the closest-approach form."""
    lvo.set_default_intersection_form(literal)
    config = CONFIGS[CONFIG_IDS.index(name)]
    pts, seg, lw = few_segments(config, n_segments) if n_segments else capsule_scene(config)
    o, d, target = grazing_rays(pts["linePosition"], seg, lw * 0.5, N_RAYS, seed=1000 + n_segments)
    sc = lvo.Scene(pts, seg, tfm.standard())
    want = sc.trace_rays(o, d, T_MIN, T_MAX, lw, use_bvh=False)
    return sc, pts, seg, lw, o, d, target, want


@functools.lru_cache(maxsize=None)
def triangle_case(name):
    config = CONFIGS[CONFIG_IDS.index(name)]
    mesh, lw = triangle_scene(config)
    o, d, target = grazing_rays_at_vertices(mesh[1]["vertexPosition"], lw * 0.5, N_RAYS, seed=2000)
    ts = lvo.TriScene(*mesh, lw)
    want = ts.trace_rays(o, d, T_MIN, T_MAX, use_bvh=False)
    return ts, mesh, lw, o, d, target, want
