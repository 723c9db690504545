"""The leaf test of the 64-byte triangle pair records (lv_leaf_test, lv_ray_triangle in lv_trace.h) at the shapes where it can go
wrong: both triangles of a tube face, (q0, q1, q2) and (q0, q2, q3), share a vertex and the diagonal; cap quads, pole fans and an
empty second slot fetch their second triangle again by address; the closest hit inside the caller's interval wins and a tie stays with
the lower index.  The library is built without the SLP vectoriser (linevis_amd/build.py), so the cross and dot products of the test
are plain float32 operations; these cases pin down that what they compute did not move.

Nothing that decides a hit may change its operands or their order, so every result is compared bit for bit with brute force over all
triangles -- the CPU oracle's render_ao / trace_rays with use_bvh=False, as in tests/test_gpu_leaf_fetch.py -- and there is no
tolerance to choose.

Scenes: one two-segment tube (12 body pairs, the cap quads and the pole fans of both ends in one tree) and one three-vertex line bent
by about 140 degrees, whose legs occlude each other; a hand-made mesh of quads on dyadic coordinates, where a ray through the shared
diagonal or through a vertex gives both triangles of a pair exactly the same t (the tie stays with the lower index), with a face whose
first and one whose second triangle has no area (det == 0 for every ray), rays inside a face's plane (det == 0 by direction), a face
on coordinates 0 and -0, and axis-parallel rays (1 / d = +-inf in the own-box rule).  Launches of 1, 63, 64, 65 and 129 rays; closest
hit and any hit; the AO G-buffer kernel (k_ao_primary) on a 64 x 64 frame; a shuffled mesh that keeps 48-byte records."""
import numpy as np
import pytest

from common import Case, scene_arrays
from linevis_amd import scenes, transfer_function as tfm
from oracle import lvo
from test_gpu_ao_stint_cycle import LW, Setup, bits, check_hit_count

pytestmark = pytest.mark.gpu

T_MIN, T_MAX = 1e-4, 1000.0
BODY, CAP_QUAD, FAN, EMPTY = 0x38, 0x2D, 0x1C, 0x3F   # LV_TRI_PAIR_CODE_BODY and the other codes of lv_tri_pair_code (lv_bvh.hip)
LINES = {"two_segments": [(-0.4, -0.1, 0.0), (0.0, 0.0, 0.0), (0.4, -0.1, 0.0)],
         "sharp_bend": [(-0.3, -0.12, 0.0), (0.05, 0.0, 0.0), (-0.3, 0.12, 0.0)]}
_cache = {}


def tube(name):
    """(trajectories, capped 6-gon triangle tube) of one line of LINES."""
    if name not in _cache:
        pos = np.asarray(LINES[name], np.float32)
        tr = scenes._pack([pos], [np.linspace(0.0, 1.0, len(pos), dtype=np.float32)])
        _cache[name] = tr, lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)
    return _cache[name]


def pair_codes(idx):
    """The code of every leaf (triangles 2 g, 2 g + 1): which of the first triangle's vertices, or the fourth one (3), the second
    triangle's vertices are, two bits each -- lv_tri_pair_code restated."""
    idx = np.asarray(idx, np.uint32).reshape(-1, 3)
    codes = []
    for s in range(0, len(idx), 2):
        if s + 1 >= len(idx):
            codes.append(EMPTY)
            continue
        first = list(idx[s])
        codes.append(sum((first.index(b) if b in first else 3) << (2 * k) for k, b in enumerate(idx[s + 1])))
    return codes


def hit_mask_of(setup):
    """The pixels whose AO rays are traced: where the oracle's G-buffer pass on the mesh records a normal.  (The frame colours the
    capsules, whose silhouette differs from the 6-gon's.)"""
    P = setup.case.oracle_params(setup.scene)
    with lvo.ao_features(P.width, P.height) as f:
        setup.tri.render_ao(P, use_bvh=False)
    mask = (f.normal != 0).any(axis=-1)
    assert int(mask.sum()) > 140
    return mask


# ---------------------------------------------------------------- AO rays (k_ao_rays, k_ao_primary)
@pytest.mark.parametrize("hit", ["closest_hit", "any_hit"])
@pytest.mark.parametrize("scene", list(LINES))
def test_ao_launches_equal_brute_force(hip_lib, scene, hit):
    tr, mesh = tube(scene)
    s = Setup("triangle_pairs", tr=tr, mesh=mesh, width=192, height=128, ambient_occlusion_distance_based=hit == "closest_hit")
    assert {BODY, CAP_QUAD, FAN} <= set(pair_codes(mesh[0]))
    mask = hit_mask_of(s)
    for spp, counts in ((1, (1, 63, 64, 65, 129)), (64, (1, 2))):
        s.set("ambient_occlusion_samples_per_frame", spp)
        for want in counts:
            check_hit_count(s, mask, want)
    s.set("ambient_occlusion_samples_per_frame", 16)
    hits, occluded = s.check((0, 0, 192, 128))
    assert hits > 140 and occluded > 0           # the legs (and the caps' neighbourhood) do occlude
    assert s.ctx.stats().tri_leaf_bytes == 64


@pytest.mark.parametrize("scene", list(LINES))
def test_ao_primary_on_a_64x64_frame(hip_lib, scene):
    """k_ao_primary traces the G-buffer's rays against the same records: the whole frame, per-ray and per-pixel generation."""
    tr, mesh = tube(scene)
    s = Setup("triangle_pairs", tr=tr, mesh=mesh, width=64, height=64)
    for spp in (3, 64):
        s.set("ambient_occlusion_samples_per_frame", spp)
        hits, occluded = s.check((0, 0, 64, 64))
        assert hits > 30 and occluded > 0


def test_ao_on_48_byte_records(hip_lib):
    """A shuffled mesh shares no vertices inside a leaf: the build keeps 48-byte records, whose path is unchanged."""
    tr, mesh = tube("sharp_bend")
    s = Setup("triangle_records", tr=tr, mesh=mesh, width=192, height=128)
    mask = hit_mask_of(s)
    for want in (1, 65):
        check_hit_count(s, mask, want)
    s.set("ambient_occlusion_samples_per_frame", 16)
    hits, occluded = s.check((0, 0, 192, 128))
    assert hits > 140 and occluded > 0
    assert s.ctx.stats().tri_leaf_bytes == 96


# ---------------------------------------------------------------- aimed rays (lv_trace_rays_triangles: the tile kernels' walk)
def quads_mesh():
    """Quads (q0, q1, q2, q3) as pairs (q0, q1, q2)(q0, q2, q3) on dyadic coordinates, every quad on vertices of its own."""
    quads = [
        [(0, 0, 0), (0.5, 0, 0), (0.5, 0.5, 0), (0, 0.5, 0)],                               # a square in z = 0
        [(-0.5, -0.0, 1), (-0.0, 0.0, 1), (0.0, 0.5, 1), (-0.5, 0.5, 1)],                   # coordinates 0 and -0
        [(1, 0, 0), (1.25, 0.25, 0), (1.5, 0.5, 0), (1, 0.5, 0)],                           # q1 on the diagonal: first triangle without area
        [(1, 1, 0), (1.5, 1, 0), (1.5, 1.5, 0), (1.5, 1.5, 0)],                             # q3 = q2: second triangle without area
        [(-1, -1, 0.25), (-0.5, -1, 0), (-0.5, -0.5, 0.25), (-1, -0.5, 0.5)],               # not planar; the diagonal is level
        [(0.25, -1, -0.0), (0.75, -1, 0.0), (0.75, -0.5, -0.0), (0.25, -0.5, 0.0)],         # z = 0 and -0 alternating
    ]
    pos = np.asarray(quads, np.float32).reshape(-1, 3)
    verts = np.zeros(len(pos), lvo.TUBE_VERTEX_DTYPE)
    verts["vertexPosition"] = pos
    verts["vertexNormal"] = (0.0, 0.0, 1.0)
    idx = np.asarray([[4 * k, 4 * k + 1, 4 * k + 2, 4 * k, 4 * k + 2, 4 * k + 3] for k in range(len(quads))], np.uint32).reshape(-1, 3)
    return idx, verts, np.asarray(quads, np.float32)


def quad_rays(quads):
    """Rays with exactly representable origins and directions: down and up the z axis through every vertex, through points of the
    diagonal q0 - q2 and of the outer edges and through the inside of both triangles; along x and y inside the plane z = 0 (det == 0)
    and just above it; diagonal directions (1, 1, -1) / (-1, 1, -1) through the same targets."""
    o, d = [], []
    for q in quads:
        q0, q1, q2, q3 = q
        targets = [q0, q1, q2, q3] + [q0 + s * (q2 - q0) for s in (0.25, 0.5, 0.75)] + [0.5 * (q0 + q1), 0.5 * (q2 + q3), 0.5 * (q3 + q0)]
        targets += [0.5 * q0 + 0.25 * q1 + 0.25 * q2, 0.5 * q0 + 0.25 * q2 + 0.25 * q3]
        for p in targets:
            for dirn in ((0, 0, -1), (0, 0, 1), (1, 1, -1), (-1, 1, -1), (1, 0, 0), (0, -1, 0), (-1, 0, 0), (0, 1, 0)):
                dirn = np.asarray(dirn, np.float32)
                o.append(p - 2.0 * dirn)
                d.append(dirn)
                o.append(p - 2.0 * dirn + np.asarray((0.0, 0.0, 0.0078125), np.float32))   # 2^-7 above: misses in-plane, moves the rest
                d.append(dirn)
    return np.asarray(o, np.float32), np.asarray(d, np.float32)


def tube_rays(idx, verts):
    """General float32 directions at the body faces of a tube: from points off each face at its four vertices and at five points of
    its diagonal, from both sides, and a grid of axis-parallel rays across the tube's box."""
    idx = np.asarray(idx, np.uint32).reshape(-1, 3)
    pos = verts["vertexPosition"].astype(np.float32)
    codes = pair_codes(idx)
    o, d = [], []
    rng = np.random.default_rng(3)
    for g, code in enumerate(codes):
        if code != BODY:
            continue
        q0, q1, q2 = pos[idx[2 * g]]
        q3 = pos[idx[2 * g + 1][2]]
        n = np.cross(q1 - q0, q2 - q0)
        n /= np.linalg.norm(n)
        for p in [q0, q1, q2, q3] + [q0 + np.float32(s) * (q2 - q0) for s in (0.1, 0.3, 0.5, 0.7, 0.9)]:
            for side in (1.0, -1.0):
                a = p + np.float32(side * 0.2) * n + rng.uniform(-0.05, 0.05, 3).astype(np.float32)
                o.append(a)
                d.append((p - a) / np.linalg.norm(p - a))
    lo, hi = pos.min(axis=0) - 0.1, pos.max(axis=0) + 0.1
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for a in np.linspace(lo[u], hi[u], 24):
            for b in np.linspace(lo[v], hi[v], 12):
                for sign in (1.0, -1.0):
                    org = np.zeros(3); org[u] = a; org[v] = b; org[axis] = lo[axis] if sign > 0 else hi[axis]
                    dirn = np.zeros(3); dirn[axis] = sign
                    o.append(org); d.append(dirn)
    return np.asarray(o, np.float32), np.asarray(d, np.float32)


def triangle_context(mesh):
    tr, _ = tube("two_segments")
    pts, seg = scene_arrays(tr, LW)
    ctx = Case(pts, seg, tfm.standard(), 32, 32, LW).hip_context()
    ctx.set_tube_triangle_mesh(*mesh)
    return ctx


def compare_with_brute_force(ctx, mesh, o, d, counts=()):
    want = lvo.TriScene(*mesh, LW).trace_rays(o, d, T_MIN, T_MAX, use_bvh=False)
    got = ctx.trace_rays_triangles(o, d, T_MIN, T_MAX)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    for n in counts:
        part = ctx.trace_rays_triangles(o[:n], d[:n], T_MIN, T_MAX)
        assert np.array_equal(bits(part[0]), bits(want[0][:n])) and np.array_equal(part[1], want[1][:n]), n
    return want


def test_ties_degenerate_faces_and_signed_zeros(hip_lib):
    idx, verts, quads = quads_mesh()
    mesh = (idx, verts, np.zeros(1, lvo.LINE_POINT_DTYPE))
    assert set(pair_codes(idx)) == {BODY}
    o, d = quad_rays(quads)
    ctx = triangle_context(mesh)
    t, tri, _ = compare_with_brute_force(ctx, mesh, o, d, counts=(1, 63, 64, 65, 129))
    assert ctx.stats().tri_leaf_bytes == 64
    hit = tri != 0xFFFFFFFF
    assert hit.sum() > 200
    # a vertical ray through the middle of the square's diagonal meets both triangles at the same t: the lower index reports it
    k = int(np.nonzero((o == np.asarray((0.25, 0.25, 2.0), np.float32)).all(axis=1) & (d == np.asarray((0, 0, -1), np.float32)).all(axis=1))[0][0])
    assert tri[k] == 0 and t[k] == 2.0
    assert set(tri[hit]) >= {0, 1, 2 * 1, 2 * 1 + 1, 2 * 2 + 1, 2 * 3, 2 * 4, 2 * 4 + 1, 2 * 5, 2 * 5 + 1}   # both slots report hits
    assert 2 * 2 not in tri[hit] and 2 * 3 + 1 not in tri[hit]                                                # the faces without area never do


@pytest.mark.parametrize("records", ["pairs", "records"])
@pytest.mark.parametrize("scene", list(LINES))
def test_rays_at_diagonals_vertices_and_along_the_axes(hip_lib, scene, records):
    _, (idx, verts, lpts) = tube(scene)
    o, d = tube_rays(idx, verts)
    if records == "records":
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)[np.random.default_rng(4).permutation(len(idx))]
    mesh = (idx, verts, lpts)
    ctx = triangle_context(mesh)
    t, tri, _ = compare_with_brute_force(ctx, mesh, o, d, counts=(1, 63, 64, 65, 129))
    assert ctx.stats().tri_leaf_bytes == (64 if records == "pairs" else 96)
    assert int((tri != 0xFFFFFFFF).sum()) > 300
