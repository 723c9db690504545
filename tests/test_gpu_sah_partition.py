"""accel_partition = sah | morton (lv_bvh.hip, k_part_*): a binned-SAH partition of the whole scene chooses which leaves share a
treelet of the fast_trace build by putting path-code bits in front of the Morton sort keys.  It changes the topology only, so every
comparison here is an equality: closest hits and frames of `sah` against `morton` and against the oracle's brute force, every leaf
exactly once, child boxes that contain their subtrees, identical node bytes from two builds.

treelet_leaves is set small (8) in most cases so that a few hundred segments go through several levels of cuts, and
accel_partition_min_leaves to 0: by default builds of fewer than 65 536 leaves keep the Morton order."""
import functools

import numpy as np
import pytest

import grazing as gz
from common import Case
from grazing import MISS, T_MAX, T_MIN, bits
from linevis_amd import capi, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LEAF, INVALID = 0x80000000, 0xFFFFFFFF
MAX_BINARY_HEIGHT = 63 + 32      # key bits + duplicate-index bits: what the traversal stack's overflow slab is specified for (lv_trace.h)
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
            ambient_occlusion_samples_per_frame=4)


def context(pts, seg, lw, **options):
    ctx = Case(pts, seg, tfm.standard(), 32, 32, lw).hip_context()
    ctx.set_options(dict(dict(accel_partition_min_leaves=0), **options))
    return ctx


def rays_at(pts, seg, lw, n, seed):
    """half grazing rays aimed at box faces of the segments (tests/grazing.py), half random rays through the scene's box"""
    pos = pts["linePosition"]
    o, d, _ = gz.grazing_rays(pos, seg, lw * 0.5, n // 2, seed, distances=(0.5, 8.0))
    rng = np.random.default_rng(seed + 1)
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    a = rng.uniform(lo - 0.1, hi + 0.1, (n - n // 2, 3))
    b = rng.uniform(lo, hi, (n - n // 2, 3))
    dd = b - a
    dd /= np.maximum(np.linalg.norm(dd, axis=1, keepdims=True), 1e-12)
    return np.concatenate([o, a.astype(np.float32)]), np.concatenate([d, dd.astype(np.float32)])


# ---------------------------------------------------------------- scenes, computed once
@functools.lru_cache(maxsize=None)
def curves_scene(n_lines=40, pts_per_line=51, lw=0.01, seed=3):
    """about 2 000 segments of normalised random curves and 4 000 rays at them"""
    tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=pts_per_line, seed=seed))
    pts, seg, _ = lvo.build_tube_aabb_render_data(tr.positions, tr.attributes, tr.line_offsets, lw)
    o, d = rays_at(pts, seg, lw, 4000, 100 + seed)
    return tr, pts, seg, lw, o, d


def _replicate(pts, seg, n):
    """n copies of the first segment, each with its own two points"""
    two = pts[[seg[0, 0], seg[0, 1]]]
    return np.tile(two, n), (np.arange(2 * n, dtype=np.uint32).reshape(n, 2))


@functools.lru_cache(maxsize=None)
def edge_scene(name):
    tr, pts, seg, lw, _, _ = curves_scene()
    t = 8   # treelet_leaves of the edge builds
    if name in ("1", "2", "3", "treelet", "treelet+1"):
        n = {"1": 1, "2": 2, "3": 3, "treelet": t, "treelet+1": t + 1}[name]
        p, s = pts[:n + 1].copy(), seg[:n].copy()              # the first n segments of the first line
    elif name == "identical":                                    # every centre equal: no plane separates anything
        p, s = _replicate(pts, seg, 300)
    elif name == "collinear":                                    # every centre on one axis-aligned line
        x = np.linspace(-0.5, 0.5, 301)
        pos = np.stack([x, np.full_like(x, 0.125), np.full_like(x, -0.25)], axis=1).astype(np.float32)
        p, s, _ = lvo.build_tube_aabb_render_data(pos, np.linspace(0, 1, 301).astype(np.float32), np.array([0, 301], np.uint32), lw)
    elif name == "clumps":                                       # 2 000 segments here, 20 of them 40 units away
        far = pts[:21].copy()
        far["linePosition"] = (far["linePosition"] * np.float32(0.25) + np.array([40.0, -3.0, 7.0], np.float32)).astype(np.float32)
        p = np.concatenate([pts, far])
        s = np.concatenate([seg, seg[:20] + np.uint32(len(pts))])
    else:
        raise KeyError(name)
    o, d = rays_at(p, s, lw, 2000, 7)
    lvo.set_default_intersection_form(True)
    want = lvo.Scene(p, s, tfm.standard()).trace_rays(o, d, T_MIN, T_MAX, lw, use_bvh=False)
    return p, s, lw, o, d, want


EDGE_SCENES = ["1", "2", "3", "treelet", "treelet+1", "identical", "collinear", "clumps"]


# ---------------------------------------------------------------- the contract: the same hits in both partitions
@pytest.mark.parametrize("treelet", [8, 512])
def test_capsule_rays_hit_the_same_in_both_partitions(hip_lib, treelet):
    _, pts, seg, lw, o, d = curves_scene()
    got = {}
    for part in ("sah", "morton"):
        ctx = context(pts, seg, lw, accel_partition=part, treelet_leaves=treelet, intersection_form="literal")
        got[part] = ctx.trace_rays(o, d, T_MIN, T_MAX)
    (t, s, k), (tm, sm, km) = got["sah"], got["morton"]
    hits = int((s != MISS).sum())
    print("SAH PARTITION capsules treelet %d: %d of %d rays hit, %d differ" % (treelet, hits, len(o), int(((bits(t) != bits(tm)) | (s != sm) | (k != km)).sum())))
    assert hits > 500
    assert np.array_equal(bits(t), bits(tm)) and np.array_equal(s, sm) and np.array_equal(k, km)


@pytest.mark.parametrize("treelet", [8, 512])
def test_triangle_rays_hit_the_same_in_both_partitions(hip_lib, treelet):
    tr, pts, seg, lw, o, d = curves_scene(n_lines=20, pts_per_line=21, lw=0.02)    # 400 segments = 4 560 triangles, 2 280 pair leaves
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
    o2, d2, _ = gz.grazing_rays_at_vertices(mesh[1]["vertexPosition"], lw * 0.5, 2000, 5, distances=(0.5, 8.0))
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    got = {}
    for part in ("sah", "morton"):
        ctx = context(pts, seg, lw, accel_partition=part, treelet_leaves=treelet)
        ctx.set_tube_triangle_mesh(*mesh)
        got[part] = ctx.trace_rays_triangles(o, d, T_MIN, T_MAX)
    (t, tri, uv), (tm, trim, uvm) = got["sah"], got["morton"]
    assert int((tri != MISS).sum()) > 500
    assert np.array_equal(bits(t), bits(tm)) and np.array_equal(tri, trim) and np.array_equal(bits(uv), bits(uvm))


@pytest.mark.parametrize("geometry", ["capsules", "triangle_tubes"])
def test_rtao_frame_is_identical_in_both_partitions(hip_lib, geometry):
    """64 x 64 at 4 samples per pixel through k_ao_rays: AO factors and frame bytes"""
    tr, pts, seg, lw, _, _ = curves_scene()
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
    got = {}
    for part in ("sah", "morton"):
        c = Case(pts, seg, tfm.standard(), 64, 64, lw, rtao_geometry=geometry, accel_partition=part, accel_partition_min_leaves=0, treelet_leaves=8,
                 **RTAO)
        ctx = c.hip_context()
        if geometry == "triangle_tubes":
            ctx.set_tube_triangle_mesh(*mesh)
        frame = ctx.render(11)
        got[part] = (np.array(frame, copy=True), np.array(ctx.get_ao(), copy=True))
    assert (got["morton"][1] < 1.0).sum() > 50
    assert np.array_equal(bits(got["sah"][1]), bits(got["morton"][1]))
    assert got["sah"][0].tobytes() == got["morton"][0].tobytes()


# ---------------------------------------------------------------- edge sizes against brute force
@pytest.mark.parametrize("name", EDGE_SCENES)
def test_edge_scenes_build_and_hit_like_brute_force(hip_lib, name):
    """1, 2, 3 leaves; exactly treelet_leaves (no cut) and one more (one cut); all centres equal; all centres on a line; two clumps of
    2 000 and 20 segments: the build finishes, every segment is a leaf exactly once, closest hits equal the oracle's brute force."""
    p, s, lw, o, d, want = edge_scene(name)
    ctx = context(p, s, lw, accel_partition="sah", treelet_leaves=8, intersection_form="literal")
    t, hit, kind = ctx.trace_rays(o, d, T_MIN, T_MAX)
    st = ctx.stats()
    _, leaf_seg = ctx.get_accel(st.num_nodes, len(s))
    assert sorted(leaf_seg.tolist()) == list(range(len(s)))
    assert (want[1] != MISS).sum() > 100
    assert np.array_equal(bits(t), bits(want[0])) and np.array_equal(kind, want[2])
    if name == "identical":     # 300 copies of one capsule tie on every hit: any of them is the closest
        assert np.array_equal(hit == MISS, want[1] == MISS)
    else:
        assert np.array_equal(hit, want[1])


# ---------------------------------------------------------------- the built tree
def decode(nodes):
    """(n, 4 slots, 6) child boxes origin + q * scale as lv_node_step's float32 fma gives them (the sum is exact in extended precision,
    so the one rounding to float32 is the fma's) and the (n, 4) child references"""
    f = nodes.view(np.float32)
    origin, scale = f[:, 0:3].astype(np.longdouble), f[:, 3:6].astype(np.longdouble)
    boxes = np.zeros((len(nodes), 4, 6), np.float32)
    for k in range(4):
        boxes[:, k, 0:3] = (origin + ((nodes[:, 6:9] >> (8 * k)) & 255).astype(np.longdouble) * scale).astype(np.float32)
        boxes[:, k, 3:6] = (origin + ((nodes[:, 9:12] >> (8 * k)) & 255).astype(np.longdouble) * scale).astype(np.float32)
    return boxes, nodes[:, 12:16]


def check_tree(ctx, pts, seg, lw):
    """each child box contains its subtree (leaf slots the padded box of their capsule), every leaf is referenced once, the node count
    is within the allocation (n - 1 nodes), the height within what the traversal stack supports.  Returns (nodes, leaf order)."""
    n = len(seg)
    st = ctx.stats()
    assert 1 <= st.num_nodes <= max(n - 1, 1)
    assert 1 <= st.bvh_depth <= MAX_BINARY_HEIGHT
    nodes, leaf_seg = ctx.get_accel(st.num_nodes, n)
    assert sorted(leaf_seg.tolist()) == list(range(n))
    boxes, child = decode(nodes)
    lo, hi = gz.segment_boxes(pts["linePosition"], seg, lw * 0.5)
    sub = np.zeros((len(nodes), 6))
    sub[:, :3], sub[:, 3:] = np.inf, -np.inf
    depth = np.zeros(len(nodes), np.int64)
    seen = np.zeros(n, np.int64)
    for node in range(len(nodes)):                      # BFS numbering: a child has a larger index than its parent
        for k in range(4):
            ref = int(child[node, k])
            if ref != INVALID and not ref & LEAF:
                assert node < ref < len(nodes)
                depth[ref] = depth[node] + 1
    for node in range(len(nodes) - 1, -1, -1):
        for k in range(4):
            ref = int(child[node, k])
            if ref == INVALID:
                continue
            if ref & LEAF:
                s = leaf_seg[ref & 0x7FFFFFFF]
                seen[ref & 0x7FFFFFFF] += 1
                inner = np.concatenate([lo[s], hi[s]])
            else:
                inner = sub[ref]
            b = boxes[node, k]
            assert np.all(b[:3] <= inner[:3]) and np.all(b[3:] >= inner[3:]), "node %d slot %d" % (node, k)
            sub[node, :3] = np.minimum(sub[node, :3], inner[:3])      # the exact boxes of the leaves below: a child's own planes are
            sub[node, 3:] = np.maximum(sub[node, 3:], inner[3:])      # rounded outwards on its own grid and may pass its parent's
    assert np.all(seen == 1)
    assert depth.max() + 1 <= st.bvh_depth                # a level of the wide tree takes at least one binary level
    return nodes, leaf_seg


@pytest.mark.parametrize("treelet", [8, 512])
def test_tree_invariants_and_determinism(hip_lib, treelet):
    """the invariants of check_tree, and two builds of the same scene give the same node bytes and leaf order: the bins are integer
    atomics on ordered float bits, so the keys do not depend on the order in which the leaves arrive"""
    _, pts, seg, lw, _, _ = curves_scene()
    built = []
    for _ in range(2):
        ctx = context(pts, seg, lw, accel_partition="sah", treelet_leaves=treelet)
        ctx.build_accel()
        built.append(check_tree(ctx, pts, seg, lw) if not built else ctx.get_accel(ctx.stats().num_nodes, len(seg)))
    assert built[0][0].tobytes() == built[1][0].tobytes() and np.array_equal(built[0][1], built[1][1])
    morton = context(pts, seg, lw, accel_partition="morton", treelet_leaves=treelet)
    morton.build_accel()
    other = morton.get_accel(morton.stats().num_nodes, len(seg))
    assert not np.array_equal(built[0][1], other[1]), "the partition moved no leaf: it did not run"


@pytest.mark.parametrize("name", ["identical", "collinear", "clumps"])
def test_tree_invariants_on_degenerate_scenes(hip_lib, name):
    p, s, lw, *_ = edge_scene(name)
    ctx = context(p, s, lw, accel_partition="sah", treelet_leaves=8)
    ctx.build_accel()
    check_tree(ctx, p, s, lw)


def test_level_cap_falls_through_to_morton_order(hip_lib):
    """The loop over the levels of cuts is bounded by a constant (32 path bits), not by the data: a cluster that still holds more than
    treelet_leaves leaves when the cap is reached, that no plane separates, or that finds the cluster table full gets no further bits
    and its leaves keep their Morton order, so the build always ends.  treelet_leaves = 3 on 2 000 segments cuts down to clusters of
    three -- the deepest partition the options allow; the build finishes with a valid tree and the hits of the Morton build."""
    _, pts, seg, lw, o, d = curves_scene()
    ctx = context(pts, seg, lw, accel_partition="sah", treelet_leaves=3, intersection_form="literal")
    ctx.build_accel()
    check_tree(ctx, pts, seg, lw)
    ref = context(pts, seg, lw, accel_partition="morton", treelet_leaves=3, intersection_form="literal")
    a, b = ctx.trace_rays(o, d, T_MIN, T_MAX), ref.trace_rays(o, d, T_MIN, T_MAX)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_option_values(hip_lib):
    """sah is the default of fast_trace for builds of at least accel_partition_min_leaves leaves (default 65 536: this scene of about 2 000
    keeps the Morton order unless the option says otherwise), morton gives the tree of the build without the partition, fast_build
    ignores the key, any other string is an error"""
    _, pts, seg, lw, _, _ = curves_scene()

    def tree(**options):
        ctx = Case(pts, seg, tfm.standard(), 32, 32, lw).hip_context()
        ctx.set_options(options)
        ctx.build_accel()
        nodes, leaf = ctx.get_accel(ctx.stats().num_nodes, len(seg))
        return nodes.tobytes() + leaf.tobytes()

    morton = tree(accel_partition="morton")
    n = len(seg)
    assert tree() == tree(accel_partition="sah") == tree(accel_partition_min_leaves=n + 1) == morton
    assert tree(accel_partition_min_leaves=0) == tree(accel_partition_min_leaves=n) == tree(accel_partition="sah", accel_partition_min_leaves=0) != morton
    assert tree(accel_partition="morton", accel_partition_min_leaves=0) == morton
    assert tree(accel_build="fast_build") == tree(accel_build="fast_build", accel_partition_min_leaves=0)
    ctx = context(pts, seg, lw)
    for bad in ("SAH", "", "lbvh", "1"):
        with pytest.raises(capi.LineVisError):
            ctx.set_option("accel_partition", bad)
    with pytest.raises(capi.LineVisError):
        ctx.set_option("accel_partition_min_leaves", "many")
