"""BVH culling on grazing rays, GPU side: the compressed 4-wide BVH never culls a box whose primitive the ray hits -- closest hits,
AO factors and PPLL fragment depths against the oracle's BRUTE FORCE on rays that pass within a small fraction of the radius of a
box face (tests/grazing.py), in scenes inside the unit box and far outside it (translated by up to 1000, scaled by 256).

Every comparison is an equality; nothing here has a tolerance.  Every radius is at least 64 ulp of the largest coordinate, the
supported range of DESIGN.md's numerics contract (asserted in test_culling_grazing.py on the same scenes).  Colours and RGBA8 frames
are not compared away from the origin: shading at |x| = 100 is outside what these tests examine."""
import zlib

import numpy as np
import pytest

import grazing as gz
from common import Case, small_case
from grazing import CONFIG_IDS, MISS, T_MAX, T_MIN, bits, capsule_case, triangle_case
from linevis_amd import camera, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

BUILDS = [("default", dict()), ("fast_build", dict(accel_build="fast_build")), ("treelet7", dict(treelet_leaves=7))]
T100 = gz.CONFIGS[CONFIG_IDS.index("t100_w0.002")]


def capsule_context(pts, seg, lw, **options):
    c = Case(pts, seg, tfm.standard(), 32, 32, lw)
    ctx = c.hip_context()
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


@pytest.mark.parametrize("n_segments", [0, 1, 2], ids=["870seg", "1seg", "2seg"])
@pytest.mark.parametrize("name", CONFIG_IDS)
def test_capsule_closest_hits_equal_brute_force_on_grazing_rays(hip_lib, name, n_segments):
    """t bits, segment and kind of lv_trace_rays against the oracle's brute force, in every build and in both intersection forms
    (literal: the library's default, roots count inside the segment's own unpadded box; closest_approach: what RTAO frames trace).
    1 segment = k_single_node, 2 segments = the smallest collapsed node."""
    counts = []
    for literal in (True, False):
        _, pts, seg, lw, o, d, _, want = capsule_case(name, n_segments, literal)
        for build_name, build in BUILDS:
            ctx = capsule_context(pts, seg, lw, intersection_form="literal" if literal else "closest_approach", **build)
            t, s, k = ctx.trace_rays(o, d, T_MIN, T_MAX)
            differ = int(((bits(t) != bits(want[0])) | (s != want[1]) | (k != want[2])).sum())
            lost = int(((want[1] != MISS) & (s == MISS)).sum())
            print("GRAZING capsules %s %dseg %s %s: %d of %d rays differ, %d hits lost (%d hits)"
                  % (name, len(seg), "literal" if literal else "closest_approach", build_name, differ, len(o), lost,
                     int((want[1] != MISS).sum())))
            counts.append(differ)
    assert counts == [0] * len(counts)


TRI_BUILDS = [("pairs", dict(triangle_leaf_records="pairs")), ("triangles", dict(triangle_leaf_records="triangles")),
              ("leaf1", dict(triangle_leaf_size=1)), ("leaf4", dict(triangle_leaf_size=4))]


@pytest.mark.parametrize("name", CONFIG_IDS)
def test_triangle_closest_hits_equal_brute_force_on_vertex_grazing_rays(hip_lib, name):
    """t bits, triangle and barycentric bits of lv_trace_rays_triangles against TriScene.trace_rays(use_bvh=False): the hit's own-box
    rule (triPad) is part of its definition and the same on both sides; the GROUP boxes of the tree are what is under test."""
    ts, mesh, lw, o, d, _, want = triangle_case(name)
    _, pts, seg, *_ = capsule_case(name)          # (a context wants lines; the triangle rays do not look at them)
    assert (want[1] != MISS).sum() > 0
    counts = []
    for build_name, build in TRI_BUILDS:
        ctx = capsule_context(pts, seg, lw)
        ctx.set_tube_triangle_mesh(*mesh)
        for k, v in build.items():
            ctx.set_option(k, v)
        t, tri, uv = ctx.trace_rays_triangles(o, d, T_MIN, T_MAX)
        differ = int(((bits(t) != bits(want[0])) | (tri != want[1]) | (bits(uv) != bits(want[2])).any(axis=1)).sum())
        lost = int(((want[1] != MISS) & (tri == MISS)).sum())
        print("GRAZING triangles %s %s: %d of %d rays differ, %d hits lost (%d hits)"
              % (name, build_name, differ, len(o), lost, int((want[1] != MISS).sum())))
        counts.append(differ)
    assert counts == [0] * len(counts)


# ---------------------------------------------------------------- the box rule, structurally
LEAF, INVALID = 0x80000000, 0xFFFFFFFF


def decoded_planes(nodes):
    """float32 planes origin + q * scale of every slot, as lv_node_step's fma gives them: (n, 4 slots, 3 axes) min and max.  The
    extended-precision sum is exact here (checked: two-sum), so the one rounding to float32 is the fma's."""
    f = nodes.view(np.float32)
    origin, scale = f[:, 0:3].astype(np.longdouble), f[:, 3:6].astype(np.longdouble)
    out = []
    for words in (nodes[:, 6:9], nodes[:, 9:12]):
        q = np.stack([(words >> (8 * k)) & 0xFF for k in range(4)], axis=1).astype(np.longdouble)
        prod = q * scale[:, None, :]
        total = prod + origin[:, None, :]
        assert np.array_equal(total - origin[:, None, :], prod) and np.array_equal(total - prod, np.broadcast_to(origin[:, None, :], prod.shape))
        out.append(total.astype(np.float32))
    return out[0], out[1]


@pytest.mark.parametrize("name", ["t100_w0.002", "unit_w0.002"])
def test_leaf_boxes_contain_the_rule_box_exactly(hip_lib, name):
    """Every decoded leaf-child box contains lo = lo0 - max(pad, |lo0| * 2^-21) .. hi (gz.segment_boxes) with NO allowance, and every
    node's grid origin IS the minimum of the rule's lo over the leaves below it, bit for bit: a leaf that is the extreme child of its
    node on a face has q = 0 there and its plane equals the rule's lo."""
    _, pts, seg, lw, *_ = capsule_case(name)
    ctx = capsule_context(pts, seg, lw)
    ctx.build_accel()
    nw, n = ctx.stats().num_nodes, len(seg)
    nodes, leaf_seg = ctx.get_accel(nw, n)
    assert sorted(leaf_seg.tolist()) == list(range(n))
    lo, hi = gz.segment_boxes(pts["linePosition"], seg, lw * 0.5)
    dmin, dmax = decoded_planes(nodes)
    origin = nodes.view(np.float32)[:, 0:3]
    child = nodes[:, 12:16]
    qmin = np.stack([(nodes[:, 6:9] >> (8 * k)) & 0xFF for k in range(4)], axis=1)
    sub_lo = np.full((nw, 3), np.inf, dtype=np.float32)       # min of the rule's lo over the leaves below a node
    leaves = extreme = 0
    for node in range(nw - 1, -1, -1):                        # BFS numbering: children have larger indices than their parent
        for k in range(4):
            ref = int(child[node, k])
            if ref == INVALID:
                continue
            if ref & LEAF:
                s = leaf_seg[ref & 0x7FFFFFFF]
                assert np.all(dmin[node, k] <= lo[s]) and np.all(dmax[node, k] >= hi[s]), "node %d slot %d" % (node, k)
                sub_lo[node] = np.minimum(sub_lo[node], lo[s])
                leaves += 1
            else:
                assert ref > node
                sub_lo[node] = np.minimum(sub_lo[node], sub_lo[ref])
        assert np.array_equal(bits(origin[node]), bits(sub_lo[node])), "origin of node %d" % node
        for k in range(4):
            ref = int(child[node, k])
            if ref != INVALID and ref & LEAF:
                s = leaf_seg[ref & 0x7FFFFFFF]
                on_face = bits(lo[s]) == bits(origin[node])
                assert np.all(qmin[node, k][on_face] == 0) and np.array_equal(bits(dmin[node, k][on_face]), bits(lo[s][on_face]))
                extreme += int(on_face.sum())
    assert leaves == n and extreme >= 3


def test_unit_box_tree_is_unchanged(hip_lib):
    """The relative term exceeds the absolute pad (>= 1e-6) only for |x| > 2.09: a normalised scene -- every benchmark scene is one --
    gets the tree it got before.  The constant is the CRC32 of the node bytes + leaf order of this scene's default build on an
    MI355X at the commit before the boxes were padded relative to their coordinates."""
    c = small_case(n_lines=60, pts_per_line=50, seed=5, line_width=0.01)
    ctx = c.hip_context()
    ctx.build_accel()
    nodes, leaf_seg = ctx.get_accel(ctx.stats().num_nodes, len(c.seg))
    crc = zlib.crc32(nodes.tobytes() + leaf_seg.tobytes())
    print("GRAZING unit-box tree: %d nodes, CRC32 0x%08X" % (len(nodes), crc))
    assert crc == UNIT_BOX_TREE_CRC32


UNIT_BOX_TREE_CRC32 = 0x4453FCD9


# ---------------------------------------------------------------- the walkers of the frame kernels at (100, -100, 100)
def translated_case(line_width, **settings):
    """20 lines x 20 points at (100, -100, 100), 64 x 48, the default camera translated along with the scene"""
    tr = scenes.normalize(scenes.random_curves(n_lines=20, points_per_line=20, seed=7))
    pts, seg, _ = lvo.build_tube_aabb_render_data(tr.positions, tr.attributes, tr.line_offsets, line_width)
    T = np.asarray(T100[1], dtype=np.float32)
    pts["linePosition"] = (pts["linePosition"] + T).astype(np.float32)
    c = Case(pts, seg, settings.pop("tf", tfm.standard()), 64, 48, line_width, **settings)
    eye = T.astype(np.float64) + np.asarray(camera.DEFAULT_POSITION)
    c.view = camera.look_at(eye, center=T.astype(np.float64))
    return c


@pytest.mark.parametrize("line_width", [0.02, 0.002])
def test_rtao_factors_equal_brute_force_at_100(hip_lib, line_width):
    """k_ao_rays (any-hit walker, hardware reciprocals) through the tree against the oracle's brute-force AO, bit for bit"""
    c = translated_case(line_width, ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0,
                        ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=4)
    ctx = c.hip_context()
    ctx.render(11)
    ao = ctx.get_ao()
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    want = c.oracle_ao(sc, P, mode=11, use_bvh=False)
    differ = bits(ao) != bits(want)
    print("GRAZING rtao at 100, width %g: %d of %d factors differ, %d pixels occluded" % (line_width, int(differ.sum()), differ.size,
                                                                                           int((want < 1.0).sum())))
    assert (want < 1.0).sum() > 0
    assert not differ.any(), "first differing pixel (y, x) %s: %r vs %r" % (np.argwhere(differ)[0], ao[differ][0], want[differ][0])


def fragment_depths(nodes, start):
    """(pixel address, depth bits) of every linked fragment, sorted: the per-pixel multisets of depths in a canonical order"""
    nxt = nodes[:, 2]
    pix = np.flatnonzero(start != 0xFFFFFFFF)
    cur = start[pix].astype(np.int64)
    pp, ii = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    while len(pix):
        pp.append(pix)
        ii.append(cur)
        n = nxt[cur]
        keep = n != 0xFFFFFFFF
        pix, cur = pix[keep], n[keep].astype(np.int64)
    pp, ii = np.concatenate(pp), np.concatenate(ii)
    assert len(np.unique(ii)) == len(ii), "a node is linked twice"
    key = np.lexsort((nodes[ii, 1], pp))
    return pp[key], nodes[ii[key], 1]


@pytest.mark.parametrize("line_width", [0.02, 0.002])
def test_ppll_fragment_depths_equal_brute_force_at_100(hip_lib, line_width):
    """k_ppll_gather's all-hits walker (ppll_fragment_source = capsule_entry): fragment count and the per-pixel multisets of fragment
    depths against the oracle's brute-force gather, bit for bit"""
    c = translated_case(line_width, tf=tfm.standard_transparent(), ppll_fragment_source="capsule_entry")
    ctx = c.hip_context()
    ctx.render(2)
    pw, ph = c.padded()
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    on, os_, ocnt = sc.ppll_gather(P, use_bvh=False)
    hn, hs, hcnt = ctx.ppll_buffers(pw * ph, int(P.ppllLinkedListSize))
    gp, gd = fragment_depths(hn, hs)
    op, od = fragment_depths(on, os_)
    print("GRAZING ppll at 100, width %g: %d fragments, oracle %d" % (line_width, hcnt, ocnt))
    assert ocnt > 0 and len(op) == ocnt
    assert hcnt == ocnt and len(gp) == hcnt
    assert np.array_equal(gp, op) and np.array_equal(gd, od)
