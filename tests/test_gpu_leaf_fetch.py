"""Leaf tests that issue their record loads first and whole, and node / leaf-record addresses formed as 32-bit offsets from the
scene's base pointers (lv_leaf_test, lv_node_step: LV_LEAF_FETCH_FIRST, LV_OFFSET32 in lv_trace.h).

Neither changes a value that is computed: the same bytes reach the same float32 operations in the same order.  So every result is
compared bit for bit with brute force over all primitives -- the CPU oracle's render_ao / trace_rays with use_bvh=False, as in
tests/test_gpu_ao_stint_cycle.py -- and there is no tolerance to choose.

Scene: 3 lines x 5 points, 0.05 apart and 0.5 long, so that the AO rays of a pixel (radius 0.1) reach the neighbouring tubes and,
from a pixel at a line's end, their caps.  Launches: one hit pixel x 64 samples (one full batch, per-pixel generation) and 65 hit pixels
x 1 sample (a full batch and a ray), in every form of the leaf record: pair records (64 bytes, cap and fan codes fetched again by
address at the line ends), 48-byte records (shuffled triangles share no vertices inside a leaf), capsules with closest-approach and with
literal roots, the any-hit instantiation, an empty scene.  lv_trace_rays / lv_trace_rays_triangles run the tile kernels' walks, which
call the same functions, on 256 random rays.

The largest reference the setters accept (2^26 - 1 primitives) cannot be allocated in a test: that its byte offset fits 32 bits is a
static_assert next to LV_REF_BITS (lv_device.h); test_reference_bound_is_what_the_setters_refuse checks on the host that the setters
refuse the first count above it."""
import ctypes as C

import numpy as np
import pytest

from common import Case, scene_arrays
from linevis_amd import capi, scenes, transfer_function as tfm
from oracle import lvo
from test_gpu_ao_stint_cycle import LW, RTAO, Setup, bits, rects_with

pytestmark = pytest.mark.gpu

T_MIN, T_MAX = 1e-4, 1000.0
LV_E_CAPACITY = -4   # include/linevis_hip.h
_cache = {}


def three_lines():
    """3 gently bent lines x 5 points along x, 0.05 apart in y (inside the AO radius of 0.1), and their capped 6-gon triangle tubes."""
    if "tr" not in _cache:
        x = np.linspace(-0.25, 0.25, 5)
        lines = [np.stack([x, np.full(5, 0.05 * (i - 1)), 0.02 * np.sin(6.0 * x + i)], axis=1).astype(np.float32) for i in range(3)]
        tr = scenes._pack(lines, [np.linspace(0.0, 1.0, 5, dtype=np.float32)] * 3)
        _cache["tr"] = tr
        _cache["mesh"] = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)
    return _cache["tr"], _cache["mesh"]


def rays():
    """256 rays from around the scene's box at points inside it (most of them hit a tube), the same for every form."""
    if "rays" not in _cache:
        rng = np.random.default_rng(11)
        a = rng.uniform([-0.4, -0.2, -0.15], [0.4, 0.2, 0.15], (256, 3))
        b = rng.uniform([-0.25, -0.06, -0.02], [0.25, 0.06, 0.02], (256, 3))
        d = b - a
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
        _cache["rays"] = a.astype(np.float32), d.astype(np.float32)
    return _cache["rays"]


def check_hit_count(setup, mask, want, at_line_end=False):
    """A viewport of a few pixels with exactly `want` hit pixels (counted by the library; the frame only proposes rectangles), its AO
    equal to brute force bit for bit.  at_line_end: the leftmost such viewport -- the lines end at the same x, their caps are there."""
    tiles = [t for slack in range(0, 4) for t in rects_with(mask, want + slack)]
    if at_line_end:
        tiles.sort(key=lambda t: t[0])
    for tile in tiles[:40]:
        hits, occluded = setup.check(tile)
        if hits == want:
            return occluded
    raise AssertionError("no viewport with %d hit pixels" % want)


@pytest.mark.parametrize("form", ["triangle_pairs", "triangle_pairs_caps", "triangle_records", "capsules", "capsules_literal",
                                  "triangle_pairs_any_hit", "capsules_any_hit"])
def test_one_batch_and_a_ray_equal_brute_force(hip_lib, form):
    tr, mesh = three_lines()
    geometry = form.replace("_caps", "").replace("_any_hit", "")
    extra = dict(ambient_occlusion_distance_based=False) if form.endswith("_any_hit") else {}
    s = Setup(geometry, tr=tr, mesh=mesh, **extra)
    s.ctx.set_option("ambient_occlusion_samples_per_frame", 1)
    img = s.ctx.render(capi.MODE_RAY_TRACER)
    assert int(s.ctx.stats().ao_hit_pixels) > 65
    mask = (img[..., :3] != 255).any(axis=-1)
    if geometry.startswith("triangle"):
        assert s.ctx.stats().tri_leaf_bytes == (96 if geometry == "triangle_records" else 64)
    end = form.endswith("_caps")
    s.set("ambient_occlusion_samples_per_frame", 64)
    occluded = check_hit_count(s, mask, 1, at_line_end=end)       # 64 rays: one pixel's batch
    s.set("ambient_occlusion_samples_per_frame", 1)
    occluded += check_hit_count(s, mask, 65, at_line_end=end)     # 65 rays: a full batch and one ray
    assert occluded > 0                                            # the rays do meet the neighbouring tubes


def test_empty_scene(hip_lib):
    case = Case(np.zeros(0, dtype=lvo.LINE_POINT_DTYPE), np.zeros((0, 2), np.uint32), tfm.standard(), 40, 24, 0.01,
                ambient_occlusion_samples_per_frame=64, **RTAO)
    ctx = case.hip_context()
    img = ctx.render(capi.MODE_RAY_TRACER)
    assert int(ctx.stats().ao_hit_pixels) == 0
    assert (img[..., :3] == 255).all() and np.array_equal(bits(ctx.get_ao()), bits(np.ones((24, 40), np.float32)))
    o, d = rays()
    t, seg, _ = ctx.trace_rays(o, d, T_MIN, T_MAX)
    assert (seg == 0xFFFFFFFF).all()


@pytest.mark.parametrize("form", ["closest_approach", "literal"])
def test_trace_rays_equal_brute_force(hip_lib, form):
    tr, _ = three_lines()
    pts, seg = scene_arrays(tr, LW)
    o, d = rays()
    case = Case(pts, seg, tfm.standard(), 32, 32, LW, intersection_form=form)
    ctx = case.hip_context()
    got = ctx.trace_rays(o, d, T_MIN, T_MAX)
    sc = case.oracle_scene()
    case.oracle_params(sc)                      # the oracle on the roots this case's settings select
    want = sc.trace_rays(o, d, T_MIN, T_MAX, LW, use_bvh=False)
    assert int((want[1] != 0xFFFFFFFF).sum()) > 100
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("records", ["pairs", "records"])
def test_trace_rays_triangles_equal_brute_force(hip_lib, records):
    tr, mesh = three_lines()
    pts, seg = scene_arrays(tr, LW)
    idx, verts, lpts = mesh
    if records == "records":                    # shuffled: no two triangles of a leaf share two vertices, the build keeps 48-byte records
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)[np.random.default_rng(4).permutation(len(idx))]
    o, d = rays()
    ctx = Case(pts, seg, tfm.standard(), 32, 32, LW).hip_context()
    ctx.set_tube_triangle_mesh(idx, verts, lpts)
    got = ctx.trace_rays_triangles(o, d, T_MIN, T_MAX)
    want = lvo.TriScene(idx, verts, lpts, LW).trace_rays(o, d, T_MIN, T_MAX, use_bvh=False)
    assert int((want[1] != 0xFFFFFFFF).sum()) > 100
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])


def test_reference_bound_is_what_the_setters_refuse(hip_lib):
    """References are below 2^26 (LV_REF_BITS, lv_device.h): the setters refuse 2^26 primitives before they read an array."""
    tr, mesh = three_lines()
    pts, seg = scene_arrays(tr, LW)
    ctx = Case(pts, seg, tfm.standard(), 32, 32, LW).hip_context()
    one = np.zeros(4, np.uint32)
    p = one.ctypes.data_as(C.c_void_p)
    assert ctx.L.lv_set_lines(ctx.h, p, 1, p, 1 << 26) == LV_E_CAPACITY
    assert ctx.L.lv_set_tube_triangle_mesh(ctx.h, p, 1 << 26, p, 1, p, 1) == LV_E_CAPACITY
