"""The simulation-mesh hull on the GPU (lv_hull.h; include/linevis_hip.h, hull_opacity): lv_hull_get_fragments bit for bit against
the restatement of tests/test_hull_restatement.py, then the hull inside rendering modes 5, 8 and 10 against the folds of the union
of the oracle's line fragments and the restated hull fragments, invariance under tile lists / a one-rank handle / repetition, no
change without a hull in every mode, the refusals, and the host plugin."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff
from linevis_amd import capi, host_api, scenes
from oracle import lvo
from test_atomic_loop_restatement import EMPTY
from test_hull_restatement import (DEFAULT_COLOR, DEFAULT_OPACITY, F, LW, al64_keys, frame_references, hull_case, hull_fragments, hull_runs,
                                   line_fragments, reference_fragments)
from test_mlab_restatement import pack
from test_wboit_restatement import WEIGHTS

pytestmark = pytest.mark.gpu
HULL_MODES = (capi.MODE_DEPTH_COMPLEXITY, capi.MODE_WBOIT, capi.MODE_ATOMIC_LOOP_64)


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _context(c, hull, opacity=DEFAULT_OPACITY, **options):
    ctx = c.hip_context()
    if hull is not None:
        ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    if opacity is not None:
        ctx.set_option("hull_opacity", opacity)
    ctx.set_options(options)
    return ctx


def _sorted_fragments(ctx):
    pix, tri, z, rgba = ctx.hull_fragments()
    order = np.lexsort((tri, pix))
    return pix[order], tri[order], z[order], rgba[order]


def _channels(packed):
    return np.stack([(packed >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=-1).astype(np.int32)


def _pack_rows(rgba):
    return pack([rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]])


# ---------------------------------------------------------------- 1. the fragments, bit for bit
@pytest.mark.parametrize("variant", ["outside", "odd", "inside", "strip", "shading_off"])
def test_fragments_bit_for_bit(hip_lib, variant):
    kind = "outside" if variant == "shading_off" else variant
    shading = variant != "shading_off"
    c, hull, V = hull_case(kind)
    want = reference_fragments(kind, shading)
    ctx = _context(c, hull, hull_use_shading=shading)
    pix, tri, z, rgba = _sorted_fragments(ctx)
    assert len(pix) == len(want["pixel"]) > 1000
    assert np.array_equal(pix, want["pixel"]) and np.array_equal(tri, want["tri"])
    assert np.array_equal(z.view(np.uint32), want["zbits"])
    # the project's +- 2 LSB contract on the packed colours; the float difference is reported, no bar on it
    diff = float(np.abs(rgba.astype(np.float64) - want["rgba"].astype(np.float64)).max())
    print("hull fragments %s: %d fragments, largest float32 colour difference %.3g" % (variant, len(pix), diff))
    assert np.abs(_channels(_pack_rows(rgba)) - _channels(_pack_rows(want["rgba"]))).max() <= 2
    if not shading:
        assert np.all(rgba[:, :3] == np.asarray(DEFAULT_COLOR, F))
    # (the call is the hull's picking query: it does not depend on hull_opacity having been set, and a second call is the first)
    again = _sorted_fragments(ctx)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (pix, tri, z, rgba)))


def test_colour_and_opacity_reach_the_fragments(hip_lib):
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull, opacity=0.7, hull_color="0.25 0.5, 1", hull_use_shading=False)
    pix, tri, z, rgba = _sorted_fragments(ctx)
    want = hull_fragments(hull, V, opacity=0.7, color=(0.25, 0.5, 1.0), use_shading=False)
    assert np.array_equal(pix, want["pixel"]) and np.array_equal(rgba.view(np.uint32), want["rgba"].view(np.uint32))
    assert np.all(rgba[:, :3] == np.array([0.25, 0.5, 1.0], F))


# ---------------------------------------------------------------- 2. the three modes with the hull
@functools.lru_cache(maxsize=None)
def _references(K, weight="reference"):
    c, hull, V = hull_case("outside")
    return frame_references(c, reference_fragments("outside"), K=K, weight=weight)


def test_mode_5_counts_the_hull(hip_lib):
    c, hull, V = hull_case("outside")
    want = reference_fragments("outside")
    hull_counts = np.bincount(want["pixel"], minlength=V.w * V.h).reshape(V.h, V.w).astype(np.uint32)
    ctx = _context(c, hull)
    img = ctx.render(capi.MODE_DEPTH_COMPLEXITY)
    with_hull = ctx.depth_complexity_buffers()
    st = ctx.depth_complexity_stats()
    frags = int(ctx.stats().fragments)
    ctx.set_option("hull_opacity", 0)
    ctx.render(capi.MODE_DEPTH_COMPLEXITY)
    without = ctx.depth_complexity_buffers()
    assert np.array_equal(with_hull - without, hull_counts) and hull_counts.sum() > 5000
    ref = _references(8)["dc"]
    assert np.array_equal(with_hull, ref[1])
    assert st["total"] == int(with_hull.sum()) == frags and st["max"] == int(with_hull.max())
    assert st["used_locations"] == int((with_hull > 0).sum()) and st["min"] == int(with_hull.min())
    assert max_lsb_diff(img, ref[0]) <= 2 and np.array_equal(img, ref[0])      # (the maximum that scales the colours includes the hull)


def test_mode_10_slots_hold_the_union(hip_lib):
    c, hull, V = hull_case("outside")
    want = reference_fragments("outside")
    K = int(_references(8)["al64"][3].max())
    assert 8 < K <= 64
    ref = _references(K)["al64"]
    ctx = _context(c, hull, atomic_loop_num_layers=K)
    ctx.render(capi.MODE_ATOMIC_LOOP_64)
    slots, tail = ctx.atomic_loop_buffers()
    assert not tail.any() and int(ctx.stats().fragments) == int(ref[3].sum())
    # the depth words: the sorted union of the oracle's line keys and the restated hull keys past the 0.001 discard
    assert np.array_equal(slots >> np.uint64(32), ref[1] >> np.uint64(32))
    off, rgba, z = line_fragments(c)
    is_line = np.isin(ref[1], al64_keys(rgba, z)) & (ref[1] != EMPTY)
    is_hull = ~is_line & (ref[1] != EMPTY)
    assert is_line.sum() > 1500 and is_hull.sum() == int((want["rgba"][:, 3] >= F(0.001)).sum()) > 5000
    assert np.array_equal(slots[is_line], ref[1][is_line])                      # line keys: whole words
    lo = lambda a: (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert np.abs(_channels(lo(slots[is_hull])) - _channels(lo(ref[1][is_hull]))).max() <= 2


def test_mode_10_tail_takes_hull_fragments(hip_lib):
    """K = 2: hull fragments reach the tail.  The fold of the union with the device's OWN hull colours (hull_fragments()) is the frame,
    the slots and the tail byte for byte -- the fold apart from the shading"""
    c, hull, V = hull_case("outside")
    want = reference_fragments("outside")
    ctx = _context(c, hull, atomic_loop_num_layers=2)
    pix, tri, z, rgba = _sorted_fragments(ctx)
    assert np.array_equal(pix, want["pixel"]) and np.array_equal(z.view(np.uint32), want["zbits"])
    ref = frame_references(c, want, K=2, hull_rgba=rgba)["al64"]
    img = ctx.render(capi.MODE_ATOMIC_LOOP_64)
    slots, tail = ctx.atomic_loop_buffers()
    hoff = hull_runs(want, V.w * V.h)
    in_tail = (ref[2][..., 0] != 0) & (np.diff(hoff).reshape(V.h, V.w) > 0)
    assert in_tail.sum() > 200
    assert np.array_equal(slots, ref[1]) and np.array_equal(tail, ref[2])
    assert max_lsb_diff(img, ref[0]) <= 2 and np.array_equal(img, ref[0])


@pytest.mark.parametrize("weight", WEIGHTS)
def test_mode_8_adds_the_hull(hip_lib, weight):
    c, hull, V = hull_case("outside")
    ref = _references(8, weight)["wboit"]
    ctx = _context(c, hull, wboit_depth_weight=weight)
    img = ctx.render(capi.MODE_WBOIT)
    sums, counts = ctx.wboit_buffers()
    assert np.array_equal(counts, ref[2]) and int(ctx.stats().fragments) == int(ref[2].sum())
    assert max_lsb_diff(img, ref[0]) <= 2
    without = _context(c, None, wboit_depth_weight=weight).render(capi.MODE_WBOIT)
    assert (img != without).any(axis=2).sum() > 1500


# ---------------------------------------------------------------- 3. invariance
def _tiles(ctx, mode, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=mode)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("mode", HULL_MODES)
def test_invariance(hip_lib, mode):
    c, hull, V = hull_case("outside")
    options = dict(depth_complexity_max_colour=64, atomic_loop_num_layers=4)   # (mode 5's scale would follow the tiles' maximum)
    ctx = _context(c, hull, **options)
    img = ctx.render(mode)
    frags = int(ctx.stats().fragments)
    assert np.array_equal(ctx.render(mode), img)                               # a second frame is the first
    assert (img != _context(c, None, **options).render(mode)).any(axis=2).sum() > 1500
    tw = th = 16
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid, dtype=np.uint32)
    out = np.zeros_like(img)
    part = 0
    for r in range(4):
        mine = tiles[r::4]
        b = _tiles(ctx, mode, mine, tw, th)
        part += int(ctx.stats().fragments)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img) and part == frags
    # every tile twice and overlapping ones on top: every pixel is counted once
    tiles = np.array(grid * 2 + [(8, 8), (24, 8), (8, 24), (20, 30), (40, 30)], dtype=np.uint32)
    b = _tiles(ctx, mode, tiles, tw, th)
    assert int(ctx.stats().fragments) == frags
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)
    # a one-rank lv_create_multi handle: the mesh and the options reach the rank
    multi = capi.Context(devices=[0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(c.settings)
    multi.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    multi.set_options(dict(hull_opacity=DEFAULT_OPACITY, **options))
    assert np.array_equal(multi.render(mode), img)
    multi.close()


# ---------------------------------------------------------------- 4. no change without the hull
@functools.lru_cache(maxsize=None)
def _tube_mesh(c):
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    return lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)


@pytest.mark.parametrize("mode", [1, 2, 3, 5, 6, 8, 9, 10, 11])
def test_no_change_without_the_hull(hip_lib, mode):
    c, hull, V = hull_case("outside")

    def frame(ctx):
        if mode == 1:
            ctx.set_tube_triangle_mesh(*_tube_mesh(c))
        return ctx.render(mode)

    fresh = frame(c.hip_context())
    assert np.array_equal(frame(_context(c, hull, opacity=None)), fresh)      # hull_opacity never set, a mesh present
    ctx = _context(c, hull, opacity=0)
    assert np.array_equal(frame(ctx), fresh)                                  # hull_opacity = 0, a mesh present
    ctx.set_option("hull_opacity", 0.5)
    ctx.set_hull_mesh(None, None, None)
    assert ctx.get_hull_mesh()[0].shape == (0, 3)
    assert np.array_equal(frame(ctx), fresh)                                  # a removed mesh


# ---------------------------------------------------------------- 5. errors
def test_refused_meshes_leave_the_old_one_drawing(hip_lib):
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull)
    base = ctx.render(capi.MODE_WBOIT)
    idx, pos, nrm = hull.triangle_indices, hull.positions, hull.normals
    got = ctx.get_hull_mesh()
    assert np.array_equal(got[0], idx) and np.array_equal(got[1], pos) and np.array_equal(got[2], nrm)
    bad_idx = idx.copy()
    bad_idx[5, 1] = len(pos)
    bad_pos, bad_nrm = pos.copy(), nrm.copy()
    bad_pos[3, 2] = np.inf
    bad_nrm[7, 0] = np.nan
    for args in ((bad_idx, pos, nrm), (idx, bad_pos, nrm), (idx, pos, bad_nrm)):
        assert _code(lambda: ctx.set_hull_mesh(*args)) == -1
    p = lambda a: a.ctypes.data
    assert ctx.L.lv_set_hull_mesh(ctx.h, p(idx), len(idx), None, p(nrm), len(pos)) == -1
    assert ctx.L.lv_set_hull_mesh(ctx.h, p(idx), len(idx), p(pos), None, len(pos)) == -1
    assert ctx.L.lv_set_hull_mesh(ctx.h, None, len(idx), p(pos), p(nrm), len(pos)) == -1
    assert np.array_equal(ctx.get_hull_mesh()[1], pos)
    assert np.array_equal(ctx.render(capi.MODE_WBOIT), base)
    # malformed option values: the old ones stay
    for key, bad in (("hull_opacity", "1.5"), ("hull_opacity", "-0.1"), ("hull_opacity", "x"), ("hull_color", "0.5 0.5"),
                     ("hull_color", "0.1 0.2 0.3 0.4"), ("hull_color", "0.1 2 0.3"), ("hull_color", "red"), ("hull_use_shading", "yes")):
        assert _code(lambda: ctx.set_option(key, bad)) == -1, (key, bad)
    assert np.array_equal(ctx.render(capi.MODE_WBOIT), base)


def test_modes_without_a_hull_pass(hip_lib):
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull)
    ctx.set_tube_triangle_mesh(*_tube_mesh(c))
    plain = c.hip_context()
    plain.set_tube_triangle_mesh(*_tube_mesh(c))
    for mode in (1, 2, 3, 11):      # not built for the hull yet: refused while one would be drawn, the context stays usable
        assert _code(lambda: ctx.render(mode)) == -1, mode
        message = ctx.L.lv_last_error(ctx.h).decode()
        assert all(word in message for word in ("5", "8", "10", "hull")), message
    ctx.set_option("hull_opacity", 0)
    for mode in (1, 2, 3, 11):
        assert np.array_equal(ctx.render(mode), plain.render(mode)), mode
    ctx.set_option("hull_opacity", DEFAULT_OPACITY)
    for mode in (6, 9):             # the reference draws no hull in these: the same frame with and without the mesh
        assert np.array_equal(ctx.render(mode), plain.render(mode)), mode
    assert (ctx.render(capi.MODE_WBOIT) != plain.render(capi.MODE_WBOIT)).any()


def test_fragment_query_errors(hip_lib):
    c, hull, V = hull_case("outside")
    n = len(reference_fragments("outside")["pixel"])
    ctx = _context(c, hull)
    ctx.render(capi.MODE_WBOIT)
    sums = ctx.wboit_buffers()[0]
    import ctypes
    count = ctypes.c_uint64(0)
    pix = np.zeros(n, np.uint32)
    assert ctx.L.lv_hull_get_fragments(ctx.h, pix.ctypes.data, None, None, None, n - 1, ctypes.byref(count)) == -4 and count.value == n
    assert not pix.any()
    assert ctx.L.lv_hull_get_fragments(ctx.h, pix.ctypes.data, None, None, None, n, ctypes.byref(count)) == 0 and count.value == n
    assert np.array_equal(np.sort(pix), reference_fragments("outside")["pixel"])
    assert np.array_equal(ctx.wboit_buffers()[0], sums)            # the last frame's read-back is untouched
    assert _code(lambda: c.hip_context().hull_fragments()) == -3   # no mesh
    bare = capi.Context(0)
    bare.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    assert _code(bare.hull_fragments) == -3                        # no camera
    # the timer id of the hull pass
    ctx.reset_timers()
    ctx.render(capi.MODE_WBOIT)
    assert len(ctx.kernel_times(capi.KERNEL_HULL)) == 1
    ctx.set_option("hull_opacity", 0)
    ctx.reset_timers()
    ctx.render(capi.MODE_WBOIT)
    assert len(ctx.kernel_times(capi.KERNEL_HULL)) == 0


# ---------------------------------------------------------------- 6. host plugin
@pytest.mark.parametrize("mode", HULL_MODES)
def test_host_plugin(hip_lib, mode):
    """the renderer plugins of modes 5, 8 and 10 upload the data set's outline mesh and forward its settings; the ray tracer's plugin
    uploads none and renders as ever"""
    import ctypes
    from linevis_amd import transfer_function as tfm
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    hull = scenes.box_hull((tr.positions.min(0), tr.positions.max(0)), 3, 0.05)

    def plugin(m, with_hull):
        flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
        if with_hull:
            flow.set_hull_mesh(hull.triangle_indices, hull.positions)     # (no normals: computeSmoothTriangleNormals)
        r = host_api.HeadlessLineRenderer(m)
        r.set_rendering_resolution(120, 80)
        r.set_transfer_function(tfm.standard_transparent())
        r.set_line_data(flow)
        return r, flow

    r, flow = plugin(mode, True)
    assert flow.shall_render_hull
    frame = r.render_frame()
    bare = plugin(mode, False)[0].render_frame()
    assert (frame != bare).any(axis=2).sum() > 1500
    hctx = ctypes.c_void_p(r.L.lvh_renderer_context(r.h))
    L = capi.load()
    nt, nv = ctypes.c_uint32(), ctypes.c_uint32()
    nrm = np.zeros((len(hull.positions), 3), np.float32)
    assert L.lv_get_hull_mesh(hctx, None, 0, None, nrm.ctypes.data, len(nrm), ctypes.byref(nt), ctypes.byref(nv)) == 0
    assert (nt.value, nv.value) == (108, 56) and np.array_equal(nrm, hull.normals)    # the host's smooth normals = scenes.py's
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    assert L.lv_render(hctx, mode, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p)) == 0 and np.array_equal(raw, frame)
    r.set_new_settings({"hull_opacity": 0.0})            # LineData::setNewSettings: the hull goes
    assert not flow.shall_render_hull and np.array_equal(r.render_frame(), bare)
    r.set_new_settings({"hull_opacity": 0.3, "hull_use_shading": False, "hull_color": "0.9 0.1 0.1"})
    other = r.render_frame()
    assert (other != bare).any(axis=2).sum() > 1500 and (mode == capi.MODE_DEPTH_COMPLEXITY or (other != frame).any())
    # a renderer that does not draw the hull uploads no mesh: its frames are not refused
    rt, _ = plugin(capi.MODE_RAY_TRACER, True)
    assert np.array_equal(rt.render_frame(), plugin(capi.MODE_RAY_TRACER, False)[0].render_frame())
