"""The second line primitive on the GPU (lv_linequad.h; include/linevis_hip.h, line_primitive_mode = "Quads (Programmable Pull)"),
through the C-ABI: lv_line_quads_get_fragments bit for bit against the restatement of tests/test_line_quads_restatement.py, the frames
of modes 5, 8 and 10 against the folds of those fragments, tile lists of an odd size, quads together with the hull, the refusals and
the recovery from them, no change without the option in every mode, and the host plugins."""
import ctypes
import functools

import numpy as np
import pytest

from common import Case, max_lsb_diff
from linevis_amd import capi, host_api, scenes
from linevis_amd import transfer_function as tfm
from oracle import lvo
from test_hull_restatement import hull_fragments
from test_line_quads_restatement import frame_references, quad_case, quad_fragments
from test_wboit_restatement import WEIGHTS

pytestmark = pytest.mark.gpu
TUBE, QUADS = "Tube (Programmable Pull)", "Quads (Programmable Pull)"
QUAD_MODES = (capi.MODE_DEPTH_COMPLEXITY, capi.MODE_WBOIT, capi.MODE_ATOMIC_LOOP_64)


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _context(c, primitive=QUADS, **options):
    ctx = c.hip_context()
    if primitive is not None:
        ctx.set_option("line_primitive_mode", primitive)
    ctx.set_options(options)
    return ctx


def _sorted_fragments(ctx):
    pix, seg, tri, z, rgba = ctx.line_quad_fragments()
    order = np.lexsort((tri, seg, pix))
    return pix[order], seg[order], tri[order], z[order], rgba[order]


def _device_reference(c, V, ctx):
    """the restatement on what the frame's lighting read: the device's own AO image and depth range (inputs of the fragment stage that
    older kernels compute), where the case's settings switch them on"""
    s = c.settings
    ao = ctx.get_ao() if s.get("ambient_occlusion_mode", "None") != "None" else None
    rng = ctx.depth_range() if float(s.get("depth_cue_strength", 0.0)) > 0.0 else None
    return quad_fragments(c, V, ao=ao, depth_range=rng)


# ---------------------------------------------------------------- 1. the fragments, bit for bit
@pytest.mark.parametrize("kind", ["plain", "odd", "wide", "thin", "cues"])
def test_fragments_bit_for_bit(hip_lib, kind):
    c, V = quad_case(kind)
    ctx = _context(c)
    ctx.render(capi.MODE_WBOIT)
    pix, seg, tri, z, rgba = _sorted_fragments(ctx)
    want = _device_reference(c, V, ctx)
    assert len(pix) == len(want["pixel"]) > (100 if kind == "thin" else 400)
    assert np.array_equal(pix, want["pixel"]) and np.array_equal(seg, want["seg"]) and np.array_equal(tri, want["tri"])
    assert np.array_equal(z.view(np.uint32), want["zbits"])
    diff = float(np.abs(rgba.astype(np.float64) - want["rgba"].astype(np.float64)).max())
    print("line quads %s: %d fragments, largest float32 colour difference %.3g" % (kind, len(pix), diff))
    assert np.array_equal(rgba.view(np.uint32), want["rgba"].view(np.uint32))
    if kind == "cues":       # the depth cues and the AO image reach the colours: against the same scene without them, and without the image
        plain = quad_fragments(*quad_case("plain"))
        assert np.array_equal(plain["zbits"], want["zbits"]) and (plain["rgba"][:, :3] != want["rgba"][:, :3]).any(axis=1).sum() > 600
        no_image = quad_fragments(c, V, depth_range=ctx.depth_range())
        assert (no_image["rgba"][:, :3] != want["rgba"][:, :3]).any(axis=1).sum() > 100
    # the same list after a mode-5 and a mode-10 frame, and a second call is the first
    for mode in (capi.MODE_DEPTH_COMPLEXITY, capi.MODE_ATOMIC_LOOP_64):
        ctx.render(mode)
        again = _sorted_fragments(ctx)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, (pix, seg, tri, z, rgba))), mode


# ---------------------------------------------------------------- 2. whole frames
@functools.lru_cache(maxsize=None)
def _references(kind, K, weight="reference"):
    c, V = quad_case(kind)
    return frame_references(c, quad_fragments(c, V), K=K, weight=weight)


def test_mode_5_counts_the_quad_fragments(hip_lib):
    c, V = quad_case("wide")
    ref = _references("wide", 2)["dc"]
    ctx = _context(c, collect_stats=True)
    img = ctx.render(capi.MODE_DEPTH_COMPLEXITY)
    counts = ctx.depth_complexity_buffers()
    st = ctx.depth_complexity_stats()
    stats = ctx.stats()
    assert np.array_equal(counts, ref[1]) and counts.max() > 2
    assert st["total"] == int(counts.sum()) == int(stats.fragments) == int(stats.hits_shaded) and st["max"] == int(counts.max())
    assert st["used_locations"] == int((counts > 0).sum())
    assert max_lsb_diff(img, ref[0]) <= 2


@pytest.mark.parametrize("weight", WEIGHTS)
def test_mode_8_adds_the_quad_fragments(hip_lib, weight):
    c, V = quad_case("wide")
    ref = _references("wide", 2, weight)["wboit"]
    ctx = _context(c, wboit_depth_weight=weight)
    img = ctx.render(capi.MODE_WBOIT)
    sums, counts = ctx.wboit_buffers()
    assert np.array_equal(counts, ref[2]) and int(ctx.stats().fragments) == int(ref[2].sum())
    assert np.array_equal(sums, ref[1])
    assert max_lsb_diff(img, ref[0]) <= 2
    tubes = _context(c, TUBE, wboit_depth_weight=weight).render(capi.MODE_WBOIT)
    assert (img != tubes).any(axis=2).sum() > 300


def test_mode_10_slots_and_tail(hip_lib):
    """K = 2 on a scene with more than two layers: the tail is exercised"""
    c, V = quad_case("wide")
    ref = _references("wide", 2)["al64"]
    assert ref[3].max() > 2 and (ref[2][..., 0] != 0).sum() > 50
    ctx = _context(c, atomic_loop_num_layers=2)
    img = ctx.render(capi.MODE_ATOMIC_LOOP_64)
    slots, tail = ctx.atomic_loop_buffers()
    assert np.array_equal(slots, ref[1]) and np.array_equal(tail, ref[2])
    assert int(ctx.stats().fragments) == int(ref[3].sum())
    assert max_lsb_diff(img, ref[0]) <= 2
    # the default K holds every fragment of this scene's pixels or not: either way the frame is the fold
    ref8 = _references("wide", 8)["al64"]
    ctx.set_option("atomic_loop_num_layers", 8)
    assert max_lsb_diff(ctx.render(capi.MODE_ATOMIC_LOOP_64), ref8[0]) <= 2
    assert np.array_equal(ctx.atomic_loop_buffers()[0], ref8[1])


# ---------------------------------------------------------------- 3. odd tile sizes and tile lists
def _tiles(ctx, mode, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=mode)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("mode", QUAD_MODES)
def test_two_disjoint_tile_lists_reproduce_the_frame(hip_lib, mode):
    c, V = quad_case("wide")
    options = dict(depth_complexity_max_colour=16, atomic_loop_num_layers=2)   # (mode 5's scale would follow the tiles' maximum)
    ctx = _context(c, **options)
    img = ctx.render(mode)
    frags = int(ctx.stats().fragments)
    tw, th = 13, 11                                 # neither divides 70 x 45, nor is a multiple of 8
    tiles = np.array([(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)], dtype=np.uint32)
    out = np.zeros_like(img)
    part = 0
    for mine in (tiles[0::2], tiles[1::2]):
        b = _tiles(ctx, mode, mine, tw, th)
        part += int(ctx.stats().fragments)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img) and part == frags          # byte for byte; count for count
    # a one-rank lv_create_multi handle: the option reaches the rank
    multi = capi.Context(devices=[0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(dict(line_primitive_mode=QUADS, **options))
    assert np.array_equal(multi.render(mode), img)
    multi.close()


# ---------------------------------------------------------------- 4. quads together with the hull
def test_quads_together_with_the_hull(hip_lib):
    c, V = quad_case("plain")
    pts = c.points["linePosition"]
    hull = scenes.box_hull((pts.min(0), pts.max(0)), 3, 0.05)
    want_hull = hull_fragments(hull, V)
    want = quad_fragments(c, V)
    ctx = _context(c, hull_opacity=0.3, atomic_loop_num_layers=4)
    ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    frames = {mode: ctx.render(mode) for mode in QUAD_MODES}
    # the fragments are the union: each list is its restatement
    pix, seg, tri, z, rgba = _sorted_fragments(ctx)
    assert np.array_equal(pix, want["pixel"]) and np.array_equal(rgba.view(np.uint32), want["rgba"].view(np.uint32))
    hp, ht, hz, hrgba = ctx.hull_fragments()
    order = np.lexsort((ht, hp))
    assert np.array_equal(hp[order], want_hull["pixel"]) and np.array_equal(hz[order].view(np.uint32), want_hull["zbits"])
    assert len(hp) > 2000 and len(pix) > 400
    # the frames are the folds of both lists (the hull's colours: the device's own, its shading is compared within 2 LSB elsewhere)
    ref = frame_references(c, want, K=4, hull=dict(want_hull, rgba=hrgba[order]))
    assert np.array_equal(ref["dc"][1], ref["wboit"][2]) and ref["dc"][1].max() >= 3
    for mode, name in zip(QUAD_MODES, ("dc", "wboit", "al64")):
        assert max_lsb_diff(frames[mode], ref[name][0]) <= 2, name
    ctx.render(capi.MODE_WBOIT)
    sums, counts = ctx.wboit_buffers()
    assert np.array_equal(sums, ref["wboit"][1]) and np.array_equal(counts, ref["wboit"][2])
    ctx.render(capi.MODE_DEPTH_COMPLEXITY)
    assert np.array_equal(ctx.depth_complexity_buffers(), ref["dc"][1])
    ctx.render(capi.MODE_ATOMIC_LOOP_64)
    slots, tail = ctx.atomic_loop_buffers()
    assert np.array_equal(slots, ref["al64"][1]) and np.array_equal(tail, ref["al64"][2])


# ---------------------------------------------------------------- 5. refusals and recovery
def test_refusals_and_recovery(hip_lib):
    c, V = quad_case("plain")
    ctx = _context(c, TUBE)
    tube = {mode: ctx.render(mode) for mode in (2, 3, 5, 6, 8, 9, 10)}
    ctx.set_option("line_primitive_mode", QUADS)
    quads = {mode: ctx.render(mode) for mode in QUAD_MODES}
    assert all((quads[mode] != tube[mode]).any() for mode in QUAD_MODES)
    for mode in (2, 3, 6, 9):
        assert _code(lambda: ctx.render(mode)) == -1, mode
        message = ctx.L.lv_last_error(ctx.h).decode()
        assert all(word in message for word in ("5", "8", "10", "Quads")), message
    # the read-back entry point after a refused frame, and after a tube frame of another mode: no such frame
    assert _code(ctx.line_quad_fragments) == -3
    for key, value in (("use_ribbons", True), ("rotating_helicity_bands", True), ("ambient_occlusion_mode", "RTAO (Prebaker)"),
                       ("ppll_fragment_source", "capsule_entry"), ("ppll_prism_rasteriser", "lbvh")):
        ctx.set_option(key, value)
        for mode in QUAD_MODES:
            assert _code(lambda: ctx.render(mode)) == -1, (key, mode)
        ctx.set_option(key, {"use_ribbons": False, "rotating_helicity_bands": False, "ambient_occlusion_mode": "None",
                             "ppll_fragment_source": "auto", "ppll_prism_rasteriser": "segments"}[key])
    # every other name of the reference's list: not built, the value in force stays
    for name in host_api.LINE_PRIMITIVE_MODE_NAMES:
        if name not in (TUBE, QUADS):
            assert _code(lambda: ctx.set_option("line_primitive_mode", name)) == -1, name
            assert "not built" in ctx.L.lv_last_error(ctx.h).decode()
    assert _code(lambda: ctx.set_option("line_primitive_mode", "Quads")) == -1
    # the context stays usable: quads -> tubes -> quads reproduces both frames, in every mode
    for mode in QUAD_MODES:
        assert np.array_equal(ctx.render(mode), quads[mode]), mode
    ctx.set_option("line_primitive_mode", TUBE)
    for mode in (2, 3, 5, 6, 8, 9, 10):
        assert np.array_equal(ctx.render(mode), tube[mode]), mode
    ctx.render(2)
    assert _code(ctx.line_quad_fragments) == -3           # after a mode-2 frame
    ctx.render(capi.MODE_WBOIT)
    assert _code(ctx.line_quad_fragments) == -3           # after a tube frame of mode 8
    ctx.set_option("line_primitive_mode", QUADS)
    for mode in QUAD_MODES:
        assert np.array_equal(ctx.render(mode), quads[mode]), mode
    # too small: the count comes back, nothing else is written, the last frame's read-back is untouched
    slots = ctx.atomic_loop_buffers()[0]
    n = len(quad_fragments(c, V)["pixel"])
    count = ctypes.c_uint64(0)
    pix = np.zeros(n, np.uint32)
    assert ctx.L.lv_line_quads_get_fragments(ctx.h, n - 1, pix.ctypes.data, None, None, None, None, ctypes.byref(count)) == -4
    assert count.value == n and not pix.any()
    assert ctx.L.lv_line_quads_get_fragments(ctx.h, n, pix.ctypes.data, None, None, None, None, ctypes.byref(count)) == 0
    assert np.array_equal(np.sort(pix), quad_fragments(c, V)["pixel"]) and np.array_equal(ctx.atomic_loop_buffers()[0], slots)
    assert _code(c.hip_context().line_quad_fragments) == -3   # no frame at all


def test_read_back_refuses_what_is_no_longer_the_frames(hip_lib):
    """The read-back evaluates the pass again on the context's resident line data and AO image: when those are not the frame's any more
    it answers -3, it does not read them"""
    c, V = quad_case("cues")
    n = len(quad_fragments(c, V)["pixel"])

    def fresh():
        ctx = _context(c)
        ctx.render(capi.MODE_WBOIT)
        assert len(ctx.line_quad_fragments()[0]) == n
        return ctx

    # more line data after the frame (the leaf-ordered records still have the old size)
    big, _ = quad_case("plain")
    ctx = fresh()
    more_points = np.concatenate([big.points, big.points])
    more_seg = np.concatenate([big.seg, big.seg + len(big.points)])
    ctx.set_lines(more_points, more_seg)
    assert _code(ctx.line_quad_fragments) == -3
    ctx.render(capi.MODE_WBOIT)
    assert len(ctx.line_quad_fragments()[0]) > n              # (every quad twice now)
    # the same number of segments, other lines
    ctx.set_lines(more_points[::-1].copy(), more_seg)
    assert _code(ctx.line_quad_fragments) == -3
    # a larger viewport after the frame (the AO image has the old size)
    ctx = fresh()
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, 2 * c.width, 2 * c.height)
    assert _code(ctx.line_quad_fragments) == -3
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    assert len(ctx.line_quad_fragments()[0]) == n             # back at the frame's size: the frame's answer
    # a line width changed after the frame
    ctx.set_option("line_width", 2 * c.line_width)
    assert _code(ctx.line_quad_fragments) == -3
    # the AO image switched on after a frame drawn without it, and off after a frame drawn with it
    plain, _ = quad_case("plain")
    ctx = _context(plain)
    ctx.render(capi.MODE_ATOMIC_LOOP_64)
    ctx.set_options(dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=0.6))
    assert _code(ctx.line_quad_fragments) == -3
    ctx = fresh()
    ctx.set_option("ambient_occlusion_strength", 0.0)
    assert _code(ctx.line_quad_fragments) == -3
    # a tile-list frame does not qualify
    ctx = fresh()
    tiles = np.array([(0, 0), (16, 16)], dtype=np.uint32)
    _tiles(ctx, capi.MODE_WBOIT, tiles, 16, 16)
    assert _code(ctx.line_quad_fragments) == -3
    ctx.render(capi.MODE_WBOIT)
    assert len(ctx.line_quad_fragments()[0]) == n


# ---------------------------------------------------------------- 6. no change without the option
@functools.lru_cache(maxsize=None)
def _tube_mesh():
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    return lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, 0.02, 6)


@pytest.mark.parametrize("mode", [1, 2, 3, 5, 6, 8, 9, 10, 11])
def test_no_change_without_the_option(hip_lib, mode):
    c, V = quad_case("plain")

    def frame(ctx):
        if mode == 1:
            ctx.set_tube_triangle_mesh(*_tube_mesh())
        return ctx.render(mode)

    fresh = frame(_context(c, None))                       # a context that never set the option
    assert np.array_equal(frame(_context(c, TUBE)), fresh)
    if mode in (1, 11):                                    # these never read the primitive mode
        assert np.array_equal(frame(_context(c, QUADS)), fresh)


# ---------------------------------------------------------------- 7. host plugin
@pytest.mark.parametrize("mode", QUAD_MODES)
def test_host_plugin(hip_lib, mode):
    """the plugins of modes 5, 8 and 10 driven with line_primitive_mode = "Quads (Programmable Pull)" give the C-ABI frame"""
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    tf = tfm.standard_transparent()
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    r = host_api.HeadlessLineRenderer(mode)
    r.set_rendering_resolution(70, 45)
    r.set_transfer_function(tf)
    r.set_line_data(flow)
    r.set_new_settings(dict(line_width=0.02))
    try:
        tubes = r.render_frame()
        r.set_new_settings(dict(line_primitive_mode=QUADS))
        assert flow.line_primitive_mode == QUADS
        img = r.render_frame()
        assert (img != tubes).any()
        pts, seg, _ = flow.tube_aabb_render_data(0.02)
        lo, hi = flow.attribute_range()
        c = Case(pts, seg, tf, 70, 45, 0.02, use_capped_tubes=False)
        view, proj, fovy, near, far = r.camera()
        for primitive, want in ((QUADS, img), (TUBE, tubes)):
            ctx = _context(c, primitive)
            ctx.set_transfer_function(tf, lo, hi)
            ctx.set_camera(view, proj, fovy, near, far, 70, 45)
            assert np.array_equal(ctx.render(mode), want), primitive
        r.set_new_settings(dict(line_primitive_mode=TUBE))
        assert np.array_equal(r.render_frame(), tubes)
    finally:
        flow.set_new_settings({"line_primitive_mode": TUBE})   # (a static member, as in the reference)
