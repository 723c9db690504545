"""The simulation-mesh hull in the pooled modes 2 and 3 on the GPU (hull_fragment_pool = on; linevis_amd/csrc/lv_hull_pool.h): the
refusal kept and the switch; mode 2's lists and frames against the union of the oracle's lists and the restated hull nodes
(tests/test_hull_pool_restatement.py), also where pixels hold more fragments than the sort arrays; mode 3's frames against the fold
of the union; pool regrowth; the 16-bit per-pixel count; invariance under tile lists, a one-rank handle and the tile sizes of the
addressing; the restrictions; the host plugins.  Every test here needs the option key."""
import functools

import numpy as np
import pytest

from common import Case, max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from linevis_amd import transfer_function as tfm
from oracle import lvo
from test_deferred_restatement import View
from test_hull_pool_restatement import END, hull_nodes, list_entries, mlab_union, ppll_union
from test_hull_restatement import DEFAULT_OPACITY, F, hull_case, hull_fragments, reference_fragments
from test_mlab_restatement import mlab_fold

pytestmark = pytest.mark.gpu
QUADS = "Quads (Programmable Pull)"


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _context(c, hull, opacity=DEFAULT_OPACITY, pool="on", **options):
    ctx = c.hip_context()
    if hull is not None:
        ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    if opacity is not None:
        ctx.set_option("hull_opacity", opacity)
    if pool is not None:
        ctx.set_option("hull_fragment_pool", pool)
    ctx.set_options(options)
    return ctx


def _device_colours(ctx, fr):
    """the device's own hull colours in the order of the restated fragments (sorted by pixel, triangle)"""
    pix, tri, z, rgba = ctx.hull_fragments()
    order = np.lexsort((tri, pix))
    assert np.array_equal(pix[order], fr["pixel"]) and np.array_equal(tri[order], fr["tri"])
    assert np.array_equal(z[order].view(np.uint32), fr["zbits"])
    return rgba[order]


def _channels(packed):
    return np.stack([(packed >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=-1).astype(np.int32)


# ---------------------------------------------------------------- 1. the refusal kept, the switch
def test_refusal_kept_and_the_switch(hip_lib):
    c, hull, V = hull_case("outside")
    for pool in (None, "off"):
        ctx = _context(c, hull, pool=pool)
        for mode in (2, 3):
            assert _code(lambda: ctx.render(mode)) == -1, (pool, mode)
            message = ctx.L.lv_last_error(ctx.h).decode()
            assert all(word in message for word in ("5", "8", "10", "hull")), message
    ctx = _context(c, hull)
    assert _code(lambda: ctx.set_option("hull_fragment_pool", "maybe")) == -1     # malformed: the old value stays
    assert _code(lambda: ctx.set_option("hull_fragment_pool", "")) == -1
    plain = c.hip_context()
    for mode in (2, 3):
        assert (ctx.render(mode) != plain.render(mode)).any(axis=2).sum() > 1500, mode
    assert np.array_equal(ctx.render(6), plain.render(6))                          # pooled mode 6 draws none, as the reference
    assert _code(lambda: ctx.render(11)) == -1                                     # mode 11 has its own switch
    ctx.set_option("hull_fragment_pool", "off")
    assert _code(lambda: ctx.render(2)) == -1
    ctx.set_option("hull_fragment_pool", "on")
    ctx.set_option("hull_opacity", 0)
    for mode in (2, 3, 6, 8, 11):                                                  # on, no hull drawn: a context that never saw a mesh
        assert np.array_equal(ctx.render(mode), plain.render(mode)), mode


# ---------------------------------------------------------------- 2. mode 2: the lists
@pytest.mark.parametrize("kind", ["outside", "odd", "inside", "strip"])
def test_mode_2_lists_hold_the_union(hip_lib, kind):
    c, hull, V = hull_case(kind)
    fr = reference_fragments(kind)
    ctx = _context(c, hull)
    img = ctx.render(2)
    frags = int(ctx.stats().fragments)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    pw, ph = c.padded()
    hn, hs, hcnt = ctx.ppll_buffers(pw * ph, int(P.ppllLinkedListSize))
    on, os_, ocnt = sc.ppll_gather(P, use_bvh=True)
    la, lc, ld = list_entries(on, os_)
    ha, hc, hd = hull_nodes(c, P, fr)
    assert len(ha) == int((fr["rgba"][:, 3] >= F(0.001)).sum()) > 500
    addr, col, dep = np.concatenate([la, ha]), np.concatenate([lc, hc]), np.concatenate([ld, hd])
    is_hull = np.concatenate([np.zeros(len(la), bool), np.ones(len(ha), bool)])
    order = np.lexsort((col, dep, addr))
    addr, col, dep, is_hull = addr[order], col[order], dep[order], is_hull[order]
    ga, gc, gd = list_entries(hn, hs)
    order = np.lexsort((gc, gd, ga))
    ga, gc, gd = ga[order], gc[order], gd[order]
    # per pixel the multiset of (depth bits, colour): line nodes as whole words, hull nodes in the depth bits exactly and in the packed
    # colour within the project's +- 2 LSB per channel
    assert len(ga) == len(addr) == frags and np.array_equal(ga, addr) and np.array_equal(gd, dep)
    assert np.array_equal(gc[~is_hull], col[~is_hull])
    assert np.abs(_channels(gc[is_hull]) - _channels(col[is_hull])).max() <= 2
    want = ppll_union(c, fr)[2]
    assert max_lsb_diff(img, want) <= 2
    # the union with the device's OWN hull colours: the lists and the frame byte for byte
    un, us, own = ppll_union(c, fr, hull_rgba=_device_colours(ctx, fr))
    ua, uc, ud = list_entries(un, us)
    order = np.lexsort((uc, ud, ua))
    assert np.array_equal(uc[order], gc) and np.array_equal(ud[order], gd)
    assert np.array_equal(img, own)
    assert np.array_equal(lvo.ppll_resolve(P, hn, hs), img)
    assert np.array_equal(ctx.render(2), img)


# ---------------------------------------------------------------- 3. mode 2 under pressure
@functools.lru_cache(maxsize=None)
def _dense():
    c = small_case(width=176, height=120, n_lines=60, pts_per_line=40, line_width=0.02, transparent=True, ppll_max_num_frags=8)
    pts = c.points["linePosition"]
    hull = scenes.box_hull((pts.min(0), pts.max(0)), 3, 0.05)
    return c, hull, hull_fragments(hull, View(c))


@pytest.mark.parametrize("sorting", ["Priority Queue", "Bitonic Sort", "Quicksort"])
def test_mode_2_with_more_fragments_than_the_sort_arrays(hip_lib, sorting):
    """ppll_max_num_frags = 8 on a line set dense enough that pixels overflow: the nearest 8 of lines AND hull are kept"""
    c, hull, fr = _dense()
    c.settings["sorting_mode"] = sorting
    ctx = _context(c, hull)
    img = ctx.render(2)
    un, us, own = ppll_union(c, fr, hull_rgba=_device_colours(ctx, fr))
    ua, uc, ud = list_entries(un, us)
    depth = np.bincount(ua)
    assert depth.max() > 8                                                          # pixels overflow the sort arrays
    assert np.array_equal(img, own)
    assert np.array_equal(ctx.render(2), img)


# ---------------------------------------------------------------- 4. mode 3
@pytest.mark.parametrize("K", [8, 2])
def test_mode_3_folds_the_union(hip_lib, K):
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    ctx = _context(c, hull, mlab_num_layers=K)
    img = ctx.render(3)
    frags = int(ctx.stats().fragments)
    runs, want = mlab_union(c, fr, K)
    assert frags == sum(len(r[0]) for r in runs)
    assert max_lsb_diff(img, want) <= 2
    runs, own = mlab_union(c, fr, K, hull_rgba=_device_colours(ctx, fr))
    assert np.array_equal(img, own)
    # the device's fold of the same runs (lv_mlab_resolve_buffers)
    off = np.zeros(len(runs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r[0]) for r in runs])
    e = np.zeros((int(off[-1]), 3), np.uint32)
    e[:, 0], e[:, 1], e[:, 2] = (np.concatenate([np.asarray(r[k]).view(np.uint32) for r in runs]) for k in range(3))
    assert np.array_equal(ctx.mlab_resolve(e, off, c.width, c.height), img)
    if K == 2:
        # the key order is exercised: pixels whose hull fragments arrive when the K layers are taken fold them into the merged last layer
        base = np.uint32(len(c.seg) << 6)
        merged = sum(1 for r in runs if len(r[0]) > K and (np.asarray(r[2]) >= base).any())
        assert merged > 200
    assert np.array_equal(ctx.render(3), img)


# ---------------------------------------------------------------- 5. regrowth
def test_mode_3_pool_regrowth_with_the_hull(hip_lib):
    c, hull, V = hull_case("outside")
    pw, ph = c.padded()
    small = _context(c, hull, ppll_expected_avg_depth_complexity=1, collect_stats=True)
    large = _context(c, hull, collect_stats=True)
    img = small.render(3)
    st = small.stats()
    assert int(st.ppll_pool_nodes) > pw * ph                                        # grown: it started at one slot per pixel
    assert np.array_equal(img, large.render(3))
    ref = large.stats()
    assert int(ref.ppll_pool_nodes) == 20 * pw * ph
    for f in ("rays_traced", "prims_tested", "hits_shaded", "fragments"):           # the front end counted once
        assert getattr(st, f) == getattr(ref, f) and getattr(st, f) > 0, f
    assert np.array_equal(small.render(3), img) and small.stats().ppll_pool_nodes == st.ppll_pool_nodes


# ---------------------------------------------------------------- 6. the 16-bit per-pixel count
def _stack_of_triangles(n):
    """n triangles stepped in depth, each covering the whole of a 4 x 4 viewport; normals across the view, so that alpha is the opacity"""
    z = (-0.2 + 6e-6 * np.arange(n)).astype(np.float32)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, 0] = (-10.0, -10.0, 0.0)
    pos[:, 1] = (10.0, -10.0, 0.0)
    pos[:, 2] = (0.0, 10.0, 0.0)
    pos[:, :, 2] = z[:, None]
    nrm = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (3 * n, 1))
    return scenes.HullMesh(np.arange(3 * n, dtype=np.uint32).reshape(n, 3), pos.reshape(-1, 3), nrm)


def _list_lengths(nodes, start):
    cur = start[start != END].astype(np.int64)
    n = np.zeros(len(cur), np.int64)
    live = np.ones(len(cur), bool)
    while live.any():
        n[live] += 1
        nxt = nodes[cur[live], 2].astype(np.int64)
        cur[live] = nxt
        live[live] = nxt != END
    return n


def test_16_bit_count_saturates(hip_lib):
    """66 000 hull triangles on every pixel of a 4 x 4 viewport, one short line outside the view: a capacity condition of the format.
    The rasteriser's rule (ranks 0 ... 65 534 are stored, the full-word add is undone from then on) leaves 65 535 stored fragments per
    pixel, the highest rank 65 535 - 1 = 65 534, exactly as tests/test_prism_raster.py finds for line fragments; mode 2 drops the
    rest and counts them, mode 3 returns LV_E_CAPACITY and the context stays usable."""
    n = 66000
    pts = np.zeros(2, dtype=lvo.LINE_POINT_DTYPE)
    pts["linePosition"][:, 0] = (50.0, 50.1)
    pts["lineTangent"][:, 0] = 1.0
    pts["lineNormal"][:, 1] = 1.0
    c = Case(pts, np.array([(0, 1)], np.uint32), tfm.standard_transparent(), 4, 4, 0.02, ppll_expected_avg_depth_complexity=70000)
    hull = _stack_of_triangles(n)
    ctx = _context(c, hull, opacity=0)
    empty = ctx.render(2)
    assert int(ctx.stats().fragments) == 0
    ctx.set_option("hull_opacity", DEFAULT_OPACITY)
    assert _code(lambda: ctx.render(3)) == -4
    ctx.set_option("hull_opacity", 0)
    assert np.array_equal(ctx.render(3), empty)                                     # the context stays usable
    ctx.set_option("hull_opacity", DEFAULT_OPACITY)
    img = ctx.render(2)
    assert int(ctx.stats().fragments) == 16 * n
    pw, ph = c.padded()
    hn, hs, hcnt = ctx.ppll_buffers(pw * ph, 0)
    lengths = _list_lengths(hn, hs)
    assert len(lengths) == 16 and np.all(lengths == 65535)
    assert (img != empty).any(axis=2).all()
    assert np.array_equal(ctx.render(2), img)


# ---------------------------------------------------------------- 7. invariance
def _tiles(ctx, mode, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=mode)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("mode", [2, 3])
def test_invariance(hip_lib, mode):
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull)
    img = ctx.render(mode)
    frags = int(ctx.stats().fragments)
    assert np.array_equal(ctx.render(mode), img)                                    # a second frame is the first
    assert (img != c.hip_context().render(mode)).any(axis=2).sum() > 1500
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
    # every tile twice and overlapping ones on top: every pixel is stored once
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
    multi.set_options(dict(hull_opacity=DEFAULT_OPACITY, hull_fragment_pool="on"))
    assert np.array_equal(multi.render(mode), img)
    multi.close()
    # the tile sizes of the per-pixel addressing
    for tile in ((1, 1), (2, 8), (8, 8)):
        ctx.set_options(dict(ppll_tile_width=tile[0], ppll_tile_height=tile[1]))
        assert np.array_equal(ctx.render(mode), img), tile


# ---------------------------------------------------------------- 8. restrictions
def test_restrictions(hip_lib):
    """The hull store fills the segment rasteriser's pool only.  (The key rule of mode 3, (segments << 6) + hull triangles <= 0xFFFFFFFE,
    cannot be reached without a scene of 2^26 segments: lv_hull_pool_keys_fit in lv_hull_pool.h, called by lv_frame_check, is left to
    code reading.)"""
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull)
    base = {mode: ctx.render(mode) for mode in (2, 3)}
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto"),
                             ("line_primitive_mode", QUADS, "Tube (Programmable Pull)")):
        ctx.set_option(key, value)
        for mode in (2, 3):
            assert _code(lambda: ctx.render(mode)) == -1, (key, mode)
            message = ctx.L.lv_last_error(ctx.h).decode()
            if mode == 3 and key == "ppll_fragment_source":   # (mode 3 never takes capsule_entry: that older refusal comes first)
                assert "capsule_entry is not supported" in message, message
            else:
                assert "hull_fragment_pool" in message and "segment rasteriser" in message, message
        ctx.set_option(key, back)
        for mode in (2, 3):
            assert np.array_equal(ctx.render(mode), base[mode]), (key, mode)
    # without a drawn hull the other rasteriser is as available as ever
    ctx.set_options(dict(hull_opacity=0, ppll_prism_rasteriser="lbvh"))
    assert np.array_equal(ctx.render(2), c.hip_context().render(2))


# ---------------------------------------------------------------- 9. host plugins
@pytest.mark.parametrize("mode", [2, 3])
def test_host_plugin(hip_lib, mode):
    """the plugins of modes 2 and 3 upload the data set's outline mesh and forward its settings under hull_fragment_pool = on; without
    the key they upload none and render as ever"""
    import ctypes
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    hull = scenes.box_hull((tr.positions.min(0), tr.positions.max(0)), 3, 0.05)

    def plugin(settings):
        flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
        flow.set_hull_mesh(hull.triangle_indices, hull.positions)     # (no normals: computeSmoothTriangleNormals)
        r = host_api.HeadlessLineRenderer(mode)
        r.set_rendering_resolution(120, 80)
        r.set_transfer_function(tfm.standard_transparent())
        r.set_line_data(flow)
        if settings:
            r.set_new_settings(settings)
        return r, flow

    L = capi.load()
    nt, nv = ctypes.c_uint32(), ctypes.c_uint32()
    r, flow = plugin({"hull_fragment_pool": "on"})
    assert flow.shall_render_hull
    frame = r.render_frame()
    rb = plugin({})[0]
    bare = rb.render_frame()
    assert (frame != bare).any(axis=2).sum() > 1500
    hctx = ctypes.c_void_p(r.L.lvh_renderer_context(r.h))
    nrm = np.zeros((len(hull.positions), 3), np.float32)
    assert L.lv_get_hull_mesh(hctx, None, 0, None, nrm.ctypes.data, len(nrm), ctypes.byref(nt), ctypes.byref(nv)) == 0
    assert (nt.value, nv.value) == (108, 56) and np.array_equal(nrm, hull.normals)
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    assert L.lv_render(hctx, mode, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p)) == 0 and np.array_equal(raw, frame)
    bctx = ctypes.c_void_p(rb.L.lvh_renderer_context(rb.h))
    assert L.lv_get_hull_mesh(bctx, None, 0, None, None, 0, ctypes.byref(nt), ctypes.byref(nv)) == 0 and nt.value == 0
    r.set_new_settings({"hull_opacity": 0.0})            # LineData::setNewSettings: the hull goes
    assert not flow.shall_render_hull and np.array_equal(r.render_frame(), bare)
    r.set_new_settings({"hull_opacity": 0.3, "hull_use_shading": False, "hull_color": "0.9 0.1 0.1"})
    other = r.render_frame()
    assert (other != bare).any(axis=2).sum() > 1500 and (other != frame).any()
    r.set_new_settings({"hull_fragment_pool": "off"})    # switched off again: nothing draws the uploaded mesh, nothing is refused
    assert np.array_equal(r.render_frame(), bare)
