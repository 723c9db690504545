"""Rendering mode 5 (depth complexity) on the GPU: the counts against the oracle's run lengths and against mode 8's counts on the
same context (which pins lv_prism_frag_kept to the `kept` of lv_shade_prism), the frame byte for byte against
depth_complexity_frame (test_depth_peeling_restatement.py) in auto and with an explicit depth_complexity_max_colour, the device-side
statistics, tile lists, the stacked scene, band data and helicity bands, a one-rank multi handle, errors and the host plugin."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from test_depth_peeling_restatement import depth_complexity_frame
from test_gpu_mlab import _stacked_case

pytestmark = pytest.mark.gpu
MODE = capi.MODE_DEPTH_COMPLEXITY


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _same(img, ref):
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


def oracle_counts(c):
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    off = sc.prism_fragments(P)["offsets"].astype(np.int64)
    return np.diff(off).reshape(c.height, c.width).astype(np.uint32)


def _stats_of(counts):
    return {"total": int(counts.sum(dtype=np.uint64)), "used_locations": int((counts > 0).sum()), "max": int(counts.max()),
            "min": int(counts.min()), "buffer_size": int(counts.size)}


def _frame_checks(c, ctx, counts, least_covered=100):
    assert int(counts.sum()) > 500 and int((counts > 0).sum()) > least_covered and int(counts.max()) >= 3
    frames = []
    for max_colour in (0, 3, max(int(counts.max()) // 2, 1), 700):
        ctx.set_option("depth_complexity_max_colour", max_colour)
        img = ctx.render(MODE)
        _same(img, depth_complexity_frame(counts, c.background, max_colour).reshape(c.height, c.width, 4))
        assert np.array_equal(ctx.depth_complexity_buffers(), counts)
        assert ctx.depth_complexity_stats() == _stats_of(counts)
        st = ctx.stats()
        assert int(st.fragments) == int(counts.sum()) and int(st.ppll_pool_nodes) == 0 and int(st.max_depth_complexity) == int(counts.max())
        assert np.array_equal(ctx.render(MODE), img)   # two renders in a row
        frames.append(img)
    assert not np.array_equal(frames[1], frames[3])   # the scale shows
    ctx.set_option("depth_complexity_max_colour", 0)
    return frames[0]


@functools.lru_cache(maxsize=None)
def _small():
    return small_case(width=120, height=80, transparent=True)


def test_counts_frame_and_statistics(hip_lib):
    c = _small()
    ctx = c.hip_context()
    counts = oracle_counts(c)
    _frame_checks(c, ctx, counts)
    ctx.render(8)
    assert np.array_equal(ctx.wboit_buffers()[1], counts)   # what the shading stage keeps, on the same context
    ctx.render(MODE)
    assert np.array_equal(ctx.depth_complexity_buffers(), counts)


def test_frame_with_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    c = band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8)
    _frame_checks(c, c.hip_context(), oracle_counts(c))


def test_frame_with_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    c = helicity_case(width=120, height=90, transparent=True)[0]
    _frame_checks(c, c.hip_context(), oracle_counts(c))


@pytest.mark.parametrize("cam", ["roll37", "lens_shift", "inside_rolled"])
def test_counts_under_general_cameras(hip_lib, cam):
    from test_gpu_cameras import cam_case
    c = cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
    c.settings["collect_stats"] = True   # (the count pass's statistics counters run too)
    ctx = c.hip_context()
    _frame_checks(c, ctx, oracle_counts(c))
    ctx.close()


def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=MODE)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_stacked_scene_tile_lists_and_a_one_rank_handle(hip_lib):
    c = _stacked_case()
    ctx = c.hip_context()
    counts = oracle_counts(c)
    assert int(counts.max()) > 1000
    auto = _frame_checks(c, ctx, counts, least_covered=20)
    tw = th = 16
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid, dtype=np.uint32)
    # an explicit scale: the lists reassemble to the whole frame
    ctx.set_option("depth_complexity_max_colour", 300)
    img = ctx.render(MODE)
    out = np.zeros_like(img)
    for r in range(4):
        mine = tiles[r::4]
        b = _tiles(ctx, mine, tw, th)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)
    assert _code(ctx.depth_complexity_buffers) == -3 and _code(ctx.depth_complexity_stats) == -3   # a tile list that leaves pixels out
    # auto: each list scales by the maximum of its own pixels
    ctx.set_option("depth_complexity_max_colour", 0)
    different = 0
    for r in range(4):
        mine = tiles[r::4]
        own = np.zeros((c.height, c.width), bool)
        for x, y in mine:
            own[y:y + th, x:x + tw] = True
        want = depth_complexity_frame(np.where(own, counts, 0), c.background, 0).reshape(c.height, c.width, 4)
        b = _tiles(ctx, mine, tw, th)
        for i, (x, y) in enumerate(mine):
            hh, ww = min(th, c.height - y), min(tw, c.width - x)
            assert np.array_equal(b[i][:hh, :ww], want[y:y + hh, x:x + ww]), (r, x, y)
            different += int(not np.array_equal(b[i][:hh, :ww], auto[y:y + hh, x:x + ww]))
    assert different > 0   # (some list does not hold the frame's deepest pixel)
    # every tile twice and overlapping ones: the counts are per pixel, not per (tile, pixel) cell
    ctx.set_option("depth_complexity_max_colour", 300)
    tiles2 = np.array(grid * 2 + [(8, 8), (24, 8), (8, 24), (20, 30), (40, 30)], dtype=np.uint32)
    b = _tiles(ctx, tiles2, tw, th)
    for i, (x, y) in enumerate(tiles2):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)
    # a one-rank lv_create_multi handle
    multi = capi.Context(devices=[0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(c.settings)
    multi.set_option("depth_complexity_max_colour", 300)
    assert np.array_equal(multi.render(MODE), img)
    assert int(multi.stats().ppll_pool_nodes) == 0
    assert _code(multi.depth_complexity_stats) == -3
    multi.close()


def test_errors(hip_lib):
    c = _small()
    ctx = c.hip_context()
    ctx.set_option("depth_complexity_max_colour", 2)
    base = ctx.render(MODE)
    assert not np.array_equal(base, c.hip_context().render(MODE))   # (a fresh context scales by the frame's maximum)
    for bad in ("", "-1", "1000001", "auto"):
        assert _code(lambda: ctx.set_option("depth_complexity_max_colour", bad)) == -1, bad
    assert np.array_equal(ctx.render(MODE), base)   # the old value stays
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto")):
        ctx.set_option(key, value)
        assert _code(lambda: ctx.render(MODE)) == -1, key
        ctx.set_option(key, back)
        assert np.array_equal(ctx.render(MODE), base)
    ctx.set_options({"use_ribbons": True, "rotating_helicity_bands": True})
    assert _code(lambda: ctx.render(MODE)) == -1
    ctx.set_options({"use_ribbons": False, "rotating_helicity_bands": False})
    assert np.array_equal(ctx.render(MODE), base)
    for other in (2, 8, capi.MODE_DEPTH_PEELING):
        ctx.render(other)
        assert _code(ctx.depth_complexity_buffers) == -3 and _code(ctx.depth_complexity_stats) == -3
    ctx.render(MODE)
    counts = np.zeros((c.height, c.width), np.uint32)
    p = lambda a: a.ctypes.data
    assert ctx.L.lv_depth_complexity_get_buffers(ctx.h, p(counts), c.width * c.height - 1) == -1   # too small
    assert ctx.L.lv_depth_complexity_get_buffers(ctx.h, p(counts), c.width * c.height) == 0
    assert ctx.L.lv_depth_complexity_get_buffers(ctx.h, None, c.width * c.height) == -1
    assert ctx.L.lv_depth_complexity_get_stats(ctx.h, None) == -1


def test_host_plugin(hip_lib):
    import ctypes
    from linevis_amd import transfer_function as tfm
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    r = host_api.HeadlessLineRenderer(MODE)
    r.set_rendering_resolution(120, 80)
    r.set_transfer_function(tfm.standard_transparent())
    r.set_line_data(flow)
    assert r.rendering_mode == 5 and r.depth_complexity_state() == {"maxColour": 0} and r.depth_peeling_state() is None
    r.set_new_state("Depth Complexity Renderer", MODE, {}, resolution=(120, 80))
    frame = r.render_frame()
    assert (frame[..., :3] != 255).any(axis=2).sum() > 100
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 5, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frame)
    counts = np.zeros((80, 120), np.uint32)
    assert capi.load().lv_depth_complexity_get_buffers(ctypes.c_void_p(hctx), counts.ctypes.data_as(ctypes.c_void_p), 120 * 80) == 0
    bg = frame[0, 0].astype(np.float32) / np.float32(255.0)
    assert counts[0, 0] == 0 and counts.max() >= 2
    r.set_new_settings({"depth_complexity_max_colour": "100"})
    assert r.depth_complexity_state() == {"maxColour": 100}
    other = r.render_frame()
    assert np.array_equal(other.reshape(-1, 4), depth_complexity_frame(counts, bg, 100))   # the plugin's key reached the kernels
    assert not np.array_equal(other, frame)
    r.set_new_settings({"depth_complexity_max_colour": "-3"})   # refused by the C ABI: the value stays
    assert r.depth_complexity_state() == {"maxColour": 100}
