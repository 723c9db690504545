"""Rendering mode 1 (deferred shading on a visibility buffer) on the GPU against test_deferred_restatement.py: the visibility buffer
bit for bit (index and depth bits) on an ordinary and an odd viewport, without culling and in a close-up that hands triangles to the
whole wave and crosses the near plane; the primitive index against the closest hits of the pixel-centre rays; frames within 2 LSB of
the restated shading, with the screen-space RTAO and depth cues; the shading of given buffers; tile lists, a one-rank multi handle, the
other modes after it, the device tessellation against the uploaded mesh; errors; the host plugin."""
import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import camera, capi, host_api, scenes, transfer_function as tfm
from oracle import lvo
import test_deferred_restatement as dr
from test_deferred_restatement import F, LW, NO_PRIMITIVE, View, deferred_shade, deferred_visibility, reference_case, split

pytestmark = pytest.mark.gpu
MODE = capi.MODE_DEFERRED


def _vis_small():
    """LV_VIS_SMALL as the library is built: the default of lv_deferred.h"""
    import os
    import re
    from linevis_amd import build as lv_build
    return int(re.search(r"#define LV_VIS_SMALL (\d+)u", open(os.path.join(lv_build.CSRC, "lv_deferred.h")).read()).group(1))


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _context(case, mesh):
    ctx = case.hip_context()
    ctx.set_tube_triangle_mesh(*mesh)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _closeup():
    """the camera inside the line set, looking along it: triangles next to the camera fill large parts of the viewport and some
    reach behind the camera plane"""
    case, mesh, _, _ = reference_case()
    c = small_case(width=96, height=64, line_width=LW)
    pts = c.points["linePosition"]
    eye = pts[len(pts) // 2] + np.array([0.011, 0.0, 0.0], F)
    c.view = camera.look_at(tuple(float(x) for x in eye), tuple(float(x) for x in pts[len(pts) // 2 + 3]))
    V = View(c)
    return c, mesh, V, deferred_visibility(mesh, V, cull=True)


# ---------------------------------------------------------------- 1. the visibility buffer
@pytest.mark.parametrize("variant", ["120x80", "257x131", "uncapped", "closeup"])
def test_visibility_buffer_bit_for_bit(hip_lib, variant):
    if variant == "closeup":
        case, mesh, V, words = _closeup()
        S = dr.triangle_setup(mesh, V, True)
        area = (S["x1"] - S["x0"] + 1) * (S["y1"] - S["y0"] + 1)
        prim = split(words)[0]
        winners = np.unique(prim[prim != NO_PRIMITIVE])
        large = set(np.nonzero(S["ok"] & (S["x1"] >= S["x0"]) & (area > _vis_small()))[0])
        crossing = set(np.nonzero(S["ok"] & S["any_behind"])[0])
        assert len(large & set(winners)) >= 5           # triangles the whole wave covers, and they win pixels
        assert len(crossing) >= 2 and len(crossing & set(winners)) >= 1   # triangles across the camera plane, one of them visible
    elif variant == "uncapped":
        case, mesh, V, words = reference_case(capped=False)
        assert not np.array_equal(words, deferred_visibility(mesh, V, cull=True))   # drawn back faces win pixels (open tube ends)
    else:
        w, h = (int(x) for x in variant.split("x"))
        case, mesh, V, words = reference_case(width=w, height=h)
    ctx = _context(case, mesh)
    ctx.set_option("collect_stats", True)
    ctx.render(MODE)
    prim, depth = ctx.deferred_buffers()
    want_prim, want_depth = split(words)
    assert (want_prim != NO_PRIMITIVE).sum() > 500
    assert np.array_equal(prim, want_prim)
    assert np.array_equal(_bits(depth), _bits(want_depth))
    assert int(ctx.stats().fragments) == int((want_prim != NO_PRIMITIVE).sum())
    ctx.close()


def test_primitive_index_against_the_closest_hits_of_the_pixel_centre_rays(hip_lib):
    case, mesh, V, _ = reference_case()
    ctx = _context(case, mesh)
    ctx.render(MODE)
    prim, depth = ctx.deferred_buffers()
    words = (_bits(depth).astype(np.uint64) << np.uint64(32)) | prim.astype(np.uint64)
    hit = dr.brute_force_primitives(mesh, V, lambda o, d: ctx.trace_rays_triangles(o, d, 0.0, 1000.0))
    _, _, unsure = dr.rasterise64(mesh, case)
    share, wrong, covered = dr.compare_with_rays(words, hit, unsure)
    assert covered > 1500
    assert share <= 0.01, share
    assert wrong == 0
    ctx.close()


# ---------------------------------------------------------------- 2. frames
RTAO_TRI = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, rtao_geometry="triangle_tubes",
                ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=8)


@pytest.mark.parametrize("variant", ["plain", "rtao_depth_cues", "no_halos_uncapped"])
def test_frames_against_the_restated_shading(hip_lib, variant):
    settings = {"plain": {}, "rtao_depth_cues": dict(depth_cue_strength=0.7, **RTAO_TRI), "no_halos_uncapped": dict(use_halos=False)}[variant]
    capped = variant != "no_halos_uncapped"
    case, mesh, V, words = reference_case(capped=capped, **settings)
    ctx = _context(case, mesh)
    img = ctx.render(MODE)
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    ao = lvo.TriScene(*mesh, LW).render_ao(P, use_bvh=True) if P.useAmbientOcclusion else None
    ref = deferred_shade(words, mesh, V, case, P, ao=ao)
    assert max_lsb_diff(img, ref) <= 2
    assert (ref[..., 3] == 255).sum() > 500 and (ref[..., :3] != ref[0, 0, :3]).any()
    if variant != "rtao_depth_cues":    # (the RTAO pass goes on accumulating from frame to frame)
        assert np.array_equal(ctx.render(MODE), img)
    ctx.close()


def _band_fixture():
    """the band data of the triangle closest-hit tests (test_gpu_elliptic.py): twisted ribbons on their elliptic triangle tubes"""
    from test_gpu_elliptic import band_case, ribbon_scene
    tr = ribbon_scene()
    mesh = lvo.build_tube_triangle_render_data_ribbons(tr.positions, tr.attributes, tr.line_offsets, tr.ribbon_directions, 0.05, 0.3, 8)
    return band_case(elliptic=False, tube_num_subdivisions=8), mesh, True


def _helicity_fixture(uniform):
    """the rotating helicity bands of the triangle closest-hit tests (test_gpu_helicity_bands.py)"""
    from test_gpu_helicity_bands import helicity_case
    from test_helicity_bands import helix_with_helicity
    tr, hel = helix_with_helicity()
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, 0.03, 8, helicities=hel)
    c, _, _ = helicity_case(line_width=0.03, tube_num_subdivisions=8, helicity_rotation_factor=0.25, use_uniform_twist_line_width=uniform)
    return c, mesh, True


@pytest.mark.parametrize("variant", ["band_data", "helicity_uniform_width", "helicity"])
def test_band_data_and_helicity_frames_against_the_restated_shading(hip_lib, variant):
    """k_deferred_shade<LV_SHADE_BANDS> and <LV_SHADE_HELICITY>: interpolateAngle, the line position and normal of the band shading;
    the interpolated rotation, its continuation on the caps and UNIFORM_HELICITY_BAND_WIDTH"""
    case, mesh, cull = _band_fixture() if variant == "band_data" else _helicity_fixture(variant == "helicity_uniform_width")
    V = View(case)
    words = deferred_visibility(mesh, V, cull=cull)
    ctx = _context(case, mesh)
    img = ctx.render(MODE)
    prim, depth = ctx.deferred_buffers()
    assert np.array_equal(prim, split(words)[0]) and np.array_equal(_bits(depth), _bits(split(words)[1]))
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    assert dr.shade_variant(P) == (dr.BANDS if variant == "band_data" else dr.HELICITY)
    ref = deferred_shade(words, mesh, V, case, P)
    assert max_lsb_diff(img, ref) <= 2
    idx, verts, _ = mesh
    cap = ((verts["vertexLinePointIndex"][idx] >> 31) != 0).any(axis=1)
    won = split(words)[0]
    assert (won != NO_PRIMITIVE).sum() > 2000 and cap[won[won != NO_PRIMITIVE]].sum() > 20    # body and cap pixels
    plain = dict(case.settings, use_ribbons=False, rotating_helicity_bands=False)
    other = _context(case, mesh)
    other.set_options(plain)
    assert (np.abs(other.render(MODE).astype(np.int32) - img.astype(np.int32)).max(axis=2) > 20).sum() > 300   # the variant shows
    assert np.array_equal(ctx.render(MODE), img)
    ctx.close(); other.close()


def test_alpha_is_the_coverage_whatever_the_transfer_function(hip_lib):
    """fragmentColor.a = 1.0: a transparent transfer function gives the frame of the opaque one, byte for byte"""
    case, mesh, _, _ = reference_case()
    a = _context(case, mesh)
    opaque = a.render(MODE)
    t = small_case(width=case.width, height=case.height, line_width=LW, transparent=True)
    tt, ct = np.asarray(t.tf).reshape(-1, 4), np.asarray(case.tf).reshape(-1, 4)
    assert (tt[:, 3] < 1).any() and np.array_equal(tt[:, :3], ct[:, :3])
    b = _context(t, mesh)
    assert np.array_equal(b.render(MODE), opaque)
    a.close(); b.close()


# ---------------------------------------------------------------- 3. given buffers
def test_shading_of_given_buffers(hip_lib):
    case = small_case(width=16, height=8, line_width=LW)
    _, mesh, _, _ = reference_case()
    idx, verts, _ = mesh
    ctx = _context(case, mesh)
    ctx.render(MODE)
    before = ctx.deferred_buffers()
    cap = ((verts["vertexLinePointIndex"][idx] >> 31) != 0).any(axis=1)
    prim = np.full((8, 16), NO_PRIMITIVE, np.uint32)
    depth = np.ones((8, 16), F)
    V = View(case)
    words = deferred_visibility(mesh, V)
    fp, fz = split(words)
    prim[:], depth[:] = fp, fz                              # the frame's own buffer, then the hand-made pixels
    body_tri, cap_tri, last_tri = int(np.nonzero(~cap)[0][7]), int(np.nonzero(cap)[0][3]), len(idx) - 1
    for (y, x), t in (((2, 3), body_tri), ((4, 5), cap_tri), ((6, 9), last_tri)):
        prim[y, x], depth[y, x] = t, F(0.9875)
    prim[1, 7], depth[1, 7] = NO_PRIMITIVE, F(1.0)
    img = ctx.deferred_shade(prim, depth)
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    given = (_bits(depth).astype(np.uint64) << np.uint64(32)) | prim.astype(np.uint64)
    ref = deferred_shade(given, mesh, V, case, P)
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img[1, 7], ref[0, 0] * 0 + dr.unorm8(np.asarray(case.background, F)))
    assert _code(ctx.deferred_buffers) == -3               # the call took the buffers over
    # an index outside the mesh is refused before anything is touched
    ctx.render(MODE)
    kept = ctx.deferred_buffers()
    assert all(np.array_equal(a, b) for a, b in zip(kept, before))
    bad = prim.copy()
    bad[0, 0] = len(idx)
    assert _code(lambda: ctx.deferred_shade(bad, depth)) == -1
    after = ctx.deferred_buffers()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after, kept))
    ctx.close()


# ---------------------------------------------------------------- 4. invariance
def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=MODE)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_tile_lists_and_a_one_rank_handle(hip_lib):
    case, mesh, _, words = reference_case()
    ctx = _context(case, mesh)
    ctx.set_option("collect_stats", True)
    img = ctx.render(MODE)
    tw = th = 16
    grid = [(x, y) for y in range(0, case.height, th) for x in range(0, case.width, tw)]
    tiles = np.array(grid, dtype=np.uint32)
    out = np.zeros_like(img)
    winners = 0
    for r in range(4):                                      # the frame in four interleaved lists
        mine = tiles[r::4]
        b = _tiles(ctx, mine, tw, th)
        winners += int(ctx.stats().fragments)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, case.height - y), :min(tw, case.width - x)]
    assert np.array_equal(out, img)
    assert winners == int((split(words)[0] != NO_PRIMITIVE).sum())   # every requested pixel counted once
    assert _code(ctx.deferred_buffers) == -3                # the last frame left pixels out
    tiles = np.array(grid * 2 + [(8, 8), (24, 8), (8, 24), (20, 30), (40, 30)], dtype=np.uint32)   # repeated and overlapping
    b = _tiles(ctx, tiles, tw, th)
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, case.height - y), min(tw, case.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)
    assert int(ctx.stats().fragments) == int((split(words)[0] != NO_PRIMITIVE).sum())   # ... and a repeated pixel once
    ctx.close()
    multi = capi.Context(devices=[0], transport="memcpy")
    multi.set_lines(case.points, case.seg)
    multi.set_transfer_function(case.tf, 0.0, 1.0)
    multi.set_camera(case.view, case.proj, case.fovy, case.near, case.far, case.width, case.height)
    multi.set_background(case.background)
    multi.set_option("line_width", case.line_width)
    multi.set_options(case.settings)
    multi.set_tube_triangle_mesh(*mesh)
    assert np.array_equal(multi.render(MODE), img)
    multi.close()


def test_other_modes_after_mode_1_and_the_device_tessellation(hip_lib):
    case, mesh, _, _ = reference_case()
    fresh = {}
    for mode in (2, 11):
        f = case.hip_context()
        fresh[mode] = f.render(mode)
        f.close()
    ctx = _context(case, mesh)
    img = ctx.render(MODE)
    for mode in (2, MODE, 11, MODE, 2):
        assert np.array_equal(ctx.render(mode), img if mode == MODE else fresh[mode]), mode
    ctx.close()
    # lv_set_trajectories' mesh (tessellated for the frame) and the same mesh uploaded
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    dev = case.hip_context()
    dev.set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    a = dev.render(MODE)
    assert (a[..., :3] != 255).any(axis=2).sum() > 500
    up = case.hip_context()
    up.set_trajectories(tr.positions, tr.attributes, tr.line_offsets)   # (the same line points)
    up.set_tube_triangle_mesh(*dev.get_tube_triangle_mesh())
    assert np.array_equal(up.render(MODE), a)
    dev.close(); up.close()


# ---------------------------------------------------------------- 5. errors
def test_errors(hip_lib):
    case, mesh, _, _ = reference_case()
    bare = case.hip_context()
    assert _code(lambda: bare.render(MODE)) == -3           # no mesh
    bare.close()
    ctx = _context(case, mesh)
    img = ctx.render(MODE)
    for key, values in (("deferred_rendering_mode", ("Draw Indirect", "BVH Draw Indirect", "BVH Mesh Shader", "Task/Mesh Shader", "")),
                        ("draw_indexed_geometry_mode", ("Programmable Pulling", "triangles")),
                        ("supersampling", ("2", "4", "0", "-1", "many"))):
        for bad in values:
            assert _code(lambda: ctx.set_option(key, bad)) == -1, (key, bad)
        assert np.array_equal(ctx.render(MODE), img), key    # the old value stays in force
    ctx.set_options({"deferred_rendering_mode": "Draw Indexed", "draw_indexed_geometry_mode": "Precomputed Triangles", "supersampling": 1})
    assert np.array_equal(ctx.render(MODE), img)
    # the pair the frame's general check refuses for every mode: passed on, and the context stays usable
    ctx.set_options({"use_ribbons": True, "rotating_helicity_bands": True})
    assert _code(lambda: ctx.render(MODE)) == -1
    ctx.set_options({"use_ribbons": False, "rotating_helicity_bands": False})
    assert np.array_equal(ctx.render(MODE), img)
    # the buffers belong to a mode-1 frame over the whole viewport
    ctx.render(2)
    assert _code(ctx.deferred_buffers) == -3
    ctx.render(MODE)
    n = case.width * case.height
    prim, depth = np.zeros(n, np.uint32), np.zeros(n, F)
    assert ctx.L.lv_deferred_get_buffers(ctx.h, prim.ctypes.data, depth.ctypes.data, n - 1) == -1   # too small
    assert ctx.L.lv_deferred_get_buffers(ctx.h, prim.ctypes.data, None, n) == 0
    # modes 0, 4 and 7 stay refused
    for mode in (0, 4, 7):
        assert _code(lambda: ctx.render(mode)) == -1
    ctx.close()


# ---------------------------------------------------------------- 6. host plugin
def test_host_plugin(hip_lib):
    import ctypes
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    r = host_api.HeadlessLineRenderer(capi.MODE_RAY_TRACER)
    r.set_rendering_resolution(120, 80)
    r.set_transfer_function(tfm.standard())
    r.set_line_data(flow)
    assert r.deferred_state() is None
    for name, mode, res, settings in host_api.get_test_modes_deferred():
        r.set_new_state(name, mode, settings, resolution=(120, 80))
        assert r.rendering_mode == 1
        assert r.deferred_state() == {"deferredRenderingMode": "Draw Indexed", "drawIndexedGeometryMode": "Precomputed Triangles",
                                      "supersampling": 1, "numSamples": 1}
        r.set_transfer_function(tfm.standard())
        r.set_line_data(flow)
        r.set_new_settings(dict(line_width=LW))
        frame = r.render_frame()
        assert (frame[..., :3] != 255).any(axis=2).sum() > 500
        hctx = r.L.lvh_renderer_context(r.h)
        raw = np.empty((80, 120, 4), dtype=np.uint8)
        rc = capi.load().lv_render(ctypes.c_void_p(hctx), 1, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0 and np.array_equal(raw, frame)
        prim = np.zeros((80, 120), np.uint32)
        assert capi.load().lv_deferred_get_buffers(ctypes.c_void_p(hctx), prim.ctypes.data_as(ctypes.c_void_p), None, 120 * 80) == 0
        assert (prim != NO_PRIMITIVE).sum() > 500
        # a value the build does not have goes to the plugin's error, the old one stays
        r.set_new_settings({"deferred_rendering_mode": "Draw Indirect"})
        assert "not built" in r.L.lvh_renderer_last_error(r.h).decode()
        assert r.deferred_state()["deferredRenderingMode"] == "Draw Indexed"
