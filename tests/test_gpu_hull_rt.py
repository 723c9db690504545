"""The simulation-mesh hull in the ray tracer on the GPU (lv_hull_rt.h; include/linevis_hip.h, hull_ray_tracing): lv_trace_rays_hull
bit for bit against the brute force of tests/test_hull_rt_restatement.py; hull-only frames against the restated loop; lines and hull
together replayed record by record against the oracle's closest line hit and the brute force; invariance; state and errors; the host
plugin.  Every test here needs the option hull_ray_tracing or the two entry points."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from oracle import lvo
from test_deferred_restatement import F, View
from test_hull_restatement import DEFAULT_OPACITY, LW, bent_strip, hull_case
from test_hull_rt_restatement import (HULL_FLAG, MISS, T_MAX, T_MIN, closest_hull_hit, fold_records, frame_of, hull_hit_shade,
                                      hull_only_loop, next_t_min, one_triangle, primary_rays, sort_records, two_triangles)
from test_mlab_restatement import pack, unpack

pytestmark = pytest.mark.gpu
RT = capi.MODE_RAY_TRACER


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _context(c, hull, opacity=DEFAULT_OPACITY, record=True, **options):
    ctx = c.hip_context()
    if hull is not None:
        ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    if opacity is not None:
        ctx.set_option("hull_opacity", opacity)
    ctx.set_option("hull_ray_tracing", "on")
    ctx.set_option("rt_record_hits", "true" if record else "false")
    ctx.set_options(options)
    return ctx


# ---------------------------------------------------------------- 1. lv_trace_rays_hull against the brute force
@functools.lru_cache(maxsize=None)
def _small_view():
    c = small_case(width=61, height=47, line_width=LW, transparent=True, camera_pos=(0.21, 0.13, 0.8))
    return c, View(c)


def _mesh(name):
    c, V = _small_view()
    pts = c.points["linePosition"]
    return {"one": one_triangle, "two": two_triangles, "strip": bent_strip,
            "box3": lambda: scenes.box_hull((pts.min(0), pts.max(0)), 3, 0.05),
            "box12": lambda: scenes.box_hull((pts.min(0), pts.max(0)), 12, 0.05)}[name]()


@pytest.mark.parametrize("name", ["one", "two", "strip", "box3", "box12"])
def test_trace_rays_hull_bit_for_bit(hip_lib, name):
    c, V = _small_view()
    hull = _mesh(name)
    assert len(hull.triangle_indices) == {"one": 1, "two": 2, "strip": 8, "box3": 108, "box12": 1728}[name]
    ctx = capi.Context(0)
    ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)        # no lines, no camera, no option: the mesh is enough
    ys, xs = np.mgrid[0:V.h, 0:V.w]
    o, d = primary_rays(V, xs, ys)
    sets = [(np.broadcast_to(o, d.shape), d)]
    rng = np.random.default_rng(11)
    centre = np.asarray(hull.positions, dtype=F).mean(0)
    inside = rng.normal(size=(600, 3)).astype(F)
    sets.append((np.broadcast_to(centre, inside.shape), inside))                  # from inside the box / behind the open meshes
    axes = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                dd = np.full(3, zero, dtype=F)
                dd[axis] = -sign
                grid = rng.uniform(-0.3, 0.3, (40, 3)).astype(F)
                grid[:, axis] = sign * 1.5
                axes.append((grid, np.broadcast_to(dd, grid.shape)))
    sets.append((np.concatenate([a[0] for a in axes]), np.concatenate([a[1] for a in axes])))
    hits = 0
    for oo, dd in sets:
        t, tri, uv = ctx.trace_rays_hull(oo, dd, float(T_MIN), float(T_MAX))
        wt, wtri, wuv = closest_hull_hit(hull, oo, dd, T_MIN, T_MAX)
        assert np.array_equal(tri, wtri) and np.array_equal(t.view(np.uint32), wt.view(np.uint32))
        assert np.array_equal(uv.view(np.uint32), wuv.view(np.uint32))
        hits += int((tri != MISS).sum())
    assert hits > 500                                                             # (the pixel rays alone: 292 on the strip ... 2292 on the boxes)
    # a t_min past the first hit: the second surface, or nothing
    oo, dd = sets[0]
    first = closest_hull_hit(hull, oo, dd, T_MIN, T_MAX)[0]
    t_min = float(np.median(first[first < T_MAX]))
    t, tri, uv = ctx.trace_rays_hull(oo, dd, t_min, float(T_MAX))
    wt, wtri, wuv = closest_hull_hit(hull, oo, dd, F(t_min), T_MAX)
    assert np.array_equal(tri, wtri) and np.array_equal(t.view(np.uint32), wt.view(np.uint32)) and np.array_equal(uv.view(np.uint32), wuv.view(np.uint32))
    assert (t[tri != MISS] >= F(t_min)).all() and (tri != MISS).sum() > 150


# ---------------------------------------------------------------- 2. hull-only frames
def _away(c):
    """the case's line points moved behind the camera: no ray meets a line"""
    pts = c.points.copy()
    pts["linePosition"][:, 2] += np.float32(50.0)
    return pts


@pytest.mark.parametrize("kind,shade", [("outside", {}), ("inside", {}), ("strip", {}),
                                        ("outside", dict(use_shading=False, color=(0.25, 0.5, 1.0), opacity=0.7))])
def test_hull_only_frames(hip_lib, kind, shade):
    c, hull, V = hull_case(kind)
    ctx = _context(c, hull, opacity=shade.get("opacity", DEFAULT_OPACITY))
    if shade:
        ctx.set_options(dict(hull_use_shading="false", hull_color="0.25 0.5 1"))
    ctx.set_lines(_away(c), c.seg)
    frame = ctx.render(RT)
    rec = sort_records(ctx.rt_hits())
    want, fc = hull_only_loop(hull, V, background=c.background, **shade)
    assert len(rec) == len(want) > 1000                                # (1 017 on the strip ... 13 278 on the box from outside)
    assert np.array_equal(rec[:, :5], want[:, :5])                     # pixel, step, triangle, t and payload.hitT, bit for bit
    diff = float(np.abs(rec[:, 5:9].view(F).astype(np.float64) - want[:, 5:9].view(F).astype(np.float64)).max())
    print("hull-only %s: %d records, largest float32 colour difference %.3g" % (kind, len(rec), diff))
    assert max_lsb_diff(frame, frame_of(fc, V.w, V.h)) <= 2
    assert np.array_equal(frame, frame_of(fold_records(rec, V.w * V.h, background=c.background), V.w, V.h))
    if shade:
        assert np.all(rec[:, 5:8].view(F) == np.asarray((0.25, 0.5, 1.0), F))


# ---------------------------------------------------------------- 3. / 4. lines and hull together
def _replay(c, V, hull, rec, frame, line_trace, num_samples=1, jittered=False):
    """Every record against the closest line hit (line_trace(o, d, t_min) -> (found, t, primitive word)) and the brute-force hull hit of
    its ray and tMin; the rays that ended with the miss shader against both; the fold against the frame.  -> (pixels with both kinds
    of record, line records)"""
    n = V.w * V.h
    ys, xs = np.mgrid[0:V.h, 0:V.w]
    dirs = [primary_rays(V, xs, ys, 0, num_samples, s, jittered)[1] for s in range(num_samples)]
    o = V.cam
    pix, sample, step = rec[:, 0].astype(np.int64), (rec[:, 1] >> 16).astype(np.int64), (rec[:, 1] & 0xFFFF).astype(np.int64)
    d = np.stack([dirs[s][p] for s, p in zip(sample, pix)])
    t_min = np.full(len(rec), T_MIN)
    later = np.nonzero(step > 0)[0]
    assert (pix[later - 1] == pix[later]).all() and (rec[later - 1, 1] + 1 == rec[later, 1]).all()
    t_min[later] = next_t_min(rec[later - 1, 4].view(F))
    ht, htri, huv = closest_hull_hit(hull, np.broadcast_to(o, d.shape), d, t_min, T_MAX)
    want_prim, want_t = np.zeros(len(rec), np.uint32), np.zeros(len(rec), F)
    for i in range(len(rec)):
        found, lt, word = line_trace(o, d[i], float(t_min[i]))
        hull_wins = htri[i] != MISS and (not found or ht[i] < lt)     # a tie goes to the line
        assert hull_wins or found, i
        want_prim[i], want_t[i] = (HULL_FLAG | htri[i], ht[i]) if hull_wins else (word, lt)
    assert np.array_equal(rec[:, 2], want_prim) and np.array_equal(rec[:, 3], want_t.view(np.uint32))
    is_hull = (rec[:, 2] & HULL_FLAG) != 0
    rgba, hit_t = hull_hit_shade(hull, V.cam, htri[is_hull], huv[is_hull])
    assert np.array_equal(rec[is_hull, 4], hit_t.view(np.uint32))
    assert np.abs(pack(list(rgba.T)).view(np.uint8).astype(int) - pack(list(rec[is_hull, 5:9].view(F).T)).view(np.uint8).astype(int)).max() <= 2
    # termination: the fold asserts that nothing follows a step that ended the loop; a ray that ended with the miss meets nothing
    state = []
    colours = fold_records(rec, n, background=c.background, num_samples=num_samples, jittered=jittered, state=state)
    assert np.array_equal(frame, frame_of(colours, V.w, V.h))
    last = {(p, s): h for p, s, h in zip(pix, sample, rec[:, 4].view(F))}           # (sorted: the last step of a ray stays)
    for s, (missed, count) in enumerate(state):
        rays = np.nonzero(missed)[0]
        tm = np.array([next_t_min(last[(p, s)]) if count[p] else T_MIN for p in rays], dtype=F)
        assert (closest_hull_hit(hull, np.broadcast_to(o, (len(rays), 3)), dirs[s][rays], tm, T_MAX)[1] == MISS).all()
        for p, t0 in zip(rays[::3], tm[::3]):                                        # (every third ray: the oracle goes ray by ray)
            assert not line_trace(o, dirs[s][p], float(t0))[0], (s, p)
    both = np.intersect1d(pix[is_hull], pix[~is_hull])
    return len(both), int((~is_hull).sum())


def _capsule_trace(c):
    sc = c.oracle_scene()
    c.oracle_params(sc)                                                              # (selects the intersection form of the case)

    def trace(o, d, t_min):
        t, seg, kind = sc.trace_rays(o[None], d[None], t_min, float(T_MAX), c.line_width, capped=True)
        return seg[0] != MISS, t[0], np.uint32(((int(seg[0]) << 2) | int(kind[0])) & 0xFFFFFFFF)
    return trace


@functools.lru_cache(maxsize=None)
def _tube_mesh():
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    return lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)


@functools.lru_cache(maxsize=None)
def _together():
    """the frame and the records of test 3, rendered once"""
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull)
    frame = ctx.render(RT)
    return ctx, frame, sort_records(ctx.rt_hits())


def test_lines_and_hull_together(hip_lib):
    c, hull, V = hull_case("outside")
    ctx, frame, rec = _together()
    both, lines = _replay(c, V, hull, rec, frame, _capsule_trace(c))
    assert both > 1000 and lines > 1500
    # the line records' colours are those of the same hits without the hull: a recording frame with hull_opacity = 0 ...
    bare = _context(c, hull, opacity=0)
    frame0 = bare.render(RT)
    rec0 = bare.rt_hits()
    assert not (rec0[:, 2] & HULL_FLAG).any()
    index = {(int(r[0]), int(r[2]), int(r[3])): r for r in rec0}
    matched = 0
    for r in rec[(rec[:, 2] & HULL_FLAG) == 0]:
        r0 = index[(int(r[0]), int(r[2]), int(r[3]))]
        assert np.array_equal(r[4:], r0[4:])
        matched += 1
    assert matched > 1500
    # ... which is the ordinary frame, byte for byte (pinned by the oracle tests)
    off = c.hip_context()
    assert np.array_equal(frame0, off.render(RT))
    assert (frame != frame0).any(axis=2).sum() > 5000


def test_jittered_samples(hip_lib):
    c = small_case(width=61, height=47, line_width=LW, transparent=True, camera_pos=(0.21, 0.13, 0.8), num_samples_per_frame=2)
    pts = c.points["linePosition"]
    hull = scenes.box_hull((pts.min(0), pts.max(0)), 3, 0.05)
    V = View(c)
    ctx = _context(c, hull)
    frame = ctx.render(RT)
    rec = sort_records(ctx.rt_hits())
    assert set(np.unique(rec[:, 1] >> 16)) == {0, 1}
    both, lines = _replay(c, V, hull, rec, frame, _capsule_trace(c), num_samples=2, jittered=True)
    assert both > 300 and lines > 500


def test_triangle_mesh_geometry(hip_lib):
    c, hull, V = hull_case("outside")
    idx, verts, points = _tube_mesh()
    ctx = _context(c, hull, geometry_mode="Triangle Mesh")
    ctx.set_tube_triangle_mesh(idx, verts, points)
    frame = ctx.render(RT)
    rec = sort_records(ctx.rt_hits())
    ts = lvo.TriScene(idx, verts, points, c.line_width)

    def trace(o, d, t_min):
        t, tri, uv = ts.trace_rays(o[None], d[None], t_min, float(T_MAX))
        return tri[0] != MISS, t[0], np.uint32((int(tri[0]) << 2) & 0xFFFFFFFF)
    both, lines = _replay(c, V, hull, rec, frame, trace)
    assert both > 1000 and lines > 1500


# ---------------------------------------------------------------- 5. invariance
def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=RT)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_invariance(hip_lib):
    c, hull, V = hull_case("outside")
    ctx, img, rec = _together()
    plain = _context(c, hull, record=False)
    assert np.array_equal(plain.render(RT), img)                                   # recording does not change the frame
    assert np.array_equal(plain.render(RT), img)                                   # nor does a second render
    assert _code(plain.rt_hits) == -3
    # a tile list that covers the view in odd tiles
    tw, th = 23, 13
    tiles = np.array([(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)], dtype=np.uint32)
    out = np.zeros_like(img)
    b = _tiles(plain, tiles, tw, th)
    for i, (x, y) in enumerate(tiles):
        out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)
    # a one-rank lv_create_multi handle: the mesh and the options reach the rank
    multi = capi.Context(devices=[0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(c.settings)
    multi.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
    multi.set_options(dict(hull_opacity=DEFAULT_OPACITY, hull_ray_tracing="on"))
    assert np.array_equal(multi.render(RT), img)
    multi.close()
    # overlap_primary_passes, with the RTAO pass it belongs to
    ao = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=0.6, ambient_occlusion_iterations=2)
    frames = []
    for overlap in ("true", "false"):
        a = _context(c, hull, record=False, overlap_primary_passes=overlap, **ao)
        frames.append(a.render(RT))
    assert np.array_equal(frames[0], frames[1]) and (frames[0] != img).any()


def test_accumulated_frames(hip_lib):
    c, hull, V = hull_case("outside")
    ctx = _context(c, hull, num_accumulated_frames=3)
    prev = None
    for k in range(3):
        ctx.set_option("frame_number", k)
        frame = ctx.render(RT)
        colours = fold_records(ctx.rt_hits(), V.w * V.h, background=c.background, jittered=True)
        if prev is not None:                                                       # the running mean through RGBA8 (lv_store_color)
            old = unpack(prev.reshape(-1, 4).copy().view(np.uint32).ravel())
            a = F(1.0) / F(k + 1)
            colours = np.stack([old[j] * (F(1.0) - a) + colours[:, j] * a for j in range(4)], 1).astype(F)
        assert np.array_equal(frame, frame_of(colours, V.w, V.h)), k
        assert prev is None or (frame != prev).any()
        prev = frame


# ---------------------------------------------------------------- 6. state and errors
def test_state_and_errors(hip_lib):
    c, hull, V = hull_case("outside")
    ctx, img, rec = _together()
    ctx = _context(c, hull)
    assert np.array_equal(ctx.render(RT), img)
    hull_rec = rec[(rec[:, 2] & HULL_FLAG) != 0]
    # a line-width change leaves the hull records as they are where no line is in front (the pad belongs to the mesh)
    ctx.set_lines(_away(c), c.seg)
    ctx.render(RT)
    alone = sort_records(ctx.rt_hits())
    ctx.set_option("line_width", 0.5 * c.line_width)
    ctx.render(RT)
    assert np.array_equal(sort_records(ctx.rt_hits()), alone)
    ctx.set_option("line_width", c.line_width)
    assert len(alone) >= len(hull_rec)
    # a new mesh rebuilds the LBVH: frames and rays follow it
    strip = bent_strip()
    ctx.set_hull_mesh(strip.triangle_indices, strip.positions, strip.normals)
    frame = ctx.render(RT)
    want, fc = hull_only_loop(strip, V, background=c.background)
    assert np.array_equal(sort_records(ctx.rt_hits())[:, :5], want[:, :5]) and max_lsb_diff(frame, frame_of(fc, V.w, V.h)) <= 2
    ys, xs = np.mgrid[0:V.h:3, 0:V.w:3]
    o, d = primary_rays(V, xs, ys)
    assert np.array_equal(ctx.trace_rays_hull(np.broadcast_to(o, d.shape), d, float(T_MIN), float(T_MAX))[1],
                          closest_hull_hit(strip, np.broadcast_to(o, d.shape), d, T_MIN, T_MAX)[1])
    # use_mlat with a ray-traced, drawn hull: refused, the message names the option, the context stays usable
    ctx.set_option("use_mlat", "true")
    assert _code(lambda: ctx.render(RT)) == -1 and "use_mlat" in ctx.L.lv_last_error(ctx.h).decode()
    ctx.set_option("use_mlat", "false")
    assert np.array_equal(ctx.render(RT), frame)
    # a malformed value: refused, the old one stays
    assert _code(lambda: ctx.set_option("hull_ray_tracing", "maybe")) == -1
    assert np.array_equal(ctx.render(RT), frame)
    # off: the refusal of today; on without a drawn hull: the ordinary frame
    ctx.set_option("hull_ray_tracing", "off")
    assert _code(lambda: ctx.render(RT)) == -1
    ctx.set_options(dict(hull_ray_tracing="on", hull_opacity=0, rt_record_hits="false"))
    ctx.set_lines(c.points, c.seg)
    assert np.array_equal(ctx.render(RT), c.hip_context().render(RT))
    # no mesh; no recording frame; a frame on a tile list that does not cover the viewport
    assert _code(lambda: c.hip_context().trace_rays_hull(np.zeros((1, 3), F), np.ones((1, 3), F), 0.0, 1.0)) == -3
    assert _code(ctx.rt_hits) == -3
    ctx.set_options(dict(hull_opacity=DEFAULT_OPACITY, rt_record_hits="true"))
    ctx.render(RT)
    assert len(ctx.rt_hits()) > 0
    _tiles(ctx, np.array([(0, 0), (32, 16)], dtype=np.uint32), 32, 16)
    assert _code(ctx.rt_hits) == -3
    # the capacity is the recording frame's: a frame that overflowed stays overflowed when the option is raised afterwards
    ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)          # (test 3's state again)
    ctx.set_option("rt_hits_capacity", 100)
    ctx.render(RT)
    assert _code(ctx.rt_hits) == -4
    ctx.set_option("rt_hits_capacity", 1 << 22)
    assert _code(ctx.rt_hits) == -4
    ctx.render(RT)
    assert np.array_equal(sort_records(ctx.rt_hits()), rec)
    # what the kernel has no variant for is refused, not rendered differently: the approximate lighting, more steps than a record numbers
    ctx.set_option("shading_numerics", "fast")
    assert _code(lambda: ctx.render(RT)) == -1 and "shading_numerics" in ctx.L.lv_last_error(ctx.h).decode()
    ctx.set_options(dict(rt_record_hits="false", hull_opacity=0))
    fast = c.hip_context()
    fast.set_option("shading_numerics", "fast")
    assert np.array_equal(ctx.render(RT), fast.render(RT))                          # on, no hull drawn, not recording: the existing kernels
    ctx.set_options(dict(shading_numerics="exact", rt_record_hits="true", hull_opacity=DEFAULT_OPACITY, max_depth_complexity=65537))
    assert _code(lambda: ctx.render(RT)) == -1 and "max_depth_complexity" in ctx.L.lv_last_error(ctx.h).decode()
    ctx.set_option("max_depth_complexity", 65536)
    assert np.array_equal(ctx.render(RT), img)


# ---------------------------------------------------------------- 7. host plugin
def test_host_plugin(hip_lib):
    """HipRayTracer with hull_ray_tracing = on uploads the data set's outline mesh and forwards its settings: the C-ABI frame of test 3;
    without the key it uploads none and renders the frame without a hull"""
    from linevis_amd import transfer_function as tfm
    c, hull, V = hull_case("outside")
    ctx, img, rec = _together()
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))

    def plugin(settings):
        flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
        flow.set_hull_mesh(hull.triangle_indices, hull.positions)                   # (no normals: computeSmoothTriangleNormals)
        r = host_api.HeadlessLineRenderer(RT)
        r.set_rendering_resolution(c.width, c.height)
        r.set_transfer_function(tfm.standard_transparent())
        r.set_camera((0.21, 0.13, 0.8))
        r.set_clear_color(*c.background)
        r.set_line_data(flow)
        r.set_new_settings(dict(line_width=c.line_width, **settings))
        return r, flow

    r, flow = plugin(dict(hull_ray_tracing="on"))
    assert flow.shall_render_hull
    on = r.render_frame()
    rb = plugin({})[0]
    bare = rb.render_frame()
    assert (on != bare).any(axis=2).sum() > 5000
    # Test 3's frame through the C ABI, byte for byte: the case's line points and hull (with scenes.py's normals) and the options of
    # test 3 in a context of their own.  Two things of the plugin's are its own and are handed to that context: its camera matrices (the
    # host's look-at differs from the case's in the last bit of the view matrix) and the data's attribute range, which the plugin passes
    # with the transfer function where the case says 0 ... 1.  Everything else -- the device-built line points, the mesh and its
    # smooth normals, hull_opacity 0.3, hull_color, hull_use_shading, capped tubes, halos -- has to arrive as test 3 has it.
    view, proj, fovy, near, far = r.camera()
    assert np.abs(view - np.asarray(c.view, np.float32).reshape(16)).max() < 1e-6 and np.array_equal(proj, np.asarray(c.proj, np.float32).reshape(16))
    direct = _context(c, hull)
    direct.set_camera(view, proj, fovy, near, far, c.width, c.height)
    direct.set_transfer_function(c.tf, *flow.attribute_range())
    assert np.array_equal(on, direct.render(RT))
    want = sort_records(direct.rt_hits())
    direct.set_option("hull_opacity", 0)
    assert np.array_equal(bare, direct.render(RT))
    # ... and test 3's own frame (the case's camera and range) differs from it only as far as those two do: the same hull triangles
    # under the same pixels wherever both frames record a hull hit first
    first = lambda rr: {int(q[0]): int(q[2]) for q in rr[(rr[:, 1] == 0) & ((rr[:, 2] & HULL_FLAG) != 0)]}
    a, b = first(want), first(rec)
    shared = set(a) & set(b)
    # (a view matrix that differs by 6e-8 moves a ray by that much: another triangle only where the ray passes that close to an edge)
    assert len(shared) > 4000 and sum(a[k] != b[k] for k in shared) <= len(shared) // 100
    # the plugin's own context: the mesh arrived only with the key, its records are the reference context's
    import ctypes
    L = capi.load()
    hctx = ctypes.c_void_p(r.L.lvh_renderer_context(r.h))
    nt, nv = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.lv_get_hull_mesh(hctx, None, 0, None, None, 0, ctypes.byref(nt), ctypes.byref(nv)) == 0 and (nt.value, nv.value) == (108, 56)
    bctx = ctypes.c_void_p(rb.L.lvh_renderer_context(rb.h))
    assert L.lv_get_hull_mesh(bctx, None, 0, None, None, 0, ctypes.byref(nt), ctypes.byref(nv)) == 0 and nt.value == 0
    raw = np.empty((c.height, c.width, 4), dtype=np.uint8)
    assert L.lv_set_option(hctx, b"rt_record_hits", b"true") == 0
    assert L.lv_render(hctx, RT, 0, 0, c.width, c.height, raw.ctypes.data_as(ctypes.c_void_p)) == 0 and np.array_equal(raw, on)
    cnt = ctypes.c_uint64()
    assert L.lv_rt_get_hits(hctx, None, 0, ctypes.byref(cnt)) == 0
    hits = np.zeros((cnt.value, 9), np.uint32)
    assert L.lv_rt_get_hits(hctx, hits.ctypes.data_as(ctypes.c_void_p), cnt.value, ctypes.byref(cnt)) == 0
    assert np.array_equal(sort_records(hits), want)
    assert L.lv_set_option(hctx, b"rt_record_hits", b"false") == 0
    r.set_new_settings({"hull_opacity": 0.0})
    assert np.array_equal(r.render_frame(), bare)
    r.set_new_settings({"hull_opacity": 0.3, "hull_use_shading": False, "hull_color": "0.9 0.1 0.1"})
    other = r.render_frame()
    assert (other != bare).any(axis=2).sum() > 5000 and (other != on).any()
