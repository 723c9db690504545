"""One long-lived context against fresh ones.

The embedder keeps one lv_ctx alive and pushes data sets, viewports, options and rendering modes through it; every other GPU test
builds a new context per case.  The rule under test ("context reuse"): after ANY sequence of successful setters, renders,
read-backs and rejected calls, a stateless frame (no SVGF, num_accumulated_frames = 1, RTAO per frame or a finished prebake) and every
read-back are byte-identical to those of a fresh context that received only the final data set, camera, transfer function, background
and options.  There is no tolerance: both sides run the same kernels on the same inputs.

A *state* is a Case (optionally fed as trajectories and / or with a caller's tube mesh) + a rendering mode + the read-backs to compare;
apply() issues only the calls in which two states differ, observe() returns the outputs.  A *walk* is a list of states: run_walk()
drives it through one context and compares every state with a fresh context.  Two conditions keep a walk from passing vacuously:
consecutive states must differ in the fresh contexts' frames, and every non-empty state covers >= 300 pixels or hits >= 300 rays.
"Fresh" is not the only witness: in every walk the state after the most destructive step is also compared with the CPU oracle.
Temporal state (progressive accumulation, SVGF) is not stateless; its reset rules are the reference's and have their own tests."""
import itertools

import numpy as np
import pytest

from common import Case, max_lsb_diff, scene_arrays
from linevis_amd import camera, capi, host_api, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LSB_TOL = 2            # the suite's bar for RGBA8 frames against the oracle (tests/test_gpu_parity.py)
MIN_COVERED = 300      # pixels shown / rays hit by every non-empty state (test_every_build_gives_the_same_hits_and_frames)
E_INVALID, E_STATE = -1, -3
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
            ambient_occlusion_samples_per_frame=4)
NO_AO = dict(ambient_occlusion_mode="None", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
             ambient_occlusion_samples_per_frame=4)
_KEEP = object()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case_of(points, seg, tf, width, height, line_width, camera_pos=camera.DEFAULT_POSITION, **kw):
    c = Case(points, seg, tf, width, height, line_width, camera_pos=camera_pos, **kw)
    c.camera_pos = camera_pos
    return c


def traj_of(tr, **bands):
    att = tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes
    return dict(positions=tr.positions, attribute=att, line_offsets=tr.line_offsets, **bands)


# ---------------------------------------------------------------- states
class State:
    """reads: frame | hits | ao | depth_range | ppll | accel | lines | mesh | no_mesh | tri_hits | stats | baked
    render: ("full",) | ("rect", (x0, y0, w, h)) | ("tiles", origins, tile_w, tile_h)"""
    _ids = itertools.count()

    def __init__(self, case, mode=11, reads=("frame",), traj=None, mesh=None, twist=None, param=None, render=("full",), label="",
                 empty=False, same_frame_as_before=False, before=(), anchor=None, data=None):
        self.case, self.mode, self.reads, self.traj, self.mesh, self.twist, self.param = case, mode, tuple(reads), traj, mesh, twist, param
        self.render, self.label, self.empty, self.same_frame_as_before = render, label, empty, same_frame_as_before
        self.before, self.anchor = tuple(before), anchor
        self.data = next(State._ids) if data is None else data      # identity of the data set (lines or trajectories)

    def but(self, label=None, mode=None, reads=None, render=None, width=None, height=None, line_width=None, tf=None, background=None,
            mesh=_KEEP, twist=_KEEP, param=_KEEP, same_frame_as_before=False, before=(), anchor=None, **settings):
        """the same data set in another configuration"""
        c = self.case
        s = dict(c.settings)
        s.update(settings)
        pos = getattr(c, "camera_pos", camera.DEFAULT_POSITION)
        n = case_of(c.points, c.seg, c.tf if tf is None else tf, width or c.width, height or c.height, line_width or c.line_width,
                    camera_pos=pos, background=c.background if background is None else background, **s)
        return State(n, mode=self.mode if mode is None else mode, reads=self.reads if reads is None else reads, traj=self.traj,
                     mesh=self.mesh if mesh is _KEEP else mesh, twist=self.twist if twist is _KEEP else twist,
                     param=self.param if param is _KEEP else param, render=render or ("full",), label=label or self.label,
                     empty=self.empty, same_frame_as_before=same_frame_as_before, before=before, anchor=anchor, data=self.data)


def _same_camera(a, b):
    return (a.width, a.height, a.fovy, a.near, a.far) == (b.width, b.height, b.fovy, b.near, b.far) and \
        np.array_equal(a.view, b.view) and np.array_equal(a.proj, b.proj)


def apply(ctx, prev, st):
    """only the calls in which `st` differs from `prev` (None: a fresh context, in Case.hip_context's order)"""
    c, p = st.case, prev.case if prev is not None else None
    new_data = prev is None or prev.data != st.data
    if new_data:
        if st.traj is not None:
            ctx.set_trajectories(**st.traj)
        else:
            ctx.set_lines(c.points, c.seg)
    if st.mesh is not None and (new_data or prev.mesh is not st.mesh):
        ctx.set_tube_triangle_mesh(*st.mesh)
    assert new_data or st.mesh is not None or prev.mesh is None, "a mesh cannot be taken away without new lines"
    if st.param is not None and (new_data or prev.param is not st.param):
        ctx.set_ao_parametrization(*st.param)
    if (prev is None and st.twist is not None) or (prev is not None and prev.twist is not st.twist):
        ctx.set_twist_line_texture(st.twist)
    if p is None or not np.array_equal(p.tf, c.tf):
        ctx.set_transfer_function(c.tf, 0.0, 1.0)
    if p is None or not _same_camera(p, c):
        ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    if p is None or p.background != c.background:
        ctx.set_background(c.background)
    if p is None or p.line_width != c.line_width:
        ctx.set_option("line_width", c.line_width)
    old = p.settings if p is not None else {}
    assert not [k for k in old if k not in c.settings], "the states of a walk spell out the same option keys"
    for k, v in c.settings.items():
        if k not in old or old[k] != v:
            ctx.set_option(k, v)


def fresh(st, **kw):
    ctx = capi.Context(0, **kw)
    apply(ctx, None, st)
    return ctx


def walk_rays(n=20000, seed=123, extent=0.4):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


T_MIN, T_MAX = 1e-4, 10.0


def render_tiles(ctx, mode, origins, tw, th):
    import torch
    out = torch.zeros((len(origins), th, tw, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_tiles_device(out.data_ptr(), origins, tw, th, mode=mode)
    ctx.stats()                       # synchronises the context's stream
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rendered_mask(st):
    """the pixels the state's render call asks for (None: the whole viewport)"""
    c = st.case
    if st.render[0] == "full":
        return None
    m = np.zeros((c.height, c.width), bool)
    if st.render[0] == "rect":
        x0, y0, w, h = st.render[1]
        m[y0:y0 + h, x0:x0 + w] = True
    else:
        _, origins, tw, th = st.render
        for x, y in origins:
            m[y:y + th, x:x + tw] = True
    return m


def ppll_multiset(ctx, st):
    """lv_ppll_get_buffers as per-pixel multisets in a canonical order: (fragment counter, pixel address, depth bits, colour, run
    lengths), restricted to the pixels the render call asked for; the read-back must have the current padded extents"""
    c = st.case
    pw, ph = c.padded()
    avg = int(c.settings.get("ppll_expected_avg_depth_complexity", 0)) or 20
    nodes, start, cnt = ctx.ppll_buffers(pw * ph, avg * pw * ph)
    keep = np.ones(pw * ph, bool)
    mask = rendered_mask(st)
    if mask is not None:
        tw, th = int(c.settings.get("ppll_tile_width", 2)), int(c.settings.get("ppll_tile_height", 8))
        ys, xs = np.nonzero(mask)
        addr = ((ys // th) * (pw // tw) + xs // tw) * (tw * th) + (ys % th) * tw + xs % tw      # TiledAddress.glsl:53-85
        keep[:] = False
        keep[addr] = True
    pix = np.flatnonzero((start != 0xFFFFFFFF) & keep)
    cur = start[pix].astype(np.int64)
    pp, ii = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    while len(pix):
        assert cur.max() < len(nodes), "a list runs out of the node pool"
        pp.append(pix)
        ii.append(cur)
        nxt = nodes[cur, 2]
        live = nxt != 0xFFFFFFFF
        pix, cur = pix[live], nxt[live].astype(np.int64)
        assert len(pp) <= 70000, "a list does not end"
    pp, ii = np.concatenate(pp), np.concatenate(ii)
    assert len(np.unique(ii)) == len(ii), "a node is linked twice"
    key = np.lexsort((nodes[ii, 0], nodes[ii, 1], pp))
    total = np.uint32(cnt) if mask is None else np.uint32(len(ii))
    return total, pp[key], nodes[ii[key], 1], nodes[ii[key], 0], np.bincount(pp, minlength=pw * ph)


def observe(ctx, st):
    c, mode, out = st.case, st.mode, {}
    reads = st.reads
    mask = rendered_mask(st)
    if "frame" in reads:
        if st.render[0] == "full":
            out["frame"] = ctx.render(mode)
            assert out["frame"].shape == (c.height, c.width, 4)
        elif st.render[0] == "rect":
            out["frame"] = ctx.render(mode, tile=st.render[1])
        else:
            out["frame"] = render_tiles(ctx, mode, *st.render[1:])
    if "hits" in reads:
        out["hits"] = ctx.trace_rays(RAYS[0], RAYS[1], T_MIN, T_MAX)
    if "ao" in reads:
        ao = ctx.get_ao()
        assert ao.shape == (c.height, c.width)
        out["ao"] = ao if mask is None else ao[mask]
    if "depth_range" in reads:
        out["depth_range"] = ctx.depth_range()
    if "ppll" in reads:
        out["ppll"] = ppll_multiset(ctx, st)
    if "stats" in reads or "accel" in reads:
        s = ctx.stats()
        out["stats"] = (s.num_segments, s.num_nodes, s.fragments, s.max_depth_complexity, s.mboit_degenerate_pixels)
        if "accel" in reads:
            out["accel"] = ctx.get_accel(s.num_nodes, s.num_segments)
    if "lines" in reads:
        out["lines"] = ctx.get_lines()
    if "mesh" in reads:
        out["mesh"] = ctx.get_tube_triangle_mesh()
    if "no_mesh" in reads:
        with pytest.raises(capi.LineVisError) as e:
            ctx.get_tube_triangle_mesh()
        out["no_mesh"] = np.int32(e.value.code)
        assert e.value.code == E_STATE
    if "tri_hits" in reads:
        out["tri_hits"] = ctx.trace_rays_triangles(RAYS[0], RAYS[1], T_MIN, T_MAX)
    if "baked" in reads:
        out["baked"] = ctx.get_baked_ao(int(c.settings.get("rtao_prebaker_num_tube_subdivisions", 8)))
    return out


def _canon(x):
    """floats are compared by their bits"""
    if isinstance(x, (tuple, list)):
        return tuple(_canon(v) for v in x)
    a = np.ascontiguousarray(x)
    return (a.shape, a.dtype.str, a.tobytes())


def assert_same(got, want, where):
    assert list(got) == list(want), where
    for k in want:
        if _canon(got[k]) != _canon(want[k]):
            a, b = got[k], want[k]
            detail = ""
            if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape:
                detail = ": %d of %d values differ" % (int((a.view(np.uint8) != b.view(np.uint8)).sum()), a.view(np.uint8).size)
            raise AssertionError("%s: '%s' of the reused context is not the fresh context's%s" % (where, k, detail))


def covered(st, out):
    """pixels that show something, rays that hit something"""
    bg8 = np.floor(np.clip(np.asarray(st.case.background, np.float32), 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    px = int((out["frame"].reshape(-1, 4) != bg8).any(axis=1).sum()) if "frame" in out else 0
    rays = int((out["hits"][1] != 0xFFFFFFFF).sum()) if "hits" in out else 0
    return max(px, rays)


def run_walk(states, ctx=None, fresh_fn=fresh, may_reject=False):
    """The walk on one context, every state against a fresh one; returns (states compared, rejected states)."""
    ctx = ctx if ctx is not None else capi.Context(0)
    prev, prev_frame, compared, rejected = None, None, 0, []
    for i, st in enumerate(states):
        where = "step %d (%s)" % (i + 1, st.label)
        apply(ctx, prev, st)
        prev = st
        f = fresh_fn(st)
        try:
            want = observe(f, st)
        except capi.LineVisError as e:
            assert may_reject, "%s: the fresh context fails: %s" % (where, e)
            with pytest.raises(capi.LineVisError) as mine:      # a combination the library rejects: rejected here as well
                observe(ctx, st)
            assert mine.value.code == e.code and ctx.L.lv_last_error(ctx.h), where
            rejected.append((st, e.code))
            continue
        finally:
            f.close()
        for hook in st.before:                                     # calls of the long-lived context only (build_accel, ...)
            hook(ctx)
        got = observe(ctx, st)
        assert_same(got, want, where)
        compared += 1
        if "frame" in want:
            if prev_frame is not None and not st.same_frame_as_before:
                assert want["frame"].shape != prev_frame.shape or not np.array_equal(want["frame"], prev_frame), \
                    "%s: the change does not reach the frame" % where
            prev_frame = want["frame"]
        if not st.empty and ("frame" in want or "hits" in want):
            assert covered(st, want) >= MIN_COVERED, "%s: covers %d pixels / rays" % (where, covered(st, want))
        if st.anchor is not None:
            st.anchor(st, got)
    ctx.close()
    return compared, rejected


# ---------------------------------------------------------------- oracle anchors
def anchor_ray_tracer(st, got):
    """mode 11 on the capsules: frame within the bar, AO factors and hits bit for bit"""
    c = st.case
    ref, ao_ref = c.oracle_render(11)
    assert max_lsb_diff(got["frame"], ref) <= LSB_TOL, st.label
    if ao_ref is not None and "ao" in got:
        if c.eaw_settings():          # exp() of libm against the device library's: the bar of tests/test_eaw.py
            assert np.abs(got["ao"] - ao_ref).max() < 2e-5, st.label
        else:
            assert np.array_equal(bits(got["ao"]), bits(ao_ref)), st.label
    if "hits" in got:
        sc = c.oracle_scene()
        c.oracle_params(sc)          # the oracle on the roots this case's settings select
        b = sc.trace_rays(RAYS[0], RAYS[1], T_MIN, T_MAX, c.line_width, use_bvh=False)
        assert np.array_equal(bits(got["hits"][0]), bits(b[0])) and np.array_equal(got["hits"][1], b[1]) and \
            np.array_equal(got["hits"][2], b[2]), st.label


def anchor_ppll(st, got):
    assert max_lsb_diff(got["frame"], st.case.oracle_render(2)[0]) <= LSB_TOL, st.label


def _oracle_ao(c):
    """the AO image the fragments of modes 3 and 6 are shaded with (None without RTAO)"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    return c.oracle_ao(sc, P, mode=2) if P.useAmbientOcclusion else None


def anchor_mlab(st, got):
    from test_gpu_mlab import frame_reference
    ref, n = frame_reference(st.case, int(st.case.settings.get("mlab_num_layers", 8)), ao=_oracle_ao(st.case))
    assert n >= MIN_COVERED and np.array_equal(got["frame"], ref), st.label          # 0 LSB, as tests/test_gpu_mlab.py
    if "stats" in got:
        assert got["stats"][2] == n


def anchor_mboit(st, got):
    from test_gpu_mboit import frame_reference
    s = st.case.settings
    bias = s.get("mboit_moment_bias", "auto")
    ref, n, _, deg = frame_reference(st.case, int(s.get("mboit_num_moments", 4)), ao=_oracle_ao(st.case),
                                     bias=None if bias == "auto" else float(bias))
    assert n >= MIN_COVERED and np.array_equal(got["frame"], ref), st.label          # 0 LSB, as tests/test_gpu_mboit.py
    if "stats" in got:
        assert got["stats"][2] == n
        assert got["stats"][4] == deg or not s.get("collect_stats", False)       # (the degenerate pixels are counted with collect_stats only)


def anchor_of(mode):
    return {11: anchor_ray_tracer, 2: anchor_ppll, 3: anchor_mlab, 6: anchor_mboit}[mode]


# ---------------------------------------------------------------- scenes
def lines_case(n_lines, pts_per_line, seed, line_width, width=96, height=64, **settings):
    tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=pts_per_line, seed=seed))
    pts, seg = scene_arrays(tr, line_width)
    return case_of(pts, seg, tfm.standard_transparent(), width, height, line_width, **settings), tr


def point_pairs_case(positions, seg, line_width, width=96, height=64, camera_pos=camera.DEFAULT_POSITION, attribute=None, **settings):
    P = np.zeros(len(positions), dtype=lvo.LINE_POINT_DTYPE)
    P["linePosition"] = np.asarray(positions, dtype=np.float32)
    P["lineTangent"] = [1, 0, 0]
    P["lineNormal"] = [0, 1, 0]
    if attribute is not None:
        P["lineAttribute"] = attribute
    return case_of(P, np.asarray(seg, np.uint32), tfm.standard_transparent(), width, height, line_width, camera_pos=camera_pos, **settings)


def deep_chain(**settings):
    """test_deep_lbvh_uses_stack_overflow_slab's construction: segment k sits on axis k % 3 at distance 2^-(k // 3 + 1), so the plain
    LBVH degenerates into a chain of ~50 levels and the traversal needs the global stack-overflow slab"""
    pts, seg = [], []
    for k in range(54):
        a = np.zeros(3)
        a[k % 3] = 0.9 * 2.0 ** (-(k // 3 + 1))
        b = a.copy()
        b[(k + 1) % 3] += 0.3 * 2.0 ** (-(k // 3 + 1))
        seg.append([len(pts), len(pts) + 1])
        pts += [a, b]
    return point_pairs_case(pts, seg, 0.0004, camera_pos=(0.3, 0.3, 0.9), attribute=np.linspace(0, 1, len(pts)), **settings)


def _rays():
    """20 000 random rays through the unit box + 5 000 aimed at the points of the deep chain (it shows in a handful of pixels only)"""
    o, d = walk_rays()
    rng = np.random.default_rng(4)
    pts = deep_chain().points["linePosition"].astype(np.float64)
    tgt = pts[rng.integers(0, len(pts), 5000)] * (1.0 + 1e-3 * rng.normal(size=(5000, 3)))
    o2 = rng.uniform(-0.1, 0.6, (5000, 3)).astype(np.float32)
    d2 = (tgt - o2).astype(np.float32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return np.concatenate([o, o2]), np.concatenate([d, d2])


RAYS = _rays()


# ---------------------------------------------------------------- walk A: data sets through lv_set_lines
WALK_A = dict(RTAO, rtao_geometry="capsules", accel_build="fast_trace", mboit_moment_bias=5e-5)
READS_A = ("frame", "hits", "ao", "depth_range", "accel", "stats")


def walk_a():
    big = State(lines_case(60, 50, 5, 0.01, **WALK_A)[0], reads=READS_A, label="2940 segments")
    tiny = State(lines_case(6, 9, 2, 0.07, **WALK_A)[0], reads=READS_A, label="48 segments")
    empty = State(case_of(np.zeros(0, dtype=lvo.LINE_POINT_DTYPE), np.zeros((0, 2), np.uint32), tfm.standard_transparent(), 96, 64, 0.04,
                          **WALK_A), reads=READS_A, label="empty", empty=True)
    one = State(point_pairs_case([[-0.2, 0.0, 0.0], [0.2, 0.05, 0.0]], [[0, 1]], 0.12, attribute=[0.1, 0.9], **WALK_A), reads=READS_A,
                label="one segment")
    pos = np.zeros((128, 3), np.float32)
    pos[0::2], pos[1::2] = [-0.1, 0.0, 0.0], [0.1, 0.0, 0.0]
    dup = State(point_pairs_case(pos, np.arange(128).reshape(64, 2), 0.2, **WALK_A), reads=READS_A, label="64 duplicates")
    deep = State(deep_chain(**dict(WALK_A, accel_build="fast_build")), reads=READS_A, label="deep chain")
    out = []
    for n, st in enumerate((big, tiny, big, empty, one, dup, deep, tiny)):
        anchored = st is tiny                                   # the small set under the stale tails of the large one / the deep one
        out.append(st.but(anchor=anchor_ray_tracer if anchored else None))
        out.append(st.but(mode=2, reads=("frame", "hits", "ppll", "stats"), label=st.label + ", mode 2", anchor=anchor_ppll if anchored else None,
                          same_frame_as_before=st.empty))        # (an empty scene is the background in every mode)
        if n < 2 or n == 7:      # modes 3 and 6 keep state per data set as well (pool slots, the points' box of the log-depth range)
            for mode in (3, 6):
                out.append(st.but(mode=mode, reads=("frame", "stats"), label="%s, mode %d" % (st.label, mode),
                                  anchor=anchor_of(mode) if anchored else None))
    return out


def test_walk_a_data_sets_replace_each_other(hip_lib):
    """several treelets -> smaller than one treelet (every buffer keeps a stale tail) -> back -> empty -> one segment -> 64 duplicates
    -> a chain that needs the stack-overflow slab -> the small set again (wideDepth and the slab shrink logically)"""
    states = walk_a()
    deep = [s for s in states if s.label == "deep chain"][0]
    f = fresh(deep)
    f.build_accel()
    assert f.stats().bvh_depth > 32          # binary height: the 4-wide traversal's stack exceeds the 32 entries kept in LDS
    f.close()
    compared, _ = run_walk(states)
    assert compared == len(states) == 22


# ---------------------------------------------------------------- walk B: trajectories <-> lines <-> the caller's mesh
def walk_b():
    s = dict(RTAO, ambient_occlusion_samples_per_frame=8, rtao_geometry="auto", geometry_mode="AABBs", tube_num_subdivisions=6)
    lw, W, H = 0.02, 96, 64
    tf = tfm.standard()

    def data(n_lines, ppl, seed):
        tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=ppl, seed=seed))
        pts, seg = scene_arrays(tr, lw)
        return tr, case_of(pts, seg, tf, W, H, lw, **s)
    tr1, c1 = data(40, 40, 11)
    tr2, c2 = data(30, 30, 7)
    tr3, c3 = data(20, 40, 3)
    everything = ("frame", "ao", "hits", "lines", "mesh", "tri_hits", "stats")

    def anchor_small_trajectories(st, got):
        """the fewer trajectories after everything before: the device's lines and mesh are the oracle's arrays, AO over the oracle's
        triangle tubes bit for bit, the frame within the bar"""
        c = st.case
        mesh = lvo.build_tube_triangle_render_data(tr3.positions, tr3.attributes, tr3.line_offsets, lw, 6)
        assert _canon(got["lines"]) == _canon((c.points, c.seg)) and _canon(got["mesh"]) == _canon(mesh)
        oc = case_of(c.points, c.seg, c.tf, W, H, lw, **dict(s, rtao_geometry="triangle_tubes"))   # what "auto" resolves to here
        sc = oc.oracle_scene()
        P = oc.oracle_params(sc)
        ts = lvo.TriScene(*mesh, lw)
        ao_ref = ts.render_ao(P, use_bvh=True)
        assert np.array_equal(bits(got["ao"]), bits(ao_ref)) and (ao_ref < 1.0).sum() > 200
        assert max_lsb_diff(got["frame"], sc.render_rt(P, ao=ao_ref, use_bvh=True)) <= LSB_TOL
        b = ts.trace_rays(RAYS[0], RAYS[1], T_MIN, T_MAX, use_bvh=True)
        assert np.array_equal(bits(got["tri_hits"][0]), bits(b[0])) and np.array_equal(got["tri_hits"][1], b[1])

    t1 = State(c1, reads=everything, traj=traj_of(tr1), label="1: 40 x 40 trajectories")
    l2 = State(c2, reads=("frame", "ao", "hits", "lines", "no_mesh", "stats"), label="2: other lines, no mesh: auto = capsules")
    m3 = State(c2, reads=everything, mesh=lvo.build_tube_triangle_render_data(tr2.positions, tr2.attributes, tr2.line_offsets, lw, 6),
               label="3: their host tessellation", data=l2.data)
    t4 = State(c3, reads=everything, traj=traj_of(tr3), label="4: fewer trajectories", anchor=anchor_small_trajectories)
    own = lvo.build_tube_triangle_render_data(tr3.positions, tr3.attributes, tr3.line_offsets, lw, 8)   # not the 6-gon the device writes
    m5 = State(c3, reads=everything, traj=t4.traj, mesh=own, label="5: the caller's mesh over trajectories", data=t4.data)

    def mesh_is_the_callers(st, got):
        assert _canon(got["mesh"]) == _canon(own), "a line-width change must not re-tessellate the caller's mesh"
    w6 = m5.but(line_width=0.03, label="6: line width (the mesh stays the caller's)", anchor=mesh_is_the_callers)
    tri = dict(geometry_mode="Triangle Mesh", reads=("frame", "ao"))
    return [t1, t1.but(label="1b: Triangle Mesh", **tri), l2.but(), m3, m3.but(label="3b: Triangle Mesh", **tri), t4.but(anchor=t4.anchor),
            m5, m5.but(label="5b: Triangle Mesh", **tri), w6.but(geometry_mode="AABBs", anchor=w6.anchor),
            w6.but(label="6b: Triangle Mesh", **tri)]


def test_walk_b_trajectories_lines_and_the_callers_mesh(hip_lib):
    """rtao_geometry = auto follows what the context holds: the device's mesh of trajectories, capsules after lv_set_lines (no mesh to
    read back), the caller's mesh once it is set -- also over trajectories, where a line-width change must not re-tessellate it"""
    states = walk_b()
    compared, _ = run_walk(states)
    assert compared == len(states)


# ---------------------------------------------------------------- walk C: geometry-affecting options on resident band trajectories
C_OPTIONS = [("line_width", [0.013, 0.03, 0.02]), ("tube_num_subdivisions", [3, 8, 6]), ("use_ribbons", [True, False]),
             ("band_width", [0.05]), ("min_band_thickness", [0.5]), ("thick_bands", [False]),
             ("use_analytic_elliptic_tubes", [True, False]), ("rotating_helicity_bands", [True, False]), ("use_capped_tubes", [False]),
             ("geometry_mode", ["Triangle Mesh", "Linear Swept Spheres", "AABBs"]), ("rtao_geometry", ["triangle_tubes", "capsules"]),
             ("intersection_form", ["literal", "closest_approach"]), ("triangle_leaf_records", ["triangles"]),
             ("accel_build", ["fast_build"]), ("treelet_leaves", [7])]
C_BASE = dict(NO_AO, tube_num_subdivisions=6, use_ribbons=False, band_width=0.03, min_band_thickness=0.3, thick_bands=True,
              use_analytic_elliptic_tubes=False, rotating_helicity_bands=False, use_capped_tubes=True, geometry_mode="AABBs",
              rtao_geometry="capsules", intersection_form="auto", triangle_leaf_records="pairs", accel_build="fast_trace",
              treelet_leaves=512, helicity_rotation_factor=0.25)
C_SEED = 9
C_MODES = [(11, False), (11, True), (2, False), (3, False), (6, False)]      # (mode, RTAO)


def walk_c_changes(seed=C_SEED):
    """the option changes in a fixed-seed order; the values of one option keep their own order"""
    tokens = [k for k, values in C_OPTIONS for _ in values]
    order = np.random.default_rng(seed).permutation(len(tokens))
    left = {k: list(v) for k, v in C_OPTIONS}
    return [(tokens[i], left[tokens[i]].pop(0)) for i in order]


def walk_c():
    from test_gpu_band_trajectories import curves
    pos, att, off, rib, hel = curves(5, 12, 30)
    W, H, lw = 160, 112, 0.02
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, att, off, lw)
    traj = dict(positions=pos, attribute=att, line_offsets=off, ribbon_directions=rib, helicity=hel)
    # (the base state renders the rotation's last mode: consecutive states then always differ in the consumer as well)
    st = State(case_of(pts, seg, tfm.standard_transparent(), W, H, lw, **C_BASE), mode=C_MODES[-1][0], traj=traj, reads=("frame", "lines"),
               label="0: base")
    states = [st]

    def build(ctx):
        ctx.build_accel()      # LV_OK on band / helicity trajectories whatever the frame is going to use
    for i, (key, value) in enumerate(walk_c_changes()):
        mode, ao = C_MODES[i % len(C_MODES)]
        reads = ("frame", "lines") + (("ao",) if ao else ()) + (("mesh",) if i % 2 else ()) + (("ppll",) if mode == 2 else ())
        kw = dict(line_width=value) if key == "line_width" else {key: value}
        st = st.but(label="%d: %s = %s, mode %d%s" % (i + 1, key, value, mode, " + RTAO" if ao else ""), mode=mode, reads=reads,
                    before=(build,) if i % 3 == 0 else (), **dict(RTAO if ao else NO_AO, **kw))
        states.append(st)

    def anchor_elliptic(s, got):
        """band data as sphere-traced elliptic tubelets + RTAO over them: the oracle's line points, AO bits and frame"""
        c = s.case
        op, os_, _ = lvo.build_tube_aabb_render_data_ribbons(pos, att, off, float(c.settings["band_width"]), rib)
        assert _canon(got["lines"]) == _canon((op, os_))
        oc = case_of(op, os_, c.tf, W, H, c.line_width, **c.settings)
        ref, ao_ref = oc.oracle_render(11)
        assert np.array_equal(bits(got["ao"]), bits(ao_ref)) and (ao_ref < 1.0).sum() > 200
        assert max_lsb_diff(got["frame"], ref) <= LSB_TOL
    last = dict(RTAO, use_ribbons=True, rotating_helicity_bands=False, use_analytic_elliptic_tubes=True, geometry_mode="AABBs",
                rtao_geometry="capsules", intersection_form="auto")
    states.append(st.but(label="last: elliptic band tubelets + RTAO", mode=11, reads=("frame", "lines", "ao"), anchor=anchor_elliptic, **last))
    return states


def test_walk_c_options_on_resident_band_trajectories(hip_lib):
    """one option per step on trajectories that stay in HBM, the modes rotating over 11, 11 + RTAO, 2, 3 and 6, lv_build_accel between
    some steps; combinations the library rejects are rejected by both contexts with the same code and leave the next state intact"""
    states = walk_c()
    compared, rejected = run_walk(states, may_reject=True)
    both = [(s, code) for s, code in rejected if s.case.settings["use_ribbons"] and s.case.settings["rotating_helicity_bands"]]
    assert both and all(code == E_INVALID for _, code in both), "use_ribbons + rotating_helicity_bands must be reached and rejected"
    assert compared >= 15 and compared + len(rejected) == len(states), (compared, [s.label for s, _ in rejected])
    assert states[-1].anchor is not None and states[-1] not in [s for s, _ in rejected]


# ---------------------------------------------------------------- walk D: viewports and tile lists
D_CONFIGS = {
    "rt_rtao_eaw": (11, dict(RTAO, rtao_geometry="capsules", ambient_occlusion_denoiser="EAW", eaw_denoiser_iterations=2)),   # halo 6 px
    "ppll_raster_prism": (2, dict(NO_AO, ppll_fragment_source="raster_prism")),
    "ppll_capsule_entry": (2, dict(NO_AO, ppll_fragment_source="capsule_entry")),
    "mlab": (3, dict(NO_AO)),
    "mboit": (6, dict(NO_AO, mboit_num_moments=4, mboit_moment_bias=5e-5)),
}


def walk_d(config):
    mode, settings = D_CONFIGS[config]
    reads = ("frame",) + (("ao",) if mode == 11 else ()) + (("ppll", "stats") if mode == 2 else ())
    st = State(lines_case(30, 30, 7, 0.06, **settings)[0], mode=mode, reads=reads, label="96 x 64")
    states = [st]
    for w, h in ((200, 120), (40, 24), (97, 61), (96, 64)):          # 97 x 61: no multiple of the PPLL tile (2 x 8) nor of 16
        states.append(st.but(width=w, height=h, label="%d x %d" % (w, h), anchor=anchor_of(mode) if (w, h) == (40, 24) else None))
    grid = np.array([(x, y) for y in (0, 32) for x in (0, 32, 64)], np.uint32)
    states.append(st.but(render=("rect", (37, 21, 50, 33)), label="a sub-rectangle"))
    states.append(st.but(render=("tiles", grid, 32, 32), label="32 x 32 tiles that cover the viewport"))
    states.append(st.but(render=("tiles", grid[[1, 4, 0]], 32, 32), label="a list that does not cover it"))
    states.append(st.but(render=("tiles", grid, 16, 16), label="the same origins, 16 x 16"))
    states.append(st.but(label="the whole frame again"))
    return states


@pytest.mark.parametrize("config", list(D_CONFIGS))
def test_walk_d_viewports_and_tile_lists(hip_lib, config):
    """96 x 64 -> 200 x 120 -> 40 x 24 (oracle) -> 97 x 61 -> 96 x 64, then a rectangle, covering and non-covering tile lists and
    another tile size: frames, AO images and PPLL buffers have the current extents and a fresh context's contents"""
    states = walk_d(config)
    compared, _ = run_walk(states)
    assert compared == len(states)


# ---------------------------------------------------------------- walk E: rendering modes interleaved on one scene
E_POOL = 400           # nodes per pixel of the mode-2 states: no fragment of theirs is dropped (a dropped one is anybody's)
E_BASE = dict(NO_AO, collect_stats=True, ppll_expected_avg_depth_complexity=E_POOL, mlab_num_layers=8, mboit_num_moments=6,
              mboit_moment_bias=5e-5, use_mlat=False, ppll_fragment_source="auto", ppll_max_num_frags=100, sorting_mode="Priority Queue")
E_SEGMENTS = 1500      # stacked through the same pixels: prism runs of up to 1402 fragments (the oracle's count)


def walk_e():
    from test_gpu_mlab import _stacked_case
    base = _stacked_case(n=E_SEGMENTS, width=120, height=80)
    reads = ("frame", "stats")
    s0 = State(case_of(base.points, base.seg, base.tf, 120, 80, base.line_width, **E_BASE), mode=2, reads=reads + ("ppll",), label="1: mode 2")

    def long_runs(st, got):
        assert got["stats"][3] > 1024, "the scene must hold a pixel run of more than 1024 fragments (%d)" % got["stats"][3]
        anchor_mlab(st, got)

    def ppll_after_the_regrown_pool(st, got):
        assert got["stats"][3] > 1024
        anchor_ppll(st, got)
    return [
        s0,
        s0.but(mode=3, reads=reads, ppll_expected_avg_depth_complexity=1, label="2: mode 3, K = 8, the pool regrows", anchor=long_runs),
        s0.but(label="3: mode 2, lv_ppll_get_buffers valid", anchor=ppll_after_the_regrown_pool),
        s0.but(mode=6, reads=reads, label="4: mode 6, N = 6", anchor=anchor_mboit),
        s0.but(mode=11, reads=reads, use_mlat=True, label="5: mode 11 with MLAT"),
        s0.but(ppll_fragment_source="capsule_entry", ppll_max_num_frags=2048,
               label="6: mode 2 from linked lists (capsule_entry)"),
        s0.but(ppll_fragment_source="raster_prism", ppll_max_num_frags=8, label="7: raster_prism, the nearest 8 fragments kept (select_nearest)"),
        s0.but(ppll_fragment_source="raster_prism", ppll_max_num_frags=4096, label="8: raster_prism, every fragment kept"),
        s0.but(ppll_fragment_source="raster_prism", ppll_max_num_frags=16, sorting_mode="Insertion Sort", label="9a: Insertion Sort, 16 kept"),
        s0.but(ppll_fragment_source="raster_prism", ppll_max_num_frags=16, sorting_mode="Quicksort Hybrid", label="9b: Quicksort Hybrid",
               same_frame_as_before=True),       # (the sorting mode never changes a pixel)
        s0.but(mode=3, reads=reads, mlab_num_layers=1, label="10: mode 3, K = 1"),
        s0.but(mode=6, reads=reads, mboit_num_moments=8, label="11: mode 6, N = 8"),
        s0.but(mode=11, reads=reads, label="12: mode 11"),
    ]


def test_walk_e_rendering_modes_interleaved(hip_lib):
    """collect_stats stays on: the statistics counters equal the fresh context's across the mode switches and the pool regrowth"""
    states = walk_e()
    compared, _ = run_walk(states)
    assert compared == len(states)


# ---------------------------------------------------------------- walk F: a two-rank handle against a fresh single-device context
def test_walk_f_two_rank_handle_forwards_every_setter(hip_lib):
    """capi.Context(devices=[0, 0]): every setter reaches both ranks -- one that does not shows as a wrong half of the frame"""
    from test_gpu_band_trajectories import curves
    s = dict(RTAO, rtao_geometry="auto", rotating_helicity_bands=False, use_twist_line_texture=False, mlab_num_layers=8,
             helicity_rotation_factor=0.25, rtao_prebaker_iterations=2, rtao_prebaker_samples_per_frame=4)
    lw = 0.02
    big, _ = lines_case(40, 40, 7, 0.012, 200, 136, **s)
    tiny, _ = lines_case(6, 9, 2, 0.04, 200, 136, **s)
    pos, att, off, rib, hel = curves(5, 12, 30)
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, att, off, lw)
    band = case_of(pts, seg, tfm.standard(), 200, 136, lw, **dict(s, rotating_helicity_bands=True, use_twist_line_texture=True))
    rng = np.random.default_rng(3)
    twist = rng.integers(0, 256, (16, 32, 4), dtype=np.uint8)
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    bpts, bseg = scene_arrays(tr, lw)
    baked = case_of(bpts, bseg, tfm.standard(), 200, 136, lw, **s)
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
    param = lvo.ao_parametrization(tr.positions, tr.line_offsets, 0.01)
    reads = ("frame",)
    a = State(big, reads=reads, label="1: first frame")
    b = State(tiny, reads=reads, label="2: set_lines + set_option", anchor=anchor_ray_tracer)
    c = b.but(mode=2, width=150, height=90, background=(0.2, 0.3, 0.4, 1.0), tf=tfm.standard(), **NO_AO,
              label="3: set_camera + set_background + set_transfer_function")
    d = State(band, reads=reads, traj=dict(positions=pos, attribute=att, line_offsets=off, helicity=hel), twist=twist,
              label="4: set_trajectories + set_twist_line_texture")
    e = State(baked, reads=reads, mesh=mesh, label="5: set_lines + set_tube_triangle_mesh (RTAO on the triangle tubes)")
    f = e.but(mode=3, width=97, height=61, tf=tfm.standard_transparent(), **NO_AO, label="6: mode 3 at 97 x 61")
    g = e.but(param=param, ambient_occlusion_mode="RTAO (Prebaker)", label="7: set_ao_parametrization + the prebaker")
    h = e.but(mode=6, tf=tfm.standard_transparent(), param=param, **NO_AO, label="8: build_accel + mode 6",
              before=(lambda ctx: ctx.build_accel(),))
    states = [a, b, c, d, e, f, g, h]
    called = set()
    multi = capi.Context(devices=[0, 0], transport="memcpy")
    assert multi.num_ranks == 2
    for name in ("set_lines", "set_trajectories", "set_tube_triangle_mesh", "set_transfer_function", "set_twist_line_texture", "set_camera",
                 "set_background", "set_option", "set_ao_parametrization", "build_accel"):
        def spy(*args, _f=getattr(multi, name), _n=name, **kw):
            if multi.frames:
                called.add(_n)
            return _f(*args, **kw)
        setattr(multi, name, spy)
    multi.frames = 0
    render = multi.render

    def counting_render(*args, **kw):
        multi.frames += 1
        return render(*args, **kw)
    multi.render = counting_render
    compared, _ = run_walk(states, ctx=multi)
    assert compared == len(states)
    assert called == {"set_lines", "set_trajectories", "set_tube_triangle_mesh", "set_transfer_function", "set_twist_line_texture",
                      "set_camera", "set_background", "set_option", "set_ao_parametrization", "build_accel"}, called


# ---------------------------------------------------------------- walk G: the prebaker
def test_walk_g_prebaker_tables_follow_the_data(hip_lib):
    from test_gpu_prebaker import PREBAKE
    s = dict(PREBAKE, rtao_prebaker_iterations=2, rtao_prebaker_samples_per_frame=4, rtao_prebaker_num_tube_subdivisions=8)

    def data(seed, lw):
        tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=seed))
        pts, seg = scene_arrays(tr, lw)
        mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
        return tr, case_of(pts, seg, tfm.standard(), 96, 64, lw, **s), mesh, lvo.ao_parametrization(tr.positions, tr.line_offsets, 0.01)
    tr1, c1, mesh1, param1 = data(7, 0.02)
    _, c1w, mesh1w, _ = data(7, 0.01)
    tr2, c2, mesh2, param2 = data(3, 0.02)

    def anchor_baked(st, got):
        """the table and the frame of the replaced lines against the oracle's bake"""
        c = st.case
        sc = c.oracle_scene()
        P = c.oracle_params(sc)
        P.useAmbientOcclusion = 1            # (oracle_params switches it on for the screen-space mode only)
        ts = lvo.TriScene(*mesh2, c.line_width)
        fac = lvo.bake_ao(sc, ts, c.line_width, param2[1], 8, 4, 2, use_bvh=True)
        assert np.array_equal(bits(got["baked"]), bits(fac)) and float(fac.min()) < 0.8
        assert max_lsb_diff(got["frame"], lvo.render_rt_prebaked(sc, None, P, fac, param2[0])) <= LSB_TOL

    def start_and_finish(ctx):
        """lv_bake_ao_start / lv_bake_ao_poll to completion (lv_get_baked_ao waits for a started bake)"""
        ctx.bake_ao_start()
        ctx.bake_ao_poll()
        ctx.get_baked_ao(8)
        assert ctx.bake_ao_poll() == (False, True)
    first = State(c1, mesh=mesh1, param=param1, reads=("baked",), label="1: bake")
    states = [
        first,
        first.but(reads=("frame", "baked"), label="2: render"),
        State(c1w, mesh=mesh1w, param=param1, reads=("baked", "frame"), label="3: line width: re-baked", data=first.data),
        State(c2, mesh=mesh2, param=param2, reads=("frame", "baked"), label="4 + 5: other lines, asynchronous bake to completion",
              before=(start_and_finish,), anchor=anchor_baked),
        State(c1, mesh=mesh1, param=param1, reads=("frame", "baked"), label="6 + 7: the first lines again, nothing pending"),
    ]
    ctx = capi.Context(0)
    tables = []
    keep = ctx.get_baked_ao

    def remember(*a, **kw):
        tables.append(keep(*a, **kw))
        return tables[-1]
    ctx.get_baked_ao = remember
    compared, _ = run_walk(states, ctx=ctx)
    assert compared == len(states)
    assert not np.array_equal(tables[0], tables[2]) and np.array_equal(tables[0], tables[-1])     # re-baked, and back


# ---------------------------------------------------------------- temporal state: progressive accumulation
PROGRESSIVE = dict(RTAO, ambient_occlusion_iterations=3, rtao_geometry="capsules", num_accumulated_frames=4, num_samples_per_frame=2,
                   ambient_occlusion_denoiser="None", eaw_denoiser_iterations=1)
N_FRAMES = 4


def sequence(ctx, n=N_FRAMES, mode=11):
    frames = []
    for f in range(n):
        ctx.set_option("frame_number", f)
        frames.append(ctx.render(mode).copy())
    return frames


def progressive_states():
    a = State(lines_case(30, 30, 7, 0.02, **PROGRESSIVE)[0], label="A")
    b = State(lines_case(12, 20, 4, 0.05, **PROGRESSIVE)[0], label="B")
    return a, b


def test_progressive_accumulation_restarts_like_a_fresh_context(hip_lib):
    """frames frame_number = 0 ... n-1 of a reused context equal a fresh context's after a data-set change, after a viewport change and
    after a detour through modes 2, 3 and 6 (the accumulation image and the RTAO accumulation start over)"""
    a, b = progressive_states()
    small = b.but(width=70, height=50, label="B at 70 x 50")
    ctx = fresh(a)
    first = sequence(ctx)
    assert not np.array_equal(first[0], first[-1])
    prev = a
    for st, what in ((b, "data-set change"), (small, "viewport change"), (b, "viewport change + detour")):
        ctx.set_option("frame_number", 0)
        apply(ctx, prev, st)
        prev = st
        if "detour" in what:
            for mode in (2, 3, 6):
                ctx.render(mode)
        got = sequence(ctx)
        f = fresh(st)
        want = sequence(f)
        f.close()
        for k in range(N_FRAMES):
            assert np.array_equal(got[k], want[k]), (what, k)
        assert covered(st, dict(frame=want[-1])) >= MIN_COVERED and not np.array_equal(want[0], want[-1])
        if what == "data-set change":          # the oracle anchor
            ref = st.case.oracle_render_progressive(N_FRAMES)
            for k in range(N_FRAMES):
                assert max_lsb_diff(got[k], ref[k]) <= LSB_TOL, k
    ctx.close()


def test_viewport_change_in_a_running_accumulation_is_rejected(hip_lib):
    a, _ = progressive_states()
    ctx = fresh(a)
    got = sequence(ctx, 2)
    other = a.but(width=70, height=50)
    c = other.case
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    ctx.set_option("frame_number", 2)
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(11)
    assert e.value.code == E_STATE and ctx.L.lv_last_error(ctx.h)
    f = fresh(other)                   # still usable: from frame 0 it is a fresh context's accumulation at the new size
    for x, y in zip(sequence(ctx), sequence(f)):
        assert np.array_equal(x, y)
    c = a.case
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    for x, y in zip(sequence(ctx, 2), got):
        assert np.array_equal(x, y)


def test_denoiser_change_in_a_running_accumulation_is_rejected(hip_lib):
    a, _ = progressive_states()
    ctx = fresh(a)
    sequence(ctx, 2)
    eaw = a.but(ambient_occlusion_denoiser="EAW")
    apply(ctx, a, eaw)
    ctx.set_option("frame_number", 2)
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(11)
    assert e.value.code == E_STATE and ctx.L.lv_last_error(ctx.h)
    f = fresh(eaw)                     # it restarts cleanly at 0
    want = sequence(f)
    for x, y in zip(sequence(ctx), want):
        assert np.array_equal(x, y)
    plain = sequence(fresh(a))
    assert not np.array_equal(plain[-1], want[-1])       # the denoiser reaches the frames


# ---------------------------------------------------------------- temporal state: SVGF
def svgf_frames(ctx, n):
    out = []
    for _ in range(n):
        img = ctx.render(11)
        out.append((img, ctx.get_ao()))
    return out


def test_svgf_history_is_cleared_by_a_viewport_change(hip_lib):
    """V.width != ctx->width: fresh history images.  lv_set_lines keeps the history (next test) and returns the RTAO seed counter to
    0, so viewport change + lv_set_lines leaves exactly a fresh context's state -- unless the viewport change kept the history.  The
    oracle is the second witness: a new lvo.Svgf of the new size that carries the frame counter and the last view-projection on."""
    from test_svgf import fat_case
    c = fat_case()
    small = case_of(c.points, c.seg, c.tf, 120, 90, c.line_width, **c.settings)
    ctx = c.hip_context()
    svgf_frames(ctx, 2)
    ctx.set_camera(small.view, small.proj, small.fovy, small.near, small.far, small.width, small.height)
    got = svgf_frames(ctx, 2)
    sc = c.oracle_scene()
    big = lvo.Svgf(c.width, c.height)
    P = c.oracle_params(sc)
    for _ in range(2):
        big.step(lambda: sc.render_ao(P), P)
    sv = lvo.Svgf(small.width, small.height)
    sv.global_frame_number, sv.last_view_proj = big.global_frame_number, big.last_view_proj
    P = small.oracle_params(sc)
    for img, ao in got:
        ao_ref = sv.step(lambda: sc.render_ao(P), P)
        assert np.abs(ao - ao_ref).max() < 3e-5 and max_lsb_diff(img, sc.render_rt(P, ao=ao_ref)) <= LSB_TOL
    assert np.abs(ao_ref - 1.0).max() > 0.2
    # byte for byte: back to the first size (history cleared again), the same lines again (seed counter 0) = a fresh context
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    ctx.set_lines(c.points, c.seg)
    f = c.hip_context()
    for (img, ao), (fimg, fao) in zip(svgf_frames(ctx, 2), svgf_frames(f, 2)):
        assert np.array_equal(img, fimg) and np.array_equal(bits(ao), bits(fao))


def test_svgf_history_is_kept_across_set_lines(hip_lib):
    """SVGFDenoiser::resetFrameNumber is empty in the reference: lv_set_lines returns globalFrameNumber to 0 and forgets the last
    view-projection, the history images stay.  The oracle's Svgf object is stepped on scene A, then on scene B."""
    from test_svgf import fat_case
    a = fat_case()
    b = case_of(a.points, a.seg[:4 * 29], a.tf, a.width, a.height, a.line_width, **a.settings)   # four of A's six lines: their history applies
    ctx = a.hip_context()
    sv = lvo.Svgf(a.width, a.height)
    history_matters = None
    for n, c in enumerate((a, b)):
        if n:
            ctx.set_lines(c.points, c.seg)
            sv.global_frame_number, sv.last_view_proj = 0, None
        sc = c.oracle_scene()
        P = c.oracle_params(sc)
        for k, (img, ao) in enumerate(svgf_frames(ctx, 2)):
            ao_ref = sv.step(lambda: sc.render_ao(P), P)
            assert np.abs(ao - ao_ref).max() < 3e-5, (n, k)
            assert max_lsb_diff(img, sc.render_rt(P, ao=ao_ref)) <= LSB_TOL, (n, k)
            if n and k == 0:
                history_matters = ao
    f = b.hip_context()                # the rule is visible: a context without A's history denoises B's first frame differently
    f.render(11)
    assert np.abs(f.get_ao() - history_matters).max() > 1e-3


# ---------------------------------------------------------------- rejected calls
@pytest.mark.parametrize("data", ["lines", "trajectories"])
def test_rejected_calls_leave_the_context_as_it_was(hip_lib, data):
    """a call that fails its input validation touches nothing: the next frame, AO image, hits and lines are those before the call"""
    s = dict(RTAO, rtao_geometry="auto", ppll_fragment_source="auto")
    c, tr = lines_case(30, 30, 7, 0.02, **s)
    st = State(c, reads=("frame", "ao", "hits", "lines", "stats"), traj=traj_of(tr) if data == "trajectories" else None)
    ctx = fresh(st)
    before = observe(ctx, st)
    assert covered(st, before) >= MIN_COVERED
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, 0.02, 6)
    bad_seg = c.seg.copy()
    bad_seg[5, 1] = len(c.points)
    bad_idx = mesh[0].copy()
    bad_idx[3, 1] = len(mesh[1])
    n = len(tr.positions)
    down = np.array([0, n // 2, n // 4, n], np.uint32)
    hel = np.linspace(-1, 1, n).astype(np.float32)

    def bad_mode_3():
        ctx.set_option("ppll_fragment_source", "capsule_entry")        # accepted; mode 3 rejects the combination
        try:
            ctx.render(3)
        finally:
            ctx.set_option("ppll_fragment_source", "auto")
    calls = [
        ("lv_set_lines, index out of range", lambda: ctx.set_lines(c.points, bad_seg), E_INVALID),
        ("lv_set_trajectories, decreasing offsets", lambda: ctx.set_trajectories(tr.positions, None, down), E_INVALID),
        ("lv_set_trajectories, NaN max_helicity", lambda: ctx.set_trajectories(tr.positions, None, tr.line_offsets, helicity=hel,
                                                                              max_helicity=float("nan")), E_INVALID),
        ("lv_set_tube_triangle_mesh, bad vertex index", lambda: ctx.set_tube_triangle_mesh(bad_idx, mesh[1], mesh[2]), E_INVALID),
        ("lv_render, unsupported mode", lambda: ctx.render(7), E_INVALID),
        ("lv_render, unsupported combination", bad_mode_3, E_INVALID),
    ]
    for key, value in (("line_width", -1.0), ("overlap_primary_passes", "Auto"), ("overlap_primary_passes", "on"),
                       ("ambient_occlusion_denoiser", "median"), ("rtao_geometry", "spheres"), ("geometry_mode", "Curved Swept Spheres"),
                       ("tube_num_subdivisions", 2), ("accel_build", "slow"), ("treelet_leaves", 2), ("no_such_key", 1)):
        calls.append(("lv_set_option %s = %s" % (key, value), lambda k=key, v=value: ctx.set_option(k, v), E_INVALID))
    for name, call, code in calls:
        with pytest.raises(capi.LineVisError) as e:
            call()
        assert e.value.code == code, name
        assert ctx.L.lv_last_error(ctx.h), name
        assert_same(observe(ctx, st), before, name)
    for ok in ("auto", "true", "false", "1", "0"):
        ctx.set_option("overlap_primary_passes", ok)
    ctx.set_option("overlap_primary_passes", "auto")
    assert_same(observe(ctx, st), before, "overlap_primary_passes never changes a pixel")


# ---------------------------------------------------------------- device memory accounting
def test_finished_points_of_the_streamline_seeder_are_owned(hip_lib):
    """point-based termination checks keep the finished points (12 B) and their list links (4 B) in HBM: device_bytes must show them"""
    from test_gpu_flow import abc_grid
    v, mag, sp = abc_grid(24)
    hel = lvo.helicity_field(v, lvo.vorticity_field(v, sp))
    ctx = capi.Context(0)
    ctx.set_flow_grid(v, sp, [mag, hel])
    S = capi.streamline_settings("Runge-Kutta 4th Order", "Forward & Backward", minimum_length=0.3, max_num_iterations=400)
    ctx.trace_streamlines_max_helicity_first(hel, S, capi.HelicitySeedingSettings(termination_check_type=1))   # every shared buffer
    before = int(ctx.stats().device_bytes)
    pos, _, off = ctx.trace_streamlines_max_helicity_first(hel, S, capi.HelicitySeedingSettings(termination_check_type=2))
    after = int(ctx.stats().device_bytes)
    assert len(off) - 1 > 10 and len(pos) > 500
    assert after - before >= 16 * len(pos), (before, after, len(pos))


def test_build_accel_builds_no_triangle_lbvh_without_a_consumer(hip_lib):
    from test_gpu_band_trajectories import curves
    pos, att, off, rib, hel = curves(5, 12, 30)
    bytes_, nodes = {}, {}
    for consumer in (False, True):
        ctx = capi.Context(0)
        ctx.set_trajectories(pos, att, off, ribbon_directions=rib, helicity=hel)
        ctx.set_options(dict(NO_AO, rtao_geometry="capsules", rotating_helicity_bands=True, line_width=0.02,
                             geometry_mode="Triangle Mesh" if consumer else "AABBs"))
        ctx.build_accel()
        s = ctx.stats()
        bytes_[consumer], nodes[consumer] = int(s.device_bytes), (int(s.num_tri_nodes), int(s.tri_leaf_bytes), int(s.num_tube_triangles))
        ctx.close()
    assert nodes[False] == (0, 0, 0) and nodes[True][0] > 0 and nodes[True][1] > 0 and nodes[True][2] > 0
    assert bytes_[False] < bytes_[True]


# ---------------------------------------------------------------- plugin level
def test_plugin_keeps_one_renderer_across_data_sets_modes_and_resolutions(hip_lib):
    """host_api.HeadlessLineRenderer: one object, three LineDataFlow objects of different sizes, a set_new_state walk over modes 11,
    2, 3 and 6 at two resolutions per data set -- every frame is the frame of a renderer created for that state alone.  A flow object
    that replaces a dropped one (possibly at its address) is uploaded again."""
    def flow(n_lines, ppl, seed):
        tr = scenes.normalize(scenes.random_curves(n_lines=n_lines, points_per_line=ppl, seed=seed))
        return host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    tf = tfm.standard_transparent()
    settings = dict(line_width=0.03)

    def alone(make, mode, res):
        r = host_api.HeadlessLineRenderer(mode)
        r.set_transfer_function(tf)
        r.set_line_data(make())
        r.set_new_state("alone", mode, settings, resolution=res)
        return r.render_frame()
    r = host_api.HeadlessLineRenderer(11)
    r.set_transfer_function(tf)
    makers = [lambda: flow(40, 40, 7), lambda: flow(16, 20, 4), lambda: flow(25, 30, 5)]
    modes = [11, 2, 3, 6]
    last = None
    for i, make in enumerate(makers):
        r.set_line_data(make())
        for mode in (modes if i % 2 == 0 else modes[::-1]):      # the mode at a data-set change stays: its context sees the new data
            for res in ((96, 64), (150, 90)):
                r.set_new_state("walk", mode, settings, resolution=res)
                assert r.rendering_mode == mode
                img = r.render_frame()
                assert np.array_equal(img, alone(make, mode, res)), (i, mode, res)
                assert (img.reshape(-1, 4) != img[0, 0]).any(axis=1).sum() >= MIN_COVERED
                assert last is None or last.shape != img.shape or not np.array_equal(last, img)
                last = img
    # uploaded flow dropped, another one set but never rendered, a NEW object of other data set: it must be uploaded
    old = flow(40, 40, 7)
    r.set_line_data(old)
    first = r.render_frame()
    r.set_line_data(flow(16, 20, 4))
    del old
    r.set_line_data(flow(25, 30, 5))
    img = r.render_frame()
    assert np.array_equal(img, alone(makers[2], 6, (150, 90))) and not np.array_equal(img, first)
