"""lv_set_trajectories_with_bands: band data (ribbon directions -> elliptic tubes) and the rotating helicity bands built on the device --
the line points of getLinePassTubeAabbRenderData (ribbon normals, per-line lineRotation) and the capped triangle tubes of
getLinePassTubeTriangleMeshRenderData (elliptic tessellation, the table's rotation running on across all lines) byte for byte what
the host layer and the oracle produce, and frames from them identical to frames from the uploaded host geometry."""
import time
import zlib

import numpy as np
import pytest

from common import Case
from linevis_amd import capi, host_api, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

NAMES = ["Velocity Magnitude", "Helicity"]
RTAO_TRI = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, rtao_geometry="triangle_tubes",
                ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=8)


@pytest.fixture(autouse=True)
def _reset_static_switches():
    """LineDataFlow::useRibbons / useRotatingHelicityBands are static, as in the reference: every test leaves the ribbons on and the
    rotating helicity bands off (setTrajectoryData switches the ribbons off while the helicity bands are on)."""
    yield
    host_api.LineDataFlow().set_new_settings(dict(rotating_helicity_bands=False))
    host_api.LineDataFlow().set_new_settings(dict(use_ribbons=True))


def band_flow(pos, att, off, rib):
    flow = host_api.LineDataFlow().set_trajectories(pos, att, off, ribbon_directions=rib)
    return flow.set_new_settings(dict(rotating_helicity_bands=False, use_ribbons=True))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def curves(seed, lines, ppl):
    """Random curves with duplicated points (zero tangents), and after the first line a dropped line (no valid point), a one-point
    line and an empty line; twisted ribbons and a signed helicity per point."""
    tr = scenes.normalize(scenes.random_curves(n_lines=lines, points_per_line=ppl, seed=seed))
    pos = tr.positions.astype(np.float32).copy()
    att = (tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes).astype(np.float32)
    off = tr.line_offsets.astype(np.int64)
    rng = np.random.default_rng(seed)
    dup = rng.integers(1, len(pos), max(4, len(pos) // 40))
    pos[dup] = pos[dup - 1]
    b = int(off[1])
    extra = np.array([pos[b - 1] + 0.01] * 3 + [pos[b - 1] + 0.02], np.float32)
    pos = np.concatenate([pos[:b], extra, pos[b:]])
    att = np.concatenate([att[:b], np.linspace(0, 1, 4).astype(np.float32), att[b:]])
    off = np.concatenate([off[:2], [b + 3, b + 4, b + 4], off[2:] + 4]).astype(np.uint32)
    rib = scenes.twisted_ribbons(scenes.Trajectories(pos, att, off)).ribbon_directions
    hel = (0.03 * np.sin(np.arange(len(pos)) * 0.37 + seed) + 0.004).astype(np.float32)
    return pos, att, off, rib, hel


def fast_twisted_ribbons(tr, twist=6.0):
    """twisted_ribbons' construction without the parallel transport, vectorised over all points (the 1 M-point scene): a unit
    direction perpendicular to the central-difference tangent, rotated about it by `twist` radians per unit arc length."""
    p = tr.positions.astype(np.float64)
    off = tr.line_offsets.astype(np.int64)
    first = np.zeros(len(p), bool)
    first[off[:-1][off[:-1] < len(p)]] = True
    last = np.zeros(len(p), bool)
    last[off[1:][off[1:] > 0] - 1] = True
    ahead = np.where(last[:, None], p, np.roll(p, -1, axis=0))
    behind = np.where(first[:, None], p, np.roll(p, 1, axis=0))
    t = ahead - behind
    t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-12)
    a = np.where(np.abs(t[:, 1:2]) < 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    nrm = a - np.sum(a * t, axis=1, keepdims=True) * t
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)
    step = np.where(first, 0.0, np.linalg.norm(p - np.roll(p, 1, axis=0), axis=1))
    arc = np.cumsum(step)
    arc -= np.repeat(arc[off[:-1].clip(max=len(p) - 1)], np.diff(off))
    ang = twist * arc[:, None]
    return (np.cos(ang) * nrm + np.sin(ang) * np.cross(t, nrm)).astype(np.float32)


CASES = [(1, 35, 25), (2, 7, 40), (4, 6000, 3)]   # (seed, points per line, lines): the last one is longer than the 2048-point LDS chunk


def device(pos, att, off, **kw):
    opts = kw.pop("options", {})
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_trajectories(pos, att, off, **kw)
    return ctx


@pytest.mark.parametrize("seed,ppl,lines", CASES)
def test_band_data_geometry_is_byte_identical_to_host_and_oracle(hip_lib, seed, ppl, lines):
    pos, att, off, rib, hel = curves(seed, lines, ppl)
    flow = band_flow(pos, att, off, rib)
    ctx = device(pos, att, off, ribbon_directions=rib, options=dict(use_ribbons=True))
    for bw, mbt in ((0.05, 0.3), (0.012, 0.15)):
        ctx.set_option("band_width", bw)
        ctx.set_option("min_band_thickness", mbt)
        ctx.set_option("use_analytic_elliptic_tubes", True)
        pts, seg = ctx.get_lines()
        hp, hs, _ = flow.tube_aabb_render_data_elliptic(bw)
        op, os_, _ = lvo.build_tube_aabb_render_data_ribbons(pos, att, off, bw, rib)
        assert same_bytes(pts, hp) and np.array_equal(seg, hs) and same_bytes(pts, op) and np.array_equal(seg, os_)
        ctx.set_option("use_analytic_elliptic_tubes", False)     # band data with circular tubelets: Gram-Schmidt records
        pts, seg = ctx.get_lines()
        hp, hs, _ = flow.tube_aabb_render_data(0.02)
        assert same_bytes(pts, hp) and np.array_equal(seg, hs)
        for n in (4, 8, 9, 16):
            ctx.set_option("tube_num_subdivisions", n)
            mesh = ctx.get_tube_triangle_mesh()
            hm = flow.tube_triangle_render_data_bands(bw, mbt, n)
            om = lvo.build_tube_triangle_render_data_ribbons(pos, att, off, rib, bw, mbt, n)
            for a, h, o in zip(mesh, hm, om):
                assert same_bytes(a, h) and same_bytes(a, o)
    st = ctx.stats()
    assert st.ms_line_points > 0.0 and st.ms_tessellate > 0.0


@pytest.mark.parametrize("seed,ppl,lines", CASES)
def test_helicity_rotation_is_byte_identical_to_host_and_oracle(hip_lib, seed, ppl, lines):
    pos, att, off, rib, hel = curves(seed, lines, ppl)
    flow = host_api.LineDataFlow().set_trajectories_multi(pos, np.stack([att, hel]), NAMES, off)
    flow.set_new_settings(dict(rotating_helicity_bands=True))
    mh = flow.max_helicity
    assert mh == np.abs(hel).max()
    lw = 0.01
    hp, hs, _ = flow.tube_aabb_render_data(lw)
    op, _, _ = lvo.build_tube_aabb_render_data(pos, att, off, lw, helicities=hel, max_helicity=mh)
    assert same_bytes(hp, op) and hp["lineRotation"].any()
    for given in (mh, 0.0):                                    # 0: max |helicity| reduced on the device
        ctx = device(pos, att, off, helicity=hel, max_helicity=given, options=dict(rotating_helicity_bands=True, line_width=lw))
        pts, seg = ctx.get_lines()
        assert same_bytes(pts, hp) and np.array_equal(seg, hs)
        for n in (4, 9):
            ctx.set_option("tube_num_subdivisions", n)
            mesh = ctx.get_tube_triangle_mesh()
            hm = flow.tube_triangle_render_data(lw, n)
            om = lvo.build_tube_triangle_render_data(pos, att, off, lw, n, helicities=hel, max_helicity=mh)
            for a, h, o in zip(mesh, hm, om):
                assert same_bytes(a, h) and same_bytes(a, o)
        ctx.set_option("rotating_helicity_bands", False)       # the same data without the bands: rotation 0 everywhere
        assert same_bytes(ctx.get_lines()[0], lvo.build_tube_aabb_render_data(pos, att, off, lw)[0])
        assert same_bytes(ctx.get_tube_triangle_mesh()[2], lvo.build_tube_triangle_render_data(pos, att, off, lw, 9)[2])
    ctx = device(pos, att, off, helicity=hel, max_helicity=2.0 * mh, options=dict(rotating_helicity_bands=True, line_width=lw))
    op2, _, _ = lvo.build_tube_aabb_render_data(pos, att, off, lw, helicities=hel, max_helicity=2.0 * mh)
    assert same_bytes(ctx.get_lines()[0], op2)


def test_option_changes_follow_and_frames_match_the_uploaded_geometry(hip_lib):
    """After one upload: band_width, use_analytic_elliptic_tubes, rotating_helicity_bands, geometry mode and renderer change; every
    frame and AO buffer equals the one of a context fed lv_set_lines + lv_set_tube_triangle_mesh from the host layer."""
    pos, att, off, rib, hel = curves(5, 12, 30)
    flow = band_flow(pos, att, off, rib)
    lw, n = 0.02, 8
    dev = None
    steps = [(11, 0.05, 0.3, True), (11, 0.03, 0.3, True), (11, 0.03, 0.3, False), (2, 0.03, 0.2, True)]
    for mode, bw, mbt, elliptic in steps:
        pts, seg, _ = flow.tube_aabb_render_data_elliptic(bw) if elliptic else flow.tube_aabb_render_data(lw)
        s = dict(use_ribbons=True, band_width=bw, min_band_thickness=mbt, use_analytic_elliptic_tubes=elliptic, tube_num_subdivisions=n)
        s.update(RTAO_TRI if mode == 11 else dict(ambient_occlusion_mode="None"))
        c = Case(pts, seg, tfm.standard_transparent() if mode == 2 else tfm.standard(), 160, 112, lw, **s)
        up = c.hip_context()
        if mode == 11:
            up.set_tube_triangle_mesh(*flow.tube_triangle_render_data_bands(bw, mbt, n))
        want = up.render(mode)
        if dev is None:
            dev = c.hip_context()
            dev.set_trajectories(pos, att, off, ribbon_directions=rib, helicity=hel)
        else:
            dev.set_options(s)
            dev.set_transfer_function(c.tf, 0.0, 1.0)
        got = dev.render(mode)
        assert np.array_equal(got, want) and (got[..., :3] != 255).any(axis=2).sum() > 300
        if mode == 11:
            assert np.array_equal(dev.get_ao().view(np.uint32), up.get_ao().view(np.uint32))
            assert (up.get_ao() < 1.0).sum() > 200
    # the same context, the same upload: the rotating helicity bands in "Triangle Mesh" mode and in the AABB mode with PPLL
    hflow = host_api.LineDataFlow().set_trajectories_multi(pos, np.stack([att, hel]), NAMES, off)
    hflow.set_new_settings(dict(rotating_helicity_bands=True))
    pts, seg, _ = hflow.tube_aabb_render_data(lw)
    for mode, s in ((11, dict(geometry_mode="Triangle Mesh", **RTAO_TRI)), (2, dict(geometry_mode="AABBs", ambient_occlusion_mode="None"))):
        s.update(use_ribbons=False, use_analytic_elliptic_tubes=False, rotating_helicity_bands=True, tube_num_subdivisions=n,
                 helicity_rotation_factor=0.25)
        c = Case(pts, seg, tfm.standard_transparent() if mode == 2 else tfm.standard(), 160, 112, lw, **s)
        up = c.hip_context()
        up.set_tube_triangle_mesh(*hflow.tube_triangle_render_data(lw, n))
        want = up.render(mode)
        dev.set_options(s)
        dev.set_transfer_function(c.tf, 0.0, 1.0)
        assert np.array_equal(dev.render(mode), want)
        if mode == 11:
            assert np.array_equal(dev.get_ao().view(np.uint32), up.get_ao().view(np.uint32))
    dev.set_option("rotating_helicity_bands", False)
    assert not np.array_equal(dev.render(2), want)


@pytest.mark.parametrize("kind", ["bands", "helicity"])
def test_plugin_surface_uses_the_device_geometry_for_band_and_helicity_data(hip_lib, kind):
    def data(seed):
        pos, att, off, rib, hel = curves(seed, 10, 30)
        if kind == "bands":
            return band_flow(pos, att, off, rib)
        return host_api.LineDataFlow().set_trajectories_multi(pos, np.stack([att, hel]), NAMES, off)
    if kind == "bands":
        settings = dict(line_width=0.02, band_width=0.04, min_band_thickness=0.3, use_analytic_elliptic_tubes=True, use_ribbons=True,
                        **RTAO_TRI)
        change = dict(band_width=0.025)
    else:
        settings = dict(line_width=0.02, rotating_helicity_bands=True, helicity_rotation_factor=0.25, geometry_mode="Triangle Mesh",
                        **RTAO_TRI)
        change = dict(line_width=0.013)
    frames = {}
    for dg in (True, False):
        r = host_api.HeadlessLineRenderer(11)
        r.set_rendering_resolution(160, 96)
        r.set_transfer_function(tfm.standard())
        r.set_new_settings(dict(use_device_geometry=dg))
        r.set_line_data(data(3))
        r.set_new_settings(settings)
        out = [r.render_frame().copy()]
        r.set_new_settings(change)
        out.append(r.render_frame().copy())
        r.set_line_data(data(9))
        out.append(r.render_frame().copy())
        st = r.stats()
        assert (st.ms_line_points > 0.0) == dg and (st.ms_tessellate > 0.0) == dg
        frames[dg] = out
    for a, b in zip(frames[True], frames[False]):
        assert np.array_equal(a, b) and (a[..., :3] != 255).any(axis=2).sum() > 300
    assert not np.array_equal(frames[True][0], frames[True][1])


@pytest.mark.parametrize("kind", ["bands", "helicity"])
def test_config3_band_geometry_on_the_device(hip_lib, kind):
    """The config-3 tornado (1 M segments) with twisted ribbons / its attribute as helicity: mesh CRCs = the host layer's; a
    band_width / line_width change (tessellation + both LBVH builds, host-synchronous) under 100 ms."""
    tr = scenes.normalize(scenes.tornado())
    att = (tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes).astype(np.float32)
    ctx = capi.Context(0)
    if kind == "bands":
        rib = fast_twisted_ribbons(tr)
        flow = band_flow(tr.positions, att, tr.line_offsets, rib)
        for k, v in dict(use_ribbons=True, band_width=0.004, min_band_thickness=0.3, tube_num_subdivisions=8).items():
            ctx.set_option(k, v)
        t0 = time.perf_counter()
        ctx.set_trajectories(tr.positions, att, tr.line_offsets, ribbon_directions=rib)
        hm = flow.tube_triangle_render_data_bands(0.004, 0.3, 8)
        key, values = "band_width", (0.004, 0.005)
    else:
        hel = (att - att.mean()).astype(np.float32)
        flow = host_api.LineDataFlow().set_trajectories_multi(tr.positions, np.stack([att, hel]), NAMES, tr.line_offsets)
        flow.set_new_settings(dict(rotating_helicity_bands=True))
        ctx.set_option("rotating_helicity_bands", True)
        ctx.set_option("line_width", 0.002)
        t0 = time.perf_counter()
        ctx.set_trajectories(tr.positions, att, tr.line_offsets, helicity=hel)
        hm = flow.tube_triangle_render_data(0.002, 6)
        key, values = "line_width", (0.002, 0.0025)
    set_ms = (time.perf_counter() - t0) * 1e3
    st = ctx.stats()
    print("\n[%s] set_trajectories_with_bands %.1f ms wall, ms_line_points %.2f" % (kind, set_ms, st.ms_line_points))
    mesh = ctx.get_tube_triangle_mesh()
    for a, b in zip(mesh, hm):
        assert zlib.crc32(np.ascontiguousarray(a).view(np.uint8)) == zlib.crc32(np.ascontiguousarray(b).view(np.uint8))
    if kind == "helicity":
        assert mesh[2]["lineRotation"].any()
    ctx.set_option("geometry_mode", "Triangle Mesh")         # a consumer of the tube mesh: lv_build_accel builds what the options use
    ctx.build_accel()
    ctx.set_option(key, values[1])
    t0 = time.perf_counter()
    ctx.build_accel()                                        # tessellation + segment LBVH + triangle LBVH, host-synchronous
    wall_ms = (time.perf_counter() - t0) * 1e3
    st = ctx.stats()
    print("[%s] %s change: %.1f ms wall, ms_tessellate %.2f, ms_tri_accel_build %.2f, ms_accel_build %.2f"
          % (kind, key, wall_ms, st.ms_tessellate, st.ms_tri_accel_build, st.ms_accel_build))
    assert st.ms_tessellate > 0.0 and st.ms_tri_accel_build > 0.0 and wall_ms < 100.0


def test_errors(hip_lib):
    pos, att, off, rib, hel = curves(2, 7, 40)
    ctx = capi.Context(0)
    with pytest.raises(ValueError):
        ctx.set_trajectories(pos, att, off, ribbon_directions=rib[:-1])
    with pytest.raises(ValueError):
        ctx.set_trajectories(pos, att, off, helicity=hel[:-1])
    with pytest.raises(capi.LineVisError):
        ctx.set_trajectories(pos, att, off, helicity=hel, max_helicity=float("nan"))
    ctx.set_trajectories(pos, att, off)
    ctx.set_option("use_ribbons", True)
    with pytest.raises(capi.LineVisError):
        ctx.get_tube_triangle_mesh()
    with pytest.raises(capi.LineVisError):
        ctx.get_lines()
    ctx.set_option("use_ribbons", False)
    ctx.set_trajectories(pos, att, off, ribbon_directions=rib)   # ribbons, but no helicity
    ctx.set_option("rotating_helicity_bands", True)
    with pytest.raises(capi.LineVisError):
        ctx.get_tube_triangle_mesh()
    ctx.set_option("rotating_helicity_bands", False)
    assert len(ctx.get_lines()[0]) > 0
