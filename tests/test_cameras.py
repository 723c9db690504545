"""The oracle under general view and projection matrices, against float64 (no GPU): the camera family of tests/cameras.py applied to
the whole-frame float64 ray tracer of test_independent_restatement2.py, to the independent float64 screen-space rasteriser of
test_prism_raster.py (extended by the near / far acceptance and by triangles that reach behind the camera plane), and to the small
pieces of camera arithmetic that had no float64 check under a general camera: the 4 x 4 inverse, MLAB's window depth, the depth range
of the depth cues, the view-space feature maps of the EAW / SVGF passes.  The oracle is the reference of the GPU comparison
(test_gpu_cameras.py); this file is what entitles it to that role away from the default camera."""
import numpy as np
import pytest

import cameras
from common import small_case
from oracle import lvo
import test_independent_restatement2 as ir2
import test_prism_raster as pr
from test_mlab_restatement import window_depth

EPS32 = 2.0 ** -23
# cameras whose hit distances exceed ~1.5: the reference's textbook roots lose digits with the distance, the frame is
# compared in the closest-approach form there; every other camera is compared on the literal roots like the committed test
FAR_CAMERAS = ("narrow_far",)


def mat(m):
    """column-major flat float32 -> float64 maths matrix"""
    return np.asarray(m, np.float64).reshape(4, 4).T


# ---------------------------------------------------------------- whole ray-tracer frames
@pytest.mark.parametrize("viewport", ["wide", "tall"])
@pytest.mark.parametrize("cam", cameras.NAMES)
def test_ray_tracer_frame_against_the_float64_restatement(cam, viewport):
    """RayGen (inverse projection, inverse view, camera position), the intersection roots and the shading under every camera: the
    committed bars of test_whole_frame_of_the_ray_tracer_against_the_float64_restatement (> 0.995 of the pixels within 1 LSB, at most
    6 pixels beyond 2 LSB where ~400 pixels are covered; the count scales with the covered pixels beyond that)."""
    w, h = cameras.VIEWPORTS[viewport]
    c = small_case(width=w, height=h, n_lines=14, pts_per_line=10, line_width=0.05, transparent=True, background=(0.9, 0.95, 1.0, 1.0),
                   camera=cam)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    with lvo.deviation_switches(literal_intersection=cam not in FAR_CAMERAS):
        got = sc.render_rt(P, use_bvh=False)
        assert np.array_equal(sc.render_rt(P, use_bvh=True), got)
    want, hit = ir2.render_rt_float64(c, P)
    want8 = np.floor(np.clip(want, 0.0, 1.0) * 255.0 + 0.5).astype(np.int32)
    d = np.abs(got.astype(np.int32) - want8).max(axis=2)
    covered = int(hit.sum())
    bar = 6 if covered <= 400 else 6 * covered // 400
    print("%s %s: covered %d, within 1 LSB %.4f, beyond 2 LSB %d (bar %d)" % (cam, viewport, covered, (d <= 1).mean(), (d > 2).sum(), bar))
    assert covered > 100
    assert (d <= 1).mean() > 0.995 and (d > 2).sum() <= bar, ((d > 1).sum(), (d > 2).sum(), d.max())


# ---------------------------------------------------------------- prism fragments
N_SUB = 6
# Weights.  The oracle (and the HIP fragment stage) obtain the perspective-correct weights of a fragment as b_i = e_i / (e0 + e1 + e2),
# e_i = det[V_j - o, V_k - o, ray] in float32, evaluated in the ray's own basis (lv_oracle_prism.h): there e_i is |ray| times a 2 x 2
# minor of the vertices' coordinates perpendicular to the ray.  Those coordinates are of the size s of the triangle but carry the
# rounding of vectors of the size of the distance d (a difference and a three-term dot product each: up to 4 eps32 d), so the minor is
# off by up to 4 eps32 d * 4 s, while e0 + e1 + e2 = 2 Area cos(tilt) |ray|.  With the screen scale f_px / (d cos(phi)) (f_px =
# |proj[5]| H / 2 pixels per unit tangent, phi = the off-axis angle of the fragment) that is
#       |weight error|  <=  8 * eps32 * f_px * L_px / (A_px * cos^2(phi)),
# L_px the longest screen edge and A_px the screen area of the triangle: the error grows with 1 / (screen area), with the focal length
# in pixels and with 1 / cos^2 off axis -- and with nothing else.  The constant 8 is the worst case of the rounding count above.
# Measured (this scene, 150 x 100 and 60 x 130): 0.29 / 0.23 for the default camera, 0.21 .. 0.64 over the family (lens shift 0.23,
# near / far = 0.001 / 10000: 0.29, near / far = 0.6 / 0.95 with cond(proj) = 7: 0.27), 2.8 for tubes 2.4 radii from the eye.  It does
# not follow cond(proj) (7 .. 6000 over the family), so the float32 inverse projection is not what limits it.  The committed absolute
# bar of 1e-4 (test_prism_raster.py, unchanged) is 0.7 of this formula at the default camera's f_px = 100 and its slivers of ~0.15 px^2.
K_WEIGHT = 8.0
# Position and depth.  position = sum b_i V_i and depth = |position - eye| in float32: the weight error times the triangle's longest
# edge, plus the roundings of three products, two sums and one length: 4 ulps of the larger of |V| and the distance.  Measured beyond
# the measured weight term: 0.53 (position) and 0.85 (depth) of an ulp for the default camera, at most 1.1 and 2.0 over the family.
# In ulps of the depth alone the default camera needs 8.3 (its committed absolute bar of 1e-6 is 16 ulps at 0.8) -- but the cameras
# at distance ~0.15 need 100, because the weight term is absolute (an edge of 0.03 times 5e-5): a bar relative to the distance alone
# cannot hold for them, so the bar has both terms.
K_POSITION = 4.0


def triangle_geometry(c, V):
    """(screen area in px^2, longest screen edge in px, longest world edge) of a triangle; area None if a vertex is behind the camera"""
    cl = np.concatenate([V, np.ones((3, 1))], 1) @ (mat(c.proj) @ mat(c.view)).T
    edges = ((0, 1), (1, 2), (2, 0))
    lw = max(np.linalg.norm(V[i] - V[j]) for i, j in edges)
    if (cl[:, 3] <= 0).any():
        return None, None, lw
    S = np.stack([(cl[:, 0] / cl[:, 3] + 1.0) * 0.5 * c.width, (cl[:, 1] / cl[:, 3] + 1.0) * 0.5 * c.height], 1)
    a = abs((S[1, 0] - S[0, 0]) * (S[2, 1] - S[0, 1]) - (S[1, 1] - S[0, 1]) * (S[2, 0] - S[0, 0])) / 2.0
    return a, max(np.linalg.norm(S[i] - S[j]) for i, j in edges), lw


def compare_prism_fragments(c):
    """The oracle's fragments against the float64 rasteriser: counts, and for every checked fragment the errors of weights, position
    and depth in units of their bars (see K_WEIGHT / K_POSITION)."""
    sc, P = pr.prism_params(c)
    fr = sc.prism_fragments(P)
    fr_bvh = sc.prism_fragments(P, use_bvh=True)
    for k in ("offsets", "seg", "tri", "weights", "depth"):
        assert np.array_equal(fr[k], fr_bvh[k]), k                          # BVH and brute-force candidates: identical fragments
    offs = fr["offsets"].astype(np.int64)
    want, pos, nrm, cam = pr.screen_space_rasteriser(c, P, N_SUB, near_far=(c.near, c.far), behind_camera=True)
    got = {}
    for pix in range(c.width * c.height):
        for i in range(offs[pix], offs[pix + 1]):
            got.setdefault((pix % c.width, pix // c.width), {})[(int(fr["seg"][i]), int(fr["tri"][i]))] = i
    pat = dict(pr.triangles64(c, N_SUB)[1])
    tan = c.points["lineTangent"].astype(np.float64)
    att = c.points["lineAttribute"].astype(np.float64)
    f_px = abs(float(c.proj[5])) * c.height / 2.0
    st = dict(fragments=len(fr["seg"]), checked=0, edge=0, extra=0, behind=0, w=0.0, pos=0.0, depth=0.0, w_abs=0.0)
    for key, lst in want.items():
        for (s, tt, w64, margin) in lst:
            i = got.get(key, {}).get((s, tt))
            if margin < 1e-4:        # pixel centre within 1e-4 of an edge (barycentric units) or 1e-5 of a clip plane: either answer
                st["edge"] += 1
                continue
            assert i is not None, ("missing fragment", key, s, tt, margin)
            st["checked"] += 1
            verts = pat[tt]
            pi = [c.seg[s, r] for r, _ in verts]
            V = np.array([pos[p, k] for p, (_, k) in zip(pi, verts)])
            Nn = np.array([nrm[p, k] for p, (_, k) in zip(pi, verts)])
            fp = w64 @ V
            dist = float(np.linalg.norm(fp - cam))
            zv = -float(cameras.view_space_z(c, fp))
            assert c.near * (1 - 1e-5) <= zv <= c.far * (1 + 1e-5)
            a_px, l_px, l_world = triangle_geometry(c, V)
            ew = float(np.abs(fr["weights"][i] - w64).max())
            if a_px is None:
                st["behind"] += 1   # a vertex behind the camera plane: no screen triangle to scale by, the weights get the absolute bar
                bar_w = 1e-4
            else:
                bar_w = K_WEIGHT * EPS32 * f_px * l_px / (a_px * (zv / dist) ** 2)
            bar_p = bar_w * l_world + K_POSITION * EPS32 * max(float(np.abs(V).max()), dist)
            st["w"] = max(st["w"], ew / bar_w)
            st["w_abs"] = max(st["w_abs"], ew)
            st["pos"] = max(st["pos"], float(np.abs(fr["pos"][i] - fp).max()) / bar_p)
            st["depth"] = max(st["depth"], abs(float(fr["depth"][i]) - dist) / bar_p)
            assert np.abs(fr["normal"][i] - w64 @ Nn).max() < 2e-5 + 2.0 * bar_w
            assert np.abs(fr["tangent"][i] - w64 @ tan[pi]).max() < 2e-5 + 2.0 * bar_w
            assert abs(float(fr["attr"][i]) - float(w64 @ att[pi])) < 2e-5 + 2.0 * bar_w
    # ... and nothing else: every oracle fragment is one of the rasteriser's (edge cases aside)
    for key, d in got.items():
        ws = {(s, tt) for (s, tt, _, m) in want.get(key, [])}
        for (s, tt), i in d.items():
            if (s, tt) not in ws:
                assert fr["weights"][i].min() < 1e-4, ("fragment the rasteriser does not produce", key, s, tt, fr["weights"][i])
                st["extra"] += 1
    return st


@pytest.mark.parametrize("viewport", [(150, 100), (60, 130)])
@pytest.mark.parametrize("cam", cameras.NAMES)
def test_prism_fragments_against_the_float64_rasteriser(cam, viewport):
    """Coverage (no missing and no extra fragment), the near / far acceptance, triangles that straddle the camera plane, weights,
    positions and depths of the rasterised prism under every camera."""
    c = small_case(width=viewport[0], height=viewport[1], n_lines=10, pts_per_line=10, line_width=0.05, transparent=True, camera=cam)
    st = compare_prism_fragments(c)
    print(cam, viewport, st)
    assert st["checked"] > 100 and st["edge"] < 0.02 * st["checked"] and st["extra"] <= st["edge"] + 2
    assert st["w"] <= 1.0 and st["pos"] <= 1.0 and st["depth"] <= 1.0, st
    if cam in cameras.INSIDE:
        assert cameras.segments_straddling_the_camera_plane(c) > 0
    if cam == "tight_clip":
        wide = small_case(width=viewport[0], height=viewport[1], n_lines=10, pts_per_line=10, line_width=0.05, transparent=True)
        sc, P = pr.prism_params(wide)
        assert len(sc.prism_fragments(P)["seg"]) > st["fragments"] + 50          # the planes removed fragments


def test_prism_fragments_of_tubes_that_pass_the_camera():
    """Straight tubes that run from behind the camera plane into the picture, 2.4 radii beside the eye: their triangles have vertices
    with clip.w <= 0 and no screen-space triangle; the float64 side rasterises them in homogeneous coordinates.  Fragments of such
    triangles exist and agree."""
    from common import Case
    from linevis_amd import transfer_function as tfm
    lw = 0.05
    z = np.array([0.5, 0.2, -0.1, -0.4])
    pos = np.concatenate([np.stack([np.full(4, 0.06), np.full(4, 0.01), z], 1), np.stack([np.full(4, -0.02), np.full(4, -0.06), z + 0.03], 1),
                          np.stack([np.linspace(-0.3, 0.3, 4), np.full(4, 0.1), np.full(4, -0.3)], 1)]).astype(np.float32)
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, np.linspace(0.0, 1.0, 12).astype(np.float32), np.array([0, 4, 8, 12], np.uint32), lw)
    c = Case(pts, seg, tfm.standard_transparent(), 120, 90, lw)
    cameras.apply_camera(c, dict(eye=(0.0, 0.0, 0.0), target=(0.02, -0.01, -1.0), up=cameras.CAMERAS["roll37"]["up"], fovy=float(np.deg2rad(100.0)),
                                 near=0.001))
    st = compare_prism_fragments(c)
    print(st)
    assert cameras.segments_straddling_the_camera_plane(c) == 2 and st["behind"] > 100
    assert st["checked"] > 1000 and st["edge"] < 0.02 * st["checked"] and st["extra"] <= st["edge"] + 2
    assert st["w"] <= 1.0 and st["pos"] <= 1.0 and st["depth"] <= 1.0, st


# ---------------------------------------------------------------- the small pieces
def family_matrices():
    for name in cameras.NAMES:
        for w, h in cameras.VIEWPORTS.values():
            view, proj, _, _, _ = cameras.matrices(cameras.get(name), w, h)
            yield name, view, proj


def test_mat4_inverse_against_numpy():
    """The cofactor inverse in float32 (lvo.mat4_inverse; lv_mat4_inverse is its twin) against numpy.linalg.inv in float64: the
    error of a backward-stable inverse is a few eps32 * cond(M) relative to |M^-1|; the cofactor expansion stays inside 4."""
    worst = 0.0
    for name, view, proj in family_matrices():
        for m in (view, proj):
            want = np.linalg.inv(mat(m))
            got = mat(lvo.mat4_inverse(m))
            rel = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, rel / (EPS32 * np.linalg.cond(mat(m))))
            assert rel <= 4.0 * EPS32 * np.linalg.cond(mat(m)), (name, rel, np.linalg.cond(mat(m)))
    print("mat4_inverse: worst error %.3f eps32 cond(M)" % worst)


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_window_depth_against_float64(cam):
    """MLAB's window depth: clip.z / clip.w of proj * view (rows z and w summed in float32) at the positions of the oracle's fragments.
    z_window = (A z_view + B) / -z_view with B = -far near / (far - near): a relative error e of z_view moves it by ~ e near / depth,
    and its own roundings are ulps of 1."""
    c = small_case(width=96, height=64, transparent=True, camera=cam)
    sc, P = pr.prism_params(c)
    pos = sc.prism_fragments(P, use_bvh=True)["pos"]
    assert len(pos) > 300
    got = window_depth(pos, c.view, c.proj).astype(np.float64)
    clip = np.concatenate([pos.astype(np.float64), np.ones((len(pos), 1))], 1) @ (mat(c.proj) @ mat(c.view)).T
    want = clip[:, 2] / clip[:, 3]
    assert (want >= -1e-6).all() and (want <= 1.0 + 1e-6).all()             # the fragments lie between the planes
    assert np.abs(got - want).max() <= 8.0 * EPS32, np.abs(got - want).max()
    # the fold only needs the order: fragments whose float64 depths differ by more than the bar keep their order
    o = np.argsort(want)
    gap = np.diff(want[o]) > 16.0 * EPS32
    assert (np.diff(got[o])[gap] > 0).all()


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_depth_range_against_float64(cam):
    """ComputeDepthValues + MinMaxReduce: min / max over the line points inside the clip volume of clamp(-z_view, near, far) -/+ 0.01.
    Points within 1e-5 of a face of the volume may fall on either side in float32: the result lies between the range of the points
    clearly inside and the range of the points possibly inside."""
    c = small_case(width=96, height=64, camera=cam)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    got = sc.depth_range(P).astype(np.float64)
    p = np.concatenate([c.points["linePosition"].astype(np.float64), np.ones((len(c.points), 1))], 1)
    vs = p @ mat(c.view).T
    cl = vs @ mat(c.proj).T
    ndc = cl[:, :3] / cl[:, 3:4]
    depth = np.clip(-vs[:, 2], c.near, c.far)

    def rng(margin):
        inside = (np.abs(ndc) <= 1.0 + margin).all(axis=1)
        assert inside.sum() > 20
        return min(c.far, depth[inside].min() - 1e-2), max(c.near, depth[inside].max() + 1e-2)
    lo_in, hi_in = rng(-1e-5)
    lo_out, hi_out = rng(1e-5)
    tol = 4.0 * EPS32 * max(hi_out, 1.0)
    assert lo_out - tol <= got[0] <= lo_in + tol and hi_in - tol <= got[1] <= hi_out + tol, (got, lo_in, hi_in, lo_out, hi_out)
    if cam == "tight_clip":
        assert abs(got[0] - (c.near - 1e-2)) < 1e-6 and (-vs[:, 2] < c.near).any()      # the clamp was at work


def first_hits_float64(c, P):
    """closest capsule hit of every pixel-centre ray in float64, via the restatement's roots: (hit mask, position, geometric normal,
    distance to the runner-up hit)"""
    W, H = c.width, c.height
    view = np.asarray(P.view[:], np.float64)
    cam = ir2.ir.camera_position(view)
    inv_proj = np.linalg.inv(mat(P.proj[:]))
    inv_view = np.linalg.inv(mat(view))
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([2.0 * (xs + 0.5) / W - 1.0, 2.0 * (ys + 0.5) / H - 1.0, np.ones((H, W)), np.ones((H, W))], -1).reshape(-1, 4)
    tgt = ndc @ inv_proj.T
    dn = tgt[:, :3] / np.linalg.norm(tgt[:, :3], axis=1, keepdims=True)
    d = (np.concatenate([dn, np.zeros((len(dn), 1))], 1) @ inv_view.T)[:, :3]
    o = np.broadcast_to(cam, d.shape)
    p0s = c.points["linePosition"][c.seg[:, 0]].astype(np.float64)
    p1s = c.points["linePosition"][c.seg[:, 1]].astype(np.float64)
    r = c.line_width * 0.5
    best_t = np.full(len(d), np.inf)
    best_c = np.zeros((len(d), 3))                                           # the point of the axis the normal starts from
    second_t = np.full(len(d), np.inf)
    for s in range(len(c.seg)):
        ok, t = ir2.ray_tube(o, d, p0s[s], p1s[s], r)
        t = np.where(ok, t, np.inf)
        v = p1s[s] - p0s[s]
        fp = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
        ctr = p0s[s] + (((fp - p0s[s]) @ v) / (v @ v))[:, None] * v
        for e in (p0s[s], p1s[s]):
            oks, ts = ir2.ray_sphere(o, d, e, r)
            take = oks & (ts < t)
            t = np.where(take, ts, t)
            ctr = np.where(take[:, None], e, ctr)
        t = np.where(t >= 1e-4, t, np.inf)
        better = t < best_t
        second_t = np.where(better, best_t, np.minimum(second_t, t))
        best_c = np.where(better[:, None], ctr, best_c)
        best_t = np.where(better, t, best_t)
    hit = np.isfinite(best_t)
    fp = o + d * np.where(hit, best_t, 0.0)[:, None]
    n = fp - best_c
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    gap = np.where(hit & np.isfinite(second_t), second_t - np.where(hit, best_t, 0.0), np.inf)
    return hit.reshape(H, W), fp.reshape(H, W, 3), n.reshape(H, W, 3), gap.reshape(H, W)


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_feature_maps_against_float64(cam):
    """The denoisers' feature maps of the RTAO pass (pixel-centre primaries, one iteration): view-space position = view * hit point,
    view-space normal = transpose(inverse(view)) * surface normal, against float64 -- rows of the rotation, translation and the
    transposed inverse all matter under a rolled camera."""
    w, h = cameras.VIEWPORTS["ragged"]
    c = small_case(width=w, height=h, n_lines=14, pts_per_line=10, line_width=0.05, camera=cam, use_jittered_primary_rays=False,
                   ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
                   ambient_occlusion_samples_per_frame=1)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    with lvo.ao_features(c.width, c.height) as f:
        sc.render_ao(P)
    hit, fp, n, gap = first_hits_float64(c, P)
    # pixels whose closest hit is clear in float64: away from silhouettes (|n . ray| not small), the runner-up well behind, no cap seam
    eye = ir2.ir.camera_position(np.asarray(P.view[:], np.float64))
    ray = fp - eye
    dist = np.linalg.norm(ray, axis=2)
    facing = np.abs((n * ray).sum(axis=2)) / np.maximum(dist, 1e-300)
    clear = hit & (facing > 0.3) & (gap > 1e-3)
    assert clear.sum() > 150
    V = mat(c.view)
    want_pos = fp @ V[:3, :3].T + V[:3, 3]
    want_n = n @ np.linalg.inv(V)[:3, :3]                       # transpose(inverse(view)) * (n, 0): rows of the product = columns of invView
    ep = np.abs(f.position[..., :3] - want_pos).max(axis=2)[clear]
    en = np.abs(f.normal[..., :3] - want_n).max(axis=2)[clear]
    # position: the float32 hit distance carries ~1e-6 relative (closest-approach roots), the transform a few ulps; normal: the hit
    # point's error divided by the radius
    good = (ep <= 1e-5 * np.maximum(dist[clear], 1.0)) & (en <= 1e-5 * np.maximum(dist[clear], 1.0) / (c.line_width * 0.5))
    print("%s: clear pixels %d, position %.2e, normal %.2e" % (cam, clear.sum(), ep.max(), en.max()))
    assert good.mean() > 0.995, (good.mean(), ep.max(), en.max())
    assert (f.position[..., 3][clear] == 1.0).all() and (f.position[..., 2][clear] < 0.0).all()


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_ao_lookup_projects_a_pixel_centre_hit_onto_its_own_texel(cam):
    """getAoFactor's literal lookup projects the view-space hit with the projection matrix and samples the AO image bilinearly.  The
    hit of a pixel-centre ray must land on its own texel centre under every projection (lens shift and non-square pixels included), so
    with an AO image of white noise -- neighbouring texels differ by up to 1 -- the literal lookup gives the frame of the direct read:
    the position error of the float32 hit, ~1e-6 f_px of a pixel, moves a channel by < 0.4 LSB (the bar of test_deviations.py)."""
    w, h = cameras.VIEWPORTS["ragged"]
    c = small_case(width=w, height=h, n_lines=14, pts_per_line=10, line_width=0.05, camera=cam, ambient_occlusion_mode="RTAO (Screen Space)",
                   ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=1)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    ao = np.random.default_rng(3).random((h, w)).astype(np.float32)
    a = sc.render_rt(P, ao=ao)
    with lvo.deviation_switches(reference_ao_lookup=True):
        b = sc.render_rt(P, ao=ao)
    d = np.abs(a.astype(np.int32) - b.astype(np.int32)).max(axis=2)
    covered = (a[..., :3] != 255).any(axis=2)
    assert covered.sum() > 150 and d.max() <= 1 and (d > 0).sum() < 0.01 * covered.sum(), (d.max(), (d > 0).sum(), covered.sum())
    # the noise matters: the neighbouring texel gives another frame
    assert np.abs(a.astype(np.int32) - sc.render_rt(P, ao=np.roll(ao, 1, axis=1)).astype(np.int32)).max() > 20


# ---------------------------------------------------------------- the cull pass's screen bound
def cull_radius_bound(proj, width, height, cw, ndc, radius):
    """k_ppll_cull_segments' bound of the screen distance (pixels) between the projection of a line point with clip.w = cw and ndc
    coordinates ndc and the projection of any point within `radius` of it, restated in float64."""
    tan_off = (abs(ndc[0]) + abs(proj[0, 2])) / abs(proj[0, 0]) + (abs(ndc[1]) + abs(proj[1, 2])) / abs(proj[1, 1])
    return 1.25 * (1.0 + tan_off) * radius * max(abs(proj[0, 0]) * width / 2.0, abs(proj[1, 1]) * height / 2.0) / (cw - radius) + 2.0


def test_the_cull_bound_is_a_bound_under_every_projection_of_the_family():
    """The formula of the sharded PPLL's cull pass against the true screen extent of a sphere of the tube's radius (4000 directions) about
    random line points anywhere in and around the viewport: fovy 10 .. 130 degrees, lens shifts up to a whole ndc unit, non-square
    pixels, radii up to 0.05, from the nearest depth the pass decides at (4 radii) outwards.  Without the shift terms in the tangent
    the bound falls short by up to 8 pixels under a shifted lens (test_gpu_cameras.py::test_cull_bound_with_a_shifted_lens)."""
    from linevis_amd import camera
    rng = np.random.default_rng(1)
    W, H = 320, 256
    dirs = rng.normal(size=(4000, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    least = np.inf
    for trial in range(1500):
        proj = mat(camera.perspective(np.deg2rad(rng.uniform(10.0, 130.0)), W / H * rng.uniform(0.6, 1.7)))
        if trial % 3:
            proj[0, 2], proj[1, 2] = rng.uniform(-1.0, 1.0, 2)
        r = float(rng.choice([0.001, 0.01, 0.025, 0.05]))
        z = rng.uniform(4.0 * r + 1e-5, 1.5)
        ndc = rng.uniform(-1.3, 1.3, 2)
        centre = np.array([(ndc[0] + proj[0, 2]) * z / proj[0, 0], (ndc[1] + proj[1, 2]) * z / proj[1, 1], -z])
        cl = np.concatenate([centre + r * dirs, np.ones((len(dirs), 1))], 1) @ proj.T
        px, py = (cl[:, 0] / cl[:, 3] + 1.0) * W / 2.0, (cl[:, 1] / cl[:, 3] + 1.0) * H / 2.0
        dev = max(np.abs(px - (ndc[0] + 1.0) * W / 2.0).max(), np.abs(py - (ndc[1] + 1.0) * H / 2.0).max())
        least = min(least, cull_radius_bound(proj, W, H, z, ndc, r) - dev)
    assert least > 0.0, least
