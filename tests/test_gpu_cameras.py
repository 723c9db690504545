"""Every rendering mode under general view and projection matrices, HIP against the oracle.

lv_set_camera takes two arbitrary 4 x 4 matrices; the rest of the GPU suite only ever passes camera.default_camera with a moving eye
(up = (0, 1, 0), one field of view, near / far = 0.01 / 100, symmetric projection, square pixels, target = origin), under which
several entries of the view matrix and most of the projection are structurally zero or constant.  The camera family of
tests/cameras.py leaves that slice (roll, target, fovy 15 .. 120 degrees, near / far cutting the data set, the eye inside the data
set, lens shift, non-square pixels); the contract is the suite's own: AO factors, depth range, PPLL fragment multisets and depths bit
for bit, frames <= 2 LSB, EAW / SVGF AO within their bars, MLAB frames = mlab_fold of the oracle's fragments with 0 LSB, and every
tile rectangle and tile list reproduces the whole frame byte for byte -- the last under cameras, tube widths and tile lists chosen so
that the conservative screen bound of the sharded PPLL's cull pass (k_ppll_cull_segments) decides something."""
import os

import numpy as np
import pytest

import cameras
from common import Case, max_lsb_diff, small_case
from linevis_amd import capi, scenes, tiling, transfer_function as tfm
from oracle import lvo
from test_gpu_fuzz import random_case
from test_gpu_mlab import frame_reference
from test_prism_raster import _lists, _walk_order

pytestmark = pytest.mark.gpu

LSB_TOL = 2
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_gamma=1.0,
            ambient_occlusion_radius=0.1)
# small-case viewports, dealt to the cameras in turn: wide, tall, and sides that are multiples neither of 8 nor of the PPLL tile
SMALL_VIEWPORTS = [(112, 80), (70, 128), (93, 61)]
# sharding viewports: several coarse cells (LV_PRISM_COARSE = 32 pixels) per side; the second is tall with ragged last cells
SHARD_VIEWPORTS = [(320, 256), (210, 300)]
COARSE = 32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def viewport_of(cam, table=SMALL_VIEWPORTS):
    return table[cameras.NAMES.index(cam) % len(table)]


def covered_pixels(img, c):
    bg = np.floor(np.clip(np.asarray(c.background[:3]), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return int((img[..., :3] != bg).any(axis=2).sum())


def cam_case(cam, width=None, height=None, **kw):
    w, h = viewport_of(cam)
    return small_case(width=width or w, height=height or h, camera=cam, **kw)


def check_inside(cam, c):
    """the inside cameras see segments with one end behind the camera plane"""
    if cam in cameras.INSIDE:
        assert cameras.segments_straddling_the_camera_plane(c) > 0


# ---------------------------------------------------------------- mode 11
@pytest.mark.parametrize("cam", cameras.NAMES)
def test_ray_tracer_with_rtao_and_depth_cues(hip_lib, cam):
    """Opaque tubes, jittered colour rays (num_samples_per_frame > 1: the AO lookup projects the hit point with view / proj and
    samples bilinearly), jittered RTAO primaries, depth cues: lv_compute_depth_range and the AO factors bit for bit, the frame and a
    ragged rectangle of it."""
    c = cam_case(cam, seed=31, num_samples_per_frame=2, depth_cue_strength=0.8, **RTAO, ambient_occlusion_iterations=2,
                 ambient_occlusion_samples_per_frame=4)
    check_inside(cam, c)
    ctx = c.hip_context()
    img = ctx.render(11)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    assert np.array_equal(bits(ctx.depth_range()), bits(sc.depth_range(P)))
    assert 0.0 < P.minDepth < P.maxDepth <= c.far + 0.02
    ref, ao_ref = c.oracle_render(11)
    assert np.array_equal(bits(ctx.get_ao()), bits(ao_ref))
    assert (ao_ref < 1.0).sum() > 50
    assert max_lsb_diff(img, ref) <= LSB_TOL
    assert covered_pixels(ref, c) > 200
    x0, y0, w, h = c.width // 3, c.height // 4, c.width // 2 + 1, c.height // 2 + 3
    assert np.array_equal(ctx.render(11, tile=(x0, y0, w, h)), img[y0:y0 + h, x0:x0 + w])
    ctx.close()


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_ray_tracer_variants(hip_lib, cam):
    """Transparent tubes without halos and caps; RTAO with pixel-centre primaries; the reference's RTAO geometry (triangle tubes);
    the Triangle Mesh geometry mode; multi-layer alpha tracing by replay (test_gpu_mlat.py)."""
    lw = 0.02
    # transparent, halos and caps off, RTAO from pixel-centre primaries
    c = cam_case(cam, seed=11, line_width=lw, transparent=True, use_halos=False, use_capped_tubes=False, use_jittered_primary_rays=False,
                 **RTAO, ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=5)
    ctx = c.hip_context()
    img = ctx.render(11)
    ref, ao_ref = c.oracle_render(11)
    assert np.array_equal(bits(ctx.get_ao()), bits(ao_ref))
    assert max_lsb_diff(img, ref) <= LSB_TOL and covered_pixels(ref, c) > 200
    ctx.close()
    # halos on, opaque, no AO: the outline width depends on fov_y and the viewport height
    c = cam_case(cam, seed=11, line_width=lw)
    ctx = c.hip_context()
    img = ctx.render(11)
    assert max_lsb_diff(img, c.oracle_render(11)[0]) <= LSB_TOL and covered_pixels(img, c) > 200
    ctx.close()
    # rtao_geometry = triangle_tubes, then geometry_mode = Triangle Mesh on the same mesh
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=11))
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
    ts = lvo.TriScene(*mesh, lw)
    c = cam_case(cam, seed=11, line_width=lw, rtao_geometry="triangle_tubes", **RTAO, ambient_occlusion_iterations=2,
                 ambient_occlusion_samples_per_frame=4)
    ctx = c.hip_context()
    ctx.set_tube_triangle_mesh(*mesh)
    img = ctx.render(11)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    ao_ref = ts.render_ao(P, use_bvh=True)
    assert np.array_equal(bits(ctx.get_ao()), bits(ao_ref)) and (ao_ref < 1.0).sum() > 50
    assert max_lsb_diff(img, sc.render_rt(P, ao=ao_ref, use_bvh=True)) <= LSB_TOL
    ctx.close()
    c = cam_case(cam, seed=11, line_width=lw, transparent=True, geometry_mode="Triangle Mesh", num_samples_per_frame=3, depth_cue_strength=0.7)
    ctx = c.hip_context()
    ctx.set_tube_triangle_mesh(*mesh)
    img = ctx.render(11)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    ref = ts.render_rt(sc, P, use_bvh=True)
    assert max_lsb_diff(img, ref) <= LSB_TOL and covered_pixels(ref, c) > 200
    ctx.close()
    # MLAT: the oracle replays the candidate order the kernel recorded
    c = cam_case(cam, seed=11, line_width=lw, transparent=True, n_lines=50, mlat_num_nodes=4, use_mlat=True, collect_stats=True,
                 mlat_record_trace=True)
    ctx = c.hip_context()
    img = ctx.render(11)
    rec = ctx.mlat_trace()
    sc = c.oracle_scene()
    ref, _, viol = sc.render_rt_mlat(c.oracle_params(sc), 4, trace=rec)
    assert viol == 0 and max_lsb_diff(img, ref) <= LSB_TOL and len(rec) > 500
    ctx.close()


@pytest.mark.parametrize("cam", ["roll37", "lens_shift", "inside_rolled"])
def test_band_data_and_elliptic_tubes(hip_lib, cam):
    """Band data: the sphere-traced elliptic tubes (their shading takes the camera position) with RTAO, frame and AO against the oracle."""
    from test_gpu_elliptic import band_case, RTAO as RTAO_BANDS
    w, h = viewport_of(cam)
    c = cameras.apply_camera(band_case(width=w, height=h, **dict(RTAO_BANDS, use_jittered_primary_rays=True)), cam)
    ctx = c.hip_context()
    img = ctx.render(11)
    ref, ao_ref = c.oracle_render(11)
    assert np.array_equal(bits(ctx.get_ao()), bits(ao_ref))
    assert max_lsb_diff(img, ref) <= LSB_TOL and covered_pixels(ref, c) > 200
    ctx.close()


# ---------------------------------------------------------------- mode 2
def ppll_lists_against_the_oracle(c, ctx, min_fragments):
    """fragment lists of the last mode-2 frame against ppll_gather, in walk order (nearest first), bit for bit"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    assert P.ppllFragmentSource == 1
    pw, ph = c.padded()
    hn, hs, hcnt = ctx.ppll_buffers(pw * ph, int(P.ppllLinkedListSize))
    on, os_, ocnt = sc.ppll_gather(P, use_bvh=True)
    assert hcnt == ocnt and hcnt > min_fragments, (hcnt, ocnt)
    assert _lists(hn, hs) == _lists(on, os_)
    walk = _walk_order(hn, hs)
    assert all(l == sorted(l) for l in walk.values())
    return sc, P, walk, hcnt


@pytest.mark.parametrize("cam", cameras.NAMES)
def test_ppll_fragment_lists(hip_lib, cam):
    """Mode 2 on the rasterised prism: the per-pixel fragment multisets (packed colour, depth bits) against ppll_gather, the frame,
    the all-hits walk front end (ppll_prism_rasteriser = lbvh) against the segment rasteriser, a ragged rectangle."""
    c = cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
    check_inside(cam, c)
    ctx = c.hip_context()
    img = ctx.render(2)
    sc, P, walk, n = ppll_lists_against_the_oracle(c, ctx, 500)
    assert max_lsb_diff(img, sc.render_ppll(P, use_bvh=True)) <= LSB_TOL
    if cam == "tight_clip":
        # near / far cut the data set: fragments were clipped away (the same scene under the default planes has more) ...
        wide = cam_case("default", *viewport_of(cam), seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
        scw = wide.oracle_scene()
        assert scw.ppll_gather(wide.oracle_params(scw), use_bvh=True)[2] > n + 100
        # ... and every depth that was kept lies between the planes: depth = distance from the eye, -z_view <= depth <= -z_view / cos
        # of the off-axis angle, at most that of the viewport's corner
        d = np.array([db for l in walk.values() for db, _ in l], dtype=np.uint32).view(np.float32)
        t = np.tan(c.fovy / 2.0)
        assert d.min() >= c.near and d.max() <= c.far * np.sqrt(1.0 + t * t * (1.0 + (c.width / c.height) ** 2))
    ctx.set_option("ppll_prism_rasteriser", "lbvh")
    img2 = ctx.render(2)
    pw, ph = c.padded()
    hn2, hs2, cnt2 = ctx.ppll_buffers(pw * ph, int(P.ppllLinkedListSize))
    assert cnt2 == n and _walk_order(hn2, hs2) == walk and np.array_equal(img2, img)
    ctx.set_option("ppll_prism_rasteriser", "segments")
    x0, y0, w, h = c.width // 3, c.height // 4, c.width // 2 + 1, c.height // 2 + 3
    assert np.array_equal(ctx.render(2, tile=(x0, y0, w, h)), img[y0:y0 + h, x0:x0 + w])
    ctx.close()


@pytest.mark.parametrize("cam", ["wide_close", "away_rolled"])
@pytest.mark.parametrize("kind", ["band_data", "helicity_bands"])
def test_ppll_of_band_data_and_helicity_bands(hip_lib, cam, kind):
    if kind == "band_data":
        from test_gpu_elliptic import band_case
        c = band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8)
    else:
        from test_gpu_helicity_bands import helicity_case
        c, _, _ = helicity_case(width=120, height=90, transparent=True)
    cameras.apply_camera(c, cam)
    ctx = c.hip_context()
    img = ctx.render(2)
    sc, P, _, _ = ppll_lists_against_the_oracle(c, ctx, 200)
    assert max_lsb_diff(img, sc.render_ppll(P, use_bvh=True)) <= LSB_TOL
    ctx.close()


# ---------------------------------------------------------------- mode 3
@pytest.mark.parametrize("cam", cameras.NAMES)
def test_mlab_frame_is_the_fold_of_the_oracle_fragments(hip_lib, cam):
    """The window depth MLAB sorts by is clip.z / clip.w of proj * view: K = 8 against mlab_fold, 0 LSB (K = 1 too on four cameras:
    the reference of a frame costs more wall time than everything the GPU does here)."""
    c = cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
    ctx = c.hip_context()
    for K in ((1, 8) if cam in ("default", "inside_rolled", "lens_shift", "wide_close") else (8,)):
        ctx.set_option("mlab_num_layers", K)
        img = ctx.render(3)
        ref, n = frame_reference(c, K)
        assert n > 500
        assert np.array_equal(img, ref), (K, max_lsb_diff(img, ref))
        assert int(ctx.stats().fragments) == n
    ctx.close()


# ---------------------------------------------------------------- sharding
def render_tile_list(ctx, mode, tiles, t):
    import torch
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1, 2)
    out = torch.zeros((len(tiles), t, t, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(out.data_ptr(), tiles, t, t, mode=mode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def single_tiles(width, height):
    """One coarse cell each (none of its neighbours requested): the four image corners and the middle, plus a 16 x 16 tile inside the
    corner cells -- where the off-axis growth of the projected radius is largest."""
    cx, cy = (width - 1) // COARSE * COARSE, (height - 1) // COARSE * COARSE
    mx, my = (width // 2) // COARSE * COARSE, (height // 2) // COARSE * COARSE
    cells = [(0, 0), (cx, 0), (0, cy), (cx, cy), (mx, my)]
    small = [(8, 8), (min(cx + 8, width - 16), 8), (8, min(cy + 8, height - 16)), (min(cx + 8, width - 16), min(cy + 8, height - 16))]
    return [(x, y, COARSE) for x, y in cells] + [(x, y, 16) for x, y in small]


SHARD_SETTINGS = {
    2: dict(),
    3: dict(),
    11: dict(RTAO, ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=4, num_samples_per_frame=2,
             ambient_occlusion_denoiser="EAW", eaw_denoiser_iterations=2),
}


@pytest.mark.parametrize("cam", cameras.NAMES)
@pytest.mark.parametrize("mode", [2, 3, 11])
def test_tile_lists_reproduce_the_whole_frame(hip_lib, cam, mode):
    """A rank of a sharded frame renders a tile list; in modes 2 and 3 a cull pass over the segments (coarse cells of 32 pixels, a
    conservative screen bound per segment) and stage A of the rasteriser decide which segments and pixels are looked at.  A bound that
    is too tight under some camera drops fragments near tile borders, and only this comparison sees it: Morton tile lists dealt to 2
    and 8 ranks, single cells at the image corners and in the middle, 16-pixel tiles inside the corner cells and a random rectangle,
    each byte for byte the whole frame's pixels -- fat tubes (line_width 0.05) and thin ones."""
    import torch  # noqa: F401
    W, H = viewport_of(cam, SHARD_VIEWPORTS)
    rng = np.random.default_rng(cameras.NAMES.index(cam) * 10 + mode)
    compared = 0
    for lw in (0.05, 0.004):
        c = cam_case(cam, width=W, height=H, seed=5, n_lines=40, pts_per_line=40, line_width=lw, transparent=mode != 11, **SHARD_SETTINGS[mode])
        ctx = c.hip_context()
        whole = ctx.render(mode)
        assert covered_pixels(whole, c) > 1000
        if mode == 2 or (mode == 11 and lw == 0.05):
            ref, ao_ref = c.oracle_render(mode, use_bvh=True)
            if ao_ref is not None:
                assert np.abs(ctx.get_ao() - ao_ref).max() < 2e-5
            assert max_lsb_diff(whole, ref) <= LSB_TOL
        tiles = tiling.make_tiles(W, H, COARSE)
        assert len(tiles) >= 48
        for world in (2, 8):
            pieces = np.zeros((len(tiles), COARSE, COARSE, 4), dtype=np.uint8)
            for r in range(world):
                pieces[r::world] = render_tile_list(ctx, mode, tiling.assign_tiles(tiles, r, world), COARSE)
            assert np.array_equal(tiling.detile(pieces, tiles, W, H, COARSE), whole), (lw, world)
        for x, y, t in single_tiles(W, H):
            got = render_tile_list(ctx, mode, [(x, y)], t)[0]
            hh, ww = min(t, H - y), min(t, W - x)
            assert np.array_equal(got[:hh, :ww], whole[y:y + hh, x:x + ww]), (lw, x, y, t)
            compared += covered_pixels(whole[y:y + hh, x:x + ww], c)
        x0, y0 = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8))
        w, h = int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))
        assert np.array_equal(ctx.render(mode, tile=(x0, y0, w, h)), whole[y0:y0 + h, x0:x0 + w]), (lw, x0, y0, w, h)
        assert np.array_equal(ctx.render(mode), whole)
        ctx.close()
    assert compared > 100       # the single tiles were not all empty


def shifted_lens_line(px, py=120.0, z=0.3, line_width=0.1, width=320, height=256):
    """A short fat vertical line at view-space depth z whose middle projects to pixel (px, py), seen with fovy 124 degrees through a
    lens shifted by (0.88, 0.1): the viewport's middle is 64 degrees off the optical axis, so the tube's screen footprint is
    stretched away from the axis by ~1 / cos^2 of that angle although its ndc coordinates are small."""
    cam = dict(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), fovy=float(np.float32(np.deg2rad(124.0))), shift=(0.88, 0.1))
    _, proj, _, _, _ = cameras.matrices(cam, width, height)
    xv = (px / (width / 2.0) - 1.0 + float(proj[8])) * z / float(proj[0])
    yv = (py / (height / 2.0) - 1.0 + float(proj[9])) * z / float(proj[5])
    pos = np.array([(xv, yv + 0.01 * k, -z) for k in (-1, 0, 1)], np.float32)
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, np.array([0.0, 0.5, 1.0], np.float32), np.array([0, 3], np.uint32), line_width)
    return cameras.apply_camera(Case(pts, seg, tfm.standard_transparent(), width, height, line_width), cam)


@pytest.mark.parametrize("mode", [2, 3])
def test_cull_bound_with_a_shifted_lens(hip_lib, mode):
    """The cull pass bounds a segment's screen footprint by its projected radius times (1 + tangent of the off-axis angle).  Under a
    lens shift the tangent is (|ndc| + |shift|) / proj[0], not |ndc| / proj[0]: taken from the ndc coordinates alone the bound of
    these lines ends 1 to 8 pixels left of the coarse-cell border at x = 192 while their fragments reach 1 to 8 pixels beyond it
    (float64 restatement of the bound against the oracle's fragments), and a rank that is asked for the cell right of the border
    alone dropped them."""
    lost = 0
    for px in (162.0, 164.0, 166.0, 168.0):
        c = shifted_lens_line(px)
        ctx = c.hip_context()
        whole = ctx.render(mode)
        if mode == 2:
            assert max_lsb_diff(whole, c.oracle_render(2, use_bvh=True)[0]) <= LSB_TOL
        want = whole[96:128, 192:224]
        assert covered_pixels(want, c) >= 5, px                 # the line reaches into the requested cell
        assert covered_pixels(whole[96:128, 160:192], c) > 50   # ... from the cell left of it
        got = render_tile_list(ctx, mode, [(192, 96)], COARSE)[0]
        lost += int((got != want).any(axis=2).sum())
        ctx.close()
    assert lost == 0


# ---------------------------------------------------------------- SVGF
def svgf_camera_path():
    """rolls, moves the target and changes fovy between frames (two frames stand still)"""
    path = []
    for k, (roll, tx, fov, ex) in enumerate([(0.0, 0.0, 53.0, 0.0), (0.0, 0.0, 53.0, 0.0), (2.0, 0.01, 53.0, 0.01), (4.0, 0.02, 50.0, 0.02),
                                             (6.0, 0.02, 47.0, 0.02), (6.0, 0.02, 47.0, 0.02)]):
        a = np.deg2rad(roll)
        path.append(dict(eye=(ex, 0.005 * k, 0.8), target=(tx, -tx, 0.0), up=(float(-np.sin(a)), float(np.cos(a)), 0.0),
                         fovy=float(np.float32(np.deg2rad(fov)))))
    return path


@pytest.mark.parametrize("jitter", [False, True])
def test_svgf_sequence_under_a_rolling_zooming_camera(hip_lib, jitter):
    """SVGF reprojects with the previous frame's matrices: a path that rolls, pans and zooms, against the oracle's sequence (the bars
    of test_svgf.py)."""
    from test_svgf import fat_case
    c = fat_case(jitter=jitter)
    ctx = c.hip_context()
    sc = c.oracle_scene()
    sv = lvo.Svgf(c.width, c.height)
    for f, cam in enumerate(svgf_camera_path()):
        cameras.apply_camera(c, cam)
        ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
        img = ctx.render(11)
        ao = ctx.get_ao()
        P = c.oracle_params(sc)
        ao_ref = sv.step(lambda: sc.render_ao(P), P)
        assert np.abs(ao - ao_ref).max() < 3e-5, "frame %d" % f
        assert max_lsb_diff(img, sc.render_rt(P, ao=ao_ref)) <= LSB_TOL, "frame %d" % f
    assert np.abs(ao_ref - 1.0).max() > 0.2
    assert np.abs(sv.flow).max() > 0.5          # the camera moved: the reprojection had motion vectors to follow
    ctx.close()


# ---------------------------------------------------------------- fuzzer
SEED_OFFSET = 100000 * int(os.environ.get("LV_FUZZ_SEED_OFFSET", "0"))
MAX_REDRAWS = 20


def random_camera(rng):
    """eye, target, up, fovy in [10, 130] degrees, near / far and the viewport; the eye may lie inside the data set"""
    d = rng.normal(size=3)
    eye = d / np.linalg.norm(d) * rng.uniform(0.05, 1.6)
    target = rng.uniform(-0.3, 0.3, 3)
    while True:
        up = rng.normal(size=3)
        up /= np.linalg.norm(up)
        f = (target - eye) / np.linalg.norm(target - eye)
        if np.linalg.norm(np.cross(f, up)) > 0.3:
            break
    near = float(10.0 ** rng.uniform(-3.0, -1.0))
    far = float(10.0 ** rng.uniform(0.5, 3.0))
    cam = dict(eye=tuple(eye), target=tuple(target), up=tuple(up), fovy=float(np.float32(np.deg2rad(rng.uniform(10.0, 130.0)))),
               near=near, far=far)
    if rng.uniform() < 0.3:
        cam["shift"] = (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.4, 0.4)))
    if rng.uniform() < 0.3:
        cam["pixel_aspect"] = float(rng.uniform(0.6, 1.7))
    return cam, int(rng.integers(17, 330)), int(rng.integers(9, 260))


@pytest.mark.parametrize("seed", range(4))
def test_random_camera_cases(hip_lib, seed):
    """random_case's scenes and settings (its own draws untouched: the camera comes from a generator of its own) under drawn cameras
    and viewports.  A drawn camera is redrawn only if it sees fewer than 50 pixels of the data set, at most 20 times per case."""
    rng = np.random.default_rng(5000 + seed + SEED_OFFSET)
    crng = np.random.default_rng(6000 + seed + SEED_OFFSET)
    for k in range(8):
        c, _ = random_case(rng)
        for attempt in range(MAX_REDRAWS + 1):
            assert attempt < MAX_REDRAWS, "seed %d case %d: no camera with 50 covered pixels in %d draws" % (seed, k, MAX_REDRAWS)
            cam, c.width, c.height = random_camera(crng)
            cameras.apply_camera(c, cam)
            with lvo.deviation_switches(literal_intersection=c.literal_form()):
                ref, ao_ref = c.oracle_render(11, use_bvh=True)
            if covered_pixels(ref, c) >= 50:
                break
        tag = "seed %d case %d: %dx%d lw %g %s %s" % (seed, k, c.width, c.height, c.line_width, cam, c.settings)
        ctx = c.hip_context()
        img = ctx.render(11)
        if ao_ref is not None:
            ao = ctx.get_ao()
            if c.eaw_settings():
                assert np.abs(ao - ao_ref).max() < 2e-5, tag
            else:
                assert np.array_equal(bits(ao), bits(ao_ref)), tag
        assert max_lsb_diff(img, ref) <= LSB_TOL, tag
        x0, y0 = int(crng.integers(0, c.width)), int(crng.integers(0, c.height))
        w, h = int(crng.integers(1, c.width - x0 + 1)), int(crng.integers(1, c.height - y0 + 1))
        assert np.array_equal(ctx.render(11, tile=(x0, y0, w, h)), img[y0:y0 + h, x0:x0 + w]), tag
        ctx.close()
        # modes 2 and 3 of the same scene and camera (transparent transfer function, the settings the PPLL fuzzer keeps)
        s = {key: v for key, v in c.settings.items() if key not in ("num_samples_per_frame", "intersection_form",
                                                                     "ambient_occlusion_denoiser", "max_depth_complexity")}
        c2 = Case(c.points, c.seg, tfm.standard_transparent(), c.width, c.height, c.line_width, background=c.background, **s)
        c2.view, c2.proj, c2.fovy, c2.near, c2.far = c.view, c.proj, c.fovy, c.near, c.far
        ctx = c2.hip_context()
        whole = ctx.render(2)
        ref2, _ = c2.oracle_render(2, use_bvh=True)
        assert max_lsb_diff(whole, ref2) <= LSB_TOL, tag
        t = int(crng.choice([16, 32]))
        tiles = tiling.make_tiles(c.width, c.height, t)
        pick = tiles[crng.permutation(len(tiles))[:max(1, len(tiles) // 5)]]
        for mode in (2, 3):
            whole = ctx.render(mode)
            got = render_tile_list(ctx, mode, pick, t)
            for i, (x, y) in enumerate(pick):
                hh, ww = min(t, c.height - int(y)), min(t, c.width - int(x))
                assert np.array_equal(got[i][:hh, :ww], whole[y:y + hh, x:x + ww]), (tag, mode, int(x), int(y), t)
        ctx.close()


# ---------------------------------------------------------------- lv_set_camera says what it accepts
def _bad_cameras():
    view, proj, fovy, near, far = cameras.matrices(cameras.get("roll37"), 96, 64)
    out = {}
    for name, m in (("view", view), ("proj", proj)):
        for bad in (np.nan, np.inf, -np.inf):
            v, p = view.copy(), proj.copy()
            (v if name == "view" else p)[5] = bad
            out["%s_%s" % (name, bad)] = (v, p, fovy, near, far)
    v = view.copy(); v[0:4] = 0.0                       # a zero column: det = 0
    out["view_singular"] = (v, proj, fovy, near, far)
    v = view.copy(); v[4:8] = v[0:4]                    # two equal columns
    out["view_rank_3"] = (v, proj, fovy, near, far)
    p = proj.copy(); p[11] = 0.0                        # no perspective divide and proj[15] = 0: singular
    out["proj_singular"] = (view, p, fovy, near, far)
    p = proj.copy(); p[11] = 0.0; p[15] = 1.0; p[10] = -0.01; p[14] = 0.0   # orthographic: ray origins are the camera position
    out["proj_orthographic"] = (view, p, fovy, near, far)
    out["near_zero"] = (view, proj, fovy, 0.0, far)
    out["near_negative"] = (view, proj, fovy, -0.01, far)
    out["far_equals_near"] = (view, proj, fovy, 0.5, 0.5)
    out["far_below_near"] = (view, proj, fovy, 0.5, 0.1)
    out["near_nan"] = (view, proj, fovy, float("nan"), far)
    out["far_inf"] = (view, proj, fovy, near, float("inf"))
    out["fovy_zero"] = (view, proj, 0.0, near, far)
    out["fovy_nan"] = (view, proj, float("nan"), near, far)
    return out


@pytest.mark.parametrize("multi", [False, True])
def test_set_camera_rejects_what_the_kernels_do_not_cover(hip_lib, multi):
    """Non-finite entries, singular matrices, an orthographic projection, near <= 0, far <= near: LV_E_INVALID, and the previous camera
    stays in force (the frame after the rejected calls is the frame before them).  Only the error is read: nothing is rendered from a
    rejected matrix.  A multi-device handle gives the same answer."""
    c = small_case(width=96, height=64, camera="roll37")
    ctx = capi.Context(devices=[0, 0], transport="memcpy") if multi else capi.Context(0)
    ctx.set_lines(c.points, c.seg)
    ctx.set_transfer_function(c.tf, 0.0, 1.0)
    ctx.set_option("line_width", c.line_width)
    for name, args in _bad_cameras().items():          # rejected before any camera was set: the context still has none
        with pytest.raises(capi.LineVisError) as e:
            ctx.set_camera(*args, 96, 64)
        assert e.value.code == -1, name
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(11, tile=(0, 0, 96, 64))
    assert e.value.code != 0                            # "lv_set_camera has not been called"
    ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, 96, 64)
    before = ctx.render(11)
    for name, args in _bad_cameras().items():
        with pytest.raises(capi.LineVisError) as e:
            ctx.set_camera(*args, 128, 32)              # the viewport of a rejected call is not taken either
        assert e.value.code == -1, name
    ctx.width, ctx.height = 96, 64
    assert np.array_equal(ctx.render(11), before)
    assert max_lsb_diff(before, c.oracle_render(11)[0]) <= LSB_TOL
    # every camera of the family is accepted
    for name in cameras.NAMES:
        ctx.set_camera(*cameras.matrices(cameras.get(name), 96, 64), 96, 64)
    ctx.close()
