"""SVGF denoiser of the RTAO pass (ambient_occlusion_denoiser = "SVGF"): the oracle's restatement of
Data/Shaders/Denoiser/SVGF.glsl + Scattering/Denoiser/SVGF.cpp, and the HIP kernels (linevis_amd/csrc/lv_svgf.hip) against it
over frame sequences -- SVGF is temporal, so parity means the same images after every frame of the same camera path."""
import numpy as np
import pytest

import cameras
from common import Case, small_case, max_lsb_diff
from linevis_amd import camera
from oracle import lvo

RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_gamma=1.0,
            ambient_occlusion_radius=0.3, ambient_occlusion_distance_based=True, ambient_occlusion_iterations=1,
            ambient_occlusion_samples_per_frame=2, ambient_occlusion_denoiser="SVGF")


def fat_case(jitter=False, **kw):
    s = dict(RTAO, use_jittered_primary_rays=jitter)
    s.update(kw)
    return small_case(width=160, height=120, n_lines=6, pts_per_line=30, line_width=0.25, **s)


def test_constant_image_is_a_fixed_point():
    """A noise-free AO image passes through unchanged (weights normalise to 1), its variance stays 0 and the history length
    counts the frames up to the cap of 32."""
    w, h = 48, 40
    n = np.zeros((h, w, 4), np.float32)
    n[..., 2] = 1.0
    depth = np.full((h, w), 0.7, np.float32)
    fwidth = np.zeros((h, w), np.float32)
    flow = np.zeros((h, w, 2), np.float32)
    noisy = np.full((h, w), 0.625, np.float32)
    hist = [np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)]
    out = np.zeros((h, w), np.float32)
    for f in range(40):
        lvo.lib().lvo_svgf_denoise(w, h, lvo._p(noisy), lvo._p(n), lvo._p(depth), lvo._p(fwidth), lvo._p(flow), 5, 0.002, 0.02,
                                   lvo._p(hist[0]), lvo._p(hist[1]), lvo._p(hist[2]), lvo._p(hist[3]), lvo._p(out))
        assert np.abs(out - 0.625).max() < 1e-6
        # the reprojection accepts coordinates 1 .. size - 1 only (is_reprj_valid): column / row 0 never build a history
        assert np.all(hist[1][1:-1, 1:-1, 2] == min(f + 1, 32))
    assert np.array_equal(hist[2], n) and np.array_equal(hist[3], depth)


def test_denoising_a_static_view_reduces_the_error():
    c = fat_case()
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.aoIterations = 128
    ref = sc.render_ao(P)
    P.aoIterations = 1
    sv = lvo.Svgf(c.width, c.height)
    for f in range(6):
        d = sv.step(lambda: sc.render_ao(P), P)
    hit = sv.depth < 50.0
    raw_rmse = np.sqrt(((sv.raw - ref)[hit] ** 2).mean())
    den_rmse = np.sqrt(((d - ref)[hit] ** 2).mean())
    print("rmse raw %.4f denoised %.4f" % (raw_rmse, den_rmse))
    assert den_rmse < 0.25 * raw_rmse
    assert sv.global_frame_number == 6 and np.abs(sv.flow).max() < 1e-3    # static camera, pixel-centre rays: no motion


def test_rtao_seeds_follow_the_global_frame_number_without_accumulation():
    """Under SVGF frame k of the RTAO pass is iteration k's raw sample set, not a running mean."""
    c = fat_case(jitter=True)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    sv = lvo.Svgf(c.width, c.height)
    raws = []
    for f in range(3):
        sv.step(lambda: sc.render_ao(P), P)
        raws.append(sv.raw.copy())
    P.aoIterations = 3
    acc = sc.render_ao(P)       # running mean of the same three sample sets
    assert np.abs(acc - (raws[0] + raws[1] + raws[2]) / 3.0).max() < 1e-6
    assert not np.array_equal(raws[0], raws[1])


def camera_path():
    return [(0.0, 0.0, 0.8), (0.0, 0.0, 0.8), (0.01, 0.0, 0.8), (0.02, 0.005, 0.79), (0.02, 0.005, 0.79), (0.02, 0.005, 0.79)]


def run_sequence(c, poses, tile=None, iterations_per_frame=1):
    """HIP frames + AO images and the oracle's for the same camera path."""
    ctx = c.hip_context()
    sc = c.oracle_scene()
    sv = lvo.Svgf(c.width, c.height, iterations=int(c.settings.get("svgf_denoiser_iterations", 5)))
    out = []
    for pos in poses:
        c.view, c.proj, c.fovy, c.near, c.far = camera.default_camera(c.width, c.height, pos)
        ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
        img = ctx.render(11, tile=tile) if tile else ctx.render(11)
        ao = ctx.get_ao()
        P = c.oracle_params(sc)
        for _ in range(iterations_per_frame):
            ao_ref = sv.step(lambda: sc.render_ao(P), P)
        ref = sc.render_rt(P, ao=ao_ref, tile=tile)
        out.append((img, ao, ref, ao_ref))
    ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jitter,its", [(False, 5), (True, 5), (True, 2), (False, 0)])
def test_svgf_sequence_matches_the_oracle(hip_lib, jitter, its):
    c = fat_case(jitter=jitter, svgf_denoiser_iterations=its)
    for f, (img, ao, ref, ao_ref) in enumerate(run_sequence(c, camera_path())):
        # exp() differs by an ulp or two between the device and glibc; everything discrete (reprojection validity, history
        # length) comes from bit-identical feature maps
        assert np.abs(ao - ao_ref).max() < 3e-5, "frame %d" % f
        assert max_lsb_diff(img, ref) <= 2, "frame %d" % f
    assert np.abs(ao_ref - 1.0).max() > 0.2


@pytest.mark.gpu
def test_svgf_thin_lines_multiple_iterations_per_frame(hip_lib):
    c = small_case(width=200, height=150, n_lines=40, pts_per_line=40, line_width=0.01, **dict(RTAO, ambient_occlusion_iterations=3))
    for f, (img, ao, ref, ao_ref) in enumerate(run_sequence(c, camera_path()[:4], iterations_per_frame=3)):
        assert np.abs(ao - ao_ref).max() < 3e-5, "frame %d" % f
        assert max_lsb_diff(img, ref) <= 2, "frame %d" % f


@pytest.mark.gpu
def test_svgf_tiles_share_the_full_frame_history(hip_lib):
    """The denoiser always runs on the whole viewport: a context that only ever renders one tile produces the crop of the full
    frames of a context that renders everything."""
    c = fat_case(jitter=True)
    tile = (37, 21, 64, 48)
    full = run_sequence(c, camera_path()[:4])
    part = run_sequence(c, camera_path()[:4], tile=tile)
    x0, y0, w, h = tile
    for (img, ao, _, _), (timg, tao, tref, _) in zip(full, part):
        assert np.array_equal(timg, img[y0:y0 + h, x0:x0 + w])
        assert np.array_equal(tao, ao)
        assert max_lsb_diff(timg, tref) <= 2


@pytest.mark.gpu
def test_switching_the_denoiser_clears_the_history(hip_lib):
    c = fat_case()
    ctx = c.hip_context()
    a0 = (ctx.render(11), ctx.get_ao())[1]
    a1 = (ctx.render(11), ctx.get_ao())[1]
    ctx.set_option("ambient_occlusion_denoiser", "None")
    ctx.render(11)
    ctx.set_option("ambient_occlusion_denoiser", "SVGF")
    ctx.set_lines(c.points, c.seg)          # setLineData: global frame counter back to 0
    b0 = (ctx.render(11), ctx.get_ao())[1]
    b1 = (ctx.render(11), ctx.get_ao())[1]
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and not np.array_equal(a0, a1)
    ctx.close()


@pytest.mark.gpu
def test_svgf_full_size_sequence(hip_lib):
    """The config-3 scene (1 M segments) at 1920 x 1080 through RTAO (8 spp per frame) + SVGF over a short camera path: every pixel
    of the denoised AO image and of the frame, after every frame, against the oracle (its own BVH for the RTAO pass)."""
    from linevis_amd import host_api, scenes, transfer_function as tfm
    tr = scenes.normalize(scenes.tornado())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    pts, seg, _ = flow.tube_aabb_render_data(0.002)
    c = Case(pts, seg, tfm.standard(), 1920, 1080, 0.002, **dict(RTAO, ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=8,
                                                                 ambient_occlusion_radius=0.1))
    ctx = c.hip_context()
    sc = c.oracle_scene()
    sv = lvo.Svgf(c.width, c.height)
    for f, pos in enumerate(camera_path()[1:4]):
        c.view, c.proj, c.fovy, c.near, c.far = camera.default_camera(c.width, c.height, pos)
        ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
        img = ctx.render(11)
        ao = ctx.get_ao()
        P = c.oracle_params(sc)
        ao_ref = sv.step(lambda: sc.render_ao(P, use_bvh=True), P)
        assert np.abs(ao - ao_ref).max() < 3e-5, "frame %d" % f
        assert max_lsb_diff(img, sc.render_rt(P, ao=ao_ref, use_bvh=True)) <= 2, "frame %d" % f
    assert (ao_ref < 0.95).sum() > 100000
    ctx.close()


# ---------------------------------------------------------------------------------------------- sequences that actually move
# camera_path() above moves the eye by 0.01 a frame: flows under 2 px, no failed load, history lengths up to 6.  The paths below are
# (eye, target) pairs at 96 x 72; before anything runs on the device the oracle's own state is classified (the float64 statement of
# test_svgf_restatement.py, fed the oracle's maps, tells which pixels load and which keep a history) and each test asserts the branch
# its path is meant for.
def orbit_path(frames, degrees, radius=0.8, height=0.1):
    a = [np.deg2rad(degrees * k) for k in range(frames)]
    return [((float(radius * np.sin(t)), height, float(radius * np.cos(t))), (0.0, 0.0, 0.0)) for t in a]


def moving_case(width=96, height=72, **kw):
    s = dict(RTAO, use_jittered_primary_rays=True)
    s.update(kw)
    return small_case(width=width, height=height, n_lines=6, pts_per_line=30, line_width=0.25, **s)


def oracle_moving_sequence(c, poses):
    """The oracle along (eye, target) poses: per frame the AO image, the frame, and the classification of the reprojection."""
    from test_svgf_restatement import Svgf64
    its = int(c.settings.get("svgf_denoiser_iterations", 5))
    th = (float(c.settings.get("svgf_denoiser_allowed_z_dist", 0.002)), float(c.settings.get("svgf_denoiser_allowed_normal_dist", 0.02)))
    sc = c.oracle_scene()
    sv = lvo.Svgf(c.width, c.height, iterations=its, allowed_z_dist=th[0], allowed_normal_dist=th[1])
    st = Svgf64(c.width, c.height, its, *th)
    frames = []
    for eye, target in poses:
        cameras.apply_camera(c, dict(eye=eye, target=target))
        P = c.oracle_params(sc)
        ao_ref = sv.step(lambda: sc.render_ao(P), P)
        st.step(sv.raw, sv.normal, sv.depth, sv.fwidth, sv.flow)
        length = sv.moments_history[..., 2].copy()
        assert np.array_equal(st.length_history, length)          # the classifier decides as the oracle does
        hit = sv.depth < 50.0
        flow = np.abs(sv.flow).max(axis=-1)
        frames.append(dict(ao=ao_ref, ref=sc.render_rt(P, ao=ao_ref), hit=int(hit.sum()), flow_over_10=int((hit & (flow > 10.0)).sum()),
                           load_failed=int((hit & ~st.masks["load"]).sum()), kept=int((hit & st.masks["success"]).sum()),
                           length_32=int((length == 32).sum()), hit_below_32=int((hit & (length < 32)).sum())))
    return frames


def compare_moving_sequence(c, poses, frames):
    ctx = c.hip_context()
    for f, ((eye, target), want) in enumerate(zip(poses, frames)):
        cameras.apply_camera(c, dict(eye=eye, target=target))
        ctx.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
        img = ctx.render(11)
        assert np.abs(ctx.get_ao() - want["ao"]).max() < 3e-5, "frame %d" % f
        assert max_lsb_diff(img, want["ref"]) <= 2, "frame %d" % f
    ctx.close()


@pytest.mark.gpu
def test_svgf_orbit_of_15_degrees_per_frame(hip_lib):
    c, poses = moving_case(), orbit_path(5, 15.0)
    frames = oracle_moving_sequence(c, poses)
    assert all(fr["flow_over_10"] >= 20 for fr in frames[1:]), [fr["flow_over_10"] for fr in frames]
    compare_moving_sequence(c, poses, frames)


@pytest.mark.gpu
def test_svgf_fast_dolly_in(hip_lib):
    c, poses = moving_case(), [((0.0, 0.0, z), (0.0, 0.0, 0.0)) for z in (1.2, 1.2, 1.0, 0.8, 0.6, 0.45)]
    frames = oracle_moving_sequence(c, poses)
    assert frames[-1]["flow_over_10"] >= 20 and frames[-2]["flow_over_10"] >= 20 and frames[-1]["hit"] > 3 * frames[0]["hit"]
    compare_moving_sequence(c, poses, frames)


@pytest.mark.gpu
def test_svgf_cut_to_the_opposite_side(hip_lib):
    c = moving_case()
    poses = [((0.0, 0.0, 0.8), (0.0, 0.0, 0.0))] * 3 + [((0.1, 0.05, -0.8), (0.0, 0.0, 0.0))] * 2
    frames = oracle_moving_sequence(c, poses)
    # of the pixels that hit the data, a fifth and more keep a history while the camera rests and under 5 % across the cut
    assert frames[2]["kept"] > 0.2 * frames[2]["hit"] and frames[3]["kept"] < 0.05 * frames[3]["hit"] and frames[4]["kept"] > 0.2 * frames[4]["hit"]
    compare_moving_sequence(c, poses, frames)


@pytest.mark.gpu
def test_svgf_pan_off_the_screen_and_back(hip_lib):
    c = moving_case()
    poses = [((0.0, 0.0, 0.8), (x, 0.0, 0.0)) for x in (0.0, 0.0, 0.25, 0.5, 0.25, 0.0)]
    frames = oracle_moving_sequence(c, poses)
    assert frames[3]["hit"] < 0.75 * frames[0]["hit"]                      # a third of the data has left the picture ...
    assert frames[4]["load_failed"] >= 20 and frames[5]["load_failed"] >= 20   # ... and what returns finds no history to load
    compare_moving_sequence(c, poses, frames)


@pytest.mark.gpu
def test_svgf_36_static_frames_reach_the_history_cap(hip_lib):
    c = moving_case(48, 36, use_jittered_primary_rays=False, svgf_denoiser_iterations=1)
    poses = [((0.0, 0.0, 1.0), (0.0, 0.0, 0.0))] * 36       # from 1.0 the data stays off row 0, where no pixel builds a history
    frames = oracle_moving_sequence(c, poses)
    assert frames[30]["length_32"] == 0 and frames[31]["length_32"] >= 20 and frames[-1]["length_32"] >= 20
    assert frames[-1]["hit"] > 300 and frames[-1]["hit_below_32"] == 0
    compare_moving_sequence(c, poses, frames)


@pytest.mark.gpu
def test_svgf_orbit_with_wide_thresholds(hip_lib):
    """allowed_z_dist = 0.02, allowed_normal_dist = 0.2 on an orbit of 3 degrees a frame: nearly every pixel keeps its history, where
    the default thresholds (same maps, classified here) drop most of them."""
    c = moving_case(svgf_denoiser_allowed_z_dist=0.02, svgf_denoiser_allowed_normal_dist=0.2)
    poses = orbit_path(4, 3.0)
    frames = oracle_moving_sequence(c, poses)
    narrow = oracle_moving_sequence(moving_case(), poses)
    assert all(fr["kept"] > 0.9 * fr["hit"] for fr in frames[1:]) and all(fr["kept"] < 0.5 * fr["hit"] for fr in narrow[1:])
    compare_moving_sequence(c, poses, frames)
