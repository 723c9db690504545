"""Rendering mode 6 (MBOIT) on the GPU: the device sweeps (k_mboit_resolve / k_mboit_resolve_long) bit for bit against mboit_fold
(test_mboit_restatement.py) on given runs -- frame and moments -- and on the oracle's prism fragments of whole frames; invariance
under rasteriser, tiling, repetition, fragment order and the host plugin's states; long runs, pool growth, options, errors, the
degenerate-pixel counter and isolation from modes 2 and 3.  The band-data and helicity frames here run the (any, band data) and
(6, helicity) instances of the fragment stage only; test_gpu_oit_instances.py holds all eight, at odd viewports and PPLL tile sizes."""
import ctypes

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from test_mboit_restatement import F, LOG_MAX, LOG_MIN, U32, log_depth_range, mboit_fold, random_runs, special_runs, view_depth

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3, 1.0)


def _flat(runs):
    offsets = np.zeros(len(runs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r[1]) for r in runs])
    e = np.zeros((int(offsets[-1]), 5), dtype=F)
    for p, (rgba, z) in enumerate(runs):
        a, b = int(offsets[p]), int(offsets[p + 1])
        e[a:b, :4], e[a:b, 4] = rgba, z
    return e, offsets


def _context(bg=BG):
    c = small_case(width=16, height=16, n_lines=2, pts_per_line=4)
    ctx = c.hip_context()
    ctx.set_background(bg)
    return ctx


def _same(got, want):
    frame, mom = got
    wf, wm = want
    return np.array_equal(frame.reshape(-1, 4), wf) and np.array_equal(mom.reshape(wm.shape).view(U32), wm.view(U32))


@pytest.mark.parametrize("N", [4, 6, 8])
def test_given_lists_bit_for_bit(hip_lib, N):
    rng = np.random.default_rng(N)
    w, h = 37, 11
    runs = random_runs(rng, w * h, 40)
    sp = special_runs(rng)
    runs[:len(sp)] = sp
    ctx = _context()
    e, off = _flat(runs)
    got = ctx.mboit_resolve(e, off, w, h, LOG_MIN, LOG_MAX, N)
    want = mboit_fold(runs, N, BG, LOG_MIN, LOG_MAX)
    assert np.array_equal(got[1].reshape(want[1].shape).view(U32), want[1].view(U32))
    assert np.array_equal(got[0].reshape(-1, 4), want[0])


def test_given_long_runs_bit_for_bit_in_any_order(hip_lib):
    """runs longer than a lane's share (one wave per pixel): 33, 1500 and 4097 fragments; shuffled copies give the same bytes"""
    rng = np.random.default_rng(99)
    w, h = 6, 2
    runs = random_runs(rng, w * h, 20, empty_share=0.0)
    for p, n in ((0, 33), (3, 1500), (7, 4097), (10, 64), (11, 49)):
        runs[p] = random_runs(rng, 1, n, alpha_lo=0.001, alpha_hi=0.05 if n > 100 else 0.3, empty_share=0.0, min_len=n)[0]
    shuffled = []
    for rgba, z in runs:
        o = rng.permutation(len(z))
        shuffled.append((rgba[o], z[o]))
    ctx = _context()
    for N in (4, 6, 8):
        want = mboit_fold(runs, N, BG, LOG_MIN, LOG_MAX)
        assert (want[0] != np.array([26, 51, 77, 255], np.uint8)).any(axis=1).sum() >= 10
        for r in (runs, shuffled):
            e, off = _flat(r)
            assert _same(ctx.mboit_resolve(e, off, w, h, LOG_MIN, LOG_MAX, N), want), N


# ---------------------------------------------------------------- whole frames
def frame_reference(c, N, ao=None, over=0.1, bias=None):
    """mboit_fold of the oracle's prism fragments: view depth from their positions, the log depth range from the points' box.
    Returns (frame, fragments, moments, degenerate pixels)."""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P, ao=ao)
    off = fr["offsets"].astype(np.int64)
    n = int(off[-1])
    rgba = np.asarray(fr["rgba"], dtype=F).reshape(-1, 4)[:n]
    z = view_depth(np.asarray(fr["pos"], dtype=F)[:n], c.view)
    runs = [(rgba[off[p]:off[p + 1]], z[off[p]:off[p + 1]]) for p in range(c.width * c.height)]
    pos = c.points["linePosition"]
    lmin, lmax = log_depth_range(pos.min(axis=0), pos.max(axis=0), c.view, c.near, c.far)
    frame, mom, deg = mboit_fold(runs, N, c.background, lmin, lmax, over, bias, details=True)
    return frame.reshape(c.height, c.width, 4), n, mom, deg


def compares_something(c, ref, n, mom, least=500):
    """fragments > 500, and more than half of the pixels with b_0 over the threshold differ from the background"""
    assert n > least
    bg8 = np.floor(np.clip(np.asarray(c.background, F), 0, 1) * F(255.0) + F(0.5)).astype(np.uint8)
    covered = mom[:, 0] > 0
    shown = (ref.reshape(-1, 4) != bg8).any(axis=1)
    assert covered.sum() > 100 and 2 * int((covered & shown).sum()) > int(covered.sum()), (int(covered.sum()), int((covered & shown).sum()))


RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=2,
            ambient_occlusion_samples_per_frame=4)
# with the default bias of 4 moments (5e-7) about a tenth of the covered pixels of these scenes (single fragments on tube
# silhouettes) degenerate to the background: the "plain" case keeps it (and checks the counter), the others run with 5e-5, under
# which the statement shows nearly every covered pixel
FRAME_BIAS = 5e-5


def variant_case(variant):
    if variant == "larger":
        return small_case(width=256, height=144, n_lines=60, pts_per_line=60, line_width=0.015, transparent=True)
    if variant == "rtao_depthcue":
        return small_case(width=120, height=80, transparent=True, depth_cue_strength=0.8, **RTAO)
    return small_case(width=120, height=80, transparent=True)


@pytest.mark.parametrize("variant", ["plain", "rtao_depthcue", "larger"])
def test_frame_matches_the_statement_on_the_oracle_fragments(hip_lib, variant):
    c = variant_case(variant)
    c.settings["collect_stats"] = True
    ctx = c.hip_context()
    bias = None if variant == "plain" else FRAME_BIAS
    ctx.set_option("mboit_moment_bias", bias or "auto")
    ao = None
    if variant == "rtao_depthcue":
        ctx.render(2)
        ao2 = ctx.get_ao().copy()
    for N in ((4, 6, 8) if variant == "plain" else (4,)):
        ctx.set_option("mboit_num_moments", N)
        img = ctx.render(6)
        if variant == "rtao_depthcue":
            ao = ctx.get_ao().copy()
            assert np.array_equal(ao.view(np.uint32), ao2.view(np.uint32))   # the same AO image as mode 2
        ref, n, mom, deg = frame_reference(c, N, ao=ao, bias=bias)
        compares_something(c, ref, n, mom)
        assert variant != "plain" or N != 4 or deg > 50   # (the default bias: degenerate single fragments, counted below)
        assert max_lsb_diff(img, ref) <= 2
        assert np.array_equal(img, ref)   # (0 LSB expected)
        st = ctx.stats()
        assert int(st.fragments) == n   # every fragment kept, none dropped
        assert int(st.mboit_degenerate_pixels) == deg
        assert np.array_equal(ctx.render(6), img)   # two renders in a row


def _band_frames(case):
    ctx = case.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    img = ctx.render(6)
    ref, n, mom, _ = frame_reference(case, 4, bias=FRAME_BIAS)
    compares_something(case, ref, n, mom)
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


def test_frame_with_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    _band_frames(band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8))


def test_frame_with_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    c, _, _ = helicity_case(width=120, height=90, transparent=True)
    _band_frames(c)


@pytest.mark.parametrize("cam", ["roll37", "lens_shift", "inside_rolled"])
def test_frame_under_general_cameras(hip_lib, cam):
    """inside_rolled: near = 0.001 and the eye inside the data set -- the depth range clamps to the near plane"""
    from test_gpu_cameras import cam_case
    c = cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    for N in (4, 8):
        ctx.set_option("mboit_num_moments", N)
        img = ctx.render(6)
        ref, n, mom, _ = frame_reference(c, N, bias=FRAME_BIAS)
        compares_something(c, ref, n, mom)
        assert max_lsb_diff(img, ref) <= 2
        assert np.array_equal(img, ref)
    if cam == "inside_rolled":
        pos = c.points["linePosition"]
        lmin, _ = log_depth_range(pos.min(axis=0), pos.max(axis=0), c.view, c.near, c.far)
        assert abs(float(lmin) - np.log(0.001)) < 1e-4
    ctx.close()


def test_rasteriser_and_tiling_invariance(hip_lib):
    c = small_case(width=128, height=96, n_lines=40, pts_per_line=40, transparent=True)
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    img = ctx.render(6)
    assert (img != 255).any(axis=2).sum() > 500
    ctx.set_option("ppll_prism_rasteriser", "lbvh")
    assert np.array_equal(ctx.render(6), img)
    ctx.set_option("ppll_prism_rasteriser", "segments")
    # a tile list dealt over four ranks, each rendered on its own, against the whole frame
    import torch
    tw = th = 32
    tiles = np.array([(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)], dtype=np.uint32)
    out = np.zeros_like(img)
    for r in range(4):
        mine = tiles[r::4]
        buf = torch.empty((len(mine), th, tw, 4), dtype=torch.uint8, device="cuda")
        ctx.render_tiles_device(buf.data_ptr(), mine, tw, th, mode=6)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)


def test_host_plugin_states_match_the_c_abi_frame(hip_lib):
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    from linevis_amd import transfer_function as tfm
    r = host_api.HeadlessLineRenderer(capi.MODE_MBOIT)
    r.set_rendering_resolution(120, 80)
    r.set_transfer_function(tfm.standard_transparent())
    r.set_line_data(flow)
    frames = {4: [], 8: []}
    for name, mode, _, settings in host_api.get_test_modes_mboit():
        r.set_new_state(name, mode, settings, resolution=(120, 80))
        assert r.rendering_mode == 6
        st = r.mboit_state()
        N = int(settings["numMoments"])
        assert st["numMoments"] == N and st["useRenderTargets"] == (settings["useRenderTargets"] == "true")
        assert abs(st["overestimationBeta"] - 0.1) < 1e-7
        if "syncMode" in settings:
            assert st["syncMode"] == int(settings["syncMode"])
        frames[N].append(r.render_frame())
    for N in (4, 8):
        assert len(frames[N]) == 5
        for f in frames[N][1:]:
            assert np.array_equal(f, frames[N][0])
    assert not np.array_equal(frames[4][0], frames[8][0])
    # the C-ABI frame of the plugin's context (same lines, camera, transfer function and options: the last state, 8 moments)
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 6, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frames[8][0])
    # a state that asks for a family that is not built is refused: the previous state stays, the next render reports the error
    name, mode, _, settings = host_api.get_test_modes_mboit()[0]
    for extra in ({"usePowerMoments": "false"}, {"pixelFormat": "UNORM"}):
        r.set_new_state(name, mode, dict(settings, **extra), resolution=(120, 80))
        assert r.mboit_state()["numMoments"] == 8
        with pytest.raises(capi.LineVisError):
            r.render_frame()
    r.set_new_state(name, mode, dict(settings, usePowerMoments="true", pixelFormat="Float"), resolution=(120, 80))
    assert np.array_equal(r.render_frame(), frames[4][0])


def test_long_runs_and_pool_growth(hip_lib):
    """a pool of one slot per pixel is far too small for the stacked scene: the first frame grows it and runs the front end again --
    the frame still matches the statement, no fragment is dropped, and the statistics of the regrown frame count the front end once"""
    from test_gpu_mlab import _stacked_case
    c = _stacked_case(ppll_expected_avg_depth_complexity=1, collect_stats=True)
    pw, ph = c.padded()
    ctx = c.hip_context()
    img = ctx.render(6)
    st1 = ctx.stats()
    ref, nfr, mom, deg = frame_reference(c, 4)
    compares_something(c, ref, nfr, mom)
    assert st1.max_depth_complexity > 1000
    assert int(st1.ppll_pool_nodes) > 10 * pw * ph and int(st1.ppll_pool_nodes) >= nfr   # grown (it started at pw * ph slots)
    assert int(st1.fragments) == nfr
    assert np.array_equal(img, ref)
    assert int(st1.mboit_degenerate_pixels) == deg
    assert np.array_equal(ctx.render(6), img)   # the grown pool is kept: no regrowth this time
    st2 = ctx.stats()
    assert st2.ppll_pool_nodes == st1.ppll_pool_nodes
    for f in ("rays_traced", "prims_tested", "hits_shaded", "fragments"):
        assert getattr(st2, f) == getattr(st1, f) and getattr(st1, f) > 0, f


def test_repeated_and_overlapping_tiles_with_long_runs(hip_lib):
    import torch
    from test_gpu_mlab import _stacked_case
    c = _stacked_case()
    ctx = c.hip_context()
    img = ctx.render(6)
    assert ctx.stats().max_depth_complexity > 1000
    tw = th = 16
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid * 8 + [(8, 8), (24, 8), (8, 16), (24, 24), (16, 16)], dtype=np.uint32)
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=6)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)


def test_options_change_the_frame_and_match_the_statement(hip_lib):
    c = small_case(width=96, height=64, n_lines=60, pts_per_line=40, line_width=0.03, transparent=True)
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    base = ctx.render(6)
    ctx.set_option("mboit_overestimation", 0.6)
    over = ctx.render(6)
    ref, n, mom, _ = frame_reference(c, 4, over=0.6, bias=FRAME_BIAS)
    compares_something(c, ref, n, mom)
    assert np.array_equal(over, ref) and not np.array_equal(over, base)
    ctx.set_option("mboit_overestimation", 0.1)
    ctx.set_option("mboit_moment_bias", 5e-3)
    biased = ctx.render(6)
    ref, _, _, _ = frame_reference(c, 4, bias=5e-3)
    assert np.array_equal(biased, ref) and not np.array_equal(biased, base)
    ctx.set_option("mboit_moment_bias", "auto")
    ref, _, _, _ = frame_reference(c, 4)
    assert np.array_equal(ctx.render(6), ref)
    ctx.set_option("mboit_num_moments", 8)
    assert np.array_equal(ctx.render(6), frame_reference(c, 8)[0])


def test_errors_leave_the_old_value_and_other_modes_untouched(hip_lib):
    c = small_case(width=96, height=64, transparent=True)
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    ctx.set_option("mboit_num_moments", 6)
    ctx.set_option("mboit_overestimation", 0.25)
    img = ctx.render(6)
    bad = [("mboit_num_moments", v) for v in ("0", "5", "10", "x")] + [("mboit_overestimation", v) for v in ("-0.1", "1.5", "x")] + \
          [("mboit_moment_bias", v) for v in ("0", "-1", "0.2", "x")] + [("mboit_use_power_moments", "false"), ("mboit_pixel_format", "UNORM")]
    for key, value in bad:
        with pytest.raises(capi.LineVisError) as e:
            ctx.set_option(key, value)
        assert e.value.code == -1, (key, value)
    with pytest.raises(capi.LineVisError) as e:
        ctx.set_option("mboit_use_power_moments", "false")
    assert "trigonometric" in str(e.value)
    with pytest.raises(capi.LineVisError) as e:
        ctx.set_option("mboit_pixel_format", "UNORM")
    assert "quantised" in str(e.value)
    ctx.set_option("mboit_use_power_moments", "true")
    ctx.set_option("mboit_pixel_format", "Float")
    assert np.array_equal(ctx.render(6), img)   # the old values are in force
    assert np.array_equal(img, frame_reference(c, 6, over=0.25, bias=FRAME_BIAS)[0])
    ctx.set_option("ppll_fragment_source", "capsule_entry")
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(6)
    assert e.value.code == -1
    ctx.set_option("ppll_fragment_source", "auto")
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(7)
    assert e.value.code == -1
    # isolation: after mode 6, modes 2 and 3 render what fresh contexts render
    fresh2, fresh3 = c.hip_context().render(2), c.hip_context().render(3)
    ctx.render(6)
    assert np.array_equal(ctx.render(2), fresh2)
    ctx.render(6)
    assert np.array_equal(ctx.render(3), fresh3)
