"""Rendering mode 3 (MLAB) on the GPU: the device fold (k_mlab_resolve / k_mlab_resolve_long) bit for bit against mlab_fold
(test_mlab_restatement.py) on given runs and on the oracle's prism fragments of whole frames; invariance under rasteriser, tiling,
repetition and the host plugin's states; long runs, pool growth, K, errors and isolation from mode 2.  The band-data and helicity
frames here run the (any, band data) and (6, helicity) instances of the fragment stage only; test_gpu_oit_instances.py holds all
eight, at odd viewports and PPLL tile sizes."""
import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from oracle import lvo
from test_mlab_restatement import F, mlab_colour, mlab_fold, random_runs, window_depth

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3, 1.0)


def _flat(runs):
    offsets = np.zeros(len(runs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r[0]) for r in runs])
    n = int(offsets[-1])
    e = np.zeros((max(n, 1), 3), dtype=np.uint32)
    for p, (c, d, k) in enumerate(runs):
        a, b = int(offsets[p]), int(offsets[p + 1])
        e[a:b, 0], e[a:b, 1], e[a:b, 2] = c, np.asarray(d, F).view(np.uint32), k
    return e[:n], offsets


def _context(bg=BG):
    c = small_case(width=16, height=16, n_lines=2, pts_per_line=4)
    ctx = c.hip_context()
    ctx.set_background(bg)
    return ctx


@pytest.mark.parametrize("K", [1, 3, 8, 17, 64])
def test_given_lists_bit_for_bit(hip_lib, K):
    rng = np.random.default_rng(K)
    w, h = 37, 11
    runs = random_runs(rng, w * h, 40)
    runs[5] = random_runs(rng, 1, 1, tie_depths=True, empty_share=0.0)[0]
    ctx = _context()
    ctx.set_option("mlab_num_layers", K)
    e, off = _flat(runs)
    got = ctx.mlab_resolve(e, off, w, h).reshape(-1, 4)
    assert np.array_equal(got, mlab_fold(runs, K, BG))


def test_given_long_runs_bit_for_bit(hip_lib):
    """runs longer than a lane's LDS share (32) and than the long path's key tile (1024): thousands of fragments, shuffled"""
    rng = np.random.default_rng(99)
    w, h = 6, 2
    runs = random_runs(rng, w * h, 20, empty_share=0.0)
    for p, n in ((0, 33), (3, 1500), (7, 4097), (10, 64)):
        runs[p] = random_runs(rng, 1, 1, empty_share=0.0)[0]
        rgba = rng.random((n, 4)).astype(F)
        rgba[:, 3] = (F(0.001) + rgba[:, 3] * F(0.2)).astype(F)
        runs[p] = (mlab_colour(rgba), rng.random(n).astype(F), rng.choice(1 << 24, n, replace=False).astype(np.uint32))
    e, off = _flat(runs)
    ctx = _context()
    for K in (8, 64):
        ctx.set_option("mlab_num_layers", K)
        assert np.array_equal(ctx.mlab_resolve(e, off, w, h).reshape(-1, 4), mlab_fold(runs, K, BG))


# ---------------------------------------------------------------- whole frames
def frame_reference(c, K, ao=None):
    """mlab_fold of the oracle's prism fragments (ascending (segment, triangle) order), window depth from their positions"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P, ao=ao)
    keep = fr["rgba"][:, 3] >= F(0.001)
    colour = mlab_colour(fr["rgba"])
    depth = window_depth(fr["pos"], c.view, c.proj)
    key = (fr["seg"].astype(np.uint32) << np.uint32(6)) | fr["tri"].astype(np.uint32)
    off = fr["offsets"].astype(np.int64)
    runs = []
    for p in range(c.width * c.height):
        s = slice(off[p], off[p + 1])
        m = keep[s]
        runs.append((colour[s][m], depth[s][m], key[s][m]))
    return mlab_fold(runs, K, c.background).reshape(c.height, c.width, 4), int(keep.sum())


RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=2,
            ambient_occlusion_samples_per_frame=4)


@pytest.mark.parametrize("variant", ["plain", "rtao_depthcue", "larger"])
def test_frame_matches_the_fold_of_the_oracle_fragments(hip_lib, variant):
    if variant == "larger":
        c = small_case(width=256, height=144, n_lines=60, pts_per_line=60, line_width=0.015, transparent=True)
    elif variant == "rtao_depthcue":
        c = small_case(width=120, height=80, transparent=True, depth_cue_strength=0.8, **RTAO)
    else:
        c = small_case(width=120, height=80, transparent=True)
    ctx = c.hip_context()
    ao = None
    if variant == "rtao_depthcue":
        ctx.render(2)
        ao2 = ctx.get_ao().copy()
    img = ctx.render(3)
    if variant == "rtao_depthcue":
        ao = ctx.get_ao().copy()
        assert np.array_equal(ao.view(np.uint32), ao2.view(np.uint32))   # the same AO image as mode 2
    ref, n = frame_reference(c, 8, ao=ao)
    assert n > 500
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)   # (0 LSB expected)
    assert int(ctx.stats().fragments) == n   # every fragment kept, none dropped
    assert np.array_equal(ctx.render(3), img)   # two renders in a row


def _band_frames(case):
    ctx = case.hip_context()
    img = ctx.render(3)
    ref, n = frame_reference(case, 8)
    assert n > 200
    assert max_lsb_diff(img, ref) <= 2
    return img, ref


def test_frame_with_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    c = band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8)
    img, ref = _band_frames(c)
    assert np.array_equal(img, ref)


def test_frame_with_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    c, _, _ = helicity_case(width=120, height=90, transparent=True)
    img, ref = _band_frames(c)
    assert np.array_equal(img, ref)


def test_rasteriser_and_tiling_invariance(hip_lib):
    c = small_case(width=128, height=96, n_lines=40, pts_per_line=40, transparent=True)
    ctx = c.hip_context()
    img = ctx.render(3)
    ctx.set_option("ppll_prism_rasteriser", "lbvh")
    assert np.array_equal(ctx.render(3), img)
    ctx.set_option("ppll_prism_rasteriser", "segments")
    # a tile list dealt over four ranks, each rendered on its own, against the whole frame
    import torch
    tw = th = 32
    tiles = np.array([(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)], dtype=np.uint32)
    out = np.zeros_like(img)
    for r in range(4):
        mine = tiles[r::4]
        buf = torch.empty((len(mine), th, tw, 4), dtype=torch.uint8, device="cuda")
        ctx.render_tiles_device(buf.data_ptr(), mine, tw, th, mode=3)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)


def test_host_plugin_states_match_the_c_abi_frame(hip_lib):
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    from linevis_amd import transfer_function as tfm
    r = host_api.HeadlessLineRenderer(capi.MODE_MLAB)
    r.set_rendering_resolution(120, 80)
    r.set_transfer_function(tfm.standard_transparent())
    r.set_line_data(flow)
    frames = []
    for name, mode, _, settings in host_api.get_test_modes_mlab():
        r.set_new_state(name, mode, settings, resolution=(120, 80))
        assert r.rendering_mode == 3
        st = r.mlab_state()
        assert st["numLayers"] == 8 and st["syncMode"] == int(settings["syncMode"])
        frames.append(r.render_frame())
    for f in frames[1:]:
        assert np.array_equal(f, frames[0])
    # the C-ABI frame of the plugin's context (same lines, camera, transfer function and options)
    import ctypes
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 3, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frames[0])


def _stacked_case(n=3000, width=48, height=40, **settings):
    """thousands of segments stacked through the same pixels (parallel lines along the view axis): runs of > 1000 fragments"""
    pos, off = [], [0]
    rng = np.random.default_rng(5)
    for i in range(n):
        z = -0.9 + 1.8 * i / n
        x0 = -0.02 + 0.0005 * rng.random()
        pos += [(x0, -0.3, z), (x0 + 0.04, 0.3, z)]
        off.append(len(pos))
    pos = np.array(pos, np.float32)
    attr = rng.random(len(pos)).astype(np.float32)
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, attr, np.array(off, np.uint32), 0.02)
    from common import Case
    from linevis_amd import transfer_function as tfm
    return Case(pts, seg, tfm.standard_transparent(), width, height, 0.02, **settings)


def test_long_runs_and_pool_growth(hip_lib):
    """a pool of one slot per pixel (ppll_expected_avg_depth_complexity = 1) is far too small for the stacked scene: the first frame
    grows it and runs the front end again -- the frame still matches the fold, no fragment is dropped, and the statistics of the
    regrown frame count the front end once"""
    c = _stacked_case(ppll_expected_avg_depth_complexity=1, collect_stats=True)
    pw, ph = c.padded()
    ctx = c.hip_context()
    img = ctx.render(3)
    st1 = ctx.stats()
    ref, nfr = frame_reference(c, 8)
    assert st1.max_depth_complexity > 1000
    assert int(st1.ppll_pool_nodes) > 10 * pw * ph and int(st1.ppll_pool_nodes) >= nfr   # grown (it started at pw * ph slots)
    assert int(st1.fragments) == nfr
    assert np.array_equal(img, ref)
    assert np.array_equal(ctx.render(3), img)   # the grown pool is kept: no regrowth this time
    st2 = ctx.stats()
    assert st2.ppll_pool_nodes == st1.ppll_pool_nodes
    for f in ("rays_traced", "prims_tested", "hits_shaded", "fragments"):
        assert getattr(st2, f) == getattr(st1, f) and getattr(st1, f) > 0, f


def test_repeated_and_overlapping_tiles_with_long_runs(hip_lib):
    """a tile list that repeats every tile eight times and adds overlapping ones: every (tile, pixel) pair with a long run is listed for
    k_mlab_resolve_long; each tile equals its part of the whole frame"""
    import torch
    c = _stacked_case()
    ctx = c.hip_context()
    img = ctx.render(3)
    assert ctx.stats().max_depth_complexity > 1000
    tw = th = 16
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid * 8 + [(8, 8), (24, 8), (8, 16), (24, 24), (16, 16)], dtype=np.uint32)
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=3)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)


def test_given_lists_with_repeated_keys_are_rejected(hip_lib):
    ctx = _context()
    runs = random_runs(np.random.default_rng(1), 4, 40, empty_share=0.0)
    runs[2] = (mlab_colour(np.full((5, 4), 0.5, F)), np.arange(5, dtype=F) / F(8.0), np.array([3, 9, 4, 9, 1], np.uint32))
    e, off = _flat(runs)
    with pytest.raises(capi.LineVisError) as err:
        ctx.mlab_resolve(e, off, 2, 2)
    assert err.value.code == -1


def test_k_is_honoured(hip_lib):
    c = small_case(width=96, height=64, n_lines=60, pts_per_line=40, line_width=0.03, transparent=True)
    ctx = c.hip_context()
    imgs = {}
    for K in (1, 64):
        ctx.set_option("mlab_num_layers", K)
        imgs[K] = ctx.render(3)
        ref, _ = frame_reference(c, K)
        assert np.array_equal(imgs[K], ref)
    assert not np.array_equal(imgs[1], imgs[64])


def test_errors_and_isolation_from_mode_2(hip_lib):
    c = small_case(width=96, height=64, transparent=True)
    ctx = c.hip_context()
    for bad in ("0", "65", "-1", "x"):
        with pytest.raises(capi.LineVisError) as e:
            ctx.set_option("mlab_num_layers", bad)
        assert e.value.code == -1
    ctx.set_option("ppll_fragment_source", "capsule_entry")
    with pytest.raises(capi.LineVisError) as e:
        ctx.render(3)
    assert e.value.code == -1
    ctx.set_option("ppll_fragment_source", "auto")
    fresh = c.hip_context().render(2)
    ctx.render(3)
    assert np.array_equal(ctx.render(2), fresh)
