"""Rendering mode 8 (Weighted Blended OIT) on the GPU, byte for byte against wboit_fold (test_wboit_restatement.py): given fragment
lists with all lanes racing, whole frames against the fold of the oracle's prism fragments under both depth weights, RTAO and depth
cues, band data and helicity bands, general cameras, deep pixels, tile lists, a one-rank multi handle, buffers shared with the other
modes, errors and the host plugin.  Every sum is an integer and lv_exp_det / lv_log_det are bit-identical on host and device, so
0 LSB is derived; max_lsb_diff <= 2 stands in front of the equality to size a failure.  "Band data and helicity bands" here are the
(any, band data) and (6, helicity) instances of k_stream_pass only; test_gpu_oit_instances.py holds all eight, at odd viewports and
PPLL tile sizes."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from test_gpu_mlab import RTAO, _stacked_case
from test_wboit_restatement import F, MAX_COUNT, WEIGHTS, random_runs, special_runs, wboit_fold, window_depth

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3, 1.0)
MODE = capi.MODE_WBOIT


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _flat(runs):
    offsets = np.zeros(len(runs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r[1]) for r in runs])
    e = np.concatenate([np.concatenate([np.asarray(r[0], F).reshape(-1, 4), np.asarray(r[1], F).reshape(-1, 1)], axis=1) for r in runs])
    return e, offsets


def _same(img, ref):
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


def _context():
    c = small_case(width=16, height=16, n_lines=2, pts_per_line=4)
    ctx = c.hip_context()
    ctx.set_background(BG)
    return ctx


def _given(ctx, runs, w, h, weight):
    ctx.set_option("wboit_depth_weight", weight)
    e, off = _flat(runs)
    img, sums = ctx.wboit_resolve(e, off, w, h)
    want, want_sums = wboit_fold(runs, BG, weight, details=True)
    assert np.array_equal(sums.reshape(-1, 5), want_sums)
    _same(img.reshape(-1, 4), want)
    return want


# ---------------------------------------------------------------- 1. given lists
@pytest.mark.parametrize("weight", WEIGHTS)
def test_given_lists_bit_for_bit(hip_lib, weight):
    rng = np.random.default_rng(4)
    w, h = 37, 11
    special = special_runs(rng)
    runs = random_runs(rng, w * h - len(special), 40) + special
    want = _given(_context(), runs, w, h, weight)
    assert (want != np.array([26, 51, 77, 255], np.uint8)).any(axis=1).sum() > w * h // 2


def test_given_long_runs_and_shuffled_copies(hip_lib):
    rng = np.random.default_rng(5)
    w, h = 6, 2
    runs = random_runs(rng, w * h, 20, empty_share=0.0)
    for p, n in ((0, 33), (3, 1500), (7, 4097), (10, 64)):
        runs[p] = random_runs(rng, 1, n, alpha_lo=0.0001, alpha_hi=0.002 if n > 100 else 0.3, empty_share=0.0, min_len=n)[0]
    shuffled = []
    for rgba, z in runs:
        o = rng.permutation(len(z))
        shuffled.append((rgba[o], z[o]))
    ctx = _context()
    for weight in WEIGHTS:
        a = _given(ctx, runs, w, h, weight)
        b = _given(ctx, shuffled, w, h, weight)
        assert np.array_equal(a, b)
        assert (a != np.array([26, 51, 77, 255], np.uint8)).any(axis=1).sum() >= 10


def test_a_pixel_with_too_many_fragments_is_refused(hip_lib):
    rng = np.random.default_rng(6)
    n = MAX_COUNT + 1
    rgba = rng.random((n, 4)).astype(F)
    rgba[:, 3] *= F(0.001)
    big = [(rgba, rng.random(n).astype(F)), (rgba[:3], rng.random(3).astype(F))]
    ctx = _context()
    e, off = _flat(big)
    assert _code(lambda: ctx.wboit_resolve(e, off, 2, 1)) == -4   # LV_E_CAPACITY
    good = [(rgba[:MAX_COUNT], big[0][1][:MAX_COUNT]), big[1]]      # exactly the limit: accepted, and exact
    _given(ctx, good, 2, 1, "reference")


# ---------------------------------------------------------------- 2. whole frames
def frame_reference(c, weight="reference", ao=None):
    """wboit_fold of the oracle's prism fragments (all of them: no alpha discard), window depth from their positions.
    Returns (frame, fragments, sums, counts)"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P, ao=ao)
    off = fr["offsets"].astype(np.int64)
    n = int(off[-1])
    rgba = np.asarray(fr["rgba"], dtype=F).reshape(-1, 4)[:n]
    z = window_depth(np.asarray(fr["pos"], dtype=F)[:n], c.view, c.proj)
    runs = [(rgba[off[p]:off[p + 1]], z[off[p]:off[p + 1]]) for p in range(c.width * c.height)]
    frame, sums = wboit_fold(runs, c.background, weight, details=True)
    shape = (c.height, c.width)
    return frame.reshape(shape + (4,)), n, sums.reshape(shape + (5,)), np.diff(off).reshape(shape).astype(np.uint32)


def compares_something(c, ref, n, counts, least_covered=100):
    """fragments > 500, and more than half of the covered pixels differ from the background"""
    assert n > 500
    bg8 = np.floor(np.clip(np.asarray(c.background, F), 0, 1) * F(255.0) + F(0.5)).astype(np.uint8)
    covered = counts > 0
    shown = (ref != bg8).any(axis=2)
    assert covered.sum() > least_covered and 2 * int((covered & shown).sum()) > int(covered.sum()), (int(covered.sum()), int((covered & shown).sum()))


def _frame_checks(c, ctx, weight="reference", ao=None, least_covered=100):
    ctx.set_option("wboit_depth_weight", weight)
    img = ctx.render(MODE)
    ref, n, sums, counts = frame_reference(c, weight, ao=ao)
    compares_something(c, ref, n, counts, least_covered)
    _same(img, ref)
    got_sums, got_counts = ctx.wboit_buffers()
    assert np.array_equal(got_sums, sums) and np.array_equal(got_counts, counts)
    st = ctx.stats()
    assert int(st.fragments) == n and int(st.ppll_pool_nodes) == 0 and int(st.max_depth_complexity) == int(counts.max())
    assert np.array_equal(ctx.render(MODE), img)   # two renders in a row
    return img


@functools.lru_cache(maxsize=None)
def _small():
    return small_case(width=120, height=80, transparent=True)


def test_frame_matches_the_fold_of_the_oracle_fragments(hip_lib):
    c = _small()
    ctx = c.hip_context()
    sums = []
    for weight in WEIGHTS:
        _frame_checks(c, ctx, weight)
        sums.append(ctx.wboit_buffers()[0])
    # the depth weight shows in the sums (0.01 against up to 300); in the frame only where alpha is small enough for the commented
    # line not to saturate, which this transfer function does not produce
    assert np.all(sums[1][..., 3] >= sums[0][..., 3]) and (sums[1][..., 3] > 100 * sums[0][..., 3]).sum() > 100


def test_frame_with_rtao_and_depth_cues(hip_lib):
    c = small_case(width=120, height=80, transparent=True, depth_cue_strength=0.8, **RTAO)
    ctx = c.hip_context()
    ctx.render(2)
    ao2 = ctx.get_ao().copy()
    ctx.render(MODE)
    ao = ctx.get_ao().copy()
    assert np.array_equal(ao.view(np.uint32), ao2.view(np.uint32))   # the same AO image as mode 2
    _frame_checks(c, ctx, ao=ao)


def test_frame_with_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    c = band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8)
    _frame_checks(c, c.hip_context())


def test_frame_with_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    c = helicity_case(width=120, height=90, transparent=True)[0]
    _frame_checks(c, c.hip_context())


@pytest.mark.parametrize("cam", ["roll37", "lens_shift", "inside_rolled"])
def test_frame_under_general_cameras(hip_lib, cam):
    from test_gpu_cameras import cam_case
    c = cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True)
    c.settings["collect_stats"] = True   # (the pass's statistics counters run too)
    ctx = c.hip_context()
    for weight in WEIGHTS:
        _frame_checks(c, ctx, weight)
    ctx.close()


# ---------------------------------------------------------------- 3. the stacked scene: deep pixels, tile lists, a one-rank handle
def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=MODE)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_stacked_scene(hip_lib):
    c = _stacked_case()
    ctx = c.hip_context()
    img = _frame_checks(c, ctx, least_covered=20)   # (a narrow stack: few pixels, deep ones)
    assert int(ctx.stats().max_depth_complexity) > 1000
    # 16 x 16 tile lists: the frame in four interleaved lists, then every tile twice with overlapping ones on top
    tw = th = 16
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid, dtype=np.uint32)
    out = np.zeros_like(img)
    for r in range(4):
        mine = tiles[r::4]
        b = _tiles(ctx, mine, tw, th)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)
    assert _code(ctx.wboit_buffers) == -3   # the last frame was a tile list that leaves pixels out
    tiles = np.array(grid * 2 + [(8, 8), (24, 8), (8, 24), (20, 30), (40, 30)], dtype=np.uint32)
    b = _tiles(ctx, tiles, tw, th)
    for i, (x, y) in enumerate(tiles):
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
    assert np.array_equal(multi.render(MODE), img)
    assert int(multi.stats().ppll_pool_nodes) == 0
    multi.close()


# ---------------------------------------------------------------- 4. errors
def test_errors(hip_lib):
    c = _small()
    ctx = c.hip_context()
    ctx.set_option("wboit_depth_weight", "opengl")
    base = ctx.render(MODE)
    base_sums = ctx.wboit_buffers()[0]
    fresh = c.hip_context()
    fresh.render(MODE)
    assert not np.array_equal(base_sums, fresh.wboit_buffers()[0])   # (a fresh context runs the reference's weight)
    for bad in ("", "OpenGL", "vulkan", "1"):
        assert _code(lambda: ctx.set_option("wboit_depth_weight", bad)) == -1, bad
    assert np.array_equal(ctx.render(MODE), base)
    assert np.array_equal(ctx.wboit_buffers()[0], base_sums)   # the old value stays
    ctx.render(2)   # (modes other than 8 ignore the option)
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto")):
        ctx.set_option(key, value)
        assert _code(lambda: ctx.render(MODE)) == -1, key
        ctx.set_option(key, back)
        assert np.array_equal(ctx.render(MODE), base)
    # (this pair is refused by the frame's general check for every mode; mode 8 only has to pass the refusal on and stay usable)
    ctx.set_options({"use_ribbons": True, "rotating_helicity_bands": True})
    assert _code(lambda: ctx.render(MODE)) == -1
    ctx.set_options({"use_ribbons": False, "rotating_helicity_bands": False})
    assert np.array_equal(ctx.render(MODE), base)
    # the buffers belong to a mode-8 frame over the whole viewport
    ctx.render(2)
    assert _code(ctx.wboit_buffers) == -3
    ctx.render(MODE)
    sums = np.zeros((c.height, c.width, 5), np.int64)
    counts = np.zeros((c.height, c.width), np.uint32)
    p = lambda a: a.ctypes.data
    assert ctx.L.lv_wboit_get_buffers(ctx.h, p(sums), p(counts), c.width * c.height - 1) == -1   # too small
    assert ctx.L.lv_wboit_get_buffers(ctx.h, p(sums), p(counts), c.width * c.height) == 0
    assert ctx.L.lv_wboit_get_buffers(ctx.h, None, p(counts), c.width * c.height) == -1


# ---------------------------------------------------------------- 5. isolation
def test_buffers_shared_with_the_other_modes(hip_lib):
    c = _small()
    streamed = {"mboit_fragment_storage": "streamed"}
    fresh = {}
    for mode in (2, 6, 10, MODE):
        ctx = c.hip_context()
        ctx.set_options(streamed)
        fresh[mode] = ctx.render(mode)
    ctx = c.hip_context()
    ctx.set_options(streamed)
    for mode in (2, MODE, 6, 10, MODE):
        assert np.array_equal(ctx.render(mode), fresh[mode]), mode


# ---------------------------------------------------------------- 6. host plugin
def test_host_plugin(hip_lib):
    import ctypes
    from linevis_amd import transfer_function as tfm
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))

    def plugin(**kw):
        flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
        r = host_api.HeadlessLineRenderer(MODE, **kw)
        r.set_rendering_resolution(120, 80)
        r.set_transfer_function(tfm.standard_transparent())
        r.set_line_data(flow)
        return r

    r = plugin()
    assert r.rendering_mode == 8 and r.wboit_state() == {"depthWeight": "reference"} and r.mlab_state() is None
    r.set_new_state("WBOIT", MODE, {}, resolution=(120, 80))
    frame = r.render_frame()
    assert (frame[..., :3] != 255).any(axis=2).sum() > 100   # (the plugin's default line width: thin lines)
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 8, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frame)

    def sums_of_last_frame():
        sums = np.zeros((80, 120, 5), np.int64)
        counts = np.zeros((80, 120), np.uint32)
        assert capi.load().lv_wboit_get_buffers(ctypes.c_void_p(hctx), sums.ctypes.data_as(ctypes.c_void_p),
                                                counts.ctypes.data_as(ctypes.c_void_p), 120 * 80) == 0
        return sums

    reference = sums_of_last_frame()
    r.set_new_settings({"wboit_depth_weight": "opengl"})
    assert r.wboit_state() == {"depthWeight": "opengl"}
    other = r.render_frame()
    opengl = sums_of_last_frame()
    assert (opengl[..., 3] > 100 * reference[..., 3]).sum() > 100   # the plugin's key reached the kernels
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 8, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, other)
    assert np.array_equal(r.render_frame(), other) and np.array_equal(sums_of_last_frame(), opengl)
    r.set_new_settings({"wboit_depth_weight": "directx"})   # refused by the C ABI: the weight stays
    assert r.wboit_state() == {"depthWeight": "opengl"}
