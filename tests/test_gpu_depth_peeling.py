"""Rendering mode 9 (depth peeling) on the GPU, byte for byte against depth_peel_fold (test_depth_peeling_restatement.py): given
fragment lists with all lanes racing for the slots, whole frames against the fold of the oracle's prism fragments, RTAO and depth
cues, band data and helicity bands, general cameras, deep pixels and the cap, tile lists (repeated and overlapping tiles), a one-rank
multi handle, buffers shared with the other modes, errors and the host plugin.  One fixed float32 order and no library exp on this
path, so 0 LSB is derived; max_lsb_diff <= 2 stands in front of the equality to size a failure.  "Band data and helicity bands"
here are the (any, band data) and (6, helicity) instances of k_peel_pass / k_peel_layer only; test_gpu_oit_instances.py holds all of
them, at odd viewports and PPLL tile sizes."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from test_depth_peeling_restatement import F, depth_peel_fold, random_runs, special_runs, window_depth
from test_gpu_mlab import RTAO, _stacked_case

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3, 1.0)
MODE = capi.MODE_DEPTH_PEELING
STACKED_N = 1100   # segments of the stacked scene: still more than 1000 fragments on a pixel, and a frame of as many passes stays short


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _flat(runs):
    offsets = np.zeros(len(runs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r[1]) for r in runs])
    rgba = np.concatenate([np.asarray(r[0], F).reshape(-1, 4) for r in runs])
    z = np.concatenate([np.asarray(r[1], F).reshape(-1) for r in runs])
    keys = np.concatenate([np.asarray(r[2], np.uint32).reshape(-1) for r in runs])
    return rgba, z, keys, offsets


def _same(img, ref):
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


def _context():
    c = small_case(width=16, height=16, n_lines=2, pts_per_line=4)
    ctx = c.hip_context()
    ctx.set_background(BG)
    return ctx


def _given(ctx, runs, w, h, max_layers=2000):
    ctx.set_option("depth_peeling_max_layers", max_layers)
    img, accum, layers = ctx.depth_peeling_resolve(*_flat(runs), w, h)
    want, want_accum, want_layers = depth_peel_fold(runs, BG, max_layers, details=True)
    assert np.array_equal(layers.reshape(-1), want_layers)
    assert np.array_equal(accum.reshape(-1, 4).view(np.uint32), want_accum.view(np.uint32))
    _same(img.reshape(-1, 4), want)
    return want


# ---------------------------------------------------------------- 1. given lists
def test_given_lists_bit_for_bit(hip_lib):
    rng = np.random.default_rng(4)
    w, h = 37, 11
    special = special_runs(rng)
    runs = random_runs(rng, w * h - len(special), 40) + special
    want = _given(_context(), runs, w, h)
    assert (want != np.array([26, 51, 77, 255], np.uint8)).any(axis=1).sum() > w * h // 2


def test_given_long_runs_shuffled_copies_and_the_cap(hip_lib):
    rng = np.random.default_rng(5)
    w, h = 6, 2
    runs = random_runs(rng, w * h, 20, empty_share=0.0)
    for p, n in ((0, 33), (3, 1500), (7, 2500), (10, 64)):
        rgba, z, keys = random_runs(rng, 1, n, empty_share=0.0, tie_share=0.02, min_len=n)[0]
        rgba[:, 3] *= F(0.01) if n > 100 else F(0.3)   # (the far layers still show in the accumulator)
        runs[p] = (rgba, z, keys)
    # the tie rule and the cap are exercised
    assert any(len(np.unique(r[1])) < len(r[1]) for r in runs)
    assert max(len(np.unique(r[1][r[1] < 1])) for r in runs) > 2000
    shuffled = []
    for rgba, z, keys in runs:
        o = rng.permutation(len(z))
        shuffled.append((rgba[o], z[o], keys[o]))
    ctx = _context()
    frames = {}
    for cap in (1, 3, 2000):
        a = _given(ctx, runs, w, h, cap)
        b = _given(ctx, shuffled, w, h, cap)
        assert np.array_equal(a, b)
        frames[cap] = a
    assert not np.array_equal(frames[1], frames[3]) and not np.array_equal(frames[3], frames[2000])


# ---------------------------------------------------------------- 2. whole frames
def frame_reference(c, max_layers=2000, ao=None):
    """depth_peel_fold of the oracle's prism fragments (all of them: no alpha discard), window depth from their positions, mode 3's
    primitive key.  Returns (frame, fragments, accumulators, layers, counts)"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P, ao=ao)
    off = fr["offsets"].astype(np.int64)
    n = int(off[-1])
    rgba = np.asarray(fr["rgba"], dtype=F).reshape(-1, 4)[:n]
    z = window_depth(np.asarray(fr["pos"], dtype=F)[:n], c.view, c.proj)
    key = ((fr["seg"].astype(np.uint32) << np.uint32(6)) | fr["tri"].astype(np.uint32))[:n]
    runs = [(rgba[off[p]:off[p + 1]], z[off[p]:off[p + 1]], key[off[p]:off[p + 1]]) for p in range(c.width * c.height)]
    frame, accum, layers = depth_peel_fold(runs, c.background, max_layers, details=True)
    shape = (c.height, c.width)
    return (frame.reshape(shape + (4,)), n, accum.reshape(shape + (4,)), layers.reshape(shape),
            np.diff(off).reshape(shape).astype(np.uint32))


def compares_something(c, ref, n, counts, layers, least_covered=100, least_deep=50):
    """fragments > 500, more than half of the covered pixels differ from the background, pixels with at least 3 layers"""
    assert n > 500
    bg8 = np.floor(np.clip(np.asarray(c.background, F), 0, 1) * F(255.0) + F(0.5)).astype(np.uint8)
    covered = counts > 0
    shown = (ref != bg8).any(axis=2)
    assert covered.sum() > least_covered and 2 * int((covered & shown).sum()) > int(covered.sum()), (int(covered.sum()), int((covered & shown).sum()))
    assert int((layers >= 3).sum()) > least_deep, int((layers >= 3).sum())


def _frame_checks(c, ctx, max_layers=2000, ao=None, least_covered=100, least_deep=50, again=True):
    ctx.set_option("depth_peeling_max_layers", max_layers)
    img = ctx.render(MODE)
    ref, n, accum, layers, counts = frame_reference(c, max_layers, ao=ao)
    compares_something(c, ref, n, counts, layers, least_covered, least_deep)
    _same(img, ref)
    got_accum, got_layers, got_counts = ctx.depth_peeling_buffers()
    assert np.array_equal(got_counts, counts) and np.array_equal(got_layers, layers)
    assert np.array_equal(got_accum.view(np.uint32), accum.view(np.uint32))
    st = ctx.stats()
    assert int(st.fragments) == n and int(st.ppll_pool_nodes) == 0 and int(st.max_depth_complexity) == int(counts.max())
    if again:
        assert np.array_equal(ctx.render(MODE), img)   # two renders in a row
    return img


@functools.lru_cache(maxsize=None)
def _small():
    return small_case(width=120, height=80, transparent=True)


def test_frame_matches_the_fold_of_the_oracle_fragments(hip_lib):
    c = _small()
    _frame_checks(c, c.hip_context())


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
    c.settings["collect_stats"] = True   # (the count pass's statistics counters run too)
    ctx = c.hip_context()
    _frame_checks(c, ctx)
    ctx.close()


# ---------------------------------------------------------------- 3. the stacked scene: deep pixels, the cap, tile lists, a one-rank handle
def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=MODE)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_stacked_scene(hip_lib):
    c = _stacked_case(n=STACKED_N)
    ctx = c.hip_context()
    # (a narrow stack: few pixels, deep ones; the cap if a pixel exceeds it; a frame of a thousand passes: not rendered twice)
    img = _frame_checks(c, ctx, least_covered=20, least_deep=20, again=False)
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
    assert _code(ctx.depth_peeling_buffers) == -3   # the last frame was a tile list that leaves pixels out
    tiles = np.array(grid * 2 + [(8, 8), (24, 8), (8, 24), (20, 30), (40, 30)], dtype=np.uint32)
    b = _tiles(ctx, tiles, tw, th)   # (a layer kernel that ran per (tile, pixel) cell would accumulate these pixels twice)
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


def test_stacked_scene_with_three_layers(hip_lib):
    c = _stacked_case(n=STACKED_N)
    ctx = c.hip_context()
    capped = _frame_checks(c, ctx, max_layers=3, least_covered=20, least_deep=20)
    ctx.set_option("depth_peeling_max_layers", 2000)
    assert not np.array_equal(ctx.render(MODE), capped)


# ---------------------------------------------------------------- 4. errors
def test_errors(hip_lib):
    c = _small()
    ctx = c.hip_context()
    ctx.set_option("depth_peeling_max_layers", 2)
    base = ctx.render(MODE)
    fresh = c.hip_context()
    assert not np.array_equal(base, fresh.render(MODE))   # (a fresh context peels every layer)
    for bad in ("", "0", "2001", "-1", "many"):
        assert _code(lambda: ctx.set_option("depth_peeling_max_layers", bad)) == -1, bad
    assert np.array_equal(ctx.render(MODE), base)   # the old value stays
    ctx.render(2)   # (modes other than 9 ignore the option)
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto")):
        ctx.set_option(key, value)
        assert _code(lambda: ctx.render(MODE)) == -1, key
        ctx.set_option(key, back)
        assert np.array_equal(ctx.render(MODE), base)
    # (this pair is refused by the frame's general check for every mode; mode 9 only has to pass the refusal on and stay usable)
    ctx.set_options({"use_ribbons": True, "rotating_helicity_bands": True})
    assert _code(lambda: ctx.render(MODE)) == -1
    ctx.set_options({"use_ribbons": False, "rotating_helicity_bands": False})
    assert np.array_equal(ctx.render(MODE), base)
    # the buffers belong to a mode-9 frame over the whole viewport
    ctx.render(2)
    assert _code(ctx.depth_peeling_buffers) == -3
    ctx.render(capi.MODE_DEPTH_COMPLEXITY)
    assert _code(ctx.depth_peeling_buffers) == -3
    ctx.render(MODE)
    accum = np.zeros((c.height, c.width, 4), np.float32)
    layers = np.zeros((c.height, c.width), np.uint32)
    counts = np.zeros((c.height, c.width), np.uint32)
    p = lambda a: a.ctypes.data
    assert ctx.L.lv_depth_peeling_get_buffers(ctx.h, p(accum), p(layers), p(counts), c.width * c.height - 1) == -1   # too small
    assert ctx.L.lv_depth_peeling_get_buffers(ctx.h, p(accum), p(layers), p(counts), c.width * c.height) == 0
    assert ctx.L.lv_depth_peeling_get_buffers(ctx.h, None, p(layers), p(counts), c.width * c.height) == -1


# ---------------------------------------------------------------- 5. isolation
def test_buffers_shared_with_the_other_modes(hip_lib):
    c = _small()
    streamed = {"mboit_fragment_storage": "streamed"}
    fresh = {}
    for mode in (2, 6, 8, 10, 5, MODE):
        ctx = c.hip_context()
        ctx.set_options(streamed)
        fresh[mode] = ctx.render(mode)
    ctx = c.hip_context()
    ctx.set_options(streamed)
    for mode in (2, MODE, 6, 5, 8, MODE, 10, 5, MODE, 2):
        assert np.array_equal(ctx.render(mode), fresh[mode]), mode


def _equal(a, b):
    if isinstance(a, dict):
        return a == b
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


STREAMED = {"mboit_fragment_storage": "streamed"}
GETTERS = {5: lambda x: (x.depth_complexity_buffers(), x.depth_complexity_stats()), 6: lambda x: x.mboit_moments(),
           8: lambda x: x.wboit_buffers(), 9: lambda x: x.depth_peeling_buffers(), 10: lambda x: x.atomic_loop_buffers()}


def _getter_case():
    return small_case(width=64, height=48, n_lines=4, pts_per_line=9, transparent=True)   # 32 segments


def _resolves(off, n=3):
    """The given-lists call of every mode that has one, on a rectangle of 2 x 1 pixels with n entries under the offsets `off`: colours
    and packed colours repeat three values, depths ascend inside (0, 1), keys are arange (unique: mode 3's rule)"""
    off = np.asarray(off, np.uint64)
    reps = (n + 2) // 3
    rgba = np.tile(np.array([[0.9, 0.2, 0.1, 0.5], [0.1, 0.8, 0.3, 0.25], [0.2, 0.3, 0.7, 0.75]], F), (reps, 1))[:n]
    packed = np.tile(np.array([0x80112233, 0x40445566, 0xC0778899], np.uint32), reps)[:n]
    z = (np.arange(1, n + 1, dtype=np.float64) / (n + 1)).astype(F)   # (n = 3: 0.25, 0.5, 0.75)
    keys = np.arange(n, dtype=np.uint32)
    return {
        3: lambda x: x.mlab_resolve(np.stack([packed, z.view(np.uint32), keys], axis=1), off, 2, 1),
        6: lambda x: x.mboit_resolve(np.concatenate([rgba, 1.0 + z[:, None]], axis=1), off, 2, 1, -1.0, 3.0),
        8: lambda x: x.wboit_resolve(np.concatenate([rgba, z[:, None]], axis=1), off, 2, 1),
        9: lambda x: x.depth_peeling_resolve(rgba, z, keys, off, 2, 1),
        10: lambda x: x.atomic_loop_resolve((z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | packed.astype(np.uint64), off, 2, 1),
    }


def test_one_record_of_the_last_frame_for_every_getter(hip_lib):
    """The context keeps ONE record of the last frame behind the *_get_* calls of modes 5, 6 (streamed), 8, 9 and 10.  A frame sets it;
    a *_resolve_buffers call of ANY other mode overwrites the per-pixel counts and the counters and clears it, so the getter answers
    LV_E_STATE (-3) until the next frame of its mode, whose buffers are those of a fresh context."""
    c = _getter_case()
    streamed, getters = STREAMED, GETTERS
    resolves = _resolves([0, 2, 3])   # two pixels, three entries
    fresh = {}
    for mode, get in getters.items():
        f = c.hip_context()
        f.set_options(streamed)
        fresh[mode] = (f.render(mode), get(f))
    ctx = c.hip_context()
    ctx.set_options(streamed)
    for mode, get in getters.items():
        for other, resolve in resolves.items():
            if other == mode:
                continue
            assert np.array_equal(ctx.render(mode), fresh[mode][0]), (mode, other)
            assert _equal(get(ctx), fresh[mode][1]), (mode, other)   # the getter succeeds, with a fresh context's buffers
            resolve(ctx)
            assert _code(lambda: get(ctx)) == -3, (mode, other)
        assert np.array_equal(ctx.render(mode), fresh[mode][0]), mode
        assert _equal(get(ctx), fresh[mode][1]), mode
    # the pair that used to answer LV_OK with the counts of the given lists: mode 8, mode 10's lists, mode 8's getter
    ctx.render(8)
    ctx.wboit_buffers()
    resolves[10](ctx)
    assert _code(ctx.wboit_buffers) == -3
    assert _code(ctx.atomic_loop_buffers) == -3   # (and the lists' own mode has no frame either)


def test_malformed_given_lists_and_short_getter_capacities(hip_lib):
    """What the *_resolve_buffers calls of modes 3, 6, 8, 9 and 10 refuse (LV_E_INVALID, -1) before they touch the context -- offsets
    that do not run from 0 to num_entries or descend, a pixel over the mode's maximum, mode 6's reserved depth word -- with the longest
    accepted pixel of every mode next to the refused one; a refused call leaves the last frame's getter as it was, byte for byte; and
    every getter refuses a capacity one short of the viewport.  Codes and acceptance only: the results of given lists have the
    bit-for-bit tests of each mode."""
    c = _getter_case()
    ctx = c.hip_context()
    ctx.set_options(STREAMED)
    # offsets: first not 0, last under and over num_entries = 3, a descending pair between the right ends
    bad_offsets = ([1, 2, 3], [0, 2, 2], [0, 2, 4], [0, 5, 3])
    for off in bad_offsets:
        for mode, resolve in _resolves(off).items():
            assert _code(lambda: resolve(ctx)) == -1, (mode, off)
    # the per-pixel maximum: all n entries in pixel 0 (mode 8 finds its own through the resolve: test_gpu_wboit.py)
    for mode, most in ((3, 65535), (6, 65534), (10, 131071)):
        assert _code(lambda: _resolves([0, most + 1, most + 1], most + 1)[mode](ctx)) == -1, mode
        _resolves([0, most, most], most)[mode](ctx)
    ctx.set_option("depth_peeling_max_layers", 2000)
    _resolves([0, 3000, 3000], 3000)[9](ctx)   # mode 9 has no maximum: more entries than layers
    # mode 6: the depth word 0xFFFFFFFF is reserved
    entries = np.array([[0.9, 0.2, 0.1, 0.5, 1.25], [0.1, 0.8, 0.3, 0.25, 1.5], [0.2, 0.3, 0.7, 0.75, 1.75]], F)
    ctx.mboit_resolve(entries, [0, 2, 3], 2, 1, -1.0, 3.0)
    entries.view(np.uint32)[1, 4] = 0xFFFFFFFF
    assert _code(lambda: ctx.mboit_resolve(entries, [0, 2, 3], 2, 1, -1.0, 3.0)) == -1
    # a refused call changes nothing: the getter of the last frame answers as before it
    for mode in (6, 8, 9, 10):
        ctx.render(mode)
        before = GETTERS[mode](ctx)
        assert _code(lambda: _resolves(bad_offsets[0])[mode](ctx)) == -1, mode
        assert _equal(GETTERS[mode](ctx), before), mode
    # a capacity one short of the viewport, then the exact one
    n = c.width * c.height
    a = [np.zeros(n * 16, np.uint64) for _ in range(3)]   # (room for the largest array of any getter: K = 8 slots per pixel)
    p = lambda i: a[i].ctypes.data
    calls = {5: lambda cap: ctx.L.lv_depth_complexity_get_buffers(ctx.h, p(0), cap),
             6: lambda cap: ctx.L.lv_mboit_get_moments(ctx.h, p(0), cap + 4 * n),   # (counted in floats: 1 + N = 5 per pixel)
             8: lambda cap: ctx.L.lv_wboit_get_buffers(ctx.h, p(0), p(1), cap),
             9: lambda cap: ctx.L.lv_depth_peeling_get_buffers(ctx.h, p(0), p(1), p(2), cap),
             10: lambda cap: ctx.L.lv_atomic_loop_get_buffers(ctx.h, p(0), p(1), cap)}
    for mode, call in calls.items():
        ctx.render(mode)
        assert call(n - 1) == -1, mode
        assert call(n) == 0, mode


# ---------------------------------------------------------------- 6. host plugin
def test_host_plugin(hip_lib):
    import ctypes
    from linevis_amd import transfer_function as tfm
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    r = host_api.HeadlessLineRenderer(MODE)
    r.set_rendering_resolution(120, 80)
    r.set_transfer_function(tfm.standard_transparent())
    r.set_line_data(flow)
    assert r.rendering_mode == 9 and r.depth_peeling_state() == {"maxLayers": 2000} and r.wboit_state() is None
    r.set_new_state("Depth Peeling", MODE, {}, resolution=(120, 80))
    frame = r.render_frame()
    assert (frame[..., :3] != 255).any(axis=2).sum() > 100   # (the plugin's default line width: thin lines)
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 9, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frame)

    def layers_of_last_frame():
        accum = np.zeros((80, 120, 4), np.float32)
        layers = np.zeros((80, 120), np.uint32)
        counts = np.zeros((80, 120), np.uint32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert capi.load().lv_depth_peeling_get_buffers(ctypes.c_void_p(hctx), vp(accum), vp(layers), vp(counts), 120 * 80) == 0
        return layers

    full = layers_of_last_frame()
    assert full.max() >= 2
    r.set_new_settings({"depth_peeling_max_layers": "1"})
    assert r.depth_peeling_state() == {"maxLayers": 1}
    other = r.render_frame()
    one = layers_of_last_frame()
    assert one.max() == 1 and np.array_equal(one, np.minimum(full, 1))   # the plugin's key reached the kernels
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 9, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, other) and not np.array_equal(other, frame)
    r.set_new_settings({"depth_peeling_max_layers": "5000"})   # refused by the C ABI: the cap stays
    assert r.depth_peeling_state() == {"maxLayers": 1}
