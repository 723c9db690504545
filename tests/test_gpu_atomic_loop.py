"""Rendering mode 10 (Atomic Loop 64) on the GPU, byte for byte against al64_fold (test_atomic_loop_restatement.py): given key lists
with all lanes racing, whole frames against the fold of the oracle's prism fragments, band data and helicity bands, K, tile lists,
deep tails, buffers shared with the other modes, errors and the host plugin.  Every sum is an integer and lv_exp_det / lv_log_det
are bit-identical on host and device, so 0 LSB is derived; max_lsb_diff <= 2 stands in front of the equality to size a failure.
"Band data and helicity bands" here are the (any, band data) and (6, helicity) instances of k_stream_pass only;
test_gpu_oit_instances.py holds all eight, at odd viewports and PPLL tile sizes."""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, host_api, scenes
from test_atomic_loop_restatement import EMPTY, F, al64_fold, al64_key, random_runs
from test_gpu_mlab import RTAO, _stacked_case
from test_mlab_restatement import pack, window_depth

pytestmark = pytest.mark.gpu
BG = (0.1, 0.2, 0.3, 1.0)
MODE = capi.MODE_ATOMIC_LOOP_64


def _code(f):
    with pytest.raises(capi.LineVisError) as e:
        f()
    return e.value.code


def _flat(runs):
    offsets = np.zeros(len(runs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in runs])
    return (np.concatenate(runs) if int(offsets[-1]) else np.zeros(0, np.uint64)), offsets


def _same(img, ref):
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


# ---------------------------------------------------------------- 1. given lists
@pytest.mark.parametrize("K", [1, 3, 8, 64])
def test_given_lists_bit_for_bit(hip_lib, K):
    rng = np.random.default_rng(K)
    w, h = 37, 11
    runs = random_runs(rng, w * h, K)
    deep = al64_key(rng.random(5000).astype(F), rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32))
    deep[1000:2000] = deep[0]   # whole waves with one key on one address
    runs[5] = deep
    c = small_case(width=16, height=16, n_lines=2, pts_per_line=4)
    ctx = c.hip_context()
    ctx.set_background(BG)
    ctx.set_option("atomic_loop_num_layers", K)
    keys, off = _flat(runs)
    img, slots, tail = ctx.atomic_loop_resolve(keys, off, w, h)
    ref, ref_slots, ref_tail = al64_fold(runs, K, BG)
    slots = slots.reshape(-1, K)
    live = slots != EMPTY
    assert np.all(slots[:, :-1] <= slots[:, 1:]) and np.all(live[:, :-1] | ~live[:, 1:])   # ascending, empty slots last
    assert np.array_equal(slots, ref_slots)
    assert np.array_equal(tail.reshape(-1, 5), ref_tail)
    _same(img.reshape(-1, 4), ref)
    assert _code(lambda: ctx.atomic_loop_resolve(np.array([EMPTY]), np.array([0, 1], np.uint64), 1, 1)) == -1   # the empty word


# ---------------------------------------------------------------- 2. whole frames
def frame_runs(c, ao=None):
    """the keys of the oracle's prism fragments past the discard, one array per pixel: straight packed colour, window depth from
    their positions"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P, ao=ao)
    rgba = fr["rgba"]
    keep = rgba[:, 3] >= F(0.001)
    key = al64_key(window_depth(fr["pos"], c.view, c.proj), pack([rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]]))
    off = fr["offsets"].astype(np.int64)
    return [key[off[p]:off[p + 1]][keep[off[p]:off[p + 1]]] for p in range(c.width * c.height)]


def frame_reference(c, K, ao=None, runs=None):
    """al64_fold of frame_runs.  Returns (frame, slots, tail sums, fragments past the discard, pixels with a tail)"""
    runs = runs if runs is not None else frame_runs(c, ao)
    img, slots, tail = al64_fold(runs, K, c.background)
    shape = (c.height, c.width)
    return (img.reshape(shape + (4,)), slots.reshape(shape + (K,)), tail.reshape(shape + (5,)), sum(len(r) for r in runs),
            int((tail[:, 0] != 0).sum()))


@functools.lru_cache(maxsize=None)
def _small():
    return small_case(width=120, height=80, transparent=True)


@functools.lru_cache(maxsize=None)
def _larger():
    return small_case(width=256, height=144, n_lines=60, pts_per_line=60, line_width=0.015, transparent=True)


@functools.lru_cache(maxsize=None)
def _larger_runs():
    return frame_runs(_larger())   # (computed once for the tests that share the scene)


def _larger_reference(K):
    return frame_reference(_larger(), K, runs=_larger_runs())


def _frame_checks(c, K, ref):
    ctx = c.hip_context()
    ctx.set_option("atomic_loop_num_layers", K)
    img = ctx.render(MODE)
    want, slots, tail, n, tail_pixels = ref if ref is not None else frame_reference(c, K, ao=ctx.get_ao().copy())
    _same(img, want)
    got_slots, got_tail = ctx.atomic_loop_buffers()
    assert np.array_equal(got_slots, slots) and np.array_equal(got_tail, tail)
    assert int(ctx.stats().fragments) == n
    assert np.array_equal(ctx.render(MODE), img)   # a second render gives the same bytes
    return n, tail_pixels


@pytest.mark.parametrize("K", [1, 2, 8])
def test_frame_matches_the_fold_of_the_oracle_fragments(hip_lib, K):
    c = _small()
    n, tail_pixels = _frame_checks(c, K, frame_reference(c, K))
    assert n == 2339
    assert tail_pixels >= {1: 400, 2: 50, 8: 0}[K]
    if K == 8:
        assert tail_pixels == 0   # (deepest pixel: 6 fragments)


def test_larger_frame_matches_the_fold(hip_lib):
    n, tail_pixels = _frame_checks(_larger(), 4, _larger_reference(4))
    assert n == 21271 and tail_pixels >= 500


def test_frame_with_rtao_and_depth_cues(hip_lib):
    c = small_case(width=120, height=80, transparent=True, depth_cue_strength=0.8, **RTAO)
    n, tail_pixels = _frame_checks(c, 2, None)
    assert n > 500 and tail_pixels >= 50


# ---------------------------------------------------------------- 3. band data and rotating helicity bands
def _band_frame(c):
    n, tail_pixels = _frame_checks(c, 2, frame_reference(c, 2))
    assert n > 200 and tail_pixels > 0


def test_frame_with_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    _band_frame(band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8))


def test_frame_with_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    _band_frame(helicity_case(width=120, height=90, transparent=True)[0])


# ---------------------------------------------------------------- 4. K
def test_k_is_honoured(hip_lib):
    c = _larger()   # deepest pixel: 11 fragments
    ctx = c.hip_context()
    imgs = {}
    for K in (2, 8, 16, 64):
        ctx.set_option("atomic_loop_num_layers", K)
        imgs[K] = ctx.render(MODE)
    assert np.array_equal(imgs[16], imgs[64])
    assert not np.array_equal(imgs[2], imgs[8])
    _same(imgs[16], _larger_reference(16)[0])


# ---------------------------------------------------------------- 5. tile lists
def _tiles(ctx, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=MODE)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_tile_lists_reassemble_the_frame(hip_lib):
    c = _larger()
    ctx = c.hip_context()
    ctx.set_option("atomic_loop_num_layers", 4)
    img = ctx.render(MODE)
    _same(img, _larger_reference(4)[0])
    tw = th = 32
    grid = [(x, y) for y in range(0, c.height, th) for x in range(0, c.width, tw)]
    tiles = np.array(grid, dtype=np.uint32)
    out = np.zeros_like(img)
    for r in range(4):
        mine = tiles[r::4]
        b = _tiles(ctx, mine, tw, th)
        for i, (x, y) in enumerate(mine):
            out[y:y + th, x:x + tw] = b[i][:min(th, c.height - y), :min(tw, c.width - x)]
    assert np.array_equal(out, img)
    assert _code(ctx.atomic_loop_buffers) == -3   # the last frame was a tile list that leaves pixels out
    # every tile twice and overlapping ones on top: the same pixels
    tiles = np.array(grid * 2 + [(16, 16), (48, 16), (16, 48), (100, 70), (200, 100)], dtype=np.uint32)
    b = _tiles(ctx, tiles, tw, th)
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)


# ---------------------------------------------------------------- 6. deep tails
def test_deep_tails(hip_lib):
    c = _stacked_case()
    ctx = c.hip_context()
    for K in (8, 64):
        ctx.set_option("atomic_loop_num_layers", K)
        img = ctx.render(MODE)
        want, _, _, n, tail_pixels = frame_reference(c, K)
        assert tail_pixels > 0
        _same(img, want)
        st = ctx.stats()
        assert int(st.fragments) == n and st.max_depth_complexity > 1000 and int(st.ppll_pool_nodes) == 0


# ---------------------------------------------------------------- 7. shared buffers
def test_buffers_shared_with_the_other_modes(hip_lib):
    c = _small()
    streamed = {"mboit_fragment_storage": "streamed"}
    fresh = {}
    for mode in (2, 3, 6, MODE):
        ctx = c.hip_context()
        ctx.set_options(streamed)
        fresh[mode] = ctx.render(mode)
    ctx = c.hip_context()
    ctx.set_options(streamed)
    for mode in (2, MODE, 3, MODE, 6, MODE):
        assert np.array_equal(ctx.render(mode), fresh[mode]), mode


# ---------------------------------------------------------------- 8. errors
def test_errors(hip_lib):
    c = _small()
    ctx = c.hip_context()
    ctx.set_option("atomic_loop_num_layers", 2)
    base = ctx.render(MODE)
    for bad in ("0", "65", "-1", "x"):
        assert _code(lambda: ctx.set_option("atomic_loop_num_layers", bad)) == -1, bad
    assert np.array_equal(ctx.render(MODE), base)   # the old value stays
    assert ctx.atomic_loop_buffers()[0].shape == (c.height, c.width, 2)
    ctx.set_option("atomic_loop_num_layers", 8)   # the buffers keep the frame's K, whatever the option says since
    assert ctx.atomic_loop_buffers()[0].shape == (c.height, c.width, 2)
    ctx.set_option("atomic_loop_num_layers", 2)
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto")):
        ctx.set_option(key, value)
        assert _code(lambda: ctx.render(MODE)) == -1, key
        ctx.set_option(key, back)
        assert np.array_equal(ctx.render(MODE), base)
    # (this pair is refused by the frame's general check for every mode; mode 10 only has to pass the refusal on and stay usable)
    ctx.set_options({"use_ribbons": True, "rotating_helicity_bands": True})
    assert _code(lambda: ctx.render(MODE)) == -1
    ctx.set_options({"use_ribbons": False, "rotating_helicity_bands": False})
    assert np.array_equal(ctx.render(MODE), base)
    for mode in (7, 0, 4):
        assert _code(lambda: ctx.render(mode)) == -1, mode
    # the buffers belong to a mode-10 frame over the whole viewport
    ctx.render(2)
    assert _code(ctx.atomic_loop_buffers) == -3
    ctx.render(MODE)
    slots = np.zeros((c.height, c.width, 2), np.uint64)
    tail = np.zeros((c.height, c.width, 5), np.uint64)
    p = lambda a: a.ctypes.data
    assert ctx.L.lv_atomic_loop_get_buffers(ctx.h, p(slots), p(tail), c.width * c.height - 1) == -1   # too small
    assert ctx.L.lv_atomic_loop_get_buffers(ctx.h, p(slots), p(tail), c.width * c.height) == 0
    assert ctx.L.lv_atomic_loop_get_buffers(ctx.h, None, p(tail), c.width * c.height) == -1


# ---------------------------------------------------------------- 9. host plugin
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
    assert r.rendering_mode == 10 and r.atomic_loop_state() == {"numLayers": 8} and r.mlab_state() is None
    r.set_new_state("Atomic Loop 64 (4 Layers)", MODE, {"numLayers": 4}, resolution=(120, 80))
    assert r.atomic_loop_state() == {"numLayers": 4}
    frame = r.render_frame()
    assert (frame[..., :3] != 255).any(axis=2).sum() > 100   # (the plugin's default line width: thin lines)
    hctx = r.L.lvh_renderer_context(r.h)
    assert hctx
    raw = np.empty((80, 120, 4), dtype=np.uint8)
    rc = capi.load().lv_render(ctypes.c_void_p(hctx), 10, 0, 0, 120, 80, raw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and np.array_equal(raw, frame)
    r.set_new_settings({"atomic_loop_num_layers": 1})
    assert r.atomic_loop_state() == {"numLayers": 1}
    r.set_new_settings({"atomic_loop_num_layers": 65})   # refused by the C ABI: numLayers stays
    assert r.atomic_loop_state() == {"numLayers": 1}
    multi = plugin(devices=[0])   # a one-rank lv_create_multi
    multi.set_new_state("Atomic Loop 64 (4 Layers)", MODE, {"numLayers": 4}, resolution=(120, 80))
    assert np.array_equal(multi.render_frame(), frame)
