"""Rendering mode 6 with mboit_fragment_storage = streamed (k_mboit_stream_pass twice + k_mboit_stream_blend: no fragment pool):
frames and lv_mboit_get_moments bit for bit against mboit_fold on the oracle's prism fragments and against the pooled frame of
the same context -- every shading variant, general cameras, tile lists, the host plugin, a two-rank handle --; no pool and no
regrowth; more than 65534 fragments on a pixel; the limit of 131071; options, errors and context reuse.  No tolerance anywhere:
the sums are integers."""
import numpy as np
import pytest

from common import Case, small_case
from linevis_amd import capi, host_api, scenes
from oracle import lvo
from test_gpu_mboit import FRAME_BIAS, compares_something, frame_reference, variant_case
from test_mboit_restatement import U32

pytestmark = pytest.mark.gpu


def _streamed(ctx, on=True):
    ctx.set_option("mboit_fragment_storage", "streamed" if on else "pool")
    return ctx


def _code(call):
    with pytest.raises(capi.LineVisError) as e:
        call()
    return e.value.code


# ---------------------------------------------------------------- 1. frames and moments against the statement
@pytest.mark.parametrize("variant", ["plain", "rtao_depthcue", "larger"])
def test_frame_and_moments_match_the_statement(hip_lib, variant):
    c = variant_case(variant)
    c.settings["collect_stats"] = True
    ctx = _streamed(c.hip_context())
    bias = None if variant == "plain" else FRAME_BIAS
    ctx.set_option("mboit_moment_bias", bias or "auto")
    ao = None
    for N in ((4, 6, 8) if variant == "plain" else (4,)):
        ctx.set_option("mboit_num_moments", N)
        img = ctx.render(6)
        got = ctx.mboit_moments()
        st = ctx.stats()
        if variant == "rtao_depthcue":
            ao = ctx.get_ao().copy()
        ref, n, mom, deg = frame_reference(c, N, ao=ao, bias=bias)
        compares_something(c, ref, n, mom)
        assert np.array_equal(img, ref)
        assert got.shape == (c.height, c.width, 1 + N)
        assert np.array_equal(got.reshape(mom.shape).view(U32), mom.view(U32))
        assert int(st.fragments) == n
        assert int(st.mboit_degenerate_pixels) == deg
        assert int(st.ppll_pool_nodes) == 0
        assert np.array_equal(ctx.render(6), img)   # two streamed renders in a row
        _streamed(ctx, False)
        assert np.array_equal(ctx.render(6), img)   # the same context, pooled
        _streamed(ctx)


# ---------------------------------------------------------------- 2. shading variants and general cameras
def _streamed_pooled_statement(c, Ns=(4,), statement=True):
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    for N in Ns:
        ctx.set_option("mboit_num_moments", N)
        pooled = _streamed(ctx, False).render(6)
        img = _streamed(ctx).render(6)
        assert (pooled != pooled[0, 0]).any(axis=2).sum() > 100
        assert np.array_equal(img, pooled)
        if statement:
            ref, n, mom, _ = frame_reference(c, N, bias=FRAME_BIAS)
            compares_something(c, ref, n, mom)
            assert np.array_equal(img, ref)
            assert np.array_equal(ctx.mboit_moments().reshape(mom.shape).view(U32), mom.view(U32))
    ctx.close()


def test_band_data(hip_lib):
    from test_gpu_elliptic import band_case
    _streamed_pooled_statement(band_case(width=120, height=90, transparent=True, use_capped_tubes=False, tube_num_subdivisions=8))


def test_rotating_helicity_bands(hip_lib):
    from test_gpu_helicity_bands import helicity_case
    _streamed_pooled_statement(helicity_case(width=120, height=90, transparent=True)[0])


def test_fast_shading_numerics(hip_lib):
    """shading_numerics = fast selects the approximate fragment stage in both storages: equal frames.  (Nothing is asserted against
    the exact frame: the fast colour differs from it by at most 1 LSB on a few pixels in a million, DESIGN.md 4, and on a frame of
    this size usually on none.)"""
    c = small_case(width=120, height=80, transparent=True)
    c.settings["shading_numerics"] = "fast"
    _streamed_pooled_statement(c, statement=False)


@pytest.mark.parametrize("cam", ["roll37", "lens_shift", "inside_rolled"])
def test_general_cameras(hip_lib, cam):
    from test_gpu_cameras import cam_case
    _streamed_pooled_statement(cam_case(cam, seed=17, n_lines=40, pts_per_line=30, line_width=0.02, transparent=True), Ns=(4, 8))


# ---------------------------------------------------------------- 3. tile lists
def _tiles_against_whole(ctx, c, img, tiles, tw, th):
    import torch
    buf = torch.empty((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), tiles, tw, th, mode=6)
    ctx.stats()   # synchronises (and reads the frame's overflow flag)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    for i, (x, y) in enumerate(tiles):
        hh, ww = min(th, c.height - y), min(tw, c.width - x)
        assert np.array_equal(b[i][:hh, :ww], img[y:y + hh, x:x + ww]), (i, x, y)


def test_four_rank_deal_of_tiles(hip_lib):
    c = small_case(width=128, height=96, n_lines=40, pts_per_line=40, transparent=True)
    ctx = c.hip_context()
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    pooled = ctx.render(6)
    img = _streamed(ctx).render(6)
    assert (img != 255).any(axis=2).sum() > 500 and np.array_equal(img, pooled)
    tiles = np.array([(x, y) for y in range(0, c.height, 32) for x in range(0, c.width, 32)], dtype=np.uint32)
    for r in range(4):
        _tiles_against_whole(ctx, c, img, tiles[r::4], 32, 32)
    assert _code(ctx.mboit_moments) == -3   # the last frame did not cover the viewport


def test_repeated_and_overlapping_tiles_with_long_runs(hip_lib):
    from test_gpu_mlab import _stacked_case
    c = _stacked_case(collect_stats=True)
    ctx = c.hip_context()
    pooled = ctx.render(6)
    img = _streamed(ctx).render(6)
    assert ctx.stats().max_depth_complexity > 1000 and np.array_equal(img, pooled)
    grid = [(x, y) for y in range(0, c.height, 16) for x in range(0, c.width, 16)]
    tiles = np.array(grid * 8 + [(8, 8), (24, 8), (8, 16), (24, 24), (16, 16)], dtype=np.uint32)
    _tiles_against_whole(ctx, c, img, tiles, 16, 16)


# ---------------------------------------------------------------- 4. no pool, no regrowth
def test_no_pool_and_no_regrowth(hip_lib):
    from test_gpu_mlab import _stacked_case
    c = _stacked_case(ppll_expected_avg_depth_complexity=1, collect_stats=True)
    ctx = _streamed(c.hip_context())
    img = ctx.render(6)
    st = ctx.stats()
    ref, nfr, mom, deg = frame_reference(c, 4)
    compares_something(c, ref, nfr, mom)
    assert np.array_equal(img, ref)
    assert int(st.ppll_pool_nodes) == 0
    pooled = c.hip_context()
    assert np.array_equal(pooled.render(6), img)
    sp = pooled.stats()
    for f in ("fragments", "rays_traced", "prims_tested", "hits_shaded", "max_depth_complexity", "mboit_degenerate_pixels"):
        assert getattr(st, f) == getattr(sp, f), (f, getattr(st, f), getattr(sp, f))
        assert getattr(st, f) > 0 or f == "mboit_degenerate_pixels", f
    assert int(st.fragments) == nfr and int(st.mboit_degenerate_pixels) == deg
    assert 0 < int(st.device_bytes) < int(sp.device_bytes)


# ---------------------------------------------------------------- 5 / 6. more fragments on a pixel than the pooled count holds
def _tall_stack(n, width=12, height=8, line_width=0.2, **settings):
    """_stacked_case's construction with tubes wider than a pixel of a small viewport: n parallel segments along the view axis
    through the same pixels, one prism front face per segment and pixel"""
    rng = np.random.default_rng(5)
    x0 = (-0.02 + 0.0005 * rng.random(n)).astype(np.float32)
    z = (-0.9 + 1.8 * np.arange(n) / n).astype(np.float32)
    pos = np.empty((2 * n, 3), np.float32)
    pos[0::2] = np.stack([x0, np.full(n, -0.3, np.float32), z], axis=1)
    pos[1::2] = np.stack([x0 + np.float32(0.04), np.full(n, 0.3, np.float32), z], axis=1)
    attr = rng.random(2 * n).astype(np.float32)
    pts, seg, _ = lvo.build_tube_aabb_render_data(pos, attr, np.arange(0, 2 * n + 1, 2, dtype=np.uint32), line_width)
    from linevis_amd import transfer_function as tfm
    return Case(pts, seg, tfm.standard_transparent(), width, height, line_width, **settings)


def test_more_than_65534_fragments_on_a_pixel(hip_lib):
    c = _tall_stack(90000, collect_stats=True)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    longest = int(np.diff(sc.prism_fragments(P, ao=None)["offsets"].astype(np.int64)).max())
    assert 66000 < longest < 120000, longest
    ctx = c.hip_context()
    assert _code(lambda: ctx.render(6)) == -4   # pooled: the 16-bit per-pixel count
    img = _streamed(ctx).render(6)
    ref, n, mom, deg = frame_reference(c, 4)
    assert (ref != ref[0, 0]).any(axis=2).sum() > 50
    assert np.array_equal(img, ref)
    assert np.array_equal(ctx.mboit_moments().reshape(mom.shape).view(U32), mom.view(U32))
    st = ctx.stats()
    assert int(st.fragments) == n and int(st.max_depth_complexity) == longest and int(st.mboit_degenerate_pixels) == deg


def test_the_limit_of_131071_fragments_on_a_pixel(hip_lib):
    big = _tall_stack(165000)
    ctx = _streamed(big.hip_context())
    assert _code(lambda: ctx.render(6)) == -4
    # the device entry point stays asynchronous: the flag is reported by the next host-synchronous read of that frame
    import torch
    buf = torch.empty((1, big.height, big.width, 4), dtype=torch.uint8, device="cuda")
    ctx.render_tiles_device(buf.data_ptr(), np.zeros((1, 2), np.uint32), big.width, big.height, mode=6)
    assert _code(ctx.stats) == -4
    assert _code(ctx.mboit_moments) == -4
    small = small_case(width=96, height=64, transparent=True)
    ctx.set_lines(small.points, small.seg)
    ctx.set_option("line_width", small.line_width)
    ctx.set_camera(small.view, small.proj, small.fovy, small.near, small.far, small.width, small.height)
    fresh = _streamed(small.hip_context())
    want = fresh.render(6)
    assert (want != want[0, 0]).any(axis=2).sum() > 300
    assert np.array_equal(ctx.render(6), want)
    assert np.array_equal(ctx.mboit_moments().view(U32), fresh.mboit_moments().view(U32))
    ctx.stats()   # a later successful frame clears the flag


# ---------------------------------------------------------------- 7. options and errors
def test_options_and_errors(hip_lib):
    c = small_case(width=96, height=64, n_lines=60, pts_per_line=40, line_width=0.03, transparent=True)
    ctx = _streamed(c.hip_context())
    ctx.set_option("mboit_moment_bias", FRAME_BIAS)
    base = ctx.render(6)
    ref, n, mom, _ = frame_reference(c, 4, bias=FRAME_BIAS)
    compares_something(c, ref, n, mom)
    assert np.array_equal(base, ref)
    for bad in ("", "Pool", "stream", "1"):
        assert _code(lambda: ctx.set_option("mboit_fragment_storage", bad)) == -1, bad
    ctx.render(6)
    assert int(ctx.stats().ppll_pool_nodes) == 0   # still streamed
    for key, value, back in (("ppll_prism_rasteriser", "lbvh", "segments"), ("ppll_fragment_source", "capsule_entry", "auto")):
        ctx.set_option(key, value)
        assert _code(lambda: ctx.render(6)) == -1, key
        ctx.set_option(key, back)
        assert np.array_equal(ctx.render(6), base)
    ctx.set_option("mboit_overestimation", 0.6)
    over = ctx.render(6)
    assert np.array_equal(over, frame_reference(c, 4, over=0.6, bias=FRAME_BIAS)[0]) and not np.array_equal(over, base)
    ctx.set_option("mboit_overestimation", 0.1)
    ctx.set_option("mboit_moment_bias", 5e-3)
    biased = ctx.render(6)
    assert np.array_equal(biased, frame_reference(c, 4, bias=5e-3)[0]) and not np.array_equal(biased, base)
    ctx.set_option("mboit_moment_bias", "auto")
    ctx.set_option("mboit_num_moments", 8)
    assert np.array_equal(ctx.render(6), frame_reference(c, 8)[0])
    # the moments belong to a streamed frame
    _streamed(ctx, False).render(6)
    assert _code(ctx.mboit_moments) == -3
    _streamed(ctx).render(6)
    ctx.mboit_moments()
    ctx.render(2)
    assert _code(ctx.mboit_moments) == -3
    # isolation: after a streamed frame, modes 2 and 3 render what fresh contexts render
    fresh2, fresh3 = c.hip_context().render(2), c.hip_context().render(3)
    ctx.render(6)
    assert np.array_equal(ctx.render(2), fresh2)
    ctx.render(6)
    assert np.array_equal(ctx.render(3), fresh3)


def test_switching_the_storage_gives_a_fresh_contexts_frames(hip_lib):
    """pool -> streamed -> pool -> streamed in one context, other moment counts and another scene in between"""
    a = small_case(width=96, height=64, transparent=True)
    b = small_case(width=96, height=64, n_lines=60, pts_per_line=40, line_width=0.03, transparent=True)
    want = {}
    for name, c in (("a", a), ("b", b)):
        for N in (4, 8):
            f = _streamed(c.hip_context())
            f.set_option("mboit_num_moments", N)
            want[name, N] = (f.render(6), f.mboit_moments())
    ctx = a.hip_context()
    for name, c, N, on in (("a", a, 8, False), ("a", a, 8, True), ("b", b, 4, True), ("b", b, 4, False), ("a", a, 4, True),
                           ("b", b, 8, True)):
        ctx.set_lines(c.points, c.seg)
        ctx.set_option("line_width", c.line_width)
        ctx.set_option("mboit_num_moments", N)
        img = _streamed(ctx, on).render(6)
        assert np.array_equal(img, want[name, N][0]), (name, N, on)
        if on:
            assert np.array_equal(ctx.mboit_moments().view(U32), want[name, N][1].view(U32)), (name, N)


# ---------------------------------------------------------------- 8. host plugin
def test_host_plugin_states_with_streamed_storage(hip_lib):
    tr = scenes.normalize(scenes.random_curves(n_lines=30, points_per_line=30, seed=7))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    from linevis_amd import transfer_function as tfm
    frames = {}
    for storage in ("pool", "streamed"):
        r = host_api.HeadlessLineRenderer(capi.MODE_MBOIT)
        r.set_rendering_resolution(120, 80)
        r.set_transfer_function(tfm.standard_transparent())
        r.set_line_data(flow)
        r.set_new_settings({"mboit_fragment_storage": storage})
        frames[storage] = {4: [], 8: []}
        for name, mode, _, settings in host_api.get_test_modes_mboit():
            r.set_new_state(name, mode, settings, resolution=(120, 80))   # (the states do not carry the key: the storage stays)
            frames[storage][int(settings["numMoments"])].append(r.render_frame())
        assert int(r.stats().ppll_pool_nodes > 0) == int(storage == "pool")
    for N in (4, 8):
        assert len(frames["streamed"][N]) == 5
        assert (frames["pool"][N][0] != frames["pool"][N][0][0, 0]).any(axis=2).sum() > 500
        for f in frames["streamed"][N]:
            assert np.array_equal(f, frames["pool"][N][0])
    assert not np.array_equal(frames["streamed"][4][0], frames["streamed"][8][0])


# ---------------------------------------------------------------- 9. two-rank handle
def test_two_rank_handle(hip_lib):
    c = small_case(width=200, height=136, n_lines=40, pts_per_line=40, line_width=0.012, transparent=True)
    want = _streamed(c.hip_context()).render(6)
    assert (want != 255).any(axis=2).sum() > 500
    multi = capi.Context(devices=[0, 0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(c.settings)
    _streamed(multi)
    assert multi.num_ranks == 2
    for _ in range(2):
        assert np.array_equal(multi.render(6), want)
    assert int(multi.stats().ppll_pool_nodes) == 0
    multi.close()
