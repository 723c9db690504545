"""The spatial-hashing denoiser on the GPU (linevis_amd/csrc/lv_sh.hip) against its restatement (tests/sh_restatement.py): given
maps bit for bit, probing in a 16-cell map, the overflow invariants, persistence and the clears, and the denoiser inside a frame."""
import numpy as np
import pytest

import sh_restatement as sh
from common import small_case
from linevis_amd import capi, tiling
from test_eaw import eaw_numpy

W, H = 24, 16
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_gamma=1.0,
            ambient_occlusion_radius=0.1, ambient_occlusion_distance_based=True, use_jittered_primary_rays=True,
            ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=4)
SH = "Spatial Hashing"


@pytest.fixture(scope="module")
def maps():
    noisy, normal, position = sh.given_maps(W, H)
    hits = int(np.count_nonzero(np.any(normal[:, :, :3] != 0.0, axis=2)))
    return noisy, normal, position, hits


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = capi.Context(0)
    yield c
    c.close()


def tail(read, normal, position):
    """three EAWDenoise.Compute passes with the denoiser's fixed settings, in float64"""
    return eaw_numpy(read, normal, position, 3, 0.49, float(np.float32(0.3) * np.float32(0.000001)), float(np.float32(0.1)),
                     False, True, True, True)


def device_cells(ctx, which=1):
    keys, sums, counts = ctx.spatial_hashing_cells(which)
    return {(int(k), int(s), int(c)) for k, s, c in zip(keys, sums, counts)}


@pytest.mark.gpu
def test_given_maps_bit_for_bit(ctx, maps):
    noisy, normal, position, hits = maps
    ctx.set_option("spatial_hashing_num_cells", 65536)
    ctx.spatial_hashing_reset(1)
    P = sh.Params(sh.CAMERAS[0], H, num_cells=65536)
    assert len({sh.log_step(P, position[y, x, :3]) for y in range(H) for x in range(W) if normal[y, x, :3].any()}) >= 3
    cells = {}
    want = sh.denoise(P, cells, noisy, normal, position)
    read, out = ctx.spatial_hashing_denoise(noisy, normal, position, sh.CAMERAS[0])
    st = ctx.spatial_hashing_stats(1)
    assert st["dropped"] == 0 and st["stored"] == 4 * hits and st["occupied"] == len(cells) and st["clears"] == 0
    assert np.array_equal(read.view(np.uint32), want.view(np.uint32))
    assert (read[7:9] == 0.0).all()
    assert device_cells(ctx) == sh.cells_as_set(cells)
    ref = tail(want, normal, position)
    assert np.abs(out - ref).max() < 2e-5
    assert np.abs(ref - want).max() > 1e-3          # the tail did blend the close plane's neighbours


@pytest.mark.gpu
def test_probing_and_wrap_in_a_map_of_16_cells(ctx):
    noisy = np.linspace(0.0, 1.0, W * H, dtype=np.float32).reshape(H, W)
    normal = np.zeros((H, W, 4), dtype=np.float32)
    position = np.zeros((H, W, 4), dtype=np.float32)
    normal[2:5, 3:20, :3] = (0.0, 0.6, -0.8)
    position[2:5, 3:20, :3] = (0.25, -0.125, -0.5)           # one point: four keys
    normal[9:12, 1:9, :3] = (-1.0, 0.0, 0.0)
    position[9:12, 1:9, :3] = (-0.4, 0.3, -2.5)              # another, farther away: four more
    P = sh.Params(sh.CAMERAS[0], H, num_cells=16)
    cells = {}
    want = sh.denoise(P, cells, noisy, normal, position)
    assert 4 < len(cells) <= 10                               # ten keys cannot fill anyone's ten-slot window: nothing is dropped
    assert sh.max_occupied_run(list(cells), 16) is not None
    ctx.set_option("spatial_hashing_num_cells", 16)
    read, out = ctx.spatial_hashing_denoise(noisy, normal, position, sh.CAMERAS[0])
    st = ctx.spatial_hashing_stats(1)
    assert st["dropped"] == 0 and st["occupied"] == len(cells)
    assert np.array_equal(read.view(np.uint32), want.view(np.uint32))
    assert device_cells(ctx) == sh.cells_as_set(cells)
    assert np.abs(out - tail(want, normal, position)).max() < 2e-5


@pytest.mark.gpu
def test_overflow_drops_and_counts(ctx, maps):
    noisy, normal, position, hits = maps
    P = sh.Params(sh.CAMERAS[0], H, num_cells=12)
    cells = {}
    sh.denoise(P, cells, noisy, normal, position)
    assert len(cells) >= 40
    ctx.set_option("spatial_hashing_num_cells", 12)
    read, out = ctx.spatial_hashing_denoise(noisy, normal, position, sh.CAMERAS[0])
    st = ctx.spatial_hashing_stats(1)
    got = device_cells(ctx)
    assert st["dropped"] > 0 and st["stored"] + st["dropped"] == 4 * hits
    assert sum(c for _, _, c in got) == st["stored"] and sum(s for _, s, _ in got) <= 100 * st["stored"]
    assert len(got) == st["occupied"] <= 12
    assert {k for k, _, _ in got} <= set(cells)
    for img in (read, out):
        assert np.isfinite(img).all() and (img >= 0.0).all() and (img <= 1.0).all()


@pytest.mark.gpu
def test_persistence_reset_and_the_half_full_clear(ctx, maps):
    noisy, normal, position, hits = maps
    cams = (sh.CAMERAS[0], sh.CAMERAS[1], sh.CAMERAS[0])
    frames = [noisy, (noisy * np.float32(0.5)).astype(np.float32), (1.0 - noisy).astype(np.float32)]
    moved = position.copy()
    moved[9:, :, 0] += np.float32(0.37)                  # the third call sees the far plane elsewhere: cells of its own
    places = [position, position, moved]
    # the keys after two and after three calls, to size the map: at most half full before the third call, more than half after it, and
    # no run of ten occupied slots -- no schedule drops anything
    probe, sizes = {}, []
    for cam, img, pos in zip(cams, frames, places):
        sh.denoise(sh.Params(cam, H), probe, img, normal, pos)
        sizes.append(len(probe))
    n2, n3 = sizes[1], sizes[2]
    num_cells = next(n for n in range(2 * n3 - 1, 2 * n2 - 1, -1) if (sh.max_occupied_run(list(probe), n) or n) < sh.PROBES)
    assert n2 <= num_cells // 2 < n3
    ctx.set_option("spatial_hashing_num_cells", num_cells)
    first, _ = ctx.spatial_hashing_denoise(frames[0], normal, position, cams[0])
    ctx.spatial_hashing_reset(1)
    assert ctx.spatial_hashing_stats(1)["occupied"] == 0 and device_cells(ctx) == set()
    cells = {}
    for i, (cam, img, pos) in enumerate(zip(cams, frames, places)):
        want = sh.denoise(sh.Params(cam, H, num_cells=num_cells), cells, img, normal, pos)
        read, out = ctx.spatial_hashing_denoise(img, normal, pos, cam)
        assert np.array_equal(read.view(np.uint32), want.view(np.uint32)), i
        assert np.abs(out - tail(want, normal, pos)).max() < 2e-5, i
        if i == 0:
            assert np.array_equal(read, first)                       # after the reset the first call's output returns
    st = ctx.spatial_hashing_stats(1)
    assert st == dict(st, dropped=0, stored=12 * hits, occupied=n3, clears=0)
    assert device_cells(ctx) == sh.cells_as_set(cells)
    # the fourth call meets a map that is more than half full: it starts from an empty one
    read, _ = ctx.spatial_hashing_denoise(frames[0], normal, position, cams[0])
    st = ctx.spatial_hashing_stats(1)
    assert st["clears"] == 1 and st["stored"] == 4 * hits and st["dropped"] == 0
    assert np.array_equal(read, first)


def frame_case(**kw):
    return small_case(width=64, height=48, n_lines=20, pts_per_line=20, line_width=0.03, **dict(RTAO, **kw))


def tube_mesh(c):
    from test_gpu_triangle_tubes import mesh_of
    from linevis_amd import scenes
    return mesh_of(scenes.normalize(scenes.random_curves(n_lines=20, points_per_line=20, seed=7)), c.line_width)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", ["capsules", "triangle_tubes"])
def test_in_a_frame_the_map_holds_the_raw_iteration(hip_lib, geometry):
    c = frame_case(rtao_geometry=geometry)
    a = c.hip_context()
    b = c.hip_context()
    if geometry == "triangle_tubes":
        mesh = tube_mesh(c)
        a.set_tube_triangle_mesh(*mesh)
        b.set_tube_triangle_mesh(*mesh)
    b.set_option("ambient_occlusion_denoiser", SH)
    img_a = a.render(11)
    raw = a.get_ao()
    hits = a.stats().ao_hit_pixels
    img_b = b.render(11)
    ao_b = b.get_ao()
    keys, sums, counts = b.spatial_hashing_cells(0)
    st = b.spatial_hashing_stats(0)
    assert 0 < hits < 64 * 48 and st["dropped"] == 0 and st["stored"] == 4 * hits and st["occupied"] == len(keys)
    assert int(counts.sum()) == 4 * hits
    # the sum over A's hit pixels = the sum over all pixels minus the misses', whose raw AO is exactly 1 (the RTAO pass writes 1 there)
    q = np.floor(raw.astype(np.float32) * np.float32(100.0) + np.float32(0.5)).astype(np.int64)
    assert int(sums.sum()) == 4 * (int(q.sum()) - 100 * (64 * 48 - hits))
    assert not np.array_equal(img_a, img_b)
    # 0 on the misses: no more than `hits` pixels are non-zero
    assert int(np.count_nonzero(ao_b)) <= hits and int(np.count_nonzero(ao_b == 0.0)) >= 64 * 48 - hits
    assert (ao_b >= 0.0).all() and (ao_b <= 1.0).all() and np.abs(ao_b - raw)[raw < 1.0].max() > 1e-3
    assert len(b.kernel_times(capi.KERNEL_SH_WRITE)) == 1 and len(b.kernel_times(capi.KERNEL_SH_READ)) == 1 and \
        len(b.kernel_times(capi.KERNEL_SH_TAIL)) == 1 and len(a.kernel_times(capi.KERNEL_SH_WRITE)) == 0
    a.close(); b.close()


@pytest.mark.gpu
def test_tiles_rectangles_ranks_and_long_lived_contexts_reproduce_the_frame(hip_lib):
    import torch
    c = frame_case(ambient_occlusion_denoiser=SH)
    ctx = c.hip_context()
    full = [ctx.render(11), ctx.render(11)]                      # the second frame reads what the first one stored
    ao1 = ctx.get_ao()
    assert not np.array_equal(full[0], full[1])
    # a sub-rectangle and a tile list, each from a fresh context: the RTAO pass and the map cover the viewport whatever is drawn
    part = c.hip_context()
    assert np.array_equal(part.render(11, tile=(13, 9, 30, 20)), full[0][9:29, 13:43])
    assert np.array_equal(part.render(11, tile=(5, 20, 40, 17)), full[1][20:37, 5:45])
    assert np.array_equal(part.get_ao(), ao1)
    part.close()
    tiled = c.hip_context()
    tiles = tiling.make_tiles(64, 48, 16)
    fn = tiling.hip_render_tiles_fn(tiled, 11)
    for want in full:
        out = torch.zeros((len(tiles), 16, 16, 4), dtype=torch.uint8, device="cuda")
        fn(out, tiles, 16, 16)
        torch.cuda.synchronize()
        assert np.array_equal(tiling.detile(out.cpu().numpy(), tiles, 64, 48, 16), want)
    tiled.set_stream(None)
    tiled.close()
    multi = capi.Context(devices=[0, 0, 0], transport="memcpy")
    multi.set_lines(c.points, c.seg)
    multi.set_transfer_function(c.tf, 0.0, 1.0)
    multi.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
    multi.set_background(c.background)
    multi.set_option("line_width", c.line_width)
    multi.set_options(c.settings)
    assert np.array_equal(multi.render(11), full[0]) and np.array_equal(multi.render(11), full[1])
    multi.close()
    # a long-lived context after a reset = a fresh map at the same frame counter
    ctx.spatial_hashing_reset(0)
    third = ctx.render(11)
    other = frame_case().hip_context()                           # no denoiser for two frames: only the RTAO seed counter advances
    other.render(11); other.render(11)
    other.set_option("ambient_occlusion_denoiser", SH)
    assert np.array_equal(other.render(11), third)
    # lv_set_lines empties the map and restarts the counter: the first frame again
    ctx.set_lines(c.points, c.seg)
    assert np.array_equal(ctx.render(11), full[0])
    # back to no denoiser: the raw image, exactly
    raw_ctx = frame_case().hip_context()
    raw_ctx.render(11)
    ctx.set_option("ambient_occlusion_denoiser", "None")
    ctx.set_lines(c.points, c.seg)
    ctx.render(11)
    assert np.array_equal(ctx.get_ao(), raw_ctx.get_ao())
    assert ctx.spatial_hashing_stats(0)["occupied"] == 0         # the map left with the denoiser
    for x in (ctx, other, raw_ctx):
        x.close()


@pytest.mark.gpu
def test_option_errors_leave_the_old_values_drawing(hip_lib):
    c = frame_case(ambient_occlusion_denoiser=SH)
    ctx = c.hip_context()
    want = ctx.render(11)
    for key, val in (("spatial_hashing_atomics_mode", "Float Atomic Add"), ("spatial_hashing_atomics_mode", "Uint Spinning Atomic Add"),
                     ("spatial_hashing_atomics_mode", "No Atomics"), ("spatial_hashing_atomics_mode", "Some Atomics"),
                     ("spatial_hashing_s_p", 0.05), ("spatial_hashing_s_p", 20.5), ("spatial_hashing_s_min_exp", 0),
                     ("spatial_hashing_s_min_exp", -21), ("spatial_hashing_s_nd", 0.5), ("spatial_hashing_s_nd", 11),
                     ("spatial_hashing_num_cells", 9), ("ambient_occlusion_denoiser", "OptiX Denoiser")):
        with pytest.raises(capi.LineVisError) as e:
            ctx.set_option(key, val)
        if key == "ambient_occlusion_denoiser":
            assert "Spatial Hashing" in str(e.value)
        if val in ("Float Atomic Add", "No Atomics"):
            assert "execution order" in str(e.value)
    ctx.set_option("spatial_hashing_atomics_mode", "Uint Quantized Atomic Add")
    ctx.set_lines(c.points, c.seg)
    assert np.array_equal(ctx.render(11), want)                  # the refused values changed nothing
    ctx.set_options(dict(spatial_hashing_s_p=2.0, spatial_hashing_s_min_exp=-5, spatial_hashing_s_nd=5, spatial_hashing_num_cells=4096))
    ctx.set_lines(c.points, c.seg)
    assert not np.array_equal(ctx.render(11), want)
    st = ctx.spatial_hashing_stats(0)
    assert st["stored"] + st["dropped"] == 4 * ctx.stats().ao_hit_pixels and st["occupied"] <= 4096
    ctx.close()
