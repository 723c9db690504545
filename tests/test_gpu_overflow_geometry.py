"""The traversal-stack slab against every launch geometry of a frame that differs from the colour pass'.

lv_frame_render reserves the global part of the traversal stacks once, for all launches of the frame, from the same statement of
their geometry the launches use (lv_ao_geometry).  The deep-tree tests of test_gpu_parity / test_gpu_context_reuse render a full
frame without halo, denoiser or tile list, where the RTAO pass has the colour pass' geometry.  Here the chain scene of
test_deep_lbvh_uses_stack_overflow_slab (a plain LBVH higher than the LDS-staged stacks) is rendered at 128 x 128 as four 64 x 64
tiles with 2 RTAO samples per pixel: the colour pass has 64 blocks (a grid of 128), the RTAO pass on tiles dilated by a 1- or
2-pixel halo 256, its ray kernel fewer than that, the paired launch 384 -- the tile grids size the slab, each differently.  Every
case asserts a relation the suite already asserts on shallow scenes, and prints the context's device memory after its frames.
"""
import numpy as np
import pytest

import test_svgf
from common import Case, max_lsb_diff
from linevis_amd import tiling, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LSB_TOL = 2  # north_star: "+-2 LSB per RGBA8 channel"
SIZE, TILE = 128, 64
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
            ambient_occlusion_samples_per_frame=2)
EAW = dict(ambient_occlusion_denoiser="EAW", eaw_denoiser_iterations=1)   # reads 2 pixels around every pixel it filters


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def chain_case(**settings):
    """test_deep_lbvh_uses_stack_overflow_slab's scene: segment k sits on axis k % 3 at distance 2^-(k // 3 + 1), so every split of
    the plain LBVH (accel_build = fast_build) peels off a single leaf and the tree is a ~50-level chain"""
    pts, seg = [], []
    for k in range(54):
        a = np.zeros(3)
        a[k % 3] = 0.9 * 2.0 ** (-(k // 3 + 1))
        b = a.copy()
        b[(k + 1) % 3] += 0.3 * 2.0 ** (-(k // 3 + 1))
        seg.append([len(pts), len(pts) + 1])
        pts += [a, b]
    P = np.zeros(len(pts), dtype=lvo.LINE_POINT_DTYPE)
    P["linePosition"] = np.array(pts, dtype=np.float32)
    P["lineTangent"] = [1, 0, 0]
    P["lineNormal"] = [0, 1, 0]
    P["lineAttribute"] = np.linspace(0, 1, len(pts))
    return Case(P, np.array(seg, np.uint32), tfm.standard_transparent(), SIZE, SIZE, 0.0004, camera_pos=(0.3, 0.3, 0.9),
                accel_build="fast_build", **dict(RTAO, **settings))


def deep_context(c):
    ctx = c.hip_context()
    ctx.build_accel()
    assert ctx.stats().bvh_depth > 32   # 3 * ceil(h / 2) + 2 stack entries: more than the LDS-staged part of every kernel
    return ctx


def render_tiles(ctx, mode):
    """the frame as four 64 x 64 tiles of one tile list"""
    import torch
    tiles = tiling.make_tiles(SIZE, SIZE, TILE)
    assert len(tiles) == 4
    out = torch.zeros((len(tiles), TILE, TILE, 4), dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.render_tiles_device(out.data_ptr(), tiles, TILE, TILE, mode=mode)
    torch.cuda.synchronize()
    ctx.set_stream(None)
    return tiling.detile(out.cpu().numpy(), tiles, SIZE, SIZE, TILE)


def report(name, ctx):
    print("device_bytes %s: %d" % (name, ctx.stats().device_bytes))


@pytest.mark.parametrize("name,mode,settings", [
    pytest.param("jittered", 11, dict(num_samples_per_frame=2), id="jittered"),   # bilinear AO lookup: 1-pixel halo, tiles of 66 x 66
    pytest.param("eaw", 11, EAW, id="eaw"),                                       # 2-pixel halo, tiles of 68 x 68
    pytest.param("eaw_ppll", 2, EAW, id="eaw_ppll"),
])
def test_halo_tiles_on_a_deep_tree(hip_lib, name, mode, settings):
    """as test_tile_list_equals_full_frame and test_deep_lbvh_uses_stack_overflow_slab: the tiled frame is the full frame bit for bit,
    the AO image has the oracle's bits, the colour is within 2 LSB"""
    c = chain_case(**settings)
    ctx = deep_context(c)
    full = ctx.render(mode)
    ao_full = ctx.get_ao()
    tiled = render_tiles(ctx, mode)
    ao_tiled = ctx.get_ao()
    report(name, ctx)
    ref, ao_ref = c.oracle_render(mode)
    print("%s: AO max |hip - oracle| full %.3g tiled %.3g, differing words %d / %d, colour %d LSB" % (
        name, np.abs(ao_full - ao_ref).max(), np.abs(ao_tiled - ao_ref).max(), int((bits(ao_full) != bits(ao_ref)).sum()),
        int((bits(ao_tiled) != bits(ao_ref)).sum()), max_lsb_diff(full, ref)))
    assert np.array_equal(tiled, full)
    assert np.array_equal(bits(ao_full), bits(ao_ref)) and np.array_equal(bits(ao_tiled), bits(ao_ref))
    assert max_lsb_diff(full, ref) <= LSB_TOL
    assert (full != full[0, 0]).any()   # the chain is in the picture (tubes far thinner than a pixel: a handful of pixels)
    ctx.close()


@pytest.mark.parametrize("name,settings", [pytest.param("pair", dict(), id="pair"), pytest.param("pair_eaw", EAW, id="pair_eaw")])
def test_paired_primaries_on_a_deep_tree(hip_lib, name, settings):
    """as test_overlap_primary_passes_gives_the_same_frames: k_primary_pair (one launch and one slab for the RTAO primaries' workgroups
    and the colour rays') against the two launches, on the four tiles, one sample per pixel: frames and AO images byte for byte"""
    c = chain_case(**settings)
    got = {}
    for on in (True, False):
        ctx = deep_context(c)
        ctx.set_option("overlap_primary_passes", on)
        got[on] = (render_tiles(ctx, 11), ctx.get_ao())
        report("%s %s" % (name, "on" if on else "off"), ctx)
        ctx.close()
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(bits(got[True][1]), bits(got[False][1]))
    assert (got[True][0] != got[True][0][0, 0]).any()


def test_svgf_viewport_pass_behind_one_tile_on_a_deep_tree(hip_lib):
    """as test_svgf_tiles_share_the_full_frame_history: the RTAO pass and the denoiser cover the whole viewport while one 64 x 48 tile
    is rendered; two frames of a context that only renders the tile are the crops of a context's that renders everything"""
    c = chain_case(ambient_occlusion_denoiser="SVGF", ambient_occlusion_radius=0.3, ambient_occlusion_distance_based=True)
    ctx = deep_context(c)          # (test_svgf.run_sequence builds its own contexts from the same case)
    ctx.render(11, tile=(37, 21, 64, 48))
    report("svgf", ctx)
    ctx.close()
    tile = (37, 21, 64, 48)
    poses = [(0.3, 0.3, 0.9), (0.31, 0.3, 0.9)]   # the view of the deep-tree test, then a small step: the history is reprojected
    full = test_svgf.run_sequence(c, poses)
    part = test_svgf.run_sequence(c, poses, tile=tile)
    x0, y0, w, h = tile
    for (img, ao, _, _), (timg, tao, tref, _) in zip(full, part):
        assert np.array_equal(timg, img[y0:y0 + h, x0:x0 + w])
        assert np.array_equal(tao, ao)
        assert max_lsb_diff(timg, tref) <= LSB_TOL
    assert (full[-1][0] != full[-1][0][0, 0]).any()
