"""The RTAO sample kernel's bookkeeping (k_ao_rays): per-pixel ray generation (ao_ray_generation), the 32-bit hit key and the
hardware reciprocal of the node steps must not move a bit of the AO image.

Scene: a short helix bundle (10 lines x 31 points = 300 segments, line width 0.03: AO rays meet the neighbouring strands), 96 x 64
pixels = one full 64 x 64 group plus a partial one, so a chunk of rays crosses a group boundary of the compacted pixel list.
per_pixel and per_ray are compared bit for bit (both are the same float32 operations in the same order: any difference is a defect,
there is no tolerance to choose); the oracle comparisons are the bit-for-bit ones of the existing parity tests."""
import numpy as np
import pytest

from common import Case, scene_arrays
from linevis_amd import capi, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LW = 0.03
W, H = 96, 64
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bundle():
    if "tr" not in _cache:
        _cache["tr"] = scenes.normalize(scenes.helix_bundle(n_lines=10, points_per_line=31, seed=5, turns=1.5))
        _cache["mesh"] = lvo.build_tube_triangle_render_data(_cache["tr"].positions, _cache["tr"].attributes, _cache["tr"].line_offsets, LW, 6)
    return _cache["tr"], _cache["mesh"]


def case_of(width=W, height=H, **settings):
    tr, _ = bundle()
    pts, seg = scene_arrays(tr, LW)
    return Case(pts, seg, tfm.standard(), width, height, LW, **RTAO, **settings)


def context(case):
    ctx = case.hip_context()
    if case.settings.get("rtao_geometry") == "triangle_tubes":
        ctx.set_tube_triangle_mesh(*bundle()[1])
    return ctx


def render_both(ctx, tile=None):
    """(frame, AO image, hit pixels) under ao_ray_generation = per_ray and per_pixel, same context."""
    out = {}
    for gen in ("per_ray", "per_pixel"):
        ctx.set_option("ao_ray_generation", gen)
        img = ctx.render(capi.MODE_RAY_TRACER, tile=tile)
        out[gen] = (img.copy(), ctx.get_ao().copy(), int(ctx.stats().ao_hit_pixels))
    return out["per_ray"], out["per_pixel"]


def assert_same(a, b):
    assert a[2] == b[2]
    assert np.array_equal(bits(a[1]), bits(b[1])), "AO images differ in %d pixels" % int((bits(a[1]) != bits(b[1])).sum())
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("geometry", ["capsules", "triangle_tubes"])
@pytest.mark.parametrize("distance_based", [True, False])
@pytest.mark.parametrize("form", ["literal", "closest_approach"])
def test_per_pixel_equals_per_ray(hip_lib, geometry, distance_based, form):
    case = case_of(rtao_geometry=geometry, ambient_occlusion_distance_based=distance_based, intersection_form=form,
                   ambient_occlusion_samples_per_frame=64)
    ctx = context(case)
    for spp in (64, 128, 192):
        ctx.set_option("ambient_occlusion_samples_per_frame", spp)
        a, b = render_both(ctx)
        assert_same(a, b)
        assert a[2] > 300 and (a[1] < 1.0).sum() > 200     # the AO rays do meet the neighbouring strands


@pytest.mark.parametrize("geometry", ["capsules", "triangle_tubes"])
def test_fallback_sample_counts_and_the_oracle(hip_lib, geometry):
    """spp 4 / 48 / 65 take the per-ray code under both option values; at spp 64 both paths give the oracle's AO (brute force over all
    primitives) on a crop that holds the boundary between the two 64 x 64 groups."""
    case = case_of(rtao_geometry=geometry, ambient_occlusion_samples_per_frame=64)
    ctx = context(case)
    for spp in (4, 48, 65):
        ctx.set_option("ambient_occlusion_samples_per_frame", spp)
        a, b = render_both(ctx)
        assert_same(a, b)
    ctx.set_option("ambient_occlusion_samples_per_frame", 64)
    a, b = render_both(ctx)
    assert_same(a, b)
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    x0, y0, w, h = 48, 16, 32, 24
    if geometry == "triangle_tubes":
        ref = lvo.TriScene(*bundle()[1], LW).render_ao(P, tile=(x0, y0, w, h), use_bvh=False)
    else:
        ref = sc.render_ao(P, tile=(x0, y0, w, h), use_bvh=False)
    crop = (slice(y0, y0 + h), slice(x0, x0 + w))
    assert (ref[crop] < 1.0).sum() > 50
    for got in (a, b):
        assert np.array_equal(bits(got[1][crop]), bits(ref[crop]))


def _rect_with(mask, count):
    """(x0, y0, w, h), w <= 16, h <= 8, whose pixels hold exactly `count` set pixels of mask."""
    ii = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), np.int64)
    ii[1:, 1:] = mask.astype(np.int64).cumsum(0).cumsum(1)
    for h in (8, 4, 2, 1, 6, 3, 5, 7):
        for w in (16, 8, 12, 4, 2, 1, 10, 14, 6, 3, 5, 7, 9, 11, 13, 15):
            s = ii[h:, w:] - ii[:-h, w:] - ii[h:, :-w] + ii[:-h, :-w]
            ys, xs = np.nonzero(s == count)
            if len(ys):
                return int(xs[0]), int(ys[0]), w, h
    raise AssertionError("no rectangle with %d hit pixels" % count)


def test_edge_pixel_counts(hip_lib):
    """Launches of 0, 1, 63, 64 and 65 hit pixels (spp 64: 0 rays, one small chunk, a last partial chunk of the large size, a drain that
    starts at once): each terminates with the per-ray path's image."""
    # primary rays of the RTAO pass through the pixel centres, like the colour pass' (1 spp): the pixels the frame colours are the pixels
    # the RTAO pass hits, which lets the frame propose the rectangles
    case = case_of(rtao_geometry="capsules", ambient_occlusion_samples_per_frame=64, use_jittered_primary_rays=False)
    ctx = context(case)
    ctx.set_option("ao_ray_generation", "per_ray")
    img = ctx.render(capi.MODE_RAY_TRACER)
    hit = (ctx.get_ao() < 1.0) | (img[..., :3] != 255).any(axis=-1)
    # hit pixels of a rectangle: counted by the library itself below; the images only propose rectangles
    full_hits = int(ctx.stats().ao_hit_pixels)
    assert full_hits > 300
    found = set()
    for want in (0, 1, 63, 64, 65):
        for slack in range(0, 6):     # should a hit pixel be neither occluded nor coloured: try rectangles with a few less
            if want - slack < 0:
                break
            tile = _rect_with(hit, want - slack)
            a, b = render_both(ctx, tile=tile)
            assert_same(a, b)
            found.add(a[2])
            if a[2] == want:
                break
    assert {0, 1, 63, 64, 65} <= found, sorted(found)


def _edge_rays(seed=3):
    rng = np.random.default_rng(seed)
    n_rand = 4096
    o = rng.uniform(-0.4, 0.4, (n_rand, 3)).astype(np.float32)
    d = rng.normal(size=(n_rand, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    den = np.array([1e-40, -1e-40, 2.0 ** -127, -(2.0 ** -127), 2.0 ** -149, 1.1e-38], np.float32)   # denormals both sides of 2^-128
    assert ((den != 0) & (np.abs(den) < np.finfo(np.float32).tiny)).all()
    special = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = np.zeros(3, np.float32)
            e[axis] = sign
            special.append(e.copy())                              # +-1 with the others +0
            e2 = e.copy(); e2[(axis + 1) % 3] = -0.0; e2[(axis + 2) % 3] = -0.0
            special.append(e2)                                    # ... with the others -0
            for k in den:
                e3 = e.copy(); e3[(axis + 1) % 3] = k
                special.append(e3)                                # ... one denormal component
                e4 = e.copy(); e4[(axis + 1) % 3] = k; e4[(axis + 2) % 3] = -k
                special.append(e4)
    # a zero / -0 / denormal component in otherwise general directions
    for k in (0.0, -0.0, 1e-40, -1e-40):
        g = d[:96].copy()
        g[:32, 0] = k; g[32:64, 1] = k; g[64:, 2] = k
        special.extend(g)
    special = np.array(special, np.float32)
    # every special direction from many origins: segment end points (rays that graze / start inside boxes) and random points
    tr, _ = bundle()
    pts, _seg = scene_arrays(tr, LW)
    ends = np.asarray(pts["linePosition"], np.float32)
    reps = 24
    so = np.concatenate([ends[rng.integers(0, len(ends), len(special) * (reps // 2))],
                         rng.uniform(-0.4, 0.4, (len(special) * (reps - reps // 2), 3)).astype(np.float32)])
    sd = np.tile(special, (reps, 1))
    so[: len(so) // 3] -= sd[: len(so) // 3] * np.float32(0.2)   # start behind the point, look at it
    return np.concatenate([so, o]), np.concatenate([sd, d])


@pytest.mark.parametrize("geometry", ["capsules", "capsules_literal", "triangle_tubes"])
def test_hardware_reciprocal_traversal_equals_brute_force(hip_lib, geometry):
    """lv_traversal_inv under arbitrary rays (traversal_reciprocal = hardware puts the ray-trace entry points on the reciprocals that
    k_ao_rays descends with): direction components 0, -0 and denormal, +-1 with the others 0, and 4096 random rays against brute force
    over the 300 segments / 3480 triangles -- t and primitive bit for bit, as for the IEEE reciprocals."""
    case = case_of(rtao_geometry="triangle_tubes" if geometry == "triangle_tubes" else "capsules",
                   intersection_form="literal" if geometry == "capsules_literal" else "closest_approach")
    ctx = context(case)
    o, d = _edge_rays()
    hits = 0
    for recip in ("hardware", "ieee"):
        ctx.set_option("traversal_reciprocal", recip)
        for tmin, tmax in ((0.0, 0.1), (1e-4, 1000.0)):
            if geometry == "triangle_tubes":
                a = ctx.trace_rays_triangles(o, d, tmin, tmax)
                b = lvo.TriScene(*bundle()[1], LW).trace_rays(o, d, tmin, tmax, use_bvh=False)
            else:
                lvo.set_default_intersection_form(case.literal_form())
                a = ctx.trace_rays(o, d, tmin, tmax)
                b = case.oracle_scene().trace_rays(o, d, tmin, tmax, LW, use_bvh=False)
            assert np.array_equal(a[1], b[1]), (recip, tmin, int((a[1] != b[1]).sum()))
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))
            hits += int((a[1] != 0xFFFFFFFF).sum())
    assert hits > 2000


def test_two_iterations_change_the_frame_number(hip_lib):
    """ambient_occlusion_iterations = 2: the second iteration's seeds carry frame number 1 (lv_tea(pixel, frame * spp + sample)) and the
    running mean mixes it into the first -- per_pixel must reproduce both."""
    case = case_of(rtao_geometry="capsules", ambient_occlusion_samples_per_frame=64)
    ctx = context(case)
    one = render_both(ctx)
    ctx.set_option("ambient_occlusion_iterations", 2)
    two = render_both(ctx)
    assert_same(*one)
    assert_same(*two)
    assert not np.array_equal(bits(one[0][1]), bits(two[0][1]))
