"""The main loop of the RTAO sample kernel (k_ao_rays) at the smallest shapes where its cycle -- leaf enqueue, retire, ballots, test
phase, refill hand-over, descend stint, drain -- can go wrong.  The loop's wave-level state (queue chunk, FIFO head / tail, the
scheduling decisions) lives on the scalar unit; these cases pin down what it computes.

Every AO image is compared bit for bit with brute force over all primitives on the same rays: the CPU oracle's render_ao / bake_ao
with use_bvh=False generates the rays from the same G-buffer arithmetic and tests each against every capsule / triangle / tubelet
(the library has no brute-force mode of its own).  There is no tolerance to choose: the same float32 operations in the same order, any
differing bit is a defect.

Shapes: launches of 1, 63, 64, 65 and 129 AO rays (a partial batch, a drain that starts at once, hand-over with fewer busy lanes than
LV_HANDOVER_MAX_BUSY), spp 1 / 3 / 64 (per-ray and per-pixel generation), every primitive instantiation, the any-hit path, the bake
instantiation on two-vertex lines, >= 64 lanes meeting a leaf in one node step (a full FIFO: a leaf survives in `cur` into the next
pass), an empty scene and a viewport without a hit pixel."""
import numpy as np
import pytest

from common import Case, scene_arrays
from linevis_amd import capi, scenes, transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LW = 0.03
W, H = 96, 64
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
            use_jittered_primary_rays=False)
GEOMETRIES = ["capsules", "capsules_literal", "triangle_pairs", "triangle_records"]
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bundle():
    """10 helices x 31 points = 300 segments (AO rays meet the neighbouring strands) and their 6-gon triangle tubes."""
    if "tr" not in _cache:
        tr = scenes.normalize(scenes.helix_bundle(n_lines=10, points_per_line=31, seed=5, turns=1.5))
        _cache["tr"] = tr
        _cache["mesh"] = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)
    return _cache["tr"], _cache["mesh"]


def mesh_of(geometry, tr_mesh):
    """triangle_records: the triangles in shuffled order share no vertices inside a leaf, the build keeps 48-byte records."""
    idx, verts, pts = tr_mesh
    if geometry == "triangle_records":
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)
        idx = idx[np.random.default_rng(4).permutation(len(idx))]
    return idx, verts, pts


class Setup:
    """A context, and the oracle's brute-force AO image of a tile of the same case."""

    def __init__(self, geometry, tr=None, mesh=None, width=W, height=H, **settings):
        if tr is None:
            tr, mesh = bundle()
        pts, seg = scene_arrays(tr, LW)
        tri = geometry.startswith("triangle")
        s = dict(RTAO, rtao_geometry="triangle_tubes" if tri else "capsules",
                 intersection_form="closest_approach" if geometry == "capsules" else "literal")
        s.update(settings)
        self.case = Case(pts, seg, tfm.standard(), width, height, LW, **s)
        self.ctx = self.case.hip_context()
        self.tri = None
        if tri:
            m = mesh_of(geometry, mesh)
            self.ctx.set_tube_triangle_mesh(*m)
            self.tri = lvo.TriScene(*m, LW)
        self.scene = self.case.oracle_scene()

    def set(self, key, value):
        self.case.settings[key] = value
        self.ctx.set_option(key, value)

    def check(self, tile):
        """Renders the tile; returns (hit pixels, occluded pixels) after comparing the tile's AO with brute force bit for bit."""
        self.ctx.render(capi.MODE_RAY_TRACER, tile=tile)
        got = self.ctx.get_ao()
        hits = int(self.ctx.stats().ao_hit_pixels)
        P = self.case.oracle_params(self.scene)
        ref = (self.tri or self.scene).render_ao(P, tile=tile, use_bvh=False)
        x0, y0, w, h = tile
        crop = (slice(y0, y0 + h), slice(x0, x0 + w))
        diff = bits(got[crop]) != bits(ref[crop])
        assert not diff.any(), "AO differs from brute force in %d of %d pixels of tile %r" % (int(diff.sum()), w * h, tile)
        return hits, int((ref[crop] < 1.0).sum())


def rects_with(mask, count):
    """Rectangles (x0, y0, w, h) of at most 32 x 16 pixels that hold exactly `count` set pixels of mask, smallest first."""
    ii = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), np.int64)
    ii[1:, 1:] = mask.astype(np.int64).cumsum(0).cumsum(1)
    for h in range(1, 17):
        for w in range(1, 33):
            if w * h < count:
                continue
            s = ii[h:, w:] - ii[:-h, w:] - ii[h:, :-w] + ii[:-h, :-w]
            ys, xs = np.nonzero(s == count)
            for y, x in list(zip(ys, xs))[:2]:
                yield int(x), int(y), w, h


def hit_mask(setup):
    """The pixels whose primary ray (pixel centres: use_jittered_primary_rays off) hits: what the frame colours."""
    setup.ctx.set_option("ambient_occlusion_samples_per_frame", 1)
    img = setup.ctx.render(capi.MODE_RAY_TRACER)
    assert int(setup.ctx.stats().ao_hit_pixels) > 300
    return (img[..., :3] != 255).any(axis=-1)


def check_hit_count(setup, mask, want):
    """A viewport of a few pixels with exactly `want` hit pixels (counted by the library, the frame only proposes rectangles)."""
    for slack in range(0, 4):
        for tile in rects_with(mask, want + slack):
            hits, occluded = setup.check(tile)
            if hits == want:
                return occluded
    raise AssertionError("no viewport with %d hit pixels" % want)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_small_launches_equal_brute_force(hip_lib, geometry):
    s = Setup(geometry)
    mask = hit_mask(s)
    if geometry.startswith("triangle"):
        assert s.ctx.stats().tri_leaf_bytes == (96 if geometry == "triangle_records" else 64)
    occluded = 0
    # (spp, hit pixels): 1, 63, 64, 65 and 129 rays per ray and per pixel, and 3 x 21 = 63, 3 x 43 = 129, 64 x 2 = 128 + a general viewport
    for spp, counts in ((1, (1, 63, 64, 65, 129)), (3, (21, 43)), (64, (1, 2, 9))):
        s.set("ambient_occlusion_samples_per_frame", spp)
        for want in counts:
            occluded += check_hit_count(s, mask, want)
    assert occluded > 40           # the rays do meet the neighbouring strands


@pytest.mark.parametrize("geometry", ["capsules", "triangle_pairs"])
def test_any_hit_path_and_a_viewport_without_hits(hip_lib, geometry):
    """ambient_occlusion_distance_based off: the ANY_HIT instantiation ends a ray at its first hit (samples 0 / 1)."""
    s = Setup(geometry, ambient_occlusion_distance_based=False)
    mask = hit_mask(s)
    occluded = 0
    for spp, counts in ((1, (1, 64, 65)), (3, (43,)), (64, (2,))):
        s.set("ambient_occlusion_samples_per_frame", spp)
        for want in counts:
            occluded += check_hit_count(s, mask, want)
    assert occluded > 10
    assert check_hit_count(s, mask, 0) == 0            # no hit pixel: no AO ray, the launch ends at once
    s.ctx.render(capi.MODE_RAY_TRACER, tile=next(rects_with(mask, 0)))
    assert int(s.ctx.stats().ao_hit_pixels) == 0


def test_full_frame_with_a_partial_last_chunk(hip_lib):
    """The whole 96 x 64 frame at spp 3 (per ray) and 64 (per pixel): refills, retirements and the drain of many waves."""
    for geometry in ("capsules", "triangle_pairs"):
        s = Setup(geometry)
        for spp in (3, 64):
            s.set("ambient_occlusion_samples_per_frame", spp)
            hits, occluded = s.check((0, 0, W, H))
            assert hits > 300 and occluded > 200


def coincident_tubes(n=80):
    """n copies of one short tube and a single tube beside them, 0.05 apart (inside the AO radius of 0.1)."""
    a, b = np.array([-0.2, 0.0, 0.0], np.float32), np.array([0.2, 0.0, 0.0], np.float32)
    off = np.array([0.0, 0.05, 0.0], np.float32)
    lines = [np.stack([a, b])] * n + [np.stack([a + off, b + off])]
    tr = scenes._pack(lines, [np.linspace(0.0, 1.0, 2, dtype=np.float32)] * len(lines))
    return tr, lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, LW, 6)


@pytest.mark.parametrize("geometry", ["capsules", "triangle_pairs"])
def test_full_fifo_keeps_a_leaf_for_the_next_pass(hip_lib, geometry):
    """80 coincident tubes: the 64 AO rays of a pixel walk the same boxes in step, so a whole wave meets a leaf in one node step while
    pairs still wait -- the FIFO is full and the leaves popped behind them wait in `cur` for the pass after the test phase."""
    tr, mesh = coincident_tubes()
    s = Setup(geometry, tr=tr, mesh=mesh, ambient_occlusion_samples_per_frame=64)
    tile = (W // 2 - 4, H // 2 - 4, 8, 8)
    hits, occluded = s.check(tile)
    assert hits >= 8 and occluded >= 8
    s.set("ambient_occlusion_samples_per_frame", 3)
    s.check(tile)


def test_elliptic_tubelets(hip_lib):
    tr = scenes.twisted_ribbons(scenes.normalize(scenes.helix_bundle(n_lines=5, points_per_line=60, seed=3, turns=2.0)), twist=8.0)
    bw = 0.05
    pts, seg, _ = lvo.build_tube_aabb_render_data_ribbons(tr.positions, tr.attributes, tr.line_offsets, bw, tr.ribbon_directions)
    case = Case(pts, seg, tfm.standard(), W, H, 0.02, use_ribbons=True, use_analytic_elliptic_tubes=True, band_width=bw,
                min_band_thickness=0.3, ambient_occlusion_radius=0.15, **RTAO)
    ctx, sc = case.hip_context(), case.oracle_scene()
    occluded = 0
    for spp, tile in ((1, (40, 24, 9, 7)), (3, (30, 20, 13, 5)), (64, (44, 28, 3, 3)), (3, (0, 0, W, H))):
        case.settings["ambient_occlusion_samples_per_frame"] = spp
        ctx.set_option("ambient_occlusion_samples_per_frame", spp)
        ctx.render(capi.MODE_RAY_TRACER, tile=tile)
        ref = sc.render_ao(case.oracle_params(sc), tile=tile, use_bvh=False)
        crop = (slice(tile[1], tile[1] + tile[3]), slice(tile[0], tile[0] + tile[2]))
        assert np.array_equal(bits(ctx.get_ao()[crop]), bits(ref[crop])), (spp, tile)
        occluded += int((ref[crop] < 1.0).sum())
    assert occluded > 100


@pytest.mark.parametrize("distance_based", [True, False])
def test_bake_on_two_vertex_lines(hip_lib, distance_based):
    """The BAKE instantiation: 7 parallel two-vertex lines 0.04 apart, 2 parametrisation vertices each x 5 subdivisions x 3 samples =
    210 rays (three full batches and a partial one, drained at once), reduced by k_ao_reduce<true>."""
    a, b = np.array([-0.3, 0.0, 0.0], np.float32), np.array([0.3, 0.0, 0.0], np.float32)
    lines = [np.stack([a, b]) + np.array([0.0, 0.04 * i, 0.01 * (i % 2)], np.float32) for i in range(7)]
    tr = scenes._pack(lines, [np.linspace(0.0, 1.0, 2, dtype=np.float32)] * len(lines))
    lw, n_sub, spp, its = 0.02, 5, 3, 2
    mesh = lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, lw, 6)
    bw, sl = lvo.ao_parametrization(tr.positions, tr.line_offsets, 1.0)
    pts, seg = scene_arrays(tr, lw)
    case = Case(pts, seg, tfm.standard(), W, H, lw, ambient_occlusion_mode="RTAO (Prebaker)", ambient_occlusion_strength=1.0,
                rtao_prebaker_iterations=its, rtao_prebaker_samples_per_frame=spp, rtao_prebaker_num_tube_subdivisions=n_sub,
                ambient_occlusion_distance_based=distance_based)
    ctx = case.hip_context()
    ctx.set_tube_triangle_mesh(*mesh)
    ctx.set_ao_parametrization(bw, sl)
    got = ctx.get_baked_ao(n_sub)
    ref = lvo.bake_ao(case.oracle_scene(), lvo.TriScene(*mesh, lw), lw, sl, n_sub, spp, its, use_distance=distance_based, use_bvh=False)
    assert got.shape == ref.shape == (len(sl), n_sub)
    assert np.array_equal(bits(got), bits(ref))
    assert float(ref.min()) < 1.0


def test_empty_scene(hip_lib):
    case = Case(np.zeros(0, dtype=lvo.LINE_POINT_DTYPE), np.zeros((0, 2), np.uint32), tfm.standard(), 40, 24, 0.01,
                ambient_occlusion_samples_per_frame=64, **RTAO)
    ctx = case.hip_context()
    img = ctx.render(capi.MODE_RAY_TRACER)
    assert int(ctx.stats().ao_hit_pixels) == 0
    assert (img[..., :3] == 255).all() and np.array_equal(bits(ctx.get_ao()), bits(np.ones((24, 40), np.float32)))
