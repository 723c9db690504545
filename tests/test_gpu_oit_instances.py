"""Every instance of the OIT fragment stage (NT = 6 / any subdivision count x plain / band data / helicity bands, and the two plain
ones again under shading_numerics = fast) in every OIT mode path -- 3, 5, 6 pooled, 6 streamed, 8, 9, 10 -- at odd viewports and at
PPLL tile sizes other than the default, against the folds of the per-mode files (frame_reference of test_gpu_mlab / _mboit / _wboit /
_atomic_loop / _depth_peeling, oracle_counts and depth_complexity_frame for mode 5).

Coverage, guaranteed by `_assert_coverage` over the parameter lists when the module is imported:
  * MATRIX crosses the six test groups (3, 5, 6, 8, 9, 10; the mode-6 group renders pooled AND streamed) with all eight CASES, so
    every (mode path, instance) pair occurs -- the "any" instances of plain tubes and helicity bands with two subdivision counts
    each.  Every knob value of a group (mlab_num_layers 1 / 4, mboit_num_moments 4 / 6 / 8, both wboit_depth_weight,
    atomic_loop_num_layers 1 / 4) runs inside each of its tests, on one context.
  * case i of group j renders at VIEWPORTS[(i + j) % 3] with TILES[(i + j) % 4]: eight consecutive values, so every
    (mode path, viewport) pair of 61x47 / 97x53 / 33x71 and every (mode path, tile size) pair of default (2x8) / 1x1 / 8x8 / 1x8 occurs.
  * RECTS: every mode path and knob value, 97x53, the "any, plain" case: seven rectangles against their part of the whole frame.
  * NARROW: every mode path at 5x67 with the two "any, plain" and the two "any, helicity" cases, one per tile size.
  * FAST: modes 3, 6 (both storages), 8, 9, 10 with the two plain cases at 61x47 and 97x53 under shading_numerics = fast.

Parts 1 to 3 are equalities: every sum is an integer and lv_pow_det / lv_exp_det / lv_log_det are build-owned, so 0 LSB is derived;
max_lsb_diff <= 2 stands in front of the equality to size a failure.  Under `fast` a fragment's {depth, alpha, kept} are the exact
mode's (the comment above lv_shade_prism), so everything that is a function of those alone is still compared bit for bit
with the EXACT fold, and the frame is held to the project's 2 LSB; the measured maxima are printed (DESIGN.md 4 carries them).

What keeps the comparisons from comparing nothing is checked on the oracle alone, without a GPU
(test_the_cases_compare_something): at the three main viewports every case has >= 700 fragments, >= 400 covered pixels and >= 35
pixels with three or more fragments; at 5x67 >= 200 fragments and >= 10 such pixels.  A thin wide strip (129x3) shows 1 to 4
fragments with the default camera, which is why the one-row check is a rectangle of a larger frame and not a viewport of its own."""
import functools

import numpy as np
import pytest

import test_gpu_atomic_loop as al64
import test_gpu_depth_complexity as dcx
import test_gpu_depth_peeling as peel
import test_gpu_mboit as mboit
import test_gpu_mlab as mlab
import test_gpu_wboit as wboit
from common import max_lsb_diff, small_case
from test_depth_peeling_restatement import depth_complexity_frame
from test_wboit_restatement import WEIGHTS

VIEWPORTS = ((61, 47), (97, 53), (33, 71))
TILES = (None, (1, 1), (8, 8), (1, 8))   # ppll_tile_width x ppll_tile_height; None = the default, 2 x 8
NARROW_VIEWPORT = (5, 67)


def _band(**kw):
    from test_gpu_elliptic import band_case
    return band_case(use_capped_tubes=False, **kw)


def _helicity(**kw):
    from test_gpu_helicity_bands import helicity_case
    return helicity_case(**kw)[0]


# name: ((NT, SHADE) instance, constructor, settings)
CASES = {
    "6_plain": (("6", "plain"), small_case, dict(line_width=0.03)),
    "any5_plain": (("any", "plain"), small_case, dict(line_width=0.03, tube_num_subdivisions=5)),
    "any3_plain": (("any", "plain"), small_case, dict(line_width=0.03, tube_num_subdivisions=3)),
    "6_band": (("6", "band data"), _band, dict()),
    "any8_band": (("any", "band data"), _band, dict(tube_num_subdivisions=8)),
    "6_helicity": (("6", "helicity"), _helicity, dict()),
    "any4_helicity": (("any", "helicity"), _helicity, dict(tube_num_subdivisions=4)),
    "any7_helicity": (("any", "helicity"), _helicity, dict(tube_num_subdivisions=7)),
}
INSTANCES = {(nt, shade) for nt in ("6", "any") for shade in ("plain", "band data", "helicity")}
GROUPS = {"m3": ("3",), "m5": ("5",), "m6": ("6 pooled", "6 streamed"), "m8": ("8",), "m9": ("9",), "m10": ("10",)}   # group: mode paths
FAST_GROUPS = ("m3", "m6", "m8", "m9", "m10")
MLAB_LAYERS = (1, 4)
MBOIT_MOMENTS = (4, 6, 8)
AL64_LAYERS = (1, 4)

MATRIX = [(g, name, VIEWPORTS[(i + j) % 3], TILES[(i + j) % 4]) for j, g in enumerate(GROUPS) for i, name in enumerate(CASES)]
RECT_CASE, RECT_VIEWPORT = "any5_plain", (97, 53)
# ragged to the right and bottom edges; the last column; the last pixel; the first row -- the last three lie beside the data of this
# scene (a rectangle that read its neighbours' words would show them) --; then a column, a row and a pixel of 4 fragments inside it
RECTS = ((60, 24, 37, 29), (96, 0, 1, 53), (96, 52, 1, 1), (0, 0, 97, 1), (45, 0, 1, 53), (0, 13, 97, 1), (67, 12, 1, 1))
RECTS_LEAST_COVERED = (50, 0, 0, 0, 25, 30, 1)
NARROW = [(g, name, NARROW_VIEWPORT, tile) for g in GROUPS
          for name, tile in (("any5_plain", None), ("any3_plain", (1, 1)), ("any4_helicity", (8, 8)), ("any7_helicity", (1, 8)))]
FAST = [(g, name, vp) for g in FAST_GROUPS for name in ("6_plain", "any5_plain") for vp in VIEWPORTS[:2]]


def _assert_coverage():
    paths = {p for g in GROUPS for p in GROUPS[g]}
    assert len(paths) == 7 and {CASES[n][0] for n in CASES} == INSTANCES
    seen = {kind: {(p, value) for g, name, vp, tile in MATRIX for p in GROUPS[g]
                   for value in [{"instance": CASES[name][0], "viewport": vp, "tile": tile}[kind]]}
            for kind in ("instance", "viewport", "tile")}
    assert seen["instance"] == {(p, i) for p in paths for i in INSTANCES}
    assert seen["viewport"] == {(p, v) for p in paths for v in VIEWPORTS}
    assert seen["tile"] == {(p, t) for p in paths for t in TILES}
    for n in ("any5_plain", "any3_plain", "any4_helicity", "any7_helicity"):   # both counts of the two doubled "any" instances, every path
        assert {p for g, name, _, _ in MATRIX if name == n for p in GROUPS[g]} == paths
    assert {p for g, _, _, _ in NARROW for p in GROUPS[g]} == paths
    assert {CASES[name][0] for _, name, _, _ in NARROW} == {("any", "plain"), ("any", "helicity")}
    assert {(g, CASES[name][0][0], vp) for g, name, vp in FAST} == {(g, nt, vp) for g in FAST_GROUPS for nt in ("6", "any")
                                                                    for vp in VIEWPORTS[:2]}
    assert all(CASES[name][0][1] == "plain" for _, name, _ in FAST) and CASES[RECT_CASE][0] == ("any", "plain")


_assert_coverage()


def make_case(name, viewport, tile=None, **settings):
    _, make, kw = CASES[name]
    if tile is not None:
        settings.update(ppll_tile_width=tile[0], ppll_tile_height=tile[1])
    return make(width=viewport[0], height=viewport[1], transparent=True, **kw, **settings)


def _id(v):
    return "default" if v is None else "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _same(img, ref):
    assert max_lsb_diff(img, ref) <= 2
    assert np.array_equal(img, ref)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- references: computed once per (mode, case, viewport, knob), never written to
# (the oracle's fragments do not depend on the PPLL tile size: one reference serves every tile size)
@functools.lru_cache(maxsize=None)
def _counts(name, viewport):
    return dcx.oracle_counts(make_case(name, viewport))


@functools.lru_cache(maxsize=None)
def _ref(group, name, viewport, knob=None):
    c = make_case(name, viewport)
    if group == "m3":
        return mlab.frame_reference(c, knob)                              # frame, fragments past the discard
    if group == "m6":
        return mboit.frame_reference(c, knob, bias=mboit.FRAME_BIAS)      # frame, fragments, moments, degenerate pixels
    if group == "m8":
        return wboit.frame_reference(c, knob)                             # frame, fragments, sums, counts
    if group == "m9":
        return peel.frame_reference(c, 2000)                              # frame, fragments, accumulators, layers, counts
    assert group == "m10"
    return al64.frame_reference(c, knob)                                  # frame, slots, tail, fragments past the discard, tail pixels


# ---------------------------------------------------------------- the conditions, on the oracle alone (no GPU)
def test_the_cases_compare_something():
    for name in CASES:
        for vp in VIEWPORTS:
            counts = _counts(name, vp)
            got = (int(counts.sum()), int((counts > 0).sum()), int((counts >= 3).sum()))
            assert got[0] >= 700 and got[1] >= 400 and got[2] >= 35, (name, vp, got)
    for name in sorted({name for _, name, _, _ in NARROW}):
        counts = _counts(name, NARROW_VIEWPORT)
        got = (int(counts.sum()), int((counts >= 3).sum()))
        assert got[0] >= 200 and got[1] >= 10, (name, got)
    counts = _counts(RECT_CASE, RECT_VIEWPORT)
    for (x, y, w, h), least in zip(RECTS, RECTS_LEAST_COVERED):
        assert int((counts[y:y + h, x:x + w] > 0).sum()) >= least, (x, y, w, h)
    assert int(counts[12, 67]) >= 4
    # the folds tell the instances apart: a frame shaded by the plain instance, or built for another subdivision count, is another frame
    vp = VIEWPORTS[0]
    for name, off in (("6_band", dict(use_ribbons=False)), ("any7_helicity", dict(rotating_helicity_bands=False))):
        plain = wboit.frame_reference(make_case(name, vp, **off))
        assert int((plain[2] != _ref("m8", name, vp, "reference")[2]).any(axis=2).sum()) > 100, name
    for a, b in (("6_plain", "any5_plain"), ("any5_plain", "any3_plain"), ("6_band", "any8_band"), ("6_helicity", "any4_helicity"),
                 ("6_helicity", "any7_helicity")):
        assert int((_counts(a, vp) != _counts(b, vp)).sum()) > 20, (a, b)
    strip = dcx.oracle_counts(make_case(RECT_CASE, (129, 3)))
    assert int(strip.sum()) < 10   # why no thin wide viewport stands among the cases


# ---------------------------------------------------------------- per mode: what its own _frame_checks asserts
def _stats(ctx, n, pool, deepest=None):
    st = ctx.stats()
    assert int(st.fragments) == n
    assert (int(st.ppll_pool_nodes) >= n) if pool else (int(st.ppll_pool_nodes) == 0)
    assert deepest is None or int(st.max_depth_complexity) == deepest


def _exact_m3(ctx, name, vp):
    for K in MLAB_LAYERS:
        ctx.set_option("mlab_num_layers", K)
        img = ctx.render(3)
        ref, n = _ref("m3", name, vp, K)
        _same(img, ref)
        _stats(ctx, n, pool=True)   # every fragment past the discard kept, none dropped
        assert np.array_equal(ctx.render(3), img)


def _exact_m5(ctx, name, vp):
    counts = _counts(name, vp)
    c = make_case(name, vp)
    for max_colour in (0, 3):
        ctx.set_option("depth_complexity_max_colour", max_colour)
        img = ctx.render(5)
        _same(img, depth_complexity_frame(counts, c.background, max_colour).reshape(c.height, c.width, 4))
        assert np.array_equal(ctx.depth_complexity_buffers(), counts)
        assert ctx.depth_complexity_stats() == dcx._stats_of(counts)
        _stats(ctx, int(counts.sum()), pool=False, deepest=int(counts.max()))
        assert np.array_equal(ctx.render(5), img)


def _exact_m6(ctx, name, vp):
    counts = _counts(name, vp)
    ctx.set_option("mboit_moment_bias", mboit.FRAME_BIAS)   # (as test_gpu_mboit_streamed.py: nearly every covered pixel shows)
    for N in MBOIT_MOMENTS:
        ctx.set_option("mboit_num_moments", N)
        ref, n, mom, _ = _ref("m6", name, vp, N)
        assert n == int(counts.sum())
        ctx.set_option("mboit_fragment_storage", "pool")
        pooled = ctx.render(6)
        _same(pooled, ref)
        _stats(ctx, n, pool=True, deepest=int(counts.max()))
        assert np.array_equal(ctx.render(6), pooled)
        ctx.set_option("mboit_fragment_storage", "streamed")
        img = ctx.render(6)
        _same(img, ref)
        assert np.array_equal(img, pooled)
        got = ctx.mboit_moments()
        assert got.shape == (vp[1], vp[0], 1 + N)
        assert np.array_equal(_bits(got.reshape(mom.shape)), _bits(mom))
        _stats(ctx, n, pool=False, deepest=int(counts.max()))
        assert np.array_equal(ctx.render(6), img)


def _exact_m8(ctx, name, vp):
    for weight in WEIGHTS:
        ctx.set_option("wboit_depth_weight", weight)
        img = ctx.render(8)
        ref, n, sums, counts = _ref("m8", name, vp, weight)
        _same(img, ref)
        got_sums, got_counts = ctx.wboit_buffers()
        assert np.array_equal(got_counts, counts) and np.array_equal(got_sums, sums)
        _stats(ctx, n, pool=False, deepest=int(counts.max()))
        assert np.array_equal(ctx.render(8), img)


def _exact_m9(ctx, name, vp):
    ctx.set_option("depth_peeling_max_layers", 2000)
    img = ctx.render(9)
    ref, n, accum, layers, counts = _ref("m9", name, vp)
    _same(img, ref)
    got_accum, got_layers, got_counts = ctx.depth_peeling_buffers()
    assert np.array_equal(got_counts, counts) and np.array_equal(got_layers, layers)
    assert np.array_equal(_bits(got_accum), _bits(accum))
    _stats(ctx, n, pool=False, deepest=int(counts.max()))
    assert np.array_equal(ctx.render(9), img)


def _exact_m10(ctx, name, vp):
    for K in AL64_LAYERS:
        ctx.set_option("atomic_loop_num_layers", K)
        img = ctx.render(10)
        ref, slots, tail, n, _ = _ref("m10", name, vp, K)
        _same(img, ref)
        got_slots, got_tail = ctx.atomic_loop_buffers()
        assert np.array_equal(got_slots, slots) and np.array_equal(got_tail, tail)
        _stats(ctx, n, pool=False)
        assert np.array_equal(ctx.render(10), img)


EXACT = {"m3": _exact_m3, "m5": _exact_m5, "m6": _exact_m6, "m8": _exact_m8, "m9": _exact_m9, "m10": _exact_m10}


# ---------------------------------------------------------------- 1. the instance matrix;  3. the narrow viewport
@pytest.mark.gpu
@pytest.mark.parametrize("group,name,viewport,tile", MATRIX + NARROW, ids=lambda v: _id(v))
def test_instance_matches_the_fold(hip_lib, group, name, viewport, tile):
    ctx = make_case(name, viewport, tile).hip_context()
    EXACT[group](ctx, name, viewport)
    ctx.close()


# ---------------------------------------------------------------- 2. ragged rectangles
def _rect_settings(group):
    """(mode, the options of one pass over the rectangles) for every knob value of the group"""
    if group == "m3":
        return [(3, {"mlab_num_layers": K}) for K in MLAB_LAYERS]
    if group == "m5":
        return [(5, {"depth_complexity_max_colour": 3})]   # explicit: in auto a rectangle scales by its own maximum
    if group == "m6":
        return [(6, {"mboit_moment_bias": mboit.FRAME_BIAS, "mboit_num_moments": N, "mboit_fragment_storage": s})
                for N in MBOIT_MOMENTS for s in ("pool", "streamed")]
    if group == "m8":
        return [(8, {"wboit_depth_weight": w}) for w in WEIGHTS]
    if group == "m9":
        return [(9, {})]
    return [(10, {"atomic_loop_num_layers": K}) for K in AL64_LAYERS]


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_ragged_rectangles_equal_their_part_of_the_frame(hip_lib, group):
    ctx = make_case(RECT_CASE, RECT_VIEWPORT).hip_context()
    for mode, options in _rect_settings(group):
        ctx.set_options(options)
        whole = ctx.render(mode)
        assert (whole != whole[0, 0]).any(axis=2).sum() > 200   # (of at least 400 covered pixels)
        for x, y, w, h in RECTS:
            assert np.array_equal(ctx.render(mode, tile=(x, y, w, h)), whole[y:y + h, x:x + w]), (options, x, y, w, h)
        assert np.array_equal(ctx.render(mode), whole)
    ctx.close()


# ---------------------------------------------------------------- 4. shading_numerics = fast against the EXACT fold
def _within_2_lsb(tag, img, ref):
    d = np.abs(img.astype(np.int32) - ref.astype(np.int32)).max(axis=2)
    print("shading_numerics=fast, %s: max %d LSB, %d of %d pixels differ" % (tag, int(d.max()), int((d > 0).sum()), d.size))
    assert int(d.max()) <= 2, tag


def _fast_m3(ctx, name, vp, tag):
    for K in MLAB_LAYERS:
        ctx.set_option("mlab_num_layers", K)
        ref, n = _ref("m3", name, vp, K)
        img = ctx.render(3)
        assert int(ctx.stats().fragments) == n
        _within_2_lsb("%s K=%d" % (tag, K), img, ref)


def _fast_m6(ctx, name, vp, tag):
    ctx.set_option("mboit_moment_bias", mboit.FRAME_BIAS)
    for N in MBOIT_MOMENTS:
        ctx.set_option("mboit_num_moments", N)
        ref, n, mom, _ = _ref("m6", name, vp, N)
        ctx.set_option("mboit_fragment_storage", "pool")
        pooled = ctx.render(6)
        assert int(ctx.stats().fragments) == n
        ctx.set_option("mboit_fragment_storage", "streamed")
        img = ctx.render(6)
        assert int(ctx.stats().fragments) == n
        assert np.array_equal(_bits(ctx.mboit_moments().reshape(mom.shape)), _bits(mom))   # functions of (alpha, depth) alone
        assert np.array_equal(img, pooled)   # the same fast fragment stage in both storages
        _within_2_lsb("%s pooled N=%d" % (tag, N), pooled, ref)
        _within_2_lsb("%s streamed N=%d" % (tag, N), img, ref)


def _fast_m8(ctx, name, vp, tag):
    for weight in WEIGHTS:
        ctx.set_option("wboit_depth_weight", weight)
        ref, n, sums, counts = _ref("m8", name, vp, weight)
        img = ctx.render(8)
        got_sums, got_counts = ctx.wboit_buffers()
        assert np.array_equal(got_counts, counts) and int(ctx.stats().fragments) == n
        assert np.array_equal(got_sums[..., 3:], sums[..., 3:])   # SA (weighted alpha) and SL (sum of -log(1 - alpha)): no colour in them
        # the fast instance ran: a 1-ulp colour change is far above the 2^-36 resolution of the colour sums
        witness = int((got_sums[..., :3] != sums[..., :3]).any(axis=2).sum())
        print("shading_numerics=fast, %s %s: colour sums differ from the exact fold's on %d pixels" % (tag, weight, witness))
        assert witness > 0
        _within_2_lsb("%s %s" % (tag, weight), img, ref)


def _fast_m9(ctx, name, vp, tag):
    ctx.set_option("depth_peeling_max_layers", 2000)
    ref, n, accum, layers, counts = _ref("m9", name, vp)
    img = ctx.render(9)
    got_accum, got_layers, got_counts = ctx.depth_peeling_buffers()
    assert np.array_equal(got_counts, counts) and np.array_equal(got_layers, layers) and int(ctx.stats().fragments) == n
    assert np.array_equal(_bits(got_accum[..., 3]), _bits(accum[..., 3]))
    witness = int((_bits(got_accum[..., :3]) != _bits(accum[..., :3])).any(axis=2).sum())   # the fast instance ran
    print("shading_numerics=fast, %s: rgb accumulators differ from the exact fold's on %d pixels" % (tag, witness))
    assert witness > 0
    _within_2_lsb(tag, img, ref)


def _fast_m10(ctx, name, vp, tag):
    for K in AL64_LAYERS:
        ctx.set_option("atomic_loop_num_layers", K)
        ref, slots, tail, n, _ = _ref("m10", name, vp, K)
        img = ctx.render(10)
        got_slots, got_tail = ctx.atomic_loop_buffers()
        assert int(ctx.stats().fragments) == n
        # key = depth bits << 32 | packed colour with alpha in the top byte: the depth word and the alpha byte of every slot; of the
        # tail, the sums of alpha and of -log(1 - alpha) (fragments that tie in depth and alpha contribute alike wherever they land)
        assert np.array_equal(got_slots >> np.uint64(24), slots >> np.uint64(24))
        assert np.array_equal(got_tail[..., (0, 4)], tail[..., (0, 4)])
        _within_2_lsb("%s K=%d" % (tag, K), img, ref)


FAST_CHECKS = {"m3": _fast_m3, "m6": _fast_m6, "m8": _fast_m8, "m9": _fast_m9, "m10": _fast_m10}


@pytest.mark.gpu
@pytest.mark.parametrize("group,name,viewport", FAST, ids=lambda v: _id(v))
def test_fast_shading_numerics_against_the_exact_fold(hip_lib, group, name, viewport):
    """The conditions of lv_prism_fast_shade: plain tubes, the raster colour (the default), collect_stats off"""
    c = make_case(name, viewport, shading_numerics="fast")
    assert not c.settings.get("collect_stats", False) and "ppll_fragment_colour" not in c.settings
    ctx = c.hip_context()
    FAST_CHECKS[group](ctx, name, viewport, "%s %s %dx%d" % (group, name, viewport[0], viewport[1]))
    ctx.close()
