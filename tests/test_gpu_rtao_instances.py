"""Every kernel instance of the mode-11 frame with RTAO -- k_ao_rays, k_ao_primary, k_primary_pair, k_render_rt and the two reduce
kernels, as lv_run_ao and lv_rt_frame (lv_render.hip) choose them from the options -- at odd viewports and tile lists, against the
oracle's brute force (use_bvh = False; never another GPU run).

Coverage, guaranteed by `_assert_coverage` over the parameter lists when the module is imported:
  * `launched` restates the dispatch of lv_run_ao / lv_rt_frame (the macros are quoted above it); the union over ROWS x their
    variants + NARROW + TINY equals FULL_TABLE: 24 k_ao_rays (2 AH x 4 geometries x (ST | PG on | PG off)), 6 k_ao_primary,
    12 k_primary_pair, 22 k_render_rt (both FAST ones among them) and both reduce kernels.
  * every k_ao_rays, k_ao_primary and k_primary_pair instance occurs at two or more of the MAIN viewports, and each of them, and both
    reduce kernels, under two or more tile lists there: after the whole frame of every variant, test_instances_match_the_oracle
    renders one of ROW_LISTS (tiles of 4, the reversed 16-pixel list, 24 x 10, a tile twice) and compares every tile with that
    variant's frame and the AO image with the oracle's.  TILED adds the whole set of lists in both dispatch orders and the rectangles
    for the four RTAO geometries and the three primaries.
  * ROWS crosses COMBOS (scene x RTAO geometry x colour geometry) with any-hit / distance-based, once at spp 64 with one iteration
    (ST, PG on, PG off, paired and not, `fast` on the plain capsule rows) and once at spp 4 / 3 / 6 with two iterations (the frame
    runs the pair and then k_ao_primary; spp 3 and 6 reach k_ao_reduce<false>), every second of those with num_samples_per_frame = 2
    (the AO tiles get their one-pixel halo: a 65 x 65 viewport becomes a 67 x 67 tile of four groups).

What is asserted (the bars are derived, not measured): AO factors bit for bit -- every operation on that path is +, -, *, /, sqrt on
float32 in a fixed order and the project holds all three geometries to that --; the frame within the project's 2 LSB of the oracle's;
frames and AO images of the variants that share an expected image (stats on / off, paired or not, per_pixel / per_ray, either
dispatch order, every tile list and rectangle) byte for byte equal to each other.  Under collect_stats the counters that do not
depend on the traversal order equal what the oracle counted: ao_rays_traced = the oracle's rays minus its primaries (= hit pixels
x spp summed over the iterations) and ao_hit_pixels = the hit pixels of the last iteration (the oracle's AO rays of this run minus
those of a run one iteration shorter, over spp).  Node and primitive counters are printed, not asserted (nothing
pins them).  Launches per LV_KERNEL_* slot are asserted too (iterations, iterations, 1); k_ao_primary and k_primary_pair record in
the same slot, so the library cannot show which of the two ran -- `launched` restates pairPrimaries of lv_frame_render instead.

lv_get_ao promises the accumulated image of the pixels the last call's RTAO pass covered (the rectangle, dilated by the halo and
clipped); outside them the buffer keeps what earlier frames left, or, with a halo, the other of two ping-pong buffers.  So after a
rectangle only its inside is compared.

What keeps the comparisons from comparing nothing is checked on the oracle alone, without a GPU (test_the_cases_compare_something):
at the five MAIN viewports every case has >= 100 pixels with AO < 1 and >= 30 of them away from the most frequent value, with three
or more distinct values; at 5 x 67 >= 10.  With the default camera a 1 x 1 viewport hits nothing, so TINY_CAMERA
looks at a tube from nearby: every 1 x 1 and 3 x 2 case has a pixel with AO < 1.  Pixels with AO < 1 on the oracle, spp 64
distance-based / spp 3 any-hit (the test prints them):
                               61x47    97x53    33x71    65x65    64x64    5x67
    plain, capsules           432/121  546/167  612/187  811/254  787/220  61/14
    plain, triangle tubes     415/113  514/160  594/172  778/238  748/196  60/10
    elliptic tubelets         398/169  524/239  793/370  789/334  740/343  66/28
    bands on capsules         392/162  509/202  797/352  752/334  721/314
    band triangle tubes       418/179  556/244  843/401  815/375  792/361
    helicity, capsules        442/234  563/314  748/420  863/429  810/436  92/56
    helicity, triangle tubes  434/230  555/312  740/415  855/436  804/424

Deliberate single-line mutations of a scratch build that this file catches (none committed; each reads and writes the addresses the
original does): the sample index of the per-pixel generation `genSmp0 + lane` -> `genSmp0 + (lane ^ 1u)` fails the fifteen
distance-based spp-64 rows (AO bits against the oracle; per_pixel against per_ray); the sum of k_ao_reduce<false> in reverse sample
order fails the eight distance-based spp-3 / spp-6 rows; `pingPong = halo` (the in-place running mean under overlapping tiles, as before
the fix) fails the three tile-list cases without a halo.  `min(64u, L.tileH - 64u * gyi)` -> `64u` in lv_ao_group_base was not run: at
97 x 53 it moves the second group's segment to slots 4096 ... 5844 of a G-buffer of 5141, a write out of bounds.  By reading, it
changes a base wherever a second group column stands in a partial group row: 97 x 53, 65 x 65 and the 67 x 67 AO tiles would show it.
"""
import functools

import numpy as np
import pytest

from common import max_lsb_diff, small_case
from linevis_amd import capi, scenes, tiling
from oracle import lvo

MAIN = ((61, 47), (97, 53), (33, 71), (65, 65), (64, 64))
NARROW_VIEWPORT = (5, 67)
TINY_VIEWPORTS = ((1, 1), (3, 2))

RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_gamma=1.0)
GEOMETRIES = ("tri", "elliptic", "capsule literal", "capsule closest")
SHADES = ("plain", "bands", "helicity")


# ---------------------------------------------------------------- the scenes (<= 400 segments each)
def _plain_curves():
    return scenes.normalize(scenes.random_curves(n_lines=20, points_per_line=20, seed=7))


def _ribbons():
    from test_gpu_elliptic import ribbon_scene
    return ribbon_scene(n_lines=5, pts=80)


@functools.lru_cache(maxsize=None)
def _mesh(scene):
    """The triangle tubes of a scene: the reference's RTAO geometry and its "Triangle Mesh" colour geometry"""
    if scene == "plain":
        tr = _plain_curves()
        return lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, 0.03, 6)
    if scene in ("bands", "elliptic"):
        tr = _ribbons()
        return lvo.build_tube_triangle_render_data_ribbons(tr.positions, tr.attributes, tr.line_offsets, tr.ribbon_directions, 0.05, 0.3, 8)
    from test_helicity_bands import helix_with_helicity
    tr, hel = helix_with_helicity()
    return lvo.build_tube_triangle_render_data(tr.positions, tr.attributes, tr.line_offsets, 0.03, 6, helicities=hel)


def _tiny_camera():
    """A camera 0.12 in front of a point of the plain scene, on the line through it and the origin: the centre ray of any viewport
    runs down that line (the point is one of the two, among every seventh, where all cases of TINY show a pixel with AO < 1)"""
    p = _plain_curves().positions[54].astype(np.float64)
    return tuple(float(x) for x in p * (1.0 + 0.12 / np.linalg.norm(p)))


TINY_CAMERA = _tiny_camera()
SCENE_SHADE = {"plain": "plain", "bands": "bands", "elliptic": "bands", "helicity": "helicity"}
SCENE_RADIUS = {"plain": 0.1, "bands": 0.15, "elliptic": 0.15, "helicity": 0.15}


def make_case(scene, viewport, camera_pos=None, **settings):
    kw = dict(width=viewport[0], height=viewport[1], **settings)
    if camera_pos is not None:
        kw["camera_pos"] = camera_pos
    if scene == "plain":
        return small_case(n_lines=20, pts_per_line=20, line_width=0.03, **kw)
    if scene in ("bands", "elliptic"):
        from test_gpu_elliptic import band_case
        # (line_width 0.03: at band_case's 0.02 the circular tubes show 23 and 28 pixels away from the most frequent any-hit value at
        # 61 x 47 and 97 x 53, under the 30 of test_the_cases_compare_something)
        return band_case(elliptic=scene == "elliptic", tr=_ribbons(), tube_num_subdivisions=8, line_width=0.03, **kw)
    from test_gpu_helicity_bands import helicity_case
    return helicity_case(**kw)[0]


# ---------------------------------------------------------------- 1. the mapping: options -> kernel instances
# lv_frame_render (lv_render.hip):
#     const bool pairWanted = ctx->opt.overlapPrimaryPasses == 1 || (ctx->opt.overlapPrimaryPasses == 2 && gridTiles <= 16u * uint32_t(ctx->numCUs));
#     const bool pairPrimaries = pairWanted && rayTracer && U.useAmbientOcclusion &&
#                                !U.aoPrebaked && !ctx->opt.useMlat && !ctx->opt.rtTriangleMesh && !U.useEllipticTubes &&
#                                !ctx->opt.svgfEnabled && !ctx->opt.shEnabled && (U.useJitteredRays ? U.numSamplesPerFrame : 1u) == 1u && ctx->numSegs > 0u &&
#                                (ctx->opt.numAccumulatedFrames <= 1u || ctx->opt.frameNumber < ctx->opt.aoIterations);
# lv_run_ao, per iteration:
#     const bool pairNow = pairColour && iter == iterBegin;
#     #define LV_LAUNCH_AOP(ST, PR)
#         if (pairNow && U.useHelicityBands) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_HELICITY);
#         else if (pairNow && U.useBands) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_BANDS);
#         else if (pairNow) LV_LAUNCH_PAIR(ST, PR, LV_SHADE_PLAIN);
#         else k_ao_primary<ST, PR>
#     #define LV_LAUNCH_AO3(ST, AH, PG)
#         if (tri) LV_LAUNCH_AO(ST, AH, LV_PRIM_TRIANGLE, false, PG);
#         else if (U.useEllipticTubes) LV_LAUNCH_AO(ST, AH, LV_PRIM_ELLIPTIC, false, PG);
#         else if (lv_literal_intersection(ctx)) LV_LAUNCH_AO(ST, AH, LV_PRIM_CAPSULE, true, PG);
#         else LV_LAUNCH_AO(ST, AH, LV_PRIM_CAPSULE, false, PG);
#     #define LV_LAUNCH_AO2(ST, AH)
#         if (!ST && pixelGen) LV_LAUNCH_AO3(ST, AH, !ST); else LV_LAUNCH_AO3(ST, AH, false);
#     if (stats) { if (tri) LV_LAUNCH_AOP(true, LV_PRIM_TRIANGLE); else if (ell) LV_LAUNCH_AOP(true, LV_PRIM_ELLIPTIC); else LV_LAUNCH_AOP(true, LV_PRIM_CAPSULE); }
#     else { if (tri) LV_LAUNCH_AOP(false, LV_PRIM_TRIANGLE); else if (ell) LV_LAUNCH_AOP(false, LV_PRIM_ELLIPTIC); else LV_LAUNCH_AOP(false, LV_PRIM_CAPSULE); }
#     const bool anyHit = !U.aoUseDistance;
#     const bool pixelGen = ctx->opt.aoPixelGeneration && spp % LV_WAVE == 0u && LV_AO_CHUNK % LV_WAVE == 0u && LV_AO_CHUNK_SMALL % LV_WAVE == 0u && ...;
#     if (stats) { if (anyHit) LV_LAUNCH_AO2(true, true); else LV_LAUNCH_AO2(true, false); }
#     else { if (anyHit) LV_LAUNCH_AO2(false, true); else LV_LAUNCH_AO2(false, false); }
#     if ((spp & 3u) == 0u) k_ao_reduce_rows else k_ao_reduce<false>
# lv_rt_frame:
#     const bool fastPlain = ctx->opt.fastShading && !stats && !tri && !U.useHelicityBands && !U.useEllipticTubes && !U.useBands;
#     #define LV_LAUNCH_RT2(ST)
#         if (fastPlain && firstHitsTraced) k_render_rt<false, LV_PRIM_CAPSULE, LV_SHADE_PLAIN, true, 1>
#         else if (fastPlain) k_render_rt<false, LV_PRIM_CAPSULE, LV_SHADE_PLAIN, false, 1>
#         else if (firstHitsTraced && U.useHelicityBands) LV_LAUNCH_RT_PRE(ST, LV_SHADE_HELICITY);
#         else if (firstHitsTraced && U.useBands) LV_LAUNCH_RT_PRE(ST, LV_SHADE_BANDS);
#         else if (firstHitsTraced) LV_LAUNCH_RT_PRE(ST, LV_SHADE_PLAIN);
#         else if (tri && U.useHelicityBands) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_HELICITY);
#         else if (tri && U.useBands) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_BANDS);
#         else if (tri) LV_LAUNCH_RT(ST, LV_PRIM_TRIANGLE, LV_SHADE_PLAIN);
#         else if (U.useHelicityBands) LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_HELICITY);
#         else if (U.useEllipticTubes) LV_LAUNCH_RT(ST, LV_PRIM_ELLIPTIC, LV_SHADE_BANDS);
#         else if (U.useBands) LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_BANDS);
#         else LV_LAUNCH_RT(ST, LV_PRIM_CAPSULE, LV_SHADE_PLAIN);
def pairs(*, overlap, colour_tri, elliptic, spf):
    """pairPrimaries for the frames of this file: the ray tracer with RTAO, no prebaker / MLAT / SVGF / Spatial Hashing / accumulation"""
    jittered = spf > 1   # useJitteredRays (lv_fill_uniforms): more than one sample per pixel, or accumulated frames
    return bool(overlap) and not colour_tri and not elliptic and (spf if jittered else 1) == 1


def launched(*, stats, any_hit, ao, shade, elliptic, colour_tri, per_pixel, spp, iterations, overlap, fast, spf):
    """The kernel instances one mode-11 frame launches.  ao: the RTAO geometry, one of GEOMETRIES (`elliptic` <=> ao == "elliptic"
    unless the RTAO pass traces the triangle tubes of an elliptic scene); shade: one of SHADES"""
    assert ao in GEOMETRIES and shade in SHADES and (ao != "elliptic" or elliptic) and (not elliptic or shade == "bands")
    tri = ao == "tri"
    paired = pairs(overlap=overlap, colour_tri=colour_tri, elliptic=elliptic, spf=spf)
    prim = "tri" if tri else "elliptic" if elliptic else "capsule"
    out = set()
    for it in range(iterations):
        if paired and it == 0:
            out.add(("k_primary_pair", stats, prim, shade))
        else:
            out.add(("k_ao_primary", stats, prim))
    pixel_gen = per_pixel and spp % 64 == 0
    geometry = "tri" if tri else "elliptic" if elliptic else ao
    out.add(("k_ao_rays", stats, any_hit, geometry, (not stats) and pixel_gen))
    out.add("k_ao_reduce_rows" if spp % 4 == 0 else "k_ao_reduce<false>")
    fast_plain = fast and not stats and not colour_tri and shade == "plain" and not elliptic
    if fast_plain:
        out.add(("k_render_rt", False, "capsule", "plain", paired, True))
    elif paired:
        out.add(("k_render_rt", stats, "capsule", shade, True, False))
    elif colour_tri:
        out.add(("k_render_rt", stats, "tri", shade, False, False))
    elif shade == "helicity":
        out.add(("k_render_rt", stats, "capsule", "helicity", False, False))
    elif elliptic:
        out.add(("k_render_rt", stats, "elliptic", "bands", False, False))
    else:
        out.add(("k_render_rt", stats, "capsule", shade, False, False))
    return out


FULL_TABLE = (
    {("k_ao_rays", st, ah, g, pg) for ah in (False, True) for g in GEOMETRIES for st, pg in ((True, False), (False, True), (False, False))}
    | {("k_ao_primary", st, p) for st in (False, True) for p in ("tri", "elliptic", "capsule")}
    | {("k_primary_pair", st, p, s) for st in (False, True) for p in ("tri", "capsule") for s in SHADES}
    | {("k_render_rt", False, "capsule", "plain", pre, True) for pre in (False, True)}
    | {("k_render_rt", st, "capsule", s, True, False) for st in (False, True) for s in SHADES}
    | {("k_render_rt", st, "tri", s, False, False) for st in (False, True) for s in SHADES}
    | {("k_render_rt", st, p, s, False, False) for st in (False, True)
       for p, s in (("capsule", "helicity"), ("elliptic", "bands"), ("capsule", "bands"), ("capsule", "plain"))}
    | {"k_ao_reduce_rows", "k_ao_reduce<false>"})
assert len(FULL_TABLE) == 24 + 6 + 12 + 22 + 2


# ---------------------------------------------------------------- 2. the parameter lists
# (scene, RTAO geometry, colour pass on the triangle mesh)
COMBOS = (("plain", "capsule closest", False), ("plain", "capsule literal", False), ("plain", "tri", False),
          ("elliptic", "elliptic", False), ("elliptic", "tri", False),
          ("bands", "capsule closest", False), ("bands", "tri", False),
          ("helicity", "capsule literal", False), ("helicity", "tri", False),
          ("plain", "tri", True), ("bands", "capsule literal", True), ("helicity", "capsule closest", True))
LOW_SPP = (4, 3, 6)


def _row(scene, ao, colour_tri, any_hit, spp, iterations, spf, jitter, viewport, camera_pos=None):
    return dict(scene=scene, ao=ao, colour_tri=colour_tri, any_hit=any_hit, spp=spp, iterations=iterations, spf=spf, jitter=jitter,
                viewport=viewport, camera_pos=camera_pos)


ROWS = []
for _i, (_scene, _ao, _ct) in enumerate(COMBOS):
    for _j, _ah in enumerate((False, True)):
        # spp 64, one iteration: ST, PG on and off, paired and not
        ROWS.append(_row(_scene, _ao, _ct, _ah, 64, 1, 1, bool((_i + _j) % 2), MAIN[(_i + 3 * _j) % 5]))
        # spp 4 / 3 / 6, two iterations (the pair, then k_ao_primary); every second row with two samples per pixel (the AO halo)
        ROWS.append(_row(_scene, _ao, _ct, _ah, LOW_SPP[(_i + _j) % 3], 2, 1 + (_i + _j) % 2, bool((_i + _j + 1) % 2), MAIN[(_i + 3 * _j + 2) % 5]))
ROWS.append(_row("plain", "capsule closest", False, False, 4, 2, 2, True, (65, 65)))   # the 67 x 67 AO tile of the issue, stated
# the tubelets are one combination: their two per-pixel-generation instances once more, at other viewports
ROWS.append(_row("elliptic", "elliptic", False, False, 64, 1, 1, False, (33, 71)))
ROWS.append(_row("elliptic", "elliptic", False, True, 64, 1, 1, True, (64, 64)))
NARROW = [_row(s, ao, ct, ah, spp, its, 1, True, NARROW_VIEWPORT)
          for s, ao, ct, ah, spp, its in (("plain", "capsule closest", False, False, 64, 1), ("plain", "tri", False, True, 3, 2),
                                          ("elliptic", "elliptic", False, False, 64, 1), ("helicity", "capsule literal", False, True, 4, 2))]


def variants(row):
    """(collect_stats, overlap_primary_passes, ao_ray_generation, shading_numerics) of one row: they share the AO image, and all but
    `fast` the frame"""
    out = [(False, True, "per_pixel", "exact"), (False, False, "per_pixel", "exact"), (True, True, "per_pixel", "exact"),
           (True, False, "per_pixel", "exact")]
    if row["spp"] % 64 == 0:
        out += [(False, True, "per_ray", "exact"), (False, False, "per_ray", "exact")]
    if row["scene"] == "plain" and not row["colour_tri"]:
        out += [(False, True, "per_pixel", "fast"), (False, False, "per_pixel", "fast")]
    return out


def _launched_by(row, variant):
    stats, overlap, gen, numerics = variant
    return launched(stats=stats, any_hit=row["any_hit"], ao=row["ao"], shade=SCENE_SHADE[row["scene"]], elliptic=row["scene"] == "elliptic",
                    colour_tri=row["colour_tri"], per_pixel=gen == "per_pixel", spp=row["spp"], iterations=row["iterations"],
                    overlap=overlap, fast=numerics == "fast", spf=row["spf"])


# tile lists and rectangles: (viewport, scene, RTAO geometry, num_samples_per_frame)
TILED = [(vp, scene, ao, spf) for vp, scene, ao, spf in (((97, 53), "plain", "capsule closest", 1), ((97, 53), "plain", "tri", 2),
                                                         ((65, 65), "plain", "capsule literal", 2), ((65, 65), "plain", "tri", 1),
                                                         ((97, 53), "elliptic", "elliptic", 2), ((65, 65), "elliptic", "elliptic", 1))]
# as RECTS of test_gpu_oit_instances.py: ragged to both edges, the last column, the last pixel, the first row, an inner column, an inner
# row and an inner pixel
RECTS = {(97, 53): ((60, 24, 37, 29), (96, 0, 1, 53), (96, 52, 1, 1), (0, 0, 97, 1), (45, 0, 1, 53), (0, 13, 97, 1), (67, 12, 1, 1)),
         (65, 65): ((30, 20, 35, 45), (64, 0, 1, 65), (64, 64, 1, 1), (0, 0, 65, 1), (32, 0, 1, 65), (0, 30, 65, 1), (33, 31, 1, 1))}


def _tiny_rows():
    return [_row(s, ao, False, ah, spp, its, 1, jitter, vp, TINY_CAMERA)
            for vp in TINY_VIEWPORTS
            for s, ao, ah, spp, its, jitter in (("plain", "capsule closest", False, 64, 1, False), ("plain", "tri", True, 6, 2, False),
                                                ("plain", "capsule closest", True, 3, 1, True))]


TINY = _tiny_rows()
EVERY = ROWS + NARROW + TINY
for _k, _r in enumerate(EVERY):
    _r["index"] = _k
# the list (a key of _tile_lists) that variant v of row k renders after its whole frame: consecutive variants take consecutive lists
ROW_LISTS = ("4", "16 reversed", "24x10", "16 with one tile twice")


def row_list(row, variant_index):
    return ROW_LISTS[(row["index"] + variant_index) % len(ROW_LISTS)]


def _assert_coverage():
    every = EVERY
    seen = set()
    for row in every:
        for v in variants(row):
            seen |= _launched_by(row, v)
    assert seen == FULL_TABLE, (sorted(map(str, FULL_TABLE - seen)), sorted(map(str, seen - FULL_TABLE)))
    # every sample and primary instance at two or more of the main viewports
    where = {}
    for row in ROWS:
        for v in variants(row):
            for inst in _launched_by(row, v):
                if isinstance(inst, tuple) and inst[0] in ("k_ao_rays", "k_ao_primary", "k_primary_pair"):
                    where.setdefault(inst, set()).add(row["viewport"])
    wanted = {i for i in FULL_TABLE if isinstance(i, tuple) and i[0] != "k_render_rt"}
    assert set(where) == wanted and all(len(v) >= 2 and v <= set(MAIN) for v in where.values()), \
        sorted((str(k), sorted(v)) for k, v in where.items() if len(v) < 2)
    assert {row["viewport"] for row in ROWS} == set(MAIN)
    # ... and every one of them, and both reduce kernels, under a tile list at a main viewport -- under two different ones, in fact:
    # test_instances_match_the_oracle renders row_list(row, v) after the whole frame of every variant
    lists = {}
    for row in ROWS:
        for v, variant in enumerate(variants(row)):
            for inst in _launched_by(row, variant):
                if not (isinstance(inst, tuple) and inst[0] == "k_render_rt"):
                    lists.setdefault(inst, set()).add(row_list(row, v))
    assert set(lists) == wanted | {"k_ao_reduce_rows", "k_ao_reduce<false>"} and all(len(v) >= 2 and v <= set(ROW_LISTS) for v in lists.values()), \
        sorted((str(k), sorted(v)) for k, v in lists.items() if len(v) < 2)
    # the whole set of lists, both dispatch orders and the rectangles (test_tile_lists_*, test_ragged_rectangles_*): all four RTAO
    # geometries, all three primaries, paired and not
    tiled = set()
    for vp, scene, ao, spf in TILED:
        assert vp in RECTS
        for overlap in (True, False):
            for st in (False, True):
                tiled |= {i[:1] + i[2:] for i in launched(stats=st, any_hit=False, ao=ao, shade=SCENE_SHADE[scene], elliptic=scene == "elliptic",
                                                           colour_tri=False, per_pixel=True, spp=4, iterations=2, overlap=overlap,
                                                           fast=False, spf=spf) if isinstance(i, tuple) and i[0] != "k_render_rt"}
    assert {g for k, _, g, _ in (i for i in tiled if i[0] == "k_ao_rays")} >= {"tri", "elliptic", "capsule literal", "capsule closest"}
    assert {i[1] for i in tiled if i[0] == "k_ao_primary"} == {"tri", "elliptic", "capsule"}
    assert {i[1] for i in tiled if i[0] == "k_primary_pair"} == {"tri", "capsule"}
    assert {vp for vp, _, _, _ in TILED} == {(97, 53), (65, 65)} and {spf for _, _, _, spf in TILED} == {1, 2}
    # the knobs of the issue's table
    assert {r["spp"] for r in ROWS} == {64, 4, 3, 6} and {r["iterations"] for r in ROWS} == {1, 2} and {r["spf"] for r in ROWS} == {1, 2}
    assert {(r["any_hit"], r["jitter"]) for r in ROWS} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(r["viewport"] == (65, 65) and r["spf"] == 2 for r in ROWS)


_assert_coverage()


# ---------------------------------------------------------------- the settings of a row, its context and its reference
def _form(ao):
    return "closest_approach" if ao == "capsule closest" else "literal"


def _settings(scene, ao, colour_tri, any_hit, spp, iterations, spf, jitter):
    s = dict(RTAO, ambient_occlusion_radius=SCENE_RADIUS[scene], ambient_occlusion_distance_based=not any_hit,
             ambient_occlusion_samples_per_frame=spp, ambient_occlusion_iterations=iterations, use_jittered_primary_rays=jitter,
             rtao_geometry="triangle_tubes" if ao == "tri" else "capsules", intersection_form=_form(ao))
    if spf > 1:
        s["num_samples_per_frame"] = spf
    if colour_tri:
        s["geometry_mode"] = "Triangle Mesh"
    return s


def _row_case(row):
    return make_case(row["scene"], row["viewport"], row["camera_pos"],
                     **_settings(row["scene"], row["ao"], row["colour_tri"], row["any_hit"], row["spp"], row["iterations"], row["spf"],
                                 row["jitter"]))


def _needs_mesh(row):
    return row["ao"] == "tri" or row["colour_tri"]


def _context(row):
    ctx = _row_case(row).hip_context()
    if _needs_mesh(row):
        ctx.set_tube_triangle_mesh(*_mesh(row["scene"]))
    return ctx


@functools.lru_cache(maxsize=None)
def _expected(scene, viewport, spp, iterations, any_hit, ao, colour_tri, spf, jitter, camera_pos=None):
    """(AO image, frame, AO rays the oracle traced, hit pixels of its last iteration), brute force; keyed by what changes the expected
    image and nothing else.  The arrays are shared by every test that needs them and never written to."""
    row = _row(scene, ao, colour_tri, any_hit, spp, iterations, spf, jitter, viewport, camera_pos)
    c = _row_case(row)
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    tsc = lvo.TriScene(*_mesh(scene), c.line_width) if _needs_mesh(row) else None
    st = lvo.Stats()
    ao_ref = tsc.render_ao(P, use_bvh=False, stats=st) if ao == "tri" else sc.render_ao(P, use_bvh=False, stats=st)
    frame = tsc.render_rt(sc, P, ao=ao_ref, use_bvh=False) if colour_tri else sc.render_rt(P, ao=ao_ref, use_bvh=False)
    ao_rays = int(st.raysTraced) - viewport[0] * viewport[1] * iterations   # every pixel's primary ray, every iteration
    assert ao_rays >= 0 and ao_rays % spp == 0
    # iteration k's seeds depend on k alone: the rays of the last iteration are this run's minus those of a run one iteration shorter
    before = _expected(scene, viewport, spp, iterations - 1, any_hit, ao, colour_tri, spf, jitter, camera_pos)[2] if iterations > 1 else 0
    assert ao_rays >= before
    ao_ref.setflags(write=False)
    frame.setflags(write=False)
    return ao_ref, frame, ao_rays, (ao_rays - before) // spp


def _expected_of(row):
    return _expected(row["scene"], row["viewport"], row["spp"], row["iterations"], row["any_hit"], row["ao"], row["colour_tri"],
                     row["spf"], row["jitter"], row["camera_pos"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _row_id(row):
    return "%s-%s%s-%s-spp%d-it%d-spf%d-%s-%dx%d" % (row["scene"], row["ao"].replace(" ", "_"), "-trimesh" if row["colour_tri"] else "",
                                                    "anyhit" if row["any_hit"] else "distance", row["spp"], row["iterations"], row["spf"],
                                                    "jitter" if row["jitter"] else "centre", row["viewport"][0], row["viewport"][1])


# ---------------------------------------------------------------- the conditions, on the oracle alone (no GPU)
def _lit(ao_img):
    """(pixels with AO < 1, those away from the most frequent such value, distinct values among them)"""
    v = ao_img[ao_img < 1.0]
    if v.size == 0:
        return 0, 0, 0
    values, counts = np.unique(v, return_counts=True)
    return int(v.size), int(v.size - counts.max()), int(len(values))


def test_the_cases_compare_something():
    for scene, ao, colour_tri in sorted({(s, a, False) for s, a, _ in COMBOS}):
        for vp in MAIN + (NARROW_VIEWPORT,):
            got = []
            for spp, any_hit in ((64, False), (3, True)):
                if vp == NARROW_VIEWPORT and not any(r["scene"] == scene and r["ao"] == ao for r in NARROW):
                    continue
                n, off, distinct = _lit(_expected(scene, vp, spp, 1, any_hit, ao, False, 1, True)[0])
                got.append(n)
                if vp == NARROW_VIEWPORT:
                    assert n >= 10, (scene, ao, vp, spp, n, off, distinct)
                else:
                    assert n >= 100 and off >= 30 and distinct >= 3, (scene, ao, vp, spp, n, off, distinct)
            if got:
                print("pixels with AO < 1: %-8s %-16s %3dx%-3d spp 64 distance-based %4d, spp 3 any-hit %4d" % (scene, ao, vp[0], vp[1], *got))
    # a 1 x 1 viewport under the default camera hits nothing, which is why the tiny viewports have a camera of their own
    assert _lit(_expected("plain", (1, 1), 64, 1, False, "capsule closest", False, 1, True)[0])[0] == 0
    for row in TINY:
        assert _lit(_expected_of(row)[0])[0] >= 1, _row_id(row)
    # the references tell the instances apart: another geometry, form or occlusion rule is another AO image
    vp = MAIN[0]
    base = _expected("plain", vp, 64, 1, False, "capsule closest", False, 1, True)[0]
    for other in (("capsule literal", False), ("tri", False), ("capsule closest", True)):
        assert int((_bits(_expected("plain", vp, 64, 1, other[1], other[0], False, 1, True)[0]) != _bits(base)).sum()) > 20, other


# ---------------------------------------------------------------- 1. the instance matrix, the narrow and the tiny viewports
def _check_counters(ctx, row, ao_rays, last_hits, tag):
    st = ctx.stats()
    print("%s: ao_rays %d ao_hit_pixels %d | not asserted: rays %d nodes %d prims %d ao_nodes %d ao_prims %d" % (
        tag, st.ao_rays_traced, st.ao_hit_pixels, st.rays_traced, st.nodes_visited, st.prims_tested, st.ao_nodes_visited, st.ao_prims_tested))
    assert int(st.ao_rays_traced) == ao_rays, tag
    assert int(st.ao_hit_pixels) == last_hits, tag   # (dc->aoCount: k_ao_tile_scan writes it every iteration)
    if row["iterations"] == 1 or not row["jitter"]:   # every iteration hits the same pixels
        assert last_hits * row["spp"] * row["iterations"] == ao_rays, tag


def _check_row(row):
    ao_ref, frame_ref, ao_rays, last_hits = _expected_of(row)
    W, H = row["viewport"]
    lists = _tile_lists(W, H)
    ctx = _context(row)
    ctx.set_option("kernel_timers", "all")
    frames = {}
    for v, variant in enumerate(variants(row)):
        stats, overlap, gen, numerics = variant
        tag = "%s %s" % (_row_id(row), variant)
        ctx.set_options(dict(collect_stats=stats, overlap_primary_passes=overlap, ao_ray_generation=gen, shading_numerics=numerics))
        ctx.reset_timers()
        img = ctx.render(capi.MODE_RAY_TRACER)
        ao = ctx.get_ao()
        assert np.array_equal(_bits(ao), _bits(ao_ref)), tag
        d = max_lsb_diff(img, frame_ref)
        assert d <= 2, (tag, d)
        first = frames.setdefault(numerics, (variant, img))   # second layer: the variants of one expected image, byte for byte
        assert np.array_equal(img, first[1]), (tag, first[0])
        launches = [len(ctx.kernel_times(k)) for k in (capi.KERNEL_AO_PRIMARY, capi.KERNEL_AO_RAYS, capi.KERNEL_RENDER_RT)]
        assert launches == [row["iterations"], row["iterations"], 1], (tag, launches)
        if stats:
            _check_counters(ctx, row, ao_rays, last_hits, tag)
        # this variant's instances under a tile list: every tile its part of the variant's frame, the AO image the whole frame's
        name = row_list(row, v)
        tiles, tw, th = lists[name]
        px = _render_tiles(ctx, tiles, tw, th)
        for i, (x0, y0) in enumerate(tiles.tolist()):
            w, h = min(tw, W - x0), min(th, H - y0)
            assert np.array_equal(px[i, :h, :w], img[y0:y0 + h, x0:x0 + w]), (tag, name, i, x0, y0)
        assert np.array_equal(_bits(ctx.get_ao()), _bits(ao_ref)), (tag, name)
    if "fast" in frames:
        d = np.abs(frames["fast"][1].astype(np.int32) - frames["exact"][1].astype(np.int32)).max(axis=2)
        print("%s: shading_numerics=fast differs from exact on %d of %d pixels, max %d LSB" % (_row_id(row), int((d > 0).sum()), d.size, int(d.max())))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", EVERY, ids=_row_id)
def test_instances_match_the_oracle(hip_lib, row):
    _check_row(row)


# ---------------------------------------------------------------- 4. tile lists and rectangles
def _tile_lists(W, H):
    """name: (origins, tile width, tile height); every list covers the viewport"""
    t16 = tiling.make_tiles(W, H, 16)
    lists = {"64": (tiling.make_tiles(W, H, 64), 64, 64), "16": (t16, 16, 16),
             "4": (tiling.make_tiles(W, H, 4), 4, 4),   # (97 x 53: 350 tiles, 65 x 65: 289 -- more than 256 groups)
             "24x10": (np.array([(x, y) for y in range(0, H, 10) for x in range(0, W, 24)], dtype=np.uint32), 24, 10),
             "16 reversed": (np.ascontiguousarray(t16[::-1]), 16, 16),
             "16 with one tile twice": (np.concatenate([t16[:5], t16[2:3], t16[5:]]), 16, 16),
             # (where the running mean of the second iteration updated in place, a pixel computed twice could blend its factor in twice:
             # lv_run_ao reads one image and writes the other whenever tiles share pixels -- the whole list twice gives that race room)
             "16 with every tile twice": (np.concatenate([t16, t16[::-1]]), 16, 16)}
    assert set(ROW_LISTS) <= set(lists)
    return lists


def _render_tiles(ctx, tiles, tw, th):
    import torch
    out = torch.zeros((len(tiles), th, tw, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_tiles_device(out.data_ptr(), tiles, tw, th, mode=capi.MODE_RAY_TRACER)
    ctx.stats()   # synchronises the context's stream
    return out.cpu().numpy()


def _tiled_row(vp, scene, ao, spf):
    return _row(scene, ao, False, False, 4, 2, spf, True, vp)


def _tiled_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace(" ", "_")


@pytest.mark.gpu
@pytest.mark.parametrize("viewport,scene,ao,spf", TILED, ids=_tiled_id)
def test_tile_lists_equal_the_whole_frame(hip_lib, viewport, scene, ao, spf):
    """Square tiles of 64, 16 and 4 (more than 256 groups: k_ao_tile_scan sums several counts per thread), 24 x 10 tiles, a reversed list
    and one with a tile twice; in both dispatch orders, paired and not, with and without collect_stats: every tile equals its part of
    the whole frame byte for byte, and the AO image the whole frame's bit for bit"""
    W, H = viewport
    row = _tiled_row(viewport, scene, ao, spf)
    ao_ref, frame_ref, _, _ = _expected_of(row)
    ctx = _context(row)
    whole = ctx.render(capi.MODE_RAY_TRACER)
    assert np.array_equal(_bits(ctx.get_ao()), _bits(ao_ref)) and max_lsb_diff(whole, frame_ref) <= 2
    assert len(_tile_lists(W, H)["4"][0]) > 256   # k_ao_tile_scan sums several counts per thread
    for order in ("cost", "as_numbered"):
        for overlap, stats in ((True, False), (False, True)) if order == "cost" else ((False, False), (True, True)):
            ctx.set_options(dict(dispatch_order=order, overlap_primary_passes=overlap, collect_stats=stats))
            assert np.array_equal(ctx.render(capi.MODE_RAY_TRACER), whole), (order, overlap, stats)
            for name, (tiles, tw, th) in _tile_lists(W, H).items():
                tag = (name, order, overlap, stats)
                px = _render_tiles(ctx, tiles, tw, th)
                for i, (x0, y0) in enumerate(tiles.tolist()):
                    w, h = min(tw, W - x0), min(th, H - y0)
                    assert np.array_equal(px[i, :h, :w], whole[y0:y0 + h, x0:x0 + w]), (tag, i, x0, y0)
                assert np.array_equal(_bits(ctx.get_ao()), _bits(ao_ref)), tag
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("viewport,scene,ao,spf", TILED, ids=_tiled_id)
def test_ragged_rectangles_equal_their_part_of_the_frame(hip_lib, viewport, scene, ao, spf):
    row = _tiled_row(viewport, scene, ao, spf)
    ao_ref, frame_ref, _, _ = _expected_of(row)
    ctx = _context(row)
    whole = ctx.render(capi.MODE_RAY_TRACER)
    assert np.array_equal(_bits(ctx.get_ao()), _bits(ao_ref)) and max_lsb_diff(whole, frame_ref) <= 2
    for overlap, stats in ((True, False), (False, True)):
        ctx.set_options(dict(overlap_primary_passes=overlap, collect_stats=stats))
        for x, y, w, h in RECTS[viewport]:
            tag = (overlap, stats, x, y, w, h)
            assert np.array_equal(ctx.render(capi.MODE_RAY_TRACER, tile=(x, y, w, h)), whole[y:y + h, x:x + w]), tag
            # lv_get_ao: the pixels the call's RTAO pass covered, nothing promised outside them
            assert np.array_equal(_bits(ctx.get_ao()[y:y + h, x:x + w]), _bits(ao_ref[y:y + h, x:x + w])), tag
        assert np.array_equal(ctx.render(capi.MODE_RAY_TRACER), whole)
        assert np.array_equal(_bits(ctx.get_ao()), _bits(ao_ref))
    ctx.close()
