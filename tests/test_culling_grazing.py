"""BVH culling on grazing rays, CPU side: the oracle's own trees against its brute force, the generator's condition, and an
independent float32 statement of the builders' box rule + the compressed node's slab test for the single-segment build.

Every comparison is an equality against brute force; nothing here has a tolerance.  The scenes leave the unit box (translated by
up to 1000, scaled by 256) but stay inside the supported coordinate range of DESIGN.md's numerics contract: every radius is at
least 64 ulp of the largest coordinate (checked below)."""
import numpy as np
import pytest

import grazing as gz
from grazing import CONFIG_IDS, MISS, T_MAX, T_MIN, bits, capsule_case, triangle_case
from oracle import lvo


@pytest.mark.parametrize("name", CONFIG_IDS)
def test_radius_is_at_least_64_ulp_of_the_largest_coordinate(name):
    """the supported range (numerics contract): below it a capsule is a few representable positions wide and the
    intersection routines themselves, not the culling, decide what is seen"""
    _, pts, _, lw, *_ = capsule_case(name)
    assert gz.radius_in_ulps(pts["linePosition"], lw * 0.5) >= 64.0
    _, mesh, lw, *_ = triangle_case(name)
    assert gz.radius_in_ulps(mesh[1]["vertexPosition"], lw * 0.5) >= 64.0


FORMS = pytest.mark.parametrize("literal", [True, False], ids=["literal", "closest_approach"])


@FORMS
@pytest.mark.parametrize("n_segments", [0, 1, 2], ids=["870seg", "1seg", "2seg"])
@pytest.mark.parametrize("name", CONFIG_IDS)
def test_oracle_bvh_equals_brute_force_on_grazing_rays(name, n_segments, literal):
    """With boxes padded by r * 1e-3 + 1e-6 alone the oracle's tree lost hits of the closest-approach form at (100, -100, 100) and
    beyond: min(p0, p1) - r - pad rounds to the float32 grid of the coordinate, which is coarser than the pad once |x| passes about
    16.  (The literal roots only count inside the segment's own unpadded box, which that tree's boxes always contain.)"""
    sc, _, _, lw, o, d, _, want = capsule_case(name, n_segments, literal)
    lvo.set_default_intersection_form(literal)
    got = sc.trace_rays(o, d, T_MIN, T_MAX, lw, use_bvh=True)
    lost = int(((want[1] != MISS) & (got[1] == MISS)).sum())
    differ = int(((bits(got[0]) != bits(want[0])) | (got[1] != want[1]) | (got[2] != want[2])).sum())
    assert differ == 0, "%d of %d rays differ from brute force, %d hits lost" % (differ, len(o), lost)


@pytest.mark.parametrize("name", CONFIG_IDS)
def test_oracle_triangle_bvh_equals_brute_force_on_grazing_rays(name):
    ts, _, _, o, d, _, want = triangle_case(name)
    got = ts.trace_rays(o, d, T_MIN, T_MAX, use_bvh=True)
    differ = int(((bits(got[0]) != bits(want[0])) | (got[1] != want[1]) | (bits(got[2]) != bits(want[2])).any(axis=1)).sum())
    assert differ == 0, "%d of %d rays differ from brute force" % (differ, len(o))
    assert (want[1] != MISS).sum() > 0


@FORMS
@pytest.mark.parametrize("name", CONFIG_IDS)
def test_generator_aims_at_what_it_hits(name, literal):
    """The tests above pass trivially on rays that miss.  At least 40 % of the rays have their brute-force closest hit on the
    targeted segment or an index neighbour (measured on the oracle when the generator was written: 0.51 to 0.90, hit share >=
    0.89; the bound comes from those measurements, not from any kernel)."""
    _, _, seg, _, _, _, target, want = capsule_case(name, 0, literal)
    hit = want[1] != MISS
    near = hit & (np.abs(want[1].astype(np.int64) - target.astype(np.int64)) <= 1)
    print("%s: hit share %.3f, on the target or a neighbour %.3f" % (name, hit.mean(), near.mean()))
    assert near.mean() >= 0.40


# ---------------------------------------------------------------- independent float32 statement, single segment
def f32(x):
    return np.asarray(x, dtype=np.float32)


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, the sum rounds once there and once to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def single_node_accepts(p0, p1, radius, o, d, t_min, t_max, literal_slack=True):
    """The build of a one-segment scene and the node step on it, restated.
    Box rule (k_seg_boxes): gz.segment_boxes.  Encoding (k_single_node): origin = lo, scale = ((hi - lo) / 255) * 1.000002 + 1e-30,
    widened by 1.00001 until plane 255 covers hi; the leaf's planes are q = 0 and q = 255.
    Slab test (lv_node_step, lv_slab_q): t = q * (scale * inv) + (origin * inv - o * inv) with inv = 1 / d, near / far chosen by the
    sign of inv, accept iff max(near, tMin) <= fma(min(far, tMax), 1.00001, 4e-7); literal roots cull against the interval
    widened by r / |d| (lv_trace_closest).
    Why 2^-21: the two large terms of t cancel, and the rounding of o * inv and of origin * inv displaces every plane by up to
    about 2 * 2^-24 * |plane| in position space, which the t-relative 1.00001 does not cover; 2^-21 |plane| is four times that.
    The absolute pad (>= 1e-6) is the larger term for |x| < 2.09, so boxes inside the unit box are what they were.
    With the relative term set to 0 this statement rejects 2724 / 5303 hits (literal / closest-approach form) at (100, -100, 100) and
    2533 / 2148 at (1000, 1000, -1000) -- the counts lv_trace_rays lost on an MI355X before the boxes were widened -- and none in the
    other four configurations."""
    lo, hi = gz.segment_boxes(np.stack([p0, p1]), np.array([[0, 1]]), radius)
    lo, hi = lo[0], hi[0]
    scale = f32(f32((hi - lo) / f32(255.0)) * f32(1.000002) + f32(1e-30))
    for a in range(3):
        while fma32(f32(255.0), scale[a], lo[a]) < hi[a]:
            scale[a] = f32(scale[a] * f32(1.00001) + f32(1e-30))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(f32(1.0) / d)
        oi = f32(o * inv)
        A = f32(scale[None, :] * inv)
        B = (lo[None, :].astype(np.float64) * inv.astype(np.float64) - oi.astype(np.float64)).astype(np.float32)
        t0, t255 = B, fma32(f32(255.0), A, B)
        near, far = np.where(inv < 0, t255, t0), np.where(inv < 0, t0, t255)
        slack = f32(f32(radius) / np.sqrt(f32((d * d).sum(axis=1)), dtype=np.float32)) if literal_slack else f32(0.0)
        tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], f32(t_min) - slack))
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], f32(t_max) + slack))
        return tn <= fma32(tf, f32(1.00001), f32(4e-7))


@FORMS
@pytest.mark.parametrize("name", CONFIG_IDS)
def test_float32_statement_of_the_single_node_never_rejects_a_hit(name, literal):
    _, pts, seg, lw, o, d, _, want = capsule_case(name, 1, literal)
    p = pts["linePosition"]
    ok = single_node_accepts(p[seg[0, 0]], p[seg[0, 1]], lw * 0.5, o, d, T_MIN, T_MAX, literal_slack=literal)
    hit = want[1] != MISS
    # every ray is aimed less than r / 100 inside the capsule's extreme point, and at 64 to 130 ulp per radius the rounding of the
    # origin to float32 moves it by about as much: by symmetry about half of the rays still hit.  A quarter keeps the statement from
    # being made about rays that miss.
    print("%s: hit share %.3f" % (name, hit.mean()))
    assert hit.mean() >= 0.25
    assert int((hit & ~ok).sum()) == 0, "%d of %d hits rejected" % (int((hit & ~ok).sum()), int(hit.sum()))
