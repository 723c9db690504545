"""Rendering mode 8 (Weighted Blended OIT) restated on the CPU.

wboit_fold() is the vectorised numpy statement the GPU tests (test_gpu_wboit.py) compare the device kernels with, bit for bit.  Here it
is checked against a scalar, line-by-line transcription of WBOITGather.glsl:17-27 and WBOITResolve.glsl:38-48 (then
BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour) under the rules of include/linevis_hip.h (wboit_depth_weight): float32, one
operation at a time, left to right; the four weighted sums and the sum of -log(1 - alpha) as 64-bit fixed-point terms
rint(clamp(term, -1024, 1024) * 2^36), and therefore independent of the order of the fragments.

A run is (rgba (n, 4) float32 straight colour, z (n,) float32 window depth)."""
import numpy as np
import pytest

from test_mboit_restatement import F, exp_det, from_fixed, log_det, to_fixed
from test_mboit_restatement import _exp1, _fixed1, _log1, _pack1, _unfixed1
from test_mlab_restatement import pack, window_depth  # noqa: F401  (window_depth: what the GPU tests feed z with)

MAX_COUNT = 131071
WEIGHTS = ("reference", "opengl")


def wboit_weight(alpha, z, weight="reference"):
    """WBOITGather.glsl:21-24; `opengl` is the line the shader keeps as a comment"""
    alpha, z = np.asarray(alpha, dtype=F), np.asarray(z, dtype=F)
    with np.errstate(all="ignore"):
        A = (np.fmin(F(1.0), alpha) * F(8.0)).astype(F) + F(0.01)
        if weight == "opengl":
            B = ((-z) * F(0.95)).astype(F) + F(1.0)
        else:
            assert weight == "reference"
            B = (((F(2.0) * z).astype(F) - F(1.0)).astype(F) * F(0.95)).astype(F) - F(1.0)
        raw = ((((((A * A).astype(F) * A).astype(F) * F(1e8)).astype(F) * B).astype(F) * B).astype(F) * B).astype(F)
        return np.fmin(np.fmax(raw, F(0.01)), F(300.0)).astype(F)   # (fmax drops a NaN: 0.01)


def wboit_terms(rgba, z, weight="reference"):
    """(n, 5) int64: the terms of SR, SG, SB, SA, SL of n fragments"""
    rgba = np.asarray(rgba, dtype=F).reshape(-1, 4)
    a = rgba[:, 3]
    w = wboit_weight(a, z, weight)
    with np.errstate(all="ignore"):
        t = (F(1.0) - a).astype(F)
        logt = to_fixed(-log_det(np.where((t > F(0.0)) & (t < F(1.0)), t, F(0.5)).astype(F)))
        rev = np.where(t <= F(0.0), to_fixed(F(1024.0)), np.where(t < F(1.0), logt, 0))   # (t >= 1 or NaN: 0)
        cols = [to_fixed(((rgba[:, k] * a).astype(F) * w).astype(F)) for k in range(3)] + [to_fixed((a * w).astype(F))]
    return np.stack(cols + [rev], axis=1).astype(np.int64)


def wboit_resolve(sums, counts, background):
    """sums (P, 5) int64, counts (P,) -> (P, 4) uint8"""
    bg = np.asarray(background, dtype=F)
    with np.errstate(all="ignore"):
        R = exp_det((-from_fixed(sums[:, 4])).astype(F))
        clear = (np.asarray(counts) == 0) | (R > F(0.9999))
        den = np.fmax(from_fixed(sums[:, 3]), F(1e-5)).astype(F)
        a = (F(1.0) - R).astype(F)
        out = []
        for k in range(3):
            v = (((from_fixed(sums[:, k]) / den).astype(F) * a).astype(F) + (bg[k] * (F(1.0) - a).astype(F)).astype(F)).astype(F)
            out.append(np.where(clear, bg[k], v).astype(F))
        out.append(np.where(clear, bg[3], (a + (bg[3] * (F(1.0) - a).astype(F)).astype(F)).astype(F)).astype(F))
    p = pack(out)
    return np.stack([(p >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=1).astype(np.uint8)


def wboit_fold(runs, background, weight="reference", details=False):
    """runs: one (rgba, z) per pixel, in any order.  Returns the frame (P, 4) uint8, with details also the sums (P, 5) int64
    {SR, SG, SB, SA, SL}."""
    P = len(runs)
    n = np.array([len(r[1]) for r in runs], dtype=np.int64)
    assert n.max(initial=0) <= MAX_COUNT
    rgba = np.concatenate([np.asarray(r[0], dtype=F).reshape(-1, 4) for r in runs]) if n.sum() else np.zeros((0, 4), F)
    z = np.concatenate([np.asarray(r[1], dtype=F).reshape(-1) for r in runs]) if n.sum() else np.zeros(0, F)
    pix = np.repeat(np.arange(P), n)
    terms = wboit_terms(rgba, z, weight)
    sums = np.zeros((P, 5), dtype=np.int64)
    for k in range(5):
        np.add.at(sums[:, k], pix, terms[:, k])
    frame = wboit_resolve(sums, n, background)
    return (frame, sums) if details else frame


# ---------------------------------------------------------------- the scalar transcription
def _scalar_pixel(frags, background, weight):
    """frags: [(r, g, b, a, z)]; the two shaders line by line, one float32 operation at a time.  Returns (rgba8 list, sums list)"""
    S = [0, 0, 0, 0, 0]
    with np.errstate(all="ignore"):
        for r, g, b, alpha, z in frags:
            r, g, b, alpha, z = F(r), F(g), F(b), F(alpha), F(z)
            pre = [F(r * alpha), F(g * alpha), F(b * alpha), alpha]                  # premultipliedColor, WBOITGather.glsl:18
            m = F(1.0) if (np.isnan(alpha) or alpha > F(1.0)) else alpha            # min(1.0, a)
            A = F(F(m * F(8.0)) + F(0.01))                                          # :21
            if weight == "opengl":
                B = F(F(F(-z) * F(0.95)) + F(1.0))                                  # :22 (the comment)
            else:
                B = F(F(F(F(F(2.0) * z) - F(1.0)) * F(0.95)) - F(1.0))              # :23
            raw = F(F(F(F(F(F(A * A) * A) * F(1e8)) * B) * B) * B)                  # :24
            w = F(0.01) if (np.isnan(raw) or raw < F(0.01)) else (F(300.0) if raw > F(300.0) else raw)
            for k in range(4):
                S[k] += _fixed1(F(pre[k] * w))                                      # :25, the blend unit's ONE, ONE as integers
            t = F(F(1.0) - alpha)                                                   # :26, the blend unit's ZERO, ONE_MINUS_SRC_COLOR
            if t <= F(0.0):
                S[4] += _fixed1(F(1024.0))
            elif t < F(1.0):
                S[4] += _fixed1(F(-_log1(t)))
        bg = [F(x) for x in background]
        out = list(bg)
        if len(frags):
            R = _exp1(F(-_unfixed1(S[4])))                                          # WBOITResolve.glsl:39
            if not R > F(0.9999):                                                   # :40
                sa = _unfixed1(S[3])
                den = sa if sa > F(1e-5) else F(1e-5)                               # :47
                a = F(F(1.0) - R)
                out = [F(F(F(_unfixed1(S[k]) / den) * a) + F(bg[k] * F(F(1.0) - a))) for k in range(3)]
                out.append(F(a + F(bg[3] * F(F(1.0) - a))))
    p = _pack1(out)
    return [(p >> (8 * k)) & 0xFF for k in range(4)], S


# ---------------------------------------------------------------- inputs
def random_runs(rng, num_pixels, max_len, alpha_lo=0.001, alpha_hi=1.0, empty_share=0.2, min_len=1):
    runs = []
    for _ in range(num_pixels):
        n = 0 if rng.random() < empty_share else int(rng.integers(min_len, max_len + 1))
        rgba = rng.random((n, 4)).astype(F)
        rgba[:, 3] = (alpha_lo + rgba[:, 3] * (alpha_hi - alpha_lo)).astype(F)
        runs.append((rgba, rng.random(n).astype(F)))
    return runs


def revealage_edge_runs():
    """two single-fragment pixels with R = exp(-unfixed(SL)) just on each side of 0.9999 (searched, not assumed)"""
    lo, hi = F(5e-5), F(2e-4)
    a, b = lo.view(np.uint32), hi.view(np.uint32)

    def covered(bits):
        _, s = wboit_fold([(np.array([[1, 0, 0, np.uint32(bits).view(F)]], F), np.array([0.5], F))], (0, 0, 0, 0), details=True)
        return not exp_det((-from_fixed(s[:, 4])).astype(F))[0] > F(0.9999)
    assert not covered(a) and covered(b)
    while b - a > 1:
        mid = (int(a) + int(b)) // 2
        if covered(mid):
            b = np.uint32(mid)
        else:
            a = np.uint32(mid)
    return [(np.array([[0.9, 0.5, 0.1, a.view(F)]], F), np.array([0.25], F)), (np.array([[0.9, 0.5, 0.1, b.view(F)]], F), np.array([0.25], F))]


def special_runs(rng):
    """alpha = 0, 1, 1e-8, 0.999999; z = 0, 1; an empty pixel; a pixel with R just on each side of 0.9999"""
    runs = [(np.zeros((0, 4), F), np.zeros(0, F))]
    for alpha in (0.0, 1.0, 1e-8, 0.999999):
        for n in (1, 3):
            r = random_runs(rng, 1, n, empty_share=0.0, min_len=n)[0]
            r[0][0, 3] = F(alpha)
            runs.append(r)
        r = random_runs(rng, 1, 2, empty_share=0.0, min_len=2)[0]
        r[0][:, 3] = F(alpha)
        runs.append(r)
    for zz in (0.0, 1.0):
        for n in (1, 4):
            r = random_runs(rng, 1, n, empty_share=0.0, min_len=n)[0]
            r[1][0] = F(zz)
            runs.append(r)
        r = random_runs(rng, 1, 2, empty_share=0.0, min_len=2, alpha_lo=0.001, alpha_hi=0.03)[0]
        r[1][:] = F(zz)
        runs.append(r)
    return runs + revealage_edge_runs()


BG = (0.2, 0.4, 0.6, 1.0)


def _check(runs, weight, bg=BG):
    frame, sums = wboit_fold(runs, bg, weight, details=True)
    for p, (rgba, z) in enumerate(runs):
        ref, S = _scalar_pixel([tuple(rgba[i]) + (z[i],) for i in range(len(z))], bg, weight)
        assert S == [int(x) for x in sums[p]], (p, weight, S, sums[p])
        assert ref == [int(x) for x in frame[p]], (p, weight, ref, frame[p])


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("weight", WEIGHTS)
def test_fold_matches_the_scalar_transcription(weight):
    rng = np.random.default_rng(8)
    runs = random_runs(rng, 120, 12) + random_runs(rng, 20, 6, alpha_lo=0.0005, alpha_hi=0.04) + special_runs(rng)
    assert any(len(r[1]) == 0 for r in runs)
    _check(runs, weight)
    _check(runs[:40], weight, bg=(0.0, 0.0, 0.0, 0.0))


def test_revealage_threshold_is_met_from_both_sides():
    under, over = revealage_edge_runs()
    assert under[0][0, 3].view(np.uint32) + 1 == over[0][0, 3].view(np.uint32)
    frame = wboit_fold([under, over], BG)
    assert [int(x) for x in frame[0]] == [51, 102, 153, 255]   # the background
    assert [int(x) for x in frame[1]][3] == 255 and frame[1][0] >= 51   # (alpha 1e-4 of another colour: covered, if barely)
    _, sums = wboit_fold([under, over], BG, details=True)
    R = exp_det((-from_fixed(sums[:, 4])).astype(F))
    assert R[0] > F(0.9999) and not R[1] > F(0.9999)


@pytest.mark.parametrize("weight", WEIGHTS)
def test_any_order_gives_the_same_bits_and_runs_can_be_split(weight):
    rng = np.random.default_rng(21)
    runs = random_runs(rng, 60, 40, empty_share=0.0, min_len=2)
    frame, sums = wboit_fold(runs, BG, weight, details=True)
    for _ in range(3):
        shuffled = []
        for rgba, z in runs:
            o = rng.permutation(len(z))
            shuffled.append((rgba[o], z[o]))
        f2, s2 = wboit_fold(shuffled, BG, weight, details=True)
        assert np.array_equal(f2, frame) and np.array_equal(s2, sums)
    # a run split in two: the sums of the parts add up to the run's
    first = [(rgba[: len(z) // 2], z[: len(z) // 2]) for rgba, z in runs]
    second = [(rgba[len(z) // 2:], z[len(z) // 2:]) for rgba, z in runs]
    _, s_a = wboit_fold(first, BG, weight, details=True)
    _, s_b = wboit_fold(second, BG, weight, details=True)
    assert np.array_equal(s_a + s_b, sums)
    assert np.array_equal(wboit_resolve(s_a + s_b, np.ones(len(runs)), BG), frame)


def test_reference_weight_is_the_constant_one_hundredth():
    """The finding, pinned: with Vulkan's gl_FragCoord.z in [0, 1] the reference's b is negative, the product is negative and the
    clamp returns its lower bound for every fragment.  Every float32 z in [0, 1] whose low 11 mantissa bits are zero, 8 alphas."""
    bits = np.arange(0, int(F(1.0).view(np.uint32)) + 1, 1 << 11, dtype=np.uint32)
    z = bits.view(F)
    assert z[0] == 0.0 and z[-1] == 1.0 and len(z) > 500000
    for alpha in (0.0, 1e-8, 0.001, 0.035, 0.25, 0.5, 0.999999, 1.0):
        w = wboit_weight(np.full(z.shape, alpha, F), z, "reference")
        assert np.all(w.view(np.uint32) == F(0.01).view(np.uint32)), alpha
        A = F(F(min(1.0, alpha)) * F(8.0)) + F(0.01)
        B = (((F(2.0) * z).astype(F) - F(1.0)) * F(0.95)).astype(F) - F(1.0)
        assert B.max() < 0.0 and A > 0.0
    # b > 0 needs z > 1.026: outside what a valid camera produces
    assert wboit_weight(F(0.5), F(1.03), "reference") > F(0.01) and wboit_weight(F(0.5), F(1.02), "reference") == F(0.01)
    # the commented line is positive, and saturated at 300 except for small alpha
    assert wboit_weight(F(0.5), F(0.5), "opengl") == F(300.0)
    assert F(0.01) < wboit_weight(F(0.005), F(0.9), "opengl") < F(300.0)


def test_opengl_weight_lets_the_nearer_fragment_dominate():
    red, blue = [1.0, 0.0, 0.0, 0.005], [0.0, 0.0, 1.0, 0.005]
    runs = [(np.array([red, blue], F), np.array([0.1, 0.95], F)), (np.array([red, blue], F), np.array([0.95, 0.1], F))]
    _, sums = wboit_fold(runs, (0.0, 0.0, 0.0, 1.0), "opengl", details=True)
    # (weights 300 and 11.6: B = 0.905 and 0.0975, A = 0.05)
    assert sums[0, 0] > 20 * sums[0, 2] and sums[1, 2] > 20 * sums[1, 0]   # red in front in the first, blue in the second
    c0 = from_fixed(sums[0, :3]) / from_fixed(sums[0, 3])
    c1 = from_fixed(sums[1, :3]) / from_fixed(sums[1, 3])
    assert c0[0] > 0.95 and c1[2] > 0.95
    # under the reference's weight the two cannot be told apart
    _, ref = wboit_fold(runs, (0.0, 0.0, 0.0, 1.0), "reference", details=True)
    assert np.array_equal(ref[0], ref[1]) and ref[0, 0] == ref[0, 2]


def _straight_blend(runs, bg):
    """one fragment over the background in float64"""
    out = np.zeros((len(runs), 4))
    for p, (rgba, _) in enumerate(runs):
        a = float(rgba[0, 3])
        out[p, :3] = a * rgba[0, :3].astype(np.float64) + (1.0 - a) * np.asarray(bg[:3], dtype=np.float64)
        out[p, 3] = a + (1.0 - a) * bg[3]
    return out * 255.0


@pytest.mark.parametrize("weight", WEIGHTS)
def test_single_fragment_is_within_one_lsb_of_straight_alpha_blending(weight):
    rng = np.random.default_rng(31)
    runs = random_runs(rng, 400, 1, empty_share=0.0, alpha_lo=0.01)
    bg = (0.9, 0.8, 0.1, 1.0)
    frame = wboit_fold(runs, bg, weight)
    assert np.abs(frame.astype(np.float64) - _straight_blend(runs, bg)).max() <= 1.0


def blend_unit_frame(runs, background, weight, order=None):
    """The reference's own arithmetic: the blend unit's float32 sums and products in submission order (accumulatedColor: ONE, ONE;
    revealage: ZERO, ONE_MINUS_SRC_COLOR from the clear value 1), WBOITResolve.glsl:38-48, then the straight-alpha blend."""
    bg = [F(x) for x in background]
    out = np.zeros((len(runs), 4), dtype=np.uint8)
    with np.errstate(all="ignore"):
        for p, (rgba, z) in enumerate(runs):
            w = wboit_weight(rgba[:, 3], z, weight)
            acc, rev = [F(0.0)] * 4, F(1.0)
            idx = range(len(z)) if order is None else order[p]
            for i in idx:
                a = rgba[i, 3]
                pre = [F(rgba[i, 0] * a), F(rgba[i, 1] * a), F(rgba[i, 2] * a), a]
                acc = [F(acc[k] + F(pre[k] * w[i])) for k in range(4)]
                rev = F(rev * F(F(1.0) - a))
            px = list(bg)
            if len(z) and not rev > F(0.9999):
                den = acc[3] if acc[3] > F(1e-5) else F(1e-5)
                ao = F(F(1.0) - rev)
                px = [F(F(F(acc[k] / den) * ao) + F(bg[k] * F(F(1.0) - ao))) for k in range(3)] + [F(ao + F(bg[3] * F(F(1.0) - ao)))]
            v = _pack1(px)
            out[p] = [(v >> (8 * k)) & 0xFF for k in range(4)]
    return out


# the largest difference (LSB of the RGBA8 frame) between the statement and the blend unit's float32 arithmetic in submission order
# over the 1500 runs below, as measured; the bound is that + 1 LSB for the other submission orders (each moves the blend unit's own
# result by its float32 rounding, far below one LSB of the 8-bit frame, but can carry a value across a rounding boundary)
BLEND_UNIT_MAX_LSB = {"reference": 0, "opengl": 0}


def blend_unit_difference(weight, seed=57, n=1500):
    rng = np.random.default_rng(seed)
    # half of the runs opaque in sum (R near 0), half thin (alpha <= 0.1: the product of 1 - alpha decides the frame)
    runs = random_runs(rng, n // 2, 40, empty_share=0.0, min_len=3) + random_runs(rng, n - n // 2, 40, alpha_hi=0.1, empty_share=0.0, min_len=3)
    bg = (1.0, 1.0, 1.0, 1.0)
    frame = wboit_fold(runs, bg, weight)
    assert np.count_nonzero(np.any(frame != 255, axis=1)) > n * 9 // 10   # (the frames are not the background)
    d = np.abs(frame.astype(np.int64) - blend_unit_frame(runs, bg, weight).astype(np.int64))
    return int(d.max()), float(d.mean())


@pytest.mark.parametrize("weight", WEIGHTS)
def test_statement_stays_next_to_the_blend_unit(weight):
    mx, mean = blend_unit_difference(weight)
    print("statement against the blend unit, %s: max %d LSB, mean %.4f LSB" % (weight, mx, mean))
    assert mx <= BLEND_UNIT_MAX_LSB[weight] + 1, (weight, mx, mean)
