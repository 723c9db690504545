"""Rendering modes 9 (depth peeling) and 5 (depth complexity) restated on the CPU.

depth_peel_fold() and depth_complexity_frame() are the vectorised numpy statements the GPU tests (test_gpu_depth_peeling.py,
test_gpu_depth_complexity.py) compare the device kernels with, bit for bit.  Here they are checked against scalar transcriptions of
the reference's passes: DepthPeelingRenderer.cpp:271-332 with DepthPeelingGather.glsl:42-49 (per pass over the fragments in
primitive order, the shader's discard `z <= previous depth && i != 0`, a LESS depth test against a buffer cleared to 1.0, the depth
images ping-ponged, FRONT_TO_BACK_PREMUL_ALPHA into the accumulator, BACK_TO_FRONT_PREMUL_ALPHA over the clear colour) and
DepthComplexityResolve.glsl:48-57 (then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour), under the rules of
include/linevis_hip.h (depth_peeling_max_layers, depth_complexity_max_colour): float32, one operation at a time, left to right.

A run is (rgba (n, 4) float32 straight colour, z (n,) float32 window depth >= +0, key (n,) uint32, distinct within a run), in any
order."""
import numpy as np

from test_mlab_restatement import F, pack, window_depth  # noqa: F401  (window_depth: what the GPU tests feed z with)

MAX_LAYERS = 2000
ONE_BITS = np.uint32(0x3F800000)


def _rgba8(v):
    packed = pack(np.asarray(v, F).reshape(-1, 4).T)   # (pack takes the four channels)
    return np.stack([(packed >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=1).astype(np.uint8)


def depth_peel_fold(runs, background, max_layers=MAX_LAYERS, details=False):
    """Per pixel: sort by (z, key), keep the first of each distinct z, drop z >= 1 (as bit patterns: anything that is not in [+0, 1)),
    cut to min(longest run of the frame, max_layers) layers, accumulate front to back in float32, blit over the background.
    Returns the (pixels, 4) uint8 frame; with details (frame, (pixels, 4) float32 accumulators, (pixels,) uint32 layer counts)."""
    num = len(runs)
    longest = max([len(r[1]) for r in runs] + [0])
    passes = min(longest, int(max_layers))
    layers = []
    for rgba, z, key in runs:
        rgba = np.asarray(rgba, F).reshape(-1, 4)
        zb = np.asarray(z, F).reshape(-1).view(np.uint32)
        key = np.asarray(key, np.uint32).reshape(-1)
        order = np.lexsort((key, zb))
        zs = zb[order]
        first = np.ones(len(zs), bool)
        first[1:] = zs[1:] != zs[:-1]
        sel = order[first & (zs < ONE_BITS)][:passes]
        layers.append(rgba[sel])
    count = np.array([len(c) for c in layers], np.uint32)
    A = np.zeros((num, 4), F)
    depth = int(count.max()) if num else 0
    col = np.zeros((num, depth, 4), F)
    for p, c in enumerate(layers):
        col[p, :len(c)] = c
    for i in range(depth):
        live = count > i
        c = col[live, i]
        t = (F(1.0) - A[live, 3]).astype(F)
        s = np.concatenate([(c[:, :3] * c[:, 3:4]).astype(F), c[:, 3:4]], axis=1)
        A[live] = (A[live] + (s * t[:, None]).astype(F)).astype(F)
    bg = np.asarray(background, F)
    out = (A + (bg[None, :] * (F(1.0) - A[:, 3:4]).astype(F)).astype(F)).astype(F)
    frame = _rgba8(out)
    return (frame, A, count) if details else frame


def depth_complexity_max_colour(max_complexity, max_colour=0):
    """numFragmentsMaxColor: the explicit value, or uint32(float(max(maxComplexity, 4)) / 1.5f)"""
    if max_colour:
        return int(max_colour)
    return int(F(F(max(int(max_complexity), 4)) / F(1.5)))


def depth_complexity_frame(counts, background, max_colour=0):
    """counts: the fragments per pixel (any shape).  Returns the (pixels, 4) uint8 frame; the maximum of `counts` sets the scale when
    max_colour = 0."""
    n = np.asarray(counts).reshape(-1).astype(np.uint32)
    mc = depth_complexity_max_colour(n.max() if n.size else 0, max_colour)
    den = F(min(mc, 512))
    pct = np.clip((n.astype(F) / den).astype(F), F(0.0), F(1.0)).astype(F)
    bg = np.asarray(background, F)
    colour = np.array([0.0, 1.0, 1.0], F)
    rest = (F(1.0) - pct).astype(F)
    rgb = ((colour[None, :] * pct[:, None]).astype(F) + (bg[None, :3] * rest[:, None]).astype(F)).astype(F)
    a = (pct + (bg[3] * rest).astype(F)).astype(F)
    return _rgba8(np.concatenate([rgb, a[:, None]], axis=1))


# ---------------------------------------------------------------- scalar transcriptions
def _scalar_peel(runs, background, max_layers=MAX_LAYERS):
    """The reference's frame, pass by pass: every pixel's fragments in primitive order through the gather's discard and the depth test"""
    num = len(runs)
    max_complexity = max([len(r[1]) for r in runs] + [0])            # computeDepthComplexity()
    frags = []
    for rgba, z, key in runs:
        order = np.argsort(np.asarray(key, np.uint32), kind="stable")
        frags.append([(np.asarray(rgba, F).reshape(-1, 4)[i], F(np.asarray(z, F)[i])) for i in order])
    accum = [[F(0.0)] * 4 for _ in range(num)]
    depth_images = [[F(1.0)] * num, [F(1.0)] * num]                    # depthRenderTextures[2]
    for i in range(min(max_complexity, int(max_layers))):
        write, read = depth_images[i % 2], depth_images[(i + 1) % 2]
        for p in range(num):
            write[p] = F(1.0)                                          # clearDepth(1.0)
            colour = None
            for c, z in frags[p]:
                if z <= read[p] and i != 0:                            # DepthPeelingGather.glsl:46-48
                    continue
                if z < write[p]:                                       # depth test LESS, depth write on, blend OVERWRITE
                    write[p] = z
                    colour = c
            if colour is None:
                continue
            s = [F(colour[0] * colour[3]), F(colour[1] * colour[3]), F(colour[2] * colour[3]), F(colour[3])]
            t = F(F(1.0) - accum[p][3])                                # FRONT_TO_BACK_PREMUL_ALPHA
            accum[p] = [F(accum[p][k] + F(s[k] * t)) for k in range(4)]
    bg = [F(b) for b in background]
    out = [[F(a[k] + F(bg[k] * F(F(1.0) - a[3]))) for k in range(4)] for a in accum]   # BACK_TO_FRONT_PREMUL_ALPHA
    return _rgba8(np.array(out, F).reshape(-1, 4)), np.array(accum, F).reshape(-1, 4)


def _scalar_complexity(counts, background, max_colour=0):
    counts = [int(n) for n in np.asarray(counts).reshape(-1)]
    max_complexity = max(counts + [0])
    num_max = int(max_colour) if max_colour else int(F(F(max(max_complexity, 4)) / F(1.5)))
    bg = [F(b) for b in background]
    colour = [F(0.0), F(1.0), F(1.0), F(1.0)]
    out = []
    for n in counts:
        pct = F(min(max(F(F(n) / F(min(num_max, 512))), F(0.0)), F(1.0)) * colour[3])
        rest = F(F(1.0) - pct)
        out.append([F(F(colour[k] * pct) + F(bg[k] * rest)) for k in range(3)] + [F(pct + F(bg[3] * rest))])
    return _rgba8(np.array(out, F).reshape(-1, 4))


# ---------------------------------------------------------------- runs
def random_runs(rng, num_pixels, max_len, empty_share=0.2, tie_share=0.3, min_len=1):
    """random pixels: straight colours, depths in [0, 1) -- a share of them drawn from a small set, so that equal depths under
    different keys occur --, distinct keys, shuffled"""
    runs = []
    for _ in range(num_pixels):
        n = 0 if rng.random() < empty_share else int(rng.integers(min_len, max_len + 1))
        rgba = rng.random((n, 4)).astype(F)
        z = rng.random(n).astype(F)
        tie = rng.random(n) < tie_share
        z[tie] = (rng.integers(0, 4, int(tie.sum())) / F(4.0)).astype(F)
        keys = rng.choice(1 << 20, size=n, replace=False).astype(np.uint32)
        runs.append((rgba, z, keys))
    return runs


def special_runs(rng):
    """equal depths under different keys; z = 1.0, above it and just below it; an empty pixel; alpha 0 and 1"""
    below = np.nextafter(F(1.0), F(0.0))
    c = lambda n: rng.random((n, 4)).astype(F)
    k = lambda n: rng.choice(1 << 20, size=n, replace=False).astype(np.uint32)
    opaque = c(4)
    opaque[1, 3] = F(1.0)
    clear = c(3)
    clear[:, 3] = F(0.0)
    return [
        (c(4), np.array([0.5, 0.5, 0.5, 0.25], F), np.array([9, 3, 7, 100], np.uint32)),        # ties: key 3 wins, 7 and 9 never peeled
        (c(5), np.array([1.0, below, 0.75, 1.0, 2.0], F), k(5)),                                 # z = 1.0 and 2.0 never peeled
        (c(2), np.array([1.0, 1.0], F), k(2)),                                                    # nothing to peel at all
        (c(0), np.zeros(0, F), k(0)),                                                            # an empty pixel
        (opaque, np.array([0.4, 0.2, 0.3, 0.1], F), k(4)),                                       # alpha 1 in the second layer
        (clear, np.array([0.1, 0.2, 0.3], F), k(3)),                                             # alpha 0 only
        (c(3), np.array([0.0, 0.0, below], F), np.array([5, 4, 1], np.uint32)),                  # z = +0 twice
    ]


BG = (0.2, 0.4, 0.6, 1.0)


def _check(runs, max_layers=MAX_LAYERS, bg=BG):
    frame, accum, layers = depth_peel_fold(runs, bg, max_layers, details=True)
    want, want_accum = _scalar_peel(runs, bg, max_layers)
    assert np.array_equal(accum.view(np.uint32), want_accum.view(np.uint32))
    assert np.array_equal(frame, want)
    return frame, accum, layers


def test_fold_matches_the_scalar_transcription():
    rng = np.random.default_rng(3)
    _check(random_runs(rng, 60, 24))
    _check(random_runs(rng, 40, 12), bg=(0.0, 0.0, 0.0, 0.0))


def test_special_runs():
    rng = np.random.default_rng(4)
    runs = special_runs(rng)
    _, accum, layers = _check(runs)
    assert layers.tolist() == [2, 2, 0, 0, 4, 3, 2]
    # the tie: the layers are z = 0.25 (key 100), then z = 0.5 under key 3, the first in primitive order
    rgba = runs[0][0]
    want = np.zeros(4, F)
    for i in (3, 1):
        t = F(1.0) - want[3]
        want = (want + (np.append(rgba[i, :3] * rgba[i, 3], rgba[i, 3]).astype(F) * t).astype(F)).astype(F)
    assert np.array_equal(accum[0], want)
    assert not accum[2].any() and not accum[3].any() and not accum[5].any()   # nothing peeled; alpha 0 adds nothing


def test_an_empty_pixel_next_to_the_longest_one_and_the_cap():
    rng = np.random.default_rng(5)
    runs = random_runs(rng, 6, 10, empty_share=0.0)
    runs[2] = (np.zeros((0, 4), F), np.zeros(0, F), np.zeros(0, np.uint32))
    runs[3] = random_runs(rng, 1, 30, empty_share=0.0, tie_share=0.0, min_len=30)[0]
    _, _, layers = _check(runs)
    assert layers[2] == 0 and layers[3] == 30
    for cap in (1, 3, 29, 30, 31):
        _, _, capped = _check(runs, max_layers=cap)
        assert capped[3] == min(cap, 30) and capped.max() <= cap
    # the cap cuts the far layers: three layers are the three nearest
    a3 = depth_peel_fold(runs, BG, 3, details=True)[1]
    rgba, z, key = runs[3]
    near = np.argsort(z)[:3]
    assert np.array_equal(a3[3], depth_peel_fold([(rgba[near], z[near], key[near])], BG, details=True)[1][0])


def test_any_order_gives_the_same_frame():
    rng = np.random.default_rng(6)
    runs = random_runs(rng, 30, 20) + special_runs(rng)
    shuffled = []
    for rgba, z, key in runs:
        o = rng.permutation(len(z))
        shuffled.append((rgba[o], z[o], key[o]))
    a = depth_peel_fold(runs, BG, details=True)
    b = depth_peel_fold(shuffled, BG, details=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_depth_complexity_frame_matches_the_resolve_shader():
    rng = np.random.default_rng(7)
    for counts, max_colour in (
            (rng.integers(0, 40, 200), 0),
            (np.array([0, 1, 2, 3]), 0),                         # a maximum below 4: numFragmentsMaxColor = uint(4 / 1.5) = 2
            (np.array([0, 0, 0]), 0),
            (np.arange(0, 1200, 7), 0),                          # auto above 512 * 1.5: the divisor saturates at 512
            (np.arange(500, 530), 512), (np.arange(500, 530), 700), (np.arange(500, 530), 511),
            (np.arange(0, 12), 10), (np.arange(0, 12), 1)):
        for bg in (BG, (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 0.5)):
            got = depth_complexity_frame(counts, bg, max_colour)
            assert np.array_equal(got, _scalar_complexity(counts, bg, max_colour)), (max_colour, bg)
    assert depth_complexity_max_colour(3) == 2 and depth_complexity_max_colour(6) == 4 and depth_complexity_max_colour(6, 9) == 9
    # n at the divisor is the full colour, one below it is not
    f = depth_complexity_frame(np.array([511, 512, 513, 2000]), (0.0, 0.0, 0.0, 0.0), 700)
    assert f[1].tolist() == [0, 255, 255, 255] and f[2].tolist() == f[1].tolist() and f[3].tolist() == f[1].tolist()
    g = depth_complexity_frame(np.array([5, 10, 11]), (0.0, 0.0, 0.0, 0.0), 10)
    assert g[0].tolist() == [0, 128, 128, 128] and g[1].tolist() == [0, 255, 255, 255] and g[2].tolist() == g[1].tolist()
