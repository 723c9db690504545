"""Multi-Layer Alpha Blending (rendering mode 3) restated on the CPU.

mlab_fold() is the vectorised numpy statement the GPU tests (test_gpu_mlab.py) compare the device fold with, bit for bit.  Here it is
checked against a scalar, line-by-line transcription of the reference's shaders: MLABGather.glsl:38-60 (multiLayerAlphaBlending),
MLABHeader.glsl:143-163,186 (loadFragmentNodes, clearPixel), MLABResolve.glsl:51-77, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear
colour (MLABRenderer.cpp:78).  float32 throughout, one operation at a time (no fused multiply-add), as the device evaluates it."""
import numpy as np

F = np.float32
INF = F(1e30)                # DISTANCE_INFINITE
CLEAR = np.uint32(0xFF000000)


# ---------------------------------------------------------------- packUnorm4x8 / unpackUnorm4x8 as the device states them
def unpack(c):
    c = np.asarray(c, dtype=np.uint32)
    return [((c >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(F) / F(255.0) for k in range(4)]


def pack(ch):
    out = np.zeros(np.shape(ch[0]), dtype=np.uint32)
    for k in range(4):
        v = np.floor(np.minimum(np.maximum(np.asarray(ch[k], dtype=F), F(0.0)), F(1.0)) * F(255.0) + F(0.5)).astype(np.uint32)
        out |= v << np.uint32(8 * k)
    return out


def mlab_colour(rgba):
    """the gather's node colour: packUnorm4x8(vec4(color.rgb * color.a, 1.0 - color.a)), MLABGather.glsl:76"""
    rgba = np.asarray(rgba, dtype=F).reshape(-1, 4)
    a = rgba[:, 3]
    return pack([rgba[:, 0] * a, rgba[:, 1] * a, rgba[:, 2] * a, F(1.0) - a])


def window_depth(pos, view, proj):
    """gl_FragCoord.z = clip.z / clip.w of world positions (n, 3): rows z, w of proj * view summed in the device's order"""
    view = np.asarray(view, dtype=F).reshape(16)
    proj = np.asarray(proj, dtype=F).reshape(16)
    mz, mw = [F(0.0)] * 4, [F(0.0)] * 4
    for c in range(4):
        for k in range(4):
            mz[c] = F(mz[c] + F(proj[4 * k + 2] * view[4 * c + k]))
            mw[c] = F(mw[c] + F(proj[4 * k + 3] * view[4 * c + k]))
    p = np.asarray(pos, dtype=F).reshape(-1, 3)
    cz = ((mz[0] * p[:, 0] + mz[1] * p[:, 1]) + mz[2] * p[:, 2]) + mz[3]
    cw = ((mw[0] * p[:, 0] + mw[1] * p[:, 1]) + mw[2] * p[:, 2]) + mw[3]
    return (cz / cw).astype(F)


# ---------------------------------------------------------------- the vectorised fold
def mlab_fold(runs, K, background):
    """runs: list (one per pixel) of (colour words uint32, window depths float32, primitive keys uint32) -- any order within a pixel,
    folded in ascending key order.  Returns (num_pixels, 4) uint8 RGBA after the blend over `background`."""
    K = int(K)
    P = len(runs)
    bg = [F(b) for b in background]
    order = []
    lens = np.zeros(P, dtype=np.int64)
    for p, (c, d, k) in enumerate(runs):
        o = np.argsort(np.asarray(k, dtype=np.uint32), kind="stable")
        order.append((np.asarray(c, dtype=np.uint32)[o], np.asarray(d, dtype=F)[o]))
        lens[p] = len(o)
    L = int(lens.max()) if P else 0
    cs = np.zeros((P, max(L, 1)), dtype=np.uint32)
    ds = np.zeros((P, max(L, 1)), dtype=F)
    for p, (c, d) in enumerate(order):
        cs[p, :len(c)] = c
        ds[p, :len(d)] = d
    nd = np.full((P, K + 1), INF, dtype=F)
    nc = np.full((P, K + 1), CLEAR, dtype=np.uint32)
    for j in range(L):
        act = lens > j
        fd = ds[:, j].copy()
        fc = cs[:, j].copy()
        nd[act, K] = INF
        for i in range(K + 1):
            sw = act & (fd <= nd[:, i])
            td, tc = nd[sw, i].copy(), nc[sw, i].copy()
            nd[sw, i], nc[sw, i] = fd[sw], fc[sw]
            fd[sw], fc[sw] = td, tc
        m = act & (nd[:, K] != INF)
        if m.any():
            s = unpack(nc[m, K - 1])
            t = unpack(nc[m, K])
            nc[m, K - 1] = pack([s[0] + t[0] * s[3], s[1] + t[1] * s[3], s[2] + t[2] * s[3], s[3] * t[3]])
    col = [np.zeros(P, dtype=F) for _ in range(3)]
    tr = np.ones(P, dtype=F)
    for i in range(K):
        s = unpack(nc[:, i])
        for k in range(3):
            col[k] = col[k] + tr * s[k]
        tr = tr * s[3]
    a = F(1.0) - tr
    out = [np.full(P, bg[k], dtype=F) for k in range(4)]
    hit = a > F(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            out[k] = np.where(hit, (col[k] / a) * a + bg[k] * (F(1.0) - a), out[k]).astype(F)
        out[3] = np.where(hit, a + bg[3] * (F(1.0) - a), out[3]).astype(F)
    packed = pack(out)
    return np.stack([(packed >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=1).astype(np.uint8)


# ---------------------------------------------------------------- scalar transcription of the shaders
def _unpack1(c):
    return [F(F((int(c) >> (8 * k)) & 0xFF) / F(255.0)) for k in range(4)]


def _pack1(v):
    r = 0
    for k in range(4):
        x = min(max(F(v[k]), F(0.0)), F(1.0))
        r |= int(np.floor(F(F(x * F(255.0)) + F(0.5)))) << (8 * k)
    return r


def _scalar_pixel(frags, K, background):
    """frags: [(key, colour, depth)], folded in primitive (key) order"""
    nodes = [[INF, int(CLEAR)] for _ in range(K)]                      # clearPixel
    for _, colour, depth in sorted(frags):
        lst = [list(n) for n in nodes] + [[INF, 0]]                    # loadFragmentNodes: node K = {DISTANCE_INFINITE, -}
        frag = [F(depth), int(colour)]
        for i in range(K + 1):                                         # multiLayerAlphaBlending
            if frag[0] <= lst[i][0]:
                temp = lst[i]
                lst[i] = frag
                frag = temp
        if lst[K][0] != INF:
            src = _unpack1(lst[K - 1][1])
            dst = _unpack1(lst[K][1])
            merged = [F(src[0] + F(dst[0] * src[3])), F(src[1] + F(dst[1] * src[3])), F(src[2] + F(dst[2] * src[3])),
                      F(src[3] * dst[3])]
            lst[K - 1] = [lst[K - 1][0], _pack1(merged)]
        nodes = lst[:K]                                                # storeFragmentNodes
    color = [F(0.0)] * 3                                               # MLABResolve main()
    transmittance = F(1.0)
    for i in range(K):
        src = _unpack1(nodes[i][1])
        color = [F(color[k] + F(transmittance * src[k])) for k in range(3)]
        transmittance = F(transmittance * src[3])
    alpha_out = F(F(1.0) - transmittance)
    bg = [F(b) for b in background]
    if alpha_out == F(0.0):                                            # (this build's rule: the background, not 0 / 0)
        res = bg
    else:                                                              # BACK_TO_FRONT_STRAIGHT_ALPHA
        res = [F(F(F(color[k] / alpha_out) * alpha_out) + F(bg[k] * F(F(1.0) - alpha_out))) for k in range(3)]
        res.append(F(alpha_out + F(bg[3] * F(F(1.0) - alpha_out))))
    p = _pack1(res)
    return np.array([(p >> (8 * k)) & 0xFF for k in range(4)], dtype=np.uint8)


def random_runs(rng, num_pixels, max_len, alpha_lo=0.001, tie_depths=False, empty_share=0.2):
    """random pixels: colours of straight-alpha fragments with alpha in [alpha_lo, 1), depths in [0, 1) (from a small set with
    tie_depths), unique keys, shuffled"""
    runs = []
    for _ in range(num_pixels):
        n = 0 if rng.random() < empty_share else int(rng.integers(1, max_len + 1))
        rgba = rng.random((n, 4)).astype(F)
        rgba[:, 3] = (F(alpha_lo) + rgba[:, 3] * F(1.0 - alpha_lo)).astype(F)
        depth = (rng.integers(0, 4, n) / F(4.0)).astype(F) if tie_depths else rng.random(n).astype(F)
        keys = rng.choice(1 << 20, size=n, replace=False).astype(np.uint32)
        runs.append((mlab_colour(rgba), depth, keys))
    return runs


def _check(runs, K, bg=(0.2, 0.4, 0.6, 1.0)):
    got = mlab_fold(runs, K, bg)
    for p, (c, d, k) in enumerate(runs):
        ref = _scalar_pixel(list(zip(k.tolist(), c.tolist(), d.tolist())), K, bg)
        assert np.array_equal(got[p], ref), (p, K, got[p], ref)


def test_fold_matches_the_scalar_transcription():
    rng = np.random.default_rng(3)
    for K in (2, 3, 8):
        _check(random_runs(rng, 60, 24), K)


def test_ties_put_the_new_fragment_in_front():
    rng = np.random.default_rng(5)
    _check(random_runs(rng, 60, 20, tie_depths=True), 3)
    # two fragments at the same depth: the later one (in primitive order) takes node 0, the earlier one moves to node 1
    a = mlab_colour([[1.0, 0.0, 0.0, 0.5]])[0]
    b = mlab_colour([[0.0, 0.0, 1.0, 0.5]])[0]
    run = (np.array([a, b], np.uint32), np.array([0.5, 0.5], F), np.array([1, 2], np.uint32))
    swapped = (np.array([a, b], np.uint32), np.array([0.5, 0.5], F), np.array([2, 1], np.uint32))
    out = mlab_fold([run, swapped], 2, (1.0, 1.0, 1.0, 1.0))
    assert out[0][2] > out[0][0] and out[1][0] > out[1][2]   # blue in front in the first, red in the second


def test_single_layer():
    _check(random_runs(np.random.default_rng(11), 80, 30), 1)


def test_alpha_near_the_discard_threshold_and_empty_pixels():
    rng = np.random.default_rng(13)
    runs = random_runs(rng, 40, 10, empty_share=0.3)
    for p in range(0, 40, 3):   # alpha in [0.001, 0.00195): 1 - a packs to 255 -> transmittance 1, alphaOut 0 -> the background
        n = int(rng.integers(1, 6))
        rgba = rng.random((n, 4)).astype(F)
        rgba[:, 3] = (F(0.001) + rgba[:, 3] * F(0.00095)).astype(F)
        runs[p] = (mlab_colour(rgba), rng.random(n).astype(F), rng.choice(1000, n, replace=False).astype(np.uint32))
    for p in range(1, 40, 3):   # alpha in [0.00196, 0.002): 1 - a packs to 254, the fragments show
        rgba = np.array([[1.0, 0.0, 0.0, 0.00197]], F)
        runs[p] = (mlab_colour(rgba), np.array([0.5], F), np.array([7], np.uint32))
    bg = (0.25, 0.5, 0.75, 1.0)
    _check(runs, 4, bg)
    out = mlab_fold(runs, 4, bg)
    bg8 = np.array([64, 128, 191, 255], np.uint8)
    for p in range(0, 40, 3):
        assert np.array_equal(out[p], bg8)
    for p in range(1, 40, 3):
        assert not np.array_equal(out[p], bg8)
    for p, r in enumerate(runs):
        if len(r[0]) == 0:
            assert np.array_equal(out[p], bg8)


def test_sixty_four_layers():
    _check(random_runs(np.random.default_rng(17), 12, 90), 64)


def test_order_within_a_run_does_not_matter():
    rng = np.random.default_rng(19)
    runs = random_runs(rng, 50, 40)
    shuffled = []
    for c, d, k in runs:
        o = rng.permutation(len(k))
        shuffled.append((c[o], d[o], k[o]))
    assert np.array_equal(mlab_fold(runs, 5, (0, 0, 0, 0)), mlab_fold(shuffled, 5, (0, 0, 0, 0)))
