"""The simulation-mesh hull in the pooled modes 2 and 3 (linevis_amd/csrc/lv_hull_pool.h; include/linevis_hip.h, hull_fragment_pool)
restated on the CPU from what is there: the hull fragments of tests/test_hull_restatement.py, the oracle's linked lists and prism
fragments, lvo.ppll_resolve and mlab_fold of tests/test_mlab_restatement.py.

ppll_union() appends the hull fragments past the 0.001 discard to the oracle's per-pixel lists as nodes {pack(rgba), bits(|pos -
camera|), next}; mlab_union() builds per-pixel runs of the line entries with the oracle's keys and the hull entries with key
(numSegs << 6) + triangle.  tests/test_gpu_hull_pool.py compares the device with both.

Here, without a GPU: neither fold depends on the order within a run; the depth is what sorts a hull node among the line nodes; every
hull key exceeds every line key; the two depth metrics (distance to the camera in mode 2, window depth in mode 3) order the two
layers of the closed box the same way."""
import numpy as np

from oracle import lvo
from test_hull_restatement import F, hull_case, hull_runs, line_fragments, reference_fragments
from test_mlab_restatement import mlab_colour, mlab_fold, pack

END = 0xFFFFFFFF


def camera_position(c):
    """the camera position as the device holds it: column 3 of the float32 inverse of the view matrix (View.cam)"""
    return np.asarray(lvo.mat4_inverse(np.asarray(c.view, dtype=F).reshape(16)), dtype=F).reshape(16)[12:15].copy()


def camera_distance(pos, cam):
    """length(fragmentPositionWorld - cameraPosition) as the device's len3: sqrt((dx dx + dy dy) + dz dz) in float32"""
    d = [np.asarray(pos[:, k], dtype=F) - F(cam[k]) for k in range(3)]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(F)


def pixel_addresses(c, P):
    """the tiled address of every pixel y * w + x (TiledAddress.glsl:53-85, vectorised as in tests/test_gpu_parity.py)"""
    pw = c.padded()[0]
    tw, th = int(P.ppllTileW), int(P.ppllTileH)
    ys, xs = np.mgrid[0:c.height, 0:c.width]
    addr = ((ys // th) * (pw // tw) + xs // tw) * (tw * th) + (ys % th) * tw + xs % tw
    assert addr[c.height - 1, c.width - 1] == lvo.ppll_addr(c.width - 1, c.height - 1, pw, tw, th)
    return addr.reshape(-1).astype(np.int64)


def list_entries(nodes, start):
    """the linked lists flattened: (address, colour, depth bits) of every node, in walk order per address"""
    addr, col, dep = [], [], []
    for a in np.nonzero(start != END)[0]:
        i = int(start[a])
        while i != END:
            addr.append(int(a)); col.append(int(nodes[i, 0])); dep.append(int(nodes[i, 1]))
            i = int(nodes[i, 2])
    return np.array(addr, np.int64), np.array(col, np.uint32), np.array(dep, np.uint32)


def build_lists(addr, col, dep, num_addr, rng=None):
    """nodes {colour, depth bits, next} and start offsets of the entries: every list in ascending (depth, colour) order -- the order
    lv_ppll_get_buffers exports and the oracle's gather builds, nearest first -- or, with rng, in a random order"""
    order = np.lexsort((col, dep, addr)) if rng is None else np.lexsort((rng.random(len(addr)), addr))
    addr, col, dep = addr[order], col[order], dep[order]
    n = len(addr)
    nodes = np.zeros((max(n, 1), 3), np.uint32)
    nodes[:n, 0], nodes[:n, 1] = col, dep
    nxt = np.arange(1, n + 1, dtype=np.int64)
    last = np.ones(n, bool)
    last[:-1] = addr[1:] != addr[:-1]
    nxt[last] = END
    nodes[:n, 2] = nxt.astype(np.uint32)
    start = np.full(num_addr, END, np.uint32)
    first = np.ones(n, bool)
    first[1:] = last[:-1]
    start[addr[first]] = np.nonzero(first)[0].astype(np.uint32)
    return nodes, start


def hull_nodes(c, P, fr, hull_rgba=None):
    """(address, colour, depth bits) of the hull fragments past the gather's discard (alpha < 0.001, LinkedListGather.glsl:34)"""
    rgba = np.asarray(fr["rgba"] if hull_rgba is None else hull_rgba, dtype=F).reshape(-1, 4)
    keep = rgba[:, 3] >= F(0.001)
    dep = camera_distance(fr["pos"], camera_position(c)).view(np.uint32)
    addr = pixel_addresses(c, P)[fr["pixel"].astype(np.int64)]
    return addr[keep], pack([rgba[keep, k] for k in range(4)]), dep[keep]


def ppll_union(c, fr, hull_rgba=None, rng=None):
    """The mode-2 lists with the hull: the oracle's lists plus the hull nodes.  hull_rgba: other colours for the hull's fragments (the
    device's own); rng: lists in random order instead of ascending.
    Returns (nodes, start offsets, the lvo.ppll_resolve frame)."""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    assert P.ppllFragmentSource == 1
    nodes, start, cnt = sc.ppll_gather(P, use_bvh=True)
    la, lc, ld = list_entries(nodes, start)
    ha, hc, hd = hull_nodes(c, P, fr, hull_rgba)
    un, us = build_lists(np.concatenate([la, ha]), np.concatenate([lc, hc]), np.concatenate([ld, hd]), len(start), rng)
    return un, us, lvo.ppll_resolve(P, un, us)


def line_runs(c):
    """per pixel the oracle's line entries of mode 3 past the discard: (colour, window depth, key = segment << 6 | triangle)"""
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    P.ppllFragmentSource = 1
    fr = sc.prism_fragments(P)
    off, rgba, z = line_fragments(c)
    key = (fr["seg"].astype(np.uint32) << np.uint32(6)) | fr["tri"].astype(np.uint32)
    return off, rgba[:, 3] >= F(0.001), mlab_colour(rgba), z, key


def hull_keys(c, fr):
    """(numSegs << 6) + triangle: behind every line key, in triangle order"""
    return (np.uint32(len(c.seg)) << np.uint32(6)) + fr["tri"].astype(np.uint32)


def mlab_union(c, fr, K, hull_rgba=None, rng=None):
    """The mode-3 runs with the hull: per pixel the line entries, then the hull entries {mlab_colour, window depth, key}.  Returns
    (runs, the mlab_fold frame (h, w, 4))."""
    off, lkeep, lcol, lz, lkey = line_runs(c)
    hrgba = np.asarray(fr["rgba"] if hull_rgba is None else hull_rgba, dtype=F).reshape(-1, 4)
    hkeep, hcol, hz, hkey = hrgba[:, 3] >= F(0.001), mlab_colour(hrgba), fr["zbits"].view(F), hull_keys(c, fr)
    hoff = hull_runs(fr, c.width * c.height)
    runs = []
    for p in range(c.width * c.height):
        s, h = slice(off[p], off[p + 1]), slice(hoff[p], hoff[p + 1])
        m, n = lkeep[s], hkeep[h]
        run = [np.concatenate([lcol[s][m], hcol[h][n]]), np.concatenate([lz[s][m], hz[h][n]]), np.concatenate([lkey[s][m], hkey[h][n]])]
        if rng is not None:
            o = rng.permutation(len(run[0]))
            run = [a[o] for a in run]
        runs.append(tuple(run))
    return runs, mlab_fold(runs, K, c.background).reshape(c.height, c.width, 4)


# ---------------------------------------------------------------- the checks
def test_order_within_a_run_does_not_matter():
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    assert np.array_equal(camera_position(c), V.cam)
    rng = np.random.default_rng(3)
    nodes, start, frame = ppll_union(c, fr)
    n2, s2, shuffled = ppll_union(c, fr, rng=rng)
    assert not np.array_equal(nodes, n2) and np.array_equal(shuffled, frame)
    without = ppll_union(c, {k: v[:0] for k, v in fr.items()})[2]
    assert (frame != without).any(axis=2).sum() > 1500
    for K in (8, 2):
        runs, fold = mlab_union(c, fr, K)
        assert np.array_equal(mlab_union(c, fr, K, rng=rng)[1], fold)
        assert (fold != mlab_union(c, {k: v[:0] for k, v in fr.items()}, K)[1]).any(axis=2).sum() > 1500


def test_the_depth_sorts_a_hull_node_among_the_line_nodes():
    """one opaque-ish hull fragment on a pixel that holds line fragments, once nearer than all of them and once farther: the two frames
    differ from the frame without it, and from each other, in that pixel only"""
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    off, rgba, z = line_fragments(c)
    counts = np.diff(off)
    p = int(np.argmax(counts))
    assert counts[p] >= 2
    sc = c.oracle_scene()
    P = c.oracle_params(sc)
    nodes, start, _ = sc.ppll_gather(P, use_bvh=True)
    a = pixel_addresses(c, P)[p]
    la, lc, ld = list_entries(nodes, start)
    mine = ld[la == a].view(F)
    assert len(mine) == (rgba[off[p]:off[p + 1], 3] >= F(0.001)).sum() >= 2
    x, y = p % c.width, p // c.width
    ray = np.array([V.cov[y, x][k] for k in range(3)], np.float64)
    ray /= np.linalg.norm(ray)

    def one(dist):
        pos = (V.cam.astype(np.float64) + dist * ray).astype(F)[None, :]
        return dict(pixel=np.array([p], np.uint32), tri=np.zeros(1, np.uint32), zbits=np.zeros(1, np.uint32),
                    rgba=np.array([[0.9, 0.1, 0.1, 0.6]], F), pos=pos, nrm=np.zeros((1, 3), F))

    none = ppll_union(c, {k: v[:0] for k, v in fr.items()})[2]
    front = ppll_union(c, one(float(mine.min()) * 0.5))[2]
    behind = ppll_union(c, one(float(mine.max()) * 1.5))[2]
    for img in (front, behind):
        changed = (img != none).any(axis=2)
        assert changed.sum() == 1 and changed[y, x]
    assert (front[y, x] != behind[y, x]).any()
    # in front, the red fragment weighs 0.6; behind the lines it weighs what they let through
    assert int(front[y, x, 0]) > int(behind[y, x, 0])


def test_every_hull_key_exceeds_every_line_key():
    c, hull, V = hull_case("outside")
    fr = reference_fragments("outside")
    off, lkeep, lcol, lz, lkey = line_runs(c)
    hkey = hull_keys(c, fr)
    assert len(lkey) > 1500 and len(hkey) > 5000
    assert int(lkey.max()) < (len(c.seg) << 6) <= int(hkey.min())
    assert int(hkey.max()) == (len(c.seg) << 6) + int(fr["tri"].max()) < 0xFFFFFFFE
    assert np.array_equal(np.argsort(hkey, kind="stable"), np.argsort(fr["tri"], kind="stable"))


def test_both_depth_metrics_order_the_layers_of_the_closed_box_alike():
    for kind in ("outside", "odd"):
        c, hull, V = hull_case(kind)
        fr = reference_fragments(kind)
        counts = np.bincount(fr["pixel"], minlength=V.w * V.h)
        assert set(np.unique(counts)) <= {0, 2}
        dist = camera_distance(fr["pos"], V.cam)
        zb = fr["zbits"]
        # (the fragments are sorted by pixel: each pixel's two are neighbours)
        a, b = slice(0, None, 2), slice(1, None, 2)
        assert np.array_equal(fr["pixel"][a], fr["pixel"][b])
        assert np.all((dist[a] < dist[b]) == (zb[a] < zb[b])) and np.all(dist[a] != dist[b]) and np.all(zb[a] != zb[b])
        print("closed box %s: %d pixels with two layers, ordered alike by the distance and by the window depth" % (kind, len(zb) // 2))
        assert len(zb) // 2 > 2000
