"""Rendering mode 10 (Atomic Loop 64) on the CPU: al64_fold is the vectorised numpy statement of the mode -- the K smallest keys of a
pixel in its slots, the rest in five integer tail sums, the resolve in float32 one operation at a time (include/linevis_hip.h,
atomic_loop_num_layers).  Checked against a scalar transcription of the gather loop
(AtomicLoop64Gather.glsl:70-79) fed sequentially in random arrival orders and against the plain front-to-back blend."""
import numpy as np
import pytest

from test_mboit_restatement import exp_det, from_fixed, log_det, to_fixed
from test_mlab_restatement import pack, unpack

F = np.float32
U64 = np.uint64
EMPTY = U64(0xFFFFFFFFFFFFFFFF)
MAX_COUNT = 131071


def al64_key(depth, colour):
    """(window depth bits << 32) | packUnorm4x8(straight colour)"""
    return (np.asarray(depth, dtype=F).view(np.uint32).astype(U64) << U64(32)) | np.asarray(colour, dtype=np.uint32).astype(U64)


def tail_terms():
    """term(a8) of the tail's absorbance sum for the 256 values of a8, int64 fixed point"""
    a8 = np.arange(256)
    with np.errstate(all="ignore"):
        t = to_fixed(-log_det(F(1.0) - a8.astype(F) / F(255.0)))
    t[0] = 0
    t[255] = to_fixed(F(1024.0))
    return t


TERMS = tail_terms()


def al64_resolve(slots, tail, background):
    """slots (P, K) uint64 ascending then EMPTY, tail (P, 5) uint64 -> (P, 4) uint8"""
    P, K = slots.shape
    bg = np.asarray(background, dtype=F)
    col = [np.zeros(P, F) for _ in range(3)]
    T = np.ones(P, F)
    live = np.ones(P, bool)
    for i in range(K):
        live = live & (slots[:, i] != EMPTY)   # (the loop breaks at the first empty slot)
        r, g, b, a = unpack((slots[:, i] & U64(0xFFFFFFFF)).astype(np.uint32))
        wgt = (T * a).astype(F)
        for k, ch in enumerate((r, g, b)):
            col[k] = np.where(live, (col[k] + (wgt * ch).astype(F)).astype(F), col[k])
        T = np.where(live, (T * (F(1.0) - a)).astype(F), T).astype(F)
    sa = tail[:, 0]
    has_tail = sa != 0
    with np.errstate(all="ignore"):
        at = (F(1.0) - exp_det(-from_fixed(tail[:, 4].astype(np.int64)))).astype(F)
        fsa = sa.astype(F)
        fb = []
        for k in range(3):
            ct = ((tail[:, 1 + k].astype(F) / fsa).astype(F) / F(255.0)).astype(F)
            fb.append(np.where(has_tail, ((ct * at).astype(F) + (bg[k] * (F(1.0) - at)).astype(F)).astype(F), bg[k]).astype(F))
        fb.append(np.where(has_tail, (at + (bg[3] * (F(1.0) - at)).astype(F)).astype(F), bg[3]).astype(F))
        a = (F(1.0) - T).astype(F)
        out = []
        for k in range(3):
            v = (((col[k] / a).astype(F) * a).astype(F) + (fb[k] * (F(1.0) - a)).astype(F)).astype(F)
            out.append(np.where(a > F(0.0), v, fb[k]))
        out.append(np.where(a > F(0.0), (a + (fb[3] * (F(1.0) - a)).astype(F)).astype(F), fb[3]))
    p = pack(out)
    return np.stack([(p >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=1).astype(np.uint8)


def al64_fold(runs, K, background):
    """runs: one uint64 key array per pixel, in any order.  Returns ((P, 4) uint8, (P, K) uint64 slots, (P, 5) uint64 tail sums
    {SA, SR, SG, SB, SL})."""
    P = len(runs)
    n = np.array([len(r) for r in runs], dtype=np.int64)
    assert n.max(initial=0) <= MAX_COUNT
    off = np.zeros(P + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    keys = np.concatenate([np.asarray(r, dtype=U64) for r in runs]) if off[-1] else np.zeros(0, U64)
    pix = np.repeat(np.arange(P), n)
    order = np.lexsort((keys, pix))
    keys = keys[order]
    rank = np.arange(len(keys)) - off[pix]
    slots = np.full((P, K), EMPTY, dtype=U64)
    front = rank < K
    slots[pix[front], rank[front]] = keys[front]
    c = (keys & U64(0xFFFFFFFF)).astype(np.uint32)
    ch = [((c >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.int64) for k in range(4)]
    a8 = ch[3]
    terms = [a8, a8 * ch[0], a8 * ch[1], a8 * ch[2], TERMS[a8]]
    first = off[:-1] + np.minimum(n, K)   # the tail of pixel p: sorted keys [first[p], off[p + 1])
    tail = np.zeros((P, 5), dtype=U64)
    for k, t in enumerate(terms):
        cs = np.concatenate([[0], np.cumsum(t, dtype=np.int64)])
        tail[:, k] = (cs[off[1:]] - cs[first]).astype(U64)
    return al64_resolve(slots, tail, background), slots, tail


# ---------------------------------------------------------------- the scalar transcription
def gather_scalar(keys, K):
    """the gather loop for one pixel, the keys inserted one after the other in the given order"""
    E = int(EMPTY)
    slots = [E] * K
    tail = [0] * 5
    for v in (int(k) for k in keys):
        carried = True
        for i in range(K):
            old = slots[i]
            slots[i] = min(old, v)
            if old == E:
                carried = False
                break
            if old > v:
                v = old
        if carried:
            c = v & 0xFFFFFFFF
            r8, g8, b8, a8 = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF, c >> 24
            for k, t in enumerate((a8, a8 * r8, a8 * g8, a8 * b8, int(TERMS[a8]))):
                tail[k] += t
    return slots, tail


def resolve_scalar(slots, tail, background):
    bg = [F(x) for x in background]
    col = [F(0.0)] * 3
    T = F(1.0)
    for v in slots:
        if v == int(EMPTY):
            break
        c = v & 0xFFFFFFFF
        r, g, b, a = (F((c >> (8 * k)) & 0xFF) / F(255.0) for k in range(4))
        wgt = F(T * a)
        col = [F(col[k] + F(wgt * ch)) for k, ch in enumerate((r, g, b))]
        T = F(T * F(F(1.0) - a))
    fb = list(bg)
    if tail[0] != 0:
        at = F(F(1.0) - exp_det(F(-from_fixed(np.int64(tail[4]))))[()])
        fsa = F(np.uint64(tail[0]))
        for k in range(3):
            ct = F(F(F(np.uint64(tail[1 + k])) / fsa) / F(255.0))
            fb[k] = F(F(ct * at) + F(bg[k] * F(F(1.0) - at)))
        fb[3] = F(at + F(bg[3] * F(F(1.0) - at)))
    a = F(F(1.0) - T)
    out = list(fb)
    if a > F(0.0):
        for k in range(3):
            out[k] = F(F(F(col[k] / a) * a) + F(fb[k] * F(F(1.0) - a)))
        out[3] = F(a + F(fb[3] * F(F(1.0) - a)))
    return [int(np.floor(min(max(x, F(0.0)), F(1.0)) * F(255.0) + F(0.5))) for x in out]


# ---------------------------------------------------------------- runs
def random_runs(rng, num_pixels, K, max_factor=3):
    """runs of 0 ... max_factor * K keys; among them empty pixels, duplicated keys, equal depths with different colours, a8 = 0 and
    a8 = 255"""
    runs = []
    for p in range(num_pixels):
        n = int(rng.integers(0, max_factor * K + 1))
        if p % 7 == 3:
            n = 0
        depth = rng.random(n).astype(F)
        colour = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if n >= 2 and p % 5 == 1:      # equal depths, different colours
            depth[: n // 2] = depth[0]
        if n >= 1 and p % 4 == 0:      # a8 = 0 and a8 = 255
            colour[::3] &= np.uint32(0x00FFFFFF)
            colour[1::3] |= np.uint32(0xFF000000)
        keys = al64_key(depth, colour)
        if n >= 3 and p % 3 == 2:      # duplicated keys
            keys[n // 2:] = keys[: n - n // 2][: len(keys[n // 2:])]
        runs.append(keys)
    return runs


BG = (0.1, 0.2, 0.3, 1.0)


def test_tail_terms_are_the_definition():
    assert TERMS[0] == 0 and TERMS[255] == 1024 << 36
    assert np.all(np.diff(TERMS[:255]) > 0) and TERMS[254] < TERMS[255]
    assert TERMS[128] == int(to_fixed(-log_det(F(1.0) - F(128.0) / F(255.0))))
    assert MAX_COUNT * int(TERMS[255]) < 1 << 63 <= (MAX_COUNT + 1) * int(TERMS[255])


@pytest.mark.parametrize("K", [1, 3, 8])
def test_fold_equals_the_gather_loop_in_any_arrival_order(K):
    rng = np.random.default_rng(100 + K)
    runs = random_runs(rng, 48, K)
    assert any(len(r) == 0 for r in runs) and any(len(r) > K for r in runs)
    assert any(len(np.unique(r)) < len(r) for r in runs)
    img, slots, tail = al64_fold(runs, K, BG)
    for p, keys in enumerate(runs):
        for _ in range(20):
            s, t = gather_scalar(rng.permutation(keys), K)
            assert s == [int(x) for x in slots[p]], p
            assert t == [int(x) for x in tail[p]], p
        assert resolve_scalar([int(x) for x in slots[p]], [int(x) for x in tail[p]], BG) == [int(x) for x in img[p]], p
    live = slots != EMPTY
    assert np.all(slots[:, :-1] <= slots[:, 1:]) and np.all(live[:, :-1] | ~live[:, 1:])


def test_fold_is_the_front_to_back_blend_when_nothing_is_carried():
    """every run at most K long: no tail, and the frame is the plain blend of the sorted fragments over the background"""
    rng = np.random.default_rng(7)
    K = 8
    runs = random_runs(rng, 64, K, max_factor=1)
    img, slots, tail = al64_fold(runs, K, BG)
    assert not tail.any()
    for p, keys in enumerate(runs):
        col, T = [F(0.0)] * 3, F(1.0)
        for v in sorted(int(k) for k in keys):
            c = v & 0xFFFFFFFF
            r, g, b, a = (F((c >> (8 * k)) & 0xFF) / F(255.0) for k in range(4))
            col = [F(col[k] + F(F(T * a) * ch)) for k, ch in enumerate((r, g, b))]
            T = F(T * F(F(1.0) - a))
        a = F(F(1.0) - T)
        out = [F(x) for x in BG]
        if a > F(0.0):
            out = [F(F(F(col[k] / a) * a) + F(F(BG[k]) * F(F(1.0) - a))) for k in range(3)] + [F(a + F(F(BG[3]) * F(F(1.0) - a)))]
        assert [int(np.floor(min(max(x, F(0.0)), F(1.0)) * F(255.0) + F(0.5))) for x in out] == [int(x) for x in img[p]], p


def test_deep_pixel_and_identical_keys():
    rng = np.random.default_rng(3)
    keys = al64_key(rng.random(5000).astype(F), rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32))
    keys[1000:2000] = keys[0]
    for K in (1, 8, 64):
        img, slots, tail = al64_fold([keys, keys[:0]], K, BG)
        s, t = gather_scalar(rng.permutation(keys), K)
        assert s == [int(x) for x in slots[0]] and t == [int(x) for x in tail[0]]
        assert np.all(slots[1] == EMPTY) and not tail[1].any()
        assert [int(x) for x in img[1]] == [26, 51, 77, 255]
