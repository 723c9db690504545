"""The traversal stack of the ray kernels: a window of LDS slots over a per-thread column of a global slab, spilled and refilled in
blocks (lv_trace.h, LvStackT).

1. lv_selftest_stack runs the stack type of the kernels on scripts, one per thread; every popped word is compared with a plain Python
   list, the number of spills and refills with a window model, so the comparison cannot pass without the slow paths having run.
2. The chain scene of test_deep_lbvh_uses_stack_overflow_slab (a tree far higher than the window) end to end: AO image and traced rays
   bit for bit against the oracle, the frame within LSB_TOL, and the node-visit counters equal to what the per-entry overflow stack
   that preceded the block scheme visited on these scenes.
3. The slab is sized by the stated bound and absent for a tree that fits the window.
"""
import functools

import numpy as np
import pytest

from common import Case, small_case, max_lsb_diff
from linevis_amd import transfer_function as tfm
from oracle import lvo

pytestmark = pytest.mark.gpu

LSB_TOL = 2
INVALID = 0xFFFFFFFF
LEAF = 0x80000000
MARK = 0x7C000000          # a marker has bit 31 clear and bits 26-30 set; references stay below 2^26 (+ the leaf bit)
PUSH3, POP, CLEAR, END = 1, 2, 3, 0
THREADS = 256


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def column_entries(levels, window, block):
    """the slab bound: M = 3 levels + 2 logical entries; a spill needs >= window - 2 entries in the window, so at most
    M - (window - 2) + block entries are ever spilled, in whole blocks; nothing when the window holds M"""
    m = 3 * levels + 2
    return -(-(m - (window - 2) + block) // block) * block if m > window else 0


# ---------------------------------------------------------------- 1. scripts against a list
class Script:
    """Builds one thread's operations and, alongside, what they must produce: `expect` from a plain list (LIFO, nothing else), the
    spill / refill counts from the window bookkeeping (how many entries sit in the window, how many in the slab)."""

    def __init__(self, window, block, max_entries, seed):
        self.W, self.K, self.M = window, block, max_entries
        self.ops, self.expect, self.stack = [], [], []
        self.in_window = self.in_slab = self.spills = self.refills = 0
        self.peak = 0
        self.finished = False
        self.next_ref = seed * 4099 + 1

    def ref(self):
        self.next_ref = (self.next_ref * 2654435761 + 12345) % (1 << 32)
        r = self.next_ref & 0x03FFFFFF
        return r | LEAF if self.next_ref & (1 << 27) else r

    def push3(self, flags, refs=None):
        assert not self.finished and len(self.stack) + bin(flags).count("1") <= self.M
        refs = refs or [self.ref(), self.ref(), self.ref()]
        self.ops.append([PUSH3 | (flags << 8)] + list(refs))
        if self.in_window + 3 > self.W:
            self.in_window -= self.K
            self.in_slab += self.K
            self.spills += 1
        for k in range(3):
            if flags & (1 << k):
                self.stack.append(refs[k])
                self.in_window += 1
        self.peak = max(self.peak, len(self.stack))

    def pop(self):
        assert not self.finished
        self.ops.append([POP, 0, 0, 0])
        if not self.stack:
            self.expect.append(INVALID)
            self.finished = True     # only clear may follow
            return
        if self.in_window == 0:
            self.in_window += self.K
            self.in_slab -= self.K
            self.refills += 1
        self.in_window -= 1
        self.expect.append(self.stack.pop())

    def clear(self):
        self.ops.append([CLEAR, 0, 0, 0])
        self.stack, self.in_window, self.in_slab, self.finished = [], 0, 0, False

    # ---- compound moves
    def grow_by(self, n):
        """n more entries; the odd ones first, so that the last pushes are full ones"""
        if n % 3:
            self.push3((1 << (n % 3)) - 1)
        for _ in range(n // 3):
            self.push3(7)

    def drain(self):
        while self.stack:
            self.pop()
        self.pop()        # the pop that finds the stack empty
        self.clear()


def build_scripts(window, block, max_entries):
    W, K, M = window, block, max_entries
    peaks = [W - 3, W - 2, W - 1, W, W + 1, W + K - 1, W + K, W + 2 * K + 1, M]
    scripts = []
    for t in range(THREADS):
        s = Script(W, K, M, t)
        kind = t % 8
        if kind == 0:                                   # peak occupancies, down through every block boundary to empty
            for p in (peaks[(t // 8) % len(peaks):] + peaks)[:3]:
                s.grow_by(p)
                assert s.peak >= p and len(s.stack) == p
                s.drain()
        elif kind == 1:                                 # boundary ping-pong: pop right after a spill, push3 right after a refill
            s.grow_by(W - 2)
            for _ in range(8):
                before = s.spills
                while s.spills == before:
                    s.push3(7)
                s.pop()
                before = s.refills
                while s.refills == before:
                    s.pop()
                s.push3(5)
            s.drain()
        elif kind == 2:                                 # clear with two blocks spilled, then reuse
            while s.in_slab < 2 * K:
                s.push3(7)
            s.clear()
            s.grow_by(W + 1)
            s.drain()
            s.grow_by(2)
            s.pop()
        elif kind in (3, 4):                            # every combination of keep flags with W - 3 ... W entries in the window
            for entries in ((W - 3, W - 2) if kind == 3 else (W - 1, W)):
                for flags in range(8):
                    s.clear()
                    s.grow_by(entries)
                    assert s.in_window == entries
                    s.push3(flags, refs=[0x03FFFFFF, LEAF | 0x03FFFFFF, LEAF] if flags == 7 else None)
                    s.pop()
                    s.pop()
        elif kind == 5:                                 # never spills: a lane next to lanes that do
            rng = np.random.default_rng(1000 + t)
            for _ in range(120):
                if len(s.stack) + 3 <= W - 3 and rng.random() < 0.55:
                    s.push3(int(rng.integers(0, 8)), refs=[0, LEAF, 1] if len(s.ops) == 0 else None)
                elif s.stack:
                    s.pop()
            assert s.spills == 0
        elif kind == 6:                                 # spills in an iteration of its own: t // 8 idle steps first
            for _ in range(t // 8):
                s.push3(1)
                s.pop()
            s.grow_by(min(W + K + (t // 8) % K, M))
            s.drain()
        else:                                           # seeded random walk, biased towards depth
            rng = np.random.default_rng(t)
            for _ in range(280):
                if s.finished:
                    s.clear()
                    continue
                u = rng.random()
                flags = int(rng.integers(0, 8))
                if u < 0.58 and len(s.stack) + 3 <= M:
                    s.push3(flags)
                elif u < 0.985:
                    s.pop()
                else:
                    s.clear()
        scripts.append(s)
    return scripts


@pytest.mark.parametrize("instantiation", [0, 1], ids=["ao_window", "tile_window"])
def test_scripted_stack_equals_a_list(hip_lib, instantiation):
    ctx = small_case().hip_context()
    info = ctx.selftest_stack(instantiation, 1)[2]
    W, K = info["window"], info["block"]
    levels = -(-(W + 2 * K + 1 - 2) // 3) + 1
    M = 3 * levels + 2
    assert M >= W + 2 * K + 1
    scripts = build_scripts(W, K, M)
    n = max(len(s.ops) for s in scripts)
    assert n <= 330, n
    ops = np.zeros((THREADS, n, 4), dtype=np.uint32)
    for t, s in enumerate(scripts):
        ops[t, :len(s.ops)] = np.array(s.ops, dtype=np.uint64).astype(np.uint32)
    words, counts, info = ctx.selftest_stack(instantiation, levels, ops)
    assert info["column_entries"] == column_entries(levels, W, K)
    # the scripts do what they are here for
    assert max(s.peak for s in scripts) == M
    assert sum(s.spills for s in scripts) > 500 and sum(s.refills for s in scripts) > 300
    for wave in range(THREADS // 64):
        lanes = scripts[64 * wave:64 * wave + 64]
        assert any(s.spills == 0 for s in lanes) and any(s.spills > 0 for s in lanes)
    for t, s in enumerate(scripts):
        got = words[t]
        assert len(got) == len(s.expect), "thread %d: %d words popped, expected %d" % (t, len(got), len(s.expect))
        exp = np.array(s.expect, dtype=np.uint64).astype(np.uint32)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, "thread %d (kind %d), pop %d: %#x, expected %#x" % (t, t % 8, bad[0], got[bad[0]], exp[bad[0]])
        assert not np.any((got < LEAF) & ((got & MARK) == MARK)), "thread %d: a marker word left pop()" % t
        assert (int(counts[t, 1]), int(counts[t, 2])) == (s.spills, s.refills), \
            "thread %d (kind %d): %d spills / %d refills, the model has %d / %d" % (t, t % 8, counts[t, 1], counts[t, 2], s.spills, s.refills)


def test_scripts_outside_the_bound_are_refused(hip_lib):
    from linevis_amd import capi
    ctx = small_case().hip_context()
    W = ctx.selftest_stack(1, 1)[2]["window"]
    ops = np.zeros((THREADS, 40, 4), dtype=np.uint32)
    ops[:, :, 0] = PUSH3 | (7 << 8)
    ops[:, :, 1:] = 5
    with pytest.raises(capi.LineVisError):      # 120 entries, 14 declared
        ctx.selftest_stack(1, 4, ops)
    # a tree whose stack fits the window gets no slab, so a script that would spill all the same is refused: (W - 2) // 3 levels hold
    # at most W entries; W - 2 of them and one more push3 (keeping nothing, so the depth bound is not what refuses it) would spill
    fits = np.zeros((THREADS, W, 4), dtype=np.uint32)
    fits[:, :W - 2, 0] = PUSH3 | (1 << 8)
    fits[:, W - 2, 0] = PUSH3
    fits[:, :, 1:] = 5
    assert 3 * ((W - 2) // 3) + 2 <= W
    assert ctx.selftest_stack(1, (W - 2) // 3, fits[:, :W - 2])[1][:, 1].max() == 0      # up to there it runs, without a spill
    with pytest.raises(capi.LineVisError, match="would spill"):
        ctx.selftest_stack(1, (W - 2) // 3, fits)
    ops[3, 0, 2] = MARK | 8
    with pytest.raises(capi.LineVisError):      # a marker is no reference
        ctx.selftest_stack(1, 60, ops)


# ---------------------------------------------------------------- 2. the chain scene, end to end
def chain_points():
    """test_deep_lbvh_uses_stack_overflow_slab's construction: segment k sits on axis k % 3 at distance 2^-(k // 3 + 1): its Morton key is
    the only one with bit k set first, so every split peels off a single leaf and the tree degenerates into a ~50-level chain"""
    pts, seg = [], []
    for k in range(54):
        a = np.zeros(3)
        a[k % 3] = 0.9 * 2.0 ** (-(k // 3 + 1))
        b = a.copy()
        b[(k + 1) % 3] += 0.3 * 2.0 ** (-(k // 3 + 1))
        seg.append([len(pts), len(pts) + 1])
        pts += [a, b]
    return np.array(pts, dtype=np.float32), np.array(seg, np.uint32)


CHAIN_LINE_WIDTH = 0.0004      # the scene of the old test: hairlines, nearly every sample ray leaves the scene at once
CHAIN_FAT_LINE_WIDTH = 0.01     # added here: tubes wide enough that the sample rays, too, walk down the chain and find occluders


def chain_case(spp, triangles, distance_based, line_width=CHAIN_LINE_WIDTH, **extra):
    pos, seg = chain_points()
    P = np.zeros(len(pos), dtype=lvo.LINE_POINT_DTYPE)
    P["linePosition"] = pos
    P["lineTangent"] = [1, 0, 0]
    P["lineNormal"] = [0, 1, 0]
    P["lineAttribute"] = np.linspace(0, 1, len(pos))
    settings = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
                    ambient_occlusion_samples_per_frame=spp, ambient_occlusion_distance_based=distance_based)
    if triangles:
        settings["rtao_geometry"] = "triangle_tubes"
    settings.update(extra)
    return Case(P, seg, tfm.standard_transparent(), 96, 96, line_width, camera_pos=(0.3, 0.3, 0.9), **settings)


@functools.lru_cache(maxsize=None)
def chain_mesh(line_width=CHAIN_LINE_WIDTH):
    pos, _ = chain_points()
    attr = np.linspace(0, 1, len(pos)).astype(np.float32)
    return lvo.build_tube_triangle_render_data(pos, attr, np.arange(0, len(pos) + 1, 2, dtype=np.uint32), line_width, 6)


def chain_context(case, triangles):
    ctx = case.hip_context()
    if triangles:
        ctx.set_tube_triangle_mesh(*chain_mesh(case.line_width))
    ctx.set_option("accel_build", "fast_build")   # the plain LBVH: the SAH treelets of the default build would balance these leaves
    ctx.build_accel()
    return ctx


@functools.lru_cache(maxsize=None)
def chain_oracle(spp, triangles, distance_based, line_width):
    """(frame, AO image) of the oracle, computed once per configuration"""
    case = chain_case(spp, triangles, distance_based, line_width)
    sc = case.oracle_scene()
    P = case.oracle_params(sc)
    ao = lvo.TriScene(*chain_mesh(case.line_width), case.line_width).render_ao(P, use_bvh=False) if triangles else sc.render_ao(P, use_bvh=False)
    img = sc.render_rt(P, ao=ao, use_bvh=True)
    for a in (img, ao):
        a.setflags(write=False)
    return img, ao


# node visits of the colour pass + the RTAO primaries (nodes_visited) and of the RTAO sample rays (ao_nodes_visited) on these frames, as
# the per-entry overflow stack that preceded the block scheme counted them (recorded once from that build; the traversal order is
# unchanged, so they must not move): (spp, triangles, distance_based, line_width) -> (nodes_visited, ao_nodes_visited)
CHAIN_NODE_VISITS = {
    (8, False, True, CHAIN_LINE_WIDTH): (20866, 40),
    (8, False, False, CHAIN_LINE_WIDTH): (20866, 40),
    (8, True, True, CHAIN_LINE_WIDTH): (22085, 70),
    (8, True, False, CHAIN_LINE_WIDTH): (22085, 70),
    (64, False, True, CHAIN_LINE_WIDTH): (21155, 329),
    (64, False, False, CHAIN_LINE_WIDTH): (21155, 329),
    (64, True, True, CHAIN_LINE_WIDTH): (22536, 521),
    (64, True, False, CHAIN_LINE_WIDTH): (22536, 521),
}

CHAIN_CONFIGS = [(spp, tri, dist, CHAIN_LINE_WIDTH) for spp in (8, 64) for tri in (False, True) for dist in (True, False)] + \
                [(8, False, False, CHAIN_FAT_LINE_WIDTH), (64, True, True, CHAIN_FAT_LINE_WIDTH), (64, False, False, CHAIN_FAT_LINE_WIDTH),
                 (8, True, True, CHAIN_FAT_LINE_WIDTH)]


def chain_stats(spp, triangles, distance_based, line_width=CHAIN_LINE_WIDTH):
    case = chain_case(spp, triangles, distance_based, line_width, collect_stats=True)
    ctx = chain_context(case, triangles)
    ctx.render(11)
    st = ctx.stats()
    return int(st.nodes_visited), int(st.ao_nodes_visited)


@pytest.mark.parametrize("spp,triangles,distance_based,line_width", CHAIN_CONFIGS)
def test_chain_scene_end_to_end(hip_lib, spp, triangles, distance_based, line_width):
    case = chain_case(spp, triangles, distance_based, line_width)
    ctx = chain_context(case, triangles)
    assert ctx.stats().bvh_depth > 32
    img = ctx.render(11)
    ref, ao_ref = chain_oracle(spp, triangles, distance_based, line_width)
    if line_width == CHAIN_FAT_LINE_WIDTH:
        assert (ao_ref < 1.0).sum() > 0     # the sample rays of this scene do find occluders
    assert np.array_equal(bits(ctx.get_ao()), bits(ao_ref))
    assert max_lsb_diff(img, ref) <= LSB_TOL
    info = ctx.selftest_stack(0, 1)[2]
    assert info["context_slab_bytes"] > 0          # the frame's launches had a slab: the tree is higher than the windows
    # The wide-tube frames have no recorded counts: with thousands of sample rays, which wave draws which chunk of them from the
    # launch's queue depends on timing, and with it the bound a lane culls against -- the same build counts a few visits more or less
    # from run to run (8 spp, triangles: 1602 and 1595 of the sample rays' visits).  Their images are compared above, bit for bit.
    if line_width == CHAIN_LINE_WIDTH:
        nodes, ao_nodes = chain_stats(spp, triangles, distance_based, line_width)
        assert (nodes, ao_nodes) == CHAIN_NODE_VISITS[(spp, triangles, distance_based, line_width)]


def test_chain_scene_traced_rays(hip_lib):
    rng = np.random.default_rng(4)
    pos, _ = chain_points()
    tgt = pos.astype(np.float64)[rng.integers(0, len(pos), 5000)] * (1.0 + 1e-3 * rng.normal(size=(5000, 3)))
    o = rng.uniform(-0.1, 0.6, (5000, 3)).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    case = chain_case(8, True, True)
    ctx = chain_context(case, True)
    a = ctx.trace_rays(o, d, 0.0, 10.0)
    assert (a[1] != INVALID).sum() > 300
    b = case.oracle_scene().trace_rays(o, d, 0.0, 10.0, case.line_width)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    ta = ctx.trace_rays_triangles(o, d, 0.0, 10.0)
    tb = lvo.TriScene(*chain_mesh(case.line_width), case.line_width).trace_rays(o, d, 0.0, 10.0, use_bvh=False)
    assert (ta[1] != INVALID).sum() > 300
    assert np.array_equal(bits(ta[0]), bits(tb[0])) and np.array_equal(ta[1], tb[1]) and np.array_equal(bits(ta[2]), bits(tb[2]))


# ---------------------------------------------------------------- 3. the slab bound
def frame_slab_bytes(levels, tri_levels, triangles, spp, width, height, num_cus, ao_info, tile_info):
    """What a full-frame mode-11 RTAO frame (one tile, no halo: the colour rays are not jittered, no denoiser) must reserve: the largest of
    its launches, each blocks x 256 threads x column x 4 bytes.
      tile kernels (colour pass, RTAO primaries): 16 x 16-pixel blocks filling whole 64 x 64 groups, rounded up to 128 workgroups, on
                    the segment tree with the tile kernels' window; launched together (paired primaries) twice that grid
      sample kernel: min(CUs x 5, rays / 256) persistent workgroups -- its slab covers the RTAO primaries' grid as well -- on the tree
                    the sample rays walk, with its own window"""
    col = lambda lv, info: column_entries(lv, info["window"], info["block"])
    grid_tiles = -(-(4 * -(-width // 64)) * (4 * -(-height // 64)) // 128) * 128
    grid_rays = max(min(num_cus * 5, -(-width * height * spp // 256)), 1)
    launches = [grid_tiles * col(levels, tile_info),
                max(grid_rays, grid_tiles) * col(tri_levels if triangles else levels, ao_info)]
    paired = [2 * grid_tiles * col(levels, tile_info)] + ([2 * grid_tiles * col(tri_levels, tile_info)] if triangles else [])
    # the pairing of the primaries is the frame's choice; it must not decide the expectation
    assert max(paired) <= max(launches), (paired, launches)
    return max(launches) * THREADS * 4


@pytest.mark.parametrize("spp,triangles", [(8, False), (64, False), (8, True)])
def test_slab_follows_the_bound(hip_lib, spp, triangles):
    """After a frame the stackOverflow buffer holds exactly blocks x 256 x column x 4 bytes of the frame's largest launch, the column
    being the bound for that launch's window (column_entries) -- and nothing at all for a tree that fits both windows."""
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    shallow = small_case(n_lines=3, pts_per_line=10, ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0,
                         ambient_occlusion_iterations=1, ambient_occlusion_samples_per_frame=spp).hip_context()
    shallow.build_accel()
    shallow.render(11)
    for inst in (0, 1):
        info = shallow.selftest_stack(inst, 1)[2]
        assert column_entries(info["wide_levels"], info["window"], info["block"]) == 0
        assert info["context_slab_bytes"] == 0
    case = chain_case(spp, triangles, True)
    ctx = chain_context(case, triangles)
    assert ctx.selftest_stack(0, 1)[2]["context_slab_bytes"] == 0      # build_accel reserves nothing; the frame does
    ctx.render(11)
    ao, tile = ctx.selftest_stack(0, 1)[2], ctx.selftest_stack(1, 1)[2]
    levels, tri_levels = ao["wide_levels"], ao["triangle_wide_levels"]
    assert 3 * levels + 2 > tile["window"] > ao["window"]
    for info, inst in ((ao, 0), (tile, 1)):       # the library's column is the bound
        assert ctx.selftest_stack(inst, levels)[2]["column_entries"] == column_entries(levels, info["window"], info["block"]) > 0
    assert ao["context_slab_bytes"] == frame_slab_bytes(levels, tri_levels, triangles, spp, case.width, case.height, num_cus, ao, tile)
