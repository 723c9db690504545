"""The float32 / uint32 restatement of the spatial-hashing denoiser (tests/sh_restatement.py) against first principles: the hash
against plain integers, the exponent rule of the cell size against math.frexp, truncation and floor at the signed zeros, accumulation
over frames and what a camera move does to the keys.  No GPU; tests/test_gpu_spatial_hashing.py compares the kernels with it."""
import math

import numpy as np

import sh_restatement as sh

F = np.float32


def test_wang_hash_against_plain_integers():
    def reference(seed):   # SH_Denoise.glsl:58-65 with explicit modular arithmetic
        seed = ((seed ^ 61) ^ (seed >> 16)) % 2**32
        seed = (seed * 9) % 2**32
        seed = (seed ^ (seed >> 4)) % 2**32
        seed = (seed * 0x27d4eb2d) % 2**32
        return (seed ^ (seed >> 15)) % 2**32
    for seed in (0, 1, 61, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 123456789):
        assert sh.wang_hash(seed) == reference(seed)
    assert sh.wang_hash(0) == reference(0) != 0
    # an argument that wrapped: the callers add two 32-bit words before hashing
    assert sh.wang_hash(0xFFFFFFFF + 5) == sh.wang_hash(4)
    # the published avalanche behaviour in miniature: neighbouring seeds land far apart
    assert len({sh.wang_hash(i) for i in range(4096)}) == 4096


def test_cell_size_takes_the_binary_exponent_of_the_quotient():
    P = sh.Params((0.0, 0.0, 0.0), 16, s_p=8.0, s_min_exp=-3)
    # distances whose quotient straddles powers of two: one ulp below, at, and one ulp above
    for target in (1.0, 2.0, 4.0, 1024.0, 0.5):
        want_quot = F(target)
        # solve dis * tan_sp / s_min = target for a point on the x axis, then step through neighbouring floats
        x0 = F(want_quot * P.s_min / P.tan_sp)
        seen = set()
        for steps in range(-3, 4):
            x = x0
            for _ in range(abs(steps)):
                x = np.nextafter(x, F(np.inf) if steps > 0 else F(-np.inf))
            quot = F(F(x * P.tan_sp) / P.s_min)      # length of (x, 0, 0) is exactly |x|
            mant, exp = math.frexp(float(quot))      # quot = mant * 2^exp, mant in [0.5, 1)
            assert sh.log_step(P, (x, 0.0, 0.0)) == exp - 1
            assert sh.cell_size(P, (x, 0.0, 0.0)) == F(math.ldexp(float(P.s_min), exp - 1))
            seen.add(exp - 1)
        assert len(seen) == 2, (target, seen)        # the steps really crossed the power of two
    # a hit at the camera (quotient 0), one whose quotient is denormal and one at infinity are skipped
    assert sh.log_step(P, (0.0, 0.0, 0.0)) is None and sh.hit_keys(P, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)) is None
    assert sh.log_step(P, (1e-42, 0.0, 0.0)) is None
    assert sh.log_step(P, (3e38, 3e38, 0.0)) is None
    assert sh.hit_keys(P, (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)) is None      # a miss


def test_normals_truncate_toward_zero_and_floor_keeps_the_signed_zero():
    P = sh.Params((0.0, 0.0, 0.0), 16)
    n = np.array([-1.0, 2.0, -3.0]) / math.sqrt(14.0)            # * 3 = (-0.80, 1.60, -2.41) -> (0, 1, -2), not (-1, 1, -3)
    assert sh.normal_words(P, n) == [sh.bits(0.0), sh.bits(1.0), sh.bits(-2.0)]
    assert sh.normal_words(P, -n) == [sh.bits(0.0), sh.bits(-1.0), sh.bits(2.0)]      # -0.80 truncates to +0: the int has no -0
    assert sh.normal_words(P, (0.0, 0.0, 5.0)) == [0, 0, sh.bits(3.0)]                 # normalised before the scale
    # floor(-0.0) = -0.0 and floor(-tiny) = -1: three different words, so three different cells along an axis
    assert sh.bits(np.floor(F(-0.0))) == 0x80000000 and sh.bits(np.floor(F(0.0))) == 0
    nw = sh.normal_words(P, (0.0, 0.0, 1.0))
    s = F(0.25)
    keys = {sh.key_word(P, (x, 0.3, 0.3), nw, s) for x in (F(0.0), F(-0.0), F(-1e-30), F(0.24), F(-0.24))}
    assert len(keys) == 3
    assert sh.key_word(P, (F(0.0), 0.3, 0.3), nw, s) == sh.key_word(P, (F(0.24), 0.3, 0.3), nw, s)
    assert sh.key_word(P, (F(-1e-30), 0.3, 0.3), nw, s) == sh.key_word(P, (F(-0.24), 0.3, 0.3), nw, s)
    # a cell size below s_min is clamped: both levels give the same key
    assert sh.key_word(P, (0.1, 0.2, 0.3), nw, F(1e-20)) == sh.key_word(P, (0.1, 0.2, 0.3), nw, F(1e-19))
    # hash and checksum are different functions of the same words
    k = sh.key_word(P, (0.1, 0.2, 0.3), nw, s)
    assert (k >> 32) != (k & sh.M32)


def test_quantisation_rounds_half_up_and_clamps():
    assert [sh.quantise(v) for v in (0.0, 1.0, 0.004, 0.005, 0.125, 0.995, 2.0, -1.0, float("nan"))] == \
        [0, 100, 0, int(np.floor(F(F(F(0.005) * F(100)) + F(0.5)))), 13, 100, 100, 0, 0]


def test_two_frames_accumulate_and_a_camera_move_keeps_the_old_cells():
    noisy, normal, position = sh.given_maps()
    hits = int(np.count_nonzero(np.any(normal[:, :, :3] != 0.0, axis=2)))
    A = sh.Params(sh.CAMERAS[0], 16, num_cells=65536)
    B = sh.Params(sh.CAMERAS[1], 16, num_cells=65536)
    steps = {sh.log_step(A, position[y, x, :3]) for y in range(16) for x in range(24) if normal[y, x, :3].any()}
    assert len(steps) >= 3, steps
    cells = {}
    r1 = sh.denoise(A, cells, noisy, normal, position)
    one = sh.cells_as_set(cells)
    assert sum(c for _, _, c in one) == 4 * hits and len(one) >= 40
    assert (r1[7:9] == 0.0).all() and (r1[:7] > 0.0).any() and (r1 <= 1.0).all()
    r2 = sh.denoise(A, cells, noisy * F(0.5), normal, position)
    two = sh.cells_as_set(cells)
    assert {k for k, _, _ in two} == {k for k, _, _ in one}                       # same camera: same keys, twice the counts
    assert all(cells[k][1] == 2 * c for k, _, c in one)
    assert not np.array_equal(r1, r2)
    # another camera: other cell sizes, hence other level-0 keys; the cells of the first two frames stay what they were
    ka = sh.hit_keys(A, position[12, 5, :3], normal[12, 5, :3])
    kb = sh.hit_keys(B, position[12, 5, :3], normal[12, 5, :3])
    assert ka[0] != kb[0]
    sh.denoise(B, cells, noisy, normal, position)
    three = {k: tuple(v) for k, v in cells.items()}
    # (a coarse level under one camera can be a fine one under the other: such cells are shared and grow)
    keys_b = {k for y in range(16) for x in range(24) for k in (sh.hit_keys(B, position[y, x, :3], normal[y, x, :3]) or [])}
    untouched = [(k, s, c) for k, s, c in two if k not in keys_b]
    assert untouched and all(three[k] == (s, c) for k, s, c in untouched)
    assert len(three) > len(two) and sum(v[1] for v in three.values()) == 12 * hits


def test_run_bound_of_the_probe_windows():
    keys = [sh.key_word(sh.Params((0, 0, 0), 16), (0.1 * i, 0.2, 0.3), [0, 0, sh.bits(3.0)], F(0.05)) for i in range(8)]
    assert sh.max_occupied_run(keys, 16) is not None and sh.max_occupied_run(keys, 16) <= 8
    assert sh.max_occupied_run(keys, 65536) <= 8
    # more keys than slots cannot all be stored
    many = [sh.key_word(sh.Params((0, 0, 0), 16), (0.1 * i, 0.2, 0.3), [0, 0, sh.bits(3.0)], F(0.05)) for i in range(40)]
    assert len(set(many)) == 40 and sh.max_occupied_run(many, 12) is None
