"""Device arithmetic the parity contract rests on: sequences that are shorter than the compiler's but must give the same
bits, and -- function by function -- every scalar definition the build owns, evaluated on the device by the inline functions the
render kernels call (lv_selftest_eval) and compared with the CPU checker's statement of the same function, bit for bit.  A parity
failure in a frame test should be looked for here first.  Argument sets and domain predicates: tests/math_args.py."""
import os

import numpy as np
import pytest

import math_args as A
import test_mboit_restatement as mboit
from common import GOLDEN_DIR
from linevis_amd import capi
from oracle import lvo

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
LV_E_INVALID = -1   # include/linevis_hip.h


def test_shortened_rsqrt_gives_the_ieee_bits_for_every_float(hip_lib):
    """lv_rsqrt_shade (lv_device.h: the argument clamped into [2^-60, 2^60], then v_sqrt_f32 + one-ulp correction and v_rcp_f32 + three
    Newton steps) against lv_rsqrt_shade_reference -- the same clamp followed by the compiler's own 1.0f / sqrtf(x) -- for ALL 2^32
    arguments: zeros, denormals, infinities, NaNs, negatives included.  The CPU checker's normalizeShade states the same clamped rule
    (and counts the calls the clamp acts on: tests/test_oracle.py); a single differing bit would show up as a parity failure
    somewhere else, far from its cause."""
    ctx = capi.Context(0)
    bad, first = ctx.selftest_rsqrt()
    assert bad == 0, "%d arguments differ, e.g. bits 0x%08x" % (bad, first)


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = capi.Context(0)
    yield c
    c.close()


def _hex(row):
    return "(" + ", ".join("0x%08x" % int(v) for v in np.atleast_1d(row)) + ")"


def assert_same_words(name, args, got, want, float_results=True, excluded=None):
    """device words == host words for every argument row (two NaNs count as equal whatever their payload or sign: the rule of
    lv_selftest_rsqrt); the message names the first offending argument by its bits"""
    args = np.asarray(args).reshape(len(got), -1)
    same = got == want
    if float_results:
        same |= np.isnan(got.view(F)) & np.isnan(want.view(F))
    bad = ~same.all(axis=1)
    if excluded is not None:
        bad &= ~excluded
    n = int(bad.sum())
    print("%s: %d arguments, %d excluded by predicate, %d differ" % (name, len(got), 0 if excluded is None else int(excluded.sum()), n))
    if n:
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d arguments differ, first: argument bits %s -> device %s, host %s"
                             % (name, n, len(got), _hex(args[i]), _hex(got[i]), _hex(want[i])))


def both(ctx, name, words, **host):
    words = np.ascontiguousarray(words, dtype=U)
    return ctx.selftest_eval(name, words), lvo.eval_words(name, words, **host)


# ---------------------------------------------------------------- the entry point itself
def test_entry_point_rejects_what_it_cannot_evaluate(ctx):
    import ctypes as C
    w = np.zeros(4, dtype=U)
    L = ctx.L
    assert L.lv_selftest_eval(ctx.h, 0, w.ctypes.data_as(C.c_void_p), 1, w.ctypes.data_as(C.c_void_p)) == LV_E_INVALID
    assert L.lv_selftest_eval(ctx.h, 21, w.ctypes.data_as(C.c_void_p), 1, w.ctypes.data_as(C.c_void_p)) == LV_E_INVALID
    assert L.lv_selftest_eval(ctx.h, 1, None, 1, w.ctypes.data_as(C.c_void_p)) == LV_E_INVALID
    assert L.lv_selftest_eval(ctx.h, 1, w.ctypes.data_as(C.c_void_p), 1, None) == LV_E_INVALID
    out = np.full(4, 0xDEADBEEF, dtype=U)
    assert L.lv_selftest_eval(ctx.h, 1, w.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p)) == capi.LV_OK
    assert (out == 0xDEADBEEF).all()
    assert sorted(v[0] for v in capi.SELFTEST_FUNCTIONS.values()) == list(range(1, 21))
    for name, shape in lvo.EVAL_FUNCTIONS.items():
        assert capi.SELFTEST_FUNCTIONS[name] == shape
    fresh = capi.Context(0)   # the two table readers need their table
    for name in ("transfer_function", "twist_sample"):
        with pytest.raises(capi.LineVisError):
            fresh.selftest_eval(name, np.zeros((1, capi.SELFTEST_FUNCTIONS[name][1]), dtype=U))
    fresh.close()


# ---------------------------------------------------------------- unary float functions
def test_sincos2pi(ctx):
    """every float except finite |xi| >= 2^29 (math_args.sincos2pi_outside_domain): there the quadrant int(floor(4 xi)) does not fit
    an int -- the device saturates (quadrant 3), x86 answers INT_MIN (quadrant 0); no caller gets there"""
    w = A.unary_words("sincos2pi")
    out = A.sincos2pi_outside_domain(w)
    assert not A.sincos2pi_outside_domain(A.f2w(A.call_domain("sincos2pi"))).any()
    got, want = both(ctx, "sincos2pi", w)
    assert_same_words("sincos2pi", w, got, want, excluded=out)


@pytest.mark.parametrize("name", ["sincos_rad", "log2_det", "exp2_det", "rsqrt_shade"])
def test_unary_definitions(ctx, name):
    w = A.unary_words(name)
    got, want = both(ctx, name, w)
    assert_same_words(name, w, got, want)


def test_atan2_det(ctx):
    w = A.atan2_words()
    got, want = both(ctx, "atan2_det", w)
    assert_same_words("atan2_det", w, got, want)


def test_pow_det(ctx):
    w = A.pow_words()
    got, want = both(ctx, "pow_det", w)
    assert_same_words("pow_det", w, got, want)
    e = A.unary_words("exp2_det")      # lv_exp2_det(p) is lv_pow_det(2, p), bit for bit
    two = np.stack([np.full_like(e, A.f2w(F(2.0))[0]), e], axis=1)
    assert_same_words("pow_det(2, p) against exp2_det(p)", two, ctx.selftest_eval("pow_det", two), ctx.selftest_eval("exp2_det", e))


# ---------------------------------------------------------------- RNG
def test_tea_and_rnd(ctx):
    g = np.load(os.path.join(GOLDEN_DIR, "rng_kat.npz"))
    assert np.array_equal(ctx.selftest_eval("tea", g["tea_in"])[:, 0], g["tea_out"])
    seeds = g["rnd_seeds"].astype(U)
    for step in range(8):
        r = ctx.selftest_eval("rnd", seeds)
        assert np.array_equal(r[:, 1], g["rnd_bits"][:, step]), step
        seeds = r[:, 0].copy()
    pairs = A.random_words(2 << 20, 0x7EA).reshape(-1, 2)
    got, want = both(ctx, "tea", pairs)
    assert_same_words("tea", pairs, got, want, float_results=False)
    # chains of 256 steps from 4096 seeds (tea outputs, as the kernels seed them): each side feeds on its own state
    dev = host = want[:4096, 0].copy()
    start = dev.copy()
    for step in range(256):
        d, h = ctx.selftest_eval("rnd", dev), lvo.eval_words("rnd", host)
        if not np.array_equal(d, h):
            assert_same_words("rnd, step %d of the chains" % step, dev, d, h, float_results=False)
        dev, host = d[:, 0].copy(), h[:, 0].copy()
    assert not np.array_equal(dev, start)
    edge = np.array([0, 1, 0xFFFFFFFF, 0x80000000, 0x00FFFFFF, 0x01000000], dtype=U)
    got, want = both(ctx, "rnd", np.concatenate([edge, A.random_words(1 << 20, 0x7EB)]))
    assert_same_words("rnd", np.concatenate([edge, A.random_words(1 << 20, 0x7EB)]), got, want, float_results=False)
    v = got[:, 1].view(F)
    assert (v >= 0).all() and (v < 1).all()


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("n", A.TF_SIZES)
def test_transfer_function(ctx, n):
    """every float attribute under every range, attrMin == attrMax and infinite bounds included: the position is clamped into [0, 1]
    (a NaN position counts as 0) before anything is converted to an index, so nothing is excluded"""
    tf = A.tf_table(n)
    for lo, hi in A.TF_RANGES:
        ctx.set_transfer_function(tf, lo, hi)
        w = A.tf_attributes(n, lo, hi)
        got, want = both(ctx, "transfer_function", w, tf=tf, attr_min=lo, attr_max=hi)
        assert_same_words("transfer_function, %d texels, range (%g, %g)" % (n, lo, hi), w, got, want)


@pytest.mark.parametrize("wh", A.TWIST_TEXTURES, ids=lambda wh: "%dx%d" % wh)
def test_twist_sample(ctx, wh):
    """all six filtering modes; u far outside the int range of the texel coordinate, +-inf and NaN included (the coordinate goes
    through the saturating conversion lv_f2i_sat / f2iSat on both sides)"""
    w, h = wh
    img = A.twist_texture(w, h)
    ctx.set_twist_line_texture(img)
    words = A.twist_words(w, h)
    for mode, mode_name in enumerate(lvo.TWIST_FILTER_MODES):
        ctx.set_option("twist_line_texture_filtering_mode_index", mode)
        with lvo.twist_line_texture(img, mode_name):
            got, want = both(ctx, "twist_sample", words)
        assert_same_words("twist_sample %d x %d, %s" % (w, h, mode_name), words, got, want)
    ctx.set_twist_line_texture(None)


# ---------------------------------------------------------------- packings and the frame's store
def test_packings_and_the_rgba8_store(ctx):
    p = A.unpack_words()
    got, want = both(ctx, "unpack_unorm4x8", p)
    assert_same_words("unpack_unorm4x8", p, got, want)
    back, back_host = both(ctx, "pack_unorm4x8", got)
    assert_same_words("pack_unorm4x8 of the unpacked words", got, back, back_host, float_results=False)
    assert np.array_equal(back[:, 0], p)                      # unpack then pack is the identity on all sampled words
    c = A.pack_words()
    for name in ("pack_unorm4x8", "store_rgba8"):
        got, want = both(ctx, name, c)
        assert_same_words(name, c, got, want, float_results=False)
    assert np.array_equal(ctx.selftest_eval("store_rgba8", c), ctx.selftest_eval("pack_unorm4x8", c))


# ---------------------------------------------------------------- MBOIT fixed point (host twin: tests/test_mboit_restatement.py)
def test_mboit_fixed_point(ctx):
    w = A.unary_words("mboit_fixed")
    got = ctx.selftest_eval("mboit_fixed", w)
    want = np.ascontiguousarray(mboit.to_fixed(A.w2f(w))).view(U).reshape(-1, 2)
    assert_same_words("mboit_fixed", w, got, want, float_results=False)
    s = A.mboit_sums()
    got = ctx.selftest_eval("mboit_unfixed", s)
    want = mboit.from_fixed(np.ascontiguousarray(s).view(np.int64).reshape(-1)).view(U).reshape(-1, 1)
    assert_same_words("mboit_unfixed", s, got, want)
    fixed = np.ascontiguousarray(mboit.to_fixed(A.w2f(w))).view(U).reshape(-1, 2)   # ... and of every term's own fixed-point word
    assert_same_words("mboit_unfixed(mboit_fixed)", fixed, ctx.selftest_eval("mboit_unfixed", fixed),
                      mboit.from_fixed(fixed.view(np.int64).reshape(-1)).view(U).reshape(-1, 1))
    w = A.unary_words("mboit_saturate")
    got = ctx.selftest_eval("mboit_saturate", w)
    with np.errstate(invalid="ignore"):
        want = mboit.saturate(A.w2f(w)).view(U).reshape(-1, 1)
    assert_same_words("mboit_saturate", w, got, want)


# ---------------------------------------------------------------- shading_numerics = fast: accuracy against float64
def _ulps(got, exact):
    """|got - exact| in units of the spacing of float32 at the float64 result rounded to float32"""
    ref = exact.astype(F)
    return np.abs(got.astype(np.float64) - exact) / np.spacing(np.abs(ref)).astype(np.float64)


def _quotient_pairs():
    """quotients a / b with both magnitudes in [2^-20, 2^20] and seeded mantissas, a of both signs: fragment depths over line widths,
    viewport heights and depth ranges (the divisions of the lighting code) -- every result is a normal float"""
    rng = np.random.default_rng(0xD1F)
    m = (2.0 ** np.linspace(-20.0, 20.0, 2048) * (1.0 + rng.random(2048) * 0.5)).astype(F)
    a, b = np.meshgrid(np.concatenate([m[::2], -m[1::2]]), m, indexing="ij")
    return a.reshape(-1), b.reshape(-1)


def test_fast_rsqrt_and_reciprocal_within_one_ulp(ctx):
    """DESIGN.md 4 rests the +-2 LSB contract of shading_numerics = fast on "<= 1 ulp" for v_rsq_f32 and v_rcp_f32: measured here
    against float64.  lv_rsqrt_fast over the unary set clamped into [2^-60, 2^60] (it clamps its argument); the reciprocal as
    lv_div_fast(1, b) over the same set and the divisors of _quotient_pairs() (as the plain product 1 * v_rcp_f32(b) it measured
    0.868 ulp; lv_div_fast refines it by one residual step).  Measured on an MI355X: DESIGN.md 4."""
    x = A.w2f(A.unary_words("rsqrt_fast"))
    x = np.unique(np.clip(x[~np.isnan(x)], F(2.0 ** -60), F(2.0 ** 60)))
    got = ctx.selftest_eval("rsqrt_fast", A.f2w(x))[:, 0].view(F)
    e = _ulps(got, 1.0 / np.sqrt(x.astype(np.float64)))
    i = int(np.argmax(e))
    print("rsqrt_fast: max %.4f ulp at argument bits 0x%08x over %d arguments" % (e[i], A.f2w(x)[i], len(x)))
    assert e[i] <= 1.0, "rsqrt_fast: %.4f ulp at argument bits 0x%08x" % (e[i], A.f2w(x)[i])
    b = np.unique(np.concatenate([_quotient_pairs()[1], x]))
    ob = np.stack([np.full(len(b), A.f2w(F(1.0))[0], dtype=U), A.f2w(b)], axis=1)
    got = ctx.selftest_eval("div_fast", ob)[:, 0].view(F)
    e = _ulps(got, 1.0 / b.astype(np.float64))
    i = int(np.argmax(e))
    print("div_fast(1, b): max %.4f ulp at argument bits 0x%08x over %d arguments" % (e[i], A.f2w(b)[i], len(b)))
    assert e[i] <= 1.0, "div_fast(1, b): %.4f ulp at argument bits 0x%08x" % (e[i], A.f2w(b)[i])


def test_fast_division_within_one_ulp(ctx):
    """lv_div_fast(a, b) against float64 a / b over _quotient_pairs(), bar: 1 ulp (DESIGN.md 4's figure).  The plain product
    a * v_rcp_f32(b) misses it -- 1.9782 ulp at argument bits (0x39ebff21, 0x3e6fdd3f): the reciprocal stays within its ulp
    (test_fast_rsqrt_and_reciprocal_within_one_ulp) but the product rounds once more -- which is why lv_div_fast carries one
    residual step.  Measured on an MI355X: DESIGN.md 4.  Then the arguments where that step has no value (0 * inf, inf - inf): zero,
    infinite and NaN operands answer what IEEE division answers.  Divisors stay where the reciprocal is a normal float or exact
    (|b| in [2^-126, 2^126], 0, inf): a form built on rcp(b) has nothing to offer beyond that, with or without the step."""
    a, b = _quotient_pairs()
    ab = np.stack([A.f2w(a), A.f2w(b)], axis=1)
    got = ctx.selftest_eval("div_fast", ab)[:, 0].view(F)
    e = _ulps(got, a.astype(np.float64) / b.astype(np.float64))
    j = int(np.argmax(e))
    print("div_fast: max %.4f ulp at argument bits %s over %d pairs" % (e[j], _hex(ab[j]), len(ab)))
    assert e[j] <= 1.0, "div_fast: %.4f ulp at argument bits %s" % (e[j], _hex(ab[j]))
    sp = np.array([0.0, -0.0, 1.0, -3.0, 1e-30, 3e38, np.inf, -np.inf, np.nan], dtype=F)
    a, b = (v.reshape(-1) for v in np.meshgrid(sp, np.where(np.abs(sp) == F(3e38), F(1e30), sp), indexing="ij"))
    ab = np.stack([A.f2w(a), A.f2w(b)], axis=1)
    got = ctx.selftest_eval("div_fast", ab)[:, 0].view(F)
    with np.errstate(all="ignore"):
        want = (a / b).astype(F)
    edge = (b == 0) | np.isinf(b) | np.isnan(a) | np.isnan(b) | np.isinf(a)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same[edge].all(), "div_fast: argument bits %s -> %r, IEEE %r" % (_hex(ab[edge][~same[edge]][0]), got[edge][~same[edge]][0], want[edge][~same[edge]][0])


def test_fast_pow_within_the_bound_of_one_ulp_logarithm_and_exponential(ctx):
    """lv_pow_fast = v_exp_f32(y * v_log_f32(x)) over the shading domain (x dense in [0, 1]; y = 1, 1.7, 30, the AO gammas, the MLAT
    depths).  One ulp on the logarithm and one on the exponential give a relative error of 2^-23 (1 + 2 ln 2 |y log2 x|); the bar is
    twice that (the one-ulp figure is a datasheet number).  Where the exact result lies below the float32 normal range (2^-126) a
    relative error means nothing: there the result must lie below 2^-125.  Measured on an MI355X: see DESIGN.md 4."""
    w = A.pow_words(A.POW_SHADING_EXPONENTS, structured=False)
    x, y = A.w2f(w[:, 0]).astype(np.float64), A.w2f(w[:, 1]).astype(np.float64)
    got = ctx.selftest_eval("pow_fast", w)[:, 0].view(F).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        exact = np.power(x, y)
        ylog = np.where(x > 0, np.abs(y * np.log2(x)), 0.0)
    bar = 2.0 * 2.0 ** -23 * (1.0 + 2.0 * np.log(2.0) * ylog)
    normal = exact >= 2.0 ** -126
    assert (got[x == 0] == 0).all()
    assert (got[~normal] < 2.0 ** -125).all()
    rel = np.abs(got[normal] / exact[normal] - 1.0)
    share = rel / bar[normal]
    i = int(np.argmax(share))
    k = int(np.argmax(rel))
    wn = w[normal]
    print("pow_fast: max relative error %.3e (argument bits %s); max share of the bar %.3f (argument bits %s, error %.3e, bar %.3e) over "
          "%d pairs" % (rel[k], _hex(wn[k]), share[i], _hex(wn[i]), rel[i], bar[normal][i], len(rel)))
    assert share[i] <= 1.0, "pow_fast: relative error %.3e over the bar %.3e at argument bits %s" % (rel[i], bar[normal][i], _hex(wn[i]))
