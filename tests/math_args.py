"""Argument sets of the function-level parity tests (tests/test_gpu_math.py: device against CPU checker, bit for bit; tests/test_oracle.py:
checker against float64).  Everything here is deterministic: structured bit patterns, the neighbourhoods of the breakpoints the code
branches on, fixed-seed random words, and each function's real call domain sampled densely.  Floats travel as uint32 bit patterns.

Domain predicates: where host and device are not bound to agree, the arguments are named by a predicate here (quoted in
include/linevis_hip.h at lv_selftest_eval and in DESIGN.md 4), never by a silent mask in a test."""
import numpy as np

F = np.float32
U = np.uint32

TAN_PI_8 = F(0.41421356237309503)
TWO_PI = 6.283185307179586


def f2w(x):
    return np.ascontiguousarray(x, dtype=F).reshape(-1).view(U)


def w2f(w):
    return np.ascontiguousarray(w, dtype=U).view(F)


def structured_words():
    """every float whose low 11 mantissa bits are zero: 2^21 patterns -- both signs, all exponents, denormals, +-0, +-inf, quiet and
    signalling NaNs"""
    return (np.arange(1 << 21, dtype=np.uint64) << np.uint64(11)).astype(U)


def neighbours(values, k=64):
    """the +-k neighbouring bit patterns of every float32 in values (wrapping at the ends of the word)"""
    w = f2w(np.asarray(values, dtype=F)).astype(np.int64)
    return ((w[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]) & 0xFFFFFFFF).astype(U).reshape(-1)


def random_words(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U)


# ---------------------------------------------------------------- breakpoints the code branches on
COMMON_BREAKPOINTS = [0.0, 1.0, 2.0, 0.5, 1.41421356, 0.41421356, 2.0 ** -60, 2.0 ** 60, 1.17549435e-38, 0.70710678]


def breakpoints(name):
    b = list(COMMON_BREAKPOINTS)
    if name == "sincos2pi":
        b += [k / 8.0 for k in range(-16, 17)]                    # the quadrant boundaries k / 4 and r = 0.5 between them
        b += [2.0 ** 29, -2.0 ** 29]                              # the edge of the domain
    elif name == "sincos_rad":
        b += [float(F(k * TWO_PI)) for k in range(-8, 9)] + [float(F(k * TWO_PI / 8)) for k in range(-16, 17)]
        b += [float(F(TWO_PI * 2.0 ** j)) for j in range(1, 40, 3)]
    elif name == "exp2_det":
        b += [-125.0, 127.0] + [n + 0.5 for n in range(-127, 129)] + [float(n) for n in range(-126, 129, 7)]
    elif name in ("log2_det", "rsqrt_shade", "rsqrt_fast"):
        b += [float(F(1.41421356) * F(2.0) ** e) for e in range(-126, 127, 9)] + [2.0 ** e for e in range(-126, 128, 5)]
    elif name in ("mboit_fixed", "mboit_saturate"):
        b += [1024.0, -1024.0, -1.0, -0.5]
    return b


def _sincos2pi_domain():
    k = np.arange(1 << 20, dtype=np.int64)
    xi = ((k * 16 + (k & 15)) / float(1 << 24)).astype(F)         # lv_rnd's outputs k / 2^24, every 16th with a moving phase
    ring = np.concatenate([(np.arange(n + 1, dtype=F) / F(n)).astype(F) for n in range(3, 65)])   # float(sub) / float(N)
    return np.concatenate([xi, ring, np.array([1.0], dtype=F)])


def call_domain(name):
    """the arguments the render code really passes, dense (float32)"""
    if name == "sincos2pi":
        return _sincos2pi_domain()
    if name == "sincos_rad":                                      # phi, atan2 / 3, rotation angles: about a turn either way
        return np.linspace(-8.0, 8.0, 1 << 18).astype(F)
    if name == "exp2_det":                                        # lv_exp_det(-b_0 * absorbance), lv_exp_det of the warps: <= 0 mostly
        return np.concatenate([np.linspace(-64.0, 8.0, 1 << 18).astype(F), -np.geomspace(1e-12, 1.0, 1 << 14).astype(F)])
    if name == "log2_det":                                        # rho > 1 of the mip selection, view depths of lv_mboit_warp
        return np.geomspace(2.0 ** -20, 2.0 ** 20, 1 << 18).astype(F)
    if name in ("rsqrt_shade", "rsqrt_fast"):                     # squared lengths of shading vectors
        return np.geomspace(1e-12, 1e12, 1 << 18).astype(F)
    if name == "mboit_saturate":
        return np.linspace(-0.5, 1.5, 1 << 16).astype(F)
    if name == "mboit_fixed":
        return np.concatenate([mboit_tie_terms(), neighbours([1024.0, -1024.0], 8).view(F)])
    return np.zeros(0, dtype=F)


def unary_words(name):
    """structured + breakpoint neighbourhoods + 2^20 seeded words + the call domain (order fixed, duplicates kept out)"""
    w = np.concatenate([structured_words(), neighbours(breakpoints(name)), random_words(1 << 20, 0x5EED0000 + len(name)),
                        f2w(call_domain(name))])
    return np.unique(w)


def mboit_tie_terms():
    """terms that sit exactly on the ties k + 1/2 of the 2^-36 grid: (2 k + 1) / 2^37, and their float32 neighbours"""
    k = np.concatenate([np.arange(0, 4096), (1 << 23) - 1 - np.arange(0, 4096), np.arange(0, 4096) * 2047 + 5])
    t = ((2 * k + 1).astype(np.float64) * 2.0 ** -37).astype(F)
    t = np.concatenate([t, -t, (t * F(1024.0)).astype(F), (t * F(-65536.0)).astype(F)])
    return neighbours(t, 1).view(F)


def mboit_sums():
    """int64 sums for lv_mboit_unfixed, as (n, 2) words {low, high}: magnitudes up to 2^62 with the bits the int64 -> float32 rounding
    decides on (25th significant bit and below) set to exact ties, ties +- 1 and seeded random tails"""
    rng = np.random.default_rng(0xB017)
    out = [np.array([0, 1, -1, (1 << 62), -(1 << 62), (1 << 62) - 1, (1 << 36), 65534 * (1 << 46)], dtype=np.int64)]
    for sh in range(1, 39):
        lead = (np.int64(1 << 23) + rng.integers(0, 1 << 23, size=64, dtype=np.int64)) << np.int64(sh)   # 24 significant bits
        half = np.int64(1 << (sh - 1))
        for tail in (half, half - 1, half + 1 if sh > 1 else half, np.int64(0)):
            out.append(lead + tail)
            out.append(-(lead + tail))
        out.append(lead + rng.integers(0, 1 << sh, size=64, dtype=np.int64))
    r = rng.integers(-(1 << 62), 1 << 62, size=1 << 18, dtype=np.int64)
    out.append(r >> rng.integers(0, 62, size=r.size, dtype=np.int64))
    s = np.concatenate(out)
    s = s[np.abs(s) <= (1 << 62)]
    return np.ascontiguousarray(s.astype(np.int64)).view(U).reshape(-1, 2)


# ---------------------------------------------------------------- two-argument sets
def atan2_axis():
    """2048 structured values for each of y and x: both signs of 0, denormals, powers of two across the exponent range, the
    neighbourhoods of 1 and of tan(pi / 8) (with the other argument 1: ratios within 64 patterns of both thresholds), seeded
    magnitudes, inf, a quiet and a signalling NaN.  The diagonal of the grid holds the equal magnitudes."""
    mags = [np.array([0.0, 1e-45, 5.9e-39, 1.17549421e-38, 1.17549435e-38, 3.4028235e38, np.inf], dtype=F),
            (F(2.0) ** np.arange(-126, 128, 4)).astype(F),
            neighbours([1.0], 64).view(F), neighbours([TAN_PI_8], 64).view(F),
            neighbours([F(1.0) / TAN_PI_8], 16).view(F), np.array([3.0, 1e-3, 1e3, 0.1], dtype=F)]
    m = np.unique(f2w(np.concatenate(mags)))
    fill = 1022 - len(m)
    rnd = (random_words(4 * fill, 0xA7A2) & U(0x7FFFFFFF))
    rnd = rnd[(rnd < U(0x7F800000)) & ~np.isin(rnd, m)][:fill]
    m = np.concatenate([m, rnd, np.array([0x7FC00000, 0x7F800001], dtype=U)])   # qNaN, sNaN
    assert len(m) == 1024
    return np.concatenate([m, m | U(0x80000000)])


def atan2_words():
    a = atan2_axis()
    y, x = np.meshgrid(a, a, indexing="ij")
    return np.stack([y.reshape(-1), x.reshape(-1)], axis=1)


AO_GAMMAS = [0.5 + 0.25 * i for i in range(11)]
MLAT_DEPTHS = [float(v) for v in np.linspace(0.01, 4.0, 32).astype(F)]
POW_EXPONENTS = [0.0, 1.0, 1.7, 30.0] + AO_GAMMAS + MLAT_DEPTHS + [-1.0, np.inf, -np.inf, np.nan]
POW_SHADING_EXPONENTS = [1.0, 1.7, 30.0] + AO_GAMMAS + MLAT_DEPTHS


def pow_bases(structured=True):
    x = (np.arange(1 << 16, dtype=np.float64) / float((1 << 16) - 1)).astype(F)   # |n . l|, |n . h|, AO factors, transmittances
    if not structured:
        return x
    return np.concatenate([x, structured_words()[::512].view(F)])


def pow_words(exponents=None, structured=True):
    x = f2w(pow_bases(structured))
    y = f2w(np.array(POW_EXPONENTS if exponents is None else exponents, dtype=F))
    xx, yy = np.meshgrid(x, y, indexing="ij")
    return np.stack([xx.reshape(-1), yy.reshape(-1)], axis=1)


# ---------------------------------------------------------------- tables
TF_SIZES = [1, 2, 3, 256]
TF_RANGES = [(0.0, 1.0), (-3.0, 7.0), (5.0, -2.0), (2.0, 2.0), (0.0, float("inf")), (float("-inf"), 1.0)]


def tf_table(n):
    return np.random.default_rng(0x7F00 + n).random((n, 4)).astype(F)


def tf_attributes(n, lo, hi):
    """texel centres and edges (position * n = k / 2) +-8 patterns, below and above the range, +-0, denormals, +-inf, NaNs, a cut of the
    structured set and seeded words"""
    lo64, hi64 = (np.float64(v) if np.isfinite(v) else np.float64(np.sign(v) * 1e30) for v in (lo, hi))
    k = np.arange(0, 2 * n + 1, dtype=np.float64) / (2.0 * n)
    at = (lo64 + k * (hi64 - lo64)).astype(F)
    span = abs(hi64 - lo64) + 1.0
    extra = np.array([lo64 - span, hi64 + span, lo64 - 1e-3 * span, hi64 + 1e-3 * span, 0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf,
                      lo, hi], dtype=F)
    w = np.concatenate([neighbours(at, 8), neighbours(extra, 8), np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], dtype=U),
                        structured_words()[::512], random_words(4096, 0x7FA0 + n)])
    return np.unique(w)


TWIST_TEXTURES = [(1, 1), (2, 1), (64, 4), (128, 8), (100, 3)]   # (w, h)


def twist_texture(w, h):
    return np.random.default_rng(0x7715 + 131 * w + h).integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def twist_levels(w, h):
    n, m = 0, max(w, h)
    while m > 1:
        n, m = n + 1, m >> 1
    return max(n, 1)


def twist_u(w):
    """texel centres and edges +-8 patterns over three periods either side of 0, seeded u up to 2^20 turns, u * w at and beyond +-2^31,
    +-inf, NaNs"""
    k = np.arange(-4 * w, 6 * w + 1, dtype=np.float64) / (2.0 * w)
    rng = np.random.default_rng(0x7716 + w)
    far = (rng.random(2048) * 2.0 - 1.0) * 2.0 ** rng.integers(0, 21, size=2048)
    edge = np.array([s * 2.0 ** e / w for s in (1.0, -1.0) for e in (23, 24, 30, 31, 32, 33, 40, 62, 100)] + [3.4e38, -3.4e38, np.inf, -np.inf])
    w_ = np.concatenate([neighbours(k.astype(F), 8), f2w(far.astype(F)), neighbours(edge.astype(F), 8),
                         np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0, 0x80000000, 1, 0x80000001], dtype=U)])
    return np.unique(w_)


def twist_derivatives(w, h):
    """0, denormal, NaN, inf, and derivatives that put lambda = log2(d * w) exactly on and +-8 patterns around every integer and every
    half-integer level of the chain, and beyond it"""
    levels = twist_levels(w, h)
    lam = np.arange(-2, 2 * (levels + 3) + 1, dtype=np.float64) / 2.0
    d = (2.0 ** lam / w).astype(F)
    special = np.array([0.0, -0.0, 1e-45, 1e-39, np.nan, np.inf, -np.inf, 1e30, -1e30, 1.0 / w, -1.0 / w], dtype=F)
    return np.unique(np.concatenate([neighbours(d, 8), neighbours(-d, 1), f2w(special), np.array([0x7F800001], dtype=U)]))


def twist_words(w, h):
    """(n, 4) words {u, dudx, dudy, useGrad}: every u without derivatives; a cut of the u set against every derivative"""
    u = twist_u(w)
    d = twist_derivatives(w, h)
    plain = np.stack([u, np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)], axis=1)
    uc = np.concatenate([u[::max(len(u) // 384, 1)], u[-64:]])
    uu, dd = np.meshgrid(uc, d, indexing="ij")
    uu, dd = uu.reshape(-1), dd.reshape(-1)
    other = np.roll(dd, 7)
    sel = np.arange(len(dd)) % 3
    dx = np.where(sel == 1, U(0), dd)
    dy = np.where(sel == 0, U(0), np.where(sel == 1, dd, other))
    grad = np.stack([uu, dx, dy, np.ones_like(uu)], axis=1)
    return np.ascontiguousarray(np.concatenate([plain, grad]).astype(U))


def unorm_channels():
    """channel values at k / 255 and at the rounding ties (k + 1/2) / 255, +-8 patterns, values below 0 and above 1, -0, inf, NaNs"""
    k = np.arange(0, 256, dtype=np.float64)
    v = np.concatenate([(k / 255.0), ((k + 0.5) / 255.0)]).astype(F)
    extra = np.array([0.0, -0.0, -1e-3, -1.0, 1.0, 1.001, 2.0, 256.0, 1e30, -1e30, np.inf, -np.inf, 1e-45, -1e-45], dtype=F)
    return np.unique(np.concatenate([neighbours(v, 8), neighbours(extra, 8), np.array([0x7FC00000, 0xFFC00000, 0x7F800001], dtype=U)]))


def pack_words():
    """(n, 4) channel words: every channel value in every channel position against seeded partners"""
    c = unorm_channels()
    rng = np.random.default_rng(0x9AC4)
    rows = []
    for pos in range(4):
        q = c[rng.integers(0, len(c), size=(len(c), 4))]
        q[:, pos] = c
        rows.append(q)
    return np.ascontiguousarray(np.concatenate(rows).astype(U))


def unpack_words():
    """all 2^32 words strided to 2^22 (the stride 1024 + a moving phase reaches every byte value in every channel)"""
    k = np.arange(1 << 22, dtype=np.uint64)
    return ((k << np.uint64(10)) + (k * np.uint64(2654435761) & np.uint64(1023))).astype(U)


# ---------------------------------------------------------------- domain predicates
def sincos2pi_outside_domain(words):
    """lv_sincos2pi is defined for every float except finite |xi| >= 2^29: there floor(4 xi) does not fit the int the quadrant is taken
    from (C++: undefined; x86 answers INT_MIN = quadrant 0, gfx950 saturates = quadrant 3).  No caller gets there: the AO sample
    passes lv_rnd's [0, 1), the tube rings sub / N in [0, 1], lv_sincos_rad a fraction in [0, 1).  NaN and +-inf are inside: both
    sides answer NaN."""
    x = w2f(words)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (np.abs(x) >= F(2.0 ** 29))


def structured_outside_sincos2pi_domain():
    """what the predicate removes from structured_words(), counted from the format: biased exponents 127 + 29 ... 254, 2^12 kept mantissa
    patterns each, both signs"""
    return (254 - (127 + 29) + 1) * (1 << 12) * 2


# ---------------------------------------------------------------- where a float64 anchor means something (tests/test_oracle.py)
def log2_det_is_a_logarithm(words):
    """lv_log2_det reads exponent and mantissa bits: a logarithm for normal x > 0 only (its callers pass rho > 1 and view depths)"""
    x = w2f(words)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x >= F(1.17549435e-38))


def sincos_rad_anchor_domain(words):
    """|a| <= 8: the range tests/test_bands.py states the accuracy of lv_sincos_rad for (the float32 reduction a / 2 pi loses |a| 2^-24
    turns beyond it)"""
    x = w2f(words)
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= F(8.0)


def pow_det_anchor_domain(words):
    """finite y with x == 0 and y >= 0, or finite x above the smallest normal: elsewhere lv_pow_det answers by its x == 0 rule (every
    x that is not > 1.17549435e-38 counts as 0; 0 to a negative power is +inf whatever the zero's sign), not with a power"""
    x, y = w2f(words[:, 0]), w2f(words[:, 1])
    with np.errstate(invalid="ignore"):
        return (((x == 0) & (y >= 0)) | (np.isfinite(x) & (x > F(1.17549435e-38)))) & np.isfinite(y)


def atan2_det_anchor_domain(words):
    """finite y and x, without the arguments where IEEE atan2 reads the sign of a zero that lv_atan2_det does not: y == 0 with
    x == 0 (GLSL: undefined; the build answers 0) and y == -0 with x < 0 (the build answers +pi, IEEE -pi: the same angle)"""
    y, x = w2f(words[:, 0]), w2f(words[:, 1])
    neg_zero_y = np.ascontiguousarray(words[:, 0]) == U(0x80000000)
    return np.isfinite(y) & np.isfinite(x) & ~((y == 0) & (x == 0)) & ~(neg_zero_y & (x < 0))
