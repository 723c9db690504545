"""Moment-based order-independent transparency (rendering mode 6: power moments, 4 / 6 / 8 of them, float32) restated on the CPU.

mboit_fold() is the vectorised numpy statement the GPU tests (test_gpu_mboit.py) compare the device kernels with, bit for bit.  Here it
is checked against a scalar, line-by-line transcription of the reference's shaders: MBOITPass1.glsl:44-52 and MBOITPass2.glsl:21-37
(gatherFragment), MBOITHeader.glsl:49-52 (logDepthWarp), MomentOIT.glsl:313-376 (generateMoments, ROV = 0) and :412-563
(resolveMoments), MomentMath.glsl:25-152 (the polynomial solvers) and :246-505 (the three reconstructions), DXHelper.glsl:19-22
(saturate), MBOITBlend.glsl:82-102, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour.

The numerics contract: float32, one operation at a time; fma() where the shader writes fma (correctly rounded);
log / exp / atan2 / sin / cos are the build's fixed float32 definitions; every per-pixel sum is a sum of 64-bit fixed-point terms
rint(clamp(term, -1024, 1024) * 2^36) and therefore independent of the order of the fragments."""
import math
from fractions import Fraction

import numpy as np

from oracle import lvo
from test_mlab_restatement import F, pack

U32 = np.uint32
FIXED_SHIFT = 36                      # 65534 fragments x 1024 x 2^36 < 2^63
FIXED_LIMIT = F(1024.0)               # a term outside [-1024, 1024] saturates (a NaN counts as -1024)
B0_THRESHOLD = F(0.00100050033)       # MomentOIT.glsl:421, MBOITBlend.glsl:89
MOMENT_BIAS = {4: 5e-7, 6: 5e-6, 8: 5e-5}   # MBOITRenderer.cpp:136-145
BIAS_VECTOR = {4: [0, 0.375, 0, 0.375], 6: [0, 0.48, 0, 0.451, 0, 0.45],     # MomentOIT.glsl:450,505,547 (SINGLE_PRECISION)
               8: [0, 0.75, 0, 0.67666666666666664, 0, 0.63, 0, 0.60030303030303034]}
LN2 = F(0.693147181)
LOG2E = F(1.44269504)
SQRT3_HALF = F(F(0.5) * np.sqrt(F(3.0)))


# ---------------------------------------------------------------- building blocks (arrays or float32 scalars alike)
def fma32(a, b, c):
    """correctly rounded float32 fma: the product of two float32 is exact in float64; its sum with c is rounded to odd in float64
    (TwoSum gives the error), so that the cast to float32 is the only rounding that counts"""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf))
        return np.where(inexact, odd, s).astype(F)


def log2_det(x):
    """lv_log2_det: exponent bits + atanh series on [sqrt(1/2), sqrt(2)]"""
    bits = np.asarray(x, dtype=F).view(U32)
    e = ((bits >> U32(23)) & U32(0xFF)).astype(np.int32) - np.int32(127)
    m = ((bits & U32(0x007FFFFF)) | U32(0x3F800000)).view(F)
    big = m > F(1.41421356)
    m = np.where(big, m * F(0.5), m)
    e = np.where(big, e + np.int32(1), e)
    f = m - F(1.0)
    s = f / (F(2.0) + f)
    z = s * s
    P = F(0.333333333) + z * (F(0.2) + z * (F(0.142857143) + z * F(0.111111111)))
    ln = F(2.0) * s + (F(2.0) * s) * (z * P)
    return (e.astype(F) + ln * LOG2E).astype(F)


def log_det(x):
    return (log2_det(x) * LN2).astype(F)


def exp2_det(p):
    """lv_exp2_det = the second half of lv_pow_det (lv_pow_det(2, p) bit for bit); a NaN stays a NaN"""
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        q = np.where(np.isfinite(p) & (p >= F(-125.0)) & (p <= F(127.0)), p, F(0.0)).astype(F)
        n = np.floor(q + F(0.5))
        t = (q - n) * LN2
        Q = F(1.0) + t * (F(1.0) + t * (F(0.5) + t * (F(0.166666667) + t * (F(0.0416666667) + t * (F(0.00833333333) + t * (
            F(0.00138888889) + t * F(0.000198412698)))))))
        r = (Q.astype(F).view(U32) + (n.astype(np.int32).astype(U32) << U32(23))).view(F)
        r = np.where(p < F(-125.0), F(0.0), r)
        r = np.where(p > F(127.0), F(np.inf), r)
        return np.where(np.isnan(p), F(np.nan), r).astype(F)


def exp_det(x):
    with np.errstate(all="ignore"):
        return exp2_det(np.asarray(x, dtype=F) * LOG2E)


def sincos_det(a):
    """lv_sincos_rad (through lv_sincos2pi)"""
    a = np.asarray(a, dtype=F)
    with np.errstate(all="ignore"):
        u = a * F(0.15915494309189535)
        u = u - np.floor(u)
        u = np.where(u < F(1.0), u, F(0.0)).astype(F)
        q = u * F(4.0)
        fq = np.floor(q)
        quad = fq.astype(np.int32) & 3
        r = q - fq
        swp = r > F(0.5)
        rr = np.where(swp, F(1.0) - r, r)
        x = rr * F(1.57079632679489662)
        x2 = x * x
        sp = x * (F(1.0) + x2 * (F(-1.0) / F(6.0) + x2 * (F(1.0) / F(120.0) + x2 * (F(-1.0) / F(5040.0) + x2 * (F(1.0) / F(362880.0))))))
        cp = F(1.0) + x2 * (F(-0.5) + x2 * (F(1.0) / F(24.0) + x2 * (F(-1.0) / F(720.0) + x2 * (F(1.0) / F(40320.0) + x2 * (
            F(-1.0) / F(3628800.0))))))
        sa = np.where(swp, cp, sp)
        ca = np.where(swp, sp, cp)
        s = np.select([quad == 0, quad == 1, quad == 2], [sa, ca, -sa], -ca)
        c = np.select([quad == 0, quad == 1, quad == 2], [ca, -sa, -ca], sa)
        return s.astype(F), c.astype(F)


def atan2_det(y, x):
    """lv_atan2_det"""
    y, x = (np.asarray(v, dtype=F) for v in np.broadcast_arrays(y, x))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.fmax(ax, ay), np.fmin(ax, ay)
        a = mn / mx
        hi = a > F(0.41421356237309503)
        a = np.where(hi, (a - F(1.0)) / (a + F(1.0)), a)
        base = np.where(hi, F(0.78539816339744831), F(0.0)).astype(F)
        s = a * a
        p = a * (F(1.0) + s * (F(-1.0) / F(3.0) + s * (F(1.0) / F(5.0) + s * (F(-1.0) / F(7.0) + s * (F(1.0) / F(9.0) + s * (
            F(-1.0) / F(11.0) + s * (F(1.0) / F(13.0))))))))
        r = base + p
        r = np.where(ay > ax, F(1.57079632679489662) - r, r)
        r = np.where(mx > F(0.0), r, F(0.0))
        r = np.where(x < F(0.0), F(3.14159265358979323846) - r, r)
        r = np.where(y < F(0.0), -r, r)
        return r.astype(F)


def saturate(x):
    """DXHelper.glsl:19-22: +-inf -> 1, then clamp; the clamp is fminf(fmaxf(x, 0), 1), so a NaN becomes 0"""
    x = np.where(np.isinf(x), F(1.0), x)
    return np.fmin(np.fmax(x, F(0.0)), F(1.0)).astype(F)


def mix(x, y, a):
    return x * (F(1.0) - a) + y * a


def to_fixed(term):
    t = np.fmin(np.fmax(np.asarray(term, dtype=F), -FIXED_LIMIT), FIXED_LIMIT)
    return np.rint(t.astype(np.float64) * float(2 ** FIXED_SHIFT)).astype(np.int64)


def from_fixed(s):
    return (np.asarray(s, dtype=np.int64).astype(F) * F(2.0 ** -FIXED_SHIFT)).astype(F)


def view_depth(pos, view):
    """-screenSpacePosition.z of world positions (n, 3): row z of the column-major view matrix, summed in the device's order"""
    v = np.asarray(view, dtype=F).reshape(16)
    p = np.asarray(pos, dtype=F).reshape(-1, 3)
    return (-(((v[2] * p[:, 0] + v[6] * p[:, 1]) + v[10] * p[:, 2]) + v[14])).astype(F)


def log_depth_range(box_min, box_max, view, near, far):
    """computeDepthRange (MBOITRenderer.cpp:484-503): the eight corners of the line points' box through row z of `view`; the
    logarithm is the build's (log_det)"""
    v = np.asarray(view, dtype=F).reshape(16)
    lo, hi = np.asarray(box_min, dtype=F), np.asarray(box_max, dtype=F)
    zs = []
    for k in range(8):
        x, y, z = (hi[0] if k & 1 else lo[0]), (hi[1] if k & 2 else lo[1]), (hi[2] if k & 4 else lo[2])
        zs.append(F(F(F(F(v[2] * x) + F(v[6] * y)) + F(v[10] * z)) + v[14]))
    mn = F(F(-max(zs)) - F(0.1))
    mx = F(F(-min(zs)) + F(0.1))
    near, far = F(near), F(far)
    mn = max(mn, near)
    mx = min(mx, far)
    mn = min(mn, far)
    mx = max(mx, near)
    return F(log_det(F(mn))), F(log_det(F(mx)))


def warp_depth(z, log_min, log_max):
    """logDepthWarp, MBOITHeader.glsl:49-52"""
    with np.errstate(all="ignore"):
        return ((log_det(z) - F(log_min)) / (F(log_max) - F(log_min)) * F(2.0) - F(1.0)).astype(F)


# ---------------------------------------------------------------- the polynomial solvers, vectorised (MomentMath.glsl:25-152)
def _solve_quadratic_monic(c1, c2):
    """solveQuadratic(vec3(1.0, c1, c2))"""
    c1 = c1 * F(0.5)
    tmp = np.sqrt(c1 * c1 - c2)
    pos = c1 >= F(0.0)
    x1 = np.where(pos, (-c2) / (c1 + tmp), -c1 + tmp)
    x2 = np.where(pos, -c1 - tmp, c2 / (-c1 + tmp))
    return x1, x2


def _solve_cubic(c0, c1, c2, c3):
    """SolveCubic"""
    x, y, z = c0 / c3, c1 / c3, c2 / c3
    y, z = y / F(3.0), z / F(3.0)
    dx = fma32(-z, z, y)
    dy = fma32(-y, z, x)
    dz = z * x + (-y) * y
    disc = (F(4.0) * dx) * dz + (-dy) * dy
    depx = fma32(F(-2.0) * z, dx, dy)
    depy = dx
    theta = atan2_det(np.sqrt(disc), -depx) / F(3.0)
    sn, cs = sincos_det(theta)
    r0 = cs
    r1 = F(-0.5) * cs + (-SQRT3_HALF) * sn
    r2 = F(-0.5) * cs + SQRT3_HALF * sn
    k = F(2.0) * np.sqrt(-depy)
    return fma32(k, r0, -z), fma32(k, r1, -z), fma32(k, r2, -z)


def _solve_cubic_blinn_smallest(c0, c1, c2):
    """solveCubicBlinnSmallest(vec4(c0, c1, c2, 1.0))"""
    x, y, z = c0 / F(1.0), c1 / F(1.0), c2 / F(1.0)
    y, z = y / F(3.0), z / F(3.0)
    dx = fma32(-z, z, y)
    dy = fma32(-z, y, x)
    dz = z * x - y * y
    disc = (F(4.0) * dx) * dz - dy * dy
    depx = dz
    depy = (-x) * dy + (F(2.0) * y) * dz
    theta = np.abs(atan2_det(x * np.sqrt(disc), -depy)) / F(3.0)
    sn, cs = sincos_det(theta)
    tmp = F(2.0) * np.sqrt(-depx)
    xx = tmp * cs
    xy = tmp * (F(-0.5) * cs - SQRT3_HALF * sn)
    sy = np.where(xx + xy < F(2.0) * y, xx + y, xy + y)
    return (-x) / sy


def _solve_quartic_neumark(c):
    B, C, D, E = c[3] / c[4], c[2] / c[4], c[1] / c[4], c[0] / c[4]
    P = F(-2.0) * C
    Q = (C * C + B * D) - F(4.0) * E
    R = (D * D + (B * B) * E) - (B * C) * D
    y = _solve_cubic_blinn_smallest(R, Q, P)
    BB = B * B
    fy = F(4.0) * y
    BB_fy = BB - fy
    Z = C - y
    ZZ = Z * Z
    fE = F(4.0) * E
    ZZ_fE = ZZ - fE
    first = (y < F(0.0)) | ((ZZ + fE) * BB_fy > ZZ_fE * (BB + fy))
    t1 = np.sqrt(BB_fy)
    G1, g1 = (B + t1) * F(0.5), (B - t1) * F(0.5)
    u1 = (B * Z - F(2.0) * D) / (F(2.0) * t1)
    H1, h1 = fma32(Z, F(0.5), u1), fma32(Z, F(0.5), -u1)
    t2 = np.sqrt(ZZ_fE)
    H2, h2 = (Z + t2) * F(0.5), (Z - t2) * F(0.5)
    u2 = (B * Z - F(2.0) * D) / (F(2.0) * t2)
    G2, g2 = fma32(B, F(0.5), u2), fma32(B, F(0.5), -u2)
    G, g, H, h = np.where(first, G1, G2), np.where(first, g1, g2), np.where(first, H1, H2), np.where(first, h1, h2)
    a1, a2 = _solve_quadratic_monic(G, H)
    a3, a4 = _solve_quadratic_monic(g, h)
    return a1, a2, a3, a4


# ---------------------------------------------------------------- the reconstructions, vectorised (MomentMath.glsl:246-505)
def _biased(b, N, bias):
    return [mix(b[i], F(BIAS_VECTOR[N][i]), F(bias)).astype(F) for i in range(N)]


def _transmittance4(b_0, b, z0, bias, over):
    b = _biased(b, 4, bias)
    L21D11 = fma32(-b[0], b[1], b[2])
    D11 = fma32(-b[0], b[0], b[1])
    InvD11 = F(1.0) / D11
    L21 = L21D11 * InvD11
    SDV = fma32(-b[1], b[1], b[3])
    D22 = fma32(-L21D11, L21, SDV)
    c0, c1, c2 = F(1.0), z0, z0 * z0
    c1 = c1 - b[0]
    c2 = c2 - (b[1] + L21 * c1)
    c1 = c1 * InvD11
    c2 = c2 / D22
    c1 = c1 - L21 * c2
    c0 = c0 - (c1 * b[0] + c2 * b[1])
    InvC2 = F(1.0) / c2
    p = c1 * InvC2
    q = c0 * InvC2
    D = (p * p) * F(0.25) - q
    r = np.sqrt(D)
    z1 = (-p) * F(0.5) - r
    z2 = (-p) * F(0.5) + r
    f0 = F(over)
    f1 = np.where(z1 < z0, F(1.0), F(0.0)).astype(F)
    f2 = np.where(z2 < z0, F(1.0), F(0.0)).astype(F)
    f01 = (f1 - f0) / (z1 - z0)
    f12 = (f2 - f1) / (z2 - z1)
    f012 = (f12 - f01) / (z2 - z0)
    p0 = f012
    p1 = p0
    p0 = f01 - p0 * z1
    p2 = p1
    p1 = p0 - p1 * z0
    p0 = f0 - p0 * z0
    absorbance = p0 + (b[0] * p1 + b[1] * p2)
    return saturate(exp_det((-b_0) * absorbance))


def _transmittance6(b_0, b, z0, bias, over):
    b = _biased(b, 6, bias)
    InvD11 = F(1.0) / fma32(-b[0], b[0], b[1])
    L21D11 = fma32(-b[0], b[1], b[2])
    L21 = L21D11 * InvD11
    D22 = fma32(-L21D11, L21, fma32(-b[1], b[1], b[3]))
    L31D11 = fma32(-b[0], b[2], b[3])
    L31 = L31D11 * InvD11
    InvD22 = F(1.0) / D22
    L32D22 = fma32(-L21D11, L31, fma32(-b[1], b[2], b[4]))
    L32 = L32D22 * InvD22
    D33 = fma32(-b[2], b[2], b[5]) - (L31D11 * L31 + L32D22 * L32)
    InvD33 = F(1.0) / D33
    c0, c1 = F(1.0), z0
    c2 = c1 * z0
    c3 = c2 * z0
    c1 = c1 - b[0]
    c2 = c2 - fma32(L21, c1, b[1])
    c3 = c3 - (b[2] + (L31 * c1 + L32 * c2))
    c1, c2, c3 = c1 * InvD11, c2 * InvD22, c3 * InvD33
    c2 = c2 - L32 * c3
    c1 = c1 - (L21 * c2 + L31 * c3)
    c0 = c0 - ((b[0] * c1 + b[1] * c2) + b[2] * c3)
    z1, z2, z3 = _solve_cubic(c0, c1, c2, c3)
    f0 = F(over)
    f1 = np.where(z1 > z0, F(0.0), F(1.0)).astype(F)
    f2 = np.where(z2 > z0, F(0.0), F(1.0)).astype(F)
    f3 = np.where(z3 > z0, F(0.0), F(1.0)).astype(F)
    f01 = (f1 - f0) / (z1 - z0)
    f12 = (f2 - f1) / (z2 - z1)
    f23 = (f3 - f2) / (z3 - z2)
    f012 = (f12 - f01) / (z2 - z0)
    f123 = (f23 - f12) / (z3 - z1)
    f0123 = (f123 - f012) / (z3 - z0)
    p0 = fma32(-f0123, z2, f012)
    p1 = f0123
    p2 = p1
    p1 = fma32(p1, -z1, p0)
    p0 = fma32(p0, -z1, f01)
    p3 = p2
    p2 = fma32(p2, -z0, p1)
    p1 = fma32(p1, -z0, p0)
    p0 = fma32(p0, -z0, f0)
    absorbance = ((p0 + p1 * b[0]) + p2 * b[1]) + p3 * b[2]
    return saturate(exp_det((-b_0) * absorbance))


def _transmittance8(b_0, b, z0, bias, over):
    b = _biased(b, 8, bias)
    D22 = fma32(-b[0], b[0], b[1])
    InvD22 = F(1.0) / D22
    L32D22 = fma32(-b[1], b[0], b[2])
    L32 = L32D22 * InvD22
    L42D22 = fma32(-b[2], b[0], b[3])
    L42 = L42D22 * InvD22
    L52D22 = fma32(-b[3], b[0], b[4])
    L52 = L52D22 * InvD22
    D33 = fma32(-L32, L32D22, fma32(-b[1], b[1], b[3]))
    InvD33 = F(1.0) / D33
    L43D33 = fma32(-L42, L32D22, fma32(-b[2], b[1], b[4]))
    L43 = L43D33 * InvD33
    L53D33 = fma32(-L52, L32D22, fma32(-b[3], b[1], b[5]))
    L53 = L53D33 * InvD33
    D44 = fma32(-b[2], b[2], b[5]) - (L42 * L42D22 + L43 * L43D33)
    InvD44 = F(1.0) / D44
    L54D44 = fma32(-b[3], b[2], b[6]) - (L52 * L42D22 + L53 * L43D33)
    L54 = L54D44 * InvD44
    D55 = fma32(-b[3], b[3], b[7]) - ((L52 * L52D22 + L53 * L53D33) + L54 * L54D44)
    InvD55 = F(1.0) / D55
    c = [F(1.0), z0, None, None, None]
    c[2] = c[1] * z0
    c[3] = c[2] * z0
    c[4] = c[3] * z0
    c[1] = c[1] - b[0]
    c[2] = c[2] - fma32(L32, c[1], b[1])
    c[3] = c[3] - (b[2] + (L42 * c[1] + L43 * c[2]))
    c[4] = c[4] - (b[3] + ((L52 * c[1] + L53 * c[2]) + L54 * c[3]))
    c[1], c[2], c[3], c[4] = c[1] * InvD22, c[2] * InvD33, c[3] * InvD44, c[4] * InvD55
    c[3] = c[3] - L54 * c[4]
    c[2] = c[2] - (L53 * c[4] + L43 * c[3])
    c[1] = c[1] - ((L52 * c[4] + L42 * c[3]) + L32 * c[2])
    c[0] = c[0] - (((b[3] * c[4] + b[2] * c[3]) + b[1] * c[2]) + b[0] * c[1])
    z1, z2, z3, z4 = _solve_quartic_neumark(c)
    f0 = F(over)
    f1, f2, f3, f4 = (np.where(z <= z0, F(1.0), F(0.0)).astype(F) for z in (z1, z2, z3, z4))
    f01 = (f1 - f0) / (z1 - z0)
    f12 = (f2 - f1) / (z2 - z1)
    f23 = (f3 - f2) / (z3 - z2)
    f34 = (f4 - f3) / (z4 - z3)
    f012 = (f12 - f01) / (z2 - z0)
    f123 = (f23 - f12) / (z3 - z1)
    f234 = (f34 - f23) / (z4 - z2)
    f0123 = (f123 - f012) / (z3 - z0)
    f1234 = (f234 - f123) / (z4 - z1)
    f01234 = (f1234 - f0123) / (z4 - z0)
    P_0 = fma32(-f01234, z3, f0123)
    P0 = f01234
    P1 = P0
    P0 = fma32(-P0, z2, P_0)
    P_0 = fma32(-P_0, z2, f012)
    P2 = P1
    P1 = fma32(-P1, z1, P0)
    P0 = fma32(-P0, z1, P_0)
    P_0 = fma32(-P_0, z1, f01)
    P3 = P2
    P2 = fma32(-P2, z0, P1)
    P1 = fma32(-P1, z0, P0)
    P0 = fma32(-P0, z0, P_0)
    P_0 = fma32(-P_0, z0, f0)
    absorbance = P_0 + (((P0 * b[0] + P1 * b[1]) + P2 * b[2]) + P3 * b[3])
    return saturate(exp_det((-b_0) * absorbance))


TRANSMITTANCE = {4: _transmittance4, 6: _transmittance6, 8: _transmittance8}


def moment_terms(depth, absorbance, N):
    """generateMoments' power moments (MomentOIT.glsl:358-374): absorbance x depth^k, k = 1 ... N, in the shader's association"""
    d2 = depth * depth
    d4 = d2 * d2
    if N == 4:
        pw = [depth, d2, d2 * depth, d4]
    elif N == 6:
        pw = [depth, d2, d2 * depth, d4, d4 * depth, d4 * d2]
    else:
        d6 = d4 * d2
        pw = [depth, d2, d2 * depth, d4, d4 * depth, d6, d6 * depth, d6 * d2]
    return [(p * absorbance).astype(F) for p in pw]


# ---------------------------------------------------------------- the vectorised statement
def mboit_sums(rgba, z, pix, P, N, log_min, log_max):
    """sweep 1 over flat fragment arrays: the integer sums (1 + N, P) of the absorbance and its power moments"""
    with np.errstate(all="ignore"):
        depth = warp_depth(z, log_min, log_max)
        tr = (F(1.0) - rgba[:, 3]).astype(F)
        live = ~(tr > F(0.9999999))            # generateMoments: discard above, MomentOIT.glsl:327
        ab = (-log_det(tr)).astype(F)
        ab = np.where(ab > F(10.0), F(10.0), ab).astype(F)   # ABSORBANCE_MAX_VALUE
        sums = np.zeros((1 + N, P), dtype=np.int64)
        terms = [ab] + moment_terms(depth, ab, N)
        for k, t in enumerate(terms):
            np.add.at(sums[k], pix[live], to_fixed(t[live]))
    return sums, depth


def mboit_fold(runs, N, background, log_min, log_max, overestimation=0.1, bias=None, details=False):
    """runs: list (one per pixel) of (rgba (n, 4) float32 straight colour, view depth (n,) float32), any order within a pixel.
    Returns (frame (num_pixels, 4) uint8, moments (num_pixels, 1 + N) float32: b_0 then the normalised b_1 ... b_N, zeros under the
    threshold); with details also the number of degenerate pixels (b_0 over the threshold and a_sum == 0)."""
    N = int(N)
    bias = MOMENT_BIAS[N] if bias is None else bias
    P = len(runs)
    lens = np.array([len(r[1]) for r in runs], dtype=np.int64)
    pix = np.repeat(np.arange(P), lens)
    rgba = np.concatenate([np.asarray(r[0], dtype=F).reshape(-1, 4) for r in runs] + [np.zeros((0, 4), F)])
    z = np.concatenate([np.asarray(r[1], dtype=F).reshape(-1) for r in runs] + [np.zeros(0, F)])
    sums, depth = mboit_sums(rgba, z, pix, P, N, log_min, log_max)
    bg = [F(v) for v in background]
    with np.errstate(all="ignore"):
        b_0 = from_fixed(sums[0])
        covered = ~(b_0 < B0_THRESHOLD)
        bn = [(from_fixed(sums[k]) / b_0).astype(F) for k in range(1, N + 1)]
        moments = np.zeros((P, 1 + N), dtype=F)
        moments[covered, 0] = b_0[covered]
        for k in range(N):
            moments[covered, 1 + k] = bn[k][covered]
        sel = covered[pix]
        fp = pix[sel]
        T = TRANSMITTANCE[N](b_0[fp], [v[fp] for v in bn], depth[sel], bias, overestimation)
        c, a = rgba[sel, :3], rgba[sel, 3]
        csum = np.zeros((4, P), dtype=np.int64)
        for k in range(3):
            np.add.at(csum[k], fp, to_fixed((c[:, k] * a) * T))
        np.add.at(csum[3], fp, to_fixed(a * T))
        s = [from_fixed(csum[k]) for k in range(4)]
        hit = covered & (csum[3] != 0)
        A = (F(1.0) - exp_det(-b_0)).astype(F)
        out = [np.full(P, bg[k], dtype=F) for k in range(4)]
        for k in range(3):
            out[k] = np.where(hit, (s[k] / s[3]) * A + bg[k] * (F(1.0) - A), out[k]).astype(F)
        out[3] = np.where(hit, A + bg[3] * (F(1.0) - A), out[3]).astype(F)
    packed = pack(out)
    frame = np.stack([(packed >> U32(8 * k)) & U32(0xFF) for k in range(4)], axis=1).astype(np.uint8)
    if details:
        return frame, moments, int((covered & ~hit).sum())
    return frame, moments


# ---------------------------------------------------------------- scalar transcription of the shaders
def _fma1(a, b, c):
    """fma() of one float32 triple through exact rational arithmetic"""
    a, b, c = F(a), F(b), F(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return _round_fraction(exact, float(a) * float(b) + float(c))


def _round_fraction(exact, hint):
    """the float32 nearest to a rational (ties to even); hint = a float64 near it (for the sign of zero and the overflow)"""
    if exact == 0:
        return F(hint) if hint == 0.0 else F(0.0)
    if abs(exact) >= Fraction(2) ** 128:
        return F(math.copysign(math.inf, exact))
    e = math.frexp(float(exact))[1] - 24                       # unit in the last place of a 24-bit significand
    e = max(e, -149)
    q = exact / (Fraction(2) ** e)
    n = math.floor(q)
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F(float(Fraction(n) * Fraction(2) ** e))


def _sincos1(a):
    s, c = np.zeros(1, F), np.zeros(1, F)
    import ctypes as C
    ss, cc = C.c_float(), C.c_float()
    lvo.lib().lvo_sincos_rad(C.c_float(float(a)), C.byref(ss), C.byref(cc))
    return F(ss.value), F(cc.value)


def _atan21(y, x):
    import ctypes as C
    return F(lvo.lib().lvo_atan2_det(C.c_float(float(y)), C.c_float(float(x))))


def _exp1(x):
    with np.errstate(all="ignore"):
        p = F(F(x) * LOG2E)
    if np.isnan(p):
        return F(np.nan)
    return F(lvo.pow_det(F(2.0), p)[0])


def _log1(x):
    return F(log_det(F(x)))


def _saturate1(x):                                                     # DXHelper.glsl:19-22
    if np.isinf(x):
        x = F(1.0)
    if np.isnan(x):
        return F(0.0)
    return min(max(x, F(0.0)), F(1.0))


def _mix1(x, y, a):
    return F(F(x * F(F(1.0) - a)) + F(y * a))


def _sqrt1(x):
    with np.errstate(all="ignore"):
        return F(np.sqrt(F(x)))


def _solve_quadratic1(c0, c1, c2):                                     # MomentMath.glsl:25-42
    c1 = F(c1 * F(0.5))
    tmp = F(F(c1 * c1) - F(c0 * c2))
    if c1 >= 0:
        tmp = _sqrt1(tmp)
        x1 = F(F(-c2) / F(c1 + tmp))
        x2 = F(F(F(-c1) - tmp) / c0)
    else:
        tmp = _sqrt1(tmp)
        x1 = F(F(F(-c1) + tmp) / c0)
        x2 = F(c2 / F(F(-c1) + tmp))
    return x1, x2


def _solve_cubic1(C0, C1, C2, C3):                                     # MomentMath.glsl:48-78
    x, y, z = F(C0 / C3), F(C1 / C3), F(C2 / C3)
    y, z = F(y / F(3.0)), F(z / F(3.0))
    Delta = [_fma1(-z, z, y), _fma1(-y, z, x), F(F(z * x) + F(F(-y) * y))]
    Discriminant = F(F(F(F(4.0) * Delta[0]) * Delta[2]) + F(F(-Delta[1]) * Delta[1]))
    Depressed = [_fma1(F(F(-2.0) * z), Delta[0], Delta[1]), Delta[0]]
    Theta = F(_atan21(_sqrt1(Discriminant), F(-Depressed[0])) / F(3.0))
    sn, cs = _sincos1(Theta)
    Root = [cs, F(F(F(-0.5) * cs) + F(F(-SQRT3_HALF) * sn)), F(F(F(-0.5) * cs) + F(SQRT3_HALF * sn))]
    k = F(F(2.0) * _sqrt1(F(-Depressed[1])))
    return [_fma1(k, r, F(-z)) for r in Root]


def _solve_cubic_blinn_smallest1(c0, c1, c2, c3):                      # MomentMath.glsl:83-99
    x, y, z = F(c0 / c3), F(c1 / c3), F(c2 / c3)
    y, z = F(y / F(3.0)), F(z / F(3.0))
    delta = [_fma1(-z, z, y), _fma1(-z, y, x), F(F(z * x) - F(y * y))]
    discriminant = F(F(F(F(4.0) * delta[0]) * delta[2]) - F(delta[1] * delta[1]))
    depressed = [delta[2], F(F(F(-x) * delta[1]) + F(F(F(2.0) * y) * delta[2]))]
    theta = F(abs(_atan21(F(x * _sqrt1(discriminant)), F(-depressed[1]))) / F(3.0))
    sn, cs = _sincos1(theta)
    tmp = F(F(2.0) * _sqrt1(F(-depressed[0])))
    xx = F(tmp * cs)
    xy = F(tmp * F(F(F(-0.5) * cs) - F(SQRT3_HALF * sn)))
    s = (F(-x), F(xx + y)) if F(xx + xy) < F(F(2.0) * y) else (F(-x), F(xy + y))
    return F(s[0] / s[1])


def _solve_quartic_neumark1(coeffs):                                   # MomentMath.glsl:104-152
    B, C, D, E = F(coeffs[3] / coeffs[4]), F(coeffs[2] / coeffs[4]), F(coeffs[1] / coeffs[4]), F(coeffs[0] / coeffs[4])
    P = F(F(-2.0) * C)
    Q = F(F(F(C * C) + F(B * D)) - F(F(4.0) * E))
    R = F(F(F(D * D) + F(F(B * B) * E)) - F(F(B * C) * D))
    y = _solve_cubic_blinn_smallest1(R, Q, P, F(1.0))
    BB = F(B * B)
    fy = F(F(4.0) * y)
    BB_fy = F(BB - fy)
    Z = F(C - y)
    ZZ = F(Z * Z)
    fE = F(F(4.0) * E)
    ZZ_fE = F(ZZ - fE)
    if y < 0 or F(F(ZZ + fE) * BB_fy) > F(ZZ_fE * F(BB + fy)):
        tmp = _sqrt1(BB_fy)
        G = F(F(B + tmp) * F(0.5))
        g = F(F(B - tmp) * F(0.5))
        tmp = F(F(F(B * Z) - F(F(2.0) * D)) / F(F(2.0) * tmp))
        H = _fma1(Z, F(0.5), tmp)
        h = _fma1(Z, F(0.5), F(-tmp))
    else:
        tmp = _sqrt1(ZZ_fE)
        H = F(F(Z + tmp) * F(0.5))
        h = F(F(Z - tmp) * F(0.5))
        tmp = F(F(F(B * Z) - F(F(2.0) * D)) / F(F(2.0) * tmp))
        G = _fma1(B, F(0.5), tmp)
        g = _fma1(B, F(0.5), F(-tmp))
    return list(_solve_quadratic1(F(1.0), G, H)) + list(_solve_quadratic1(F(1.0), g, h))


def _transmittance1(N, b_0, bn, depth, bias, over):
    """computeTransmittanceAtDepthFrom{4,6,8}PowerMoments; bn = the normalised b_1 ... b_N"""
    bias, over = F(bias), F(over)
    b = [_mix1(bn[i], F(BIAS_VECTOR[N][i]), bias) for i in range(N)]
    z = [F(depth)]
    if N == 4:                                                          # MomentMath.glsl:246-301
        L21D11 = _fma1(-b[0], b[1], b[2])
        D11 = _fma1(-b[0], b[0], b[1])
        InvD11 = F(F(1.0) / D11)
        L21 = F(L21D11 * InvD11)
        SquaredDepthVariance = _fma1(-b[1], b[1], b[3])
        D22 = _fma1(-L21D11, L21, SquaredDepthVariance)
        c = [F(1.0), z[0], F(z[0] * z[0])]
        c[1] = F(c[1] - b[0])
        c[2] = F(c[2] - F(b[1] + F(L21 * c[1])))
        c[1] = F(c[1] * InvD11)
        c[2] = F(c[2] / D22)
        c[1] = F(c[1] - F(L21 * c[2]))
        c[0] = F(c[0] - F(F(c[1] * b[0]) + F(c[2] * b[1])))
        InvC2 = F(F(1.0) / c[2])
        p = F(c[1] * InvC2)
        q = F(c[0] * InvC2)
        D = F(F(F(p * p) * F(0.25)) - q)
        r = _sqrt1(D)
        z.append(F(F(F(-p) * F(0.5)) - r))
        z.append(F(F(F(-p) * F(0.5)) + r))
        f0 = over
        f1 = F(1.0) if z[1] < z[0] else F(0.0)
        f2 = F(1.0) if z[2] < z[0] else F(0.0)
        f01 = F(F(f1 - f0) / F(z[1] - z[0]))
        f12 = F(F(f2 - f1) / F(z[2] - z[1]))
        f012 = F(F(f12 - f01) / F(z[2] - z[0]))
        polynomial = [f012, None, None]
        polynomial[1] = polynomial[0]
        polynomial[0] = F(f01 - F(polynomial[0] * z[1]))
        polynomial[2] = polynomial[1]
        polynomial[1] = F(polynomial[0] - F(polynomial[1] * z[0]))
        polynomial[0] = F(f0 - F(polynomial[0] * z[0]))
        absorbance = F(polynomial[0] + F(F(b[0] * polynomial[1]) + F(b[1] * polynomial[2])))
    elif N == 6:                                                        # MomentMath.glsl:305-385
        InvD11 = F(F(1.0) / _fma1(-b[0], b[0], b[1]))
        L21D11 = _fma1(-b[0], b[1], b[2])
        L21 = F(L21D11 * InvD11)
        D22 = _fma1(-L21D11, L21, _fma1(-b[1], b[1], b[3]))
        L31D11 = _fma1(-b[0], b[2], b[3])
        L31 = F(L31D11 * InvD11)
        InvD22 = F(F(1.0) / D22)
        L32D22 = _fma1(-L21D11, L31, _fma1(-b[1], b[2], b[4]))
        L32 = F(L32D22 * InvD22)
        D33 = F(_fma1(-b[2], b[2], b[5]) - F(F(L31D11 * L31) + F(L32D22 * L32)))
        InvD33 = F(F(1.0) / D33)
        c = [F(1.0), z[0], None, None]
        c[2] = F(c[1] * z[0])
        c[3] = F(c[2] * z[0])
        c[1] = F(c[1] - b[0])
        c[2] = F(c[2] - _fma1(L21, c[1], b[1]))
        c[3] = F(c[3] - F(b[2] + F(F(L31 * c[1]) + F(L32 * c[2]))))
        c[1], c[2], c[3] = F(c[1] * InvD11), F(c[2] * InvD22), F(c[3] * InvD33)
        c[2] = F(c[2] - F(L32 * c[3]))
        c[1] = F(c[1] - F(F(L21 * c[2]) + F(L31 * c[3])))
        c[0] = F(c[0] - F(F(F(b[0] * c[1]) + F(b[1] * c[2])) + F(b[2] * c[3])))
        z += _solve_cubic1(*c)
        f0 = over
        f1, f2, f3 = (F(0.0) if z[i] > z[0] else F(1.0) for i in (1, 2, 3))
        f01 = F(F(f1 - f0) / F(z[1] - z[0]))
        f12 = F(F(f2 - f1) / F(z[2] - z[1]))
        f23 = F(F(f3 - f2) / F(z[3] - z[2]))
        f012 = F(F(f12 - f01) / F(z[2] - z[0]))
        f123 = F(F(f23 - f12) / F(z[3] - z[1]))
        f0123 = F(F(f123 - f012) / F(z[3] - z[0]))
        polynomial = [None] * 4
        polynomial[0] = _fma1(-f0123, z[2], f012)
        polynomial[1] = f0123
        polynomial[2] = polynomial[1]
        polynomial[1] = _fma1(polynomial[1], -z[1], polynomial[0])
        polynomial[0] = _fma1(polynomial[0], -z[1], f01)
        polynomial[3] = polynomial[2]
        polynomial[2] = _fma1(polynomial[2], -z[0], polynomial[1])
        polynomial[1] = _fma1(polynomial[1], -z[0], polynomial[0])
        polynomial[0] = _fma1(polynomial[0], -z[0], f0)
        absorbance = F(F(F(F(polynomial[0] * F(1.0)) + F(polynomial[1] * b[0])) + F(polynomial[2] * b[1])) + F(polynomial[3] * b[2]))
    else:                                                               # MomentMath.glsl:389-505
        D22 = _fma1(-b[0], b[0], b[1])
        InvD22 = F(F(1.0) / D22)
        L32D22 = _fma1(-b[1], b[0], b[2])
        L32 = F(L32D22 * InvD22)
        L42D22 = _fma1(-b[2], b[0], b[3])
        L42 = F(L42D22 * InvD22)
        L52D22 = _fma1(-b[3], b[0], b[4])
        L52 = F(L52D22 * InvD22)
        D33 = _fma1(-L32, L32D22, _fma1(-b[1], b[1], b[3]))
        InvD33 = F(F(1.0) / D33)
        L43D33 = _fma1(-L42, L32D22, _fma1(-b[2], b[1], b[4]))
        L43 = F(L43D33 * InvD33)
        L53D33 = _fma1(-L52, L32D22, _fma1(-b[3], b[1], b[5]))
        L53 = F(L53D33 * InvD33)
        D44 = F(_fma1(-b[2], b[2], b[5]) - F(F(L42 * L42D22) + F(L43 * L43D33)))
        InvD44 = F(F(1.0) / D44)
        L54D44 = F(_fma1(-b[3], b[2], b[6]) - F(F(L52 * L42D22) + F(L53 * L43D33)))
        L54 = F(L54D44 * InvD44)
        D55 = F(_fma1(-b[3], b[3], b[7]) - F(F(F(L52 * L52D22) + F(L53 * L53D33)) + F(L54 * L54D44)))
        InvD55 = F(F(1.0) / D55)
        c = [F(1.0), z[0], None, None, None]
        c[2] = F(c[1] * z[0])
        c[3] = F(c[2] * z[0])
        c[4] = F(c[3] * z[0])
        c[1] = F(c[1] - b[0])
        c[2] = F(c[2] - _fma1(L32, c[1], b[1]))
        c[3] = F(c[3] - F(b[2] + F(F(L42 * c[1]) + F(L43 * c[2]))))
        c[4] = F(c[4] - F(b[3] + F(F(F(L52 * c[1]) + F(L53 * c[2])) + F(L54 * c[3]))))
        c[1], c[2], c[3], c[4] = F(c[1] * InvD22), F(c[2] * InvD33), F(c[3] * InvD44), F(c[4] * InvD55)
        c[3] = F(c[3] - F(L54 * c[4]))
        c[2] = F(c[2] - F(F(L53 * c[4]) + F(L43 * c[3])))
        c[1] = F(c[1] - F(F(F(L52 * c[4]) + F(L42 * c[3])) + F(L32 * c[2])))
        c[0] = F(c[0] - F(F(F(F(b[3] * c[4]) + F(b[2] * c[3])) + F(b[1] * c[2])) + F(b[0] * c[1])))
        z += _solve_quartic_neumark1(c)
        f0 = over
        f1, f2, f3, f4 = (F(1.0) if z[i] <= z[0] else F(0.0) for i in (1, 2, 3, 4))
        f01 = F(F(f1 - f0) / F(z[1] - z[0]))
        f12 = F(F(f2 - f1) / F(z[2] - z[1]))
        f23 = F(F(f3 - f2) / F(z[3] - z[2]))
        f34 = F(F(f4 - f3) / F(z[4] - z[3]))
        f012 = F(F(f12 - f01) / F(z[2] - z[0]))
        f123 = F(F(f23 - f12) / F(z[3] - z[1]))
        f234 = F(F(f34 - f23) / F(z[4] - z[2]))
        f0123 = F(F(f123 - f012) / F(z[3] - z[0]))
        f1234 = F(F(f234 - f123) / F(z[4] - z[1]))
        f01234 = F(F(f1234 - f0123) / F(z[4] - z[0]))
        Polynomial = [None] * 4
        Polynomial_0 = _fma1(-f01234, z[3], f0123)
        Polynomial[0] = f01234
        Polynomial[1] = Polynomial[0]
        Polynomial[0] = _fma1(-Polynomial[0], z[2], Polynomial_0)
        Polynomial_0 = _fma1(-Polynomial_0, z[2], f012)
        Polynomial[2] = Polynomial[1]
        Polynomial[1] = _fma1(-Polynomial[1], z[1], Polynomial[0])
        Polynomial[0] = _fma1(-Polynomial[0], z[1], Polynomial_0)
        Polynomial_0 = _fma1(-Polynomial_0, z[1], f01)
        Polynomial[3] = Polynomial[2]
        Polynomial[2] = _fma1(-Polynomial[2], z[0], Polynomial[1])
        Polynomial[1] = _fma1(-Polynomial[1], z[0], Polynomial[0])
        Polynomial[0] = _fma1(-Polynomial[0], z[0], Polynomial_0)
        Polynomial_0 = _fma1(-Polynomial_0, z[0], f0)
        absorbance = F(Polynomial_0 + F(F(F(F(Polynomial[0] * b[0]) + F(Polynomial[1] * b[1])) + F(Polynomial[2] * b[2])) +
                                        F(Polynomial[3] * b[3])))
    return _saturate1(_exp1(F(F(-b_0) * absorbance)))


def _fixed1(term):
    t = F(term)
    t = -FIXED_LIMIT if np.isnan(t) else min(max(t, -FIXED_LIMIT), FIXED_LIMIT)
    exact = Fraction(float(t)) * 2 ** FIXED_SHIFT
    n = math.floor(exact)
    rem = exact - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return n


def _unfixed1(n):
    return F(_round_fraction(Fraction(n), float(n)) * F(2.0 ** -FIXED_SHIFT))


def _pack1(v):
    r = 0
    for k in range(4):
        x = min(max(F(v[k]), F(0.0)), F(1.0))
        r |= int(np.floor(F(F(x * F(255.0)) + F(0.5)))) << (8 * k)
    return r


def _scalar_pixel(frags, N, background, log_min, log_max, over, bias):
    """frags: [(r, g, b, a, viewDepth)]; returns (rgba8, moments, degenerate)"""
    log_min, log_max = F(log_min), F(log_max)
    with np.errstate(all="ignore"):
        def warp(zv):                                                   # logDepthWarp, MBOITHeader.glsl:49-52
            return F(F(F(F(_log1(zv) - log_min) / F(log_max - log_min)) * F(2.0)) - F(1.0))
        sums = [0] * (1 + N)
        for r, g, b, a, zv in frags:                                    # MBOITPass1.glsl:44-52 + generateMoments, MomentOIT.glsl:324-375
            depth = warp(F(zv))
            transmittance = F(F(1.0) - F(a))
            if transmittance > F(0.9999999):
                continue
            absorbance = F(-_log1(transmittance))
            if absorbance > F(10.0):
                absorbance = F(10.0)
            depth_pow2 = F(depth * depth)
            depth_pow4 = F(depth_pow2 * depth_pow2)
            if N == 4:
                pw = [depth, depth_pow2, F(depth_pow2 * depth), depth_pow4]
            elif N == 6:
                pw = [depth, depth_pow2, F(depth_pow2 * depth), depth_pow4, F(depth_pow4 * depth), F(depth_pow4 * depth_pow2)]
            else:
                depth_pow6 = F(depth_pow4 * depth_pow2)
                pw = [depth, depth_pow2, F(depth_pow2 * depth), depth_pow4, F(depth_pow4 * depth), depth_pow6, F(depth_pow6 * depth),
                      F(depth_pow6 * depth_pow2)]
            sums[0] += _fixed1(absorbance)
            for k in range(N):
                sums[1 + k] += _fixed1(F(pw[k] * absorbance))
        bg = [F(v) for v in background]
        moments = np.zeros(1 + N, dtype=F)
        b_0 = _unfixed1(sums[0])
        if b_0 < B0_THRESHOLD:                                          # MomentOIT.glsl:421 / MBOITBlend.glsl:89: discard
            p = _pack1(bg)
            return np.array([(p >> (8 * k)) & 0xFF for k in range(4)], dtype=np.uint8), moments, False
        bn = [F(_unfixed1(sums[1 + k]) / b_0) for k in range(N)]         # b_even /= b_0; b_odd /= b_0
        moments[0] = b_0
        moments[1:] = bn
        acc = [0] * 4
        for r, g, b, a, zv in frags:                                    # MBOITPass2.glsl:21-37
            T = _transmittance1(N, b_0, bn, warp(F(zv)), bias, over)
            a = F(a)
            for k, cv in enumerate((r, g, b)):
                acc[k] += _fixed1(F(F(F(cv) * a) * T))
            acc[3] += _fixed1(F(a * T))
        if acc[3] == 0:                                                 # (this build's rule: the background, not 0 / 0)
            p = _pack1(bg)
            return np.array([(p >> (8 * k)) & 0xFF for k in range(4)], dtype=np.uint8), moments, True
        color = [_unfixed1(v) for v in acc]
        total_transmittance = _exp1(F(-b_0))                             # MBOITBlend.glsl:92
        alpha = F(F(1.0) - total_transmittance)                          # fragColor = vec4(color.rgb / color.a, 1.0 - total_transmittance)
        res = [F(F(F(color[k] / color[3]) * alpha) + F(bg[k] * F(F(1.0) - alpha))) for k in range(3)]
        res.append(F(alpha + F(bg[3] * F(F(1.0) - alpha))))
        p = _pack1(res)
        return np.array([(p >> (8 * k)) & 0xFF for k in range(4)], dtype=np.uint8), moments, False


# ---------------------------------------------------------------- inputs
LOG_MIN, LOG_MAX = F(math.log(0.5)), F(math.log(3.0))


def depth_to_view(d, log_min=LOG_MIN, log_max=LOG_MAX):
    """a view depth whose warped depth is (about) d"""
    d = np.asarray(d, dtype=np.float64)
    return np.exp((d + 1.0) * 0.5 * (float(log_max) - float(log_min)) + float(log_min)).astype(F)


def random_runs(rng, num_pixels, max_len, alpha_lo=0.001, alpha_hi=1.0, empty_share=0.2, min_len=1, depth_lo=-0.9, depth_hi=0.9):
    runs = []
    for _ in range(num_pixels):
        n = 0 if rng.random() < empty_share else int(rng.integers(min_len, max_len + 1))
        rgba = rng.random((n, 4)).astype(F)
        rgba[:, 3] = (alpha_lo + rgba[:, 3] * (alpha_hi - alpha_lo)).astype(F)
        runs.append((rgba, depth_to_view(rng.uniform(depth_lo, depth_hi, n))))
    return runs


def special_runs(rng):
    """empty pixels, single fragments, two fragments at one depth, alpha around 1e-7 and around 0.001, alpha = 1 (absorbance cap),
    depths outside [-1, 1]"""
    runs = [(np.zeros((0, 4), F), np.zeros(0, F))]
    for _ in range(12):
        runs += random_runs(rng, 1, 1, empty_share=0.0)
    for _ in range(6):
        r = random_runs(rng, 1, 2, empty_share=0.0, min_len=2)[0]
        r[1][1] = r[1][0]
        runs.append(r)
    for lo, hi in ((5e-8, 2e-7), (0.0009, 0.0011)):
        for n in (1, 2, 5):
            runs += random_runs(rng, 3, n, alpha_lo=lo, alpha_hi=hi, empty_share=0.0, min_len=n)
    for n in (1, 3):
        r = random_runs(rng, 1, n, empty_share=0.0, min_len=n)[0]
        r[0][:, 3] = F(1.0)
        runs.append(r)
        r = random_runs(rng, 1, n + 1, empty_share=0.0, min_len=n + 1)[0]
        r[0][0, 3] = F(1.0)
        runs.append(r)
    runs += random_runs(rng, 8, 6, empty_share=0.0, depth_lo=-1.4, depth_hi=1.4)
    return runs


def _check(runs, N, bg=(0.2, 0.4, 0.6, 1.0), over=0.1, bias=None):
    bias = MOMENT_BIAS[N] if bias is None else bias
    frame, moments, degenerate = mboit_fold(runs, N, bg, LOG_MIN, LOG_MAX, over, bias, details=True)
    count = 0
    for p, (rgba, z) in enumerate(runs):
        ref, mom, deg = _scalar_pixel([tuple(rgba[i]) + (z[i],) for i in range(len(z))], N, bg, LOG_MIN, LOG_MAX, over, bias)
        assert np.array_equal(frame[p], ref), (p, N, frame[p], ref)
        assert np.array_equal(moments[p].view(U32), mom.view(U32)), (p, N, moments[p], mom)
        count += int(deg)
    assert count == degenerate


# ---------------------------------------------------------------- tests
def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(1)
    n = 4000
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F)
    c[: n // 2] = (-(a[: n // 2].astype(np.float64) * b[: n // 2].astype(np.float64))).astype(F)   # cancelling: c = -round(a b)
    # halfway cases of the double rounding: a b + c lands next to a float32 tie
    a[-200:] = (F(1.0) + rng.integers(0, 1 << 23, 200).astype(F) * F(2.0 ** -23)).astype(F)
    b[-200:] = (F(1.0) + F(2.0 ** -12)) * np.ones(200, F)
    c[-200:] = (rng.integers(-3, 4, 200) * 2.0 ** -40).astype(F)
    got = fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = _round_fraction(exact, float(a[i]) * float(b[i]) + float(c[i]))
        assert got[i].view(U32) == want.view(U32), (a[i], b[i], c[i], got[i], want)
    assert (got[: n // 2] != 0).sum() > n // 4   # the cancelling cases keep the product's low bits (a two-rounding a * b + c gives 0)


def test_transcendentals_of_the_statement():
    rng = np.random.default_rng(2)
    p = np.concatenate([rng.uniform(-20.0, 20.0, 20000), rng.uniform(-130.0, 130.0, 2000), [0.0, -125.0, 127.0, 0.5, -0.5]]).astype(F)
    assert np.array_equal(exp2_det(p).view(U32), lvo.pow_det(F(2.0), p).view(U32))
    x = rng.uniform(-14.0, 3.0, 20000).astype(F)
    got = exp_det(x).astype(np.float64)
    want = np.exp(x.astype(np.float64))
    big = want > 1e-4
    assert np.abs(got[big] / want[big] - 1.0).max() < 3e-6 and np.abs(got[~big] - want[~big]).max() < 1e-9   # pow_det's bounds (test_oracle.py)
    v = np.concatenate([rng.uniform(1e-4, 1.0, 20000), 10.0 ** rng.uniform(-6, 3, 5000)]).astype(F)
    lg = log_det(v).astype(np.float64)
    want = np.log(v.astype(np.float64))
    far = np.abs(want) > 0.1
    assert np.abs(lg[far] / want[far] - 1.0).max() < 3e-6 and np.abs(lg[~far] - want[~far]).max() < 3e-7
    a = np.concatenate([rng.uniform(-7.0, 7.0, 3000), [0.0, np.nan, np.inf]]).astype(F)
    s, c = sincos_det(a)
    for i in range(len(a)):
        ss, cc = _sincos1(a[i])
        assert s[i].view(U32) == ss.view(U32) and c[i].view(U32) == cc.view(U32), a[i]
    y = np.concatenate([rng.standard_normal(3000), [0.0, 0.0, 1.0, -1.0, np.nan]]).astype(F)
    xx = np.concatenate([rng.standard_normal(3000), [0.0, -1.0, 0.0, 0.0, 1.0]]).astype(F)
    t = atan2_det(y, xx)
    for i in range(len(y)):
        assert t[i].view(U32) == _atan21(y[i], xx[i]).view(U32), (y[i], xx[i])


def test_fold_matches_the_scalar_transcription():
    for N in (4, 6, 8):
        rng = np.random.default_rng(10 + N)
        _check(random_runs(rng, 40, 16), N)
        _check(special_runs(rng), N)
        _check(random_runs(rng, 12, 8), N, over=0.4, bias=10.0 * MOMENT_BIAS[N])


def test_any_order_gives_the_same_bits_and_runs_can_be_split():
    rng = np.random.default_rng(23)
    runs = random_runs(rng, 50, 40)
    shuffled = []
    for rgba, z in runs:
        o = rng.permutation(len(z))
        shuffled.append((rgba[o], z[o]))
    for N in (4, 6, 8):
        f0, m0 = mboit_fold(runs, N, (0, 0, 0, 0), LOG_MIN, LOG_MAX)
        f1, m1 = mboit_fold(shuffled, N, (0, 0, 0, 0), LOG_MIN, LOG_MAX)
        assert np.array_equal(f0, f1) and np.array_equal(m0.view(U32), m1.view(U32))
    # a run split in two: the integer sums of the parts add up to the sums of the whole
    rgba = np.concatenate([r[0] for r in runs])
    z = np.concatenate([r[1] for r in runs])
    zero = np.zeros(len(z), dtype=np.int64)
    whole, _ = mboit_sums(rgba, z, zero, 1, 8, LOG_MIN, LOG_MAX)
    h = len(z) // 3
    a, _ = mboit_sums(rgba[:h], z[:h], zero[:h], 1, 8, LOG_MIN, LOG_MAX)
    b, _ = mboit_sums(rgba[h:], z[h:], zero[h:], 1, 8, LOG_MIN, LOG_MAX)
    assert np.array_equal(whole, a + b) and whole[0, 0] > 0


def degenerate_count(N, bias, max_len, seed, n=3000):
    """pixels of one ... max_len fragments (depth uniform in [-0.9, 0.9], alpha uniform in [0.001, 1)) that end with a_sum == 0"""
    rng = np.random.default_rng(seed)
    runs = random_runs(rng, n, max_len, empty_share=0.0)
    return mboit_fold(runs, N, (0, 0, 0, 1), LOG_MIN, LOG_MAX, 0.1, bias, details=True)[2]


def test_degenerate_pixels_fall_with_the_bias():
    """DESIGN.md 6 quotes these counts; asserted in direction only: a larger bias does not increase the count, and at the largest
    bias tried -- 0.1, the largest mboit_moment_bias accepts -- the count for single fragments is 0.  (The statement does not confirm
    the prototype's 0 at 5e-4 for N = 4: 1 of 3000 single fragments still degenerates there.)"""
    for N in (4, 6, 8):
        ladder = [MOMENT_BIAS[N] * 10.0 ** k for k in range(4)] + [0.1]
        for max_len in (1, 2):
            counts = [degenerate_count(N, bias, max_len, 40 + max_len) for bias in ladder]
            print("degenerate of 3000, N = %d, 1 ... %d fragments, bias x 1 / 10 / 100 / 1000 and 0.1:" % (N, max_len), counts)
            assert all(counts[k + 1] <= counts[k] for k in range(4)), (N, max_len, counts)
            if max_len == 1:
                assert counts[-1] == 0, (N, counts)


def _exact_blend(runs, bg):
    """front-to-back compositing in float64, sorted by depth"""
    out = np.zeros((len(runs), 4))
    for p, (rgba, z) in enumerate(runs):
        o = np.argsort(z, kind="stable")
        col, tr = np.zeros(3), 1.0
        for i in o:
            a = float(rgba[i, 3])
            col += tr * a * rgba[i, :3].astype(np.float64)
            tr *= 1.0 - a
        out[p, :3] = col + tr * np.asarray(bg[:3], dtype=np.float64)
        out[p, 3] = (1.0 - tr) + tr * bg[3]
    return out * 255.0


def test_single_fragment_equals_the_straight_alpha_blend():
    rng = np.random.default_rng(31)
    runs = random_runs(rng, 400, 1, empty_share=0.0, alpha_lo=0.01)
    bg = (0.9, 0.8, 0.1, 1.0)
    for N in (4, 6, 8):
        frame, _, deg = mboit_fold(runs, N, bg, LOG_MIN, LOG_MAX, 0.1, 1000.0 * MOMENT_BIAS[N], details=True)
        assert deg == 0
        assert np.abs(frame.astype(np.float64) - _exact_blend(runs, bg)).max() <= 1.0


def test_depth_decides_which_of_two_fragments_dominates():
    red, blue = [1.0, 0.0, 0.0, 0.7], [0.0, 0.0, 1.0, 0.7]
    near, far = depth_to_view(-0.6), depth_to_view(0.6)
    for N in (4, 6, 8):
        runs = [(np.array([red, blue], F), np.array([near, far], F)), (np.array([red, blue], F), np.array([far, near], F))]
        frame, _ = mboit_fold(runs, N, (0.0, 0.0, 0.0, 1.0), LOG_MIN, LOG_MAX, 0.1, 100.0 * MOMENT_BIAS[N])
        assert not np.array_equal(frame[0], frame[1])
        assert frame[0][0] > frame[0][2] and frame[1][2] > frame[1][0]   # red in front in the first, blue in the second


# mean error (LSB) of the statement against exact front-to-back blending on dense runs of 3 ... 40 fragments with alpha <= 0.1, as
# measured with the seed below (DESIGN.md 6 has mean and maximum); the bound is the measured mean x 1.5 -- the margin covers a change
# of seed, nothing else
DENSE_MEAN_LSB = {4: 1.002, 6: 0.762, 8: 0.647}   # (maxima: 8.4, 5.6, 4.6 LSB)


def dense_error(N, seed=57, n=1500):
    rng = np.random.default_rng(seed)
    runs = random_runs(rng, n, 40, alpha_lo=0.001, alpha_hi=0.1, empty_share=0.0, min_len=3)
    bg = (1.0, 1.0, 1.0, 1.0)
    frame, _, deg = mboit_fold(runs, N, bg, LOG_MIN, LOG_MAX, details=True)
    err = np.abs(frame.astype(np.float64) - _exact_blend(runs, bg))[:, :3]
    return float(err.mean()), float(err.max()), deg


def test_dense_runs_stay_near_exact_compositing():
    for N in (4, 6, 8):
        mean, mx, deg = dense_error(N)
        print("dense runs, N = %d: mean %.3f LSB, max %.1f LSB, degenerate %d" % (N, mean, mx, deg))
        assert deg == 0
        assert mean <= 1.5 * DENSE_MEAN_LSB[N], (N, mean, mx)
