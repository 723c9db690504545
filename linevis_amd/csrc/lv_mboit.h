// Moment-based order-independent transparency (rendering mode 6): the arithmetic of MBOITPass1/2.glsl, MomentOIT.glsl and
// MomentMath.glsl for power moments (4 / 6 / 8, float32) under the numerics contract of DESIGN.md 4 -- float32, one operation at a
// time (-ffp-contract=off), __builtin_fmaf exactly where the shaders write fma(), the build's fixed log / exp / atan2 / sin / cos,
// per-pixel sums as 64-bit fixed point.  tests/test_mboit_restatement.py states the same on the CPU, bit for bit.
#pragma once
#include "lv_device.h"

#define LV_MBOIT_FIXED_SCALE 68719476736.0          // 2^36: 65534 fragments x |term| <= 1024 stays below 2^63
#define LV_MBOIT_FIXED_INV 1.4551915228366852e-11f  // 2^-36
#define LV_MBOIT_FIXED_LIMIT 1024.0f                // a term outside [-1024, 1024] saturates (NaN -> -1024)
#define LV_MBOIT_B0_MIN 0.00100050033f              // MomentOIT.glsl:421, MBOITBlend.glsl:89
#define LV_MBOIT_SQRT3_HALF 0.866025388f            // 0.5f * sqrt(3.0f)

struct LvMboitParams {
    float logDepthMin, logDepthMax;   // computeDepthRange, MBOITRenderer.cpp:484-503
    float overestimation, momentBias; // MomentOITUniformData
    uint32_t stats;                   // collect_stats: count the degenerate pixels
};

// exp2(p): the second half of lv_pow_det (lv_pow_det(2, p) bit for bit); a NaN stays a NaN
__device__ __forceinline__ float lv_exp2_det(float p) {
    if (p != p) return p;
    if (p < -125.0f) return 0.0f;
    if (p > 127.0f) return __builtin_inff();
    const float n = floorf(p + 0.5f);
    const float t = (p - n) * 0.693147181f;
    const float Q = 1.0f + t * (1.0f + t * (0.5f + t * (0.166666667f + t * (0.0416666667f + t * (0.00833333333f + t * (0.00138888889f + t * 0.000198412698f))))));
    return __uint_as_float(__float_as_uint(Q) + (uint32_t(int(n)) << 23));
}
__device__ __forceinline__ float lv_exp_det(float x) { return lv_exp2_det(x * 1.44269504f); }
__device__ __forceinline__ float lv_log_det(float x) { return lv_log2_det(x) * 0.693147181f; }
// saturate, DXHelper.glsl:19-22: +-inf -> 1; the clamp as fminf(fmaxf(x, 0), 1) turns a NaN into 0
__device__ __forceinline__ float lv_mboit_saturate(float x) {
    if (__builtin_isinf(x)) x = 1.0f;
    return fminf(fmaxf(x, 0.0f), 1.0f);
}
__device__ __forceinline__ float lv_mboit_mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
__device__ __forceinline__ long long lv_mboit_fixed(float t) {
    t = fminf(fmaxf(t, -LV_MBOIT_FIXED_LIMIT), LV_MBOIT_FIXED_LIMIT);
    return (long long)__builtin_rint(double(t) * LV_MBOIT_FIXED_SCALE);   // ties to even
}
__device__ __forceinline__ float lv_mboit_unfixed(long long s) { return float(s) * LV_MBOIT_FIXED_INV; }
// logDepthWarp, MBOITHeader.glsl:49-52
__device__ __forceinline__ float lv_mboit_warp(float z, const LvMboitParams& M) {
    return (lv_log_det(z) - M.logDepthMin) / (M.logDepthMax - M.logDepthMin) * 2.0f - 1.0f;
}

// solveQuadratic(vec3(1, c1, c2)), MomentMath.glsl:25-42
__device__ __forceinline__ void lv_mboit_quadratic(float c1, float c2, float& x1, float& x2) {
    c1 *= 0.5f;
    const float tmp = sqrtf(c1 * c1 - c2);
    if (c1 >= 0.0f) { x1 = (-c2) / (c1 + tmp); x2 = -c1 - tmp; }
    else { x1 = -c1 + tmp; x2 = c2 / (-c1 + tmp); }
}
// SolveCubic, MomentMath.glsl:48-78
__device__ __forceinline__ void lv_mboit_cubic(float c0, float c1, float c2, float c3, float& r0, float& r1, float& r2) {
    const float x = c0 / c3;
    const float y = (c1 / c3) / 3.0f, z = (c2 / c3) / 3.0f;
    const float dx = __builtin_fmaf(-z, z, y), dy = __builtin_fmaf(-y, z, x), dz = z * x + (-y) * y;
    const float disc = (4.0f * dx) * dz + (-dy) * dy;
    const float depx = __builtin_fmaf(-2.0f * z, dx, dy), depy = dx;
    const float theta = lv_atan2_det(sqrtf(disc), -depx) / 3.0f;
    float sn, cs;
    lv_sincos_rad(theta, sn, cs);
    const float k = 2.0f * sqrtf(-depy);
    r0 = __builtin_fmaf(k, cs, -z);
    r1 = __builtin_fmaf(k, -0.5f * cs + (-LV_MBOIT_SQRT3_HALF) * sn, -z);
    r2 = __builtin_fmaf(k, -0.5f * cs + LV_MBOIT_SQRT3_HALF * sn, -z);
}
// solveCubicBlinnSmallest(vec4(c0, c1, c2, 1)), MomentMath.glsl:83-99
__device__ __forceinline__ float lv_mboit_cubic_smallest(float c0, float c1, float c2) {
    const float x = c0, y = c1 / 3.0f, z = c2 / 3.0f;
    const float dx = __builtin_fmaf(-z, z, y), dy = __builtin_fmaf(-z, y, x), dz = z * x - y * y;
    const float disc = (4.0f * dx) * dz - dy * dy;
    const float depx = dz, depy = (-x) * dy + (2.0f * y) * dz;
    const float theta = fabsf(lv_atan2_det(x * sqrtf(disc), -depy)) / 3.0f;
    float sn, cs;
    lv_sincos_rad(theta, sn, cs);
    const float tmp = 2.0f * sqrtf(-depx);
    const float xx = tmp * cs, xy = tmp * (-0.5f * cs - LV_MBOIT_SQRT3_HALF * sn);
    const float sy = (xx + xy < 2.0f * y) ? xx + y : xy + y;
    return (-x) / sy;
}
// solveQuarticNeumark, MomentMath.glsl:104-152
__device__ __forceinline__ void lv_mboit_quartic(const float c[5], float z[4]) {
    const float B = c[3] / c[4], C = c[2] / c[4], D = c[1] / c[4], E = c[0] / c[4];
    const float P = -2.0f * C;
    const float Q = (C * C + B * D) - 4.0f * E;
    const float R = (D * D + (B * B) * E) - (B * C) * D;
    const float y = lv_mboit_cubic_smallest(R, Q, P);
    const float BB = B * B, fy = 4.0f * y, BB_fy = BB - fy;
    const float Z = C - y, ZZ = Z * Z, fE = 4.0f * E, ZZ_fE = ZZ - fE;
    float G, g, H, h;
    if (y < 0.0f || (ZZ + fE) * BB_fy > ZZ_fE * (BB + fy)) {
        float tmp = sqrtf(BB_fy);
        G = (B + tmp) * 0.5f;
        g = (B - tmp) * 0.5f;
        tmp = (B * Z - 2.0f * D) / (2.0f * tmp);
        H = __builtin_fmaf(Z, 0.5f, tmp);
        h = __builtin_fmaf(Z, 0.5f, -tmp);
    } else {
        float tmp = sqrtf(ZZ_fE);
        H = (Z + tmp) * 0.5f;
        h = (Z - tmp) * 0.5f;
        tmp = (B * Z - 2.0f * D) / (2.0f * tmp);
        G = __builtin_fmaf(B, 0.5f, tmp);
        g = __builtin_fmaf(B, 0.5f, -tmp);
    }
    lv_mboit_quadratic(G, H, z[0], z[1]);
    lv_mboit_quadratic(g, h, z[2], z[3]);
}

// bias vectors of the SINGLE_PRECISION path, MomentOIT.glsl:450,505,547
template <int N> __device__ __forceinline__ float lv_mboit_bias_vector(int i);
template <> __device__ __forceinline__ float lv_mboit_bias_vector<4>(int i) { return (i & 1) ? 0.375f : 0.0f; }
template <> __device__ __forceinline__ float lv_mboit_bias_vector<6>(int i) { return i == 1 ? 0.48f : i == 3 ? 0.451f : i == 5 ? 0.45f : 0.0f; }
template <> __device__ __forceinline__ float lv_mboit_bias_vector<8>(int i) {
    return i == 1 ? 0.75f : i == 3 ? 0.67666666666666664f : i == 5 ? 0.63f : i == 7 ? 0.60030303030303034f : 0.0f;
}

// computeTransmittanceAtDepthFrom{4,6,8}PowerMoments (MomentMath.glsl:246-301, 305-385, 389-505): bn = the normalised b_1 ... b_N
// after the bias (lv_mboit_biased), z0 = the warped depth of the fragment
template <int N> __device__ __forceinline__ void lv_mboit_biased(float* b, float bias) {
#pragma unroll
    for (int i = 0; i < N; i++) b[i] = lv_mboit_mix(b[i], lv_mboit_bias_vector<N>(i), bias);
}

// The factorisation of the Hankel matrix depends on the pixel's moments only: computed once per pixel (same operations, same
// results as the shader's per-fragment evaluation), the fragments then run the substitution, the root finder and the weights.
template <int N> struct LvMboitPixel;

template <> struct LvMboitPixel<4> {
    float b[4], L21, InvD11, D22;
    __device__ __forceinline__ void setup() {
        const float L21D11 = __builtin_fmaf(-b[0], b[1], b[2]);
        const float D11 = __builtin_fmaf(-b[0], b[0], b[1]);
        InvD11 = 1.0f / D11;
        L21 = L21D11 * InvD11;
        const float SquaredDepthVariance = __builtin_fmaf(-b[1], b[1], b[3]);
        D22 = __builtin_fmaf(-L21D11, L21, SquaredDepthVariance);
    }
    __device__ __forceinline__ float absorbance(float z0, float over) const {
        float c0 = 1.0f, c1 = z0, c2 = z0 * z0;
        c1 -= b[0];
        c2 -= b[1] + L21 * c1;
        c1 *= InvD11;
        c2 /= D22;
        c1 -= L21 * c2;
        c0 -= c1 * b[0] + c2 * b[1];
        const float InvC2 = 1.0f / c2;
        const float p = c1 * InvC2, q = c0 * InvC2;
        const float D = (p * p) * 0.25f - q;
        const float r = sqrtf(D);
        const float z1 = (-p) * 0.5f - r, z2 = (-p) * 0.5f + r;
        const float f0 = over, f1 = z1 < z0 ? 1.0f : 0.0f, f2 = z2 < z0 ? 1.0f : 0.0f;
        const float f01 = (f1 - f0) / (z1 - z0);
        const float f12 = (f2 - f1) / (z2 - z1);
        const float f012 = (f12 - f01) / (z2 - z0);
        float p0 = f012, p1, p2;
        p1 = p0;
        p0 = f01 - p0 * z1;
        p2 = p1;
        p1 = p0 - p1 * z0;
        p0 = f0 - p0 * z0;
        return p0 + (b[0] * p1 + b[1] * p2);
    }
};

template <> struct LvMboitPixel<6> {
    float b[6], InvD11, InvD22, InvD33, L21, L31, L32;
    __device__ __forceinline__ void setup() {
        InvD11 = 1.0f / __builtin_fmaf(-b[0], b[0], b[1]);
        const float L21D11 = __builtin_fmaf(-b[0], b[1], b[2]);
        L21 = L21D11 * InvD11;
        const float D22 = __builtin_fmaf(-L21D11, L21, __builtin_fmaf(-b[1], b[1], b[3]));
        const float L31D11 = __builtin_fmaf(-b[0], b[2], b[3]);
        L31 = L31D11 * InvD11;
        InvD22 = 1.0f / D22;
        const float L32D22 = __builtin_fmaf(-L21D11, L31, __builtin_fmaf(-b[1], b[2], b[4]));
        L32 = L32D22 * InvD22;
        const float D33 = __builtin_fmaf(-b[2], b[2], b[5]) - (L31D11 * L31 + L32D22 * L32);
        InvD33 = 1.0f / D33;
    }
    __device__ __forceinline__ float absorbance(float z0, float over) const {
        float c0 = 1.0f, c1 = z0, c2 = c1 * z0, c3 = c2 * z0;
        c1 -= b[0];
        c2 -= __builtin_fmaf(L21, c1, b[1]);
        c3 -= b[2] + (L31 * c1 + L32 * c2);
        c1 *= InvD11; c2 *= InvD22; c3 *= InvD33;
        c2 -= L32 * c3;
        c1 -= L21 * c2 + L31 * c3;
        c0 -= (b[0] * c1 + b[1] * c2) + b[2] * c3;
        float z1, z2, z3;
        lv_mboit_cubic(c0, c1, c2, c3, z1, z2, z3);
        const float f0 = over, f1 = z1 > z0 ? 0.0f : 1.0f, f2 = z2 > z0 ? 0.0f : 1.0f, f3 = z3 > z0 ? 0.0f : 1.0f;
        const float f01 = (f1 - f0) / (z1 - z0);
        const float f12 = (f2 - f1) / (z2 - z1);
        const float f23 = (f3 - f2) / (z3 - z2);
        const float f012 = (f12 - f01) / (z2 - z0);
        const float f123 = (f23 - f12) / (z3 - z1);
        const float f0123 = (f123 - f012) / (z3 - z0);
        float p0, p1, p2, p3;
        p0 = __builtin_fmaf(-f0123, z2, f012);
        p1 = f0123;
        p2 = p1;
        p1 = __builtin_fmaf(p1, -z1, p0);
        p0 = __builtin_fmaf(p0, -z1, f01);
        p3 = p2;
        p2 = __builtin_fmaf(p2, -z0, p1);
        p1 = __builtin_fmaf(p1, -z0, p0);
        p0 = __builtin_fmaf(p0, -z0, f0);
        return ((p0 + p1 * b[0]) + p2 * b[1]) + p3 * b[2];
    }
};

template <> struct LvMboitPixel<8> {
    float b[8], InvD22, InvD33, InvD44, InvD55, L32, L42, L52, L43, L53, L54;
    __device__ __forceinline__ void setup() {
        const float D22 = __builtin_fmaf(-b[0], b[0], b[1]);
        InvD22 = 1.0f / D22;
        const float L32D22 = __builtin_fmaf(-b[1], b[0], b[2]);
        L32 = L32D22 * InvD22;
        const float L42D22 = __builtin_fmaf(-b[2], b[0], b[3]);
        L42 = L42D22 * InvD22;
        const float L52D22 = __builtin_fmaf(-b[3], b[0], b[4]);
        L52 = L52D22 * InvD22;
        const float D33 = __builtin_fmaf(-L32, L32D22, __builtin_fmaf(-b[1], b[1], b[3]));
        InvD33 = 1.0f / D33;
        const float L43D33 = __builtin_fmaf(-L42, L32D22, __builtin_fmaf(-b[2], b[1], b[4]));
        L43 = L43D33 * InvD33;
        const float L53D33 = __builtin_fmaf(-L52, L32D22, __builtin_fmaf(-b[3], b[1], b[5]));
        L53 = L53D33 * InvD33;
        const float D44 = __builtin_fmaf(-b[2], b[2], b[5]) - (L42 * L42D22 + L43 * L43D33);
        InvD44 = 1.0f / D44;
        const float L54D44 = __builtin_fmaf(-b[3], b[2], b[6]) - (L52 * L42D22 + L53 * L43D33);
        L54 = L54D44 * InvD44;
        const float D55 = __builtin_fmaf(-b[3], b[3], b[7]) - ((L52 * L52D22 + L53 * L53D33) + L54 * L54D44);
        InvD55 = 1.0f / D55;
    }
    __device__ __forceinline__ float absorbance(float z0, float over) const {
        float c[5];
        c[0] = 1.0f;
        c[1] = z0;
        c[2] = c[1] * z0;
        c[3] = c[2] * z0;
        c[4] = c[3] * z0;
        c[1] -= b[0];
        c[2] -= __builtin_fmaf(L32, c[1], b[1]);
        c[3] -= b[2] + (L42 * c[1] + L43 * c[2]);
        c[4] -= b[3] + ((L52 * c[1] + L53 * c[2]) + L54 * c[3]);
        c[1] *= InvD22; c[2] *= InvD33; c[3] *= InvD44; c[4] *= InvD55;
        c[3] -= L54 * c[4];
        c[2] -= L53 * c[4] + L43 * c[3];
        c[1] -= (L52 * c[4] + L42 * c[3]) + L32 * c[2];
        c[0] -= ((b[3] * c[4] + b[2] * c[3]) + b[1] * c[2]) + b[0] * c[1];
        float z[4];
        lv_mboit_quartic(c, z);
        const float z1 = z[0], z2 = z[1], z3 = z[2], z4 = z[3];
        const float f0 = over, f1 = z1 <= z0 ? 1.0f : 0.0f, f2 = z2 <= z0 ? 1.0f : 0.0f, f3 = z3 <= z0 ? 1.0f : 0.0f,
                    f4 = z4 <= z0 ? 1.0f : 0.0f;
        const float f01 = (f1 - f0) / (z1 - z0);
        const float f12 = (f2 - f1) / (z2 - z1);
        const float f23 = (f3 - f2) / (z3 - z2);
        const float f34 = (f4 - f3) / (z4 - z3);
        const float f012 = (f12 - f01) / (z2 - z0);
        const float f123 = (f23 - f12) / (z3 - z1);
        const float f234 = (f34 - f23) / (z4 - z2);
        const float f0123 = (f123 - f012) / (z3 - z0);
        const float f1234 = (f234 - f123) / (z4 - z1);
        const float f01234 = (f1234 - f0123) / (z4 - z0);
        float P_0, P0, P1, P2, P3;
        P_0 = __builtin_fmaf(-f01234, z3, f0123);
        P0 = f01234;
        P1 = P0;
        P0 = __builtin_fmaf(-P0, z2, P_0);
        P_0 = __builtin_fmaf(-P_0, z2, f012);
        P2 = P1;
        P1 = __builtin_fmaf(-P1, z1, P0);
        P0 = __builtin_fmaf(-P0, z1, P_0);
        P_0 = __builtin_fmaf(-P_0, z1, f01);
        P3 = P2;
        P2 = __builtin_fmaf(-P2, z0, P1);
        P1 = __builtin_fmaf(-P1, z0, P0);
        P0 = __builtin_fmaf(-P0, z0, P_0);
        P_0 = __builtin_fmaf(-P_0, z0, f0);
        return P_0 + (((P0 * b[0] + P1 * b[1]) + P2 * b[2]) + P3 * b[3]);
    }
};

// sweep 1 of one fragment (MBOITPass1.glsl:44-52 + generateMoments, MomentOIT.glsl:324-375): adds to s[0 ... N]
template <int N>
__device__ __forceinline__ void lv_mboit_moments(float alpha, float viewDepth, const LvMboitParams& M, long long* s) {
    const float transmittance = 1.0f - alpha;
    if (transmittance > 0.9999999f) return;
    float absorbance = -lv_log_det(transmittance);
    if (absorbance > 10.0f) absorbance = 10.0f;   // ABSORBANCE_MAX_VALUE
    const float d = lv_mboit_warp(viewDepth, M);
    const float d2 = d * d, d4 = d2 * d2;
    s[0] += lv_mboit_fixed(absorbance);
    s[1] += lv_mboit_fixed(d * absorbance);
    s[2] += lv_mboit_fixed(d2 * absorbance);
    s[3] += lv_mboit_fixed((d2 * d) * absorbance);
    s[4] += lv_mboit_fixed(d4 * absorbance);
    if (N >= 6) s[5] += lv_mboit_fixed((d4 * d) * absorbance);
    if (N == 6) s[6] += lv_mboit_fixed((d4 * d2) * absorbance);
    if (N == 8) {
        const float d6 = d4 * d2;
        s[6] += lv_mboit_fixed(d6 * absorbance);
        s[7] += lv_mboit_fixed((d6 * d) * absorbance);
        s[8] += lv_mboit_fixed((d6 * d2) * absorbance);
    }
}
// the pixel after sweep 1: b_0 and, when it reaches the threshold, the normalised, biased moments and their factorisation
template <int N>
__device__ __forceinline__ bool lv_mboit_pixel(const long long* s, const LvMboitParams& M, float& b_0, float* normalised, LvMboitPixel<N>& X) {
    b_0 = lv_mboit_unfixed(s[0]);
    if (b_0 < LV_MBOIT_B0_MIN) return false;
#pragma unroll
    for (int k = 0; k < N; k++) { normalised[k] = lv_mboit_unfixed(s[1 + k]) / b_0; X.b[k] = normalised[k]; }
    lv_mboit_biased<N>(X.b, M.momentBias);
    X.setup();
    return true;
}
// sweep 2 of one fragment (MBOITPass2.glsl:21-37): adds (rgb * a * T, a * T) to c[0 ... 3]
template <int N>
__device__ __forceinline__ void lv_mboit_colour(const f4& color, float viewDepth, float b_0, const LvMboitPixel<N>& X,
                                                const LvMboitParams& M, long long* c) {
    const float T = lv_mboit_saturate(lv_exp_det((-b_0) * X.absorbance(lv_mboit_warp(viewDepth, M), M.overestimation)));
    c[0] += lv_mboit_fixed((color.x * color.w) * T);
    c[1] += lv_mboit_fixed((color.y * color.w) * T);
    c[2] += lv_mboit_fixed((color.z * color.w) * T);
    c[3] += lv_mboit_fixed(color.w * T);
}
// MBOITBlend.glsl:87-101, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour as the resolve passes of modes 2 and 3 write
// it; a_sum == 0 (every fragment's transmittance reconstructed to 0 or NaN) shows the background
__device__ __forceinline__ uint32_t lv_mboit_blend(const LvUniforms& U, bool covered, float b_0, const long long* c) {
    f4 r;
    r.x = U.background[0]; r.y = U.background[1]; r.z = U.background[2]; r.w = U.background[3];
    if (covered && c[3] != 0) {
        const float asum = lv_mboit_unfixed(c[3]);
        const float a = 1.0f - lv_exp_det(-b_0);
        r.x = (lv_mboit_unfixed(c[0]) / asum) * a + U.background[0] * (1.0f - a);
        r.y = (lv_mboit_unfixed(c[1]) / asum) * a + U.background[1] * (1.0f - a);
        r.z = (lv_mboit_unfixed(c[2]) / asum) * a + U.background[2] * (1.0f - a);
        r.w = a + U.background[3] * (1.0f - a);
    }
    return lv_pack_unorm4x8(r);
}
