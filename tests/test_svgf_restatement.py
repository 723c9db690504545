"""A float64 statement of the whole SVGFDenoiser::denoise() chain, written from Data/Shaders/Denoiser/SVGF.glsl (reproject, filter
moments, a-trous), svgf_common.glsl and the history copies of SVGF.cpp:107-174 -- not from oracle/ or lv_svgf.hip -- and compared with
the oracle frame after frame on synthetic sequences of the five input maps that take every branch of the temporal half.

The statement (Svgf64) carries the four history images from frame to frame.  Discrete decisions are evaluated in float32, as the
shader evaluates them: the reprojected positions (0.5 + pixel) - flow and (0.01 + pixel) - flow and their truncation, the two threshold
comparisons of is_reprj_valid, sum_w >= 0.001 and the history length.  Every sum and every weight is float64; the fractional parts
that make the bilinear weights are taken in float64 from the float32 position the shader holds.

Where GLSL leaves a result open, the statement follows the build's rules (include/linevis_hip.h, lv_svgf_denoise_buffers):
  * max(a, b) / min(a, b) with a NaN operand return the other operand (np.fmax / np.fmin);
  * `out` parameters the callee did not write: prev_moments = 0 when load_moments_and_history_length fails; color_last_frame keeps
    the colour history at the pixel itself (it then enters the mix with weight 0);
  * texel fetches outside the image return 0 (filter_variance at the border);
  * the moments filter reads temp_accum as the reprojection pass wrote it;
  * a reprojected position that is not finite or lies outside the int range fails the load and is never converted;
  * a non-finite depth_fwidth drops the depth term of compute_weight (max(NaN, 0) = 0, x / inf = 0).

The sequences are built so that float32 and float64 cannot decide differently, and the tests ASSERT that instead of excluding pixels:
every evaluated threshold comparison is off equality by a factor of 2, every sum_w is off 0.001 by a factor of 2, and every fractional
position is at least 1/64 from an integer -- except at exactly zero flow, where the position is pixel + 0.01 (pixel + 0.5): that is how
the weight-under-0.001 case is built (only the tap with weight 0.01 * 0.01 valid), and its truncation is the pixel itself.

alpha_color's floor of 0.01 cannot be reached: the history length is capped at 32 and 1 / 32 > 0.01 (SVGF.glsl:243-245).  The
statement counts it all the same; the tests assert the count stays 0 and that alpha_moments' floor of 0.2 is reached.
"""
import functools

import numpy as np
import pytest

from oracle import lvo

F32 = np.float32
VIEWPORTS = ((37, 27), (53, 39))          # one with fewer than 3 blocks of 16 x 16 a side, one with 4 x 3; neither a multiple of 16
DEFAULT_THRESHOLDS = (0.002, 0.02)        # SVGF.hpp:70-71
THRESHOLD_PAIRS = ((0.01, 0.1), (0.0005, 0.005))
# output, colour history and moments against the float64 statement: the bar of test_independent_restatement.py's first-frame test
# (expf and float32 sums).  Measured maximum over every sequence below, 36-frame runs included: 7.0e-7 (see the docstring of
# test_oracle_matches_the_float64_statement), so the bar holds as it stands.
BAR = 2e-5


# ---------------------------------------------------------------------------------------------- the float64 statement
def _shift(img, dx, dy):
    """img fetched at (x + dx, y + dy): (values with 0 outside the image, inside mask)"""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    inside = np.zeros((h, w), bool)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    if xs0 < xs1 and ys0 < ys1:
        out[ys0:ys1, xs0:xs1] = img[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
        inside[ys0:ys1, xs0:xs1] = True
    return out, inside


def compute_weight(cd, od, phi_depth, cn, on, cc, oc, phi_color):
    """svgf_common.glsl:29-41 on arrays, float64"""
    with np.errstate(all="ignore"):
        weight_n = np.fmax(0.0, (cn * on).sum(axis=-1)) ** 128
        weight_z = np.where(phi_depth == 0, 0.0, np.abs(cd - od) / phi_depth)
        weight_c = np.abs(cc - oc) * 2 / phi_color
        return np.exp(0.0 - np.fmax(weight_c, 0.0) - np.fmax(weight_z, 0.0)) * weight_n


def atrous_pass(color, normal, depth, fwidth, iteration):
    """SVGF.glsl Compute-ATrous: color (H, W, 2) = {colour, variance} -> the same"""
    step = 1 << iteration
    kv = [1.0, 2.0 / 3.0, 1.0 / 6.0]
    vk = [[1.0 / 4.0, 1.0 / 8.0], [1.0 / 8.0, 1.0 / 16.0]]
    fv = np.zeros(depth.shape)
    for yy in (-1, 0, 1):
        for xx in (-1, 0, 1):
            fv = fv + _shift(color[..., 1], xx, yy)[0] * vk[abs(xx)][abs(yy)]
    with np.errstate(all="ignore"):
        phi_color = np.sqrt(np.fmax(0.0, 1e-10 + fv))
    acc = np.full(depth.shape, kv[0] * kv[0])
    sum_c, sum_v = color[..., 0] * acc, color[..., 1] * acc
    for y in range(-2, 3):
        for x in range(-2, 3):
            if x == 0 and y == 0:
                continue
            oc, inside = _shift(color, x * step, y * step)
            on, od = _shift(normal, x * step, y * step)[0], _shift(depth, x * step, y * step)[0]
            with np.errstate(all="ignore"):
                phi_depth = np.abs(fwidth * np.hypot(x, y) * step) + 0.0001
                wgt = compute_weight(depth, od, phi_depth, normal, on, color[..., 0], oc[..., 0], phi_color) * (kv[abs(x)] * kv[abs(y)])
                sum_c = np.where(inside, sum_c + wgt * oc[..., 0], sum_c)
                sum_v = np.where(inside, sum_v + wgt * wgt * oc[..., 1], sum_v)
                acc = np.where(inside, acc + wgt, acc)
    with np.errstate(all="ignore"):
        return np.stack([sum_c / acc, sum_v / (acc * acc)], axis=-1)


def _int_range(v):
    with np.errstate(invalid="ignore"):
        return (v >= F32(-2147483648.0)) & (v < F32(2147483648.0))


def _off_by_2(value, threshold):
    """value is under threshold / 2 or over 2 * threshold (NaN: neither)"""
    with np.errstate(invalid="ignore"):
        return (value < 0.5 * threshold) | (value > 2.0 * threshold)


class Svgf64:
    def __init__(self, w, h, iterations=5, allowed_z_dist=0.002, allowed_normal_dist=0.02):
        self.w, self.h, self.iterations = w, h, iterations
        self.z_dist, self.n_dist = F32(allowed_z_dist), F32(allowed_normal_dist)
        self.color_history = np.zeros((h, w))
        self.moments_history = np.zeros((h, w, 2))
        self.length_history = np.zeros((h, w), F32)
        self.normal_history = np.zeros((h, w, 3), F32)
        self.depth_history = np.zeros((h, w), F32)
        self.counts = {}
        self.conditions = {}
        self.masks = {}

    def _reprj_valid(self, cx, cy, z, normal, evaluated):
        """is_reprj_valid at integer coordinate arrays; records the factor-2 condition of the comparisons it evaluates"""
        w, h = self.w, self.h
        inb = (cx >= 1) & (cy >= 1) & ~(cx > w - 1) & ~(cy > h - 1)
        ccx, ccy = np.clip(cx, 0, w - 1), np.clip(cy, 0, h - 1)
        z_prev, n_prev = self.depth_history[ccy, ccx], self.normal_history[ccy, ccx]
        with np.errstate(invalid="ignore"):
            dz = np.abs(z_prev - z)
            d = n_prev - normal
            dn = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            z_ok, n_ok = ~(dz > self.z_dist), ~(dn > self.n_dist)
        ev = evaluated & inb
        self.conditions["threshold"] &= bool(np.all(_off_by_2(dz, self.z_dist)[ev]))
        self.conditions["threshold"] &= bool(np.all(_off_by_2(dn, self.n_dist)[ev & z_ok]))
        return inb & z_ok & n_ok

    def step(self, noisy, normal, depth, fwidth, flow):
        """one denoise(): float32 maps in, the denoised float64 image out; self.counts = pixels per branch of this frame"""
        w, h = self.w, self.h
        c = noisy.astype(np.float64)
        n32, n64, d64, f64 = normal[..., :3], normal[..., :3].astype(np.float64), depth.astype(np.float64), fwidth.astype(np.float64)
        ys, xs = np.mgrid[0:h, 0:w]
        xf, yf = xs.astype(F32), ys.astype(F32)
        self.conditions = {"threshold": True, "sum_w": True, "fraction": True}
        # ---- Compute-Reproject
        with np.errstate(invalid="ignore"):
            fpx, fpy = (F32(0.5) + xf) - flow[..., 0], (F32(0.5) + yf) - flow[..., 1]
            ppx, ppy = (F32(0.01) + xf) - flow[..., 0], (F32(0.01) + yf) - flow[..., 1]
        assert fpx.dtype == F32 and ppx.dtype == F32
        in_range = _int_range(fpx) & _int_range(fpy) & _int_range(ppx) & _int_range(ppy)   # the build's rule: tested before any conversion
        zero_flow = (flow[..., 0] == 0) & (flow[..., 1] == 0)
        for p in (fpx, fpy, ppx, ppy):
            pp = np.where(in_range, p, F32(0.5)).astype(np.float64)
            self.conditions["fraction"] &= bool(np.all((np.abs(pp - np.rint(pp)) >= 1.0 / 64.0) | zero_flow))
        tr = lambda p: np.trunc(np.where(in_range, p, F32(0))).astype(np.int64)
        ipx, ipy, qx, qy = tr(fpx), tr(fpy), tr(ppx), tr(ppy)
        load = in_range & ~((ipx < 0) | (ipy < 0) | (ipx >= w) | (ipy >= h))              # load_moments_and_history_length
        lx, ly = np.clip(ipx, 0, w - 1), np.clip(ipy, 0, h - 1)
        prev_m = np.where(load[..., None], self.moments_history[ly, lx], 0.0)             # unwritten `out`: 0
        hist_len = np.where(load, self.length_history[ly, lx], F32(0))
        color_last = self.color_history.copy()
        # try_2x2_tap
        offsets = ((0, 0), (0, 1), (1, 0), (1, 1))
        valids = [self._reprj_valid(qx + ox, qy + oy, depth, n32, load) for ox, oy in offsets]
        any_valid = valids[0] | valids[1] | valids[2] | valids[3]
        pp64x, pp64y = np.where(in_range, ppx, F32(0)).astype(np.float64), np.where(in_range, ppy, F32(0)).astype(np.float64)
        x, y = pp64x - np.floor(pp64x), pp64y - np.floor(pp64y)                            # fract()
        wts = ((1 - x) * (1 - y), x * (1 - y), (1 - x) * y, x * y)
        sum_w, cb, mb = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 2))
        for (ox, oy), v, wt in zip(offsets, valids, wts):
            tx, ty = np.clip(qx + ox, 0, w - 1), np.clip(qy + oy, 0, h - 1)
            wt = np.where(v, wt, 0.0)
            mb += wt[..., None] * self.moments_history[ty, tx]
            cb += wt * self.color_history[ty, tx]
            sum_w += wt
        tried2 = load & any_valid
        self.conditions["sum_w"] &= bool(np.all(_off_by_2(sum_w, 0.001)[tried2]))
        ok2 = tried2 & (sum_w.astype(F32) >= F32(0.001))
        with np.errstate(all="ignore"):
            color_last = np.where(ok2, cb / sum_w, color_last)
            prev_m = np.where(ok2[..., None], mb / sum_w[..., None], prev_m)
        # try_3x3_bilat
        need3 = load & ~ok2
        n_valid, fc, fm = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 2))
        at_last = np.zeros((h, w), bool)
        for yy in (-1, 0, 1):
            for xx in (-1, 0, 1):
                ox, oy = qx + xx, qy + yy
                skip = (ox < 1) | (oy < 1) | (ox >= w) | (oy >= h)
                v = need3 & ~skip & self._reprj_valid(ox, oy, depth, n32, need3 & ~skip)
                tx, ty = np.clip(ox, 0, w - 1), np.clip(oy, 0, h - 1)
                fc += np.where(v, self.color_history[ty, tx], 0.0)
                fm += np.where(v[..., None], self.moments_history[ty, tx], 0.0)
                n_valid += v
                at_last |= v & ((ox == w - 1) | (oy == h - 1))
        ok3 = need3 & (n_valid > 0)
        with np.errstate(all="ignore"):
            color_last = np.where(ok3, fc / n_valid, color_last)
            prev_m = np.where(ok3[..., None], fm / n_valid[..., None], prev_m)
        success = ok2 | ok3
        new_len = np.fmin(np.where(success, hist_len + F32(1), F32(1)), F32(32)).astype(F32)
        with np.errstate(all="ignore"):
            alpha_color = np.where(success, np.fmax(0.01, 1.0 / new_len.astype(np.float64)), 1.0)
            alpha_moments = np.where(success, np.fmax(0.2, 1.0 / new_len.astype(np.float64)), 1.0)
            cur_m = np.stack([c, c * c], axis=-1)
            moments = prev_m * (1.0 - alpha_moments[..., None]) + cur_m * alpha_moments[..., None]     # mix()
            variance = np.fmax(0.0, moments[..., 1] - moments[..., 0] * moments[..., 0])
            temp = np.stack([color_last * (1.0 - alpha_color) + c * alpha_color, variance], axis=-1)
        # ---- Compute-Filter-Moments (history length < 4; every read sees what the reprojection pass wrote)
        sw, sc, sm = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 2))
        with np.errstate(all="ignore"):
            phi_depth = np.abs(f64) + 0.0001
        for yy in range(-3, 4):
            for xx in range(-3, 4):
                oc, inside = _shift(temp[..., 0], xx, yy)
                wgt = compute_weight(d64, _shift(d64, xx, yy)[0], phi_depth, n64, _shift(n64, xx, yy)[0], temp[..., 0], oc, 10.0)
                with np.errstate(all="ignore"):
                    sw = np.where(inside, sw + wgt, sw)
                    sc = np.where(inside, sc + wgt * oc, sc)
                    sm = np.where(inside[..., None], sm + wgt[..., None] * _shift(moments, xx, yy)[0], sm)
        with np.errstate(all="ignore"):
            sw = np.fmax(sw, 1e-6)
            sm = sm / sw[..., None]
            spatial = np.stack([sc / sw, (sm[..., 1] - sm[..., 0] * sm[..., 0]) * (4.0 / new_len.astype(np.float64))], axis=-1)
        young = ~(new_len >= F32(4))
        filtered = np.where(young[..., None], spatial, temp)
        # ---- Compute-ATrous x iterations; with none, temp_accum is blitted to the output and the colour history (SVGF.cpp:347-360)
        img = filtered
        if self.iterations < 1:
            self.color_history = filtered[..., 0].copy()
        for it in range(self.iterations):
            img = atrous_pass(img, n64, d64, f64, it)
            if it == 0:
                self.color_history = img[..., 0].copy()
        # ---- "update previous frame images", SVGF.cpp:112-173
        self.normal_history, self.depth_history = n32.copy(), depth.copy()
        self.moments_history, self.length_history = moments, new_len
        self.masks = {"load": load, "success": success}
        not_in_range = ~in_range
        with np.errstate(invalid="ignore"):
            fl = flow
            self.counts = {
                "load_failed": int((~load).sum()),
                "left": int((in_range & (ipx < 0)).sum()), "right": int((in_range & (ipx >= w)).sum()),
                "top": int((in_range & (ipy < 0)).sum()), "bottom": int((in_range & (ipy >= h)).sum()),
                "flow_1e4": int((in_range & ((np.abs(fl) > F32(9e3)) & (np.abs(fl) < F32(2e4))).any(axis=-1)).sum()),
                "flow_3e9": int((not_in_range & (np.abs(fl) == F32(3e9)).any(axis=-1)).sum()),
                "flow_inf": int((not_in_range & np.isinf(fl).any(axis=-1)).sum()),
                "flow_nan": int((not_in_range & np.isnan(fl).any(axis=-1)).sum()),
                "taps_4": int((ok2 & valids[0] & valids[1] & valids[2] & valids[3]).sum()),
                "taps_4_fractional": int((ok2 & ~zero_flow & valids[0] & valids[1] & valids[2] & valids[3]).sum()),
                "taps_1_to_3": int((ok2 & ~(valids[0] & valids[1] & valids[2] & valids[3])).sum()),
                "sum_w_low": int((tried2 & ~ok2).sum()),
                "sum_w_low_one_tap": int((tried2 & ~ok2 & (sum(v.astype(int) for v in valids) == 1)).sum()),
                "fallback_3x3": int(ok3.sum()),
                "fallback_at_last_column_or_row": int((ok3 & at_last).sum()),
                "nothing_valid": int((load & ~success).sum()),
                "coordinate_0": int((load & ((qx == 0) | (qy == 0))).sum()),
                "truncated_up_to_0": int((load & ((fpx < 0) | (fpy < 0))).sum()),
                "tap_at_last_column": int((ok2 & ((valids[2] | valids[3]) & (qx + 1 == w - 1) | (valids[0] | valids[1]) & (qx == w - 1))).sum()),
                "tap_at_last_row": int((ok2 & ((valids[1] | valids[3]) & (qy + 1 == h - 1) | (valids[0] | valids[2]) & (qy == h - 1))).sum()),
                "length_capped": int((success & (hist_len + F32(1) > F32(32))).sum()),
                "alpha_moments_floor": int((success & (1.0 / new_len.astype(np.float64) < 0.2)).sum()),
                "alpha_color_floor": int((success & (1.0 / new_len.astype(np.float64) < 0.01)).sum()),
                "temporal_variance": int((~young).sum()),
                "spatial_variance": int(young.sum()),
                "fwidth_0": int((fwidth == 0).sum()), "fwidth_inf": int(np.isinf(fwidth).sum()), "fwidth_nan": int(np.isnan(fwidth).sum()),
            }
        return img[..., 0]


# ---------------------------------------------------------------------------------------------- synthetic sequences
def _normals(rng, base, amp):
    n = np.asarray(base, np.float64) + rng.uniform(-amp, amp, base.shape)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    out = np.zeros(base.shape[:2] + (4,), F32)
    out[..., :3] = n.astype(F32)
    return out


def _banded_scene(rng, w, h, zt, nt):
    """depth steps of 3 * zt every 7 columns, two normals 3 * nt apart alternating every 6 rows; noise zt / 8 and nt / 8: differences
    stay under half a threshold within a band and over twice the threshold across a step, and a step is small enough for another
    pair of thresholds to accept it"""
    ys, xs = np.mgrid[0:h, 0:w]
    depth = (0.7 + 3.0 * zt * (xs // 7) + rng.uniform(-zt / 8, zt / 8, (h, w))).astype(F32)
    tilt = np.where((ys // 6) % 2 == 0, 0.0, 3.0 * nt)
    base = np.stack([np.sin(tilt), np.zeros((h, w)), np.cos(tilt)], axis=-1)
    return _normals(rng, base, nt / 8), depth


def _checker_scene(rng, w, h, zt, nt, shift=0, offset=0.0):
    """four depth levels so that every 2 x 2 block holds all four; `shift` moves the pattern by (-shift, -shift) pixels"""
    ys, xs = np.mgrid[0:h, 0:w]
    level = ((xs + shift) % 2) + 2 * ((ys + shift) % 2)
    depth = (1.9 + offset + 3.0 * zt * level + rng.uniform(-zt / 8, zt / 8, (h, w))).astype(F32)
    base = np.zeros((h, w, 3))
    base[..., 1] = 1.0
    return _normals(rng, base, nt / 8), depth


def _frame(rng, w, h, scene, flow=(0.0, 0.0), special_fwidth=False):
    normal, depth = scene
    f = np.zeros((h, w, 2), F32)
    f[..., 0], f[..., 1] = flow
    fwidth = rng.uniform(0.0, 0.3, (h, w)).astype(F32)
    if special_fwidth:
        fwidth[3, 2:6] = 0.0
        fwidth[h // 2, 5:9] = np.inf
        fwidth[h - 4, w - 9:w - 5] = np.nan
        fwidth[h // 2 + 1, 7] = -np.inf
    noisy = rng.uniform(0.2, 1.0, (h, w)).astype(F32)
    noisy[:, w // 2:] *= F32(0.5)
    return dict(noisy=noisy, normal=normal, depth=depth, fwidth=fwidth, flow=f)


# +-1e4 carries a fraction: float32 holds 0.001 steps there, and pixel + 0.01 - 1e4 would sit 0.01 from an integer
SPECIAL_FLOWS = (1e4 + 0.37, -1e4 - 0.37, 3e9, -3e9, np.inf, -np.inf, np.nan)


def _with_special_flows(frame, component):
    """rows 2, 5, 8, ... carry one special value each in one flow component, the other component keeps a fractional flow"""
    fl = frame["flow"]
    for k, v in enumerate(SPECIAL_FLOWS):
        fl[2 + 3 * k, :, component] = F32(v)
    return frame


def sequence(name, w, h, thresholds=DEFAULT_THRESHOLDS):
    """(iterations, frames): every frame a dict of the five float32 maps"""
    zt, nt = thresholds
    rng = np.random.default_rng([w, h, sum(map(ord, name))])
    if name == "static":        # zero flow for more than 32 frames: the cap of 32, alpha_moments' floor, the temporal variance
        scene = _banded_scene(rng, w, h, zt, nt)
        return 1, [_frame(rng, w, h, scene, special_fwidth=(k % 5 == 1)) for k in range(36)]
    banded = _banded_scene(rng, w, h, zt, nt)
    if name == "flows":         # fractional flows on a scene with depth and normal steps; leaves the picture on all four sides
        flows = [(0, 0), (0, 0), (2.37, -1.6), (-2.37, 1.6), (5.37, 4.6), (-5.37, -4.6), (0.37, 0.6), (0, 0), (-0.63, -0.4), (0, 0)]
        return 5, [_frame(rng, w, h, banded, fl, special_fwidth=(k == 3)) for k, fl in enumerate(flows)]
    if name == "special":       # flows of +-1e4, +-3e9, +-inf and NaN in either component
        frames = [_frame(rng, w, h, banded), _frame(rng, w, h, banded, (0.37, 0.6))]
        frames.append(_with_special_flows(_frame(rng, w, h, banded, (0.37, 0.6), special_fwidth=True), 0))
        frames.append(_with_special_flows(_frame(rng, w, h, banded, (-0.63, 0.6)), 1))
        frames.append(_frame(rng, w, h, banded))
        return 3, frames
    if name.startswith("fallback"):   # only the tap of weight 0.01 * 0.01 valid -> 3 x 3 fallback; then nothing valid at all
        its = int(name[-1])
        frames = [_frame(rng, w, h, banded), _frame(rng, w, h, banded)]
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 0)))                  # nothing of the banded history fits
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 0)))
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 1), special_fwidth=True))   # the pattern moved by (-1, -1)
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 1), (0.37, 0.6)))
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 1, offset=100.0 * zt)))      # history length back to 1
        frames.append(_frame(rng, w, h, _checker_scene(rng, w, h, zt, nt, 1, offset=100.0 * zt)))
        return its, frames
    raise KeyError(name)


# (sequence name, viewport index, thresholds): a-trous iterations 0 ... 5 are spread over them
CASES = [("static", 0, DEFAULT_THRESHOLDS), ("static", 1, DEFAULT_THRESHOLDS),
         ("flows", 0, DEFAULT_THRESHOLDS), ("flows", 1, THRESHOLD_PAIRS[0]),
         ("special", 0, THRESHOLD_PAIRS[1]), ("special", 1, DEFAULT_THRESHOLDS),
         ("fallback0", 0, DEFAULT_THRESHOLDS), ("fallback2", 1, THRESHOLD_PAIRS[1]), ("fallback4", 0, THRESHOLD_PAIRS[0]),
         ("fallback5", 1, DEFAULT_THRESHOLDS)]
CASE_IDS = ["%s-%dx%d-z%g" % (n, VIEWPORTS[v][0], VIEWPORTS[v][1], t[0]) for n, v, t in CASES]


def oracle_histories(w, h):
    return [np.zeros((h, w), F32), np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32), np.zeros((h, w), F32)]


def oracle_step(w, h, fr, its, thresholds, hist):
    """lvo_svgf_denoise on one frame; hist = [colour, moments + length, normal, depth], updated in place"""
    out = np.zeros((h, w), F32)
    lvo.lib().lvo_svgf_denoise(w, h, lvo._p(fr["noisy"]), lvo._p(fr["normal"]), lvo._p(fr["depth"]), lvo._p(fr["fwidth"]),
                               lvo._p(fr["flow"]), its, float(thresholds[0]), float(thresholds[1]), lvo._p(hist[0]), lvo._p(hist[1]),
                               lvo._p(hist[2]), lvo._p(hist[3]), lvo._p(out))
    return out


@functools.lru_cache(maxsize=None)
def run_statement(name, vp, thresholds):
    """per frame: (output, colour history, moments, history length, counts, conditions) of the float64 statement"""
    w, h = VIEWPORTS[vp]
    its, frames = sequence(name, w, h, thresholds)
    st = Svgf64(w, h, its, *thresholds)
    res = []
    for fr in frames:
        out = st.step(fr["noisy"], fr["normal"], fr["depth"], fr["fwidth"], fr["flow"])
        res.append(dict(out=out, color=st.color_history.copy(), moments=st.moments_history.copy(), length=st.length_history.copy(),
                        counts=dict(st.counts), conditions=dict(st.conditions)))
    return res


@functools.lru_cache(maxsize=None)
def run_oracle(name, vp, thresholds):
    """per frame: copies of (output, colour history, moments + length, normal history, depth history) of the oracle"""
    w, h = VIEWPORTS[vp]
    its, frames = sequence(name, w, h, thresholds)
    hist = oracle_histories(w, h)
    res = []
    for fr in frames:
        out = oracle_step(w, h, fr, its, thresholds, hist)
        res.append(dict(out=out, color=hist[0].copy(), moments=hist[1].copy(), normal=hist[2].copy(), depth=hist[3].copy()))
    return res


def deviation(got_out, got_color, got_moments, want):
    """largest difference of output, colour history and the two moments from the statement's frame (NaN counts as inf)"""
    d = max(np.abs(got_out - want["out"]).max(), np.abs(got_color - want["color"]).max(),
            np.abs(got_moments[..., :2] - want["moments"]).max())
    return float("inf") if np.isnan(d) else float(d)


# ---------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name,vp,thresholds", CASES, ids=CASE_IDS)
def test_oracle_matches_the_float64_statement(name, vp, thresholds):
    """History length, normal and depth history exact; output, colour history and moments under BAR = 2e-5 after every frame, no
    pixel excluded: the conditions under which float32 and float64 decide alike are asserted.  Measured maxima over all frames:
    static 5.5e-7 (37 x 27) and 5.9e-7 (53 x 39), flows 5.5e-7 / 5.9e-7, special 3.9e-7 / 4.7e-7, fallback 4.2e-7 ... 7.0e-7."""
    w, h = VIEWPORTS[vp]
    _, frames = sequence(name, w, h, thresholds)
    worst = 0.0
    for k, (fr, want, got) in enumerate(zip(frames, run_statement(name, vp, thresholds), run_oracle(name, vp, thresholds))):
        assert all(want["conditions"].values()), "frame %d: %s" % (k, want["conditions"])
        assert np.array_equal(got["moments"][..., 2], want["length"]), "frame %d: history length" % k
        assert np.array_equal(got["normal"].view(np.uint32), fr["normal"].view(np.uint32)), "frame %d" % k
        assert np.array_equal(got["depth"].view(np.uint32), fr["depth"].view(np.uint32)), "frame %d" % k
        assert np.all(got["moments"][..., 3] == 0)
        d = deviation(got["out"], got["color"], got["moments"], want)
        worst = max(worst, d)
        assert d < BAR, "frame %d: %.3g" % (k, d)
    print("%s %dx%d: largest deviation %.3g" % (name, w, h, worst))


# branch -> the cases (indices into CASES) one of which must hold it on at least 20 pixels of some frame
REQUIRED = {
    "length_capped": (0, 1), "alpha_moments_floor": (0, 1), "temporal_variance": (0, 1), "spatial_variance": (0, 1),
    "taps_4_fractional": (2, 3), "taps_1_to_3": (2, 3), "left": (2, 3), "right": (2, 3), "top": (2, 3), "bottom": (2, 3),
    "coordinate_0": (2, 3), "truncated_up_to_0": (2, 3), "tap_at_last_column": (2, 3), "tap_at_last_row": (2, 3),
    "flow_1e4": (4, 5), "flow_3e9": (4, 5), "flow_inf": (4, 5), "flow_nan": (4, 5),
    "sum_w_low_one_tap": (6, 7, 8, 9), "fallback_3x3": (6, 7, 8, 9), "fallback_at_last_column_or_row": (6, 7, 8, 9),
    "nothing_valid": (6, 7, 8, 9), "load_failed": (2, 3),
}


@pytest.mark.parametrize("branch", sorted(REQUIRED))
def test_every_branch_holds_20_pixels_in_every_case_meant_for_it(branch):
    for i in REQUIRED[branch]:
        best = max(fr["counts"][branch] for fr in run_statement(*CASES[i]))
        assert best >= 20, "%s: at most %d pixels in %s" % (branch, best, CASE_IDS[i])


def test_lengths_alpha_floors_and_special_depth_fwidths():
    for i in (0, 1):
        res = run_statement(*CASES[i])
        w, h = VIEWPORTS[CASES[i][1]]
        # every pixel keeps a history (row and column 0 through the taps at coordinate 1): the length counts up to the cap
        for k, fr in enumerate(res):
            assert np.all(fr["length"] == min(k + 1, 32))
        assert res[-1]["counts"]["length_capped"] == w * h
        assert all(fr["counts"]["alpha_color_floor"] == 0 for fr in res)     # 1 / 32 > 0.01: unreachable
    seen = {k: 0 for k in ("fwidth_0", "fwidth_inf", "fwidth_nan")}
    for case in CASES:
        for fr in run_statement(*case):
            for k in seen:
                seen[k] = max(seen[k], fr["counts"][k])
        assert all(np.isfinite(fr["out"]).all() for fr in run_statement(*case))
    assert min(seen.values()) >= 4, seen
    assert sorted({sequence(c[0], *VIEWPORTS[c[1]], c[2])[0] for c in CASES}) == [0, 1, 2, 3, 4, 5]


def test_thresholds_decide():
    """The same maps under the default thresholds give another image: the non-default pairs are not idle."""
    for i in (3, 4, 7, 8):
        name, vp, thresholds = CASES[i]
        w, h = VIEWPORTS[vp]
        its, frames = sequence(name, w, h, thresholds)
        hist = oracle_histories(w, h)
        outs = [oracle_step(w, h, fr, its, DEFAULT_THRESHOLDS, hist) for fr in frames]
        assert max(np.abs(o - r["out"]).max() for o, r in zip(outs, run_oracle(name, vp, thresholds))) > 1e-3


def test_vectorised_passes_equal_the_scalar_statement():
    """atrous_pass / compute_weight above are the numpy-shift form of test_independent_restatement.py's scalar loops."""
    from test_independent_restatement import svgf_atrous_pass, svgf_compute_weight
    rng = np.random.default_rng(5)
    h, w = 11, 13
    normal = _normals(rng, np.tile(np.array([0.0, 0.0, 1.0]), (h, w, 1)), 0.1)[..., :3].astype(np.float64)
    depth = 0.7 + 0.001 * rng.standard_normal((h, w))
    fwidth = rng.uniform(0.0, 0.3, (h, w))
    fwidth[2, 3] = 0.0
    color = np.stack([rng.uniform(0.2, 1.0, (h, w)), rng.uniform(0.0, 0.05, (h, w))], axis=-1)
    for it in (0, 1, 2):
        assert np.abs(atrous_pass(color, normal, depth, fwidth, it) - svgf_atrous_pass(color, normal, depth, fwidth, it)).max() < 1e-13
    a = compute_weight(np.array([0.7]), np.array([0.71]), np.array([0.02]), normal[1:2, 1], normal[2:3, 2], np.array([0.4]), np.array([0.6]),
                       np.array([0.3]))
    assert abs(a[0] - svgf_compute_weight(0.7, 0.71, 0.02, normal[1, 1], normal[2, 2], 0.4, 0.6, 0.3)) < 1e-15


# ---------------------------------------------------------------------------------------------- the SVGF feature maps
# VulkanRayTracedAmbientOcclusion.glsl:413-464 (WRITE_FLOW_MAP, WRITE_DEPTH_FWIDTH_MAP) and :365-385 (depth), restated in float64 from
# the hit's position and world normal.  The hit itself is the oracle's: its view-space position map (float32) is taken back to world
# space with the float64 inverse of the view matrix.
FLOW_BAR = 2.8e-5      # 4 x 6.9e-6 px, the largest difference measured here between the oracle's float32 flow and the float64 value
                       # (72 x 48; the margin is for the float32 products lastFrameViewProjection = projection * view and its
                       # application, whose rounding grows with the pixel coordinate)


def _mat(m):
    """column-major flat float32 -> float64 (4, 4) indexed [row, col]"""
    return np.asarray(m, np.float64).reshape(4, 4).T


@pytest.mark.parametrize("name,moved", [("roll37", dict(eye=(0.36, 0.17, 0.66))), ("lens_shift", dict(eye=(0.07, -0.04, 0.74)))])
def test_feature_maps_against_the_float64_statement(name, moved):
    """Flow, depth and depth fwidth of the second of two frames under a rolled and under a lens-shifted camera of tests/cameras.py,
    the eye moved between the frames.  Depth: exact (-z of the float32 view-space position; farDistance on a miss).  Flow: under
    FLOW_BAR; measured maxima 6.9e-6 px (roll37) and 6.7e-6 px (lens_shift).  Depth fwidth = |A / sqrt(1 - A^2)| + |B / sqrt(1 - B^2)|,
    A, B = x, y of the view-space normal: the float32 normal carries about 8 eps = 4.8e-7 of rounding (input, three products, two sums),
    which the cotangent magnifies by (1 - A^2)^-1.5; that is the tolerance, plus 1e-6 relative.  Pixels with 1 - A^2 or 1 - B^2
    under 1e-4 (a normal along a camera axis; the value passes 100) are counted, not compared, and must stay under 1 %."""
    import cameras
    from common import small_case
    from test_svgf import RTAO
    w, h = 72, 48
    c = small_case(width=w, height=h, n_lines=6, pts_per_line=30, line_width=0.25, **dict(RTAO, use_jittered_primary_rays=True))
    sc = c.oracle_scene()
    sv = lvo.Svgf(w, h)
    cam0 = cameras.get(name)
    cam1 = dict(cam0, **moved)
    feats = lvo.ao_features(w, h)
    mats = []
    for cam in (cam0, cam1):
        cameras.apply_camera(c, cam)
        P = c.oracle_params(sc)
        mats.append((_mat(c.view), _mat(c.proj)))

        def render():
            with feats:
                return sc.render_ao(P)
        sv.step(render, P)
    (view0, proj0), (view1, proj1) = mats
    hit = sv.depth < np.float32(c.far)
    assert 500 < hit.sum() < w * h - 500
    pos_view = feats.position[..., :3].astype(np.float64)
    assert np.array_equal(sv.depth[hit], -feats.position[..., 2][hit]) and np.all(sv.depth[~hit] == np.float32(c.far))
    world = (np.concatenate([pos_view, np.ones((h, w, 1))], axis=-1) @ np.linalg.inv(view1).T)
    ndc = world @ (proj0 @ view0).T                                            # lastFrameViewProjectionMatrix * vec4(position, 1)
    ndc = ndc[..., :3] / ndc[..., 3:4]
    ys, xs = np.mgrid[0:h, 0:w]
    last = (0.5 * ndc[..., :2] + 0.5) * np.array([w, h]) - 0.5
    flow = np.stack([xs, ys], axis=-1) - last
    flow[~hit] = 0.0
    d = np.abs(sv.flow - flow).max()
    print("%s: largest flow %.2f px, largest difference %.3g px" % (name, np.abs(flow).max(), d))
    assert np.abs(flow[hit]).max() > 3.0 and d < FLOW_BAR
    # camNormal = (transpose(inverse(view)) * vec4(normal, 0)).xyz
    cam_normal = sv.normal[..., :3].astype(np.float64) @ np.linalg.inv(view1)[:3, :3]
    a2, b2 = 1.0 - cam_normal[..., 0] ** 2, 1.0 - cam_normal[..., 1] ** 2
    with np.errstate(all="ignore"):
        fwidth = np.abs(cam_normal[..., 0] / np.sqrt(a2)) + np.abs(cam_normal[..., 1] / np.sqrt(b2))
    fwidth[~hit] = 0.0
    near_axis = hit & ((a2 < 1e-4) | (b2 < 1e-4))
    assert near_axis.sum() < 0.01 * hit.sum()
    ok = hit & ~near_axis
    tol = 4.8e-7 * (a2[ok] ** -1.5 + b2[ok] ** -1.5) + 1e-6 * fwidth[ok]
    assert np.all(np.abs(sv.fwidth[ok] - fwidth[ok]) <= tol) and np.all(sv.fwidth[~hit] == 0)
    assert fwidth[ok].max() > 2.0 and fwidth[ok].min() < 0.5
