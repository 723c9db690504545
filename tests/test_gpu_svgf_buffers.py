"""lv_svgf_denoise_buffers: k_svgf_reproject, k_svgf_filter_moments and k_svgf_atrous (linevis_amd/csrc/lv_svgf.hip) on given buffers.
Every synthetic sequence of test_svgf_restatement.py goes through the entry point, frame after frame with the history images the
device wrote back, and is compared with both references: the oracle (discrete images exact, the rest under 3e-5, the bar of
test_svgf.py) and the float64 statement (its bar of 2e-5 plus 3e-5).  The sequences take every branch of the temporal half --
test_svgf_restatement.py asserts the pixel counts -- including flows of +-1e4, +-3e9, +-inf and NaN and non-finite depth fwidths."""
import numpy as np
import pytest

import test_svgf_restatement as rs
from linevis_amd import capi
from test_svgf import fat_case

F32 = np.float32
ORACLE_BAR = 3e-5
E_INVALID = -1


def device_images(fr):
    """the entry point's layout of a frame: normal + depth, flow + depth fwidth"""
    h, w = fr["depth"].shape
    nd, ff = np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32)
    nd[..., :3], nd[..., 3] = fr["normal"][..., :3], fr["depth"]
    ff[..., :2], ff[..., 2] = fr["flow"], fr["fwidth"]
    return nd, ff


def device_histories(w, h):
    return [np.zeros((h, w), F32), np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32)]


def device_run(ctx, name, vp, thresholds):
    """per frame (output, colour history, moments + length, normal + depth history) of the device"""
    w, h = rs.VIEWPORTS[vp]
    its, frames = rs.sequence(name, w, h, thresholds)
    ctx.set_option("svgf_denoiser_iterations", its)
    ctx.set_option("svgf_denoiser_allowed_z_dist", thresholds[0])
    ctx.set_option("svgf_denoiser_allowed_normal_dist", thresholds[1])
    hist = device_histories(w, h)
    res = []
    for fr in frames:
        nd, ff = device_images(fr)
        out = ctx.svgf_denoise(fr["noisy"], nd, ff, hist[0], hist[1], hist[2])
        res.append((out, hist[0].copy(), hist[1].copy(), hist[2].copy()))
    return frames, res


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,vp,thresholds", rs.CASES, ids=rs.CASE_IDS)
def test_sequence_matches_the_oracle_and_the_float64_statement(ctx, name, vp, thresholds):
    frames, res = device_run(ctx, name, vp, thresholds)
    worst_o = worst_s = 0.0
    for k, (fr, (out, color, moments, ndh), ora, want) in enumerate(zip(frames, res, rs.run_oracle(name, vp, thresholds),
                                                                        rs.run_statement(name, vp, thresholds))):
        assert np.array_equal(moments[..., 2], ora["moments"][..., 2]) and np.array_equal(moments[..., 2], want["length"]), "frame %d" % k
        assert np.all(moments[..., 3] == 0)
        assert np.array_equal(ndh[..., :3].view(np.uint32), fr["normal"][..., :3].view(np.uint32)), "frame %d" % k
        assert np.array_equal(ndh[..., 3].view(np.uint32), fr["depth"].view(np.uint32)), "frame %d" % k
        d_o = rs.deviation(out, color, moments, dict(out=ora["out"], color=ora["color"], moments=ora["moments"][..., :2]))
        d_s = rs.deviation(out, color, moments, want)
        worst_o, worst_s = max(worst_o, d_o), max(worst_s, d_s)
        assert d_o < ORACLE_BAR, "frame %d against the oracle: %.3g" % (k, d_o)
        assert d_s < rs.BAR + ORACLE_BAR, "frame %d against the float64 statement: %.3g" % (k, d_s)
    print("%s: largest deviation from the oracle %.3g, from the statement %.3g" % (name, worst_o, worst_s))


@pytest.mark.gpu
@pytest.mark.parametrize("case", (3, 4, 8))
def test_each_threshold_reaches_the_kernel(ctx, case):
    """The cases with non-default thresholds match above; here either threshold alone, put back to its default on the same maps,
    changes the image and still matches the oracle run with that pair -- an option that is not forwarded would pass neither."""
    name, vp, thresholds = rs.CASES[case]
    w, h = rs.VIEWPORTS[vp]
    its, frames = rs.sequence(name, w, h, thresholds)
    base = rs.run_oracle(name, vp, thresholds)
    for pair in ((rs.DEFAULT_THRESHOLDS[0], thresholds[1]), (thresholds[0], rs.DEFAULT_THRESHOLDS[1])):
        ctx.set_option("svgf_denoiser_iterations", its)
        ctx.set_option("svgf_denoiser_allowed_z_dist", pair[0])
        ctx.set_option("svgf_denoiser_allowed_normal_dist", pair[1])
        hist, ohist = device_histories(w, h), rs.oracle_histories(w, h)
        changed = 0.0
        for k, fr in enumerate(frames):
            nd, ff = device_images(fr)
            out = ctx.svgf_denoise(fr["noisy"], nd, ff, hist[0], hist[1], hist[2])
            ref = rs.oracle_step(w, h, fr, its, pair, ohist)
            assert np.array_equal(hist[1][..., 2], ohist[1][..., 2]), "frame %d" % k
            assert np.abs(out - ref).max() < ORACLE_BAR and np.abs(hist[0] - ohist[0]).max() < ORACLE_BAR, "frame %d" % k
            changed = max(changed, float(np.abs(out - base[k]["out"]).max()))
        assert changed > 1e-3, pair


@pytest.mark.gpu
def test_entry_point_calls_leave_a_rendered_sequence_alone(ctx):
    """A rendered SVGF sequence with entry-point calls between its frames equals the sequence without them, byte for byte."""
    c = fat_case(jitter=True)
    c.width, c.height = 96, 72
    from linevis_amd import camera
    name, vp, thresholds = rs.CASES[2]
    w, h = rs.VIEWPORTS[vp]
    _, frames = rs.sequence(name, w, h, thresholds)
    runs = []
    for interleave in (False, True):
        r = c.hip_context()
        hist = device_histories(w, h)
        imgs = []
        for k, pos in enumerate([(0.0, 0.0, 0.8), (0.03, 0.0, 0.8), (0.06, 0.01, 0.79), (0.06, 0.01, 0.79)]):
            c.view, c.proj, c.fovy, c.near, c.far = camera.default_camera(c.width, c.height, pos)
            r.set_camera(c.view, c.proj, c.fovy, c.near, c.far, c.width, c.height)
            imgs.append((r.render(11), r.get_ao()))
            if interleave:
                nd, ff = device_images(frames[k + 1])
                r.svgf_denoise(frames[k + 1]["noisy"], nd, ff, hist[0], hist[1], hist[2])
        runs.append(imgs)
        r.close()
    for (img_a, ao_a), (img_b, ao_b) in zip(*runs):
        assert np.array_equal(img_a, img_b) and np.array_equal(ao_a.view(np.uint32), ao_b.view(np.uint32))
    assert not np.array_equal(runs[0][0][1], runs[0][3][1])


@pytest.mark.gpu
def test_bad_arguments_are_lv_e_invalid(ctx):
    w, h = 8, 6
    z = lambda *s: np.zeros((h, w) + s, F32)
    p = capi._p
    args = lambda: [p(z()), p(z(4)), p(z(4)), p(z()), p(z(4)), p(z(4)), p(z())]
    L = ctx.L
    assert L.lv_svgf_denoise_buffers(ctx.h, w, h, *args()) == 0
    for bad_w, bad_h in ((0, h), (w, 0), (16385, 1), (1, 16385), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert L.lv_svgf_denoise_buffers(ctx.h, bad_w, bad_h, *args()) == E_INVALID, (bad_w, bad_h)
        assert L.lv_last_error(ctx.h)
    for i in range(7):
        a = args()
        a[i] = None
        assert L.lv_svgf_denoise_buffers(ctx.h, w, h, *a) == E_INVALID, i
    assert L.lv_svgf_denoise_buffers(None, w, h, *args()) == E_INVALID
    assert L.lv_svgf_denoise_buffers(ctx.h, w, h, *args()) == 0
