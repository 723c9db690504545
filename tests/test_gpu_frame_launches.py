"""What a frame of every rendering mode records, pinned: the launches per LV_KERNEL_* slot (lv_get_kernel_times), the phase marks
behind the ms_* fields of lv_get_stats, and that kernel_timers = none changes neither image nor counters.  The numbers are the host
code's, not the device's: a frame function that drops an event record, records one twice or runs its front end once more than it
has to shows here and in no image.

The cases run with RTAO (one iteration, four samples) and depth cues, so that a kernel runs between every two phase marks and each
phase's time is positive by construction; the phases of a frame then add up to ms_total, which holds only when all six marks were
recorded by this frame, in order.  The two frames with a regrowing pool run without RTAO instead (its any-hit traversal tests a
slightly different number of primitives from run to run): their ms_ao may be zero, and prims_tested, which the regrown frame
restores before its second front end, is compared too.  Each case is rendered over the whole viewport and over every other 16 x 16 tile (the requested
pixels marked and the segments culled inside the raster slot), twice each: the second frame is the steady state, which differs from
the first only where a fragment pool regrows."""
import numpy as np
import pytest

from common import small_case
from linevis_amd import capi
from test_gpu_mlab import _stacked_case

pytestmark = pytest.mark.gpu

W, H, TILE = 96, 64, 16
BASE = dict(depth_cue_strength=0.7, collect_stats=True)
RTAO = dict(ambient_occlusion_mode="RTAO (Screen Space)", ambient_occlusion_strength=1.0, ambient_occlusion_iterations=1,
            ambient_occlusion_samples_per_frame=4)
TILES = np.array([(x, y) for y in range(0, H, TILE) for x in range(0, W, TILE) if (x // TILE + y // TILE) % 2 == 0], dtype=np.uint32)
PEEL_LAYERS = 4

PHASES_RT = {"ms_total", "ms_depth_range", "ms_ao", "ms_color"}
PHASES_OIT = {"ms_total", "ms_depth_range", "ms_ao", "ms_ppll_clear", "ms_ppll_gather", "ms_ppll_resolve"}
FRAME_FIELDS = PHASES_RT | PHASES_OIT
BUILD_FIELDS = {"ms_accel_build"}   # recorded once, by the first frame's acceleration-structure build; kept by lv_get_stats
COUNTERS = ("rays_traced", "hits_shaded", "fragments", "max_depth_complexity", "ppll_pool_nodes", "ao_rays_traced", "ao_hit_pixels")

AO = {"k_ao_primary": 1, "k_ao_rays": 1}


def _oit(raster=0, shade=0, gather=0, resolve=1, ao=AO):
    return dict(ao, k_ppll_raster_prism=raster, k_ppll_shade_prism=shade, k_ppll_gather=gather, k_ppll_resolve=resolve)


def _plain():
    return small_case(width=W, height=H, transparent=True, **BASE, **RTAO)


def _stacked():
    # (as walk e of test_gpu_context_reuse.py: a pool of one slot per pixel, far too small for the stacked segments)
    return _stacked_case(n=1100, width=W, height=H, ppll_expected_avg_depth_complexity=1, **BASE)


P = PEEL_LAYERS
# name: (case, mode, options, launches of the first frame, launches of the next frame)
CASES = {
    "mode 2, prism": (_plain, 2, {}, _oit(1, 1), None),
    "mode 2, capsule_entry": (_plain, 2, dict(ppll_fragment_source="capsule_entry"), _oit(gather=1), None),
    "mode 3": (_plain, 3, {}, _oit(1, 1), None),
    "mode 6, pool": (_plain, 6, {}, _oit(1, 1), None),
    "mode 3, the pool regrows": (_stacked, 3, {}, _oit(2, 1, ao={}), _oit(1, 1, ao={})),
    "mode 6, the pool regrows": (_stacked, 6, {}, _oit(2, 1, ao={}), _oit(1, 1, ao={})),
    "mode 6, streamed": (_plain, 6, dict(mboit_fragment_storage="streamed"), _oit(2), None),
    "mode 8": (_plain, 8, {}, _oit(1), None),
    "mode 10": (_plain, 10, {}, _oit(1), None),
    "mode 5": (_plain, 5, {}, _oit(1, gather=1), None),
    "mode 9": (_plain, 9, dict(depth_peeling_max_layers=P), _oit(1 + P, P, gather=1), None),
    "mode 11": (_plain, 11, {}, dict(AO, k_render_rt=1), None),
    "mode 11, MLAT": (_plain, 11, dict(use_mlat=True), dict(AO, k_render_rt=1), None),   # (lv_mlat_render records its kernel in that slot)
}


def _render(ctx, mode, tiles):
    if tiles is None:
        return ctx.render(mode)
    import torch
    out = torch.zeros((len(tiles), TILE, TILE, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_tiles_device(out.data_ptr(), tiles, TILE, TILE, mode=mode)
    ctx.stats()   # synchronises the context's stream
    return out.cpu().numpy()


def _frame(ctx, mode, tiles):
    ctx.reset_timers()
    img = _render(ctx, mode, tiles)
    st = ctx.stats()
    launches = {name: len(ctx.kernel_times(k)) for k, name in enumerate(capi.KERNEL_NAMES)}
    assert launches == {name: int(st.kernel_launches[k]) for k, name in enumerate(capi.KERNEL_NAMES)}
    return img, st, launches


def _ms_fields(st):
    return {n: getattr(st, n) for n, _ in capi.Stats._fields_ if n.startswith("ms_") and n != "ms_kernel_avg"}


@pytest.mark.parametrize("tiled", [False, True], ids=["whole", "tiles"])
@pytest.mark.parametrize("name", list(CASES))
def test_launches_and_phase_marks(hip_lib, name, tiled):
    make, mode, options, first, steady = CASES[name]
    tiles = TILES if tiled else None
    c = make()
    rtao = "ambient_occlusion_mode" in c.settings
    idle = set() if rtao else {"ms_ao"}   # no kernel between its two marks
    counters = COUNTERS if rtao else COUNTERS + ("prims_tested",)
    ctx = c.hip_context()
    ctx.set_options(options)
    ctx.set_option("kernel_timers", "all")
    if mode == 9:   # P of the table: the deepest requested pixel holds at least depth_peeling_max_layers fragments
        ctx.render(9)
        counts = ctx.depth_peeling_buffers()[2]
        mask = np.zeros((H, W), bool)
        for x, y in (TILES if tiled else [(0, 0)]):
            mask[y:y + (TILE if tiled else H), x:x + (TILE if tiled else W)] = True
        assert counts[mask].max() >= PEEL_LAYERS
        ctx = c.hip_context()
        ctx.set_options(options)
    frames = []
    for k, want in enumerate((first, steady or first)):
        img, st, launches = _frame(ctx, mode, tiles)
        ms = _ms_fields(st)
        print(name, "tiles" if tiled else "whole", "frame", k, launches, {n: v for n, v in ms.items() if v != 0.0})
        # (a) launches per slot
        assert launches == dict({n: 0 for n in capi.KERNEL_NAMES}, **want), (name, k)
        # (b) the phases this mode has, each with a kernel inside; together they are the frame
        phases = PHASES_RT if mode == 11 else PHASES_OIT
        assert {n for n, v in ms.items() if v != 0.0} - idle == (phases | BUILD_FIELDS) - idle, (name, k)
        assert all(ms[n] > 0.0 for n in phases - idle) and all(ms[n] >= 0.0 for n in idle), (name, k)
        assert abs(sum(ms[n] for n in phases - {"ms_total"}) - ms["ms_total"]) <= 1e-3   # event times: float32 ms of exact ticks
        for slot, n in enumerate(capi.KERNEL_NAMES):
            assert (st.ms_kernel_avg[slot] > 0.0) == (launches[n] > 0), (name, k, n)
        frames.append((img, st))
    # the frame after a regrown one: the same image, the same counters (the front end counted once)
    assert np.array_equal(frames[0][0], frames[1][0])
    for f in counters:
        assert getattr(frames[0][1], f) == getattr(frames[1][1], f), (name, f)
    # (c) kernel_timers = none: the same image, nothing recorded
    ctx.set_option("kernel_timers", "none")
    img, st, launches = _frame(ctx, mode, tiles)
    assert np.array_equal(img, frames[1][0])
    assert launches == {n: 0 for n in capi.KERNEL_NAMES}
    ms = _ms_fields(st)
    assert all(ms[n] == 0.0 for n in FRAME_FIELDS)
    for f in counters:
        assert getattr(st, f) == getattr(frames[1][1], f), (name, f)
