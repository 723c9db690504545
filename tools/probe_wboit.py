"""Rendering mode 8 (Weighted Blended OIT) against mode 2 on bench.py's c4 scene, in one process: the 1M-segment tornado streamlines
through lv_set_trajectories, 1920 x 1080, c4's settings and transparent transfer function.  Per run (mode 2; mode 8 with
wboit_depth_weight = reference and = opengl): warm-up frames, then timed frames (lv_render_device into a device image, wall clock per
frame with the stream synchronised, and the per-kernel timers of lv_get_kernel_times: the pass / the fragment stage of mode 2 / the
resolve), device_bytes, the fragment count, and for mode 8 the prediction of DESIGN.md 6 next to the measured pass: kept fragments x
atomic requests per fragment / 19.5 G requests/s, with the requests counted from the frame's own sums (lv_wboit_get_buffers,
untimed): 1 for the count word + the fragment's non-zero terms, of which at most 5.  Writes profiles/wboit_c4.json.

    python tools/probe_wboit.py [--frames 30] [--warmup 5] [--out profiles/wboit_c4.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (c4's settings and line width)
from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm  # noqa: E402

KERNELS = {"raster": 7, "shade": 6, "resolve": 4}   # LV_KERNEL_PPLL_RASTER / _SHADE / _RESOLVE
ATOMIC_RATE = 19.5e9                                 # requests/s, DESIGN.md 6 (streamed mode 6 and mode 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wboit_c4.json"))
    args = ap.parse_args()
    import torch
    wl = bench.WORKLOADS["c4"]
    W, H = 1920, 1080
    tr = scenes.normalize(scenes.tornado())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    attr = np.ascontiguousarray(tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes, dtype=np.float32)
    ctx = capi.Context(0)
    ctx.set_option("line_width", bench.LINE_WIDTH)
    ctx.set_trajectories(tr.positions, attr, tr.line_offsets)
    ctx.set_transfer_function(tfm.standard_transparent(), *flow.attribute_range())
    view, proj, fovy, near, far = camera.default_camera(W, H)
    ctx.set_camera(view, proj, fovy, near, far, W, H)
    ctx.set_options(wl["settings"])
    ctx.build_accel()
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    tile_w, tile_h = int(wl["settings"].get("ppll_tile_width", 2)), int(wl["settings"].get("ppll_tile_height", 8))
    padded = (-(-W // tile_w) * tile_w) * (-(-H // tile_h) * tile_h)
    runs = [("mode2", 2, None), ("mode8_reference", 8, "reference"), ("mode8_opengl", 8, "opengl")]
    result = {"workload": "c4 scene and settings (bench.py), modes 2 and 8", "source_sha": build.source_sha(),
              "library": os.path.basename(capi.LIB_PATH), "frames": args.frames, "warmup": args.warmup, "padded_pixels": padded,
              "atomic_rate_assumed": ATOMIC_RATE, "runs": {}}
    med = lambda v: float(np.median(v)) if len(v) else None   # noqa: E731
    for name, mode, weight in runs:
        if weight:
            ctx.set_option("wboit_depth_weight", weight)
        for _ in range(args.warmup):
            ctx.render_device(image.data_ptr(), mode=mode)
        torch.cuda.synchronize()
        ctx.reset_timers()
        wall = []
        for _ in range(args.frames):
            t0 = time.perf_counter()
            ctx.render_device(image.data_ptr(), mode=mode)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.stats()
        raster = np.asarray(ctx.kernel_times(KERNELS["raster"]), dtype=np.float64)
        per_frame = max(1, int(round(len(raster) / max(args.frames, 1))))
        run = {"mode": mode, "weight": weight, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
               "frame_ms_p90": float(np.percentile(wall, 90)), "ms_total": st.ms_total, "fragments": int(st.fragments),
               "max_depth_complexity": int(st.max_depth_complexity), "pool_slots": int(st.ppll_pool_nodes),
               "device_bytes": int(st.device_bytes), "raster_launches_per_frame": per_frame,
               "kernels_ms_median": {"raster": [med(raster[i::per_frame]) for i in range(per_frame)],
                                     "shade": med(ctx.kernel_times(KERNELS["shade"])) if mode == 2 else None,
                                     "resolve": med(ctx.kernel_times(KERNELS["resolve"]))}}
        if mode == 8:
            run["frame_memory_bytes"] = padded * (5 * 8 + 8)
            sums, counts = ctx.wboit_buffers()
            frags = int(counts.sum(dtype=np.int64))
            # a pixel's zero sum means none of its fragments issued that add (terms are >= 0); a non-zero one is counted as one add
            # per fragment of the pixel: an upper bound that is exact unless single fragments of a pixel have a zero channel
            requests = frags + int((counts[..., None].astype(np.int64) * (sums != 0)).sum())
            pass_ms = sum(x for x in run["kernels_ms_median"]["raster"] if x is not None)
            run["atomic_requests"] = requests
            run["requests_per_fragment"] = requests / max(frags, 1)
            run["pass_ms_predicted"] = requests / ATOMIC_RATE * 1e3
            run["pass_ms_measured"] = pass_ms
            run["requests_per_second_measured"] = requests / (pass_ms * 1e-3) if pass_ms else None
        result["runs"][name] = run
        print(name, json.dumps(run), flush=True)
    m2 = result["runs"]["mode2"]["frame_ms_median"]
    for name in result["runs"]:
        if name != "mode2":
            result[name + "_over_mode2"] = result["runs"][name]["frame_ms_median"] / m2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
