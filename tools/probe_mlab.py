"""Rendering mode 3 (MLAB) against mode 2 on bench.py's c4 scene, in one process: the 1M-segment tornado streamlines through
lv_set_trajectories, 1920 x 1080, c4's settings and transparent transfer function.  Per mode (mode 2; mode 3 with K = 1, 8, 16, 64):
warm-up frames, then timed frames (lv_render_device into a device image, wall clock per frame with the stream synchronised, and the
per-kernel timers of lv_get_kernel_times).  Writes profiles/mlab_c4.json.

    python tools/probe_mlab.py [--frames 20] [--warmup 5] [--out profiles/mlab_c4.json]
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

KERNELS = {"raster": 7, "shade": 6, "resolve": 4}   # LV_KERNEL_PPLL_RASTER / _SHADE / _RESOLVE (the fold of mode 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlab_c4.json"))
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
    runs = [("mode2", 2, None), ("mode3_K1", 3, 1), ("mode3_K8", 3, 8), ("mode3_K16", 3, 16), ("mode3_K64", 3, 64)]
    result = {"workload": "c4 scene and settings (bench.py), modes 2 and 3", "source_sha": build.source_sha(),
              "frames": args.frames, "warmup": args.warmup, "runs": {}}
    for name, mode, K in runs:
        if K is not None:
            ctx.set_option("mlab_num_layers", K)
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
        kern = {k: float(np.median(ctx.kernel_times(i))) if len(ctx.kernel_times(i)) else None for k, i in KERNELS.items()}
        result["runs"][name] = {"mode": mode, "K": K, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
                                "kernels_ms_median": kern, "ms_ppll_clear": st.ms_ppll_clear, "ms_ppll_gather": st.ms_ppll_gather,
                                "ms_ppll_resolve": st.ms_ppll_resolve, "ms_total": st.ms_total, "fragments": int(st.fragments),
                                "max_depth_complexity": int(st.max_depth_complexity), "pool_slots": int(st.ppll_pool_nodes)}
        print(name, json.dumps(result["runs"][name]), flush=True)
    m2 = result["runs"]["mode2"]["frame_ms_median"]
    result["mode3_K8_over_mode2"] = result["runs"]["mode3_K8"]["frame_ms_median"] / m2
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"mode3_K8_over_mode2": result["mode3_K8_over_mode2"]}))


if __name__ == "__main__":
    main()
