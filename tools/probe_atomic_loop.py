"""Rendering mode 10 (Atomic Loop 64) against mode 2 and streamed mode 6 on bench.py's c4 scene, in one process: the 1M-segment
tornado streamlines through lv_set_trajectories, 1920 x 1080, c4's settings and transparent transfer function.  Per run (mode 2; mode 6
with N = 4 and mboit_fragment_storage = streamed; mode 10 with K = 4, 8, 16): warm-up frames, then timed frames (lv_render_device
into a device image, wall clock per frame with the stream synchronised, and the per-kernel timers of lv_get_kernel_times: the
rasteriser launches / the fragment stage of mode 2 / the resolve), device_bytes, and the memory of a mode-10 frame by its formula:
(K + 5) x 8 B per padded pixel plus the two 4-byte per-pixel words.  Also: the share of the frame's fragments that went to the tail
(from lv_atomic_loop_get_buffers, untimed).  Writes profiles/atomic_loop_c4.json.

    python tools/probe_atomic_loop.py [--frames 30] [--warmup 5] [--out profiles/atomic_loop_c4.json]

The shortcut of lv_al64_insert (LV_AL64_SHORTCUT, lv_al64.h) is compared with a second library of the same tree, built with
-DLV_AL64_SHORTCUT=0 (LV_EXTRA_HIPCC_FLAGS of linevis_amd/build.py, or lv_render.hip alone) and loaded through LV_LIB_PATH; that
run writes a file of its own and names the build in it:

    LV_LIB_PATH=<that library> python tools/probe_atomic_loop.py --variant "LV_AL64_SHORTCUT=0" --out profiles/atomic_loop_c4_no_shortcut.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atomic_loop_c4.json"))
    ap.add_argument("--variant", default="default build", help="what LV_LIB_PATH's library was built with (recorded in the file)")
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
    ctx.set_option("mboit_fragment_storage", "streamed")
    ctx.set_option("mboit_num_moments", 4)
    ctx.build_accel()
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    tile_w, tile_h = int(wl["settings"].get("ppll_tile_width", 2)), int(wl["settings"].get("ppll_tile_height", 8))
    padded = (-(-W // tile_w) * tile_w) * (-(-H // tile_h) * tile_h)
    runs = [("mode2", 2, None), ("mode6_N4_streamed", 6, 4), ("mode10_K4", 10, 4), ("mode10_K8", 10, 8), ("mode10_K16", 10, 16)]
    result = {"workload": "c4 scene and settings (bench.py), modes 2, 6 (streamed) and 10", "source_sha": build.source_sha(),
              "library": os.path.basename(capi.LIB_PATH), "variant": args.variant, "frames": args.frames, "warmup": args.warmup, "padded_pixels": padded, "runs": {}}
    med = lambda v: float(np.median(v)) if len(v) else None   # noqa: E731
    for name, mode, n in runs:
        if mode == 10:
            ctx.set_option("atomic_loop_num_layers", n)
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
        run = {"mode": mode, "n": n, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
               "frame_ms_p90": float(np.percentile(wall, 90)), "ms_total": st.ms_total, "fragments": int(st.fragments),
               "max_depth_complexity": int(st.max_depth_complexity), "pool_slots": int(st.ppll_pool_nodes),
               "device_bytes": int(st.device_bytes), "raster_launches_per_frame": per_frame,
               "kernels_ms_median": {"raster": [med(raster[i::per_frame]) for i in range(per_frame)],
                                     "shade": med(ctx.kernel_times(KERNELS["shade"])) if mode == 2 else None,
                                     "resolve": med(ctx.kernel_times(KERNELS["resolve"]))}}
        if mode == 10:
            run["frame_memory_bytes"] = padded * ((n + 5) * 8 + 8)
            slots, tail = ctx.atomic_loop_buffers()
            in_slots = int((slots != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())
            run["fragments_in_slots"] = in_slots
            run["tail_share"] = 1.0 - in_slots / max(int(st.fragments), 1)
            run["tail_pixels"] = int((tail[..., 0] != 0).sum())
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
