"""The ray-traced simulation-mesh hull (rendering mode 11, hull_ray_tracing = on) on two scenes at 1920 x 1080: config 2 (the 100k-segment
helix bundle, opaque transfer function) and the config-4 transparent scene through the ray tracer's transparency loop (bench.py's
c4l: the 1M-segment tornado, opacity ramp 0.1 .. 0.6), with scenes.box_hull around the data, n = 8 (768 triangles) and n = 64 (49 152
triangles), hull_opacity 0.3.

In ONE process, scene by scene: the frame without a hull mesh (k_render_rt, the reference of the comparison), then with each box
(k_render_rt_hull) -- warm-up frames, then the timed frames (lv_render_device into a device image, wall clock per frame with the stream
synchronised; the median is the figure) and the LV_KERNEL_RENDER_RT timer of lv_get_kernel_times.  The hull LBVH build is the wall
clock of the first lv_trace_rays_hull call after lv_set_hull_mesh (one ray: build + one launch) minus that of the second call (the
launch alone), three times per box.  Writes profiles/hull_rt.json.

    python tools/probe_hull_rt.py [--frames 7] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL_RENDER_RT = 2   # LV_KERNEL_RENDER_RT (capi.KERNEL_NAMES)
BOXES = [8, 64]
W, H = 1920, 1080
SCENES = [("c2", "c2"), ("c4_transparent", "c4l")]


def measure(args, workload):
    import torch
    import bench
    from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm
    wl = bench.WORKLOADS[workload]
    tr = scenes.normalize({"tornado": scenes.tornado, "helix": scenes.helix_bundle}[wl["scene"]]())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    ctx = capi.Context(0)
    ctx.set_option("line_width", bench.LINE_WIDTH)
    ctx.set_trajectories(tr.positions, np.ascontiguousarray(tr.attributes, dtype=np.float32), tr.line_offsets)
    ctx.set_transfer_function(tfm.standard_transparent() if wl.get("transparent") else tfm.standard(), *flow.attribute_range())
    ctx.set_options(wl["settings"])
    view, proj, fovy, near, far = camera.default_camera(W, H)
    ctx.set_camera(view, proj, fovy, near, far, W, H)
    ctx.set_option("hull_ray_tracing", "on")
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    lo, hi = tr.positions.min(0), tr.positions.max(0)
    hulls = [("no_hull", None)] + [("box_n%d" % n, scenes.box_hull((lo, hi), n, 0.05)) for n in BOXES]
    runs = {}
    ray = (np.array([[0.0, 0.0, 2.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32))
    for name, hull in hulls:
        build_ms = []
        if hull is None:
            ctx.set_hull_mesh(None, None, None)
        else:
            for _ in range(3):
                ctx.set_hull_mesh(hull.triangle_indices, hull.positions, hull.normals)
                t0 = time.perf_counter()
                ctx.trace_rays_hull(ray[0], ray[1], 0.0, 1000.0)
                t1 = time.perf_counter()
                ctx.trace_rays_hull(ray[0], ray[1], 0.0, 1000.0)
                t2 = time.perf_counter()
                build_ms.append(((t1 - t0) - (t2 - t1)) * 1e3)
            ctx.set_option("hull_opacity", 0.3)
        for _ in range(args.warmup):
            ctx.render_device(image.data_ptr(), mode=capi.MODE_RAY_TRACER)
        torch.cuda.synchronize()
        ctx.reset_timers()
        wall = []
        for _ in range(args.frames):
            t0 = time.perf_counter()
            ctx.render_device(image.data_ptr(), mode=capi.MODE_RAY_TRACER)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        kernel = np.asarray(ctx.kernel_times(KERNEL_RENDER_RT), dtype=np.float64)
        runs[name] = {"hull_triangles": 0 if hull is None else int(len(hull.triangle_indices)),
                      "frame_ms_median": float(np.median(wall)), "frame_ms_all": [float(x) for x in wall],
                      "colour_kernel_ms_median": float(np.median(kernel)) if len(kernel) else None,
                      "hull_lbvh_build_ms": [float(x) for x in build_ms]}
        print(workload, name, json.dumps(runs[name]), flush=True)
    return {"workload": wl["name"], "source_sha": build.source_sha(), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_rt.json"))
    args = ap.parse_args()
    result = {"frames": args.frames, "warmup": args.warmup, "resolution": [W, H], "scenes": {}}
    for name, workload in SCENES:
        result["scenes"][name] = measure(args, workload)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
