"""What the spatial-hashing denoiser costs, on the c3c frame (bench.py: the 1M-segment tornado streamlines, 1920 x 1080, RTAO 64 spp on
the analytic capsules), in ONE process:

  * the same frame with ambient_occlusion_denoiser = None, SVGF and Spatial Hashing: warm-up frames, then timed frames -- wall clock
    per frame with the stream synchronised (the median is the figure) and the per-kernel timers LV_KERNEL_AO_PRIMARY,
    LV_KERNEL_AO_RAYS, LV_KERNEL_SH_WRITE, LV_KERNEL_SH_READ and LV_KERNEL_SH_TAIL of lv_get_kernel_times;
  * occupancy over a camera orbit of --orbit-frames frames around the data: occupied / stored / dropped / clears after every frame.

(The distinct keys per wave -- what a combine of equal keys inside a wave could save -- were counted by the write kernel that had such
a combine: 56.0 of 64 per level on this frame.  That kernel lost and is gone; DESIGN.md section 6 has its numbers.)

Writes profiles/spatial_hashing_c3c.json.

    python tools/probe_spatial_hashing.py [--frames 5] [--warmup 2] [--orbit-frames 24] [--num-cells 10000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
KERNELS = {"k_ao_primary": 0, "k_ao_rays": 1, "k_sh_write": 9, "k_sh_read": 10, "sh_tail": 11}
VARIANTS = [("none", {"ambient_occlusion_denoiser": "None"}),
            ("svgf", {"ambient_occlusion_denoiser": "SVGF"}),
            ("spatial_hashing", {"ambient_occlusion_denoiser": "Spatial Hashing"})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--orbit-frames", type=int, default=24)
    ap.add_argument("--num-cells", type=int, default=10000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_hashing_c3c.json"))
    args = ap.parse_args()
    import torch
    import bench
    from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm
    tr = scenes.normalize(scenes.tornado())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    ctx = capi.Context(0)
    ctx.set_option("line_width", bench.LINE_WIDTH)
    ctx.set_trajectories(tr.positions, np.ascontiguousarray(tr.attributes, dtype=np.float32), tr.line_offsets)
    ctx.set_transfer_function(tfm.standard(), *flow.attribute_range())
    ctx.set_options(bench.WORKLOADS["c3c"]["settings"])
    ctx.set_option("spatial_hashing_num_cells", args.num_cells)
    view, proj, fovy, near, far = camera.default_camera(W, H)
    ctx.set_camera(view, proj, fovy, near, far, W, H)
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    result = {"workload": bench.C3C, "source_sha": build.source_sha(), "frames": args.frames, "warmup": args.warmup,
              "num_cells": args.num_cells, "runs": {}}

    def frame():
        t0 = time.perf_counter()
        ctx.render_device(image.data_ptr(), mode=11)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, settings in VARIANTS:
        ctx.set_options(settings)
        for _ in range(args.warmup):
            frame()
        ctx.reset_timers()
        wall = [frame() for _ in range(args.frames)]
        times = {k: np.asarray(ctx.kernel_times(i), dtype=np.float64) for k, i in KERNELS.items()}
        run = {"frame_ms_median": float(np.median(wall)), "frame_ms_all": [float(x) for x in wall],
               "ao_hit_pixels": int(ctx.stats().ao_hit_pixels),
               "kernel_ms_median": {k: (float(np.median(v)) if len(v) else None) for k, v in times.items()},
               "kernel_ms_all": {k: [float(x) for x in v] for k, v in times.items() if len(v)}}
        if name.startswith("spatial_hashing"):
            st = ctx.spatial_hashing_stats(0)
            run["map"] = st
        result["runs"][name] = run
        print(name, json.dumps({k: v for k, v in run.items() if k not in ("frame_ms_all", "kernel_ms_all")}), flush=True)

    # occupancy over an orbit: one frame per pose, the map persists (a camera move does not clear it)
    ctx.set_options(VARIANTS[2][1])
    ctx.spatial_hashing_reset(0)
    orbit = []
    for k in range(args.orbit_frames):
        t = 2.0 * np.pi * k / args.orbit_frames
        view, proj, fovy, near, far = camera.default_camera(W, H, (float(0.8 * np.sin(t)), 0.1, float(0.8 * np.cos(t))))
        ctx.set_camera(view, proj, fovy, near, far, W, H)
        ctx.reset_timers()
        ms = frame()
        st = ctx.spatial_hashing_stats(0)
        w = ctx.kernel_times(KERNELS["k_sh_write"])
        orbit.append(dict(st, frame=k, frame_ms=ms, k_sh_write_ms=float(w[0]) if len(w) else None, fill=st["occupied"] / args.num_cells))
        print("orbit", json.dumps(orbit[-1]), flush=True)
    result["orbit"] = orbit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
