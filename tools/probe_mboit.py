"""Rendering mode 6 (MBOIT) against modes 2 and 3 on bench.py's c4 scene, in one process: the 1M-segment tornado streamlines through
lv_set_trajectories, 1920 x 1080, c4's settings and transparent transfer function.  Per run (mode 2; mode 3 with K = 8; mode 6 with
N = 4, 6, 8): warm-up frames, then timed frames (lv_render_device into a device image, wall clock per frame with the stream
synchronised, and the per-kernel timers of lv_get_kernel_times: rasteriser / fragment stage / resolve).  Then, untimed and with
collect_stats, the share of covered pixels that degenerate to the background for N = 4, 6, 8 at mboit_moment_bias = auto and at
ten times that bias.  Writes profiles/mboit_c4.json.

    python tools/probe_mboit.py [--frames 20] [--warmup 5] [--out profiles/mboit_c4.json]

--storage: mode 6 alone, per N = 4, 6, 8 with mboit_fragment_storage = pool and = streamed in the same process: frame time, the
two pass launches and the blend of the streamed frame (LV_KERNEL_PPLL_RASTER holds both launches of a frame, in order),
device_bytes of both, and whether the two frames are byte-identical.  Writes profiles/mboit_c4_streamed.json.

    python tools/probe_mboit.py --storage [--frames 30] [--warmup 5] [--out profiles/mboit_c4_streamed.json]
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

KERNELS = {"raster": 7, "shade": 6, "resolve": 4}   # LV_KERNEL_PPLL_RASTER / _SHADE / _RESOLVE (the sweeps of mode 6)
AUTO_BIAS = {4: 5e-7, 6: 5e-6, 8: 5e-5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--storage", action="store_true", help="mode 6 with mboit_fragment_storage = pool and = streamed (profiles/mboit_c4_streamed.json)")
    ap.add_argument("--only-mode-6", action="store_true", help="skip modes 2 and 3 and the degenerate-pixel frames (kernel tuning builds)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mboit_c4_streamed.json" if args.storage else "mboit_c4.json")
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
    if args.storage:
        return storage_runs(args, ctx, image)
    runs = [("mode2", 2, None), ("mode3_K8", 3, 8), ("mode6_N4", 6, 4), ("mode6_N6", 6, 6), ("mode6_N8", 6, 8)]
    if args.only_mode_6:
        runs = [r for r in runs if r[1] == 6]
    result = {"workload": "c4 scene and settings (bench.py), modes 2, 3 and 6", "source_sha": build.source_sha(), "library": os.path.basename(capi.LIB_PATH),
              "frames": args.frames, "warmup": args.warmup, "runs": {}}
    for name, mode, n in runs:
        if mode == 3:
            ctx.set_option("mlab_num_layers", n)
        if mode == 6:
            ctx.set_option("mboit_num_moments", n)
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
        result["runs"][name] = {"mode": mode, "n": n, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
                                "frame_ms_p90": float(np.percentile(wall, 90)),
                                "kernels_ms_median": kern, "ms_ppll_clear": st.ms_ppll_clear, "ms_ppll_gather": st.ms_ppll_gather,
                                "ms_ppll_resolve": st.ms_ppll_resolve, "ms_total": st.ms_total, "fragments": int(st.fragments),
                                "max_depth_complexity": int(st.max_depth_complexity), "pool_slots": int(st.ppll_pool_nodes)}
        print(name, json.dumps(result["runs"][name]), flush=True)
    if not args.only_mode_6:
        m2 = result["runs"]["mode2"]["frame_ms_median"]
        for name in ("mode3_K8", "mode6_N4", "mode6_N6", "mode6_N8"):
            result[name + "_over_mode2"] = result["runs"][name]["frame_ms_median"] / m2
        # degenerate pixels: covered = the pixels whose frame differs from a frame without any line (the background) at a bias
        # of 0.1, under which the CPU statement finds no degenerate single fragment
        ctx.set_option("collect_stats", True)
        result["degenerate"] = {}
        for n in (4, 6, 8):
            ctx.set_option("mboit_num_moments", n)
            ctx.set_option("mboit_moment_bias", 0.1)
            ctx.render_device(image.data_ptr(), mode=6)
            torch.cuda.synchronize()
            covered = int((image != 255).any(dim=2).sum().item()) + int(ctx.stats().mboit_degenerate_pixels)
            for label, bias in (("auto", "auto"), ("x10", 10.0 * AUTO_BIAS[n])):
                ctx.set_option("mboit_moment_bias", bias)
                ctx.render_device(image.data_ptr(), mode=6)
                torch.cuda.synchronize()
                deg = int(ctx.stats().mboit_degenerate_pixels)
                result["degenerate"]["N%d_%s" % (n, label)] = {"degenerate_pixels": deg, "covered_pixels": covered,
                                                               "share": deg / max(covered, 1)}
        print("degenerate", json.dumps(result["degenerate"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


def storage_runs(args, ctx, image):
    import torch
    result = {"workload": "c4 scene and settings (bench.py), mode 6, mboit_fragment_storage = pool | streamed", "source_sha": build.source_sha(),
              "library": os.path.basename(capi.LIB_PATH), "frames": args.frames, "warmup": args.warmup, "runs": {}}
    for n in (4, 6, 8):
        ctx.set_option("mboit_num_moments", n)
        frames = {}
        for storage in ("pool", "streamed"):
            ctx.set_option("mboit_fragment_storage", storage)
            for _ in range(args.warmup):
                ctx.render_device(image.data_ptr(), mode=6)
            torch.cuda.synchronize()
            ctx.reset_timers()
            wall = []
            for _ in range(args.frames):
                t0 = time.perf_counter()
                ctx.render_device(image.data_ptr(), mode=6)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.stats()
            frames[storage] = image.cpu().numpy().copy()
            med = lambda v: float(np.median(v)) if len(v) else None   # noqa: E731
            raster = np.asarray(ctx.kernel_times(KERNELS["raster"]), dtype=np.float64)
            run = {"n": n, "storage": storage, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
                   "frame_ms_p90": float(np.percentile(wall, 90)), "ms_total": st.ms_total, "fragments": int(st.fragments),
                   "max_depth_complexity": int(st.max_depth_complexity), "pool_slots": int(st.ppll_pool_nodes),
                   "device_bytes": int(st.device_bytes)}
            if storage == "streamed":   # two launches per frame: moments pass, colours pass
                run["kernels_ms_median"] = {"pass_moments": med(raster[0::2]), "pass_colours": med(raster[1::2]),
                                            "blend": med(ctx.kernel_times(KERNELS["resolve"]))}
                run["raster_launches_per_frame"] = len(raster) / max(args.frames, 1)
            else:
                run["kernels_ms_median"] = {"raster": med(raster), "shade": med(ctx.kernel_times(KERNELS["shade"])),
                                            "resolve": med(ctx.kernel_times(KERNELS["resolve"]))}
            result["runs"]["N%d_%s" % (n, storage)] = run
            print("N%d_%s" % (n, storage), json.dumps(run), flush=True)
        result["N%d_frames_identical" % n] = bool(np.array_equal(frames["pool"], frames["streamed"]))
        result["N%d_streamed_over_pool" % n] = result["runs"]["N%d_streamed" % n]["frame_ms_median"] / result["runs"]["N%d_pool" % n]["frame_ms_median"]
        print("N%d identical %s, streamed / pool %.3f" % (n, result["N%d_frames_identical" % n], result["N%d_streamed_over_pool" % n]), flush=True)
    ctx.set_option("mboit_fragment_storage", "pool")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
