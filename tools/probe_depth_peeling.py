"""Rendering modes 9 (depth peeling) and 5 (depth complexity) against modes 2 and 8 on bench.py's c4 scene, in one process: the
1M-segment tornado streamlines through lv_set_trajectories, 1920 x 1080, c4's settings and transparent transfer function.  Per run
(mode 2, mode 8, mode 5, mode 9): warm-up frames, then timed frames (lv_render_device into a device image, wall clock per frame with
the stream synchronised) and the per-kernel timers of lv_get_kernel_times.  Mode 9's split: LV_KERNEL_PPLL_RASTER holds the count pass
and then one launch per peel pass, LV_KERNEL_PPLL_GATHER the reduce, LV_KERNEL_PPLL_SHADE the layer launches, LV_KERNEL_PPLL_RESOLVE
the blit (the rings keep the last 512 launches: sums are scaled from the launches they hold).  Reads nothing outside the repository.

The knobs LV_PEEL_MASK_DONE and LV_PEEL_PRELOAD are compile-time: build the variants with
    python tools/variants.py build peel_mask_done:-DLV_PEEL_MASK_DONE=1 peel_preload:-DLV_PEEL_PRELOAD=1
and name them with --variants: each runs in a child process of its own (LV_LIB_PATH), mode 9 only, --repeats times each, interleaved
with the regular build, so that the spread of the regular build stands next to the difference.  Writes profiles/depth_peeling_c4.json.

    python tools/probe_depth_peeling.py [--frames 5] [--warmup 1] [--max-layers 2000] [--variants peel_mask_done peel_preload]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"gather": 3, "resolve": 4, "shade": 6, "raster": 7}   # LV_KERNEL_PPLL_*


def measure(args, modes):
    import torch
    import bench  # (c4's settings and line width)
    from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm
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
    ctx.set_option("depth_peeling_max_layers", args.max_layers)
    ctx.build_accel()
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    result = {"source_sha": build.source_sha(), "library": os.path.basename(capi.LIB_PATH), "frames": args.frames, "warmup": args.warmup,
              "max_layers": args.max_layers, "runs": {}}
    for mode in modes:
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
        times = {k: np.asarray(ctx.kernel_times(i), dtype=np.float64) for k, i in KERNELS.items()}
        run = {"mode": mode, "frame_ms_median": float(np.median(wall)), "frame_ms_min": float(np.min(wall)),
               "frame_ms_max": float(np.max(wall)), "frame_ms_all": [float(x) for x in wall], "fragments": int(st.fragments),
               "max_depth_complexity": int(st.max_depth_complexity), "device_bytes": int(st.device_bytes),
               "launches_held": {k: int(len(v)) for k, v in times.items()},
               "kernel_ms_median": {k: (float(np.median(v)) if len(v) else None) for k, v in times.items()}}
        if mode == 9:
            passes = min(int(st.max_depth_complexity), args.max_layers)
            raster = times["raster"]
            run["passes"] = passes
            if args.frames * (passes + 1) <= 512 and len(raster) == args.frames * (passes + 1):   # the ring holds every launch
                per = raster.reshape(args.frames, passes + 1)
                run["count_pass_ms"] = float(np.median(per[:, 0]))
                run["first_peel_pass_ms"] = float(np.median(per[:, 1])) if passes else None
                run["peel_passes_ms_sum"] = float(np.median(per[:, 1:].sum(axis=1)))
                run["peel_pass_ms_by_index"] = [float(x) for x in np.median(per[:, 1:], axis=0)]
            else:   # the last 512 launches: peel passes (the count pass is one in passes + 1 of them)
                run["peel_passes_ms_sum_scaled"] = float(np.mean(raster)) * passes if len(raster) else None
            run["layer_launches_ms_sum_scaled"] = float(np.mean(times["shade"])) * passes if len(times["shade"]) else None
        result["runs"]["mode%d" % mode] = run
        print("mode", mode, json.dumps({k: v for k, v in run.items() if k not in ("peel_pass_ms_by_index", "frame_ms_all")}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-layers", type=int, default=2000)
    ap.add_argument("--variants", nargs="*", default=[])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_peeling_c4.json"))
    args = ap.parse_args()
    if args.child:   # one mode-9 measurement under the library LV_LIB_PATH names; the result on the last line
        print("RESULT " + json.dumps(measure(args, [9])["runs"]["mode9"]), flush=True)
        return
    result = measure(args, [2, 8, 5, 9])
    result["workload"] = "c4 scene and settings (bench.py), modes 2, 8, 5 and 9"
    if args.variants:
        from linevis_amd import build
        libs = {"regular": build.LIB}
        libs.update({v: os.path.join(build.OUT_DIR, "variants", v + ".so") for v in args.variants})
        knobs = {name: [] for name in libs}
        for _ in range(args.repeats):
            for name, lib in libs.items():   # interleaved: drift hits every build alike
                env = dict(os.environ, LV_LIB_PATH=lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(args.frames),
                                      "--warmup", str(args.warmup), "--max-layers", str(args.max_layers)], env=env,
                                     capture_output=True, text=True, timeout=600)
                line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
                if out.returncode != 0 or not line:
                    raise SystemExit("variant %s failed (exit status %d):\n%s" % (name, out.returncode, out.stderr[-2000:]))
                knobs[name].append(json.loads(line[-1][7:])["frame_ms_median"])
                print("knob", name, knobs[name][-1], flush=True)
        result["knobs_mode9_frame_ms_median_per_process"] = knobs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
