"""Rendering mode 1 (deferred shading on a visibility buffer) next to the ray tracer on the same triangles, in one process: the
1M-segment tornado streamlines through lv_set_trajectories (12 M tube triangles, tessellated on the device), config 2's settings
(primary rays only, AO and depth cues off), the opaque transfer function, 1920 x 1080 and 3840 x 2160.  Per resolution and run --
mode 1, mode 11 with geometry_mode = "Triangle Mesh", mode 11 on the analytic capsules: the reference's own comparison of its
"Deferred Draw Indexed" and ray-tracing states -- warm-up frames, then timed frames (lv_render_device into a device image, wall clock
per frame with the stream synchronised) and the per-kernel timers of lv_get_kernel_times.  Mode 1's split: LV_KERNEL_PPLL_RASTER is the
visibility pass with its clear, LV_KERNEL_PPLL_RESOLVE the shading pass.  Reads nothing outside the repository.

The knobs LV_VIS_SMALL and LV_VIS_PRELOAD are compile-time: build the variants with
    python tools/variants.py build vis_small4:-DLV_VIS_SMALL=4u vis_small16:-DLV_VIS_SMALL=16u vis_small256:-DLV_VIS_SMALL=256u vis_preload:-DLV_VIS_PRELOAD=1
and name them with --variants: each runs in a child process of its own (LV_LIB_PATH), mode 1 only, --repeats times each, interleaved
with the regular build, so that the spread of the regular build stands next to the difference.  Writes profiles/deferred_c2.json.

    python tools/probe_deferred.py [--frames 10] [--warmup 2] [--variants vis_small4 vis_small16 vis_small256 vis_preload]
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

KERNELS = {"render_rt": 2, "resolve": 4, "raster": 7}   # LV_KERNEL_RENDER_RT, LV_KERNEL_PPLL_RESOLVE, LV_KERNEL_PPLL_RASTER
RESOLUTIONS = [(1920, 1080), (3840, 2160)]
RUNS = [("mode1", 1, {}), ("mode11_triangle_mesh", 11, {"geometry_mode": "Triangle Mesh"}), ("mode11_capsules", 11, {"geometry_mode": "AABBs (analytic)"})]


def measure(args, runs):
    import torch
    import bench  # (config 2's settings and the line width)
    from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm
    tr = scenes.normalize(scenes.tornado())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    attr = np.ascontiguousarray(tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes, dtype=np.float32)
    ctx = capi.Context(0)
    ctx.set_option("line_width", bench.LINE_WIDTH)
    ctx.set_trajectories(tr.positions, attr, tr.line_offsets)
    ctx.set_transfer_function(tfm.standard(), *flow.attribute_range())
    ctx.set_options(bench.WORKLOADS["c2"]["settings"])
    result = {"source_sha": build.source_sha(), "library": os.path.basename(capi.LIB_PATH), "frames": args.frames, "warmup": args.warmup,
              "runs": {}}
    for W, H in RESOLUTIONS:
        view, proj, fovy, near, far = camera.default_camera(W, H)
        ctx.set_camera(view, proj, fovy, near, far, W, H)
        image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        for name, mode, settings in runs:
            ctx.set_options(settings)
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
            run = {"mode": mode, "width": W, "height": H, "settings": settings, "frame_ms_median": float(np.median(wall)),
                   "frame_ms_min": float(np.min(wall)), "frame_ms_max": float(np.max(wall)), "frame_ms_all": [float(x) for x in wall],
                   "gpu_frame_ms": float(st.ms_total), "fragments": int(st.fragments), "tube_triangles": int(st.num_tube_triangles),
                   "segments": int(st.num_segments), "device_bytes": int(st.device_bytes),
                   "kernel_ms_median": {k: (float(np.median(v)) if len(v) else None) for k, v in times.items()}}
            result["runs"]["%s_%dx%d" % (name, W, H)] = run
            print(name, "%dx%d" % (W, H), json.dumps({k: v for k, v in run.items() if k != "frame_ms_all"}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", nargs="*", default=[])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deferred_c2.json"))
    args = ap.parse_args()
    if args.child:   # one mode-1 measurement under the library LV_LIB_PATH names; the result on the last line
        runs = measure(args, RUNS[:1])["runs"]
        print("RESULT " + json.dumps({k: {"frame_ms_median": v["frame_ms_median"], "kernel_ms_median": v["kernel_ms_median"]}
                                      for k, v in runs.items()}), flush=True)
        return
    result = measure(args, RUNS)
    result["workload"] = "tornado scene (1M segments, 12M tube triangles), config 2's settings, opaque transfer function; modes 1 and 11"
    if args.variants:
        from linevis_amd import build
        libs = {"regular": build.LIB}
        libs.update({v: os.path.join(build.OUT_DIR, "variants", v + ".so") for v in args.variants})
        knobs = {name: [] for name in libs}
        for _ in range(args.repeats):
            for name, lib in libs.items():   # interleaved: drift hits every build alike
                env = dict(os.environ, LV_LIB_PATH=lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--frames", str(args.frames),
                                      "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
                line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
                if out.returncode != 0 or not line:
                    raise SystemExit("variant %s failed (exit status %d):\n%s" % (name, out.returncode, out.stderr[-2000:]))
                knobs[name].append(json.loads(line[-1][7:]))
                print("knob", name, json.dumps(knobs[name][-1]), flush=True)
        result["knobs_mode1_per_process"] = knobs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
