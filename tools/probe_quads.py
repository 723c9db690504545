"""The two line primitives in rendering modes 5, 8 and 10 (K = 8) on the config-4 scene: the 1M-segment tornado streamlines at
1920 x 1080 with config 4's settings and the transparent transfer function, line_primitive_mode = "Tube (Programmable Pull)" against
"Quads (Programmable Pull)" in the SAME process.  Per mode and primitive: warm-up frames, then 100 timed frames (lv_render_device into
a device image, wall clock per frame with the stream synchronised; the median is the figure), the per-kernel timers of
lv_get_kernel_times (LV_KERNEL_PPLL_RASTER = the line pass, LV_KERNEL_PPLL_GATHER = mode 5's reduce, LV_KERNEL_PPLL_RESOLVE = the
resolve), the fragment count of lv_stats and the bytes the mode keeps per frame.  Three such processes run one after the other.

The timing gate is the parent commit, not this code: with --parent-tree DIR (a checkout of the parent commit with its library built)
the tube frames of the three modes are measured in three processes of the parent too, interleaved with this build's, and the result
records both and whether this build's medians stay within the parent's own spread above the parent's median.
Reads nothing outside the repository and the given tree.  Writes profiles/quads_c4.json.

    python tools/probe_quads.py [--frames 100] [--warmup 5] [--processes 3] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"gather": 3, "resolve": 4, "raster": 7}   # LV_KERNEL_PPLL_GATHER, _RESOLVE, _RASTER
MODES = [("mode5", 5, {}), ("mode8", 8, {}), ("mode10_k8", 10, {"atomic_loop_num_layers": 8})]
PRIMITIVES = [("tubes", "Tube (Programmable Pull)"), ("quads", "Quads (Programmable Pull)")]
W, H = 1920, 1080


def frame_bytes(mode, settings, padded_pixels):
    """what a frame of the mode keeps per padded pixel besides the image: the requested-pixel mask and the count (4 B each), then mode
    8's five sums or mode 10's K slots and five tail sums (8 B each)"""
    words = {5: 0, 8: 5, 10: settings.get("atomic_loop_num_layers", 8) + 5}[mode]
    return int(padded_pixels * (8 + 8 * words))


def measure(args, tree):
    """one process: every mode with tubes and -- when the tree's library knows the option -- with quads"""
    sys.path.insert(0, tree)
    import torch
    import bench  # (config 4's settings and the line width)
    from linevis_amd import build, camera, capi, host_api, scenes, transfer_function as tfm
    tr = scenes.normalize(scenes.tornado())
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    ctx = capi.Context(0)
    ctx.set_option("line_width", bench.LINE_WIDTH)
    ctx.set_trajectories(tr.positions, np.ascontiguousarray(tr.attributes, dtype=np.float32), tr.line_offsets)
    ctx.set_transfer_function(tfm.standard_transparent(), *flow.attribute_range())
    settings4 = bench.WORKLOADS["c4"]["settings"]
    ctx.set_options(settings4)
    view, proj, fovy, near, far = camera.default_camera(W, H)
    ctx.set_camera(view, proj, fovy, near, far, W, H)
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    has_quads = hasattr(ctx, "line_quad_fragments")
    tw, th = int(settings4.get("ppll_tile_width", 2)), int(settings4.get("ppll_tile_height", 8))
    padded = (-(-W // tw) * tw) * (-(-H // th) * th)
    result = {"source_sha": build.source_sha(), "frames": args.frames, "warmup": args.warmup, "runs": {}}
    for prim_name, prim in PRIMITIVES[:2 if has_quads else 1]:
        if has_quads:
            ctx.set_option("line_primitive_mode", prim)
        for name, mode, settings in MODES:
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
            run = {"mode": mode, "primitive": prim_name, "frame_ms_median": float(np.median(wall)), "frame_ms_all": [float(x) for x in wall],
                   "gpu_frame_ms": float(st.ms_total), "fragments": int(st.fragments), "max_depth_complexity": int(st.max_depth_complexity),
                   "frame_bytes": frame_bytes(mode, settings, padded),
                   "kernel_ms_median": {k: (float(np.median(v)) if len(v) else None) for k, v in times.items()}}
            result["runs"]["%s_%s" % (name, prim_name)] = run
            print(name, prim_name, json.dumps({k: v for k, v in run.items() if k != "frame_ms_all"}), flush=True)
    return result


def child(args, tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--frames", str(args.frames), "--warmup",
                          str(args.warmup)], capture_output=True, text=True, timeout=900, cwd=tree)
    line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit("the process on %s failed (exit status %d):\n%s" % (tree, out.returncode, out.stderr[-3000:]))
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quads_c4.json"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args, args.child)), flush=True)
        return
    this, parent = [], []
    for i in range(args.processes):   # interleaved: drift hits both builds alike
        if args.parent_tree:
            parent.append(child(args, os.path.abspath(args.parent_tree)))
            print("parent process", i, json.dumps({k: v["frame_ms_median"] for k, v in parent[-1]["runs"].items()}), flush=True)
        this.append(child(args, ROOT))
        print("process", i, json.dumps({k: v["frame_ms_median"] for k, v in this[-1]["runs"].items()}), flush=True)
    med = lambda procs, key: [p["runs"][key]["frame_ms_median"] for p in procs]
    summary = {}
    for key in this[0]["runs"]:
        r = this[0]["runs"][key]
        summary[key] = {"frame_ms_median_per_process": med(this, key), "fragments": r["fragments"], "frame_bytes": r["frame_bytes"],
                        "kernel_ms_median_per_process": [p["runs"][key]["kernel_ms_median"] for p in this]}
    result = {"workload": "config-4 scene (tornado, 1M segments, 1920 x 1080, config 4's settings, transparent transfer function); "
                          "modes 5, 8 and 10 (K = 8) with line_primitive_mode = tubes / quads in the same process",
              "frames": args.frames, "warmup": args.warmup, "summary": summary, "processes": this}
    if parent:
        gate = {}
        for name, _, _ in MODES:
            key = name + "_tubes"
            p, t = med(parent, key), med(this, key)
            spread = max(p) - min(p)
            gate[key] = {"parent_ms": p, "this_ms": t, "parent_spread_ms": spread, "this_median_ms": float(np.median(t)),
                         "parent_median_ms": float(np.median(p)), "not_slower": bool(np.median(t) <= np.median(p) + spread)}
        result["timing_gate_tubes_against_parent"] = gate
        result["parent_source_sha"] = parent[0]["source_sha"]
        result["parent_processes"] = parent
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k in ("summary", "timing_gate_tubes_against_parent")}, indent=1))


if __name__ == "__main__":
    main()
