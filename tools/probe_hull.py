"""The simulation-mesh hull in rendering modes 5, 8 and 10 (K = 8) and -- hull_fragment_pool = on -- in the pooled modes 2 and 3 on the
config-4 scene: the 1M-segment tornado streamlines at
1920 x 1080 with config 4's settings and the transparent transfer function, scenes.box_hull around the data with n = 8 (768
triangles) and n = 64 (49 152 triangles).  Per mode, in ONE process: the frame without a hull mesh, then with each box -- warm-up
frames, then 5 timed frames (lv_render_device into a device image, wall clock per frame with the stream synchronised; the median is the
figure) and the per-kernel timers of lv_get_kernel_times (LV_KERNEL_PPLL_RASTER = the line pass, LV_KERNEL_HULL = the hull pass,
LV_KERNEL_PPLL_RESOLVE = the resolve; modes 2 and 3: LV_KERNEL_HULL holds two launches per frame, the record pass and the hull's fragment
stage, and the figure is their sum; LV_KERNEL_PPLL_SHADE = the lines' fragment stage).  Three such processes run one after the other.
Without --modes the three pool-free modes are measured, as before; --modes picks others (--modes mode2,mode3,mode8 --out
profiles/hull_pool_c4.json is the pooled hull's measurement).

The timing gate is the parent commit, not this code: with --parent-tree DIR (a checkout of the parent commit with its library built)
the no-hull frames of the three modes are measured in three processes of the parent too, interleaved with this build's, and the
result records both and whether this build's medians stay within the parent's own spread above the parent's slowest process.
Reads nothing outside the repository and the given tree.  Writes profiles/hull_c4.json.

    python tools/probe_hull.py [--frames 5] [--warmup 2] [--processes 3] [--parent-tree DIR] [--modes mode5,mode8,...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"gather": 3, "resolve": 4, "shade": 6, "raster": 7, "hull": 8}   # LV_KERNEL_PPLL_GATHER, _RESOLVE, _SHADE, _RASTER, LV_KERNEL_HULL
MODES = [("mode5", 5, {}), ("mode8", 8, {}), ("mode10_k8", 10, {"atomic_loop_num_layers": 8}),
         ("mode2", 2, {"hull_fragment_pool": "on"}), ("mode3", 3, {"hull_fragment_pool": "on"})]   # (the pooled modes: behind the switch)
DEFAULT_MODES = "mode5,mode8,mode10_k8"   # without --modes: the three of profiles/hull_c4.json; the pooled modes on request
BOXES = [8, 64]
W, H = 1920, 1080


def measure(args, tree):
    """one process: every mode without a hull and -- when the tree's library has the hull -- with the two boxes"""
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
    ctx.set_options(bench.WORKLOADS["c4"]["settings"])
    view, proj, fovy, near, far = camera.default_camera(W, H)
    ctx.set_camera(view, proj, fovy, near, far, W, H)
    image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    has_hull = hasattr(ctx, "set_hull_mesh")
    kernels = {k: i for k, i in KERNELS.items() if has_hull or k != "hull"}
    hulls = [("no_hull", None)]
    if has_hull:
        lo, hi = tr.positions.min(0), tr.positions.max(0)
        hulls += [("box_n%d" % n, scenes.box_hull((lo, hi), n, 0.05)) for n in BOXES]
    result = {"source_sha": build.source_sha(), "frames": args.frames, "warmup": args.warmup, "runs": {}}
    for hull_name, hull in hulls:
        if has_hull:
            ctx.set_hull_mesh(*((hull.triangle_indices, hull.positions, hull.normals) if hull else (None, None, None)))
            if hull:
                ctx.set_option("hull_opacity", 0.3)
        for name, mode, settings in MODES:
            if name not in args.selected:
                continue
            try:
                ctx.set_options(settings)
            except capi.LineVisError:      # (a parent tree without the switch: its pooled modes are measured without a hull only)
                if hull is not None:
                    continue
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
            times = {k: np.asarray(ctx.kernel_times(i), dtype=np.float64) for k, i in kernels.items()}
            if mode in (2, 3) and len(times.get("hull", ())):   # two launches per frame: the frame's sum (a mode-3 frame that regrows
                # its pool has three: the warm-up frames absorb it, --warmup >= 1; another count is reported as it is, not summed)
                if len(times["hull"]) == 2 * args.frames:
                    times["hull"] = times["hull"].reshape(args.frames, 2).sum(1)
            run = {"mode": mode, "hull": hull_name, "hull_triangles": 0 if hull is None else int(len(hull.triangle_indices)),
                   "frame_ms_median": float(np.median(wall)), "frame_ms_all": [float(x) for x in wall], "gpu_frame_ms": float(st.ms_total),
                   "fragments": int(st.fragments), "max_depth_complexity": int(st.max_depth_complexity),
                   "kernel_ms_median": {k: (float(np.median(v)) if len(v) else None) for k, v in times.items()}}
            result["runs"]["%s_%s" % (name, hull_name)] = run
            print(name, hull_name, json.dumps({k: v for k, v in run.items() if k != "frame_ms_all"}), flush=True)
    return result


def child(args, tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--frames", str(args.frames), "--warmup",
                          str(args.warmup), "--modes", ",".join(args.selected)], capture_output=True, text=True, timeout=900, cwd=tree)
    line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        raise SystemExit("the process on %s failed (exit status %d):\n%s" % (tree, out.returncode, out.stderr[-3000:]))
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--modes", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_c4.json"))
    args = ap.parse_args()
    args.selected = [m for m in (args.modes or DEFAULT_MODES).split(",") if m]
    unknown = [m for m in args.selected if m not in [name for name, _, _ in MODES]]
    if unknown:
        ap.error("unknown modes %s (known: %s)" % (unknown, ", ".join(name for name, _, _ in MODES)))
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
        k = this[0]["runs"][key]["kernel_ms_median"]
        summary[key] = {"frame_ms_median_per_process": med(this, key), "fragments": this[0]["runs"][key]["fragments"],
                        "kernel_ms_median_first_process": k}
    result = {"workload": "config-4 scene (tornado, 1M segments, 1920 x 1080, config 4's settings, transparent transfer function); "
                          "%s (mode 10: K = 8; modes 2 and 3: hull_fragment_pool = on) without a hull mesh and with box_hull n = 8 / n = 64, "
                          "hull_opacity 0.3" % ", ".join(args.selected),
              "frames": args.frames, "warmup": args.warmup, "summary": summary, "processes": this}
    if parent:
        gate = {}
        for name, _, _ in MODES:
            key = name + "_no_hull"
            if key not in this[0]["runs"] or key not in parent[0]["runs"]:
                continue
            p, t = med(parent, key), med(this, key)
            spread = max(p) - min(p)
            gate[key] = {"parent_ms": p, "this_ms": t, "parent_spread_ms": spread, "this_median_ms": float(np.median(t)),
                         "parent_median_ms": float(np.median(p)), "not_slower": bool(np.median(t) <= np.median(p) + spread)}
        result["timing_gate_no_hull_against_parent"] = gate
        result["parent_source_sha"] = parent[0]["source_sha"]
        result["parent_processes"] = parent
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k in ("summary", "timing_gate_no_hull_against_parent")}, indent=1))


if __name__ == "__main__":
    main()
