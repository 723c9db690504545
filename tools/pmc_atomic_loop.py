"""Atomic requests of the rasterise-and-accumulate passes against their time, from one counter pass of its own over the probe:

    rocprofv3 --pmc TCC_EA0_ATOMIC_sum TCC_REQ_sum --kernel-trace --output-format csv -d <dir> -o p -- \\
        python tools/probe_atomic_loop.py --frames 3 --warmup 1 --out <dir>/probe.json
    python tools/pmc_atomic_loop.py <dir>/p_counter_collection.csv [--out profiles/atomic_loop_c4_pmc.json]

Per kernel of interest (the passes of modes 10 and 6, mode 2's rasteriser and fragment stage) and per distinct launch shape: the
median of each counter over its dispatches, the median time between the dispatch's timestamps, atomic requests per second and that
rate in bytes at 64 B per request.  The mode-10 dispatches come in the probe's order K = 4, 8, 16 and are grouped by that order."""
import argparse
import collections
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from linevis_amd import build  # noqa: E402

KERNELS = ["k_stream_pass",   # (mode 10: the probe renders no mode-8 frame)
           "k_mboit_stream_pass", "k_ppll_raster_prism", "k_ppll_shade_prism"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atomic_loop_c4_pmc.json"))
    args = ap.parse_args()
    disp = collections.OrderedDict()
    for r in csv.DictReader(open(args.csv)):
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        d = disp.setdefault(int(r["Dispatch_Id"]), {"kernel": name})
        d[r["Counter_Name"]] = float(r["Counter_Value"])
        d["us"] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    groups = collections.OrderedDict()
    al64 = [d for d in disp.values() if d["kernel"] == "k_stream_pass"]
    per_k = len(al64) // 3
    for i, d in enumerate(al64):
        groups.setdefault("k_stream_pass<10> K=%d" % (4, 8, 16)[min(i // max(per_k, 1), 2)], []).append(d)
    mboit = [d for d in disp.values() if d["kernel"] == "k_mboit_stream_pass"]
    for i, d in enumerate(mboit):
        groups.setdefault("k_mboit_stream_pass N=4 %s" % ("moments", "colours")[i % 2], []).append(d)
    for d in disp.values():
        if d["kernel"] in ("k_ppll_raster_prism", "k_ppll_shade_prism"):
            groups.setdefault(d["kernel"], []).append(d)
    result = {"source_sha": build.source_sha(), "collected_with": "rocprofv3 --pmc TCC_EA0_ATOMIC_sum TCC_REQ_sum --kernel-trace -- "
              "python tools/probe_atomic_loop.py --frames 3 --warmup 1", "kernels": {}}
    for name, ds in groups.items():
        a = float(np.median([d["TCC_EA0_ATOMIC_sum"] for d in ds]))
        us = float(np.median([d["us"] for d in ds]))
        result["kernels"][name] = {"dispatches": len(ds), "TCC_EA0_ATOMIC_sum": a, "TCC_REQ_sum": float(np.median([d["TCC_REQ_sum"] for d in ds])),
                                   "time_us": us, "atomic_requests_per_s": a / (us * 1e-6), "atomic_TB_per_s_at_64B": a * 64 / (us * 1e-6) / 1e12}
        print(name, json.dumps(result["kernels"][name]))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
