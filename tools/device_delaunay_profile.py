"""BASELINE cfg 5 (bench_cfg5's workload and parameters: a 1M-cell section, windows 1200 / overlap 300, radius 25, knn 8, float costs)
through same_amd.sliding_window_incumbent(merge=True) on the three triangulation routes of optim_params["hip_delaunay"] -- "qhull"
(the default: scipy in helper processes), "native" (csrc/delaunay.cpp on host threads) and "device" (csrc/delaunay_dev.hip) -- in one
process, on one set of resident frames.  One JSON line per route: windows/s (best of --passes timed passes after one untimed), the
windows refused / re-finished with scipy, the share of the pass spent in the device triangulation call (kernels + its one wait, from
the stage timer), and whether the merged table is identical to the qhull route's.
Usage: python3 tools/device_delaunay_profile.py [--cells 1000000] [--routes qhull,native,device] [--passes 3] [--workers 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import same_amd                                    # noqa: E402
from same_amd import _trace, delaunay, synth       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--routes", default="qhull,native,device")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    r_df["Cell_Num_Old"], m_df["Cell_Num_Old"] = np.arange(len(r_df)), np.arange(len(m_df))
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)
    cpus = len(os.sched_getaffinity(0))
    from same_amd.incumbent import _default_workers

    n_workers = args.workers or _default_workers()
    _trace.enable(True)
    with same_amd.resident_frames(r_df, m_df) as res:
        want = None
        for route in args.routes.split(","):
            def one(route=route):
                return same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op, hip_delaunay=route), merge=True,
                                                         return_stats=True, workers=args.workers)
            table, stats = one()                     # untimed: helpers, threads and window states start here
            if route == "qhull":
                want = table
            native = delaunay.shared() if route == "native" else None
            counts0 = (native.submitted, native.asked_qhull) if native else None
            best, dev_share, refused, refinished = float("inf"), None, 0, 0
            for _ in range(args.passes):
                _trace.reset()
                t0 = time.perf_counter()
                table, stats = one()
                dt = time.perf_counter() - t0
                if dt < best:
                    best = dt
                    rep = _trace.report()
                    dev = rep.get("triangulate (device)", (0, 0.0))[1]
                    dev_share = dev / n_workers / dt if route == "device" else None     # (the stage timer sums over the workers)
                    if route == "device":
                        st = delaunay.last_device_stats()
                        refused, refinished = st["refused"], st["refinished"]
            if native:
                refused = (native.asked_qhull - counts0[1]) // (args.passes)
            line = {"tool": "device_delaunay_profile", "tag": args.tag, "route": route, "cells": args.cells, "cpus": cpus,
                    "workers": n_workers, "windows": len(stats), "pass_ms": round(best * 1e3, 2), "windows_per_s": round(len(stats) / best, 1),
                    "refused": refused, "refinished": refinished,
                    "device_triangulation_share": None if dev_share is None else round(dev_share, 4),
                    "same_table_as_qhull": None if want is None else bool(table.equals(want))}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
