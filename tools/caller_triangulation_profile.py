"""optim_params["hip_caller_delaunay"] = "device" against the general route on MetaCell inputs (csrc/window_caller.hip):
BASELINE cfg 5's generator (bench_cfg5's parameters: windows 1200 / overlap 300, radius 25, knn 8), BOTH sides collapsed by
greedy_triangle_collapse with max_metacell_size = 3 and handed to same_amd.sliding_window_incumbent as MetaCell objects, the way every
run the reference ships does (run_same.sh / run_robustness.sh).  Both routes in one job and one process: an untimed pass each, then the
best of --passes; the two tables must be identical (checked, and said in the record).  ONE JSON line, appended to --out (default
profiles/caller_triangulation_profile.jsonl): windows, metacells, windows/s of either route, their ratio, and with --merge the same for merge=True.
Usage: python3 tools/caller_triangulation_profile.py [--cells 1000000] [--passes 3] [--workers N] [--merge] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import same_amd                                          # noqa: E402
from same_amd import synth                               # noqa: E402

MS = 3


def timed(run, passes):
    """-> (table, stats, best seconds of `passes` after an untimed pass)"""
    table, stats = run()
    best = float("inf")
    for _ in range(passes):
        t0 = time.perf_counter()
        table, stats = run()
        best = min(best, time.perf_counter() - t0)
    return table, stats, best


def identical(a, b):
    if list(a.columns) != list(b.columns) or len(a) != len(b):
        return False
    return all(np.array_equal(a[c].to_numpy(), b[c].to_numpy()) for c in a.columns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--merge", action="store_true", help="also time both routes with merge=True")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caller_triangulation_profile.jsonl"))
    args = ap.parse_args()
    from same_amd.metacell_utils import greedy_triangle_collapse

    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    t0 = time.perf_counter()
    kw = dict(original_idx_col="Cell_Num_Old", max_metacell_size=MS, r_max=25, min_angle_deg=15, return_object=True, verbose=False)
    mc_m, mc_r = greedy_triangle_collapse(m_df, **kw), greedy_triangle_collapse(r_df, **kw)
    collapse_s = time.perf_counter() - t0
    op = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, cell_id_col="metacell_id",
              ref_metacell_match_multiplier=MS)
    line = {"tool": "caller_triangulation_profile", "workload": "cfg5_generator_metacell_MS3", "cells": args.cells,
            "metacells": [len(mc_r.metacell_df), len(mc_m.metacell_df)], "triangles": int(len(mc_m.metacell_delaunay)),
            "collapse_s": round(collapse_s, 1), "passes": args.passes, "cpus": len(os.sched_getaffinity(0))}
    for tag, extra in (("", {}),) + ((("merge_", {"merge": True}),) if args.merge else ()):
        general = lambda: same_amd.sliding_window_incumbent(mc_r, mc_m, commonCT=cols, optim_params=dict(op), return_stats=True, **extra)
        device = lambda: same_amd.sliding_window_incumbent(mc_r, mc_m, commonCT=cols, optim_params=dict(op, hip_caller_delaunay="device"),
                                                           return_stats=True, _route="device", workers=args.workers, **extra)
        g_table, g_stats, g_s = timed(general, args.passes)
        d_table, d_stats, d_s = timed(device, args.passes)
        same = identical(g_table, d_table) and [s["matched"] for s in g_stats] == [s["matched"] for s in d_stats]
        line.update({tag + "windows": len(g_stats), tag + "rows": len(g_table), tag + "tables_identical": bool(same),
                     tag + "general_windows_per_s": round(len(g_stats) / g_s, 1), tag + "device_windows_per_s": round(len(d_stats) / d_s, 1),
                     tag + "device_over_general": round(g_s / d_s, 2)})
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if not all(v for k, v in line.items() if k.endswith("tables_identical")):
        sys.exit("the two routes' tables differ")


if __name__ == "__main__":
    main()
