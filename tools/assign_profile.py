"""BASELINE cfg 5 (bench_cfg5's workload and parameters: a 1M-cell section, windows 1200 / overlap 300, radius 25, knn 8, float costs)
through same_amd.sliding_window_incumbent(merge=True) with the greedy start (the default) and with optim_params["hip_incumbent"] =
"assignment" (csrc/assign.hip), in one process on one set of resident frames.  Prints ONE JSON line: windows/s of both incumbents on the
default (Qhull) route and with the triangulations given (windows.TriangulationCache, filled by an untimed pass), best of --passes; the
finish call's wall time per batch of 8 windows for both (the stage timer, summed over workers: the difference is what the assignment
adds per batch); the assignment's searches and fallbacks; the windows' summed objective for both and the relative gap.  The greedy
objective is the same sum over the greedy matching of each window's pairs (the general route's per-window problems).
Usage: python3 tools/assign_profile.py [--cells 1000000] [--passes 2] [--tag ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import same_amd                                          # noqa: E402
from same_amd import _trace, ops, synth                  # noqa: E402
from same_amd.windows import TriangulationCache          # noqa: E402

FINISH = "filter + signs + incumbent + sweeps (device)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)
    line = {"tool": "assign_profile", "tag": args.tag, "cells": args.cells, "cpus": len(os.sched_getaffinity(0))}
    _trace.enable(True)
    with same_amd.resident_frames(r_df, m_df) as res:
        cache = TriangulationCache()
        for name, mode in (("greedy", "greedy"), ("assignment", "assignment")):
            o = dict(op, hip_incumbent=mode)
            for route, tri in (("default", None), ("tris_given", cache)):
                run = lambda: same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(o), merge=True, return_stats=True,
                                                                triangulator=tri)
                table, stats = run()                             # untimed: helpers, states, the cache
                best, finish = float("inf"), None
                for _ in range(args.passes):
                    _trace.reset()
                    t0 = time.perf_counter()
                    table, stats = run()
                    dt = time.perf_counter() - t0
                    if dt < best:
                        best, finish = dt, _trace.report().get(FINISH, (0, 0.0))
                line[f"{name}_{route}_windows_per_s"] = round(len(stats) / best, 1)
                line[f"{name}_{route}_finish_ms_per_batch8"] = round(finish[1] * 1e3 / max(1, len(stats) / 8), 3)
            line["windows"] = len(stats)
            if mode == "assignment":
                line["assignment_fallbacks"] = int(sum(s["fallback"] for s in stats))
                line["assignment_objective"] = float(sum(s["objective"] for s in stats))
    # the greedy objective of the same windows, from the general route's per-window problems
    seen, inner = [], ops.sparse_assign

    def spy(pairs, costs, unmatched, n_a, n_r, ctx=None):
        out = inner(pairs, costs, unmatched, n_a, n_r, ctx=ctx)
        prefer = ops.pair_rowmin(pairs, costs, n_a, ctx=ctx) < unmatched
        greedy, _r = ops.greedy_match(pairs, costs, n_a, n_r, prefer, ctx=ctx)
        seen.append((ops.assign_objective(greedy, costs, unmatched), out[1]["objective"], out[1]["rounds"]))
        return out

    ops.sparse_assign = spy
    try:
        t0 = time.perf_counter()
        same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op, hip_incumbent="assignment"), _route="general")
        line["general_route_s"] = round(time.perf_counter() - t0, 2)
    finally:
        ops.sparse_assign = inner
    g, a, r = (np.array(x, dtype=np.float64) for x in zip(*seen))
    line["greedy_objective"], line["assignment_objective_general"] = float(g.sum()), float(a.sum())
    line["relative_gap"] = float((g.sum() - a.sum()) / g.sum())
    line["searches_per_window_mean"], line["searches_per_window_max"] = float(r.mean()), int(r.max())
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
