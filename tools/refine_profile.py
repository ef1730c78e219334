"""BASELINE cfg 5 (bench_cfg5's workload and parameters: a 1M-cell section, windows 1200 / overlap 300, radius 25, knn 8, float costs)
through same_amd.sliding_window_incumbent(merge=True) with and without optim_params["hip_refine"] = "local" (csrc/refine.hip), for both
incumbents, in one process on one set of resident frames.  Prints ONE JSON line and appends it to --out: windows/s with and without the
search on the default (Qhull) route and with the triangulations given (windows.TriangulationCache, filled by an untimed pass), best of
--passes; the finish call's wall time per batch of 8 windows; per incumbent the windows' summed lazy-model objective before and after the
search (mip_objective_start, mip_objective), summed `flipped` without and with it, rounds per window (mean, max), moves, and the windows
that stopped at the round cap.
Usage: python3 tools/refine_profile.py [--cells 1000000] [--passes 2] [--rounds 32] [--only-refine] [--tag ...] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import same_amd                                          # noqa: E402
from same_amd import _trace, synth                       # noqa: E402
from same_amd.windows import TriangulationCache          # noqa: E402

FINISH = "filter + signs + incumbent + sweeps (device)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=None, help="hip_refine_rounds (default: the library's)")
    ap.add_argument("--only-refine", action="store_true", help="one refining default-route pass per incumbent (kernel traces)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_refine_profile.jsonl"))
    args = ap.parse_args()
    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)
    R = dict(hip_refine="local") if args.rounds is None else dict(hip_refine="local", hip_refine_rounds=args.rounds)
    line = {"tool": "refine_profile", "tag": args.tag, "cells": args.cells, "cpus": len(os.sched_getaffinity(0)), "refine": R}
    _trace.enable(True)
    with same_amd.resident_frames(r_df, m_df) as res:
        cache = TriangulationCache()
        for inc in ("greedy", "assignment"):
            if args.only_refine:
                _t, stats = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op, hip_incumbent=inc, **R),
                                                              merge=True, return_stats=True)
                line[f"{inc}_windows"] = len(stats)
                continue
            for name, extra in (("plain", {}), ("refine", R)):
                o = dict(op, hip_incumbent=inc, **extra)
                for route, tri in (("default", None), ("tris_given", cache)):
                    run = lambda: same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(o), merge=True,
                                                                    return_stats=True, triangulator=tri)
                    _table, stats = run()                        # untimed: helpers, states, the cache
                    best, finish = float("inf"), None
                    for _ in range(args.passes):
                        _trace.reset()
                        t0 = time.perf_counter()
                        _table, stats = run()
                        dt = time.perf_counter() - t0
                        if dt < best:
                            best, finish = dt, _trace.report().get(FINISH, (0, 0.0))
                    line[f"{inc}_{name}_{route}_windows_per_s"] = round(len(stats) / best, 1)
                    line[f"{inc}_{name}_{route}_finish_ms_per_batch8"] = round(finish[1] * 1e3 / max(1, len(stats) / 8), 3)
                line["windows"] = len(stats)
                line[f"{inc}_{name}_flipped"] = int(sum(s["flipped"] for s in stats))
                if name == "refine":
                    rounds = np.array([s["refine_rounds"] for s in stats])
                    line[f"{inc}_objective_start"] = float(sum(s["mip_objective_start"] for s in stats))
                    line[f"{inc}_objective_refined"] = float(sum(s["mip_objective"] for s in stats))
                    line[f"{inc}_objective_relative_drop"] = 1.0 - line[f"{inc}_objective_refined"] / line[f"{inc}_objective_start"]
                    line[f"{inc}_rounds_mean"], line[f"{inc}_rounds_max"] = float(rounds.mean()), int(rounds.max())
                    line[f"{inc}_moves"] = int(sum(s["refine_moves"] for s in stats))
                    line[f"{inc}_windows_at_cap"] = int(sum(1 for s in stats if not s["refine_settled"]))
            line[f"{inc}_refine_vs_plain_default"] = round(line[f"{inc}_refine_default_windows_per_s"] /
                                                           line[f"{inc}_plain_default_windows_per_s"], 3)
    print(json.dumps(line), flush=True)
    if not args.only_refine and args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
