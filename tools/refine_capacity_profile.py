"""optim_params["hip_refine"] = "capacity" against "local" (csrc/refine.hip) through same_amd.sliding_window_incumbent on two workloads,
in one process, and ONE JSON line per workload (appended to --out):

  cfg5   BASELINE cfg 5's section (bench_cfg5's parameters: windows 1200 / overlap 300, radius 25, knn 8, float costs) with
         max_matches = 2, on resident frames (the device route), merge=True;
  meta   the same kind of section, smaller, with BOTH sides collapsed into metacells by greedy_triangle_collapse with MS = 3 and
         ref_metacell_match_multiplier = MS, as the reference's tongue / heart / LUAD flows do (MetaCell inputs: the general route).

Modes: "local", "capacity", and "capacity" with penalty_coeff 10 ("capacity_pc10").  Per mode: windows/s (best of --passes, after an untimed pass), the windows' summed model objective before and after the search
(mip_objective_start, mip_objective; the penalty_coeff term included), summed ref_extra_matches (sum_j max(0, count_j - 1)), the
moving size left unmatched by the merged table, and rounds per window (mean, max).
Usage: python3 tools/refine_capacity_profile.py [--cells 1000000] [--meta-cells 100000] [--passes 2] [--only cfg5|meta] [--out ...]"""
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


def measure(run, total_size, passes):
    """-> {windows_per_s, objective_start, objective, ref_extra_matches, unmatched_size, rounds_mean, rounds_max, windows}"""
    table, stats = run()                                 # untimed: helpers, states
    best = float("inf")
    for _ in range(passes):
        t0 = time.perf_counter()
        table, stats = run()
        best = min(best, time.perf_counter() - t0)
    rounds = np.array([s["refine_rounds"] for s in stats])
    return {"windows": len(stats), "windows_per_s": round(len(stats) / best, 1),
            "objective_start": float(sum(s["mip_objective_start"] for s in stats)),
            "objective": float(sum(s["mip_objective"] for s in stats)),
            "ref_extra_matches": int(sum(s.get("ref_extra_matches", 0) for s in stats)),
            "unmatched_size": float(total_size - table["size"].to_numpy(dtype=np.float64).sum()),
            "rounds_mean": round(float(rounds.mean()), 3), "rounds_max": int(rounds.max())}


def modes(op):
    """"local", "capacity" at the default penalty_coeff (100 = no_match_penalty: a size-1 cell never gains by sharing a reference),
    and "capacity" at penalty_coeff 10"""
    return (("local", dict(op, hip_refine="local")), ("capacity", dict(op, hip_refine="capacity")),
            ("capacity_pc10", dict(op, hip_refine="capacity", penalty_coeff=10)))


def cfg5(args):
    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10,
              max_matches=2)
    line = {"tool": "refine_capacity_profile", "workload": "cfg5_max_matches_2", "cells": args.cells,
            "cpus": len(os.sched_getaffinity(0))}
    total = float(m_df["size"].to_numpy(dtype=np.float64).sum())
    with same_amd.resident_frames(r_df, m_df) as res:
        for name, o in modes(op):
            run = lambda: same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(o), merge=True, return_stats=True)
            line[name] = measure(run, total, args.passes)
    return line


def meta(args):
    from same_amd.metacell_utils import greedy_triangle_collapse

    T = 8
    ref = synth.make_cells(args.meta_cells, T, seed=2)
    mov = synth.make_jittered(ref, seed=3)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    t0 = time.perf_counter()
    kw = dict(original_idx_col="Cell_Num_Old", max_metacell_size=MS, r_max=25, min_angle_deg=15, return_object=True, verbose=False)
    mc_m, mc_r = greedy_triangle_collapse(m_df, **kw), greedy_triangle_collapse(r_df, **kw)
    collapse_s = time.perf_counter() - t0
    op = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, cell_id_col="metacell_id",
              ref_metacell_match_multiplier=MS)
    line = {"tool": "refine_capacity_profile", "workload": "metacell_MS3", "cells": args.meta_cells,
            "metacells": [len(mc_r.metacell_df), len(mc_m.metacell_df)], "collapse_s": round(collapse_s, 1),
            "cpus": len(os.sched_getaffinity(0))}
    total = float(mc_m.metacell_df["size"].to_numpy(dtype=np.float64).sum())
    for name, o in modes(op):
        run = lambda: same_amd.sliding_window_incumbent(mc_r, mc_m, commonCT=cols, optim_params=dict(o), merge=True, return_stats=True)
        line[name] = measure(run, total, args.passes)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--meta-cells", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--only", choices=("cfg5", "meta"), default=None)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    for name, fn in (("cfg5", cfg5), ("meta", meta)):
        if args.only not in (None, name):
            continue
        line = fn(args)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
