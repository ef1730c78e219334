"""same_amd.sliding_window_scores(unpack=...) against what a MetaCell study did before it (same_amd/scores.py, csrc/window_unpack.hip,
DESIGN §5.15), at a LUAD-like shape: about 100k x 100k seeded cells, both sides collapsed at max_metacell_size=3, r_max=40,
min_angle_deg=10 (tools/sweep_profile.py's MetaCell recipe), the six delaunay_penalty sets of the LUAD sweep (dp = 0, 1, 5, 10, 25, 50),
hip_caller_delaunay="device", one resident_frames object for everything.  Per strategy two things are timed, each the best of --passes
after an untimed pass:
  (a) the path that exists without the feature: sliding_window_scores(tables=True), then per table score_unpacked's two steps --
      unpack_metacell_matches and the two label maps, as examples/luad/reproduce_figures.ipynb cell 12 does them -- split into the pass
      and the unpacking;
  (b) sliding_window_scores(unpack=strategy), no tables.
The records of (a) and (b) must be identical (asserted).  The unpack call's GPU time per set is read from the context's event timer
around the library call.  ONE JSON line, appended to --out (default profiles/unpack_scores_profile.jsonl).
Usage: python3 tools/unpack_scores_profile.py [--cells N] [--passes 3] [--workers N] [--out ...]"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import same_amd                                          # noqa: E402
from same_amd import synth                               # noqa: E402
from same_amd import windows as W                        # noqa: E402

UNPACK_MS = []
SETS = [{"knn": 8, "hip_refine": "local", "delaunay_penalty": p} for p in (0, 1, 5, 10, 25, 50)]
OP = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, hip_cost_dtype="float32",
          hip_caller_delaunay="device")


def time_unpack_calls():
    """every same_merge_acc_unpack call between two events of its context's stream"""
    inner = W.MergeAccumulator.unpack

    def unpack(self, *a, **k):
        self.ctx.timer_start()
        out = inner(self, *a, **k)
        UNPACK_MS.append(self.ctx.timer_stop())
        return out

    W.MergeAccumulator.unpack = unpack


def best_of(run, passes):
    """-> (result of the last pass, [seconds of each timed pass]) after an untimed pass"""
    out, secs = run(), []
    for _ in range(passes):
        t0 = time.perf_counter()
        out = run()
        secs.append(time.perf_counter() - t0)
    return out, secs


def records_of(scores):
    bits = lambda col: [struct.pack("<d", float(v)) if col.dtype.kind == "f" else int(v) for v in col]
    return {k: bits(scores[k]) for k in scores.columns}


def main():
    import pandas as pd

    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_scores_profile.jsonl"))
    args = ap.parse_args()

    T = 8
    cells = synth.make_cells(args.cells, T, seed=0)
    r_c, a_c = synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=1))
    a_c["Cell_Num_Old"] = np.arange(len(a_c))
    labels = a_c["cell_type"].to_numpy().copy()          # one label in nine changed, or every cell would sit on a cell of its label
    labels[::9] = np.roll(labels, 1)[::9]
    a_c["cell_type"] = labels
    t0 = time.perf_counter()
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    mc_r, mc_a = collapse(r_c), collapse(a_c)
    collapse_s = time.perf_counter() - t0
    cols = synth.type_columns(T)
    time_unpack_calls()
    line = {"tool": "unpack_scores_profile", "workload": "luad_like_metacells_ms3_delaunay_penalty_sweep", "cells": [len(r_c), len(a_c)],
            "metacells": [len(mc_r.metacell_df), len(mc_a.metacell_df)], "sets": len(SETS), "passes": args.passes,
            "cpus": len(os.sched_getaffinity(0)), "collapse_s": round(collapse_s, 3), "strategies": {}}
    kw = dict(param_sets=SETS, optim_params=dict(OP), workers=args.workers)
    all_same = True
    with same_amd.resident_frames(mc_r, mc_a) as frames:
        for strategy in ("distribute", "nearest"):
            split = {"pass": [], "unpacking": []}

            def before():
                t0 = time.perf_counter()
                scores, tables = same_amd.sliding_window_scores(frames, mc_a, cols, tables=True, **kw)
                t1 = time.perf_counter()
                recs = [same_amd.score_unpacked(table, mc_r, mc_a, strategy)[0] for table in tables[0]]
                split["pass"].append(t1 - t0)
                split["unpacking"].append(time.perf_counter() - t1)
                return pd.concat([scores, pd.DataFrame(recs)], axis=1)

            a, a_s = best_of(before, args.passes)
            del UNPACK_MS[:]
            b, b_s = best_of(lambda: same_amd.sliding_window_scores(frames, mc_a, cols, unpack=strategy, **kw), args.passes)
            unpack_ms = list(UNPACK_MS)
            assert len(unpack_ms) == len(SETS) * (args.passes + 1), "the device did not unpack every result"
            same = records_of(a) == records_of(b) and list(a.columns) == list(b.columns)
            all_same = all_same and same
            timed = split["pass"][1:], split["unpacking"][1:]
            line["strategies"][strategy] = {
                "records_identical": bool(same),
                "a_tables_then_score_unpacked_s": round(min(a_s), 4), "a_pass_with_tables_s": round(min(timed[0]), 4),
                "a_unpacking_s": round(min(timed[1]), 4), "a_s_all": [round(s, 4) for s in a_s],
                "b_scores_unpack_s": round(min(b_s), 4), "b_s_all": [round(s, 4) for s in b_s],
                "b_over_a": round(min(b_s) / min(a_s), 4),
                "unpack_call_gpu_ms_per_set": round(float(np.median(unpack_ms[len(SETS):])), 4),
                "unpack_call_gpu_ms_first_pass": [round(m, 4) for m in unpack_ms[:len(SETS)]],
                "matched": [int(v) for v in b["matched"]], "cells_matched": [int(v) for v in b["cells_matched"]],
                "cell_accuracy": [round(float(v), 3) for v in b["cell_accuracy"]]}
    print(json.dumps(line), flush=True)
    if not all_same:
        sys.exit("the records of (a) and (b) differ")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
