"""same_amd.sliding_window_scores against what a study did before it (same_amd/scores.py, csrc/window_score.hip): BASELINE
cfg 5's generator (1M cells, windows 1200 / overlap 300, radius 25, knn 8, fp32 costs) with the SIX type-matrix variants of
tools/variants_profile.py, every result reduced to the numbers the reference's figure notebooks read.  The moving frame's triangulation
(scipy, the whole frame) is made once, outside every timed region.  Three things are timed, each the best of --passes after an untimed
pass, in one job, on the default route (Qhull helpers) and with the triangulations given (windows.TriangulationCache):
  (a) what the package offered before: sliding_window_variants(merge=True), then per table check_alignment at kNN=1 on SAME_X = ref_X and
      check_triangle_violations, as examples/heart/reproduce_figures.ipynb calls them -- split into the pass and the scoring;
  (b) sliding_window_scores(tables=False);
  (c) sliding_window_scores(tables=True).
The records of (a), (b) and (c) must be identical (asserted).  The score call's GPU time per set is read from the context's event timer
around the library call.  ONE JSON line, appended to --out (default profiles/scores_profile.jsonl).
Usage: python3 tools/scores_profile.py [--cells N] [--passes 3] [--workers N] [--routes qhull,given] [--out ...]"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import same_amd                                          # noqa: E402
from same_amd import windows as W                        # noqa: E402
from variants_profile import BASE, inputs                # noqa: E402

CID = "Cell_Num_Old"
SCORE_MS = []


def time_score_calls():
    """every same_merge_acc_score call between two events of its context's stream"""
    inner = W.MergeAccumulator.score

    def score(self, *a, **k):
        self.ctx.timer_start()
        out = inner(self, *a, **k)
        SCORE_MS.append(self.ctx.timer_stop())
        return out

    W.MergeAccumulator.score = score


def best_of(run, passes):
    """-> (result of the last pass, [seconds of each timed pass]) after an untimed pass"""
    out, secs = run(), []
    for _ in range(passes):
        t0 = time.perf_counter()
        out = run()
        secs.append(time.perf_counter() - t0)
    return out, secs


def notebook_record(table, r_df, m_df, carrier):
    """one table scored as the notebook scores it -> the record sliding_window_scores gives"""
    rows = table[f"Aligned_{CID}"].to_numpy()                                  # (the generator's ids are the row numbers)
    query = table.assign(SAME_X=table["ref_X"], SAME_Y=table["ref_Y"], cell_type=m_df["cell_type"].to_numpy()[rows])
    checked, _mean = same_amd.check_alignment(query, r_df, xcol="SAME_X", ycol="SAME_Y", ctype_col="cell_type", kNN=1)
    query.index = rows
    _df, stats = same_amd.check_triangle_violations(query, carrier, aligned_id_col=f"Aligned_{CID}", ref_id_col=f"Ref_{CID}",
                                                    mapped_x_col="ref_X", mapped_y_col="ref_Y", cell_type_col="cell_type",
                                                    ignore_same_type_triangles=True, verbose=False)
    return same_amd.record_from_counts({"matched": len(table), "type_matches": int(checked["_1NN_match"].sum()),
                                        **{k: int(stats[k]) for k in ("total_triangles", "triangles_with_all_matched",
                                                                      "triangles_same_type_skipped", "triangles_flipped",
                                                                      "nodes_in_violating_triangles")}})


def records_of(scores):
    bits = lambda col: [struct.pack("<d", float(v)) if col.dtype.kind == "f" else int(v) for v in col]
    return {k: bits(scores[k]) for k in scores.columns}


def main():
    import types

    import pandas as pd
    from scipy.spatial import Delaunay

    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--routes", default="qhull,given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_profile.jsonl"))
    args = ap.parse_args()

    r_df, m_df, cols, variants = inputs(args.cells)
    assert np.array_equal(m_df[CID].to_numpy(), np.arange(len(m_df))) and np.array_equal(r_df[CID].to_numpy(), np.arange(len(r_df)))
    rxy = r_df[["X", "Y"]].to_numpy()
    assert len(np.unique(rxy, axis=0)) == len(rxy)             # a matched cell's nearest template cell is its own reference cell
    r_df = r_df.assign(SAME_X=r_df["X"], SAME_Y=r_df["Y"])
    t0 = time.perf_counter()
    tris = Delaunay(m_df[["X", "Y"]].to_numpy()).simplices.astype(np.int64)
    tri_s = time.perf_counter() - t0
    carrier = types.SimpleNamespace(metacell_df=m_df, metacell_delaunay=tris)
    time_score_calls()
    line = {"tool": "scores_profile", "workload": "cfg5_generator_six_type_variants", "cells": args.cells, "passes": args.passes,
            "cpus": len(os.sched_getaffinity(0)), "variants": len(variants), "score_triangles": len(tris),
            "score_triangulation_s": round(tri_s, 3), "routes": {}}
    with same_amd.resident_frames(r_df, m_df) as frames:
        for route in args.routes.split(","):
            tri = W.TriangulationCache() if route == "given" else None
            kw = dict(workers=args.workers, optim_params=dict(BASE), triangulator=tri)
            split = {"pass": [], "scoring": []}

            def before():
                t0 = time.perf_counter()
                tables = same_amd.sliding_window_variants(frames, m_df, variants, cols, merge=True, **kw)
                t1 = time.perf_counter()
                recs = [notebook_record(t, r_df, m_df, carrier) for t in tables]
                split["pass"].append(t1 - t0)
                split["scoring"].append(time.perf_counter() - t1)
                return pd.DataFrame([{"variant": v, "set": 0, **rec} for v, rec in enumerate(recs)])

            scored = lambda tables: same_amd.sliding_window_scores(frames, m_df, cols, type_variants=variants, score_delaunay=tris,
                                                                   tables=tables, **kw)
            a, a_s = best_of(before, args.passes)
            del SCORE_MS[:]
            b, b_s = best_of(lambda: scored(False), args.passes)
            score_ms = list(SCORE_MS)
            (c, _tables), c_s = best_of(lambda: scored(True), args.passes)
            same = records_of(a) == records_of(b) == records_of(c) and list(a.columns) == list(b.columns) == list(c.columns)
            timed = split["pass"][1:], split["scoring"][1:]
            assert len(score_ms) == len(variants) * (args.passes + 1)
            line["routes"][route] = {
                "records_identical": bool(same),
                "a_variants_then_notebook_s": round(min(a_s), 4), "a_pass_s": round(min(timed[0]), 4), "a_pass_s_all": [round(s, 4) for s in timed[0]],
                "a_scoring_s": round(min(timed[1]), 4),
                "b_scores_s": round(min(b_s), 4), "b_scores_s_all": [round(s, 4) for s in b_s],
                "c_scores_with_tables_s": round(min(c_s), 4),
                "b_over_a": round(min(b_s) / min(a_s), 4), "b_over_a_pass": round(min(b_s) / min(timed[0]), 4),
                "score_call_gpu_ms_per_set": round(float(np.median(score_ms[len(variants):])), 4),
                "score_call_gpu_ms_first_pass": [round(m, 4) for m in score_ms[:len(variants)]],
                "accuracy": [round(float(v), 3) for v in b["accuracy"]], "violations": [round(float(v), 3) for v in b["violations"]]}
            if not same:
                print(json.dumps(line), flush=True)
                sys.exit(f"route {route}: the records of (a), (b) and (c) differ")
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
