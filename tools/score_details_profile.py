"""same_amd.sliding_window_score_details against what a study does without it (same_amd/score_details.py, csrc/window_score_detail.hip,
DESIGN §5.16): BASELINE cfg 5's generator (1M cells, windows 1200 / overlap 300, radius 25, knn 8, fp32 costs) with the SIX type-matrix
variants of tools/variants_profile.py, every result broken down by a 4 x 4 grid of the moving frame, by label pair and by type rank
(top_k = 1, 2, 3).  The moving frame's triangulation (scipy, the whole frame) is made once, outside every timed region.  Timed in one job,
with the windows' triangulations given (windows.TriangulationCache):
  (a) the path that exists without the feature: sliding_window_scores(tables=True), then score_table_details per table -- split into the
      pass and the host work, --host-passes times after the device is warm;
  (b) sliding_window_score_details, the best of --passes after an untimed pass.
The frames of (a) and (b) must be identical (asserted).  The detail call's and the score call's GPU time per set are read from the
context's event timer around the two library calls of the same run.  ONE JSON line, appended to --out (default
profiles/score_details_profile.jsonl).
Usage: python3 tools/score_details_profile.py [--cells N] [--passes 3] [--host-passes 1] [--workers N] [--out ...]"""
import argparse
import json
import os
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
TOP_K = (1, 2, 3)
CALL_MS = {"score": [], "score_detail": []}


def time_calls():
    """every same_merge_acc_score and same_merge_acc_score_detail call between two events of its context's stream"""
    for name in CALL_MS:
        def timed(self, *a, _inner=getattr(W.MergeAccumulator, name), _into=CALL_MS[name], **k):
            self.ctx.timer_start()
            out = _inner(self, *a, **k)
            _into.append(self.ctx.timer_stop())
            return out

        setattr(W.MergeAccumulator, name, timed)


def grid_groups(frame, n=4):
    """the cell of an n x n grid over the frame's extent each row lies in, as a label"""
    cell = lambda v: np.minimum(((v - v.min()) / (v.max() - v.min()) * n).astype(np.int64), n - 1)
    cx, cy = cell(frame["X"].to_numpy()), cell(frame["Y"].to_numpy())
    return np.array([f"{x}{y}" for x, y in zip(cx.tolist(), cy.tolist())], dtype=object)


def identical(got, per_table, n_sets=1):
    """the study's frames against the tables' own, frame for frame (values, dtypes, order)"""
    import pandas as pd

    try:
        for q, want in enumerate(per_table):
            v, s = q // n_sets, q % n_sets
            rows = lambda f: f[(f["variant"] == v) & (f["set"] == s)].drop(columns=["variant", "set"]).reset_index(drop=True)
            pd.testing.assert_frame_equal(rows(got.scores), want.scores, check_exact=True)
            pd.testing.assert_frame_equal(got.confusion.loc[(v, s)], want.confusion, check_exact=True)
            for what in ("groups", "cross", "top_k"):
                pd.testing.assert_frame_equal(rows(getattr(got, what)), getattr(want, what), check_exact=True)
    except AssertionError as e:
        print(e, file=sys.stderr)
        return False
    return True


def main():
    from scipy.spatial import Delaunay

    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=1)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_details_profile.jsonl"))
    args = ap.parse_args()

    r_df, m_df, cols, variants = inputs(args.cells)
    groups = grid_groups(m_df)
    t0 = time.perf_counter()
    tris = Delaunay(m_df[["X", "Y"]].to_numpy()).simplices.astype(np.int64)
    tri_s = time.perf_counter() - t0
    time_calls()
    line = {"tool": "score_details_profile", "workload": "cfg5_generator_six_type_variants", "cells": args.cells, "passes": args.passes,
            "host_passes": args.host_passes, "cpus": len(os.sched_getaffinity(0)), "variants": len(variants), "groups": len(set(groups)),
            "top_k": list(TOP_K), "score_triangles": len(tris), "score_triangulation_s": round(tri_s, 3)}
    with same_amd.resident_frames(r_df, m_df) as frames:
        kw = dict(workers=args.workers, optim_params=dict(BASE), triangulator=W.TriangulationCache(), type_variants=variants,
                  score_delaunay=tris)
        device = lambda: same_amd.sliding_window_score_details(frames, m_df, cols, group_by=groups, top_k=TOP_K, **kw)
        got = device()                                  # untimed: buffers grown, the resident objects made
        del CALL_MS["score"][:], CALL_MS["score_detail"][:]
        b_s = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            got = device()
            b_s.append(time.perf_counter() - t0)
        assert len(CALL_MS["score_detail"]) == len(CALL_MS["score"]) == len(variants) * args.passes
        detail_ms, score_ms = list(CALL_MS["score_detail"]), list(CALL_MS["score"])
        a_pass, a_host, per_table = [], [], None
        for _ in range(args.host_passes):
            t0 = time.perf_counter()
            _scores, tables = same_amd.sliding_window_scores(frames, m_df, cols, tables=True, **kw)
            t1 = time.perf_counter()
            per_table = [same_amd.score_table_details(t, r_df, m_df, cell_id_col=CID, commonCT=cols, group_by=groups, top_k=TOP_K,
                                                      score_delaunay=tris) for per_set in tables for t in per_set]
            a_pass.append(t1 - t0)
            a_host.append(time.perf_counter() - t1)
        same = identical(got, per_table)
        a = min(p + h for p, h in zip(a_pass, a_host))
        line.update({"records_identical": bool(same),
                     "a_scores_with_tables_then_table_details_s": round(a, 4), "a_pass_s": round(min(a_pass), 4),
                     "a_table_details_s": round(min(a_host), 4),
                     "b_score_details_s": round(min(b_s), 4), "b_score_details_s_all": [round(s, 4) for s in b_s],
                     "b_over_a": round(min(b_s) / a, 4), "device_path_is_faster": bool(min(b_s) < a),
                     "detail_call_gpu_ms_per_set": round(float(np.median(detail_ms)), 4),
                     "score_call_gpu_ms_per_set": round(float(np.median(score_ms)), 4),
                     "matched": [int(v) for v in got.scores["matched"]],
                     "top1_accuracy": [round(float(v), 3) for v in got.top_k["top1_accuracy"]]})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    if not same:
        sys.exit("the frames of (a) and (b) differ")


if __name__ == "__main__":
    main()
