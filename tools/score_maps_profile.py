"""same_amd.sliding_window_score_maps against what a study does without it (same_amd/score_maps.py, csrc/window_score_map.hip,
DESIGN §5.18): BASELINE cfg 5's generator (1M cells, windows 1200 / overlap 300, radius 25, knn 8, fp32 costs) with the SIX type-matrix
variants of tools/variants_profile.py, every result read per cell with ranks=True and, as truth, the generator's own pairing (a moving
cell is the jittered copy of one reference cell: synth.make_jittered keeps the rows its first draw keeps).  The moving frame's
triangulation (scipy, the whole frame) is made once, outside every timed region.  Timed in one job, with the windows' triangulations
given (windows.TriangulationCache):
  (a) the path that exists without the feature: sliding_window_scores(tables=True), then score_table_maps per table -- split into the
      pass and the host work, --host-passes times after the device is warm;
  (b) sliding_window_score_maps, the best of --passes after an untimed pass.
The frames of (a) and (b) must be identical (asserted), and (b)'s tally the sum over them.  The map call's and the score call's GPU time
per set are read from the context's event timer around the library calls, in passes of their own that are not wall-timed.  ONE JSON
line, appended to --out (default profiles/score_maps_profile.jsonl).
Usage: python3 tools/score_maps_profile.py [--cells N] [--passes 3] [--host-passes 1] [--workers N] [--out ...]"""
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
CALL_MS = {"score": [], "score_map": []}


def timed_calls():
    """every same_merge_acc_score and same_merge_acc_score_map call between two events of its context's stream -> the undo"""
    kept = {name: getattr(W.MergeAccumulator, name) for name in CALL_MS}
    for name, inner in kept.items():
        def timed(self, *a, _inner=inner, _into=CALL_MS[name], **k):
            self.ctx.timer_start()
            out = _inner(self, *a, **k)
            _into.append(self.ctx.timer_stop())
            return out

        setattr(W.MergeAccumulator, name, timed)
    return lambda: [setattr(W.MergeAccumulator, name, inner) for name, inner in kept.items()]


def generator_truth(r_df, m_df, seed=1, drop=0.05):
    """per moving row the id of the reference cell it was jittered from (synth.make_jittered(ref, seed): the rows its first draw keeps)"""
    keep = np.random.default_rng(seed).random(len(r_df)) >= drop
    assert int(keep.sum()) == len(m_df)
    return r_df[CID].to_numpy()[keep]


def identical(got, per_table, n_sets=1):
    """the study's frames against the tables' own, frame for frame (values, dtypes, order), and the tally against their sum"""
    import pandas as pd

    from same_amd.score_maps import tally_from_cells

    try:
        for q, want in enumerate(per_table):
            pd.testing.assert_frame_equal(got.cells[q // n_sets][q % n_sets], want, check_exact=True)
        pd.testing.assert_frame_equal(got.tally, tally_from_cells(per_table, got.tally.index), check_exact=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_maps_profile.jsonl"))
    args = ap.parse_args()

    r_df, m_df, cols, variants = inputs(args.cells)
    truth = generator_truth(r_df, m_df)
    t0 = time.perf_counter()
    tris = Delaunay(m_df[["X", "Y"]].to_numpy()).simplices.astype(np.int64)
    tri_s = time.perf_counter() - t0
    line = {"tool": "score_maps_profile", "workload": "cfg5_generator_six_type_variants", "cells": args.cells, "passes": args.passes,
            "host_passes": args.host_passes, "cpus": len(os.sched_getaffinity(0)), "variants": len(variants), "ranks": True,
            "truth": "the generator's pairing", "score_triangles": len(tris), "score_triangulation_s": round(tri_s, 3)}
    with same_amd.resident_frames(r_df, m_df) as frames:
        kw = dict(workers=args.workers, optim_params=dict(BASE), triangulator=W.TriangulationCache(), type_variants=variants,
                  score_delaunay=tris)
        device = lambda **more: same_amd.sliding_window_score_maps(frames, m_df, cols, truth=truth, ranks=True, **more, **kw)
        got = device()                                  # untimed: buffers grown, the resident objects made
        b_s, lean_s = [], []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            got = device()
            b_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            device(per_result=False)                    # counts and tally only: no marks come back, no frames are made
            lean_s.append(time.perf_counter() - t0)
        a_pass, a_host, per_table = [], [], None
        for _ in range(args.host_passes):
            t0 = time.perf_counter()
            _scores, tables = same_amd.sliding_window_scores(frames, m_df, cols, tables=True, **kw)
            t1 = time.perf_counter()
            per_table = [same_amd.score_table_maps(t, r_df, m_df, cell_id_col=CID, commonCT=cols, truth=truth, ranks=True, score_delaunay=tris)
                         for per_set in tables for t in per_set]
            a_pass.append(t1 - t0)
            a_host.append(time.perf_counter() - t1)
        same = identical(got, per_table)
        # GPU time per set, in passes of their own: the map call, then the score call over the same rows
        undo = timed_calls()
        device()
        same_amd.sliding_window_scores(frames, m_df, cols, **kw)
        undo()
        assert len(CALL_MS["score_map"]) == len(CALL_MS["score"]) == len(variants)
        a = min(p + h for p, h in zip(a_pass, a_host))
        line.update({"frames_identical": bool(same),
                     "a_scores_with_tables_then_table_maps_s": round(a, 4), "a_pass_s": round(min(a_pass), 4),
                     "a_table_maps_s": round(min(a_host), 4),
                     "b_score_maps_s": round(min(b_s), 4), "b_score_maps_s_all": [round(s, 4) for s in b_s],
                     "b_without_frames_s": round(min(lean_s), 4),
                     "b_over_a": round(min(b_s) / a, 4), "device_path_is_faster": bool(min(b_s) < a),
                     "map_call_gpu_ms_per_set": round(float(np.median(CALL_MS["score_map"])), 4),
                     "score_call_gpu_ms_per_set": round(float(np.median(CALL_MS["score"])), 4),
                     "matched": [int(v) for v in got.scores["matched"]],
                     "truth_accuracy": [round(float(v), 3) for v in got.scores["truth_accuracy"]],
                     "cells_in_every_result": int((got.tally["matched_in"] == len(variants)).sum())})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    if not same:
        sys.exit("the frames of (a) and (b) differ")


if __name__ == "__main__":
    main()
