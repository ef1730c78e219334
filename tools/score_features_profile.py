"""same_amd.sliding_window_score_features against what a study does without it (same_amd/score_features.py,
csrc/window_score_feature.hip): BASELINE cfg 5's generator (1M cells, windows 1200 / overlap 300, radius 25, knn 8, fp32
costs) with the SIX type-matrix variants of tools/variants_profile.py and the windows' triangulations given
(windows.TriangulationCache).  Every result is read as feature means: 200 reference and 20 moving feature columns (lognormal), groups =
the moving labels, a zone of about 20 % of the pairs (a mask over the reference rows), a subset of about 10 % (a mask over the moving
rows), edges 0 / 15 / 30 / inf.  Timed in one job:
  (a) the path that exists without the feature: sliding_window_scores(tables=True), then score_table_features per table -- split into
      the pass and the host work, --host-passes times after the device is warm;
  (b) sliding_window_score_features, the best of --passes after an untimed pass.
The frames of (a) and (b) must be identical (asserted).  The feature call's and the score call's GPU time per set are read from the
context's event timer around the library calls, with the zone and without, in passes of their own that are not wall-timed.  ONE JSON
line, appended to --out (default profiles/score_features_profile.jsonl).
Usage: python3 tools/score_features_profile.py [--cells N] [--passes 3] [--host-passes 1] [--workers N] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import same_amd                                          # noqa: E402
from same_amd import windows as W                        # noqa: E402
from variants_profile import BASE, inputs                # noqa: E402

CID = "Cell_Num_Old"
CALL_MS = {"score": [], "score_features": []}


def timed_calls():
    """every same_merge_acc_score and same_merge_acc_score_features call between two events of its context's stream -> the undo"""
    kept = {name: getattr(W.MergeAccumulator, name) for name in CALL_MS}
    for name, inner in kept.items():
        def timed(self, *a, _inner=inner, _into=CALL_MS[name], **k):
            self.ctx.timer_start()
            out = _inner(self, *a, **k)
            _into.append(self.ctx.timer_stop())
            return out

        setattr(W.MergeAccumulator, name, timed)
    return lambda: [setattr(W.MergeAccumulator, name, inner) for name, inner in kept.items()]


def identical(got, per_table, n_sets=1):
    """the study's frames against the tables' own, frame for frame (values, dtypes, order)"""
    try:
        for q, want in enumerate(per_table):
            v, s = q // n_sets, q % n_sets
            pd.testing.assert_series_equal(got.rows[v][s], want.rows, check_exact=True)
            pd.testing.assert_frame_equal(got.sums[v][s], want.sums, check_exact=True)
            pd.testing.assert_frame_equal(got.means[v][s], want.means, check_exact=True)
            z = got.zones[v][s]                          # the whole ZoneReading
            pd.testing.assert_series_equal(z.rows, want.zones.rows, check_exact=True)
            pd.testing.assert_frame_equal(z.sums, want.zones.sums, check_exact=True)
            pd.testing.assert_frame_equal(z.means, want.zones.means, check_exact=True)
            assert (z.zone_pairs, z.subset_pairs) == (want.zones.zone_pairs, want.zones.subset_pairs), "the zone's pair counts differ"
            pd.testing.assert_series_equal(got.resolution, want.resolution, check_exact=True)
            pd.testing.assert_frame_equal(got.pairs[v][s], want.pairs, check_exact=True)
    except AssertionError as e:
        print(e, file=sys.stderr)
        return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=1)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--ref-columns", type=int, default=200)
    ap.add_argument("--moving-columns", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_features_profile.jsonl"))
    args = ap.parse_args()

    r_df, m_df, cols, variants = inputs(args.cells)
    rng = np.random.default_rng(7)
    ref_x = rng.lognormal(0.0, 1.5, (len(r_df), args.ref_columns))
    mov_x = rng.lognormal(0.0, 1.5, (len(m_df), args.moving_columns))
    zones = same_amd.FeatureZones(None, rng.random(len(r_df)) < 0.2, rng.random(len(m_df)) < 0.1, None, [0, 15, 30, np.inf])
    what = dict(moving_features=mov_x, ref_features=ref_x, group_by="cell_type")
    line = {"tool": "score_features_profile", "workload": "cfg5_generator_six_type_variants", "cells": args.cells, "passes": args.passes,
            "host_passes": args.host_passes, "cpus": len(os.sched_getaffinity(0)), "variants": len(variants),
            "ref_columns": args.ref_columns, "moving_columns": args.moving_columns, "groups": int(m_df["cell_type"].nunique()),
            "edges": [0, 15, 30, "inf"]}
    with same_amd.resident_frames(r_df, m_df) as frames:
        kw = dict(workers=args.workers, optim_params=dict(BASE), triangulator=W.TriangulationCache(), type_variants=variants)
        device = lambda **more: same_amd.sliding_window_score_features(frames, m_df, cols, **{**what, "zones": zones, "per_pair": True, **more}, **kw)
        got = device()                                  # untimed: buffers grown, the resident objects made
        b_s, lean_s = [], []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            got = device()
            b_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            device(zones=None, per_pair=False)          # the means per group alone
            lean_s.append(time.perf_counter() - t0)
        a_pass, a_host, per_table = [], [], None
        for _ in range(args.host_passes):
            t0 = time.perf_counter()
            _scores, tables = same_amd.sliding_window_scores(frames, m_df, cols, tables=True, **kw)
            t1 = time.perf_counter()
            per_table = [same_amd.score_table_features(t, r_df, m_df, cell_id_col=CID, zones=zones, per_pair=True, **what)
                         for per_set in tables for t in per_set]
            a_pass.append(t1 - t0)
            a_host.append(time.perf_counter() - t1)
        same = identical(got, per_table)
        # GPU time per set, in passes of their own: the feature call with the zone and without, the score call over the same rows
        undo = timed_calls()
        device()
        with_zone, CALL_MS["score_features"][:] = list(CALL_MS["score_features"]), []
        device(zones=None, per_pair=False)
        undo()
        assert len(with_zone) == len(CALL_MS["score_features"]) == len(variants) and len(CALL_MS["score"]) == 2 * len(variants)
        a = min(p + h for p, h in zip(a_pass, a_host))
        z = got.zones[0][0]
        line.update({"frames_identical": bool(same),
                     "a_scores_with_tables_then_table_features_s": round(a, 4), "a_pass_s": round(min(a_pass), 4),
                     "a_table_features_s": round(min(a_host), 4),
                     "b_score_features_s": round(min(b_s), 4), "b_score_features_s_all": [round(s, 4) for s in b_s],
                     "b_without_zone_s": round(min(lean_s), 4),
                     "b_over_a": round(min(b_s) / a, 4), "device_path_is_faster": bool(min(b_s) < a),
                     "feature_call_gpu_ms_per_set_with_zone": round(float(np.median(with_zone)), 4),
                     "feature_call_gpu_ms_per_set_without_zone": round(float(np.median(CALL_MS["score_features"])), 4),
                     "score_call_gpu_ms_per_set": round(float(np.median(CALL_MS["score"])), 4),
                     "matched": [int(v) for v in got.scores["matched"]],
                     "zone_pairs": z.zone_pairs, "subset_pairs": z.subset_pairs, "pairs_per_bin": [int(v) for v in z.rows]})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    if not same:
        sys.exit("the frames of (a) and (b) differ")


if __name__ == "__main__":
    main()
