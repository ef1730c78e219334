"""same_amd.sliding_window_score_features(unpack=...) against what a MetaCell study did for the same frames before it
(same_amd/score_features.py, csrc/window_unpack_feature.hip), on tools/unpack_details_profile.py's workload: about
100k x 100k seeded cells, both sides collapsed at max_metacell_size=3, the six delaunay_penalty sets of the LUAD sweep,
hip_caller_delaunay="device", one resident_frames object for everything.  Every result is read as feature means of its CELL pairs: 200
reference and 20 moving feature columns per original cell (lognormal), groups = the moving cells' labels, a zone of about 20 % of the
pairs (a mask over the reference cells), a subset of about 10 % (a mask over the moving cells), edges 0 / 15 / 30 / inf, as in
tools/score_features_profile.py.  Per strategy, in one job:
  (a) the path that exists without the feature: sliding_window_scores(tables=True, unpack=strategy), then score_unpacked_features per
      table, split into the pass and the per-table statement;
  (b) sliding_window_score_features(unpack=strategy), no tables.
The frames of (a) and (b) are checked identical BEFORE anything is timed (the tool stops where they differ); then each is timed, the
best of --passes after the untimed pass that made the check, with nothing wrapped around the library calls.  After the wall times (b)
runs --passes + 1 times more with same_merge_acc_unpack_features between two events of the context's timer and, after it,
same_merge_acc_unpack (counts only) over the same rows: the GPU time per set of each, in passes that are not wall-timed.  No speed-up is
promised; the numbers are recorded as measured.  ONE JSON line, appended to --out (default profiles/unpack_features_profile.jsonl).
Usage: python3 tools/unpack_features_profile.py [--cells N] [--passes 3] [--workers N] [--out ...]"""
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
from same_amd import synth                               # noqa: E402
from same_amd import windows as W                        # noqa: E402
from unpack_scores_profile import OP, SETS, best_of      # noqa: E402

FEATURE_MS, COUNTS_MS = [], []


def time_unpack_feature_calls():
    """from now on every same_merge_acc_unpack_features call between two events of its context's stream, and after it
    same_merge_acc_unpack (counts only) over the same rows  -> the call that puts the method back as it was"""
    inner = W.MergeAccumulator.unpack_features

    def unpack_features(self, mov_members, ref_members, strategy, features, zone=None, d2=False, pairs=False):
        self.ctx.timer_start()
        out = inner(self, mov_members, ref_members, strategy, features, zone, d2, pairs)
        FEATURE_MS.append(self.ctx.timer_stop())
        self.ctx.timer_start()
        counts = self.unpack(mov_members, ref_members, strategy)
        COUNTS_MS.append(self.ctx.timer_stop())
        assert counts.tolist() == out[0].tolist()
        return out

    W.MergeAccumulator.unpack_features = unpack_features
    return lambda: setattr(W.MergeAccumulator, "unpack_features", inner)


def identical(got, per_table):
    """the study's frames against the tables' own, frame for frame (values, dtypes, order)"""
    try:
        for s, want in enumerate(per_table):
            pd.testing.assert_series_equal(got.rows[0][s], want.rows, check_exact=True)
            pd.testing.assert_frame_equal(got.sums[0][s], want.sums, check_exact=True)
            pd.testing.assert_frame_equal(got.means[0][s], want.means, check_exact=True)
            z = got.zones[0][s]
            pd.testing.assert_series_equal(z.rows, want.zones.rows, check_exact=True)
            pd.testing.assert_frame_equal(z.sums, want.zones.sums, check_exact=True)
            pd.testing.assert_frame_equal(z.means, want.zones.means, check_exact=True)
            assert (z.zone_pairs, z.subset_pairs) == (want.zones.zone_pairs, want.zones.subset_pairs), "the zone's pair counts differ"
            pd.testing.assert_series_equal(got.resolution, want.resolution, check_exact=True)
            pd.testing.assert_frame_equal(got.pairs[0][s], want.pairs, check_exact=True)
    except AssertionError as e:
        print("frames differ:", str(e)[:400], file=sys.stderr)
        return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--ref-columns", type=int, default=200)
    ap.add_argument("--moving-columns", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_features_profile.jsonl"))
    args = ap.parse_args()

    T = 8
    cells = synth.make_cells(args.cells, T, seed=0)
    r_c, a_c = synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=1))
    a_c["Cell_Num_Old"] = np.arange(len(a_c))
    labels = a_c["cell_type"].to_numpy().copy()          # one label in nine changed, or every cell would sit on a cell of its label
    labels[::9] = np.roll(labels, 1)[::9]
    a_c["cell_type"] = labels
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    mc_r, mc_a = collapse(r_c), collapse(a_c)
    cols = synth.type_columns(T)
    rng = np.random.default_rng(7)
    ref_x = rng.lognormal(0.0, 1.5, (len(mc_r.original_df), args.ref_columns))
    mov_x = rng.lognormal(0.0, 1.5, (len(mc_a.original_df), args.moving_columns))
    zones = same_amd.FeatureZones(None, rng.random(len(mc_r.original_df)) < 0.2, rng.random(len(mc_a.original_df)) < 0.1, None, [0, 15, 30, np.inf])
    what = dict(moving_features=mov_x, ref_features=ref_x, group_by=None, zones=zones, per_pair=True)
    line = {"tool": "unpack_features_profile", "workload": "luad_like_metacells_ms3_delaunay_penalty_sweep", "cells": [len(r_c), len(a_c)],
            "metacells": [len(mc_r.metacell_df), len(mc_a.metacell_df)], "sets": len(SETS), "passes": args.passes,
            "ref_columns": args.ref_columns, "moving_columns": args.moving_columns, "groups": int(pd.Series(labels).nunique()),
            "edges": [0, 15, 30, "inf"], "cpus": len(os.sched_getaffinity(0)), "strategies": {}}
    kw = dict(param_sets=SETS, optim_params=dict(OP), workers=args.workers)
    with same_amd.resident_frames(mc_r, mc_a) as frames:
        for strategy in ("distribute", "nearest"):
            split = {"pass": [], "statement": []}

            def before():
                t0 = time.perf_counter()
                _scores, tables, _cells = same_amd.sliding_window_scores(frames, mc_a, cols, tables=True, unpack=strategy, **kw)
                t1 = time.perf_counter()
                per_table = [same_amd.score_unpacked_features(table, mc_r, mc_a, strategy, **what) for table in tables[0]]
                split["pass"].append(t1 - t0)
                split["statement"].append(time.perf_counter() - t1)
                return per_table

            after = lambda: same_amd.sliding_window_score_features(frames, mc_a, cols, unpack=strategy, **what, **kw)
            # the check first, on untimed passes of both paths (they also grow the buffers and make the resident objects)
            same = identical(after(), before())
            line["strategies"][strategy] = {"frames_identical": bool(same)}
            if not same:
                print(json.dumps(line), flush=True)
                sys.exit("the frames of (a) and (b) differ: nothing was timed")
            del split["pass"][:], split["statement"][:]
            a_s, b_s = [], []
            for _ in range(args.passes):
                t0 = time.perf_counter()
                before()
                a_s.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                b = after()
                b_s.append(time.perf_counter() - t0)
            del FEATURE_MS[:], COUNTS_MS[:]
            unwrap = time_unpack_feature_calls()
            try:
                best_of(after, args.passes)                       # (GPU time per call: the event timer waits, so these passes are not timed)
            finally:
                unwrap()
            feature_ms, counts_ms = list(FEATURE_MS), list(COUNTS_MS)
            assert len(feature_ms) == len(SETS) * (args.passes + 1), "the device did not read every result"
            med = lambda ms: float(np.median(ms[len(SETS):]))
            z = b.zones[0][0]
            line["strategies"][strategy].update({
                "a_tables_then_score_unpacked_features_s": round(min(a_s), 4), "a_pass_with_tables_s": round(min(split["pass"]), 4),
                "a_statement_s": round(min(split["statement"]), 4), "a_s_all": [round(s, 4) for s in a_s],
                "b_score_features_unpack_s": round(min(b_s), 4), "b_s_all": [round(s, 4) for s in b_s],
                "b_over_a": round(min(b_s) / min(a_s), 4),
                "unpack_features_call_gpu_ms_per_set": round(med(feature_ms), 4), "unpack_counts_only_gpu_ms_per_set": round(med(counts_ms), 4),
                "features_share_gpu_ms_per_set": round(med(feature_ms) - med(counts_ms), 4),
                "unpack_features_call_gpu_ms_first_pass": [round(m, 4) for m in feature_ms[:len(SETS)]],
                "cells_matched": [int(v) for v in b.scores["cells_matched"]],
                "zone_pairs": z.zone_pairs, "subset_pairs": z.subset_pairs, "pairs_per_bin": [int(v) for v in z.rows]})
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
