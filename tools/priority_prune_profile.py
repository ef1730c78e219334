"""optim_params["hip_priority_prune"] = "device" against the general route on a job with ignore_knn_if_matched (csrc/window_priority.hip,
DESIGN §5.11): BASELINE cfg 5's generator (bench_cfg5's parameters: windows 1200 / overlap 300, radius 25, knn 8) with the
cell-type-priority prune on.  Both routes in one job and one process: an untimed pass each, then the best of --passes; the two tables
must be identical (checked, and said in the record).  Then one more walk over the plan with the library's own timer (same_timer_start /
_stop, events on the context's stream) around every batch's same_window_priority_pairs call: the GPU time the prune adds per window.
ONE JSON line, appended to --out (default profiles/priority_prune_profile.jsonl): windows, windows/s of either route, their ratio, pairs
staged and left, rows that kept one pair and rows that kept all, the prune's GPU milliseconds per window.
Usage: python3 tools/priority_prune_profile.py [--cells 1000000] [--passes 3] [--workers N] [--out ...]"""
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


def prune_gpu_ms(r_df, m_df, cols, op, batch=8):
    """the plan walked once more, stage + prune only: GPU milliseconds inside same_window_priority_pairs, summed over the batches"""
    from same_amd import windows as W
    from same_amd.window_api import _WindowJob

    job = _WindowJob(r_df, m_df, cols, None, None, None, op, None, False, None)
    frames, _own = job.device_frames("device")
    states = []
    try:
        frames.label_codes_on_device()
        ctx, o = frames.ctx, job.optim_params
        states = [W.DeviceWindow(ctx) for _ in range(batch)]
        ms, windows = 0.0, 0
        for rep in range(2):                     # the first walk grows the windows' buffers; the second is the one that counts
            ms, windows = 0.0, 0
            for at in range(0, len(job.plan), batch):
                group = job.plan[at:at + batch]
                W.stage_windows(states[:len(group)], frames.dmov, frames.dref, [w["box"] for w in group], abs(float(o["radius"])), o["knn"],
                                o["dist_ct_coeff"])
                ctx.timer_start()
                W.priority_windows(states[:len(group)])
                ms += ctx.timer_stop()
                windows += len(group)
        return ms, windows
    finally:
        for st in states:
            st.close()
        frames.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priority_prune_profile.jsonl"))
    args = ap.parse_args()

    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, ignore_knn_if_matched=True)
    general = lambda: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op), return_stats=True)
    device = lambda: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op, hip_priority_prune="device"),
                                                       return_stats=True, _route="device", workers=args.workers)
    g_table, g_stats, g_s = timed(general, args.passes)
    d_table, d_stats, d_s = timed(device, args.passes)
    same = identical(g_table, d_table) and [s["pairs"] for s in g_stats] == [s["pairs"] for s in d_stats]
    ms, timed_windows = prune_gpu_ms(r_df, m_df, cols, op)
    line = {"tool": "priority_prune_profile", "workload": "cfg5_generator_ignore_knn_if_matched", "cells": args.cells,
            "passes": args.passes, "cpus": len(os.sched_getaffinity(0)), "windows": len(g_stats), "rows": len(g_table),
            "tables_identical": bool(same), "general_windows_per_s": round(len(g_stats) / g_s, 1),
            "device_windows_per_s": round(len(d_stats) / d_s, 1), "device_over_general": round(g_s / d_s, 2),
            "pairs_staged": int(sum(s["pairs_staged"] for s in d_stats)), "pairs_left": int(sum(s["pairs"] for s in d_stats)),
            "rows_one_pair": int(sum(s["priority_rows"] for s in d_stats)), "rows_all_pairs": int(sum(s["keep_all_rows"] for s in d_stats)),
            "prune_gpu_ms_per_window": round(ms / max(timed_windows, 1), 4), "prune_timed_windows": timed_windows}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if not same:
        sys.exit("the two routes' tables differ")


if __name__ == "__main__":
    main()
