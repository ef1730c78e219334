"""same_amd.sliding_window_sweep against the loop of stand-alone jobs it replaces (same_amd/sweep.py, csrc/window_knn_prefix.hip, DESIGN
§5.12): BASELINE cfg 5's generator (bench_cfg5's parameters: windows 1200 / overlap 300, radius 25, fp32 costs) under the reference's two
heart grids (examples/heart/run_parameter_sweep.sh) as six sets each -- knn in {1, 2, 4, 6, 8, 10} with hip_refine="local", and
delaunay_penalty in {0, 1, 5, 10, 25, 50} at knn = 8 (hip_refine="local": the key is read by the search) -- on each triangulation route.
The loop is the best the single-job function offers: six sliding_window_incumbent calls over ONE resident_frames object, in the same
process and job as the sweep.  An untimed pass of each, then the best of --passes; every set's table must be the job's (checked, and said
in the record).  Stage calls and tickets are counted where the binding makes them.  Then one more walk over the plan with the library's
own timer around every batch's same_window_knn_prefix call: the GPU time a prefix costs per window.
--case metacell: the workload the reference's sweep scripts run (examples/heart/run_same.sh hands MetaCell objects over): both frames
collapsed at max_metacell_size = 3, hip_caller_delaunay="device", the knn grid; the shared pass (one stage call and one selection of the
caller's triangles per batch, same_window_caller_pairs per further knn) against the loop of jobs over one resident_frames object, as
windows/s (windows x sets / seconds), and one more walk with the library's timer around every batch's same_window_caller_pairs call.
ONE JSON line per case, appended to --out (default profiles/sweep_profile.jsonl).
Usage: python3 tools/sweep_profile.py [--case frames|metacell] [--cells N] [--passes 3] [--workers N] [--routes qhull,native,device] [--out ...]"""
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
from same_amd import windows as W                        # noqa: E402

GRIDS = {"knn": [{"knn": k, "hip_refine": "local"} for k in (1, 2, 4, 6, 8, 10)],
         "delaunay_penalty": [{"knn": 8, "hip_refine": "local", "delaunay_penalty": p} for p in (0, 1, 5, 10, 25, 50)]}
SEEN = {"stage": 0, "tickets": 0, "caller_tris": 0, "caller_pairs": 0}


def count_calls():
    """stage calls of the binding, tickets asked of whichever triangulator a pass uses (a device ticket is one triangulation too)"""
    from same_amd import delaunay

    inner = W.stage_windows

    def stage(*a, **k):
        SEEN["stage"] += 1
        return inner(*a, **k)

    W.stage_windows = stage
    for name in ("caller_tris", "caller_pairs"):
        def call(*a, _inner=getattr(W, name + "_windows"), _name=name, **k):
            SEEN[_name] += 1
            return _inner(*a, **k)

        setattr(W, name + "_windows", call)
    for cls in (delaunay.QhullTriangulator, delaunay.NativeTriangulator, delaunay.DeviceTriangulator):
        def submit(self, points, key=None, _inner=cls.submit):
            SEEN["tickets"] += 1
            return _inner(self, points, key)

        cls.submit = submit


def timed(run, passes):
    """-> (result, best seconds of `passes` after an untimed pass, calls of one pass)"""
    out = run()
    best = float("inf")
    for _ in range(passes):
        SEEN.update(dict.fromkeys(SEEN, 0))
        t0 = time.perf_counter()
        out = run()
        best = min(best, time.perf_counter() - t0)
    return out, best, dict(SEEN)


def identical(a, b):
    if list(a.columns) != list(b.columns) or len(a) != len(b):
        return False
    return all(np.array_equal(a[c].to_numpy(), b[c].to_numpy()) for c in a.columns)


def prefix_gpu_ms(r_df, m_df, cols, op, k_staged, k, batch=8):
    """the plan walked once more, stage at k_staged + prefix at k only: GPU milliseconds inside same_window_knn_prefix, summed"""
    from same_amd.window_api import _WindowJob

    job = _WindowJob(r_df, m_df, cols, None, None, None, op, None, False, None)
    frames, _own = job.device_frames("device")
    states = []
    try:
        ctx, o = frames.ctx, job.optim_params
        states = [W.DeviceWindow(ctx) for _ in range(batch)]
        ms, windows = 0.0, 0
        for rep in range(2):                     # the first walk grows the windows' buffers; the second is the one that counts
            ms, windows = 0.0, 0
            for at in range(0, len(job.plan), batch):
                group = job.plan[at:at + batch]
                W.stage_windows(states[:len(group)], frames.dmov, frames.dref, [w["box"] for w in group], abs(float(o["radius"])), k_staged,
                                o["dist_ct_coeff"])
                ctx.timer_start()
                W.prefix_windows(states[:len(group)], k)
                ms += ctx.timer_stop()
                windows += len(group)
        return ms, windows
    finally:
        for st in states:
            st.close()
        frames.close()


def caller_pairs_gpu_ms(mc_r, mc_a, cols, op, k_staged, k, batch=8):
    """the plan walked once more -- stage at k_staged, the caller's triangles, prefix at k -- with the library's timer around
    same_window_caller_pairs alone: GPU milliseconds inside it, summed, and the windows that held a selection"""
    from same_amd.triangles import cos_threshold
    from same_amd.window_api import _WindowJob

    job = _WindowJob(mc_r, mc_a, cols, None, None, None, op, None, False, None)
    frames, _own = job.device_frames("device")
    states = []
    try:
        ctx, o = frames.ctx, job.optim_params
        caller = frames.caller_tris(job.moving_delaunay, job.vertex_col)
        en, thr = cos_threshold(o.get("min_angle_deg", 15))
        tol = float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0
        filt = (o["radius"], en, thr, tol, o["ignore_same_type_triangles"])
        states = [W.DeviceWindow(ctx) for _ in range(batch)]
        ms, windows = 0.0, 0
        for rep in range(2):                     # the first walk grows the windows' buffers; the second is the one that counts
            ms, windows = 0.0, 0
            for at in range(0, len(job.plan), batch):
                group = job.plan[at:at + batch]
                counts = W.stage_windows(states[:len(group)], frames.dmov, frames.dref, [w["box"] for w in group], abs(float(o["radius"])),
                                         k_staged, o["dist_ct_coeff"])
                live = [st for st, c in zip(states, counts) if c[3]]
                if not live:
                    continue
                got = W.caller_tris_windows(live, caller, *filt)
                live = [st for st, g in zip(live, got) if g[2] == 0]      # (a cosine at the threshold: the host's to decide, not timed here)
                if not live:
                    continue
                W.prefix_windows(live, k)
                ctx.timer_start()
                W.caller_pairs_windows(live)
                ms += ctx.timer_stop()
                windows += len(live)
        return ms, windows
    finally:
        for st in states:
            st.close()
        frames.close()


def metacell_case(args):
    """-> the record of the MetaCell case"""
    T = 8
    n = args.cells if args.cells is not None else 200_000
    cells = synth.make_cells(n, T, seed=0)
    r_c, a_c = synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=1))
    a_c["Cell_Num_Old"] = np.arange(len(a_c))
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    mc_r, mc_a = collapse(r_c), collapse(a_c)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, hip_cost_dtype="float32",
              hip_caller_delaunay="device")
    sets = GRIDS["knn"]
    kw = dict(commonCT=cols, return_stats=True, workers=args.workers)
    with same_amd.resident_frames(mc_r, mc_a) as frames:
        loop = lambda: [same_amd.sliding_window_incumbent(frames, mc_a, optim_params={**op, **ps}, **kw) for ps in sets]
        sweep = lambda: same_amd.sliding_window_sweep(frames, mc_a, sets, optim_params=dict(op), **kw)
        want, loop_s, loop_calls = timed(loop, args.passes)
        got, sweep_s, sweep_calls = timed(sweep, args.passes)
    same = all(identical(g[0], w[0]) and g[1] == w[1] for g, w in zip(got, want))
    finished = sum(len(w[1]) for w in want)              # windows x sets that were finished
    ms, timed_windows = caller_pairs_gpu_ms(mc_r, mc_a, cols, op, 10, 4)
    return {"tool": "sweep_profile", "workload": "metacells_ms3_caller_delaunay_device_knn_grid", "cells": n,
            "metacells": [len(mc_r.metacell_df), len(mc_a.metacell_df)], "passes": args.passes, "cpus": len(os.sched_getaffinity(0)),
            "sets": len(sets), "windows": len(want[-1][1]), "tables_identical": bool(same),
            "sweep_s": round(sweep_s, 4), "loop_s": round(loop_s, 4), "sweep_windows_per_s": round(finished / sweep_s, 1),
            "loop_windows_per_s": round(finished / loop_s, 1),
            "sweep_calls": sweep_calls, "loop_calls": loop_calls,
            "caller_pairs_gpu_ms_per_window": round(ms / max(timed_windows, 1), 4), "caller_pairs_timed_windows": timed_windows}, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("frames", "metacell"), default="frames")
    ap.add_argument("--cells", type=int, default=None, help="default: 1000000 (frames), 200000 (metacell)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--routes", default="qhull,native,device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_profile.jsonl"))
    args = ap.parse_args()

    count_calls()
    if args.case == "metacell":
        line, all_same = metacell_case(args)
        emit(line, args.out, all_same)
        return
    args.cells = 1_000_000 if args.cells is None else args.cells
    T = 8
    ref = synth.make_cells(args.cells, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    base = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, hip_cost_dtype="float32")
    line = {"tool": "sweep_profile", "workload": "cfg5_generator_heart_grids", "cells": args.cells, "passes": args.passes,
            "cpus": len(os.sched_getaffinity(0)), "sets_per_grid": 6, "routes": {}}
    all_same = True
    with same_amd.resident_frames(r_df, m_df) as frames:
        for route in args.routes.split(","):
            op = dict(base) if route == "qhull" else dict(base, hip_delaunay=route)
            rec = {}
            for grid, sets in GRIDS.items():
                kw = dict(commonCT=cols, return_stats=True, workers=args.workers)
                loop = lambda: [same_amd.sliding_window_incumbent(frames, m_df, optim_params={**op, **ps}, **kw) for ps in sets]
                sweep = lambda: same_amd.sliding_window_sweep(frames, m_df, sets, optim_params=dict(op), **kw)
                want, loop_s, loop_calls = timed(loop, args.passes)
                got, sweep_s, sweep_calls = timed(sweep, args.passes)
                same = all(identical(g[0], w[0]) and g[1] == w[1] for g, w in zip(got, want))
                all_same = all_same and same
                rec[grid] = {"windows": len(want[0][1]), "tables_identical": bool(same), "sweep_s": round(sweep_s, 4),
                             "loop_s": round(loop_s, 4), "loop_over_sweep": round(loop_s / sweep_s, 2),
                             "sweep_stage_calls": sweep_calls["stage"], "loop_stage_calls": loop_calls["stage"],
                             "sweep_triangulations": sweep_calls["tickets"], "loop_triangulations": loop_calls["tickets"]}
            line["routes"][route] = rec
    ms, timed_windows = prefix_gpu_ms(r_df, m_df, cols, base, 10, 4)
    line["prefix_gpu_ms_per_window"] = round(ms / max(timed_windows, 1), 4)
    line["prefix_timed_windows"] = timed_windows
    emit(line, args.out, all_same)


def emit(line, out, all_same):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if not all_same:
        sys.exit("a sweep's table differs from the stand-alone job's")


if __name__ == "__main__":
    main()
