"""same_amd.sliding_window_variants against the loop of stand-alone jobs it replaces (same_amd/variants.py, csrc/window_recost.hip, DESIGN
§5.13): BASELINE cfg 5's generator (bench_cfg5's parameters: 1M cells, windows 1200 / overlap 300, radius 25, knn 8, fp32 costs) with SIX
type-matrix variants of the moving frame -- the frame's own and five noise levels on its type columns, renormalised per row, as the
reference's robustness script (examples/heart/run_robustness.sh) injects them.
The loop is what the single-job function offers: six sliding_window_incumbent calls, the first over the resident_frames object the shared
pass uses, the others on the moving frame with the variant's columns assigned (a frame of its own, so sections of its own: the frames a
resident_frames object holds are the caller's two).  An untimed pass of each, then the best of --passes; every variant's table must be the
job's (checked, and said in the record).  Both on the default route (Qhull helpers) and with the triangulations given
(windows.TriangulationCache: what a pass costs when nothing is triangulated).  Stage calls, recost calls and tickets are counted where the
binding makes them.
The recost kernel's own GPU time comes from a run of ITS own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/variants_profile.py --recost-walk
walks the plan once with stage + one recost call per batch and nothing else; `--stats-dir DIR` on the measuring run then reads the
recost kernels' rows of DIR's kernel_stats csv into the record (recost_kernel_gpu_ms_per_window).
ONE JSON line, appended to --out (default profiles/variants_profile.jsonl).
Usage: python3 tools/variants_profile.py [--cells N] [--passes 3] [--workers N] [--routes qhull,given] [--stats-dir DIR] [--out ...]"""
import argparse
import csv
import glob
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

NOISE = (0.05, 0.1, 0.2, 0.3, 0.5)
BASE = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, hip_cost_dtype="float32")
SEEN = {"stage": 0, "recost": 0, "tickets": 0}


def count_calls():
    """stage and recost calls of the binding, tickets asked of the triangulator a pass uses"""
    from same_amd import delaunay

    for key in ("stage", "recost"):
        def call(*a, _inner=getattr(W, key + "_windows"), _key=key, **k):
            SEEN[_key] += 1
            return _inner(*a, **k)

        setattr(W, key + "_windows", call)
    for cls in (delaunay.QhullTriangulator, W.TriangulationCache):
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


def inputs(cells):
    T = 8
    ref = synth.make_cells(cells, T, seed=0)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=1))
    cols = synth.type_columns(T)
    own = m_df[cols].to_numpy(dtype=np.float64)
    rng = np.random.default_rng(5)
    variants = [None]
    for sigma in NOISE:
        noised = np.abs(own + sigma * rng.standard_normal(own.shape))
        variants.append(np.ascontiguousarray(noised / np.maximum(noised.sum(axis=1, keepdims=True), 1e-12)))
    return r_df, m_df, cols, variants


def recost_walk(r_df, m_df, cols, variants, batch=8):
    """the plan walked once: per batch one stage call and ONE recost call, nothing else (the run the profiler watches) -> windows"""
    from same_amd.window_api import _WindowJob

    job = _WindowJob(r_df, m_df, cols, None, None, None, dict(BASE), None, False, None)
    frames, _own = job.device_frames("device")
    states = []
    try:
        ctx, o = frames.ctx, job.optim_params
        layer = frames.types_layer(variants[1], variants[1])
        states = [W.DeviceWindow(ctx) for _ in range(batch)]
        windows = 0
        for at in range(0, len(job.plan), batch):
            group = job.plan[at:at + batch]
            W.stage_windows(states[:len(group)], frames.dmov, frames.dref, [w["box"] for w in group], abs(float(o["radius"])), o["knn"],
                            o["dist_ct_coeff"])
            W.recost_windows(states[:len(group)], frames.dmov, frames.dref, layer, o["dist_ct_coeff"])
            windows += len(group)
        return windows
    finally:
        for st in states:
            st.close()
        frames.close()


def kernel_stats(stats_dir):
    """the recost kernels' rows of a `rocprofv3 --kernel-trace --stats` run's kernel_stats csv -> (calls, total ns), or None"""
    calls = total = 0
    found = False
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "recost_" in row.get("Name", ""):
                    found = True
                    calls += int(float(row["Calls"]))
                    total += int(float(row["TotalDurationNs"]))
    return (calls, total) if found else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--routes", default="qhull,given")
    ap.add_argument("--recost-walk", action="store_true", help="only stage + recost over the plan (the profiler's run)")
    ap.add_argument("--stats-dir", default=None, help="output directory of the profiler's run over --recost-walk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants_profile.jsonl"))
    args = ap.parse_args()

    r_df, m_df, cols, variants = inputs(args.cells)
    if args.recost_walk:
        print(json.dumps({"tool": "variants_profile", "recost_walk_windows": recost_walk(r_df, m_df, cols, variants)}), flush=True)
        return
    count_calls()
    from same_amd.variants import moving_variant

    moving_v = [m_df if v is None else moving_variant(m_df, cols, v) for v in variants]
    line = {"tool": "variants_profile", "workload": "cfg5_generator_six_type_variants", "cells": args.cells, "passes": args.passes,
            "cpus": len(os.sched_getaffinity(0)), "variants": len(variants), "noise": list(NOISE), "routes": {}}
    all_same = True
    with same_amd.resident_frames(r_df, m_df) as frames:
        for route in args.routes.split(","):
            tri = W.TriangulationCache() if route == "given" else None
            kw = dict(commonCT=cols, return_stats=True, workers=args.workers, optim_params=dict(BASE), triangulator=tri)
            loop = lambda: [same_amd.sliding_window_incumbent(frames if q == 0 else r_df, mv, **kw) for q, mv in enumerate(moving_v)]
            shared = lambda: same_amd.sliding_window_variants(frames, m_df, variants, **kw)
            want, loop_s, loop_calls = timed(loop, args.passes)
            got, shared_s, shared_calls = timed(shared, args.passes)
            same = all(identical(g[0], w[0]) and g[1] == w[1] for g, w in zip(got, want))
            all_same = all_same and same
            finished = sum(len(w[1]) for w in want)              # windows x variants that were finished
            line["routes"][route] = {"windows": len(want[0][1]), "tables_identical": bool(same), "shared_s": round(shared_s, 4),
                                     "loop_s": round(loop_s, 4), "loop_over_shared": round(loop_s / shared_s, 2),
                                     "shared_windows_per_s": round(finished / shared_s, 1), "loop_windows_per_s": round(finished / loop_s, 1),
                                     "shared_calls": shared_calls, "loop_calls": loop_calls}
    if args.stats_dir:
        got = kernel_stats(args.stats_dir)
        if got is not None:
            windows = next(iter(line["routes"].values()))["windows"]       # (the profiler's walk makes one recost call per batch of them)
            line["recost_kernel_calls"], line["recost_kernel_gpu_ms"] = got[0], round(got[1] / 1e6, 4)
            line["recost_kernel_gpu_ms_per_window"] = round(got[1] / 1e6 / max(windows, 1), 5)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if not all_same:
        sys.exit("a variant's table differs from the stand-alone job's")


if __name__ == "__main__":
    main()
