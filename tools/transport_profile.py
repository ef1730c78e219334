"""optim_params["hip_incumbent"] = "transport" (csrc/assign.hip's transport form) through same_amd.sliding_window_incumbent, in one
process, ONE JSON line per workload (printed, and appended to --out, default profiles/transport_profile.jsonl):

  parity   BASELINE cfg 5 (bench_cfg5's parameters: a 1M-cell section, windows 1200 / overlap 300, radius 25, knn 8, float costs) at
           max_matches = 1, on resident frames: "transport" against "assignment" -- where nothing can be shared the generalisation
           should cost nothing.  windows/s on the default (Qhull) route and with the triangulations given (windows.TriangulationCache),
           best of --passes after an untimed pass, and the finish call's wall time per batch of 8 (the stage timer); "assignment" is
           measured --repeats times so that the ratio stands next to the spread of the one-to-one kernel itself.
  cfg5     the same section at max_matches = 2, penalty_coeff 100 and 10: the transport start alone, then hip_refine="capacity" from
           it and from the greedy start.
  meta     both sides collapsed by greedy_triangle_collapse (MS = 3, ref_metacell_match_multiplier = MS; MetaCell inputs: the general
           route), penalty_coeff 100 and 10, the same three runs.

Per run of cfg5 / meta: windows/s, summed `objective` (the transport optimum: a lower bound on the model), summed `mip_objective`
after the search, summed extra matches of the start and of the result, summed `mip_gap`, rounds and searches per window, fallbacks.
Usage: python3 tools/transport_profile.py [--cells 1000000] [--meta-cells 100000] [--passes 3] [--repeats 3]
                                          [--only parity|cfg5|meta] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import same_amd                                          # noqa: E402
from same_amd import _trace, synth                       # noqa: E402
from same_amd.windows import TriangulationCache          # noqa: E402

FINISH = "filter + signs + incumbent + sweeps (device)"
MS = 3
CFG5 = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)


def timed(run, passes):
    """-> (stats of the last pass, windows/s of the best pass, its finish-call ms per batch of 8) after an untimed pass"""
    _table, stats = run()
    best, finish = float("inf"), (0, 0.0)
    for _ in range(passes):
        _trace.reset()
        t0 = time.perf_counter()
        _table, stats = run()
        dt = time.perf_counter() - t0
        if dt < best:
            best, finish = dt, _trace.report().get(FINISH, (0, 0.0))
    return stats, round(len(stats) / best, 1), round(finish[1] * 1e3 / max(1, len(stats) / 8), 3)


def record(stats, wps):
    rec = {"windows": len(stats), "windows_per_s": wps}
    total = lambda k: float(sum(s[k] for s in stats))
    if "objective" in stats[0]:
        searches = np.array([s["transport_searches"] for s in stats])
        rec.update(objective=total("objective"), fallbacks=int(total("fallback")),
                   ref_extra_matches_start=int(total("ref_extra_matches_start")),
                   searches_mean=round(float(searches.mean()), 2), searches_max=int(searches.max()))
    if "mip_objective" in stats[0]:
        rounds = np.array([s["refine_rounds"] for s in stats])
        rec.update(mip_objective_start=total("mip_objective_start"), mip_objective=total("mip_objective"),
                   ref_extra_matches=int(total("ref_extra_matches")), rounds_mean=round(float(rounds.mean()), 3),
                   rounds_max=int(rounds.max()))
    if "mip_gap" in stats[0]:
        rec.update(mip_gap_sum=total("mip_gap"), mip_gap_max=float(max(s["mip_gap"] for s in stats)))
    return rec


def capacity_runs(call, op, passes):
    """the transport start alone, the search from it, the search from the greedy start -- at penalty_coeff 100 and 10"""
    out = {}
    for pc in (100, 10):
        o = dict(op, penalty_coeff=pc)
        for name, mode in (("transport", dict(o, hip_incumbent="transport")),
                           ("transport_capacity", dict(o, hip_incumbent="transport", hip_refine="capacity")),
                           ("greedy_capacity", dict(o, hip_refine="capacity"))):
            stats, wps, _ms = timed(lambda: call(mode), passes)
            out[f"pc{pc}_{name}"] = record(stats, wps)
    return out


def frames(cells, seed):
    T = 8
    ref = synth.make_cells(cells, T, seed=seed)
    mov = synth.make_jittered(ref, seed=seed + 1)
    return synth.to_frame(ref), synth.to_frame(mov), synth.type_columns(T)


def parity(args):
    r_df, m_df, cols = frames(args.cells, 0)
    line = {"tool": "transport_profile", "workload": "cfg5_max_matches_1_parity", "cells": args.cells,
            "cpus": len(os.sched_getaffinity(0))}
    with same_amd.resident_frames(r_df, m_df) as res:
        cache = TriangulationCache()
        for route, tri in (("default", None), ("tris_given", cache)):
            call = lambda o: same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(o), merge=True,
                                                               return_stats=True, triangulator=tri)
            base = [timed(lambda: call(dict(CFG5, hip_incumbent="assignment")), args.passes) for _ in range(args.repeats)]
            stats, wps, ms = timed(lambda: call(dict(CFG5, hip_incumbent="transport")), args.passes)
            line[route] = {"assignment_windows_per_s": [b[1] for b in base], "assignment_finish_ms_per_batch8": [b[2] for b in base],
                           "transport_windows_per_s": wps, "transport_finish_ms_per_batch8": ms,
                           "ratio_windows_per_s": round(wps / float(np.median([b[1] for b in base])), 4),
                           "same_objective_bits": [s["objective"] for s in stats] == [s["objective"] for s in base[-1][0]],
                           "fallbacks": int(sum(s["fallback"] for s in stats)), "windows": len(stats)}
    return line


def cfg5(args):
    r_df, m_df, cols = frames(args.cells, 0)
    line = {"tool": "transport_profile", "workload": "cfg5_max_matches_2", "cells": args.cells, "cpus": len(os.sched_getaffinity(0))}
    with same_amd.resident_frames(r_df, m_df) as res:
        call = lambda o: same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(o), merge=True, return_stats=True)
        line.update(capacity_runs(call, dict(CFG5, max_matches=2), args.passes))
    return line


def meta(args):
    from same_amd.metacell_utils import greedy_triangle_collapse

    r_df, m_df, cols = frames(args.meta_cells, 2)
    kw = dict(original_idx_col="Cell_Num_Old", max_metacell_size=MS, r_max=25, min_angle_deg=15, return_object=True, verbose=False)
    mc_m, mc_r = greedy_triangle_collapse(m_df, **kw), greedy_triangle_collapse(r_df, **kw)
    op = dict(radius=25, knn=8, no_match_penalty=100, window_size=1200, overlap=300, min_cells_per_window=10, cell_id_col="metacell_id",
              ref_metacell_match_multiplier=MS)
    line = {"tool": "transport_profile", "workload": "metacell_MS3", "cells": args.meta_cells,
            "metacells": [len(mc_r.metacell_df), len(mc_m.metacell_df)], "cpus": len(os.sched_getaffinity(0))}
    call = lambda o: same_amd.sliding_window_incumbent(mc_r, mc_m, commonCT=cols, optim_params=dict(o), merge=True, return_stats=True)
    line.update(capacity_runs(call, op, args.passes))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--meta-cells", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("parity", "cfg5", "meta"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transport_profile.jsonl"))
    args = ap.parse_args()
    _trace.enable(True)
    for name, fn in (("parity", parity), ("cfg5", cfg5), ("meta", meta)):
        if args.only not in (None, name):
            continue
        line = fn(args)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
