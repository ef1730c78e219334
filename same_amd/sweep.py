"""A list of parameter sets over ONE pass of the windows: `sliding_window_sweep`.

`sliding_window_incumbent` is what a caller tries parameters with before a licensed solve is paid for, and such a search is a sweep:
several values of `knn` at one penalty, several penalties at one `knn`, the starts and the searches, always over the same two frames.
As single jobs every point stages and triangulates every window again, although none of these keys changes a window's triangulation:

* the prune keeps an aligned row when ANY reference lies within `radius`: the kept rows, and the points triangulated, do not depend on `knn`;
* a row's pairs are ordered by (squared distance, reference row), a total order: the list at k' < k is every row's first min(k', count)
  pairs of the list at k (csrc/window_knn_prefix.hip derives it on the device);
* the penalties, the start and the search are read by the finish call alone (`WindowMode`).

So the sweep stages every window once at the largest `knn`, triangulates it once, and finishes it once per set
(windows.iter_device_windows with `sets`).  `sliding_window_sweep(...)[i]` is `sliding_window_incumbent` under
{**optim_params, **param_sets[i]}: table, dtypes, row order, stats."""
import threading

from .incumbent import (_TableBuilder, _begin_accumulators, _default_workers, _device_ref_idx, _device_stats, _route_table,
                        sliding_window_incumbent)
from .window_api import ResidentFrames, _WindowJob, _window_error
from .window_mode import WindowMode, caller_delaunay_route, priority_prune_route

# what a set may override: the keys that change neither a window's rows nor its triangulation
SWEEP_KEYS = ("knn", "no_match_penalty", "delaunay_penalty", "penalty_coeff", "max_matches", "ref_metacell_match_multiplier",
              "hip_incumbent", "hip_refine", "hip_refine_rounds")


def _checked_sets(param_sets, optim_params, gurobi_params, moving):
    """-> [(the set's full optim_params, its WindowMode)]; ValueError for anything a set may not be, before a job exists"""
    import numbers

    if param_sets is None or isinstance(param_sets, (dict, str)) or len(param_sets) == 0:
        raise ValueError("param_sets must be a non-empty list of dicts of overrides")
    shared = dict(optim_params or {})
    out = []
    for q, ps in enumerate(param_sets):
        if not isinstance(ps, dict):
            raise ValueError(f"param_sets[{q}] must be a dict of overrides, not {type(ps).__name__}")
        other = [k for k in ps if k not in SWEEP_KEYS]
        if other:
            raise ValueError(f"param_sets[{q}] overrides {other}: a set may override only {SWEEP_KEYS}")
        op = {**shared, **ps}
        mode = WindowMode.from_params(op, gurobi_params, moving)
        if "knn" in op:
            k = op["knn"]
            if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
                raise ValueError(f"param_sets[{q}]: knn must be an int >= 1, not {k!r}")
        out.append((op, mode))
    return out


def sliding_window_sweep(ref, moving, param_sets, commonCT=None, *, optim_params=None, gurobi_params=None, workers=None,
                         window_local_indices=False, return_stats=False, triangulator=None, ctx=None, merge=False, batch=None):
    """`sliding_window_incumbent` for every parameter set of `param_sets` over one pass of the windows.
    -> [table per set, in param_sets order] (with return_stats: [(table, [per-window stats dict in plan order]) per set]).
    `optim_params` is what the sets share; each set is a dict of overrides drawn from SWEEP_KEYS.  Any other key in a set, an empty list
    or a set `WindowMode.from_params` refuses raises ValueError before a window job or a device is touched.
    Result i is `sliding_window_incumbent(ref, moving, commonCT, optim_params={**optim_params, **param_sets[i]}, ...)` with the same
    `gurobi_params`, `workers`, `window_local_indices`, `triangulator`, `ctx`, `merge` and `batch` -- table, dtypes, row order and stats
    -- on every triangulation route (optim_params["hip_delaunay"]), with and without hip_priority_prune="device", merged or not (one
    merge accumulator per set).  Every window is staged once at the sets' largest knn and triangulated once, then finished once per set.
    `ref` / `moving` may be a `resident_frames` object.
    Inputs that do not take the plain device route -- a caller's triangulation or MetaCell objects, ignore_knn_if_matched without
    hip_priority_prune="device", frames the device sections refuse -- are run set by set through `sliding_window_incumbent`: the same
    results, nothing shared.  (Sharing under hip_caller_delaunay="device", an `outprefix` and sweeps over ranks are not offered here.)"""
    checked = _checked_sets(param_sets, optim_params, gurobi_params, moving)
    new_job = lambda op, mode, **kw: _WindowJob(ref, moving, commonCT, None, None, None, op, gurobi_params, False, None, mode=mode, **kw)
    job = new_job(*checked[0])
    kw = {}
    if not isinstance(ref, ResidentFrames) and not isinstance(moving, ResidentFrames):
        # the sets share window_size, overlap and min_cells: the first job's plan serves the others (this object holds nothing else)
        kw["resident"] = ResidentFrames(ref, moving)
        kw["resident"].plans[(job.window_size, job.overlap, job.optim_params["min_cells_per_window"])] = (job.plan, job.grid)
    jobs = [job] + [new_job(op, mode, **kw) for op, mode in checked[1:]]
    op0 = job.optim_params
    priority = bool(op0["ignore_knn_if_matched"]) and priority_prune_route(op0) == "device"
    host_prune = bool(op0["ignore_knn_if_matched"]) and not priority
    caller_delaunay_route(op0)
    frames, own = job.device_frames(None, ctx=ctx)
    shared_pass = frames is not None and not job.caller_triangulation and not host_prune
    try:
        if shared_pass:
            if triangulator is None:
                from . import delaunay

                triangulator = delaunay.triangulator_for(op0)
            return _sweep_device_route(jobs, frames, workers, window_local_indices, triangulator, merge, batch, priority, return_stats)
    finally:
        if own and frames is not None:
            frames.close()
    # set by set: the general route (or a caller's triangulation on the device route), nothing shared
    return [sliding_window_incumbent(ref, moving, commonCT, optim_params=op, gurobi_params=gurobi_params, workers=workers,
                                     window_local_indices=window_local_indices, return_stats=return_stats, triangulator=triangulator,
                                     ctx=ctx, merge=merge, batch=batch) for op, _mode in checked]


def _sweep_device_route(jobs, frames, workers, with_ref_idx, triangulator, merge, batch, priority, return_stats):
    """incumbent._device_route for several jobs that differ in SWEEP_KEYS only (one plan, one share of it): the windows are walked once,
    every set has its own builders, accumulators and stats, and its table is made by the single job's own tail (_route_table)."""
    import os

    from .windows import MergeAccumulator

    job = jobs[0]
    n_workers = max(1, int(workers if workers is not None else _default_workers()))
    n_workers = min(n_workers, max(1, len(job.todo)))
    contexts = frames.worker_contexts(n_workers)
    sections = (frames.ref_sec, frames.mov_sec)
    builders = [[_TableBuilder(j, sections, with_ref_idx) for _ in range(n_workers)] for j in jobs]
    lock = threading.Lock()
    cut = [len(job.todo) * q // n_workers for q in range(n_workers + 1)]
    device_table = builders[0][0].device_columns_possible() and os.environ.get("SAME_TABLE_COLUMNS", "device") != "host"
    accs, extra = None, []
    stats = [{} for _ in jobs]
    try:
        if not with_ref_idx and (merge or device_table):
            # set 0 takes the frames' own accumulators (which also puts the id codes on the device), every other set a set of its own
            accs = [_begin_accumulators(job, frames, contexts, cut, None)]
            for _j in jobs[1:]:
                mine = [MergeAccumulator(c) for c in contexts]
                extra.extend(mine)
                for q, acc in enumerate(mine):
                    acc.begin(sum(w["n_mov"] for _pos, w in job.todo[cut[q]:cut[q + 1]]))
                accs.append(mine)
        if priority:
            frames.label_codes_on_device()
        pos_of = {id(w): pos for pos, w in job.todo}
        sets = [(j.optim_params["knn"], j.mode, j.optim_params["no_match_penalty"]) for j in jobs]

        def walk(q):
            mine = [w for _p, w in job.todo[cut[q]:cut[q + 1]]]
            collector = None
            if accs is not None:
                collector = lambda states, windows, s: accs[s][q].collect(states, [w["trim"] for w in windows],
                                                                          [w["window_id"] for w in windows],
                                                                          [pos_of[id(w)] for w in windows])
            for dw in frames.windows(mine, ctx=contexts[q], triangulator=triangulator, collector=collector, batch=batch,
                                     priority=priority, sets=sets):
                s, pos = dw.set, pos_of[id(dw.window)]
                if dw.error is not None:
                    raise _window_error(dw, jobs[s].optim_params)
                if accs is None:
                    builders[s][q].add(pos, dw.window, dw, _device_ref_idx(dw) if with_ref_idx else None)
                rec = _device_stats(dw)
                with lock:
                    stats[s][pos] = rec

        if n_workers == 1:
            walk(0)
        else:
            errors = []

            def guarded(q):
                try:
                    walk(q)
                except BaseException as e:   # noqa: BLE001 -- re-raised in the calling thread below
                    errors.append(e)

            threads = [threading.Thread(target=guarded, args=(q,), name=f"same-sweep-{q}") for q in range(n_workers)]
            [t.start() for t in threads]
            [t.join() for t in threads]
            if errors:
                raise errors[0]
        out = []
        for s, j in enumerate(jobs):
            table = _route_table(j, frames, builders[s], None if accs is None else accs[s], merge, None, device_table)
            out.append((table, [stats[s][pos] for pos in sorted(stats[s])]) if return_stats else table)
        return out
    finally:
        for acc in extra:
            acc.close()
