"""A list of parameter sets over ONE pass of the windows: `sliding_window_sweep`.

`sliding_window_incumbent` is what a caller tries parameters with before a licensed solve is paid for, and such a search is a sweep:
several values of `knn` at one penalty, several penalties at one `knn`, the starts and the searches, always over the same two frames.
As single jobs every point stages and triangulates every window again, although none of these keys changes a window's triangulation:

* the prune keeps an aligned row when ANY reference lies within `radius`: the kept rows, and the points triangulated, do not depend on `knn`;
* a row's pairs are ordered by (squared distance, reference row), a total order: the list at k' < k is every row's first min(k', count)
  pairs of the list at k (csrc/window_knn_prefix.hip derives it on the device);
* the penalties, the start and the search are read by the finish call alone (`WindowMode`).

A CALLER's triangulation -- MetaCell objects bring theirs, which is what the reference's own sweep scripts pass -- shares as much under
optim_params["hip_caller_delaunay"] = "device": which of the caller's triangles are a window's, the filter's node mask, the unconstrained
nodes that go and the renumbering of the rest are read off the kept rows and their XY, none of which depends on `knn`; the removal takes
whole rows of pairs and the prefix cuts every row, so the two commute.  Only the pair list behind the mask is made again per `knn`
(csrc/window_caller.hip: same_window_caller_pairs).

So the sweep stages every window once at the largest `knn`, triangulates it once -- or selects the caller's triangles once -- and finishes
it once per set (windows.iter_device_windows with `sets`).  `sliding_window_sweep(...)[i]` is `sliding_window_incumbent` under
{**optim_params, **param_sets[i]}: table, dtypes, row order, stats.  It is that function's own device route, too: a single job is a
sweep of one set, and `incumbent._device_pass` walks the windows for either -- this module checks the sets, makes a job per set and
shapes the result."""
from .incumbent import _device_pass, sliding_window_incumbent
from .window_api import ResidentFrames, _WindowJob
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
                         window_local_indices=False, return_stats=False, triangulator=None, ctx=None, merge=False, batch=None,
                         moving_delaunay=None, moving_delaunay_vertex_col=None):
    """`sliding_window_incumbent` for every parameter set of `param_sets` over one pass of the windows.
    -> [table per set, in param_sets order] (with return_stats: [(table, [per-window stats dict in plan order]) per set]).
    `optim_params` is what the sets share; each set is a dict of overrides drawn from SWEEP_KEYS.  Any other key in a set, an empty list
    or a set `WindowMode.from_params` refuses raises ValueError before a window job or a device is touched.
    Result i is `sliding_window_incumbent(ref, moving, commonCT, optim_params={**optim_params, **param_sets[i]}, ...)` with the same
    `gurobi_params`, `workers`, `window_local_indices`, `triangulator`, `ctx`, `merge`, `batch`, `moving_delaunay` and
    `moving_delaunay_vertex_col` -- table, dtypes, row order and stats -- on every triangulation route (optim_params["hip_delaunay"]),
    with and without hip_priority_prune="device", merged or not (one merge accumulator per set).  Every window is staged once at the
    sets' largest knn and triangulated once, then finished once per set.  `ref` / `moving` may be a `resident_frames` object.
    A caller's triangulation -- MetaCell objects, `moving_delaunay=` -- shares the pass under optim_params["hip_caller_delaunay"] =
    "device", where the device route takes these inputs (window_api.caller_triangulation_refusal): per batch the caller's triangles are
    selected and the unconstrained nodes removed ONCE, at the largest knn, and per further knn the cut pair lists go through the node
    masks the windows hold (windows.caller_pairs_windows).  `max_matches` and `ref_metacell_match_multiplier` stay sweepable there.
    Inputs that do not take the device route -- a caller's triangulation without that key or refused by it, ignore_knn_if_matched
    without hip_priority_prune="device", frames the device sections refuse -- are run set by set through `sliding_window_incumbent`:
    the same results, nothing shared.  (An `outprefix` and sweeps over ranks are not offered here.)"""
    checked = _checked_sets(param_sets, optim_params, gurobi_params, moving)
    new_job = lambda op, mode, **kw: _WindowJob(ref, moving, commonCT, None, moving_delaunay, moving_delaunay_vertex_col, op, gurobi_params,
                                                False, None, mode=mode, **kw)
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
    caller_route = caller_delaunay_route(op0)
    frames, own = job.device_frames(None, ctx=ctx)
    shared_pass = frames is not None and not job.caller_triangulation and not host_prune
    caller = None
    try:
        if frames is not None and job.caller_triangulation and caller_route == "device" and not host_prune:
            # the caller's triangulation resident beside the moving section, as sliding_window_incumbent keeps it -- unless the device
            # route refuses these inputs (window_api.caller_triangulation_refusal): then every set takes the general route
            caller = frames.caller_tris(job.moving_delaunay, job.vertex_col)
            shared_pass = caller is not None
        if shared_pass:
            if triangulator is None and caller is None:
                from . import delaunay

                triangulator = delaunay.triangulator_for(op0)
            done = _device_pass(jobs, frames, workers, window_local_indices, triangulator, merge, None, batch, caller, priority)
            return [(table, [stats[pos] for pos in sorted(stats)]) if return_stats else table for table, stats in done]
    finally:
        if own and frames is not None:
            frames.close()
    # set by set: the general route, nothing shared
    return [sliding_window_incumbent(ref, moving, commonCT, moving_delaunay=moving_delaunay,
                                     moving_delaunay_vertex_col=moving_delaunay_vertex_col, optim_params=op, gurobi_params=gurobi_params,
                                     workers=workers, window_local_indices=window_local_indices, return_stats=return_stats,
                                     triangulator=triangulator, ctx=ctx, merge=merge, batch=batch) for op, _mode in checked]
