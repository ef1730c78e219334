"""Type-matrix variants of the moving frame over ONE pass of the windows: `sliding_window_variants`.

A robustness study (the reference's Fig. S5 script) runs the same two frames several times with noise injected into the moving frame's
`commonCT` columns and nothing else changed -- `cell_type` is taken before the noise, so it stays.  As single jobs every run stages,
prunes, compacts and triangulates every window again, although of everything a window is made of only the pair costs read those columns:

* the kept rows and the pair lists are geometry (csrc/knn.hip);
* the triangle filter and the cell-type-priority prune read `cell_type` CODES and XY;
* the reference limits read sizes;
* the type columns enter the candidate costs (csrc/cost.hip) and, afterwards, the table's `commonCT` columns.

So a list of type matrices shares one pass as a list of parameter sets does (sweep.py): every window is staged and triangulated once --
or has the caller's triangles selected once --, and per variant ONE device call prices the staged pair lists again from the variant's
matrix (csrc/window_recost.hip), after which the window is finished as under `sliding_window_incumbent` / `sliding_window_sweep`.  This
module checks the variants, makes a job per (variant, set) for `incumbent._device_pass` and shapes the result."""
import copy

import numpy as np
import pandas as pd

from .incumbent import _device_pass, sliding_window_incumbent
from .sweep import _checked_sets, sliding_window_sweep
from .window_api import ResidentFrames, _WindowJob
from .window_mode import WindowMode, caller_delaunay_route, priority_prune_route


def _frames_of(ref, moving):
    """-> (ref, moving) as the caller made them (a `resident_frames` object names both), and the two DataFrames behind them"""
    resident = ref if isinstance(ref, ResidentFrames) else moving if isinstance(moving, ResidentFrames) else None
    ref = resident.ref_arg if isinstance(ref, ResidentFrames) else ref
    moving = resident.moving_arg if isinstance(moving, ResidentFrames) else moving
    return ref, moving, getattr(ref, "metacell_df", ref), getattr(moving, "metacell_df", moving)


def _common_types(ref, moving, ref_df, mov_df, commonCT):
    """commonCT as `_WindowJob` settles it (src/same.py:437-470): the caller's, or the sorted labels of the reference's cell-type column"""
    if commonCT is not None:
        return list(commonCT)
    ref_col, mov_col = getattr(ref, "cell_type_col", "cell_type"), getattr(moving, "cell_type_col", "cell_type")
    if ref_col not in ref_df.columns or mov_col not in mov_df.columns:
        raise ValueError("commonCT is None, but cell_type columns were not found to infer it. Pass commonCT explicitly.")
    return sorted(set(pd.Series(ref_df[ref_col]).dropna().unique().tolist()))


def _checked_list(type_variants):
    """ValueError unless `type_variants` is a non-empty list (or tuple) of variants"""
    if not isinstance(type_variants, (list, tuple)) or len(type_variants) == 0:
        raise ValueError("type_variants must be a non-empty list of None, (rows, commonCT) arrays or DataFrames, not "
                         f"{type(type_variants).__name__}" + (" (empty)" if isinstance(type_variants, (list, tuple)) else ""))


def _checked_variants(type_variants, n_rows, cts):
    """-> [None or the variant as a C-contiguous float64 (n_rows, len(cts)) matrix]; ValueError for anything an entry may not be"""
    out = []
    for q, v in enumerate(type_variants):
        if v is None:
            out.append(None)
            continue
        if isinstance(v, pd.DataFrame):
            missing = [c for c in cts if c not in v.columns]
            if missing:
                raise ValueError(f"type_variants[{q}] lacks the commonCT columns {missing[:20]}")
            v = v[cts]                    # rows by position: the index is not read
        try:
            m = np.ascontiguousarray(v.to_numpy() if isinstance(v, pd.DataFrame) else v, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"type_variants[{q}] is not convertible to float64: {e}") from None
        if m.shape != (n_rows, len(cts)):
            raise ValueError(f"type_variants[{q}] has shape {m.shape}; the moving frame has {n_rows} rows and commonCT {len(cts)} columns")
        out.append(m)
    return out


def moving_variant(moving, commonCT, types):
    """`moving` with its commonCT columns replaced: a copy of the frame in which column commonCT[t] is float64 `types`[:, t] -- for a
    MetaCell object a shallow copy of the object over such a copy of its `.metacell_df`.  What result v of `sliding_window_variants` is
    the stand-alone job of."""
    if hasattr(moving, "metacell_df"):
        out = copy.copy(moving)
        out.metacell_df = moving_variant(moving.metacell_df, commonCT, types)
        return out
    out = moving.copy()
    types = np.asarray(types, dtype=np.float64)
    for t, c in enumerate(commonCT):
        out[c] = types[:, t]
    return out


def sliding_window_variants(ref, moving, type_variants, commonCT=None, *, param_sets=None, optim_params=None, gurobi_params=None,
                            workers=None, window_local_indices=False, return_stats=False, triangulator=None, ctx=None, merge=False,
                            batch=None, moving_delaunay=None, moving_delaunay_vertex_col=None, _score=None):
    """`sliding_window_incumbent` -- with `param_sets`: `sliding_window_sweep` -- for every type-matrix variant of the moving frame over one
    pass of the windows.  -> [result per variant, in the order given]: a table (with return_stats: (table, [per-window stats dict in plan
    order])), or with `param_sets` the sweep's list of those per set.
    `type_variants`: a non-empty list; an entry is None (the moving frame as it is), an (n_moving_rows, len(commonCT)) array convertible
    to float64 with its columns in commonCT order, or a DataFrame holding the commonCT columns whose rows align with the moving frame's
    by position (its index is ignored).  For MetaCell objects the rows are those of `.metacell_df`.
    Result v is what the existing functions give for `moving_v` = `moving_variant(moving, commonCT, variant)` -- table, dtypes, row order
    and stats --: `sliding_window_incumbent(ref, moving_v, commonCT, ...)`, or `sliding_window_sweep(ref, moving_v, param_sets, commonCT,
    ...)`, with the same `optim_params`, `gurobi_params`, `workers`, `window_local_indices`, `triangulator`, `ctx`, `merge`, `batch`,
    `moving_delaunay` and `moving_delaunay_vertex_col`.  `dist_ct_coeff` is shared by all variants.
    A wrong shape, a DataFrame without a commonCT column, an empty list or a dict / str in place of the list raise ValueError before a
    window job or a device is touched; `param_sets` is checked by the sweep's own check.  `ref` / `moving` may be a `resident_frames`
    object: a variant is then uploaded once and kept for that object's life.
    Every window is staged once (at the sets' largest knn) and triangulated once; per batch and variant that is not None one call prices
    the staged pair lists again (windows.recost_windows).  Inputs that do not take the device route -- the ones `sliding_window_sweep`
    lists -- run variant by variant through `sliding_window_incumbent` / `sliding_window_sweep` on `moving_v`: the same results, nothing
    shared.  (An `outprefix` and ranks are not offered here.)
    `_score` (scores.sliding_window_scores' scores.DeviceScores): it is told the job (`_score.job`), and where the pass is shared and
    `_score.prepare(frames, job)` agrees every result is scored on the device (`incumbent._device_pass`); a result is then None unless
    `_score.tables`.  After the last record `_score.finished(frames)` is called while the frames are still resident."""
    _checked_list(type_variants)
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    cts = _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT)
    mats = _checked_variants(type_variants, len(mov_df), cts)
    if param_sets is None:
        checked = [(dict(optim_params or {}), WindowMode.from_params(optim_params, gurobi_params, moving))]
    else:
        checked = _checked_sets(param_sets, optim_params, gurobi_params, moving)
    new_job = lambda op, mode, **kw: _WindowJob(ref, moving, commonCT, None, moving_delaunay, moving_delaunay_vertex_col, op, gurobi_params,
                                                False, None, mode=mode, **kw)
    job = new_job(*checked[0])
    if _score is not None:
        _score.job = job
    kw = {}
    if not isinstance(ref, ResidentFrames) and not isinstance(moving, ResidentFrames):
        # the jobs share window_size, overlap and min_cells: the first job's plan serves the others (this object holds nothing else)
        kw["resident"] = ResidentFrames(ref, moving)
        kw["resident"].plans[(job.window_size, job.overlap, job.optim_params["min_cells_per_window"])] = (job.plan, job.grid)
    op0 = job.optim_params
    priority = bool(op0["ignore_knn_if_matched"]) and priority_prune_route(op0) == "device"
    host_prune = bool(op0["ignore_knn_if_matched"]) and not priority
    frames, own = job.device_frames(None, ctx=ctx)
    shared_pass = frames is not None and not job.caller_triangulation and not host_prune and list(job.commonCT) == cts
    caller = None
    try:
        if frames is not None and job.caller_triangulation and caller_delaunay_route(op0) == "device" and not host_prune:
            caller = frames.caller_tris(job.moving_delaunay, job.vertex_col)
            shared_pass = caller is not None and list(job.commonCT) == cts
        if shared_pass:
            if triangulator is None and caller is None:
                from . import delaunay

                triangulator = delaunay.triangulator_for(op0)
            layers = [None if m is None else frames.types_layer(v, m) for v, m in zip(type_variants, mats)]
            score = _score if _score is not None and _score.prepare(frames, job) else None
            jobs = []
            for v, m in enumerate(mats):            # a job per (variant, set), variants outermost
                for s, (op, mode) in enumerate(checked):
                    j = job if (v, s) == (0, 0) else new_job(op, mode, **kw)
                    j.variant, j.variant_types, j.variant_layer = v, m, layers[v]
                    jobs.append(j)
            done = _device_pass(jobs, frames, workers, window_local_indices, triangulator, merge, None, batch, caller, priority,
                                variants=layers, score=score)
            if score is not None:
                score.records = [j.score_record for j in jobs]
                score.finished(frames)
            res = [(table, [stats[pos] for pos in sorted(stats)]) if return_stats else table for table, stats in done]
            n_sets = len(checked)
            return [res[v * n_sets] if param_sets is None else res[v * n_sets:(v + 1) * n_sets] for v in range(len(mats))]
    finally:
        if own and frames is not None:
            frames.close()
    # variant by variant: the stand-alone calls on moving_v, nothing shared
    shared_kw = dict(optim_params=optim_params, gurobi_params=gurobi_params, workers=workers, window_local_indices=window_local_indices,
                     return_stats=return_stats, triangulator=triangulator, ctx=ctx, merge=merge, batch=batch,
                     moving_delaunay=moving_delaunay, moving_delaunay_vertex_col=moving_delaunay_vertex_col)
    out = []
    for m in mats:
        r_v, m_v = (ref, moving) if m is None else (ref_arg, moving_variant(moving_arg, cts, m))
        out.append(sliding_window_incumbent(r_v, m_v, commonCT, **shared_kw) if param_sets is None
                   else sliding_window_sweep(r_v, m_v, param_sets, commonCT, **shared_kw))
    return out
