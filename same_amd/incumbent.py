"""The window loop without a solver: sliding_window_matching (src/same.py:297-595) with every window's solution taken to be the greedy
MIP start (src/init_helpers.py:104-133) -- the incumbent the reference itself hands Gurobi first -- swept by the lazy-constraint body
(src/same.py:645-669), the XY-order sweep (src/violationhelper.py:53-117) and the area flips (src/same.py:1362-1402), and trimmed
to each window's central region (src/same.py:565-582).  It is the product function for hosts without a Gurobi licence, the first stage
of a two-stage run (the table is what `merge_window_matches_unique_ref` takes) and what `bench.py --workload cfg5` times.

Same arguments as `sliding_window_matching`; the result has its columns wherever they are defined without a solver:

    aligned_idx [ref_idx] <commonCT...> X Y ref_X ref_Y size ref_size Ref_<cell_id_col> Aligned_<cell_id_col> time_limit_reached
    triangle_violation filtered_violation run_time window_id

* `triangle_violation`: the cell is a vertex of a triangle whose signed area flips under the matching (as src/same.py:1464-1469).
* `filtered_violation`: the reference intersects the XY-order sweep's points with the triangles the SOLVER penalised
  (src/same.py:1411-1432); without a solver there are no penalties, and the column carries the sweep's own per-cell flag -- the
  ranking key the window merge sorts by (src/helpers.py:745-753) keeps its meaning: unflagged proposals of a pair win.
* `ref_idx` (index in the window's compacted reference frame) needs the window's pair list on the host and is only made on request
  (`window_local_indices=True`); `aligned_idx` is free.  `run_time` is 0.0, `time_limit_reached` False.

Several parameter sets over the same frames -- a sweep of `knn`, of the penalties, of the start and the search -- are ONE pass of the
windows through `same_amd.sliding_window_sweep` (sweep.py): every window is staged and triangulated once and finished once
per set, and each set's table and stats are this function's -- made by this module's one device route (`_device_pass`), to which a
single job is a sweep of one set.

optim_params["hip_incumbent"] = "assignment" (opt-in; "greedy" is the default) takes each window's OPTIMAL one-to-one assignment
instead: the reference's Hungarian start (src/init_helpers.py:135-175) on its sparse form, without `init_hungarian_max_n`, solved on the
GPU (csrc/assign.hip).  It needs max_matches == 1 and every no-match cost below init_big_m / 2 (`incumbent_mode`).  With
return_stats each window's stats then carry its `objective` and `fallback` (the device's certificate refused it; scipy answered).

optim_params["hip_refine"] = "local" (opt-in; without the key or with None nothing changes) runs a local search on the GPU after
either incumbent and before the sweeps (csrc/refine.hip).  It lowers each window's full lazy-model objective
(src/same.py:1191-1196): pair costs + no_match_penalty * size per unmatched cell + delaunay_penalty * the size sum of every kept triangle
the lazy body (:645-669) sees flip.  Moves: a cell to a free candidate reference, to or from unmatched, two cells swapping references;
rounds of non-overlapping best moves until a round has none or optim_params["hip_refine_rounds"] (default 32) is reached.  The matching
stays one-to-one like both starts, so penalty_coeff's p_j stay 0: with max_matches > 1 the result is still a feasible solution of the
model, one that leaves reference capacity unused.  The table, `flipped` and the flag columns describe the refined matching; with
return_stats each window's stats gain `mip_objective_start`, `mip_objective` (the model's objective before and after), `refine_rounds`,
`refine_moves` and `refine_settled` (0: stopped at the round cap); `objective` stays the assignment's.

optim_params["hip_refine"] = "capacity" is the same search within the model's reference capacities (src/helpers.py:102-161,
`api.ref_match_limits`): reference j of a window may take up to max_matches * ref_metacell_match_multiplier cells when the window's
reference frame holds metacells and j is one (the multiplier None: the frame's largest size), else max_matches, at most 1001; every match
after a reference's first costs penalty_coeff, so the objective gains penalty_coeff * sum_j max(0, count_j - 1).  Moves go to references
with room.  With every limit 1 it is "local" bit for bit.  The stats also carry `ref_extra_matches` (sum_j max(0, count_j - 1) of the
result), and both objectives include the penalty_coeff term.  The "greedy" and "assignment" starts stay one-to-one.

optim_params["hip_incumbent"] = "transport" (opt-in) is the start that uses those capacities: the model WITHOUT its triangle term,
solved to its optimum on the GPU (csrc/assign.hip) -- every cell takes one of its pairs or stays unmatched, reference j takes
at most limit_j cells, each after its first priced penalty_coeff.  Any max_matches >= 1; with every limit 1 it is "assignment" bit for
bit.  Its `objective` is a lower bound on the window's full lazy model (delaunay_penalty * w_t * q_t >= 0), so with
hip_refine="capacity" on top the stats carry `mip_gap` = (mip_objective - objective) / |mip_objective|: how far the refined window can be
from optimal.  The stats also carry `ref_extra_matches_start`, `transport_searches` and `fallback` (the certificate refused; the host solved the expanded
graph).  hip_refine="local" does not go with it (that search holds every reference to one match).

optim_params["hip_caller_delaunay"] = "device" (opt-in; without the key, None or "host" nothing changes) keeps a CALLER's triangulation
-- MetaCell objects, `moving_delaunay=` arrays or frames, with or without `moving_delaunay_vertex_col` -- on the device route:
the triangulation is uploaded once as rows of the moving section, and per batch the device selects and remaps every window's triangles
in the caller's order, works out the filter's node mask and removes the unconstrained nodes with their pairs (src/same.py:1016-1085;
csrc/window_caller.hip).  Table and stats are the general route's.  Inputs it refuses
(window_api.caller_triangulation_refusal: ids not unique in the frame, two triangles with one vertex set, ids that are not integers,
ignore_knn_if_matched without hip_priority_prune="device") take the general route as before; `hip_delaunay` is irrelevant there
(nothing is triangulated).

optim_params["hip_priority_prune"] = "device" (opt-in; without the key, None or "host" nothing changes, and without
ignore_knn_if_matched the key means nothing) keeps a job with ignore_knn_if_matched=True -- the cell-type-priority prune,
src/knn_utils.py:5-78 -- on the device route: the frames' `cell_type` labels are coded jointly and uploaded once, and per batch one call
right after the stage call ranks every row's pairs by distance, lets the rows whose nearest reference has their label bid for it (the
lowest row wins and keeps that one pair, every other row keeps all) and compacts the pair list (csrc/window_priority.hip).
Everything behind it -- hip_incumbent, hip_refine, hip_delaunay, hip_caller_delaunay, merge=True, ranks -- sees the smaller list; the
reference limits and `ref_idx` still read the list as staged.  Table and stats are the general route's; `pairs` is the filtered count
and each window's stats gain `pairs_staged`, `priority_rows` (rows that kept one pair) and `keep_all_rows`.

Two routes produce the same table (tests/test_gpu_run_same.py::test_incumbent_table_routes_agree):
  device   both frames resident on the GPU, two library calls per window, the incumbent and the sweeps computed where the pairs are
           (csrc/window_stage.hip, csrc/window_finish.hip); the host triangulates, receives (match, flags) per window, keeps its matched
           central cells as `windows.FINAL_RECORD`s (what the device's accumulator holds of them) and gathers the table's columns ONCE at the end.  Windows are walked by `workers` threads with a context each.
  general  every window becomes a `PreparedInputs` (either pipeline of same_amd.api) and the incumbent + sweeps run through the
           host-buffer entry points: caller-supplied triangulations (MetaCell inputs) without hip_caller_delaunay="device", the
           cell-type-priority filter without hip_priority_prune="device", inputs the sections cannot hold.
"""
import os
import threading

import numpy as np
import pandas as pd

from . import ops
from ._trace import stage
from .api import _Staged, prepare_same_inputs, ref_match_limits
from .ops import MAX_REF_LIMIT          # noqa: F401  (the bound of every reference's match limit, "capacity" and "transport")
from .window_api import _WindowJob, _walk_windows, _window_error
from .window_mode import (INCUMBENTS, REFINE_ROUNDS, REFINES, WindowMode, caller_delaunay_route, incumbent_mode,  # noqa: F401
                          priority_prune_route, refine_mode, transport_capacity)
from .windows import FINAL_RECORD, MergeAccumulator

STAT_KEYS = ("pairs", "triangles", "checked", "flipped", "xy_violations", "area_flips", "matched")


def _default_workers():
    from . import qhull_pool

    share = qhull_pool.cpu_budget() / qhull_pool.cpu_sharers()[0]
    return 2 if share >= 8 else 1       # a second Python thread only pays where there are CPUs to feed it


class _TableBuilder:
    """The device route's result table.  As the windows come a builder keeps, per window, one `windows.FINAL_RECORD` per matched cell inside
    the central trim -- the form in which the device's accumulator hands the same rows back; the columns are gathered from the caller's
    frames ONCE, when the pass is over, by `gather()`:
    the final columns are allocated at their full length and filled slice by slice on `GATHER_THREADS` threads (numpy copies without the
    interpreter lock; the Qhull helpers are idle by then) -- no per-window frames, no concatenation.  Where the frame's own columns are
    float64 (the usual case) the type columns and the coordinates come from the sections' row-major copies: a slice's rows are fetched as
    whole rows (one cache line per row instead of one per column) and laid out as columns while they are in cache."""

    SLICE = 16384        # rows per task: a slice's row-major block of type columns stays in L2 between its gather and its split

    def __init__(self, job, sections, with_ref_idx):
        ref, mov = job.ref, job.moving
        self.job, self.with_ref_idx = job, with_ref_idx
        self.cts, self.cid = list(job.commonCT), job.optim_params["cell_id_col"]
        f64 = np.dtype(np.float64)
        # a frame's column may be a strided view of its block (a frame made from a 2-D array): np.take would copy such a source whole on
        # EVERY call, so the 1-D sources are made contiguous here, once per job (no copy where they already are)
        col = lambda df, c: np.ascontiguousarray(df[c].to_numpy())
        distinct = len(set(self.cts)) == len(self.cts)
        # a type-matrix variant of the moving frame (variants.py): the job's type columns are the variant's -- float64, column t under
        # commonCT[t] (a name listed twice holds its last column) -- and on the device its layer's
        variant, self.layer = getattr(job, "variant_types", None), getattr(job, "variant_layer", None)
        if variant is None:
            plain_types = all(mov[c].dtype == f64 for c in self.cts) and distinct
            self.type_block = sections[1].types if plain_types else None
            self.type_cols = None if self.type_block is not None else [col(mov, c) for c in self.cts]
        else:
            self.type_block = variant if distinct else None
            self.type_cols = None if distinct else [np.ascontiguousarray(variant[:, len(self.cts) - 1 - self.cts[::-1].index(c)])
                                                    for c in self.cts]
        both_xy = all(df[c].dtype == f64 for df in (ref, mov) for c in ("X", "Y"))
        self.mov_xy, self.ref_xy = (sections[1].xy, sections[0].xy) if both_xy else (None, None)
        self.xy_cols = None if both_xy else ([col(mov, c) for c in ("X", "Y")], [col(ref, c) for c in ("X", "Y")])
        self.mov_size = col(mov, "size") if "size" in mov.columns else None
        self.ref_size = col(ref, "size") if "size" in ref.columns else None
        self.ref_id, self.mov_id = col(ref, self.cid), col(mov, self.cid)
        self.parts, self.ref_idx = [], []        # per window: its records; with_ref_idx: the rows' indices in its compacted reference frame

    def add(self, pos, w, dw, ref_idx=None):
        x, y = dw.axy[:, 0], dw.axy[:, 1]
        tx0, tx1, ty0, ty1 = w["trim"]                                  # central region (src/same.py:565-582), matched cells only
        c = np.flatnonzero((dw.match_row >= 0) & (x >= tx0) & (x < tx1) & (y >= ty0) & (y < ty1))
        rec = np.empty(len(c), FINAL_RECORD)
        rec["a_row"], rec["r_row"], rec["cidx"], rec["wid"], rec["pos"] = dw.rows_m[c], dw.match_row[c], c, w["window_id"], pos
        rec["flags"] = dw.point_flag[c] | dw.flip_flag[c] << 1          # the accumulator's bits: 1 the XY-order flag, 2 the area flip
        self.parts.append(rec)
        if self.with_ref_idx:
            self.ref_idx.append(ref_idx[c])

    @staticmethod
    def rows(builders):
        """The builders' windows laid end to end (each builder walked a contiguous run of the plan, so this is plan order) -> (their
        FINAL_RECORDs, with_ref_idx: the rows' `ref_idx`, else None)."""
        cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dt)
        return (cat([p for b in builders for p in b.parts], FINAL_RECORD),
                cat([r for b in builders for r in b.ref_idx], np.int64) if builders[0].with_ref_idx else None)

    @staticmethod
    def table(builders, select=None, plan_pos=None):
        """The table of `rows(builders)`; `select`: of these rows only, in this order (the rows the window merge keeps: the other rows'
        columns are never gathered)."""
        me = builders[0]                 # the sources are the job's: the same for every builder
        rows, ref_idx = _TableBuilder.rows(builders)
        if select is not None:
            rows, ref_idx = rows[select], ref_idx if ref_idx is None else ref_idx[select]
        return me.gather(rows, ref_idx, me.job.mine is not None if plan_pos is None else plan_pos)

    def gather(self, rows, ref_idx=None, with_pos=False, only=None):
        """The result table of the matched cells `rows` (FINAL_RECORDs: moving section row -> reference section row, the cell's index in its
        window, window id, plan position, flag bits): the columns of src/same.py:1264-1278, :1464-1470, gathered from the caller's frames
        slice by slice on the gather threads.  No rows: the empty frame.
        only: gather just these table columns (-> dict of arrays): the ones the device-side gather of `table_from_device` does not cover."""
        from concurrent.futures import ThreadPoolExecutor

        from .merge import GATHER_THREADS

        me, n = self, len(rows)
        if n == 0 and only is None:
            return pd.DataFrame()
        ra, rr = rows["a_row"].astype(np.int64), rows["r_row"].astype(np.int64)      # contiguous index arrays, made once
        want = (lambda name: True) if only is None else (lambda name: name in only)
        xy_names = ("X", "Y", "ref_X", "ref_Y")
        # from the sections' row-major blocks: the type columns, the coordinates; column by column (column, its source, the rows to take
        # of it) whatever has no block.  A frame without `size` is no source: `_result_frame` says what the column holds then.
        block_types = me.type_block is not None and any(want(ct) for ct in me.cts)
        block_xy = me.mov_xy is not None and any(want(k) for k in xy_names)
        singles = [("size", me.mov_size, ra), ("ref_size", me.ref_size, rr), (f"Ref_{me.cid}", me.ref_id, rr),
                   (f"Aligned_{me.cid}", me.mov_id, ra)]
        if me.type_block is None:
            singles += [(ct, col, ra) for ct, col in zip(me.cts, me.type_cols)]
        if me.mov_xy is None:
            singles += zip(xy_names, me.xy_cols[0] + me.xy_cols[1], (ra, ra, rr, rr))
        singles = [(k, src, rows_of) for k, src, rows_of in singles if want(k) and src is not None]
        out = {k: np.empty(n, src.dtype) for k, src, _rows_of in singles}
        out.update({k: np.empty(n, np.float64) for k in (me.cts if block_types else []) + (list(xy_names) if block_xy else [])})

        def fill(lo):
            hi = min(n, lo + _TableBuilder.SLICE)
            a, r = ra[lo:hi], rr[lo:hi]
            # np.take(src, rows, axis=0) copies whole rows: 3-6x the speed of src[rows] on the (n, 8) / (n, 2) blocks
            take = np.take
            if block_types:
                block = take(me.type_block, a, axis=0)       # (rows, T): the commonCT columns in commonCT order
                for q, ct in enumerate(me.cts):
                    out[ct][lo:hi] = block[:, q]
            if block_xy:
                axy, rxy = take(me.mov_xy, a, axis=0), take(me.ref_xy, r, axis=0)
                out["X"][lo:hi], out["Y"][lo:hi], out["ref_X"][lo:hi], out["ref_Y"][lo:hi] = axy[:, 0], axy[:, 1], rxy[:, 0], rxy[:, 1]
            for k, src, rows_of in singles:
                take(src, rows_of[lo:hi], out=out[k][lo:hi], mode="clip")       # (valid rows: "clip" only spares numpy its bounce buffer)

        starts = range(0, n, _TableBuilder.SLICE)
        if len(starts) == 1 or not out:
            fill(0)
        else:
            with ThreadPoolExecutor(max_workers=GATHER_THREADS) as pool:
                list(pool.map(fill, starts))
        if only is not None:
            return out
        flags = rows["flags"]
        out.update({"aligned_idx": rows["cidx"].astype(np.int64), "ref_idx": ref_idx, "triangle_violation": (flags & 2) != 0,
                    "filtered_violation": (flags & 1) != 0, "window_id": rows["wid"].astype(np.int64),
                    "__plan_pos": rows["pos"].astype(np.int64)})
        return _result_frame(out, n, me.cts, me.cid, ref_idx is not None, with_pos)

    def device_columns_possible(self):
        """the frame's type columns and coordinates are float64 and the type columns distinct: the sections hold exactly their values"""
        return self.type_block is not None and self.mov_xy is not None

    def table_from_device(self, frames, acc, with_plan_pos=False):
        """The merged table with its columns gathered where the sections are: the DEVICE writes the type columns, X, Y, ref_X, ref_Y, the
        8-byte id / size columns of the frames, aligned_idx, window_id and the two flag columns of the final rows straight into a pooled
        page-locked host block (MergeAccumulator.columns); the table's arrays are views of it.  Columns the device cannot hold (ids that
        are strings ...) are gathered by the host meanwhile.  None: no block to be had -- the caller gathers on the host."""
        n = acc.n_final
        with stage("table: page-locked block + the device's gather enqueued"):
            extra = frames.table_columns(self.cid)
            got = acc.columns(frames.dmov, frames.dref, n, len(self.cts), [b for _n, b, _d in extra["mov"]],
                              [b for _n, b, _d in extra["ref"]], layer=self.layer)
        if got is None:
            return None
        wide, flags = got
        names = (list(self.cts) + ["X", "Y", "ref_X", "ref_Y"] + [nm for nm, _b, _d in extra["mov"] + extra["ref"]]
                 + ["aligned_idx", "window_id", "__plan_pos"])
        dtypes = [np.float64] * (len(self.cts) + 4) + [d for _n, _b, d in extra["mov"] + extra["ref"]] + [np.int64, np.int64, np.int64]
        missing = {"size", "ref_size", f"Ref_{self.cid}", f"Aligned_{self.cid}"} - set(names)
        # beside the device's gather (which was only enqueued)
        host = self.gather(acc.final_rows(), only=missing) if missing else {}
        with stage("table: wait for the device's columns"):
            acc.ctx.sync()
        with stage("table: the frame over the block"):
            cols = {nm: wide[q].view(dt) for q, (nm, dt) in enumerate(zip(names, dtypes))}
            cols.update(host, triangle_violation=flags[0].view(bool), filtered_violation=flags[1].view(bool))
            return _result_frame(cols, n, self.cts, self.cid, with_pos=with_plan_pos)


def incumbent_of_prepared(prep, commonCT, with_ref_idx=True, ctx=None, use_device=True, mode=None):
    """(match table of ONE window as run_same's post-solve builds it, stats) from its pre-MIP artefacts, through the host-buffer entry
    points: greedy start -> matching -> lazy-constraint body, XY-order sweep, area flips.  The general route of this module.
    use_device: a PreparedInputs made by the device-resident window path with its pair list untouched carries the incumbent and the
    sweeps already (computed where the pairs are, by same_window_filter_finish): take them instead of computing them again.
    `mode`: a WindowMode (None: the greedy start alone).  Its start through ops.sparse_assign / ops.sparse_transport, its search
    through ops.refine_matching / ops.refine_matching_cap with the reference limits of prep.ref_df (api.ref_match_limits); the stats
    carry the keys the module text lists for the start and the search."""
    mode = WindowMode.default() if mode is None else mode
    op = prep.optim_params
    dw = getattr(prep, "device", None)
    if use_device and dw is not None and dw.match_row is not None and isinstance(prep.valid_pairs, np.ndarray):
        return _table_of_device_window(prep, dw, commonCT, with_ref_idx)
    pairs = np.ascontiguousarray(np.asarray(prep.valid_pairs, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
    costs, n_a, n_r = prep.costs_array, prep.n_aligned, prep.n_ref
    a_df, r_df, tris = prep.aligned_df, prep.ref_df, prep.triangles_array
    size = a_df["size"].to_numpy(dtype=np.float64)
    unmatched = float(op["no_match_penalty"]) * size
    start = search = None
    if mode.incumbent == "assignment":
        pair_of_row, start = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r, ctx=ctx)
    elif mode.incumbent == "transport":
        pair_of_row, st = ops.sparse_transport(pairs, costs, unmatched, n_a, n_r, _ref_limits(r_df, mode.capacity), mode.capacity[2],
                                               ctx=ctx)
        start = {"objective": st["objective"], "fallback": st["fallback"], "rounds": st["rounds"],
                 "ref_extra_matches_start": st["ref_extra_matches"]}       # (the device route's names: windows._assignment_fallback)
    else:
        wants = ops.pair_rowmin(pairs, costs, n_a, ctx=ctx) < unmatched     # src/init_helpers.py:104,118-122
        pair_of_row, _rounds = ops.greedy_match(pairs, costs, n_a, n_r, wants, ctx=ctx)
    axy, rxy = a_df[["X", "Y"]].to_numpy(dtype=np.float64), r_df[["X", "Y"]].to_numpy(dtype=np.float64)
    t32 = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    if mode.refine is not None:
        problem, (rounds, dp) = (pairs, costs, unmatched, n_a, n_r, t32, axy, rxy, size), mode.search_args
        if mode.refine == "capacity":
            pair_of_row, search = ops.refine_matching_cap(*problem, dp, _ref_limits(r_df, mode.capacity), mode.capacity[2], rounds,
                                                          pair_of_row, ctx=ctx)
        else:
            pair_of_row, search = ops.refine_matching(*problem, dp, rounds, pair_of_row, ctx=ctx)
    ai = np.flatnonzero(pair_of_row >= 0)
    ri = pairs[pair_of_row[ai], 1].astype(np.int64)
    match = np.full(n_a, -1, np.int32)
    match[ai] = ri
    sw = ops.BoundSweep(t32, prep.signs_array.astype(np.int8), rxy, n_a, ctx=ctx)
    try:
        checked, viol = sw.sweep_match(match)
    finally:
        sw.close()
    _edge, _tflag, pflag, counts = ops.xyorder_sweep(axy, rxy, t32, match, ctx=ctx)
    _before, _after, _m3, flipped = ops.area_flip(axy, rxy, t32, match, ctx=ctx)
    flip_node = np.zeros(n_a, bool)
    if len(t32):
        flip_node[t32[flipped.astype(bool)].reshape(-1)] = True
    stats = {"pairs": len(pairs), "triangles": len(t32), "checked": int(checked), "flipped": len(viol), "xy_violations": int(counts[1]),
             "area_flips": int(np.count_nonzero(flipped)), "matched": len(ai), **_mode_stats(mode, start, search)}
    return _window_table(prep, commonCT, ai, ri, flip_node, pflag, with_ref_idx), stats


def _ref_limits(r_df, capacity):
    """the model's match limit of every reference of a window's frame (api.ref_match_limits), at most MAX_REF_LIMIT, int32"""
    mm, mult, _pc = capacity
    return np.minimum(np.asarray(ref_match_limits(r_df, mm, mult), dtype=np.float64), MAX_REF_LIMIT).astype(np.int32)


def mip_gap(mip_objective, bound):
    """(mip_objective - bound) / max(|mip_objective|, tiny): how far a refined window is from the transport optimum, which bounds the
    full lazy model from below (the triangle term is >= 0 and the start solves the model's own capacities)"""
    return (float(mip_objective) - float(bound)) / max(abs(float(mip_objective)), np.finfo(np.float64).tiny)


def _match_table(a_df, r_df, ra, rr, commonCT, cid, aligned_idx, ref_idx, triangle_violation, filtered_violation):
    """run_same's post-solve match table (src/same.py:1264-1278, :1464-1470): the columns of the matched cells read from `a_df` / `r_df`
    at rows `ra` / `rr` -- a window's own two frames at its own indices, or the CALLER's frames at section rows (the same values: a
    window's frames are rows of the caller's).  Plain indexing: a frame's column may be a strided view of its block, which np.take would
    first copy whole."""
    cols = {"aligned_idx": aligned_idx.astype(np.int64), "ref_idx": None if ref_idx is None else ref_idx.astype(np.int64)}
    for ct in list(commonCT) + ["X", "Y"]:
        cols[ct] = a_df[ct].to_numpy()[ra]
    for ct in ("X", "Y"):
        cols[f"ref_{ct}"] = r_df[ct].to_numpy()[rr]
    cols["size"] = a_df["size"].to_numpy()[ra] if "size" in a_df.columns else None
    cols["ref_size"] = r_df["size"].to_numpy()[rr] if "size" in r_df.columns else None
    cols[f"Ref_{cid}"] = r_df[cid].to_numpy()[rr]
    cols[f"Aligned_{cid}"] = a_df[cid].to_numpy()[ra]
    cols["triangle_violation"] = np.asarray(triangle_violation).astype(bool)
    cols["filtered_violation"] = np.asarray(filtered_violation).astype(bool)
    return _result_frame(cols, len(ra), commonCT, cid, ref_idx is not None)


def _result_frame(cols, n, cts, cid, with_ref_idx=False, with_pos=False):
    """The result table of `n` rows over the arrays `cols` (by column name): the one statement of its column order (module text) and of
    the columns that are constant without a solver.  No `size` / `ref_size` (absent or None): the frame has no sizes and every cell counts
    1 (src/same.py:934-940).  No `window_id`: one window's table, which the caller stamps."""
    size = lambda k: cols[k] if cols.get(k) is not None else np.ones(n, np.int64)
    out = {"aligned_idx": cols["aligned_idx"]}
    if with_ref_idx:
        out["ref_idx"] = cols["ref_idx"]
    for k in list(cts) + ["X", "Y", "ref_X", "ref_Y"]:
        out[k] = cols[k]
    out["size"], out["ref_size"] = size("size"), size("ref_size")
    out[f"Ref_{cid}"], out[f"Aligned_{cid}"] = cols[f"Ref_{cid}"], cols[f"Aligned_{cid}"]
    out["time_limit_reached"] = np.zeros(n, bool)
    out["triangle_violation"], out["filtered_violation"] = cols["triangle_violation"], cols["filtered_violation"]
    out["run_time"] = np.zeros(n)
    if "window_id" in cols:
        out["window_id"] = cols["window_id"]
    if with_pos:
        out["__plan_pos"] = cols["__plan_pos"]
    return pd.DataFrame(out, copy=False)      # the columns are the caller's own arrays: no consolidating copy


def _window_table(prep, commonCT, ai, ri, flip_node, pflag, with_ref_idx):
    """the table of matched aligned rows `ai` -> reference rows `ri` of the window's own (compacted) frames"""
    return _match_table(prep.aligned_df, prep.ref_df, ai, ri, commonCT, prep.optim_params["cell_id_col"], ai, ri if with_ref_idx else None,
                        flip_node[ai], pflag[ai])


def _table_of_device_window(prep, dw, commonCT, with_ref_idx):
    """The window's table from what the device left.  The columns are read from the CALLER's frames by section row (prep.rows_m, the
    matched reference's section row), so the window's own two frames -- rows of the caller's, made on first access -- are never made."""
    ai = np.flatnonzero(dw.match_row >= 0)
    rj = dw.match_row[ai].astype(np.int64)                    # section rows of the matched reference cells
    stats = _device_stats(dw)
    # rows_r (ascending section rows of the compacted reference frame) -> the compacted index of every matched reference cell
    ri = np.searchsorted(prep.rows_r, rj) if (with_ref_idx or prep.sources is None) else None
    if prep.sources is None:
        return _window_table(prep, commonCT, ai, ri, dw.flip_flag, dw.point_flag, with_ref_idx), stats
    a_src, r_src = prep.sources
    return _match_table(a_src, r_src, np.asarray(prep.rows_m, dtype=np.int64)[ai], rj, commonCT, prep.optim_params["cell_id_col"], ai, ri,
                        dw.flip_flag[ai], dw.point_flag[ai]), stats


def _mode_stats(mode, start, search):
    """what `mode` adds to a window's stats record, on either route: from the record of its start ({"objective", "fallback", "rounds",
    "ref_extra_matches_start"}; None for greedy) and of its search (WindowMode.records; None without one)"""
    rec = {}
    if mode.incumbent != "greedy":
        rec["objective"], rec["fallback"] = start["objective"], start["fallback"]
    if mode.incumbent == "transport":
        rec["ref_extra_matches_start"], rec["transport_searches"] = start["ref_extra_matches_start"], start["rounds"]
    if mode.refine is not None:
        rec.update(mip_objective_start=search["objective_start"], mip_objective=search["objective"], refine_rounds=search["rounds"],
                   refine_moves=search["moves"], refine_settled=search["settled"])
    if mode.refine == "capacity":
        rec["ref_extra_matches"] = search["ref_extra_matches"]
    if mode.incumbent == "transport" and mode.refine is not None:       # the transport start: a bound on the model
        rec["mip_gap"] = mip_gap(rec["mip_objective"], rec["objective"])
    return rec


def _device_stats(dw):
    """a window's stats record (STAT_KEYS) from what the device counted"""
    st = dw.stats
    rec = {"pairs": dw.counts[3], "triangles": dw.n_triangles, "checked": st["checked"], "flipped": st["flipped"],
           "xy_violations": st["xy_violations"], "area_flips": st["area_flips"], "matched": st["matched"],
           **_mode_stats(dw.mode, dw.assignment, dw.refine)}
    if dw.priority is not None:       # the priority prune ran on the device: `pairs` is what it left
        rec["pairs_staged"], _left, rec["priority_rows"], rec["keep_all_rows"] = dw.priority
    return rec


def _device_ref_idx(dw):
    """index of every kept aligned cell's matched reference in the window's COMPACTED reference frame (src/utils.py:734-742), -1 = none"""
    from .windows import _W_MATCH, _W_ROWS_R, _W_STAGED_PAIRS

    st = dw.state
    # (the pair list as staged: the reference frame is the prune's even where a caller's triangulation removed cells and their pairs)
    pairs, n_box = st.fetch(_W_STAGED_PAIRS), len(st.fetch(_W_ROWS_R))
    used = np.zeros(n_box, bool)
    used[pairs[:, 1]] = True
    m = st.fetch(_W_MATCH)
    return np.where(m >= 0, (np.cumsum(used) - 1)[np.maximum(m, 0)], -1)


def sliding_window_incumbent(ref, moving, commonCT=None, outprefix=None, moving_delaunay=None, moving_delaunay_vertex_col=None,
                             optim_params=None, gurobi_params=None, ignore_precomputed_triangulation=False, *, workers=None,
                             window_local_indices=False, return_stats=False, triangulator=None, ctx=None, merge=False, batch=None,
                             _shard=None, _pipeline=None, _route=None, _merge_channel=None):
    """See the module text.  -> DataFrame (with return_stats: (DataFrame, [per-window stats dict in plan order])).
    workers: threads walking this process's windows on the device route (default: 2 where the process has >= 8 CPUs, else 1).
    A window whose prune leaves no pairs raises the ValueError run_same raises for it (src/same.py:1003), as the reference's loop does.
    `triangulator`, `batch` (windows per library call on the device route): see windows.iter_device_windows.  `_route` = 'device' |
    'general' (testing: forces a route).  optim_params["hip_delaunay"] = "native" (device route): the windows are triangulated by
    libsame_hip's own triangulator where that is provably the same as asking scipy (delaunay.py); the table is the same.  "device":
    the same, triangulated on the GPU (delaunay.DeviceTriangulator; the pass's counts in delaunay.last_device_stats()).
    merge=True: the table after `merge_window_matches_unique_ref` (src/helpers.py:692-815) -- one row per aligned and per reference cell,
    aligned ids ascending -- without the pre-merge table ever being laid out: the merge reads the rows' keys, and only the rows it keeps
    get their columns.  With `_shard` and a `_merge_channel` (dist.MergeChannel) the result is this rank's PART of the merged table
    (dist.sharded_merged_window_incumbent)."""
    mode = WindowMode.from_params(optim_params, gurobi_params, moving)
    job = _WindowJob(ref, moving, commonCT, outprefix, moving_delaunay, moving_delaunay_vertex_col, optim_params, gurobi_params,
                     ignore_precomputed_triangulation, _shard, mode=mode)
    frames, own = job.device_frames(_pipeline, ctx=ctx)
    # the cell-type-priority prune: on the host -- the general route -- unless optim_params["hip_priority_prune"] = "device"
    priority = bool(job.optim_params["ignore_knn_if_matched"]) and priority_prune_route(job.optim_params) == "device"
    host_prune = bool(job.optim_params["ignore_knn_if_matched"]) and not priority
    fast = frames is not None and not job.caller_triangulation and not host_prune
    caller = None
    if frames is not None and job.caller_triangulation and caller_delaunay_route(job.optim_params) == "device":
        # the caller's triangulation resident beside the moving section -- unless the device route refuses these inputs
        # (window_api.caller_triangulation_refusal): then the general route runs, as without the key
        if not host_prune:
            caller = frames.caller_tris(job.moving_delaunay, job.vertex_col)
        fast = caller is not None
    if _route is not None:
        if _route == "device" and not fast:
            raise ValueError("the device route does not apply to these inputs")
        fast = _route == "device"
    stats = {}
    try:
        if merge and job.all_matches:
            raise ValueError("merge=True does not resume from an outprefix that already holds windows")
        if fast:
            if triangulator is None and caller is None:
                from . import delaunay

                triangulator = delaunay.triangulator_for(job.optim_params)   # optim_params["hip_delaunay"] / $SAME_DELAUNAY
            (table, stats), = _device_pass([job], frames, workers, window_local_indices, triangulator, merge, _merge_channel, batch,
                                           caller, priority)
        else:
            table = _general_route(job, frames, window_local_indices, stats, ctx)
            if merge:
                from .merge import merge_table_part

                # (reach: the prune's radius bounds the distance of a pair's two cells on every route -- no collective to measure it, so
                # ranks on different routes still make the same exchanges)
                from .window_api import codes_of_ids, frame_id_codes

                cid = job.optim_params["cell_id_col"]
                _codes, unique, (mov_ids, ref_ids) = frame_id_codes(job.moving, job.ref, cid)
                to_codes = lambda a, r: (codes_of_ids(mov_ids, a), codes_of_ids(ref_ids, r))       # what the device route exchanges too
                table = merge_table_part(table, job.plan, job.owner, _merge_channel, cid, reach=abs(float(job.optim_params["radius"])),
                                         ids_unique=unique, id_codes=to_codes)
    finally:
        if own:
            frames.close()
    if job.output_file and len(table):
        table.to_csv(job.output_file, index=False)
    return (table, [stats[pos] for pos in sorted(stats)]) if return_stats else table


def _merged_rows(job, frames, rows, channel):
    """The window merge on what the FINAL_RECORDs `rows` of the builders say of their cells -> the rows the merged table keeps, in its
    order."""
    from . import merge as M

    a_row, r_row, wid, pos = (rows[k].astype(np.int64) for k in ("a_row", "r_row", "wid", "pos"))
    viol = (rows["flags"] & 1) != 0
    with stage("merge: cell ids of the rows"):
        (a_code, r_code), unique = frames.id_codes(job.optim_params["cell_id_col"])
        a_ids, r_ids = a_code[a_row], r_code[r_row]
    if channel is None or channel.world == 1:
        return M.merged_part_rows(a_ids, r_ids, viol, wid, None, None)
    with stage("merge: seam rows marked"):
        if unique:
            axy, rxy = frames.mov_sec.xy, frames.ref_sec.xy
            # rows whose window has no foreign window near are not looked at (seam_rows); the prune's radius bounds a pair's distance
            def coords(b, e):
                a, r = axy[a_row[b:e]], rxy[r_row[b:e]]
                return a[:, 0], a[:, 1], r[:, 0], r[:, 1]

            seam = M.seam_rows(pos, coords, job.plan, job.owner, channel.rank, abs(float(job.optim_params["radius"])))
        else:
            seam = np.ones(len(a_row), bool)
    return M.merged_part_rows(a_ids, r_ids, viol, wid, pos, seam, channel.rank, channel.tables)


def _device_pass(jobs, frames, workers, with_ref_idx, triangulator, merge=False, channel=None, batch=None, caller=None, priority=False,
                 variants=None, score=None):
    """The device route: ONE walk of the windows for `jobs` -- _WindowJobs over the same frames, plan and share of the plan that differ
    in sweep.SWEEP_KEYS only (`sliding_window_incumbent`: its one job; `sliding_window_sweep`: a job per parameter set) and in the
    type-matrix variant of the moving frame they are priced from (`sliding_window_variants`: a job per (variant, set); `variants` the
    variants' windows.DeviceTypesLayers, None for the frame's own types; a job names its variant by `job.variant`, an index into them,
    and carries the matrix and the layer as `job.variant_types` / `job.variant_layer`).  Every job has
    its own builders, accumulators and stats.  -> [(table, {plan position: stats record}) per job].  `caller`: the jobs' (one)
    triangulation as a windows.DeviceCallerTris -- selected once per batch, whatever the number of jobs.  A merge channel goes with a
    single job.  `score` (scores.DeviceScores; merge=True, no window-local indices, no channel): every job's merged rows are scored
    where the merge left them and the record kept as `job.score_record`; with `score.tables` False the job's table is None -- never
    made."""
    if len(jobs) > 1 and channel is not None:
        raise ValueError("several jobs over one pass: not with a merge channel")
    if score is not None and (not merge or with_ref_idx or channel is not None):
        raise ValueError("scores are read off the merged rows of one process: merge=True, no window-local indices, no merge channel")
    job = jobs[0]                 # what the jobs share is read from the first
    n_workers = max(1, int(workers if workers is not None else _default_workers()))
    n_workers = min(n_workers, max(1, len(job.todo)))
    contexts = frames.worker_contexts(n_workers)
    sections = (frames.ref_sec, frames.mov_sec)
    builders = [[_TableBuilder(j, sections, with_ref_idx) for _ in range(n_workers)] for j in jobs]
    lock = threading.Lock()
    # worker q walks a contiguous run of this process's windows
    cut = [len(job.todo) * q // n_workers for q in range(n_workers + 1)]
    # merge=True: the windows' matches stay where they are.  Every batch's central rows join the pass's accumulator on the device
    # (csrc/window_merge.hip); the merge runs there, and only what it could not decide alone comes to the host (`_merge_on_device`).
    # (window_local_indices needs every window's pair list on the host: the keys go through the builders then, `_merged_rows`.)
    accs, extra = None, []
    # (every job's builder: a variant's type columns are float64 whatever the frame's own are)
    device_table = all(b[0].device_columns_possible() for b in builders) and os.environ.get("SAME_TABLE_COLUMNS", "device") != "host"
    stats = [{} for _ in jobs]
    try:
        if not with_ref_idx and (merge or (device_table and not job.all_matches)):
            # job 0 takes the frames' own accumulators (which also puts the id codes on the device), every further job a set of its own
            accs = [_begin_accumulators(job, frames, contexts, cut, channel if merge else None)]
            for _j in jobs[1:]:
                mine = [MergeAccumulator(c) for c in contexts]
                extra.extend(mine)
                for q, acc in enumerate(mine):
                    acc.begin(sum(w["n_mov"] for _pos, w in job.todo[cut[q]:cut[q + 1]]))
                accs.append(mine)
        if priority or score is not None:  # once, here: before a worker thread stages its first window (as the id codes above)
            frames.label_codes_on_device()
        pos_of = {id(w): pos for pos, w in job.todo}
        sets = [(j.optim_params["knn"], j.mode, j.optim_params["no_match_penalty"], getattr(j, "variant", 0)) for j in jobs]

        def walk(q):
            collector = None
            if accs is not None:
                collector = lambda states, windows, s: accs[s][q].collect(states, [w["trim"] for w in windows],
                                                                          [w["window_id"] for w in windows],
                                                                          [pos_of[id(w)] for w in windows])
            for dw in frames.windows([w for _p, w in job.todo[cut[q]:cut[q + 1]]], ctx=contexts[q], triangulator=triangulator,
                                     collector=collector, batch=batch, caller=caller, priority=priority, sets=sets, variants=variants):
                s, pos = dw.set, pos_of[id(dw.window)]
                if dw.error is not None:
                    raise _window_error(dw, jobs[s].optim_params)      # (the priority prune's own failure for a window without pairs)
                if dw.skipped:                   # every pair went with the unconstrained nodes: nothing to match (as the general route)
                    continue
                with stage("table rows (central trim)"):
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

            threads = [threading.Thread(target=guarded, args=(q,), name=f"same-windows-{q}") for q in range(n_workers)]
            [t.start() for t in threads]
            [t.join() for t in threads]
            if errors:
                raise errors[0]
        return [(_route_table(j, frames, builders[s], None if accs is None else accs[s], merge, channel, device_table, score), stats[s])
                for s, j in enumerate(jobs)]
    finally:
        for acc in extra:
            acc.close()


def _route_table(job, frames, builders, accs, merge, channel, device_table, score=None):
    """The device route's table once its windows are walked: from the builders' rows or from the accumulators' (None: the builders hold
    them), merged or laid end to end.  `score`: see `_device_pass`."""
    # the rows that stay, as FINAL_RECORDs: the builders' (the merge chooses among them on the host) or the accumulator's (the merge chose
    # on the device; its columns may come from there too) -- then one way from records to the table
    me, with_pos = builders[0], job.mine is not None and not merge
    if accs is None:
        rows, ref_idx = _TableBuilder.rows(builders)
        if merge:
            keep = _merged_rows(job, frames, rows, channel)
            rows, ref_idx = rows[keep], ref_idx if ref_idx is None else ref_idx[keep]
    else:
        calls0 = accs[0].ctx.stats()
        if merge:
            done = _merge_on_device(job, frames, accs, channel)
        else:               # the windows' tables end to end, as they were collected (src/same.py:583-590)
            from .windows import plain_accumulators

            with stage("table rows (accumulated on the device, in plan order)"):
                done = plain_accumulators(accs)
        if score is not None:
            # the merged rows are final in the accumulator: scored there; without tables that is all -- no columns, no frame
            with stage("scores (counted on the device from the merged rows)"):
                calls1 = accs[0].ctx.stats()
                job.score_record = score.record(frames, done)
                _count_merge_calls(frames, accs[0].ctx, calls1, passes=0)
            if not score.tables:
                return None
        if not done.n_final:
            return pd.DataFrame()
        if device_table:
            with stage("table (columns of the rows that stay: by the device into page-locked memory)"):
                table = me.table_from_device(frames, done, with_pos)
            if table is not None:
                # (the merge counted its own calls; what is new here: the rows laid end to end, the columns' launch and wait)
                _count_merge_calls(frames, accs[0].ctx, accs[0].ctx.stats() if merge else calls0, passes=0 if merge else 1)
                return table
        rows, ref_idx = done.final_rows(), None
    with stage("table (columns gathered on the gather threads)"):
        table = me.gather(rows, ref_idx, with_pos)
    if job.all_matches:                      # rows of windows finished by an earlier run (resume)
        table = pd.concat(job.all_matches + ([table] if len(table) else []), ignore_index=True)
    return table


def _begin_accumulators(job, frames, contexts, cut, channel):
    """A merge accumulator per worker context, begun for this pass: sized for the worker's windows, with the seams of this rank's share
    of the plan when the plan is dealt over ranks."""
    from . import merge as M

    accs, unique = frames.accumulators(contexts, job.optim_params["cell_id_col"])
    near, reach = None, 0.0
    if channel is not None and channel.world > 1 and unique:
        reach = abs(float(job.optim_params["radius"]))          # the prune's radius bounds the distance of a pair's two cells
        known = frames.__dict__.setdefault("_seam_tables", {})
        key = (channel.rank, channel.world, reach, job.owner.tobytes(), len(job.plan))
        if key not in known:
            known[key] = M.seam_tables(job.plan, job.owner, channel.rank, reach)
        near = known[key]
    calls0 = accs[0].ctx.stats()
    for q, acc in enumerate(accs):
        expected = sum(w["n_mov"] for _pos, w in job.todo[cut[q]:cut[q + 1]])
        acc.begin(expected, near, reach, all_seam=channel is not None and channel.world > 1 and not unique)
    _count_merge_calls(frames, accs[0].ctx, calls0, passes=0)
    return accs


def _count_merge_calls(frames, ctx0, calls0, passes=1):
    """what a pass asked of the runtime ONCE on the first worker's context -- the accumulator's begin, the merge (resolve, finish: a sort's
    worth of launches) or the rows laid end to end, the table's columns; the windows' calls are counted per window -- read by bench.py
    and by the launch-budget test"""
    spent = frames.__dict__.setdefault("merge_runtime_calls", {})
    for k, v in ctx0.stats().items():
        spent[k] = spent.get(k, 0) + v - calls0[k]
    spent["passes"] = spent.get("passes", 0) + passes


def _merge_on_device(job, frames, accs, channel):
    """The window merge of the accumulated rows (src/helpers.py:692-815): codes, de-duplication, degrees and the rows that stand alone
    on the device; components / Hopcroft-Karp of the contested cells, and the seam rows' exchange between ranks, here.
    -> the accumulator that holds the merged table's rows (aligned ids ascending; `.n_final`, `.final_rows()`)."""
    from . import merge as M
    from .windows import resolve_accumulators

    ctx0 = accs[0].ctx
    calls0 = ctx0.stats()
    with stage("merge: accumulated rows resolved (device)"):
        _counts, rest = resolve_accumulators(accs, frames.dmov, frames.dref)
    a, r, wid = rest["ac"].astype(np.int64), rest["rc"].astype(np.int64), rest["wid"].astype(np.int64)
    viol = (rest["flags"] & 1) != 0
    if channel is None or channel.world == 1:
        rows = M._resolve_rows(a, r, viol, wid, M.already_deduplicated) if len(rest) else np.zeros(0, np.int64)
    else:
        seam = (rest["flags"] & 4) != 0
        mine, sent = M.part_decided_here(a, r, viol, wid, rest["pos"].astype(np.int64), seam, channel.rank, M.already_deduplicated,
                                         seq=rest["cidx"])
        with stage("merge: seam rows exchanged"):
            parts = channel.tables(sent)
        with stage("merge: seam step (the same on every rank)"):
            rows = np.concatenate((mine, _seam_step_on_device(frames, ctx0, parts, channel.rank)))
    with stage("merge: winners to the device, final rows in order"):
        # the rows stay on the device: the table's columns are gathered from them there
        accs[0].finish(rest["row"][rows], fetch=False)
    _count_merge_calls(frames, ctx0, calls0)
    return accs[0]


def _seam_step_on_device(frames, ctx, parts, rank):
    """The common step of a merge dealt over ranks (merge.part_after_seam_step) with the gathered seam rows on the device: they are
    loaded into an accumulator of their own (their cells named by codes, in the single process's order), de-duplicated, counted and
    classed there like a pass's own rows; the host matches the few cells that are still contested.  -> this rank's winners (indices into
    the table it sent)."""
    from . import merge as M
    from .windows import MergeAccumulator, resolve_accumulators

    parts = [p for p in parts if len(p["row"])]
    if not parts:
        return np.zeros(0, np.int64)
    col = lambda c: np.concatenate([p[c] for p in parts])
    order_key = col("order")
    order = None if bool(np.all(order_key[1:] >= order_key[:-1])) else np.argsort(order_key, kind="stable")
    take = (lambda c: col(c)) if order is None else (lambda c: col(c)[order])
    a, r = take("a"), take("r")
    acc = frames.__dict__.get("_seam_acc")
    if acc is None or acc.ctx is not ctx:
        acc = frames.__dict__["_seam_acc"] = MergeAccumulator(ctx)
        frames.__dict__.setdefault("_accs", {})[("seam", id(ctx))] = acc           # closed with the frames
    # pos carries the sender's rank, cidx its row in the table it sent: what comes back names the winners by both
    acc.load(a, r, take("viol"), take("window"), take("rank"), take("row"), int(a.max()) + 1, int(r.max()) + 1)
    _counts, rest = resolve_accumulators([acc], None, None)
    won = M._resolve_rows(rest["ac"].astype(np.int64), rest["rc"].astype(np.int64), (rest["flags"] & 1) != 0, rest["wid"].astype(np.int64),
                          M.already_deduplicated, mark=False) if len(rest) else np.zeros(0, np.int64)
    final = acc.finish(rest["row"][won])
    return final["cidx"][final["pos"] == rank].astype(np.int64)


def _general_route(job, frames, with_ref_idx, stats, ctx):
    commonCT = job.commonCT
    keep_csv, job.outprefix = job.outprefix, None        # the table is written once, by the caller of this route
    try:
        for pos, w, prep in _walk_windows(job.todo, frames, job.ref, job.moving, commonCT, job.optim_params, job.gurobi_params,
                                          moving_delaunay=job.moving_delaunay, vertex_col=job.vertex_col, ignore_pre=job.ignore_pre,
                                          verbose=False, ctx=ctx, fetch_triangles=True):
            if isinstance(prep, Exception):
                raise prep
            if isinstance(prep, _Staged):
                prep = prepare_same_inputs(None, None, commonCT, verbose=False, ctx=ctx, _staged=prep)
            if len(prep.valid_pairs) == 0:               # every node unconstrained under the caller's triangulation: nothing to match
                continue
            with stage("incumbent + sweeps + table (general route)"):
                window_matches, stats[pos] = incumbent_of_prepared(prep, commonCT, with_ref_idx, ctx=ctx, use_device=False, mode=job.mode)
            job.collect(pos, w, window_matches)
    finally:
        job.outprefix = keep_csv
    return job.result()
