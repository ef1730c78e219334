"""A study read per CELL, not per study: `sliding_window_score_maps`.

The reference's notebooks plot every spatial panel per cell: examples/synthetic/reproduce_figures.ipynb ("Check triangle violations",
Fig 2e) splits the matches into good and bad by `in_violating_triangle`; the tongue notebook plots every moving cell as correct or
incorrect (Fig 4, `_1NN_match`); the LUAD notebook plots the pairs as in or out of the top k (FigS19, cell 13); the synthetic benchmark
ships `ground_truth.csv` with the true pairs.  `sliding_window_scores` and `sliding_window_score_details` reduce a result to counts;
the columns behind those counts were to be had only from the tables, on the host.

When a set's merge ends everything a per-cell column reads is on the device, in the score call's own work buffer.
`sliding_window_score_maps` keeps it: one call per result in the score call's place (csrc/window_score_map.hip) returns the score
call's counts and one 16-byte mark per moving row, and folds the result into a per-cell tally that stays resident until the study's
last result.  `score_table_maps` is the same frame from a result TABLE with the functions the package already has: what the device
must equal, and what inputs the device refuses go through."""
import collections
import types

import numpy as np
import pandas as pd

from . import _lib, ops
from .eval_utils import _label_codes, check_triangle_violations
from .params import init_optim_params
from .score_details import DetailSpec, label_ranks
from .scores import DeviceScores, _frame_rows, _scored_study, checked_score_params, counts_from_words, record_from_counts
from .triangles import _as_triangle_array
from .variants import _common_types, _frames_of

ScoreMaps = collections.namedtuple("ScoreMaps", "scores cells tally")
TRUTH_KEYS = ("truth_rows", "truth_matches", "truth_accuracy")
TALLY_KEYS = ("results", "matched_in", "type_match_in", "violating_in", "on_truth_in")
UNRANKED, RANK_TOP = _lib.SAME_MARK_UNRANKED, 254       # the rank bytes of a row that is not ranked; where a rank saturates


def truth_record(truth_rows, truth_matches):
    """the truth keys from their two counts: matched rows whose truth is known, those matched to it, truth_accuracy = 100 * (matches /
    rows), NaN with no rows"""
    n, k = int(truth_rows), int(truth_matches)
    return {"truth_rows": n, "truth_matches": k, "truth_accuracy": 100 * (k / n) if n else float("nan")}


def _study_cell_id_col(ref_arg, moving_arg, optim_params):
    """the id column a window job over these arguments settles on (window_api._WindowJob): optim_params', else a MetaCell object's
    `metacell_idx_col` (the reference's first), else the parameters' default"""
    op = dict(optim_params or {})
    for obj in (ref_arg, moving_arg):
        if op.get("cell_id_col") is None and hasattr(obj, "metacell_df") and hasattr(obj, "metacell_idx_col"):
            op["cell_id_col"] = obj.metacell_idx_col
    return init_optim_params(**op)["cell_id_col"]


def checked_truth(truth, ref_df, mov_df, cell_id_col):
    """-> int32 per row of the moving frame: the row of `ref_df` whose `cell_id_col` is the moving row's true reference id (an id that
    names several rows: the last, as `_frame_rows`), -1 where the truth is missing; None for None.  `truth`: a Series aligned on the
    moving frame's index, an array of its length, or a dict from moving id (`cell_id_col`) to reference id.  ValueError for any other
    type, a wrong length, a missing id column or an id that names no reference cell."""
    if truth is None:
        return None
    for df, name in ((ref_df, "ref"), (mov_df, "moving")):
        if cell_id_col not in getattr(df, "columns", ()):
            raise ValueError(f"truth names cells by '{cell_id_col}': the {name} frame has no such column")
    n = len(mov_df)
    if isinstance(truth, dict):
        values = mov_df[cell_id_col].map(truth).to_numpy(dtype=object)
    elif isinstance(truth, pd.Series):
        values = truth.reindex(mov_df.index).to_numpy(dtype=object) if not truth.index.equals(mov_df.index) else truth.to_numpy(dtype=object)
        if len(values) != n:
            raise ValueError(f"truth does not align with the moving frame's index ({len(values)} values for {n} rows)")
    else:
        if isinstance(truth, (str, bytes)) or not hasattr(truth, "__len__"):
            raise ValueError(f"truth must be a Series on the moving index, an array of its {n} rows or a dict, not {type(truth).__name__}")
        values = np.empty(len(truth), dtype=object)
        values[:] = list(truth)
        if len(values) != n:
            raise ValueError(f"truth has {len(values)} values; the moving frame has {n} rows")
    known = ~np.asarray(pd.isna(values), dtype=bool)
    rows = np.full(n, -1, np.int32)
    if known.any():
        try:
            rows[known] = _frame_rows(ref_df[cell_id_col].to_numpy(), pd.Series(values[known]).infer_objects().to_numpy(), "reference")
        except ValueError:
            raise ValueError(f"truth names reference ids that are not in the reference frame's '{cell_id_col}'") from None
    return rows


def _cells_frame(index, ref_ids, ref_row, type_match, node_tri, node_flip, violating, truth=None, ranks=None):
    """the per-cell frame of one result, the one statement of its columns and dtypes for the device's marks and the host's arrays.
    `truth`: (truth_known, on_truth) or None; `ranks`: (rank_strict, rank_weak, ranked) or None"""
    ref_row = np.asarray(ref_row, np.int64)
    matched = ref_row >= 0
    ids = pd.Series(np.asarray(ref_ids))
    if ids.dtype.kind in "iu":
        ids = ids.astype("Int64")               # (a missing id beside integer ids: <NA>, not a float)
    ref_id = ids.take(np.maximum(ref_row, 0)).reset_index(drop=True).where(pd.Series(matched)) if len(ids) else pd.Series([None] * len(ref_row))
    node_tri = np.asarray(node_tri, np.int64)
    cols = {"ref_row": ref_row, "ref_id": ref_id.to_numpy() if ref_id.dtype == object else ref_id.array, "matched": matched,
            "type_match": np.asarray(type_match, bool), "node_triangles": node_tri, "node_flips": np.asarray(node_flip, np.int64),
            "considered": node_tri > 0, "in_violating_triangle": np.asarray(violating, bool)}
    if truth is not None:
        cols["truth_known"], cols["on_truth"] = np.asarray(truth[0], bool), np.asarray(truth[1], bool)
    if ranks is not None:
        cols["rank_strict"], cols["rank_weak"] = np.asarray(ranks[0], np.uint8), np.asarray(ranks[1], np.uint8)
        cols["ranked"] = np.asarray(ranks[2], bool)
    return pd.DataFrame(cols, index=index)


def cells_from_marks(marks, index, ref_ids, with_truth, with_ranks):
    """`_cells_frame` of the library's marks (windows.CELL_MARK, one per row of the moving frame)"""
    f = marks["flags"]
    bit = lambda b: (f & b) != 0
    return _cells_frame(index, ref_ids, marks["ref_row"], bit(_lib.SAME_MARK_TYPE_MATCH), marks["node_tri"], marks["node_flip"],
                        bit(_lib.SAME_MARK_VIOLATING),
                        (bit(_lib.SAME_MARK_TRUTH_KNOWN), bit(_lib.SAME_MARK_ON_TRUTH)) if with_truth else None,
                        (marks["rank_strict"], marks["rank_weak"], bit(_lib.SAME_MARK_RANKED)) if with_ranks else None)


def tally_from_cells(cells, index):
    """the host's tally: the sum over the per-result frames `cells` (a flat list)"""
    n = len(index)
    total = lambda col: sum((c[col].to_numpy().astype(np.int64) for c in cells if col in c.columns), np.zeros(n, np.int64))
    return pd.DataFrame({"results": np.full(n, len(cells), np.int64), "matched_in": total("matched"), "type_match_in": total("type_match"),
                         "violating_in": total("in_violating_triangle"), "on_truth_in": total("on_truth")}, index=index)


def score_table_maps(table, ref, moving, *, cell_id_col, commonCT=None, truth=None, ranks=False, score_delaunay=None,
                     score_delaunay_vertex_col=None, score_params=None, ctx=None, _truth_row=None):
    """The per-cell frame of ONE result table of `sliding_window_incumbent` / `_sweep` / `_variants` over the frames `ref` and `moving`
    (MetaCell objects: their `.metacell_df`), with the functions the package already has -- what `sliding_window_score_maps`'
    `cells[v][s]` must equal.  Indexed like the moving frame, in its row order:
      ref_row, ref_id        the position in the reference frame of the cell the row was put on (-1: unmatched) and its `cell_id_col`;
      matched, type_match    is it matched; do the two `cell_type` labels compare equal (`score_table`'s rule);
      node_triangles, node_flips, considered   `ops.tri_flip_stats`' counters of the row over `score_delaunay`'s triangles that are all
                             matched and not skipped, the flipped ones among them, and node_triangles > 0 (all 0 / False without one);
      in_violating_triangle  `check_triangle_violations`' own column under `score_params`, called as `score_table` calls it;
      truth_known, on_truth  with `truth` (`checked_truth`): is the row's true reference cell known; is the row matched to it;
      rank_strict, rank_weak, ranked   with `ranks` (needs `commonCT`): `label_ranks` of (the row's label, its reference cell's commonCT
                             columns), saturated at 254; 255 and False where the row is not ranked.  `rank_weak < k`: in the top k under
                             every tie order (`top_k_counts`).
    Rows the table does not name are unmatched: -1, <NA> / None, False, 0, 255."""
    p = checked_score_params(score_params)
    ref, moving = getattr(ref, "metacell_df", ref), getattr(moving, "metacell_df", moving)
    for df, name in ((ref, "ref"), (moving, "moving")):
        if "cell_type" not in df.columns:
            raise ValueError(f"scores compare cell types: the {name} frame has no 'cell_type' column")
    if ranks and commonCT is None:
        raise ValueError("ranks=True ranks the reference cells' commonCT columns: pass commonCT")
    truth_row = checked_truth(truth, ref, moving, cell_id_col) if _truth_row is None else _truth_row     # (rows the caller checked already)
    n, n_mov = len(table), len(moving)
    rows_m = _frame_rows(moving[cell_id_col].to_numpy(), table[f"Aligned_{cell_id_col}"].to_numpy(), "moving") if n else np.zeros(0, np.int64)
    rows_r = _frame_rows(ref[cell_id_col].to_numpy(), table[f"Ref_{cell_id_col}"].to_numpy(), "reference") if n else np.zeros(0, np.int64)
    ref_row = np.full(n_mov, -1, np.int64)
    ref_row[rows_m] = rows_r
    mov_type = moving["cell_type"].to_numpy()[rows_m]
    code_m, code_r = _label_codes(mov_type, ref["cell_type"].to_numpy()[rows_r])
    type_match = np.zeros(n_mov, bool)
    type_match[rows_m] = (code_m >= 0) & (code_m == code_r)
    node_tri, node_flip, violating = np.zeros(n_mov, np.int64), np.zeros(n_mov, np.int64), np.zeros(n_mov, bool)
    if score_delaunay is not None and n:
        tri = np.asarray(_as_triangle_array(score_delaunay)).reshape(-1, 3)
        if score_delaunay_vertex_col is not None and score_delaunay_vertex_col not in moving.columns:
            raise ValueError(f"score_delaunay_vertex_col='{score_delaunay_vertex_col}' not in the moving frame")
        vertex_ids = moving.index.to_numpy() if score_delaunay_vertex_col is None else moving[score_delaunay_vertex_col].to_numpy()
        if not pd.Index(vertex_ids).is_unique:
            raise ValueError("the moving frame's vertex ids are not unique: its triangulation names no definite cells")
        mapped_xy = np.column_stack((table["ref_X"].to_numpy(dtype=np.float64), table["ref_Y"].to_numpy(dtype=np.float64)))
        out = pd.DataFrame({"__vertex_id": vertex_ids[rows_m], f"Ref_{cell_id_col}": table[f"Ref_{cell_id_col}"].to_numpy(),
                            "ref_X": mapped_xy[:, 0], "ref_Y": mapped_xy[:, 1], "cell_type": mov_type})
        frame = pd.DataFrame({"X": moving["X"].to_numpy(), "Y": moving["Y"].to_numpy()}, index=vertex_ids)
        carrier = types.SimpleNamespace(metacell_df=frame, metacell_delaunay=tri)
        marked, _stats = check_triangle_violations(out, carrier, aligned_id_col="__vertex_id", ref_id_col=f"Ref_{cell_id_col}",
                                                   mapped_x_col="ref_X", mapped_y_col="ref_Y", cell_type_col="cell_type", ctx=ctx, **p)
        violating[rows_m] = marked["in_violating_triangle"].to_numpy().astype(bool)
        # the node counters themselves: the kernel behind that call on the same arrays (eval_utils.check_triangle_violations makes them so)
        corner = pd.Index(vertex_ids).get_indexer(tri.reshape(-1)).reshape(-1, 3)
        is_matched = np.zeros(n_mov, np.uint8)
        is_matched[rows_m] = 1
        mapped = np.zeros((n_mov, 2))
        mapped[rows_m] = mapped_xy
        type_id = None
        if p["ignore_same_type_triangles"]:
            type_id = np.full(n_mov, -1, np.int32)
            type_id[rows_m] = pd.factorize(mov_type, use_na_sentinel=False)[0].astype(np.int32)
        _flag, n_tri, n_flip = ops.tri_flip_stats(frame[["X", "Y"]].to_numpy(dtype=np.float64), mapped, is_matched,
                                                  corner[(corner >= 0).all(axis=1)].astype(np.int32), type_id, ctx=ctx)
        node_tri[rows_m], node_flip[rows_m] = n_tri[rows_m], n_flip[rows_m]
    truth_cols = rank_cols = None
    if truth_row is not None:
        truth_cols = (truth_row >= 0, (ref_row >= 0) & (ref_row == truth_row))
    if ranks:
        columns = list(commonCT)
        strict, weak, typed = label_ranks(mov_type, ref[columns].to_numpy(dtype=np.float64)[rows_r] if n else np.zeros((0, len(columns))), columns)
        rs, rw, ranked = np.full(n_mov, UNRANKED, np.uint8), np.full(n_mov, UNRANKED, np.uint8), np.zeros(n_mov, bool)
        rs[rows_m] = np.where(typed, np.minimum(strict, RANK_TOP), UNRANKED)
        rw[rows_m] = np.where(typed, np.minimum(weak, RANK_TOP), UNRANKED)
        ranked[rows_m] = typed
        rank_cols = (rs, rw, ranked)
    return _cells_frame(moving.index, ref[cell_id_col].to_numpy(), ref_row, type_match, node_tri, node_flip, violating, truth_cols, rank_cols)


class MapScores(DeviceScores):
    """`scores.DeviceScores` whose `record` makes the map call in the score call's place (windows.MergeAccumulator.score_map): the
    record of the counts, the result's per-cell frame (`cells`, in the jobs' order) and, resident until `finished`, the study's tally."""

    def __init__(self, score_delaunay, vertex_col, params, truth_row, ranks, per_result, tally):
        super().__init__(score_delaunay, vertex_col, params, tables=False)
        self.truth_row, self.ranks, self.per_result, self.with_tally = truth_row, bool(ranks), bool(per_result), bool(tally)
        self.rank_dev = self.map = None      # the label columns (windows.DeviceScoreDetail) and the map (windows.DeviceScoreMap) once `prepare` agreed
        self.cells = []                      # with per_result: the frame per job, in the jobs' order
        self.tally_words, self.n_results = None, 0

    def prepare(self, frames, job):
        """`DeviceScores.prepare`, then the label columns (with ranks: `DetailSpec.resident` with no groups; None beyond the library's
        label cap) and the map resident beside the sections"""
        if not super().prepare(frames, job):
            return False
        if self.ranks:
            self.rank_dev = DetailSpec(None, None, (1,)).resident(frames)
            if self.rank_dev is None:
                return False
        self.map = frames.score_map(self.truth_row, self.with_tally)
        return True

    def record(self, frames, acc):
        p = self.params
        counts, marks = acc.score_map(frames.dmov, frames.dref, self.tris, self.rank_dev, self.map, p["ignore_same_type_triangles"],
                                      p["node_local"], p["majority_threshold"], p["min_flips"], marks=self.per_result)
        rec = record_from_counts(counts_from_words(counts, self.total), p)
        if self.truth_row is not None:
            rec.update(truth_record(counts[8], counts[9]))
        if self.per_result:
            cid = self.job.optim_params["cell_id_col"]
            self.cells.append(cells_from_marks(marks, frames.moving.index, frames.ref[cid].to_numpy(), self.truth_row is not None, self.ranks))
        return rec

    def finished(self, frames):
        """the tally read from the device once, after the last result; the map is closed with it"""
        if self.map is not None:
            self.tally_words, self.n_results = self.map.tally()
            held = frames.__dict__.get("_score_maps", [])
            if self.map in held:
                held.remove(self.map)
            self.map.close()
            self.map = None


def sliding_window_score_maps(ref, moving, commonCT=None, *, truth=None, ranks=False, per_result=True, tally=True, type_variants=None,
                              param_sets=None, optim_params=None, gurobi_params=None, score_delaunay=None, score_delaunay_vertex_col=None,
                              score_params=None, workers=None, triangulator=None, ctx=None, batch=None, moving_delaunay=None,
                              moving_delaunay_vertex_col=None):
    """`sliding_window_scores` with every result read per CELL as well, over the same one pass of the windows and without a table:
    -> `ScoreMaps`
      scores   `sliding_window_scores`' frame for the same arguments; with `truth` it gains `truth_rows` (matched rows whose truth is
               known), `truth_matches` (those matched to it) and `truth_accuracy` = 100 * matches / rows (NaN with no rows);
      cells    `cells[v][s]`: the per-cell frame of result (variant v, set s), indexed like the moving frame (a MetaCell object's
               `metacell_df`) in its row order, with `score_table_maps`' columns; None with per_result=False;
      tally    one frame over the same index: `results`, the number of results, and per cell in how many of them it was matched
               (`matched_in`), type-matched (`type_match_in`), in a violating triangle (`violating_in`) and matched to its truth
               (`on_truth_in`); None with tally=False.
    `truth`: per moving row the id -- in `cell_id_col`'s terms -- of its true or baseline reference cell: a Series aligned on the moving
    frame's index, an array of its length or a dict from moving id to reference id; a missing value means unknown.  A baseline study is
    the same thing: pass an earlier result's `ref_id`.  `ranks=True` (needs `commonCT`) adds the rank columns.  The other keywords are
    `sliding_window_scores`' but for `tables` and `unpack` (cell-level maps are not offered).  A truth id that names no reference cell,
    a truth of the wrong length, `ranks` without `commonCT` and what `sliding_window_scores` refuses raise ValueError before a job or
    a device is touched.
    On the device ONE call per result takes the score call's place (csrc/window_score_map.hip): its marks come back in one copy per
    result, the tally stays resident and is read once, after the last result.  What `scores.DeviceScores.prepare` refuses, more labels
    than the library's cap with `ranks`, and whatever keeps the job off the shared pass go through `score_table_maps` on the tables:
    the same frames, nothing saved; the tally is then the sum over them."""
    params = checked_score_params(score_params)
    if ranks and commonCT is None:
        raise ValueError("ranks=True ranks the reference cells' commonCT columns: pass commonCT")
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    cid = _study_cell_id_col(ref_arg, moving_arg, optim_params)
    truth_row = checked_truth(truth, ref_df, mov_df, cid)
    hook = MapScores(score_delaunay, score_delaunay_vertex_col, params, truth_row, ranks, per_result, tally)
    scores, nested, hook = _scored_study(ref, moving, commonCT, type_variants=type_variants, param_sets=param_sets, optim_params=optim_params,
                                         gurobi_params=gurobi_params, score_delaunay=score_delaunay,
                                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=params, tables=False,
                                         workers=workers, triangulator=triangulator, ctx=ctx, batch=batch, moving_delaunay=moving_delaunay,
                                         moving_delaunay_vertex_col=moving_delaunay_vertex_col, unpack=None, hook=hook)
    n_sets = len(nested[0])
    job = hook.job
    index = job.moving.index
    if hook.records is not None:
        flat = hook.cells if per_result else None
        if truth_row is not None:
            for k in TRUTH_KEYS:
                scores[k] = [rec[k] for rec in hook.records]
        tally_frame = None
        if tally:
            words = hook.tally_words.astype(np.int64)
            tally_frame = pd.DataFrame({"results": np.full(len(index), hook.n_results, np.int64), **{k: words[:, q] for q, k in enumerate(TALLY_KEYS[1:])}},
                                       index=index)
    else:                                               # not scored on the device: the host statement on every table
        tri, vertex_col = hook.triangulation(job)
        cts = _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT) if ranks else None
        flat = [score_table_maps(t, job.ref, job.moving, cell_id_col=job.optim_params["cell_id_col"], commonCT=cts, _truth_row=truth_row, ranks=ranks,
                                 score_delaunay=tri, score_delaunay_vertex_col=vertex_col, score_params=params, ctx=ctx)
                for per_set in nested for t in per_set]
        if truth_row is not None:
            records = [truth_record(int((c["matched"] & c["truth_known"]).sum()), int(c["on_truth"].sum())) for c in flat]
            for k in TRUTH_KEYS:
                scores[k] = [rec[k] for rec in records]
        tally_frame = tally_from_cells(flat, index) if tally else None
        if not per_result:
            flat = None
    cells = None if flat is None else [flat[q:q + n_sets] for q in range(0, len(flat), n_sets)]
    return ScoreMaps(scores, cells, tally_frame)

