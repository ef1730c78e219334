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
must equal, and what inputs the device refuses go through.

With MetaCell objects and `unpack=` the same reading is made per original CELL as well: the reference's paper-scale
notebooks unpack the metacell matches and plot every cell by what the reference CELL it was put on says of it (examples/tongue cells
15-16, examples/luad cells 12-13).  One call per result in the unpack call's place (csrc/window_unpack_map.hip) returns one 16-byte
mark per moving member and folds the result into a per-member tally; `score_unpacked_maps` is the host statement per table."""
import collections
import types

import numpy as np
import pandas as pd

from . import _lib, ops
from .eval_utils import _label_codes, check_triangle_violations
from .params import init_optim_params
from .score_details import DetailSpec, _NoMetaCellObjects, label_ranks
from .scores import (DeviceScores, _frame_rows, _scored_study, checked_score_params, checked_unpack, counts_from_words, record_from_counts,
                     score_unpacked, unpack_record)
from .triangles import _as_triangle_array
from .variants import _common_types, _frames_of

ScoreMaps = collections.namedtuple("ScoreMaps", "scores cells tally")
CellScoreMaps = collections.namedtuple("CellScoreMaps", ScoreMaps._fields + ("cell_cells", "cell_tally"))
TRUTH_KEYS = ("truth_rows", "truth_matches", "truth_accuracy")
CELL_TRUTH_KEYS = ("cell_truth_rows", "cell_truth_matches", "cell_truth_accuracy")
TALLY_KEYS = ("results", "matched_in", "type_match_in", "violating_in", "on_truth_in")
CELL_TALLY_KEYS = ("results", "matched_in", "type_match_in", "on_truth_in")
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


def checked_truth(truth, ref_df, mov_df, cell_id_col, moving_id_col=None):
    """-> int32 per row of the moving frame: the row of `ref_df` whose `cell_id_col` is the moving row's true reference id (an id that
    names several rows: the last, as `_frame_rows`), -1 where the truth is missing; None for None.  `truth`: a Series aligned on the
    moving frame's index, an array of its length, or a dict from moving id (`cell_id_col`; `moving_id_col` where the moving frame names
    its ids otherwise) to reference id.  ValueError for any other type, a wrong length, a missing id column or an id that names no
    reference cell."""
    if truth is None:
        return None
    moving_id_col = cell_id_col if moving_id_col is None else moving_id_col
    for df, name, col in ((ref_df, "ref", cell_id_col), (mov_df, "moving", moving_id_col)):
        if col not in getattr(df, "columns", ()):
            raise ValueError(f"truth names cells by '{col}': the {name} frame has no such column")
    n = len(mov_df)
    if isinstance(truth, dict):
        values = mov_df[moving_id_col].map(truth).to_numpy(dtype=object)
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


def _ids_at(ref_ids, ref_row):
    """the `ref_id` column: `ref_ids` at the rows `ref_row`, missing where the row is -1 (a missing id beside integer ids: <NA>, not a
    float)"""
    ref_row = np.asarray(ref_row, np.int64)
    matched = ref_row >= 0
    ids = pd.Series(np.asarray(ref_ids))
    if ids.dtype.kind in "iu":
        ids = ids.astype("Int64")
    ref_id = ids.take(np.maximum(ref_row, 0)).reset_index(drop=True).where(pd.Series(matched)) if len(ids) else pd.Series([None] * len(ref_row))
    return ref_id.to_numpy() if ref_id.dtype == object else ref_id.array


def _cells_frame(index, ref_ids, ref_row, type_match, node_tri, node_flip, violating, truth=None, ranks=None):
    """the per-cell frame of one result, the one statement of its columns and dtypes for the device's marks and the host's arrays.
    `truth`: (truth_known, on_truth) or None; `ranks`: (rank_strict, rank_weak, ranked) or None"""
    ref_row = np.asarray(ref_row, np.int64)
    matched = ref_row >= 0
    node_tri = np.asarray(node_tri, np.int64)
    cols = {"ref_row": ref_row, "ref_id": _ids_at(ref_ids, ref_row), "matched": matched,
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
        if not self.prepare_cells(frames):
            return False
        self.map = frames.score_map(self.truth_row, self.with_tally)
        return True

    def prepare_cells(self, frames):
        """what a cell-level reading needs resident (UnpackMapScores), asked before the study's own map is made -> whether it is"""
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


# ---- at cell level: the unpacked pairs per moving CELL --------------------------------------------------------------------------------------
def checked_cell_truth(cell_truth, ref_mc, moving_mc):
    """`checked_truth` over the objects' ORIGINAL frames -> int32 per row of `moving_mc.original_df`: the row of `ref_mc.original_df`
    whose `original_idx_col` id is the moving cell's true reference cell, -1 unknown; None for None.  Each object names its own id
    column."""
    return checked_truth(cell_truth, ref_mc.original_df, moving_mc.original_df, ref_mc.original_idx_col, moving_mc.original_idx_col)


def _metacell_rows(mc):
    """per row of `mc.original_df` the row of `mc.metacell_df` whose member list names the cell (named by several: the last), -1: none"""
    lists = mc.metacell_df["members"].tolist()
    out = np.full(len(mc.original_df), -1, np.int64)
    ids = [x for m in lists for x in m]
    if ids:
        out[_frame_rows(mc.original_df[mc.original_idx_col].to_numpy(), np.asarray(ids), "member")] = np.repeat(np.arange(len(lists)),
                                                                                                              [len(m) for m in lists])
    return out


def _cell_cells_frame(ref_mc, moving_mc, metacell_row, ref_cell_row, ref_metacell_row, pair, type_match, truth=None, ranks=None):
    """the per-CELL frame of one result, the one statement of its columns and dtypes for the device's marks and the host's arrays: one
    entry per row of `moving_mc.original_df`.  `truth`: (truth_known, on_truth) or None; `ranks`: (rank_strict, rank_weak, ranked) or None"""
    ref_cell_row = np.asarray(ref_cell_row, np.int64)
    cols = {"ref_id": _ids_at(ref_mc.original_df[ref_mc.original_idx_col].to_numpy(), ref_cell_row), "ref_cell_row": ref_cell_row,
            "metacell_row": np.asarray(metacell_row, np.int64), "ref_metacell_row": np.asarray(ref_metacell_row, np.int64),
            "pair": np.asarray(pair, np.int64), "matched": ref_cell_row >= 0, "type_match": np.asarray(type_match, bool)}
    if truth is not None:
        cols["truth_known"], cols["on_truth"] = np.asarray(truth[0], bool), np.asarray(truth[1], bool)
    if ranks is not None:
        cols["rank_strict"], cols["rank_weak"] = np.asarray(ranks[0], np.uint8), np.asarray(ranks[1], np.uint8)
        cols["ranked"] = np.asarray(ranks[2], bool)
    return pd.DataFrame(cols, index=pd.Index(moving_mc.original_df[moving_mc.original_idx_col].to_numpy(), name=moving_mc.original_idx_col))


def score_unpacked_maps(table, ref_mc, moving_mc, strategy, *, commonCT=None, cell_truth=None, ranks=False, cells=None, _truth_row=None):
    """The per-CELL frame of ONE result table over the MetaCell objects `ref_mc` and `moving_mc`, with the functions the package already
    has -- what `sliding_window_score_maps(unpack=strategy)`'s `cell_cells[v][s]` must equal, and what it falls back to.  The pairs are
    `score_unpacked`'s unpacked table (examples/luad/reproduce_figures.ipynb cell 12, examples/tongue cell 15); every moving CELL then
    takes what the notebooks' next cell gives it (tongue cell 16: the reference cell it was put on and that cell's label).  Indexed by
    `moving_mc.original_df[original_idx_col]` in that frame's row order:
      ref_id, ref_cell_row   the `original_idx_col` id of the reference cell the cell was put on and its row in `ref_mc.original_df`
                             (-1, <NA> / None: unmatched -- its metacell is in no row of the table, or the cell is in no member list);
      metacell_row           the row of `moving_mc.metacell_df` whose member list names the cell (-1: none);
      ref_metacell_row       the table's Ref_metacell_id of the cell's pair (-1 unmatched);
      pair                   the pair's row in the unpacked table (-1 unmatched);
      matched, type_match    is it matched; do the two cells' `cell_type_col` labels compare equal (the notebook's
                             `cell_type == pred_cell_type`; a missing label equals nothing);
      truth_known, on_truth  with `cell_truth` (`checked_cell_truth`): is the cell's true reference cell known; is it matched to it;
      rank_strict, rank_weak, ranked   with `ranks` (needs `commonCT`): `label_ranks` of (the cell's label, `ref_mc.original_df[commonCT]`
                             at its reference cell), saturated at 254; 255 and False where the cell is not ranked.  `rank_weak < k`:
                             among the k largest columns under every tie order -- the LUAD notebook's cell 13.
    `cells`: `score_unpacked`'s unpacked table of `table` under `strategy` where the caller has it already."""
    if ranks and commonCT is None:
        raise ValueError("ranks=True ranks the reference cells' commonCT columns: pass commonCT")
    truth_row = checked_cell_truth(cell_truth, ref_mc, moving_mc) if _truth_row is None else _truth_row
    if cells is None:
        _record, cells = score_unpacked(table, ref_mc, moving_mc, strategy)
    n, n_mov = len(cells), len(moving_mc.original_df)
    rows_of = lambda mc, ids, what: _frame_rows(mc.original_df[mc.original_idx_col].to_numpy(), ids.to_numpy(), what)
    rows_m = rows_of(moving_mc, cells["Aligned_cell_id"], "moving") if n else np.zeros(0, np.int64)
    rows_r = rows_of(ref_mc, cells["Ref_cell_id"], "reference") if n else np.zeros(0, np.int64)
    metacell_row = _metacell_rows(moving_mc)
    ref_cell_row, ref_metacell_row, pair = (np.full(n_mov, -1, np.int64) for _q in range(3))
    type_match = np.zeros(n_mov, bool)
    if n:
        lists = moving_mc.metacell_df["members"].tolist()
        a_ids, r_ids = (table[c].to_numpy().astype(np.int64) for c in ("Aligned_metacell_id", "Ref_metacell_id"))
        per_row = [len(lists[a]) for a in a_ids.tolist()]
        assert sum(per_row) == n
        ref_cell_row[rows_m], pair[rows_m] = rows_r, np.arange(n)
        metacell_row[rows_m], ref_metacell_row[rows_m] = np.repeat(a_ids, per_row), np.repeat(r_ids, per_row)
        label = lambda mc: mc.original_df.set_index(mc.original_idx_col)[mc.cell_type_col]
        aligned_ct, ref_ct = cells["Aligned_cell_id"].map(label(moving_mc)), cells["Ref_cell_id"].map(label(ref_mc))
        type_match[rows_m] = (aligned_ct == ref_ct).to_numpy().astype(bool)
    truth_cols = rank_cols = None
    if truth_row is not None:
        truth_cols = (truth_row >= 0, (ref_cell_row >= 0) & (ref_cell_row == truth_row))
    if ranks:
        columns = list(commonCT)
        mov_labels = moving_mc.original_df[moving_mc.cell_type_col].to_numpy()[rows_m]
        types_r = ref_mc.original_df[columns].to_numpy(dtype=np.float64)[rows_r] if n else np.zeros((0, len(columns)))
        strict, weak, typed = label_ranks(mov_labels, types_r, columns)
        rs, rw, ranked = np.full(n_mov, UNRANKED, np.uint8), np.full(n_mov, UNRANKED, np.uint8), np.zeros(n_mov, bool)
        rs[rows_m] = np.where(typed, np.minimum(strict, RANK_TOP), UNRANKED)
        rw[rows_m] = np.where(typed, np.minimum(weak, RANK_TOP), UNRANKED)
        ranked[rows_m] = typed
        rank_cols = (rs, rw, ranked)
    return _cell_cells_frame(ref_mc, moving_mc, metacell_row, ref_cell_row, ref_metacell_row, pair, type_match, truth_cols, rank_cols)


def cell_tally_from_cells(cell_cells, index):
    """the host's cell-level tally: the sum over the per-result frames `cell_cells` (a flat list)"""
    n = len(index)
    total = lambda col: sum((c[col].to_numpy().astype(np.int64) for c in cell_cells if col in c.columns), np.zeros(n, np.int64))
    return pd.DataFrame({"results": np.full(n, len(cell_cells), np.int64), "matched_in": total("matched"), "type_match_in": total("type_match"),
                         "on_truth_in": total("on_truth")}, index=index)


def cell_truth_record(rows, matches):
    """`truth_record` under CELL_TRUTH_KEYS"""
    return {f"cell_{k}": v for k, v in truth_record(rows, matches).items()}


class UnpackMapScores(MapScores):
    """`MapScores` that also reads every result per moving CELL: the map call runs as it does, and `record` makes the cell-level map call
    in the unpack call's place (windows.MergeAccumulator.unpack_map, csrc/window_unpack_map.hip): the record gains UNPACK_KEYS (and the
    cell truth keys), `cell_cells` the result's per-cell frame, and the study's cell tally stays resident until `finished`."""

    def __init__(self, score_delaunay, vertex_col, params, truth_row, ranks, per_result, tally, unpack, ref_mc, moving_mc, cell_truth_row):
        super().__init__(score_delaunay, vertex_col, params, truth_row, ranks, per_result, tally)
        self.unpack, self.ref_mc, self.moving_mc, self.cell_truth_row = unpack, ref_mc, moving_mc, cell_truth_row
        self.cell_rank_dev = self.cell_map = None     # windows.DeviceUnpackDetail (with ranks), windows.DeviceUnpackMap once `prepare` agreed
        self.cell_cells = []                          # with per_result: the frame per job, in the jobs' order
        self.cell_tally_words, self.n_cell_results = None, 0
        self.metacell_row = None

    def prepare_cells(self, frames):
        """The member lists are resident (`DeviceScores.prepare` made them).  The device does not map these objects -- the whole call
        then goes through `score_unpacked_maps` on the tables -- where a cell is in two member lists of its side (a member's mark then
        names no definite cell), where a known truth cell is in no reference list (a mark names reference MEMBERS), and, with `ranks`,
        beyond the library's cap of cell labels."""
        mm, rm = self.members
        n_mov, n_ref = len(self.moving_mc.original_df), len(self.ref_mc.original_df)
        if len(np.unique(mm.rows)) != len(mm.rows) or len(np.unique(rm.rows)) != len(rm.rows):
            return False
        truth_member = None
        if self.cell_truth_row is not None:
            member_of = np.full(n_ref, -1, np.int64)                 # reference cell row -> its flat member
            member_of[rm.rows] = np.arange(len(rm.rows))
            known = self.cell_truth_row >= 0
            if bool((member_of[self.cell_truth_row[known]] < 0).any()):
                return False
            per_cell = np.where(known, member_of[np.maximum(self.cell_truth_row, 0)], -1)
            truth_member = per_cell[mm.rows].astype(np.int32)
        if self.ranks:
            self.cell_rank_dev = frames.unpack_detail(self.ref_mc, self.moving_mc, frames.commonCT, (1,))
            if self.cell_rank_dev is None:
                return False
        self.metacell_row = np.full(n_mov, -1, np.int64)
        self.metacell_row[mm.rows] = np.repeat(np.arange(len(mm.off) - 1), np.diff(mm.off))
        self.cell_map = frames.unpack_map(mm, rm, truth_member, self.with_tally)
        return True

    def record(self, frames, acc):
        rec = super().record(frames, acc)
        mm, rm = self.members
        counts, marks = self._infeasible_as_the_reference(
            lambda: acc.unpack_map(mm, rm, self.unpack, self.cell_rank_dev, self.cell_map, marks=self.per_result))
        rec.update(unpack_record(counts[1], counts[2]))
        if self.cell_truth_row is not None:
            rec.update(cell_truth_record(counts[4], counts[5]))
        if self.per_result:
            self.cell_cells.append(self.cells_from_member_marks(marks))
        return rec

    def cells_from_member_marks(self, marks):
        """`_cell_cells_frame` of the library's marks (windows.MEMBER_MARK, one per moving member): a member's mark is its cell's, a cell
        in no list is unmatched"""
        mm, rm = self.members
        n_mov = len(self.moving_mc.original_df)
        f = marks["flags"]
        bit = lambda b: (f & b) != 0

        def per_cell(values, idle, dtype):
            out = np.full(n_mov, idle, dtype)
            out[mm.rows] = values
            return out

        matched = bit(_lib.SAME_MARK_MATCHED)
        ref_cell = np.where(matched, rm.rows[np.maximum(marks["ref_member"], 0)] if len(rm.rows) else -1, -1)
        truth = ranks = None
        if self.cell_truth_row is not None:
            known = self.cell_truth_row >= 0                      # (a cell in no list has no mark: its truth is the host's)
            known[mm.rows] = bit(_lib.SAME_MARK_TRUTH_KNOWN)
            truth = (known, per_cell(bit(_lib.SAME_MARK_ON_TRUTH), False, bool))
        if self.ranks:
            ranks = (per_cell(marks["rank_strict"], UNRANKED, np.uint8), per_cell(marks["rank_weak"], UNRANKED, np.uint8),
                     per_cell(bit(_lib.SAME_MARK_RANKED), False, bool))
        return _cell_cells_frame(self.ref_mc, self.moving_mc, self.metacell_row, per_cell(ref_cell, -1, np.int64),
                                 per_cell(marks["ref_row"], -1, np.int64), per_cell(marks["pair"], -1, np.int64),
                                 per_cell(bit(_lib.SAME_MARK_TYPE_MATCH), False, bool), truth, ranks)

    def finished(self, frames):
        """both tallies read from the device once, after the last result; the maps are closed with them"""
        super().finished(frames)
        if self.cell_map is not None:
            self.cell_tally_words, self.n_cell_results = self.cell_map.tally()
            held = frames.__dict__.get("_unpack_maps", [])
            if self.cell_map in held:
                held.remove(self.cell_map)
            self.cell_map.close()
            self.cell_map = None


def sliding_window_score_maps(ref, moving, commonCT=None, *, truth=None, ranks=False, per_result=True, tally=True, type_variants=None,
                              param_sets=None, optim_params=None, gurobi_params=None, score_delaunay=None, score_delaunay_vertex_col=None,
                              score_params=None, workers=None, triangulator=None, ctx=None, batch=None, moving_delaunay=None,
                              moving_delaunay_vertex_col=None, unpack=None, cell_truth=None):
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
    `sliding_window_scores`' but for `tables`.  A truth id that names no reference cell, a truth of the wrong length, `ranks` without
    `commonCT` and what `sliding_window_scores` refuses raise ValueError before a job or a device is touched.
    On the device ONE call per result takes the score call's place (csrc/window_score_map.hip): its marks come back in one copy per
    result, the tally stays resident and is read once, after the last result.  What `scores.DeviceScores.prepare` refuses, more labels
    than the library's cap with `ranks`, and whatever keeps the job off the shared pass go through `score_table_maps` on the tables:
    the same frames, nothing saved; the tally is then the sum over them.
    `unpack` ("distribute" / "nearest"; `ref` and `moving` MetaCell objects, `checked_unpack`'s rules): the maps at CELL level as well
     -> `CellScoreMaps`, the three fields above -- `scores` with UNPACK_KEYS, as `sliding_window_scores(unpack=)` gives them
    -- and
      cell_cells   `cell_cells[v][s]`: one frame per result over the moving object's ORIGINAL cells, indexed by
                   `moving.original_df[original_idx_col]` in that frame's row order, with `score_unpacked_maps`' columns (the reference
                   cell every cell was put on, its metacell, its pair, matched, type_match, and the truth and rank columns); None with
                   per_result=False;
      cell_tally   one frame over the same index: `results`, `matched_in`, `type_match_in`, `on_truth_in`; None with tally=False.
    `cell_truth`: per original moving cell the `original_idx_col` id of its true or baseline reference CELL -- a Series on
    `moving.original_df`'s index, an array of its length or a dict from moving cell id to reference cell id (the objects may name their
    id columns differently); a missing value means unknown; `checked_truth`'s rules, ValueError without `unpack`.  With it `scores` gains
    `cell_truth_rows`, `cell_truth_matches` and `cell_truth_accuracy`.  `ranks=True` with `unpack` also needs the commonCT columns in
    `ref.original_df`.  Non-finite member coordinates under "nearest" raise ValueError("cost matrix is infeasible").
    On the device ONE call per result takes the unpack call's place (csrc/window_unpack_map.hip): one 16-byte mark per moving member
    in one copy, the cell tally resident until the last result.  Objects `DeviceScores.device_members` refuses, what
    `UnpackMapScores.prepare_cells` names, more than 64 cell labels with `ranks` and whatever keeps the job off the shared pass go
    through `score_unpacked_maps` on the tables: the same frames, the tally then their sum."""
    params = checked_score_params(score_params)
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    checked_unpack(unpack, ref_arg, moving_arg, no_objects=_NoMetaCellObjects)
    if cell_truth is not None and unpack is None:
        raise ValueError("cell_truth names the true reference CELLS of a MetaCell study: pass unpack=")
    if ranks and commonCT is None:
        raise ValueError("ranks=True ranks the reference cells' commonCT columns: pass commonCT")
    cid = _study_cell_id_col(ref_arg, moving_arg, optim_params)
    truth_row = checked_truth(truth, ref_df, mov_df, cid)
    cell_truth_row = None
    if unpack is not None:
        if ranks:
            lacking = [c for c in _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT) if c not in ref_arg.original_df.columns]
            if lacking:
                raise ValueError(f"ranks with unpack={unpack!r} ranks the reference cells' type columns: ref.original_df has no {lacking}")
        cell_truth_row = checked_cell_truth(cell_truth, ref_arg, moving_arg)
        hook = UnpackMapScores(score_delaunay, score_delaunay_vertex_col, params, truth_row, ranks, per_result, tally, unpack, ref_arg,
                               moving_arg, cell_truth_row)
    else:
        hook = MapScores(score_delaunay, score_delaunay_vertex_col, params, truth_row, ranks, per_result, tally)
    scores, nested, hook = _scored_study(ref, moving, commonCT, type_variants=type_variants, param_sets=param_sets, optim_params=optim_params,
                                         gurobi_params=gurobi_params, score_delaunay=score_delaunay,
                                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=params, tables=False,
                                         workers=workers, triangulator=triangulator, ctx=ctx, batch=batch, moving_delaunay=moving_delaunay,
                                         moving_delaunay_vertex_col=moving_delaunay_vertex_col, unpack=unpack, hook=hook)
    n_sets = len(nested[0])
    job = hook.job
    index = job.moving.index
    nest = lambda flat: None if flat is None else [flat[q:q + n_sets] for q in range(0, len(flat), n_sets)]
    cell_flat = cell_tally_frame = None
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
        if unpack is not None:
            cell_flat = hook.cell_cells if per_result else None
            if cell_truth_row is not None:
                for k in CELL_TRUTH_KEYS:
                    scores[k] = [rec[k] for rec in hook.records]
            if tally:
                mm = hook.members[0]
                words = np.zeros((len(moving_arg.original_df), 3), np.int64)
                words[mm.rows] = hook.cell_tally_words
                cell_index = pd.Index(moving_arg.original_df[moving_arg.original_idx_col].to_numpy(), name=moving_arg.original_idx_col)
                cell_tally_frame = pd.DataFrame({"results": np.full(len(cell_index), hook.n_cell_results, np.int64),
                                                 **{k: words[:, q] for q, k in enumerate(CELL_TALLY_KEYS[1:])}}, index=cell_index)
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
        if unpack is not None:
            tables = [t for per_set in nested for t in per_set]             # (hook.cell_tables: `_scored_study` unpacked every table already)
            cell_flat = [score_unpacked_maps(t, ref_arg, moving_arg, unpack, commonCT=cts, _truth_row=cell_truth_row, ranks=ranks, cells=c)
                         for t, c in zip(tables, hook.cell_tables)]
            if cell_truth_row is not None:
                records = [cell_truth_record(int((c["matched"] & c["truth_known"]).sum()), int(c["on_truth"].sum())) for c in cell_flat]
                for k in CELL_TRUTH_KEYS:
                    scores[k] = [rec[k] for rec in records]
            if tally:
                cell_tally_frame = cell_tally_from_cells(cell_flat, cell_flat[0].index)
        if not per_result:
            flat = cell_flat = None
    if unpack is None:
        return ScoreMaps(scores, nest(flat), tally_frame)
    return CellScoreMaps(scores, nest(flat), tally_frame, nest(cell_flat), cell_tally_frame)
