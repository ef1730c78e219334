"""What a finished window run is read by, without its table: `sliding_window_scores`.

The reference's figure notebooks (examples/heart/reproduce_figures.ipynb: Fig 3c, S4-S7) reduce every run to a few numbers:

* the share of matched cells whose `cell_type` is that of the reference cell they were put on -- `check_alignment` at kNN=1 with the
  matched cells placed ON their reference cells (SAME_X = ref_X), which asks of every row whether its own reference cell has its label;
* `check_triangle_violations`' stats over the moving frame's whole triangulation under the merged matching, and the notebooks'
  `violations` = 100 * triangles_flipped / total_triangles.

A study -- a sweep of parameter sets, type-matrix variants of the moving frame, both -- is one pass of the windows (sweep.py,
variants.py), and when a set's merge ends everything these numbers read is on the device: the merged rows as (moving section row,
reference section row), both sections' XY, the triangulation as section rows, the joint `cell_type` codes.  `sliding_window_scores` counts
there (csrc/window_score.hip, three short kernels per result) and with tables=False no table is ever made.

With MetaCell objects on both sides a study is read at CELL level (examples/luad/reproduce_figures.ipynb cell 12, examples/tongue cell 15):
the metacell matches are unpacked to cells (`unpack_metacell_matches`, strategy 'nearest' / 'distribute'), both sides' labels mapped on
and the pairs and their label agreement counted.  `unpack=` adds those numbers to every record, counted where the merged rows are
(csrc/window_unpack.hip); `score_unpacked` is the same from a result table -- the notebook cell with the functions the package
already has.

score_details.py breaks every record down by group of the moving rows, by label pair and by type rank over the same pass: its
`DetailSpec` rides on the hook below, which then makes the detail call beside the score call (csrc/window_score_detail.hip).

`score_table` is the same record from a result TABLE with the functions the package already has: what the device record must equal,
what inputs the device cannot score go through, and the tests' yardstick.  Both end in `record_from_counts`, the one place where counts
become percentages."""
import numbers
import types

import numpy as np
import pandas as pd

from . import _lib
from .eval_utils import _label_codes, check_triangle_violations
from .metacell_utils import unpack_metacell_matches
from .triangles import _as_triangle_array
from .variants import _frames_of, sliding_window_variants

# check_triangle_violations' own arguments and defaults (src/eval_utils.py:66-78)
SCORE_PARAMS = {"ignore_same_type_triangles": True, "node_local": False, "majority_threshold": 0.5, "min_flips": 1}
TRIANGLE_KEYS = ("total_triangles", "triangles_with_all_matched", "triangles_same_type_skipped", "triangles_flipped", "percent_flipped",
                 "nodes_in_violating_triangles", "percent_nodes_violating", "violations")
RECORD_KEYS = ("matched", "type_matches", "accuracy") + TRIANGLE_KEYS
# the cell-level keys of `unpack=`: rows of the unpacked table, those whose two cells' labels compare equal, their share times 100
UNPACK_KEYS = ("cells_matched", "cell_type_matches", "cell_accuracy")
UNPACK_STRATEGIES = ("distribute", "nearest")
# the longest member list the product unpacks on the device: one lane solves a row in O(n^3) (the library takes SAME_ASSIGN_MAX_MEMBERS)
UNPACK_DEVICE_MAX = 64


def checked_score_params(score_params):
    """-> SCORE_PARAMS overridden by `score_params`; ValueError for a key that is none of them or a value of the wrong type"""
    if score_params is not None and not isinstance(score_params, dict):
        raise ValueError(f"score_params must be a dict over {tuple(SCORE_PARAMS)}, not {type(score_params).__name__}")
    other = [k for k in (score_params or {}) if k not in SCORE_PARAMS]
    if other:
        raise ValueError(f"score_params has {other}: its keys are {tuple(SCORE_PARAMS)}")
    p = {**SCORE_PARAMS, **(score_params or {})}
    for k in ("ignore_same_type_triangles", "node_local"):
        if not isinstance(p[k], (bool, np.bool_)):
            raise ValueError(f"score_params[{k!r}] must be a bool, not {p[k]!r}")
        p[k] = bool(p[k])
    t = p["majority_threshold"]
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, numbers.Real) or t != t:
        raise ValueError(f"score_params['majority_threshold'] must be a number, not {t!r}")
    m = p["min_flips"]
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, numbers.Integral) or abs(int(m)) >= 2**62:
        raise ValueError(f"score_params['min_flips'] must be an int, not {m!r}")
    p["majority_threshold"], p["min_flips"] = float(t), int(m)
    return p


def record_from_counts(counts, score_params=None):
    """The score record of the integer `counts` -- a dict: `matched` (rows of the merged table), `type_matches`, and where a triangulation
    was scored against `total_triangles` (not None), `triangles_with_all_matched`, `triangles_same_type_skipped`, `triangles_flipped`
    (among the triangles that are not skipped) and `nodes_in_violating_triangles` -- or in its place `node_triangles` / `node_flips`, per
    row of the table the triangles not skipped its cell is a corner of and the flipped ones among them, which are then counted under
    `score_params` by check_triangle_violations' rule (src/eval_utils.py:199-211): any flip, or with node_local at least min_flips flips
    that are at least majority_threshold of the cell's triangles.
    The percentages are eval_utils.check_triangle_violations' own expressions: percent_flipped = 100.0 * flipped / considered (0.0 with
    none considered), percent_nodes_violating = 100.0 * (nodes / matched); accuracy = 100 * (type_matches / matched), the mean of
    check_alignment's match column times 100; violations = 100 * flipped / total_triangles, the notebooks' column.  No rows, no
    triangles: the quotient is NaN."""
    p = checked_score_params(score_params)
    over = lambda a, b: float(a) / float(b) if b else float("nan")
    matched, type_matches = int(counts["matched"]), int(counts["type_matches"])
    rec = {"matched": matched, "type_matches": type_matches, "accuracy": 100 * over(type_matches, matched)}
    if counts.get("total_triangles") is None:
        return rec
    if "nodes_in_violating_triangles" in counts:
        nodes = int(counts["nodes_in_violating_triangles"])
    else:
        n_tri, n_flip = np.asarray(counts["node_triangles"], np.int64), np.asarray(counts["node_flips"], np.int64)
        if p["node_local"]:
            with np.errstate(divide="ignore", invalid="ignore"):
                nodes = int(np.count_nonzero((n_tri > 0) & (n_flip >= p["min_flips"]) & (n_flip / n_tri >= p["majority_threshold"])))
        else:
            nodes = int(np.count_nonzero(n_flip > 0))
    total, all_matched = int(counts["total_triangles"]), int(counts["triangles_with_all_matched"])
    same, flipped = int(counts["triangles_same_type_skipped"]), int(counts["triangles_flipped"])
    considered = all_matched - same
    rec.update(total_triangles=total, triangles_with_all_matched=all_matched, triangles_same_type_skipped=same, triangles_flipped=flipped,
               percent_flipped=100.0 * flipped / considered if considered else 0.0, nodes_in_violating_triangles=nodes,
               percent_nodes_violating=100.0 * over(nodes, matched), violations=over(100 * flipped, total))
    return rec


def counts_from_words(w, total):
    """The library's eight count words -- same_merge_acc_score's out_counts, a group's record of the detail call -- under
    `record_from_counts`' keys.  Word 6, not word 5, is `triangles_flipped` (the flipped among the triangles not skipped); `total` is
    total_triangles (None: no triangulation was scored) -- word 2 leaves out the triangles that name an id the frame lacks."""
    return {"matched": int(w[0]), "type_matches": int(w[1]), "total_triangles": total, "triangles_with_all_matched": int(w[3]),
            "triangles_same_type_skipped": int(w[4]), "triangles_flipped": int(w[6]), "nodes_in_violating_triangles": int(w[7])}


def _frame_rows(frame_ids, ids, what):
    """rows of a frame named by `ids` through its id column `frame_ids` (an id that names several rows: the last, as the reference's
    dicts keep it)"""
    index = pd.Index(frame_ids)
    rows = np.arange(len(index))
    if not index.is_unique:
        keep = ~index.duplicated(keep="last")
        index, rows = index[keep], rows[keep]
    at = index.get_indexer(np.asarray(ids))
    if len(at) and at.min() < 0:
        raise ValueError(f"the table names {what} ids the frame does not have")
    return rows[at]


def score_table(table, ref, moving, *, cell_id_col, score_delaunay=None, score_delaunay_vertex_col=None, score_params=None, ctx=None):
    """The score record (`record_from_counts`) of a result table of `sliding_window_incumbent` / `_sweep` / `_variants` over the frames
    `ref` and `moving` (MetaCell objects: their `.metacell_df`), with the functions the package already has.
    The table's rows are mapped to frame rows through Aligned_<cell_id_col> / Ref_<cell_id_col>; `type_matches` compares the two frames'
    `cell_type` at those rows (labels that compare equal; a missing label equals nothing).  With `score_delaunay` -- anything
    `moving_delaunay` accepts, its vertex ids the moving frame's index labels or `score_delaunay_vertex_col`'s values -- the triangle keys
    are `check_triangle_violations`' stats, called as the reference's notebook calls it: mapped_x_col="ref_X", mapped_y_col="ref_Y", the
    table's `cell_type` assigned from the moving frame, and an object carrying the moving frame indexed by vertex id and the triangulation.
    `score_params`: `checked_score_params`.  A frame without `cell_type` raises ValueError."""
    p = checked_score_params(score_params)
    ref, moving = getattr(ref, "metacell_df", ref), getattr(moving, "metacell_df", moving)
    for df, name in ((ref, "ref"), (moving, "moving")):
        if "cell_type" not in df.columns:
            raise ValueError(f"scores compare cell types: the {name} frame has no 'cell_type' column")
    n = len(table)
    rows_m = _frame_rows(moving[cell_id_col].to_numpy(), table[f"Aligned_{cell_id_col}"].to_numpy(), "moving") if n else np.zeros(0, np.int64)
    rows_r = _frame_rows(ref[cell_id_col].to_numpy(), table[f"Ref_{cell_id_col}"].to_numpy(), "reference") if n else np.zeros(0, np.int64)
    mov_type = moving["cell_type"].to_numpy()[rows_m]
    code_m, code_r = _label_codes(mov_type, ref["cell_type"].to_numpy()[rows_r])
    counts = {"matched": n, "type_matches": int(np.count_nonzero((code_m >= 0) & (code_m == code_r)))}
    if score_delaunay is not None:
        tri = _as_triangle_array(score_delaunay)
        if score_delaunay_vertex_col is not None and score_delaunay_vertex_col not in moving.columns:
            raise ValueError(f"score_delaunay_vertex_col='{score_delaunay_vertex_col}' not in the moving frame")
        vertex_ids = moving.index.to_numpy() if score_delaunay_vertex_col is None else moving[score_delaunay_vertex_col].to_numpy()
        if not pd.Index(vertex_ids).is_unique:
            raise ValueError("the moving frame's vertex ids are not unique: its triangulation names no definite cells")
        counts.update(total_triangles=len(tri), triangles_with_all_matched=0, triangles_same_type_skipped=0, triangles_flipped=0,
                      nodes_in_violating_triangles=0)
        if n:
            out = pd.DataFrame({"__vertex_id": vertex_ids[rows_m], f"Ref_{cell_id_col}": table[f"Ref_{cell_id_col}"].to_numpy(),
                                "ref_X": table["ref_X"].to_numpy(), "ref_Y": table["ref_Y"].to_numpy(), "cell_type": mov_type})
            frame = pd.DataFrame({"X": moving["X"].to_numpy(), "Y": moving["Y"].to_numpy()}, index=vertex_ids)
            carrier = types.SimpleNamespace(metacell_df=frame, metacell_delaunay=tri)
            _out, stats = check_triangle_violations(out, carrier, aligned_id_col="__vertex_id", ref_id_col=f"Ref_{cell_id_col}",
                                                    mapped_x_col="ref_X", mapped_y_col="ref_Y", cell_type_col="cell_type", ctx=ctx, **p)
            counts.update({k: int(stats[k]) for k in ("triangles_with_all_matched", "triangles_same_type_skipped", "triangles_flipped",
                                                      "nodes_in_violating_triangles")})
    return record_from_counts(counts, p)


def unpack_record(cells_matched, cell_type_matches):
    """the cell-level keys from their two counts: cell_accuracy = (cell_type_matches / cells_matched) * 100 -- the notebooks'
    `celltype_match.mean() * 100` --, NaN with no pairs"""
    n, k = int(cells_matched), int(cell_type_matches)
    return {"cells_matched": n, "cell_type_matches": k, "cell_accuracy": (k / n) * 100 if n else float("nan")}


def checked_unpack(unpack, ref, moving, no_objects=ValueError):
    """ValueError unless `unpack` is None or a strategy and, with a strategy, `ref` and `moving` are MetaCell-like objects: `metacell_df`
    with a `members` column of lists, `original_df`, `original_idx_col` (`no_objects`: the ValueError raised for an object without them)"""
    if unpack is None:
        return
    if not isinstance(unpack, str) or unpack not in UNPACK_STRATEGIES:
        raise ValueError(f"unpack must be None or one of {UNPACK_STRATEGIES}, not {unpack!r}")
    for obj, name in ((ref, "ref"), (moving, "moving")):
        lacking = [f for f in ("metacell_df", "original_df", "original_idx_col") if not hasattr(obj, f)]
        if lacking:
            raise no_objects(f"unpack={unpack!r} reads MetaCell objects on both sides: {name} has no {lacking}")
        frame = obj.metacell_df
        if "members" not in getattr(frame, "columns", ()) or not all(isinstance(m, list) for m in frame["members"].tolist()):
            raise ValueError(f"unpack={unpack!r}: {name}.metacell_df has no 'members' column of lists")


def score_unpacked(table, ref_mc, moving_mc, strategy):
    """The cell-level record of a result table over the MetaCell objects `ref_mc` and `moving_mc`, as the reference's notebooks make it
    (examples/luad/reproduce_figures.ipynb cell 12): `unpack_metacell_matches(table, moving_mc.metacell_df, ref_mc.metacell_df,
    aligned_df=moving_mc.original_df, ref_df=ref_mc.original_df, strategy=strategy, ...)`, both sides' labels mapped on through the
    objects' `original_idx_col`, `celltype_match` = the two labels compare equal.  -> ({cells_matched: len of the unpacked table,
    cell_type_matches: celltype_match.sum(), cell_accuracy: (cell_type_matches / cells_matched) * 100}, the unpacked table with
    Aligned_cell_id and Ref_cell_id).  What `sliding_window_scores(unpack=strategy)` must equal, and what it falls back to."""
    if not len(table):
        return unpack_record(0, 0), pd.DataFrame([])
    cells = unpack_metacell_matches(table, moving_mc.metacell_df, ref_mc.metacell_df, aligned_df=moving_mc.original_df,
                                    ref_df=ref_mc.original_df, strategy=strategy, aligned_original_idx_col=moving_mc.original_idx_col,
                                    ref_original_idx_col=ref_mc.original_idx_col, x_col=moving_mc.x_col, y_col=moving_mc.y_col)
    if not len(cells):
        return unpack_record(0, 0), cells
    label = lambda mc: mc.original_df.set_index(mc.original_idx_col)[mc.cell_type_col]
    aligned_ct, ref_ct = cells["Aligned_cell_id"].map(label(moving_mc)), cells["Ref_cell_id"].map(label(ref_mc))
    celltype_match = aligned_ct == ref_ct
    return unpack_record(len(cells), int(celltype_match.sum())), cells


class DeviceScores:
    """The score hook of `incumbent._device_pass`: what to score every job's merged rows against, and the call that does it."""

    def __init__(self, score_delaunay, vertex_col, params, tables, unpack=None, ref_mc=None, moving_mc=None, detail=None):
        self.score_delaunay, self.vertex_col, self.params, self.tables = score_delaunay, vertex_col, params, bool(tables)
        # what to break every record down by (score_details.DetailSpec; None: totals only); its resident object once `prepare` agreed
        self.detail, self.detail_dev = detail, None
        self.unpack, self.ref_mc, self.moving_mc = unpack, ref_mc, moving_mc      # the strategy (None: metacell level only), the two objects
        self.members = None      # (moving, reference) windows.DeviceMembers once `prepare` agreed
        self.cell_dev = None     # with `unpack` and `detail`: what the cell pairs are binned by (windows.DeviceUnpackDetail) once `prepare` agreed
        self.cell_tables = []    # with tables: the unpacked table per job, in the jobs' order
        self.job = None          # the first job of the pass (sliding_window_variants tells): MetaCell unwrapping, cell_id_col, its triangulation
        self.records = None      # [record per job, variants outermost] once the device scored them
        self.tris, self.total = None, None

    def triangulation(self, job):
        """(the triangulation to score against, its vertex id column): `score_delaunay`, else the job's own caller triangulation"""
        if self.score_delaunay is not None:
            return self.score_delaunay, self.vertex_col
        return (job.moving_delaunay, job.vertex_col) if job.caller_triangulation else (None, None)

    def prepare(self, frames, job):
        """Before the pass: the scoring triangulation resident beside the moving section (`frames.caller_tris`: the job's own object is the
        copy its windows select from).  -> whether the device can score these inputs: not with cell ids that name several rows of a frame
        (a merged row then names no definite cell), a `cell_type` with missing labels (the reference's same-type rule factorizes them
        into one label, the joint codes make each equal nothing) or a triangulation `caller_triangulation_rows` refuses."""
        if not frames.id_codes(job.optim_params["cell_id_col"])[1]:
            return False
        known = frames.__dict__                              # (asked once per frames: a resident_frames object serves many calls)
        if "_labels_complete" not in known:
            known["_labels_complete"] = not any(bool(pd.isna(df["cell_type"].to_numpy()).any()) for df in (job.ref, job.moving))
        if not known["_labels_complete"]:
            return False
        tri, vertex_col = self.triangulation(job)
        if tri is not None:
            self.tris = frames.caller_tris(tri, vertex_col)
            if self.tris is None:
                return False
            self.total = len(_as_triangle_array(tri))
        if self.unpack is not None:
            self.members = self.device_members(frames, job)
            if self.members is None:
                return False
        if self.detail is not None:
            self.detail_dev = self.detail.resident(frames)
            if self.detail_dev is None:
                return False
            if self.unpack is not None:
                # the cell pairs binned too (csrc/window_unpack_detail.hip): the cell-level labels' columns, the reference members' type rows
                self.cell_dev = frames.unpack_detail(self.ref_mc, self.moving_mc, frames.commonCT, self.detail.ks)
                if self.cell_dev is None:
                    return False
        return True

    def device_members(self, frames, job):
        """(moving, reference) member lists resident beside the sections, or None where the device does not unpack these objects (the
        whole call then goes through `score_unpacked` on the tables): a table that does not name metacells by `metacell_id`; metacell ids
        that are not 0 .. n-1 in row order (the reference indexes `members` with .iloc[id]); coordinate columns that differ between the
        objects; what `window_api.member_layout` refuses; a reference row without members; a list longer than UNPACK_DEVICE_MAX; an
        original label that is missing (pandas' == makes it equal nothing, the joint codes make None equal None)."""
        mov, ref = self.moving_mc, self.ref_mc
        if job.optim_params["cell_id_col"] != "metacell_id" or (mov.x_col, mov.y_col) != (ref.x_col, ref.y_col):
            return None
        for mc in (mov, ref):
            ids = mc.metacell_df[mc.metacell_idx_col].to_numpy() if mc.metacell_idx_col in mc.metacell_df.columns else None
            if mc.metacell_idx_col != "metacell_id" or ids is None or ids.dtype.kind not in "iu" or not np.array_equal(ids, np.arange(len(ids))):
                return None
            if bool(pd.isna(mc.original_df[mc.cell_type_col].to_numpy()).any()):
                return None
            counts = np.fromiter((len(m) for m in mc.metacell_df["members"].tolist()), np.int64, len(mc.metacell_df))
            if len(counts) and (counts.max() > UNPACK_DEVICE_MAX or (mc is ref and counts.min() == 0)):
                return None
        made = frames.members(mov, "moving", ref), frames.members(ref, "ref", mov)
        return None if made[0] is None or made[1] is None else made

    def record(self, frames, acc):
        """the record of the merged rows `acc` holds after its finish (windows.MergeAccumulator.score)"""
        p = self.params
        c = acc.score(frames.dmov, frames.dref, self.tris, p["ignore_same_type_triangles"], p["node_local"], p["majority_threshold"],
                      p["min_flips"])
        rec = record_from_counts(counts_from_words(c, self.total), p)             # (total_triangles: the caller's own count)
        if self.cell_dev is not None:
            # ONE call in the unpack call's place: its counts are the record's cell keys, its bins the cell-level breakdown
            rec["_cell_detail"] = d = self._infeasible_as_the_reference(
                lambda: acc.unpack_detail(*self.members, self.unpack, self.cell_dev, self.detail_dev))
            rec.update(unpack_record(d["counts"][1], d["counts"][2]))
        elif self.unpack is not None:
            rec.update(self.unpacked(acc))
        if self.detail_dev is not None:
            # the detail call beside the score call: the same rows, triangles and rule, binned (csrc/window_score_detail.hip)
            rec["_detail"] = acc.score_detail(frames.dmov, frames.dref, self.tris, self.detail_dev, p["ignore_same_type_triangles"],
                                              p["node_local"], p["majority_threshold"], p["min_flips"])
        return rec

    def finished(self, frames):
        """after the pass's last record, while the frames are still resident (a hook that keeps something on the device reads it here)"""

    def _infeasible_as_the_reference(self, call):
        """call(), an unpack call of the library: non-finite member coordinates under "nearest" raise as `unpack_metacell_matches` does"""
        try:
            return call()
        except _lib.SameHipError as e:
            if e.code == _lib.SAME_ERANGE and self.unpack == "nearest":
                raise ValueError("cost matrix is infeasible") from e
            raise

    def unpacked(self, acc):
        """the cell-level keys of the merged rows `acc` holds (windows.MergeAccumulator.unpack); with tables the unpacked table joins
        `cell_tables`: the moving rows' members in their order, each with the reference member the device gave it"""
        mm, rm = self.members
        got = self._infeasible_as_the_reference(lambda: acc.unpack(mm, rm, self.unpack, pairs=self.tables))
        counts, ref_member = got if self.tables else (got, None)
        if self.tables:
            a = acc.final_rows()["a_row"].astype(np.int64)
            n_a = mm.off[a + 1] - mm.off[a]
            within = np.arange(int(n_a.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_a) - n_a, n_a)
            mov_member = np.repeat(mm.off[a], n_a) + within
            self.cell_tables.append(pd.DataFrame({"Aligned_cell_id": mm.ids[mov_member], "Ref_cell_id": rm.ids[ref_member]})
                                    if len(mov_member) else pd.DataFrame([]))
        return unpack_record(counts[1], counts[2])


def sliding_window_scores(ref, moving, commonCT=None, *, type_variants=None, param_sets=None, optim_params=None, gurobi_params=None,
                          score_delaunay=None, score_delaunay_vertex_col=None, score_params=None, tables=False, workers=None,
                          triangulator=None, ctx=None, batch=None, moving_delaunay=None, moving_delaunay_vertex_col=None, unpack=None):
    """The score records of `sliding_window_variants(ref, moving, type_variants, commonCT, param_sets=param_sets, merge=True, ...)` over one
    pass of the windows, counted on the device from every result's merged rows: -> a DataFrame with one row per (variant, set), variants
    outermost, in the callers' order; with tables=True (scores, tables), `tables[v][s]` that call's tables.  `type_variants=None`: the
    frame's own types alone; `param_sets=None`: one set, {}.  Without tables no table is made: no columns gathered, no frame built.
    Columns: `variant`, `set` (indices into the callers' lists), then RECORD_KEYS -- `matched` (rows of the merged table), `type_matches`
    (rows whose moving cell's `cell_type` compares equal to its matched reference cell's), `accuracy`, and `check_triangle_violations`'
    stats with `violations` = 100 * triangles_flipped / total_triangles (`record_from_counts`).  The triangle columns are left out when
    there is no triangulation to score against.
    `score_delaunay`: the triangulation of the moving frame to score against -- anything `moving_delaunay` accepts, ids read through
    `score_delaunay_vertex_col` --, used for scoring only; None: the job's own caller triangulation (a MetaCell object's, or
    `moving_delaunay=`).  On plain frames: scipy.spatial.Delaunay(moving[["X", "Y"]]).simplices.  `score_params`: a dict over SCORE_PARAMS,
    check_triangle_violations' arguments.  The other arguments are `sliding_window_variants`' and are checked by its checks; an unknown
    `score_params` key, a value of the wrong type or a frame without `cell_type` raise ValueError before a job or a device is touched.
    `unpack` ("distribute" / "nearest"; `ref` and `moving` MetaCell objects): every record gains UNPACK_KEYS -- `cells_matched`, the rows of
    `unpack_metacell_matches` of the result under that strategy, `cell_type_matches`, those whose two cells' labels compare equal, and
    `cell_accuracy` (`unpack_record`) --, counted on the device from the merged rows and the objects' member lists resident beside the
    sections (csrc/window_unpack.hip); with tables=True -> (scores, tables, cell_tables), `cell_tables[v][s]` that unpacked table.  Every
    record and table equals `score_unpacked` of its table, which is also what objects the device does not unpack go through
    (`DeviceScores.device_members` names them).  An unknown `unpack`, or objects without `metacell_df` / `original_df` /
    `original_idx_col` / a `members` column of lists, raise ValueError first; non-finite member coordinates under "nearest" raise
    ValueError("cost matrix is infeasible") as `unpack_metacell_matches` does.
    Every record equals `score_table` of its table.  Inputs the device cannot score -- whatever keeps the job off the shared device pass
    (`sliding_window_sweep` lists it), and what `DeviceScores.prepare` names -- go through `score_table` on the tables: the same records,
    nothing saved."""
    scores, nested, hook = _scored_study(ref, moving, commonCT, type_variants=type_variants, param_sets=param_sets, optim_params=optim_params,
                                         gurobi_params=gurobi_params, score_delaunay=score_delaunay,
                                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=score_params, tables=tables,
                                         workers=workers, triangulator=triangulator, ctx=ctx, batch=batch, moving_delaunay=moving_delaunay,
                                         moving_delaunay_vertex_col=moving_delaunay_vertex_col, unpack=unpack)
    if tables and unpack is not None:
        n_sets = len(nested[0])
        return scores, nested, [hook.cell_tables[q:q + n_sets] for q in range(0, len(scores), n_sets)]
    return (scores, nested) if tables else scores


def _scored_study(ref, moving, commonCT, *, type_variants, param_sets, optim_params, gurobi_params, score_delaunay,
                  score_delaunay_vertex_col, score_params, tables, workers, triangulator, ctx, batch, moving_delaunay,
                  moving_delaunay_vertex_col, unpack, detail=None, hook=None):
    """`sliding_window_scores`' pass -> (its scores frame, the results per variant and set -- tables, or None where the device scored
    and none was asked for --, the hook: `hook.records` is None where the host scored the tables).  With `detail`
    (score_details.DetailSpec) every record of the device carries the detail call's words under "_detail".  `hook`: a DeviceScores
    variant made by the caller to ride on the pass in the plain one's place (score_maps.MapScores)."""
    params = checked_score_params(score_params)
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    checked_unpack(unpack, ref_arg, moving_arg)
    for df, name in ((ref_df, "ref"), (mov_df, "moving")):
        if "cell_type" not in getattr(df, "columns", ()):
            raise ValueError(f"scores compare cell types: the {name} frame has no 'cell_type' column")
    if score_delaunay is not None:
        _as_triangle_array(score_delaunay)                  # (its shape: the reference's ValueError)
    if hook is None:
        hook = DeviceScores(score_delaunay, score_delaunay_vertex_col, params, tables, unpack, ref_arg, moving_arg, detail)
    results = sliding_window_variants(ref, moving, [None] if type_variants is None else type_variants, commonCT, param_sets=param_sets,
                                      optim_params=optim_params, gurobi_params=gurobi_params, workers=workers, triangulator=triangulator,
                                      ctx=ctx, merge=True, batch=batch, moving_delaunay=moving_delaunay,
                                      moving_delaunay_vertex_col=moving_delaunay_vertex_col, _score=hook)
    nested = [[r] if param_sets is None else list(r) for r in results]
    records = hook.records
    if records is None:                                     # not scored on the device: the host statement on every table
        job = hook.job
        tri, vertex_col = hook.triangulation(job)
        records = [score_table(t, job.ref, job.moving, cell_id_col=job.optim_params["cell_id_col"], score_delaunay=tri,
                               score_delaunay_vertex_col=vertex_col, score_params=params, ctx=ctx) for per_set in nested for t in per_set]
        if unpack is not None:
            cells = [score_unpacked(t, ref_arg, moving_arg, unpack) for per_set in nested for t in per_set]
            records = [{**rec, **cell_rec} for rec, (cell_rec, _t) in zip(records, cells)]
            hook.cell_tables = [t for _rec, t in cells]
    n_sets = len(nested[0])
    rows = [{"variant": q // n_sets, "set": q % n_sets, **rec} for q, rec in enumerate(records)]
    scores = pd.DataFrame(rows, columns=["variant", "set"] + [k for k in RECORD_KEYS + UNPACK_KEYS if k in rows[0]])
    return scores, nested, hook
