"""A study's scores broken down by group, label pair and type rank: `sliding_window_score_details`.

`sliding_window_scores` reduces every result of a study to one record.  The reference's notebooks read every table three more ways:

* per region -- examples/synthetic/reproduce_figures.ipynb (Fig 2, FigS1) counts triangle violations within quadrants
  (src/synthetic_datagen.py:1314-1418): only triangles whose three corners lie in one quadrant count, each quadrant is reported alone;
* per label pair -- which `cell_type` was put on which, the crosstab behind every accuracy figure;
* per type rank -- examples/luad/reproduce_figures.ipynb cell 13 (FigS19): is the moving cell's label among the k largest commonCT
  columns of its matched reference cell, for k = 1, 2, 3.

Everything the three read is resident when a set's merge ends, so `sliding_window_score_details` bins there
(csrc/window_score_detail.hip, the detail call beside the score call) and no table is made.  `score_table_details` is the same from a
result TABLE with the functions the package already has: what the device must equal and what inputs the device refuses go through.
`top_k_counts` is the host statement of the rank rule; it works on any list of pairs, so the cell-level top-k of an unpacked table is
one call of it on `cell_tables`.

With MetaCell objects and `unpack=` the same three readings are made at CELL level as well: the notebook's FigS19 asks
of every unpacked cell pair whether the moving cell's label is among the k largest type columns of the reference CELL it was put on --
another number than the metacell rows' rank count, a metacell's type row being a mean over its members.  The pairs are binned where the
unpack call makes them (csrc/window_unpack_detail.hip: the reference members' type rows resident, one kernel behind the solve kernel);
`score_unpacked_details` is the host statement per table, and what the device refuses goes through it."""
import collections
import collections.abc
import numbers
import types

import numpy as np
import pandas as pd

from . import _lib
from .eval_utils import _label_codes, check_triangle_violations
from .scores import (RECORD_KEYS, UNPACK_KEYS, _frame_rows, _scored_study, checked_score_params, checked_unpack, counts_from_words,
                     record_from_counts, score_table, score_unpacked, unpack_record)
from .triangles import _as_triangle_array
from .variants import _common_types, _frames_of

ScoreDetails = collections.namedtuple("ScoreDetails", "scores confusion groups cross top_k")
CellDetails = collections.namedtuple("CellDetails", "cell_confusion cell_groups cell_cross cell_top_k")
CellScoreDetails = collections.namedtuple("CellScoreDetails", ScoreDetails._fields + CellDetails._fields)
MAX_TOP_K = _lib.SAME_SCORE_RANKS
# the cross record: RECORD_KEYS without the node counts (a node is counted in its own group)
CROSS_KEYS = tuple(k for k in RECORD_KEYS if k not in ("nodes_in_violating_triangles", "percent_nodes_violating"))


class _NoMetaCellObjects(ValueError, TypeError):
    """`sliding_window_score_details(unpack=...)` over something that is no MetaCell object.  Callers are told ValueError, as for every
    refusal; it is a TypeError too only because the call raised that for `unpack` over plain frames before it had the keyword
    (tests/test_score_details_cpu.py still asserts it).  Private: to become a plain ValueError once that assertion is retired."""


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def checked_top_k(top_k):
    """-> the ks ascending, () for None; ValueError unless `top_k` is a collection of ints in 1 .. MAX_TOP_K"""
    if top_k is None:
        return ()
    if isinstance(top_k, (str, bytes, dict)) or not isinstance(top_k, collections.abc.Iterable):
        raise ValueError(f"top_k must be a set of ints in 1..{MAX_TOP_K}, not {top_k!r}")
    ks = list(top_k)
    for k in ks:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= MAX_TOP_K:
            raise ValueError(f"top_k must be a set of ints in 1..{MAX_TOP_K}, not {top_k!r}")
    return tuple(sorted({int(k) for k in ks}))


def checked_groups(group_by, moving_df):
    """-> (int32 group code per row of the moving frame, -1 where the value is missing; the groups in pd.factorize order), or
    (None, None) for None.  `group_by`: a column of the moving frame or an array of its length; ValueError otherwise"""
    if group_by is None:
        return None, None
    if isinstance(group_by, str):
        if group_by not in moving_df.columns:
            raise ValueError(f"group_by='{group_by}' is not a column of the moving frame")
        values = moving_df[group_by].to_numpy()
    else:
        values = np.asarray(group_by)
        if values.ndim != 1 or len(values) != len(moving_df):
            raise ValueError(f"group_by must be a column of the moving frame or an array of its {len(moving_df)} rows")
    codes, names = pd.factorize(values)
    return codes.astype(np.int32), list(names)


def joint_labels(mov_labels, ref_labels):
    """-> (moving codes, reference codes, the labels in the codes' order): `_label_codes` of the two frames' labels -- equal non-negative
    codes <=> labels that compare equal, a missing label is negative --, code q naming labels[q]"""
    code_m, code_r = _label_codes(mov_labels, ref_labels)
    both = pd.concat([pd.Series(mov_labels).reset_index(drop=True), pd.Series(ref_labels).reset_index(drop=True)], ignore_index=True)
    labels = list(pd.factorize(both)[1])
    top = max(int(code_m.max()) if len(code_m) else -1, int(code_r.max()) if len(code_r) else -1)
    if top == len(labels):                 # (None equals None: the code after the labels')
        labels.append(None)
    return code_m, code_r, labels


def label_columns(labels, columns):
    """-> int32 per label: the position in `columns` of the column the label names (the first of equal names), -1 where it names none"""
    cols = pd.Index(list(columns), dtype=object)
    first = np.flatnonzero(~cols.duplicated())
    at = cols[first].get_indexer(pd.Index(list(labels), dtype=object)) if len(labels) else np.zeros(0, np.int64)
    return np.where(at >= 0, first[np.maximum(at, 0)] if len(first) else -1, -1).astype(np.int32)


# ---- the rank rule -----------------------------------------------------------------------------------------------------------------------
def label_ranks(mov_labels, ref_type_rows, columns):
    """Per pair (moving label, matched reference cell's type row over `columns`): with c the column the label names and v the row's value
    there, `strict` = how many OTHER columns hold a value > v, `weak` = how many hold one >= v (float64 comparisons); `typed` = the label
    names a column and the row holds no NaN -- where it is False the two counts mean nothing.  -> (strict, weak, typed)"""
    labels = np.asarray(mov_labels, dtype=object)
    rows = np.asarray(ref_type_rows, dtype=np.float64).reshape(len(labels), len(list(columns)))
    c = label_columns(labels, columns).astype(np.int64)
    typed = (c >= 0) & ~np.isnan(rows).any(axis=1)
    at = np.arange(len(labels))
    with np.errstate(invalid="ignore"):
        v = rows[at, np.maximum(c, 0)] if rows.shape[1] else np.zeros(len(labels))
        greater, at_least = rows > v[:, None], rows >= v[:, None]
    if rows.shape[1]:
        at_least[at, np.maximum(c, 0)] = False
    return greater.sum(axis=1).astype(np.int64), at_least.sum(axis=1).astype(np.int64), typed


def top_k_counts(mov_labels, ref_type_rows, columns, ks):
    """Is a moving cell's label among the k largest type columns of the reference cell it was put on?  For every k of `ks` ->
    `top{k}_matches`, the pairs with fewer than k other columns at or above the label's (`weak < k`: in the top k however ties are
    ordered), and `top{k}_tied`, the pairs whose answer depends on the order of tied columns (`strict < k <= weak`); `typed_rows`, the
    pairs that were ranked at all (`label_ranks`).  Where no tie sits at the k-th place `matches` is what np.argpartition's k largest
    give, and under any tie order the count lies in [matches, matches + tied]."""
    ks = checked_top_k(ks)
    strict, weak, typed = label_ranks(mov_labels, ref_type_rows, columns)
    out = {"typed_rows": int(typed.sum())}
    for k in ks:
        out[f"top{k}_matches"] = int(np.count_nonzero(typed & (weak < k)))
        out[f"top{k}_tied"] = int(np.count_nonzero(typed & (strict < k) & (weak >= k)))
    return out


def _top_k_from_histograms(strict_hist, weak_hist, ks):
    """`top_k_counts` from the histograms of min(strict, R) and min(weak, R): weak < k implies strict < k, so tied = #(strict < k) - #(weak < k)"""
    out = {"typed_rows": int(np.sum(weak_hist))}
    for k in ks:
        matches = int(np.sum(weak_hist[:k]))
        out[f"top{k}_matches"], out[f"top{k}_tied"] = matches, int(np.sum(strict_hist[:k])) - matches
    return out


# ---- counts to frames: one way for the host's counts and the device's --------------------------------------------------------------------
def _frames_of_counts(counts, labels, group_names, ks, params):
    """One table's ScoreDetails but for `scores`, from its integer counts: `confusion` (L, L); `groups` a record_from_counts dict per
    group and `cross` one for the rest (None: no groups asked for); `ranks` top_k_counts' dict (None: no top_k)"""
    over = lambda a, b: float(a) / float(b) if b else float("nan")
    confusion = pd.DataFrame(np.asarray(counts["confusion"], np.int64).reshape(len(labels), len(labels)),
                             index=pd.Index(labels, dtype=object, name="moving_label"), columns=pd.Index(labels, dtype=object))
    groups = cross = top = None
    if group_names is not None:
        records = [{"group": name, **record_from_counts(c, params)} for name, c in zip(group_names, counts["groups"])]
        rest = record_from_counts(counts["cross"], params)             # (with or without the triangle keys, as every group's)
        groups = pd.DataFrame(records, columns=["group"] + [k for k in RECORD_KEYS if k in rest])
        cross = pd.DataFrame([{k: rest[k] for k in CROSS_KEYS if k in rest}])
    if ks:
        ranks, matched = counts["ranks"], int(counts["matched"])
        row = {"typed_rows": ranks["typed_rows"]}
        for k in ks:
            row.update({f"top{k}_matches": ranks[f"top{k}_matches"], f"top{k}_tied": ranks[f"top{k}_tied"],
                        f"top{k}_accuracy": 100 * over(ranks[f"top{k}_matches"], matched)})
        top = pd.DataFrame([row])
    return confusion, groups, cross, top


def _stacked(per_table, n_sets):
    """the per-table frames of a study under (variant, set), variants outermost"""
    def stack(which, index_name=None):
        parts = []
        for q, frames in enumerate(per_table):
            f = frames[which]
            if f is None:
                return None
            f = f.reset_index() if index_name else f.copy()
            f.insert(0, "set", q % n_sets)
            f.insert(0, "variant", q // n_sets)
            parts.append(f)
        out = pd.concat(parts, ignore_index=True)
        return out.set_index(["variant", "set", index_name]) if index_name else out
    return stack(0, "moving_label"), stack(1), stack(2), stack(3)


# ---- from a table: the host statement ----------------------------------------------------------------------------------------------------
def _table_counts(table, ref, moving, cell_id_col, columns, group_codes, n_groups, ks, tri, vertex_col, p, ctx):
    """a result table's counts for `_frames_of_counts` with the functions the package already has"""
    n = len(table)
    rows_m = _frame_rows(moving[cell_id_col].to_numpy(), table[f"Aligned_{cell_id_col}"].to_numpy(), "moving") if n else np.zeros(0, np.int64)
    rows_r = _frame_rows(ref[cell_id_col].to_numpy(), table[f"Ref_{cell_id_col}"].to_numpy(), "reference") if n else np.zeros(0, np.int64)
    code_m, code_r, labels = joint_labels(moving["cell_type"].to_numpy(), ref["cell_type"].to_numpy())
    L = len(labels)
    cm, cr = code_m[rows_m].astype(np.int64), code_r[rows_r].astype(np.int64)
    in_cell = (cm >= 0) & (cr >= 0)
    confusion = np.bincount(cm[in_cell] * L + cr[in_cell], minlength=L * L).astype(np.int64)
    agree = (cm >= 0) & (cm == cr)
    counts = {"matched": n, "confusion": confusion, "unlabelled": int(n - in_cell.sum())}
    if group_codes is not None:
        row_group = group_codes[rows_m]
        with_tris = tri is not None
        per = [{"matched": int(np.count_nonzero(row_group == g)), "type_matches": int(np.count_nonzero(agree & (row_group == g)))}
               for g in range(n_groups)]
        rest = {"matched": int(np.count_nonzero(row_group < 0)), "type_matches": int(np.count_nonzero(agree & (row_group < 0)))}
        if with_tris:
            vertex_ids = moving.index.to_numpy() if vertex_col is None else moving[vertex_col].to_numpy()
            if not pd.Index(vertex_ids).is_unique:
                raise ValueError("the moving frame's vertex ids are not unique: its triangulation names no definite cells")
            corner = pd.Index(vertex_ids).get_indexer(tri.reshape(-1)).reshape(-1, 3)
            g3 = np.where(corner >= 0, group_codes[np.maximum(corner, 0)], -1) if len(group_codes) else np.full(corner.shape, -1)
            tri_group = np.where((g3[:, 0] >= 0) & (g3[:, 0] == g3[:, 1]) & (g3[:, 0] == g3[:, 2]), g3[:, 0], -1)
            out = frame = None
            if n:
                out = pd.DataFrame({"__vertex_id": vertex_ids[rows_m], f"Ref_{cell_id_col}": table[f"Ref_{cell_id_col}"].to_numpy(),
                                    "ref_X": table["ref_X"].to_numpy(), "ref_Y": table["ref_Y"].to_numpy(),
                                    "cell_type": moving["cell_type"].to_numpy()[rows_m]})
                frame = pd.DataFrame({"X": moving["X"].to_numpy(), "Y": moving["Y"].to_numpy()}, index=vertex_ids)
            keys = ("triangles_with_all_matched", "triangles_same_type_skipped", "triangles_flipped", "nodes_in_violating_triangles")

            def restricted(which):
                """check_triangle_violations over the triangles `which` alone"""
                stats = dict.fromkeys(keys, 0)
                if n and which.any():
                    carrier = types.SimpleNamespace(metacell_df=frame, metacell_delaunay=tri[which])
                    _out, got = check_triangle_violations(out, carrier, aligned_id_col="__vertex_id", ref_id_col=f"Ref_{cell_id_col}",
                                                          mapped_x_col="ref_X", mapped_y_col="ref_Y", cell_type_col="cell_type", ctx=ctx, **p)
                    stats = {k: int(got[k]) for k in keys}
                return {"total_triangles": int(which.sum()), **stats}

            for g in range(n_groups):
                per[g].update(restricted(tri_group == g))
            rest.update(restricted(tri_group < 0))
            rest["nodes_in_violating_triangles"] = 0                # (a node is counted in its own group)
        counts["groups"], counts["cross"] = per, rest
    if ks:
        counts["ranks"] = top_k_counts(moving["cell_type"].to_numpy()[rows_m], ref[list(columns)].to_numpy(dtype=np.float64)[rows_r]
                                       if n else np.zeros((0, len(columns))), columns, ks)
    return counts, labels


def score_table_details(table, ref, moving, *, cell_id_col, commonCT, group_by=None, top_k=None, score_delaunay=None,
                        score_delaunay_vertex_col=None, score_params=None, ctx=None):
    """`ScoreDetails` of ONE result table of `sliding_window_incumbent` / `_sweep` / `_variants` over the frames `ref` and `moving`
    (MetaCell objects: their `.metacell_df`), with the functions the package already has -- what `sliding_window_score_details` must
    equal, without the `variant` and `set` columns:
      scores     `score_table`'s record, one row;
      confusion  rows the moving labels, one int64 column per reference label, labels in the order of the two frames' joint codes
                 (`joint_labels`: the moving frame's labels first, as met); a row with a missing label on either side is in no cell;
      groups     one row per group of `group_by` (`checked_groups`: pd.factorize order): `group`, then `record_from_counts` over the
                 group's rows and -- with `score_delaunay` -- over `check_triangle_violations` on the triangulation restricted to the
                 triangles whose three corners lie in the group;
      cross      one row: the rows without a group, and the triangles that are in no group -- corners in different groups, in none, or
                 naming an id the frame lacks; `total_triangles` is the caller's total minus the groups'; no node counts, a node is
                 counted in its own group;
      top_k      one row: `top_k_counts` of (the row's moving label, its reference cell's `commonCT` columns) and `top{k}_accuracy` =
                 100 * matches / rows.
    `groups` and `cross` are None without `group_by`, `top_k` is None without `top_k`.  The other arguments are `score_table`'s."""
    p = checked_score_params(score_params)
    ks = checked_top_k(top_k)
    ref, moving = getattr(ref, "metacell_df", ref), getattr(moving, "metacell_df", moving)
    for df, name in ((ref, "ref"), (moving, "moving")):
        if "cell_type" not in df.columns:
            raise ValueError(f"scores compare cell types: the {name} frame has no 'cell_type' column")
    group_codes, group_names = checked_groups(group_by, moving)
    tri = None if score_delaunay is None else np.asarray(_as_triangle_array(score_delaunay)).reshape(-1, 3)
    if score_delaunay_vertex_col is not None and score_delaunay_vertex_col not in moving.columns:
        raise ValueError(f"score_delaunay_vertex_col='{score_delaunay_vertex_col}' not in the moving frame")
    record = score_table(table, ref, moving, cell_id_col=cell_id_col, score_delaunay=score_delaunay,
                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=p, ctx=ctx)
    counts, labels = _table_counts(table, ref, moving, cell_id_col, list(commonCT), group_codes, 0 if group_names is None else len(group_names),
                                   ks, tri, score_delaunay_vertex_col, p, ctx)
    scores = pd.DataFrame([record], columns=[k for k in RECORD_KEYS if k in record])
    return ScoreDetails(scores, *_frames_of_counts(counts, labels, group_names, ks, p))


# ---- at cell level: the unpacked pairs ---------------------------------------------------------------------------------------------------
def _cell_frames_of_counts(counts, labels, group_names, ks):
    """One table's `CellDetails` from its integer counts: `pairs`; `confusion` (L, L) over the cell-level labels; `groups` a (pairs,
    agreeing pairs) per group and `cross` one for the rest (None: no groups asked for); `ranks` top_k_counts' dict (None: no top_k)"""
    over = lambda a, b: float(a) / float(b) if b else float("nan")
    confusion = pd.DataFrame(np.asarray(counts["confusion"], np.int64).reshape(len(labels), len(labels)),
                             index=pd.Index(labels, dtype=object, name="moving_label"), columns=pd.Index(labels, dtype=object))
    groups = cross = top = None
    if group_names is not None:
        groups = pd.DataFrame([{"group": name, **unpack_record(*c)} for name, c in zip(group_names, counts["groups"])],
                              columns=("group",) + UNPACK_KEYS)
        cross = pd.DataFrame([unpack_record(*counts["cross"])], columns=UNPACK_KEYS)
    if ks:
        ranks, pairs = counts["ranks"], int(counts["pairs"])
        row = {"typed_rows": ranks["typed_rows"]}
        for k in ks:
            row.update({f"top{k}_matches": ranks[f"top{k}_matches"], f"top{k}_tied": ranks[f"top{k}_tied"],
                        f"top{k}_accuracy": 100 * over(ranks[f"top{k}_matches"], pairs)})
        top = pd.DataFrame([row])
    return CellDetails(confusion, groups, cross, top)


def score_unpacked_details(table, ref_mc, moving_mc, strategy, *, commonCT, group_by=None, top_k=None, cells=None):
    """`CellDetails` of ONE result table over the MetaCell objects `ref_mc` and `moving_mc`, with the functions the package already has
    -- what `sliding_window_score_details(unpack=strategy)` must equal per table, without the `variant` and `set` columns, and what it
    falls back to.  The pairs are `score_unpacked`'s unpacked table (examples/luad/reproduce_figures.ipynb cell 12), which lists them in
    the order of the table's rows and of each moving row's members:
      cell_confusion  rows the moving cells' labels, one int64 column per reference cell label, labels in the order of the joint codes
                      of the two objects' `original_df[cell_type_col]` (`joint_labels`); np.bincount over the codes;
      cell_groups     one row per group of `group_by` -- a column of `moving_mc.metacell_df` or an array of its length; a pair is in its
                      metacell row's group, np.repeat of the row's group over its member count --: `group` and UNPACK_KEYS;
      cell_cross      one row: UNPACK_KEYS over the pairs of rows without a group;
      cell_top_k      one row: `top_k_counts` of (the moving cell's label, `ref_mc.original_df[commonCT]` at the row of Ref_cell_id) --
                      the notebook's cell 13 --, and `top{k}_accuracy` = 100 * matches / cells_matched.
    `cell_groups` and `cell_cross` are None without `group_by`, `cell_top_k` is None without `top_k`.  `cells`: `score_unpacked`'s unpacked
    table of `table` under `strategy` where the caller has it already (it is not made again)."""
    ks = checked_top_k(top_k)
    columns = list(commonCT)
    group_codes, group_names = checked_groups(group_by, moving_mc.metacell_df)
    if cells is None:
        _record, cells = score_unpacked(table, ref_mc, moving_mc, strategy)
    n = len(cells)
    mov_labels, ref_labels = (mc.original_df[mc.cell_type_col].to_numpy() for mc in (moving_mc, ref_mc))
    code_m, code_r, labels = joint_labels(mov_labels, ref_labels)
    L = len(labels)
    rows_of = lambda mc, ids, what: _frame_rows(mc.original_df[mc.original_idx_col].to_numpy(), ids.to_numpy(), what)
    rows_m = rows_of(moving_mc, cells["Aligned_cell_id"], "moving") if n else np.zeros(0, np.int64)
    rows_r = rows_of(ref_mc, cells["Ref_cell_id"], "reference") if n else np.zeros(0, np.int64)
    cm, cr = code_m[rows_m].astype(np.int64), code_r[rows_r].astype(np.int64)
    in_cell = (cm >= 0) & (cr >= 0)
    agree = (cm >= 0) & (cm == cr)
    counts = {"pairs": n, "confusion": np.bincount(cm[in_cell] * L + cr[in_cell], minlength=L * L).astype(np.int64),
              "unlabelled": int(n - in_cell.sum())}
    if group_codes is not None:
        lists = moving_mc.metacell_df["members"].tolist()
        a_ids = table["Aligned_metacell_id"].to_numpy().astype(np.int64) if n else np.zeros(0, np.int64)
        pair_group = np.repeat(group_codes[a_ids], [len(lists[a]) for a in a_ids.tolist()]) if n else np.zeros(0, np.int32)
        assert len(pair_group) == n
        counts["groups"] = [(int(np.count_nonzero(pair_group == g)), int(np.count_nonzero(agree & (pair_group == g))))
                            for g in range(len(group_names))]
        counts["cross"] = (int(np.count_nonzero(pair_group < 0)), int(np.count_nonzero(agree & (pair_group < 0))))
    if ks:
        types = ref_mc.original_df[columns].to_numpy(dtype=np.float64)[rows_r] if n else np.zeros((0, len(columns)))
        counts["ranks"] = top_k_counts(mov_labels[rows_m], types, columns, ks)
    return _cell_frames_of_counts(counts, labels, group_names, ks)


def _cell_counts_of_words(d, group_names, ks):
    """the device's words of one result (windows.split_unpack_detail) as `_cell_frames_of_counts` reads them"""
    out = {"pairs": int(d["counts"][1]), "confusion": d["confusion"], "unlabelled": d["unlabelled"]}
    if group_names is not None:
        out["groups"] = [tuple(int(x) for x in w) for w in d["groups"][:len(group_names)]]
        out["cross"] = tuple(int(x) for x in d["groups"][len(group_names):].sum(axis=0))     # (no group at all: as DetailSpec.counts)
    if ks:
        out["ranks"] = _top_k_from_histograms(d["strict"], d["weak"], ks)
    return out


# ---- on the device -------------------------------------------------------------------------------------------------------------------------
class DetailSpec:
    """What `scores.DeviceScores` breaks every record down by: the moving rows' group codes and names (None: no groups), the ks."""

    def __init__(self, group_codes, group_names, ks):
        self.group_codes, self.group_names, self.ks = group_codes, group_names, ks
        self.labels = None                     # the frames' labels in their joint codes' order, once `resident` looked

    def resident(self, frames):
        """the resident object of these groups and of the frames' label columns (`frames.score_detail`), or None where the library's
        caps refuse them: more labels than SAME_SCORE_MAX_LABELS, more groups than SAME_SCORE_MAX_GROUPS"""
        _cm, _cr, labels = joint_labels(frames.moving["cell_type"].to_numpy(), frames.ref["cell_type"].to_numpy())
        self.labels = labels                   # (kept: the frames' indices are made of them)
        n_groups = 1 if self.group_names is None else max(len(self.group_names), 1)
        if len(labels) > _lib.SAME_SCORE_MAX_LABELS or n_groups > _lib.SAME_SCORE_MAX_GROUPS:
            return None
        cols = label_columns(labels, frames.commonCT) if self.ks else None
        return frames.score_detail(self.group_codes, n_groups, len(labels), cols)

    def counts(self, record, labels, total):
        """the device's words of one result (`record["_detail"]`, windows.split_score_detail) as `_frames_of_counts` reads them;
        `total`: the caller's triangle count, None without a triangulation"""
        d = record["_detail"]
        word = lambda w: counts_from_words(w, None if total is None else int(w[2]))      # (a group's triangles: the resident ones in it)
        out = {"matched": int(record["matched"]), "confusion": d["confusion"], "unlabelled": d["unlabelled"]}
        if self.group_names is not None:
            n_groups = len(self.group_names)
            out["groups"] = [word(w) for w in d["groups"][:n_groups]]
            rest = d["groups"][n_groups:].sum(axis=0)          # (no group at all: the library's one group holds what is in none)
            out["cross"] = word(rest)
            if total is not None:
                out["cross"]["total_triangles"] = int(total) - sum(c["total_triangles"] for c in out["groups"])
            out["cross"]["nodes_in_violating_triangles"] = 0
        if self.ks:
            out["ranks"] = _top_k_from_histograms(d["strict"], d["weak"], self.ks)
        return out


def sliding_window_score_details(ref, moving, commonCT=None, *, group_by=None, top_k=None, type_variants=None, param_sets=None,
                                 optim_params=None, gurobi_params=None, score_delaunay=None, score_delaunay_vertex_col=None,
                                 score_params=None, workers=None, triangulator=None, ctx=None, batch=None, moving_delaunay=None,
                                 moving_delaunay_vertex_col=None, unpack=None):
    """`sliding_window_scores` with every record broken down three ways, over the same one pass of the windows and still without a table:
    -> `ScoreDetails`
      scores     exactly `sliding_window_scores`' frame for the same arguments;
      confusion  indexed by (variant, set, moving_label), one int64 column per reference label: the rows whose moving cell carries the
                 one label and whose matched reference cell the other; labels in the order of the frames' joint codes;
      groups     one row per (variant, set, group): `group` and RECORD_KEYS over the group (`record_from_counts`); the triangle keys
                 count the triangles whose three corners lie in the group and are left out without a triangulation;
      cross      one row per (variant, set): the rows without a group, their type matches, and the triangles in no group -- its
                 `total_triangles` is the caller's total minus the groups', so triangles that name an id the frame lacks land here;
      top_k      one row per (variant, set): `typed_rows` and per k `top{k}_matches`, `top{k}_tied` (`top_k_counts`) and
                 `top{k}_accuracy` = 100 * matches / matched.
    `group_by`: a column of the moving frame (a MetaCell object's `metacell_df`) or an array of its length; missing values mean no
    group; groups in pd.factorize order; None: `groups` and `cross` are None.  `top_k`: a set of ints in 1..16, the ranks are read from
    the reference frame's commonCT columns; None: `top_k` is None.  The other keywords are `sliding_window_scores`' but for `tables`;
    a `group_by` that is neither, a `top_k` outside the range and what `sliding_window_scores` refuses raise ValueError before a job or
    a device is touched.
    Counted on the device from every result's merged rows (csrc/window_score_detail.hip: the detail call beside the score call).  What
    `scores.DeviceScores.prepare` refuses, and more labels or groups than the library's caps (64, 256), go through
    `score_table_details` on the tables: the same frames, nothing saved.
    `unpack` ("distribute" / "nearest"; `ref` and `moving` MetaCell objects, `checked_unpack`'s rules): -> `CellScoreDetails`, the five
    fields above -- `scores` with UNPACK_KEYS, as `sliding_window_scores(unpack=)` gives them -- and the same readings of the unpacked
    CELL pairs (examples/luad/reproduce_figures.ipynb cells 12, 13):
      cell_confusion  indexed by (variant, set, moving_label) over the cell-level labels (`joint_labels` of the two objects'
                      `original_df[cell_type_col]`), one int64 column per reference cell label;
      cell_groups     one row per (variant, set, group): `group` and UNPACK_KEYS over the pairs whose metacell row is in the group;
      cell_cross      one row per (variant, set): UNPACK_KEYS over the pairs of rows without a group;
      cell_top_k      one row per (variant, set): `typed_rows`, `top{k}_matches`, `top{k}_tied` over (the moving cell's label, the type
                      row `ref.original_df[commonCT]` of the reference cell it was put on) and `top{k}_accuracy` = 100 * matches /
                      cells_matched; with `top_k`, a commonCT column `ref.original_df` lacks raises ValueError first.
    The group and top-k frames are None without `group_by` / `top_k`.  On the device ONE call per result takes the unpack call's place
    and bins the pairs where they are made (csrc/window_unpack_detail.hip); objects `DeviceScores.device_members` refuses, more than 64
    cell labels and whatever keeps the job off the shared pass go through `score_unpacked_details` on every table: the same frames."""
    params = checked_score_params(score_params)
    ks = checked_top_k(top_k)
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    checked_unpack(unpack, ref_arg, moving_arg, no_objects=_NoMetaCellObjects)
    if unpack is not None and ks:
        cell_cts = _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT)
        lacking = [c for c in cell_cts if c not in ref_arg.original_df.columns]
        if lacking:
            raise ValueError(f"top_k with unpack={unpack!r} ranks the reference cells' type columns: ref.original_df has no {lacking}")
    group_codes, group_names = checked_groups(group_by, mov_df)
    group_values = mov_df[group_by].to_numpy() if isinstance(group_by, str) else group_by       # (the host route's frames may be copies)
    spec = DetailSpec(group_codes, group_names, ks)
    scores, nested, hook = _scored_study(ref, moving, commonCT, type_variants=type_variants, param_sets=param_sets, optim_params=optim_params,
                                         gurobi_params=gurobi_params, score_delaunay=score_delaunay,
                                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=params, tables=False,
                                         workers=workers, triangulator=triangulator, ctx=ctx, batch=batch, moving_delaunay=moving_delaunay,
                                         moving_delaunay_vertex_col=moving_delaunay_vertex_col, unpack=unpack, detail=spec)
    n_sets = len(nested[0])
    job = hook.job
    if hook.records is not None:
        labels = spec.labels
        per_table = [_frames_of_counts(spec.counts(rec, labels, hook.total), labels, group_names, ks, params) for rec in hook.records]
    else:                                               # not scored on the device: the host statement on every table
        tri, vertex_col = hook.triangulation(job)
        cts = _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT)
        per_table = [score_table_details(t, job.ref, job.moving, cell_id_col=job.optim_params["cell_id_col"], commonCT=cts,
                                         group_by=group_values, top_k=ks or None, score_delaunay=tri,
                                         score_delaunay_vertex_col=vertex_col, score_params=params, ctx=ctx)[1:]
                     for per_set in nested for t in per_set]
    if unpack is None:
        return ScoreDetails(scores, *_stacked(per_table, n_sets))
    if hook.records is not None:
        cells = [_cell_frames_of_counts(_cell_counts_of_words(rec["_cell_detail"], group_names, ks), hook.cell_dev.labels, group_names, ks)
                 for rec in hook.records]
    else:                                               # the host statement on every table
        cts = _common_types(ref_arg, moving_arg, ref_df, mov_df, commonCT)
        tables = [t for per_set in nested for t in per_set]             # (hook.cell_tables: `_scored_study` unpacked every table already)
        cells = [score_unpacked_details(t, ref_arg, moving_arg, unpack, commonCT=cts, group_by=group_values, top_k=ks or None, cells=c)
                 for t, c in zip(tables, hook.cell_tables)]
    return CellScoreDetails(scores, *_stacked(per_table, n_sets), *_stacked(cells, n_sets))
