"""The reference's window API on top of the pre-MIP path: sliding_window_matching (src/same.py:297-595) and what stands behind it.

Split from same_amd/api.py (run_same and prepare_same_inputs live there).  Two pipelines stand behind the same signature; which one
runs, and on what, is said at the head of the code below and in DESIGN.md section 0."""
import os
import threading
from typing import Any, Dict, Optional

import numpy as np
import pandas as pd

from . import ops
from ._trace import stage
from .api import PreparedInputs, _Staged, _run_same, _say, _stage_prune, prepare_same_inputs
from .params import init_gurobi_params, init_optim_params


# ------------------------------------------------------------------------------------------ windows
# The reference's window loop (src/same.py:507-593) cuts both frames per window with four comparisons over the WHOLE frame
# (subset_data, :293-295) and runs the whole pre-MIP path of run_same on the subsets.  Two pipelines stand behind the same
# signature here:
#   "device" (default)  both frames are uploaded ONCE as sections binned on the window grid (windows.DeviceSection); per window the
#                       rows of the box, the prune, the pair costs, the compaction, the triangle filter, weights and signs come from
#                       two library calls on the resident sections (csrc/window_stage.hip, csrc/window_finish.hip); the host only
#                       triangulates (Qhull helpers, windows ahead) and hands `PreparedInputs` -- whose frames are made from the
#                       section rows when somebody reads them -- to the unchanged run_same body.
#   "frames"            every window's frames are cut on the host and go through the host-buffer entry points (`_stage_prune`): the
#                       pipeline of rounds 1-4, kept as the fallback for inputs the sections cannot hold and as the comparison
#                       the tests and `bench.py --cfg5-pipeline frames` run.
# SAME_WINDOW_PIPELINE=frames forces the second one.
def window_pipeline(requested=None):
    v = (requested or os.environ.get("SAME_WINDOW_PIPELINE", "device")).lower()
    if v not in ("device", "frames"):
        raise ValueError(f"window pipeline must be 'device' or 'frames', got {v!r}")
    return v


def subset_data(df, x_min, x_max, y_min, y_max):
    """src/same.py:293-295."""
    return df[(df["X"] >= x_min) & (df["X"] < x_max) & (df["Y"] >= y_min) & (df["Y"] < y_max)]


class _WindowSubsetter:
    """subset_data for many boxes of one frame.  The reference evaluates four comparisons over the WHOLE frame for every
    window (O(N * windows), src/same.py:521-526); here the rows are binned once into a uniform grid (windows.GridRows), a
    window gathers the cells its box touches and only those rows are tested exactly.  The rows come back in frame order with
    their original labels, i.e. the frame `subset_data` returns (NaN / infinite coordinates fall outside every box either way)."""

    def __init__(self, df):
        from .windows import GridRows

        self.df = df
        self.grid = GridRows(df["X"].to_numpy(dtype=np.float64), df["Y"].to_numpy(dtype=np.float64))

    def subset(self, x_min, x_max, y_min, y_max):
        return self.df.iloc[self.grid.rows(x_min, x_max, y_min, y_max)]


def _window_frame(df, rows, vertex_col=None, aligned=False):
    """Rows `rows` of the caller's frame as the frame run_same holds after its prune: the helper columns of src/same.py:934-970
    (size default, __orig_idx = the caller's index labels, __tri_vid on the aligned side) and the renumbering of src/utils.py:739-740."""
    # iloc with a row list makes fresh data; the shallow copy only drops pandas' "copy of a slice" mark
    out = df.iloc[rows].copy(deep=False)
    labels = out.index.to_numpy()
    out.index = pd.RangeIndex(len(out))           # the renumbering, in place: reset_index(drop=True) would copy every block once more
    if "size" not in out.columns:
        out["size"] = 1
    if "__orig_idx" not in out.columns:
        out["__orig_idx"] = labels
    if aligned:
        if vertex_col is None:
            out["__tri_vid"] = labels
        else:
            if vertex_col not in out.columns:
                raise ValueError(f"aligned_delaunay_vertex_col='{vertex_col}' not in aligned_df")
            out["__tri_vid"] = out[vertex_col].to_numpy()
    return out


def frame_id_codes(moving, ref, cid):
    """((aligned code per moving row, reference code per ref row), whether every id names one row, (sorted distinct moving ids, sorted
    distinct ref ids)): the cell ids of both frames as int64 ranks in the ORDER of the ids (equal id <=> equal code) -- what the window
    merge compares, orders by and exchanges between ranks instead of the ids themselves (strings, floats ...)."""
    def codes(df):
        ids = df[cid].to_numpy()
        if ids.dtype.kind in "iu" and (len(ids) < 2 or bool(np.all(ids[1:] > ids[:-1]))):
            return np.arange(len(ids), dtype=np.int64), True, ids                 # ascending ids: a row's code is its number
        c, uniq = pd.factorize(ids, sort=True, use_na_sentinel=False)
        return c.astype(np.int64), len(uniq) == len(ids), np.asarray(uniq)

    (mc, mu, m_ids), (rc, ru, r_ids) = codes(moving), codes(ref)
    return (mc, rc), mu and ru, (m_ids, r_ids)


def codes_of_ids(sorted_distinct_ids, ids):
    """the codes `frame_id_codes` gave these ids"""
    return pd.Index(sorted_distinct_ids).get_indexer(np.asarray(ids)).astype(np.int64)


def caller_triangulation_rows(moving, moving_delaunay, vertex_col=None):
    """A caller's triangulation of `moving` for the device route, once per job: -> (int32 (Tr, 3) ROWS of the frame, None), or (None,
    why it stays on the general route).  The triangulation is normalised as `triangles._as_triangle_array` does; a vertex id is
    `vertex_col`'s value of a row, or the row's index label (src/same.py:425-435: `__tri_vid`); triangles that name an id the frame does
    not have are dropped (no window could keep them, src/same.py:262-290); the caller's order of triangles and of corners stays.
    Refused: ids that are not unique in the frame (the reference's per-window dict keeps the last row of the WINDOW); two triangles with
    the same vertex set (the device's re-add de-duplicates by triangle, the reference by vertex tuple); ids that are not integers."""
    from .triangles import _as_triangle_array

    def integral(a):
        a = np.asarray(a)
        if a.dtype.kind in "iu":
            return a.astype(np.int64)
        if a.dtype.kind == "f" and a.size == np.count_nonzero(np.isfinite(a) & (a == np.floor(a))) and (a.size == 0 or np.abs(a).max() < 2.0**62):
            return a.astype(np.int64)
        return None

    if vertex_col is not None and vertex_col not in moving.columns:
        return None, "aligned_delaunay_vertex_col missing"
    frame = isinstance(moving_delaunay, pd.DataFrame)
    raw = np.asarray(moving_delaunay.iloc[:, :3] if frame else moving_delaunay)
    if raw.size and integral(raw) is None:
        return None, "the triangulation's vertex ids are not integers"
    tri = _as_triangle_array(moving_delaunay).astype(np.int64, copy=False).reshape(-1, 3)
    ids = integral(moving.index.to_numpy() if vertex_col is None else moving[vertex_col].to_numpy())
    if ids is None:
        return None, "the frame's vertex ids are not integers"
    n = len(ids)
    order = np.argsort(ids, kind="stable")
    by_id = ids[order]
    if n > 1 and bool(np.any(by_id[1:] == by_id[:-1])):
        return None, "the frame's vertex ids are not unique"
    rows = np.zeros((0, 3), np.int64)
    if len(tri) and n:
        at = np.minimum(np.searchsorted(by_id, tri), n - 1)
        known = by_id[at] == tri
        rows = order[at][known.all(axis=1)].reshape(-1, 3)
    if len(rows) > 1 and len(np.unique(np.sort(rows, axis=1), axis=0)) != len(rows):
        return None, "two triangles have the same vertex set"
    if len(rows) and (rows.min() < 0 or rows.max() >= n):                # (by construction; nothing is uploaded that was not looked at)
        return None, "a vertex row outside the frame"
    return np.ascontiguousarray(rows, dtype=np.int32), None


def member_layout(mc):
    """The member lists of a MetaCell object as the device reads them: -> (int64 CSR offsets over the rows of `mc.metacell_df`, the
    members' ids in CSR order, their rows in `mc.original_df`, None), or (None, None, None, why the lists stay on the host): ids that
    are not integers, ids `mc.original_df[mc.original_idx_col]` repeats, a member id it does not have."""
    lists = mc.metacell_df["members"].tolist()
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(m) for m in lists], out=off[1:])
    ids = np.asarray([x for m in lists for x in m]) if off[-1] else np.zeros(0, np.int64)
    if ids.dtype.kind not in "iu" or ids.ndim != 1:
        return None, None, None, "member ids are not integers"
    index = pd.Index(mc.original_df[mc.original_idx_col].to_numpy())
    if not index.is_unique:
        return None, None, None, "the original frame repeats a cell id"
    rows = index.get_indexer(ids)
    if len(rows) and rows.min() < 0:
        return None, None, None, "a member id the original frame does not have"
    return off, ids.astype(np.int64), rows.astype(np.int64), None


def caller_triangulation_refusal(ref, moving, commonCT, op, moving_delaunay, vertex_col=None):
    """Why a caller's triangulation does not take the device route of sliding_window_incumbent under
    optim_params["hip_caller_delaunay"] = "device" (None: it does): a reason `_DeviceFrames.refusal` names, ignore_knn_if_matched
    without optim_params["hip_priority_prune"] = "device" (the priority filter then runs on the host, window by window), or one of
    `caller_triangulation_rows`."""
    from .window_mode import priority_prune_route

    why = _DeviceFrames.refusal(ref, moving, commonCT, op, vertex_col)
    if why is None and op["ignore_knn_if_matched"] and priority_prune_route(op) != "device":
        why = "ignore_knn_if_matched"
    return why if why is not None else caller_triangulation_rows(moving, moving_delaunay, vertex_col)[1]


class _DeviceFrames:
    """The two frames of a window loop as sections resident on the device (windows.DeviceSection), binned on the grid on which every
    window box is a union of cells (windows.window_cell_grid).  `windows(plan)` runs the per-window device path over them."""

    def __init__(self, ref, moving, commonCT, optim_params, cell_grid=None, ctx=None):
        from .windows import DeviceSection, Section

        self.ref, self.moving, self.commonCT, self.op = ref, moving, list(commonCT), optim_params
        self.cost_dtype = np.dtype(optim_params.get("hip_cost_dtype", "float64"))
        self.ctx = ops._ctx(ctx)
        self.ref_sec, self.mov_sec = Section.from_frame(ref, self.commonCT), Section.from_frame(moving, self.commonCT)
        self.dref = self.dmov = None
        self._worker_ctx = []            # contexts (= streams) of the worker threads beyond the first, kept with their window states
        self._label_lock = threading.Lock()
        with stage("sections to the device + binning on the window grid"):
            self.dref = DeviceSection(self.ref_sec, self.cost_dtype, self.ctx)
            self.dmov = DeviceSection(self.mov_sec, self.cost_dtype, self.ctx)
            if cell_grid is not None:
                from ._lib import SAME_EINVAL, SameHipError
                for sec in (self.dref, self.dmov):
                    try:
                        sec.bin(*cell_grid)
                    except SameHipError as e:
                        # the one thing that may be passed over is the REFUSAL of a window grid too fine for the section's extent (> 2^22
                        # cells, SAME_EINVAL): that section keeps the grid of its own and boxes that cut through its cells are tested row
                        # by row -- the same rows either way.  A failed sort or allocation inside the binning is an error of this call.
                        if e.code != SAME_EINVAL:
                            raise

    @staticmethod
    def refusal(ref, moving, commonCT, op, vertex_col=None):
        """Why these inputs go through the frame pipeline instead (None: the sections can hold them).  Everything listed makes the
        reference itself raise inside run_same; the frame pipeline raises the same error at the same window."""
        if np.dtype(op.get("hip_cost_dtype", "float64")) not in (np.dtype(np.float64), np.dtype(np.float32)):
            return "hip_cost_dtype"
        for df in (ref, moving):
            if any(c not in df.columns for c in list(commonCT) + ["X", "Y"]):
                return "a commonCT / coordinate column is missing"
            if any(df[c].dtype.kind not in "fiub" for c in list(commonCT) + ["X", "Y"]):
                return "a commonCT / coordinate column is not numeric"
            if "size" in df.columns and df["size"].dtype.kind not in "fiub":
                return "size is not numeric"
        if vertex_col is not None and vertex_col not in moving.columns:
            return "aligned_delaunay_vertex_col missing"
        if op["ignore_same_type_triangles"] and "cell_type" not in moving.columns:
            return "cell_type missing (same-type triangle rule)"
        if op["ignore_knn_if_matched"] and ("cell_type" not in moving.columns or "cell_type" not in ref.columns):
            return "cell_type missing (priority filter)"
        return None

    def caller_tris(self, moving_delaunay, vertex_col):
        """The caller's triangulation of the moving frame resident beside its section (windows.DeviceCallerTris), or None where
        `caller_triangulation_rows` refuses it.  Made once per triangulation object and id column, kept until close(): an object of its
        own, so what the sections mean to a job without a triangulation does not change; the worker contexts share it like a section."""
        from .windows import DeviceCallerTris

        known = self.__dict__.setdefault("_caller_tris", {})
        key = (id(moving_delaunay), vertex_col)
        if key not in known:
            rows, _why = caller_triangulation_rows(self.moving, moving_delaunay, vertex_col)
            # (the caller's object is held with the entry: its id names it for as long as the entry lives)
            known[key] = (moving_delaunay, None if rows is None else DeviceCallerTris(self.dmov, rows, self.ctx))
        return known[key][1]

    def members(self, mc, side, other):
        """The members of MetaCell object `mc`'s rows resident beside its section (windows.DeviceMembers) -- `side` "moving" or "ref",
        `other` the object of the other side: the CSR of `mc.metacell_df["members"]`, per member its cell's XY in `mc.original_df`
        (float64) and its code among the joint codes of the two objects' original `cell_type_col` labels (eval_utils._label_codes).
        None where `member_layout` refuses the lists.  Made once per pair of objects and kept until close() -- the objects are held with
        the entry, as `caller_tris` holds its triangulation; `.ids` is the members' ids in CSR order."""
        from .eval_utils import _label_codes
        from .windows import DeviceMembers

        known = self.__dict__.setdefault("_members", {})
        key = (id(mc), id(other), side)
        if key not in known:
            off, ids, rows, _why = member_layout(mc)
            made = None
            if off is not None and len(off) == len(self.moving if side == "moving" else self.ref) + 1:
                mov_mc, ref_mc = (mc, other) if side == "moving" else (other, mc)
                codes = _label_codes(mov_mc.original_df[mov_mc.cell_type_col].to_numpy(), ref_mc.original_df[ref_mc.cell_type_col].to_numpy())
                xy = mc.original_df[[mc.x_col, mc.y_col]].to_numpy(dtype=np.float64)
                with stage("member lists to the device"):
                    made = DeviceMembers(self.dmov if side == "moving" else self.dref, off, xy[rows], codes[0 if side == "moving" else 1][rows])
                made.ids, made.rows = ids, rows
            known[key] = ((mc, other), made)
        return known[key][1]

    def unpack_detail(self, ref_mc, mov_mc, commonCT, ks):
        """What a study's cell pairs are binned by, resident beside the reference members (windows.DeviceUnpackDetail): the cell-level
        labels -- `score_details.joint_labels` of the two objects' `original_df[cell_type_col]`, the codes `members` uploads --, with
        `ks` their columns among `commonCT` (`label_columns`) and one type row per reference member, `ref_mc.original_df[commonCT]` as
        float64 at `member_layout`'s rows.  `.labels`: the labels in their codes' order.  None for more than SAME_SCORE_MAX_LABELS cell
        labels, and where `members` refuses the lists.  Made once per pair of objects and kept until close(), like `members`."""
        from ._lib import SAME_SCORE_MAX_LABELS
        from .score_details import joint_labels, label_columns
        from .windows import DeviceUnpackDetail

        known = self.__dict__.setdefault("_unpack_details", {})
        key = (id(ref_mc), id(mov_mc), tuple(commonCT), bool(ks))
        if key not in known:
            made, ref_members = None, self.members(ref_mc, "ref", mov_mc)
            _cm, _cr, labels = joint_labels(mov_mc.original_df[mov_mc.cell_type_col].to_numpy(),
                                            ref_mc.original_df[ref_mc.cell_type_col].to_numpy())
            if ref_members is not None and len(labels) <= SAME_SCORE_MAX_LABELS:
                cols = types = None
                if ks:
                    cols = label_columns(labels, commonCT)
                    types = ref_mc.original_df[list(commonCT)].to_numpy(dtype=np.float64)[ref_members.rows]
                with stage("cell labels' columns and member type rows to the device"):
                    made = DeviceUnpackDetail(ref_members, len(labels), cols, types)
                made.labels = labels
            known[key] = ((ref_mc, mov_mc), made)
        return known[key][1]

    def score_detail(self, group_of, n_groups, n_labels, col_of_label):
        """What a study's scores are broken down by, resident beside the moving section (windows.DeviceScoreDetail): `group_of` the
        moving rows' group codes (None: one group), `col_of_label` the joint label codes' type columns (None: no rank counts).  Made
        once per (group codes, column map) -- keyed by their values -- and kept until close(), as `caller_tris` and `members` are."""
        from .windows import DeviceScoreDetail

        g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.int32)
        c = None if col_of_label is None else np.ascontiguousarray(col_of_label, dtype=np.int32)
        known = self.__dict__.setdefault("_score_details", {})
        key = (None if g is None else g.tobytes(), int(n_groups), int(n_labels), None if c is None else c.tobytes())
        if key not in known:
            with stage("score groups and label columns to the device"):
                known[key] = DeviceScoreDetail(self.dmov, g, n_groups, n_labels, c)
        return known[key]

    def score_map(self, truth_row, tally):
        """A study's per-cell map resident beside the sections (windows.DeviceScoreMap): `truth_row` the moving rows' true reference
        rows (None: none known), `tally` whether results are folded into per-cell counters.  One per call -- its tally is a study's
        own --, kept until close() or until the study closes it."""
        from .windows import DeviceScoreMap

        with stage("truth rows and the per-cell tally to the device"):
            made = DeviceScoreMap(self.dmov, self.dref, truth_row, tally, self.ctx)
        self.__dict__.setdefault("_score_maps", []).append(made)
        return made

    def unpack_map(self, mov_members, ref_members, truth_member, tally):
        """`score_map` at cell level: a study's per-CELL map resident beside the two member lists (windows.DeviceUnpackMap):
        `truth_member` the moving members' true reference members, flat into `ref_members`' CSR (None: none known), `tally` whether
        results are folded into per-member counters.  One per call -- its tally is a study's own --, kept until close() or until the
        study closes it."""
        from .windows import DeviceUnpackMap

        with stage("truth members and the per-member tally to the device"):
            made = DeviceUnpackMap(mov_members, ref_members, truth_member, tally)
        self.__dict__.setdefault("_unpack_maps", []).append(made)
        return made

    def score_features(self, mov_q, ref_q, group_of, n_groups, zone=None):
        """A study's fixed-point feature columns resident beside the sections (windows.DeviceScoreFeatures) and, with `zone` =
        (moving flags, reference flags, squared-distance edges), its distance reading (windows.DeviceFeatureZone; else None).  One pair
        per call -- the matrices are a study's own --, kept until close() or until the study closes them.  -> (features, zone)"""
        from .windows import DeviceFeatureZone, DeviceScoreFeatures

        held = self.__dict__.setdefault("_score_features", [])
        with stage("feature columns, groups and zone masks to the device"):
            feats = DeviceScoreFeatures(self.dmov, self.dref, mov_q, ref_q, group_of, n_groups)
            held.append(feats)
            made = None
            if zone is not None:
                made = DeviceFeatureZone(feats, *zone)
                held.append(made)
        return feats, made

    def unpack_features(self, mov_members, ref_members, mov_q, ref_q, member_group, n_groups, zone=None):
        """`score_features` at cell level: one fixed-point row per MEMBER in CSR order and the moving cells' groups resident beside the
        two member lists (windows.DeviceUnpackFeatures) and, with `zone` = (moving member flags, reference member flags,
        squared-distance edges), the distance reading (windows.DeviceUnpackZone; else None).  One pair per call, kept until close() or
        until the study closes them.  -> (features, zone)"""
        from .windows import DeviceUnpackFeatures, DeviceUnpackZone

        held = self.__dict__.setdefault("_unpack_features", [])
        with stage("member feature columns, groups and zone masks to the device"):
            feats = DeviceUnpackFeatures(mov_members, ref_members, mov_q, ref_q, member_group, n_groups)
            held.append(feats)
            made = None
            if zone is not None:
                made = DeviceUnpackZone(feats, *zone)
                held.append(made)
        return feats, made

    def types_layer(self, variant, types):
        """A type-matrix variant of the moving frame resident beside its section (windows.DeviceTypesLayer): `types` the variant as a
        float64 (rows, commonCT) matrix, `variant` the caller's object it was read from.  Uploaded once per object and kept until close()
        -- with a `resident_frames` object for that object's life; the worker contexts share it like a section."""
        from .windows import DeviceTypesLayer

        known = self.__dict__.setdefault("_types_layers", {})
        if id(variant) not in known:
            # (the caller's object is held with the entry: its id names it for as long as the entry lives)
            with stage("a type-matrix variant of the moving frame to the device"):
                known[id(variant)] = (variant, DeviceTypesLayer(self.dmov, types, self.ctx))
        return known[id(variant)][1]

    def label_codes_on_device(self):
        """The joint codes of the two frames' `cell_type` labels (eval_utils._label_codes: equal code <=> labels that compare equal; a
        label that equals nothing is negative) in the sections' slot for them: what the cell-type-priority prune on the device compares
        (windows.priority_windows).  Made and uploaded once per frames: the library wants the codes set before the first prune over a
        section and frees the old ones when they are set again, so the device route calls this before its worker threads start."""
        with self._label_lock:        # worker threads may all ask (`windows`): one uploads, before any of them prunes
            if not self.__dict__.get("_label_codes_on_device"):
                from .eval_utils import _label_codes

                with stage("cell-type label codes to the device"):
                    mov_code, ref_code = _label_codes(self.moving["cell_type"].to_numpy(), self.ref["cell_type"].to_numpy())
                    self.dmov.set_label_codes(mov_code)
                    self.dref.set_label_codes(ref_code)
                self.__dict__["_label_codes_on_device"] = True

    def windows(self, plan, triangulate=True, ctx=None, triangulator=None, fetch_triangles=False, collector=None, batch=None, mode=None,
                caller=None, priority=False, sets=None, variants=None):
        from .windows import iter_device_windows

        op = self.op
        if priority:
            self.label_codes_on_device()
        return iter_device_windows(self.ref_sec, self.mov_sec, self.dref, self.dmov, plan, radius=op["radius"], knn=op["knn"],
                                   dist_ct_coeff=op["dist_ct_coeff"], min_angle_deg=op.get("min_angle_deg", 15),
                                   ignore_same_type_triangles=op["ignore_same_type_triangles"], no_match_penalty=op["no_match_penalty"],
                                   ctx=self.ctx if ctx is None else ctx, triangulate=triangulate, triangulator=triangulator,
                                   fetch_triangles=fetch_triangles, collector=collector, batch=batch, mode=mode, caller=caller,
                                   priority=priority, sets=sets, variants=variants)

    def accumulators(self, contexts, cid):
        """One merge accumulator per worker context (kept with the frames: a pass re-uses the arrays of the last), and the sections' id
        codes for `cid` on the device.  -> ([accumulator per context], whether every id names one row)."""
        from .windows import MergeAccumulator

        accs = self.__dict__.setdefault("_accs", {})
        for c in contexts:
            if id(c) not in accs:
                accs[id(c)] = MergeAccumulator(c)
        (mov_code, ref_code), unique = self.id_codes(cid)
        if self.__dict__.get("_codes_on_device") != cid:
            identity = lambda code: len(code) == 0 or (code[0] == 0 and code[-1] == len(code) - 1 and bool(np.all(code[1:] > code[:-1])))
            for sec, code in ((self.dmov, mov_code), (self.dref, ref_code)):
                sec.set_codes(None if identity(code) else code, int(code.max()) + 1 if len(code) else 0)
            self.__dict__["_codes_on_device"] = cid
        return [accs[id(c)] for c in contexts], unique

    def box_rows(self, box, state):
        """(aligned rows, reference rows) of the frames inside the box -- subset_data of both frames, as row positions."""
        from .windows import _W_ROWS_M, _W_ROWS_R

        state.stage(self.dmov, self.dref, box, 1.0, 1, 1.0)
        return state.fetch(_W_ROWS_M), state.fetch(_W_ROWS_R)

    def id_codes(self, cid):
        """((aligned code per moving row, reference code per ref row), whether every id names one row) -- `frame_id_codes`, made once per
        frames and id column."""
        known = self.__dict__.setdefault("_id_codes", {})
        if cid not in known:
            known[cid] = frame_id_codes(self.moving, self.ref, cid)
        return known[cid][:2]

    def id_uniques(self, cid):
        """the sorted distinct ids of (moving, ref): code -> id"""
        self.id_codes(cid)
        return self._id_codes[cid][2]

    def table_columns(self, cid):
        """The frames' columns that are 8-byte numbers and go into the result table besides the sections' own (sizes, cell ids), resident on
        the device for the device-side gather of the merged table (MergeAccumulator.columns): -> {"mov": [(table column, DeviceBuffer,
        dtype)], "ref": [...]}; columns of other types are gathered by the host.  Uploaded once per frames and id column."""
        known = self.__dict__.setdefault("_table_columns", {})
        if cid not in known:
            def eligible(df, names):
                out = []
                for column, name in names:
                    dt = df[column].dtype if column in df.columns else None
                    if isinstance(dt, np.dtype) and dt.kind in "iuf" and dt.itemsize == 8:
                        host = np.ascontiguousarray(df[column].to_numpy())
                        out.append((name, self.ctx.to_device(host.view(np.uint64)), host.dtype))
                return out
            known[cid] = {"mov": eligible(self.moving, (("size", "size"), (cid, f"Aligned_{cid}"))),
                          "ref": eligible(self.ref, (("size", "ref_size"), (cid, f"Ref_{cid}")))}
        return known[cid]

    def worker_contexts(self, n):
        """n contexts on the sections' device for n worker threads: this object's own first, then extra ones that live (with the window
        states they have grown) until close()."""
        from . import _lib

        while len(self._worker_ctx) < n - 1:
            self._worker_ctx.append(_lib.Context(self.ctx.device))
        return [self.ctx] + self._worker_ctx[:n - 1]

    def close(self):
        for acc in self.__dict__.pop("_accs", {}).values():
            acc.close()
        for held in self.__dict__.pop("_table_columns", {}).values():
            for _name, buf, _dt in held["mov"] + held["ref"]:
                buf.free()
        for _held, tris in self.__dict__.pop("_caller_tris", {}).values():      # before the section they are binned by
            if tris is not None:
                tris.close()
        for _held, layer in self.__dict__.pop("_types_layers", {}).values():   # before the section they belong to
            layer.close()
        for _held, detail in self.__dict__.pop("_unpack_details", {}).values():   # before the members whose type rows they hold
            if detail is not None:
                detail.close()
        for made in self.__dict__.pop("_unpack_maps", []):                     # before the members they were made for
            made.close()
        for made in reversed(self.__dict__.pop("_unpack_features", [])):       # a zone before its features, both before their members
            made.close()
        for _held, members in self.__dict__.pop("_members", {}).values():      # before the section whose rows they list
            if members is not None:
                members.close()
        for made in self.__dict__.pop("_score_maps", []):                      # before the sections they were made for
            made.close()
        for made in reversed(self.__dict__.pop("_score_features", [])):        # a zone before its features, both before the sections
            made.close()
        for detail in self.__dict__.pop("_score_details", {}).values():        # before the section whose rows they group
            detail.close()
        for c in self._worker_ctx:
            c.close()
        self._worker_ctx = []
        for sec in (self.dref, self.dmov):
            if sec is not None:
                sec.close()
        self.dref = self.dmov = None


def _window_error(dw, optim_params):
    """What the reference raises for a window whose prune finds no pair: run_same's ValueError (src/same.py:1003) -- unless the
    cell-type-priority prune is on, whose summary print divides by the number of rows that kept a pair first (src/knn_utils.py:76)."""
    no_pairs = isinstance(dw.error, ValueError) and str(dw.error).startswith("No valid_pairs after KNN filtering")
    if optim_params["ignore_knn_if_matched"] and no_pairs:
        return ZeroDivisionError("division by zero")
    return dw.error


def _device_pairs(dw):
    """The window's pair list with the reference side compacted the way src/utils.py:734-742 compacts it (np.unique of the used
    reference rows): -> (valid_pairs (P, 2) int64, section rows of the compacted reference cells).  The device keeps reference cells
    under their rows in the box (nothing on the device needs the renumbering)."""
    from .windows import _W_PAIRS, _W_ROWS_R

    pairs, rows_r_box = dw.state.fetch(_W_PAIRS), dw.state.fetch(_W_ROWS_R)
    used = np.zeros(len(rows_r_box), bool)
    used[pairs[:, 1]] = True
    valid_pairs = np.empty((len(pairs), 2), np.int64)
    valid_pairs[:, 0] = pairs[:, 0]
    valid_pairs[:, 1] = (np.cumsum(used) - 1)[pairs[:, 1]]
    return valid_pairs, rows_r_box[used]


def _prepared_from_device(dw, frames, optim_params, gurobi_params, verbose=True, vertex_col=None):
    """PreparedInputs of one window from what the device path left (windows.DeviceWindowResult after filter_finish): pairs, costs, kept
    triangles, weights and signs are fetched as arrays; the two frames are rows of the caller's frames, made when first read."""
    from .windows import _W_COSTS, _W_SIGNS, _W_TRIANGLES, _W_WEIGHTS

    st = dw.state
    valid_pairs, rows_r = _device_pairs(dw)
    rows_m = dw.rows_m
    _say(verbose, f"Number of valid pairs after knn: {len(valid_pairs)}")
    costs = st.fetch(_W_COSTS)
    if optim_params["ignore_knn_if_matched"]:
        # the cell-type-priority filter (src/knn_utils.py:28-65) is a sequential walk over the rows: host, on the fetched lists; the
        # frames are not compacted again (:66-78) and every kept pair keeps the cost the device computed for it
        from .knn import priority_filter

        n_r = max(len(rows_r), 1)
        kept, same_type, keep_all = priority_filter(valid_pairs, dw.axy, frames.ref_sec.xy[rows_r],
                                                    frames.moving["cell_type"].to_numpy()[rows_m],
                                                    frames.ref["cell_type"].to_numpy()[rows_r])
        key = valid_pairs[:, 0] * n_r + valid_pairs[:, 1]
        order = np.argsort(key, kind="stable")
        costs = costs[order[np.searchsorted(key[order], kept[:, 0] * n_r + kept[:, 1])]]
        valid_pairs = list(zip(kept[:, 0].tolist(), kept[:, 1].tolist()))
        _say(verbose, f"Total pairs after filtering: {len(valid_pairs)}")
        _say(verbose, f"Average pairs per matched point: {len(valid_pairs) / (same_type + keep_all):.2f}")
    tris = dw.triangles if dw.triangles is not None else st.fetch(_W_TRIANGLES)
    signs = st.fetch(_W_SIGNS).astype(np.float64)
    weights = st.fetch(_W_WEIGHTS)
    if np.issubdtype(frames.mov_sec.size.dtype, np.integer):
        # integer size columns sum to integers in the reference (triangles.triangle_weights_and_signs)
        weights = weights.astype(np.int64)
    prep = PreparedInputs(lambda: _window_frame(frames.moving, rows_m, vertex_col, aligned=True), lambda: _window_frame(frames.ref, rows_r),
                          valid_pairs, costs, tris, weights, signs, set(), False, optim_params, gurobi_params,
                          n_aligned=len(rows_m), n_ref=len(rows_r))
    prep.device, prep.rows_m, prep.rows_r, prep.sources = dw, rows_m, rows_r, (frames.moving, frames.ref)
    return prep


def _staged_from_device(dw, frames, commonCT, optim_params, gurobi_params, caller_triangles, vertex_col, verbose=True):
    """A window whose triangulation is the caller's: rows, prune and compaction from the device, then the frames are made at once
    (the vertex-id remap, the filter with unconstrained-node removal and the re-indexing of src/same.py:1016-1085 read them) and the
    second half runs as `prepare_same_inputs` runs it."""
    st = _Staged()
    st.verbose, st.commonCT = verbose, commonCT
    st.optim_params, st.gurobi_params = optim_params, gurobi_params
    try:
        valid_pairs, rows_r = _device_pairs(dw)
        _say(verbose, f"Number of valid pairs after knn: {len(valid_pairs)}")
        st.aligned_df = _window_frame(frames.moving, dw.rows_m, vertex_col, aligned=True)
        st.ref_df = _window_frame(frames.ref, rows_r)
        if optim_params["ignore_knn_if_matched"]:
            from .knn import priority_filter

            kept, same_type, keep_all = priority_filter(valid_pairs, dw.axy, frames.ref_sec.xy[rows_r],
                                                        st.aligned_df["cell_type"].to_numpy(),
                                                        st.ref_df["cell_type"].to_numpy())
            valid_pairs = list(zip(kept[:, 0].tolist(), kept[:, 1].tolist()))
            _say(verbose, f"Total pairs after filtering: {len(valid_pairs)}")
            _say(verbose, f"Average pairs per matched point: {len(valid_pairs) / (same_type + keep_all):.2f}")
        st.valid_pairs = valid_pairs
        st.caller_triangles = caller_triangles
    except Exception as e:   # noqa: BLE001 -- raised where the serial flow would have raised it (prepare_same_inputs)
        st.error = e
    return st


class ResidentFrames:
    """`resident_frames(ref, moving, ...)`: the two frames of a window job uploaded and binned ONCE, for callers that run several jobs over
    the same frames (a parameter search, bench.py's steps).  Pass it in place of `ref` (or with the same ref / moving objects) to
    sliding_window_matching / sliding_window_incumbent; `close()` (or the context manager) frees the device memory.  It remembers what
    depends on the frames alone -- their cell-type sets, the window plans per (window_size, overlap, min_cells) -- and holds one pair of
    device sections per (commonCT, cost dtype, window grid)."""

    def __init__(self, ref, moving, ctx=None):
        self.ref_arg, self.moving_arg, self.ctx = ref, moving, ctx
        self.type_sets, self.plans, self._frames = {}, {}, {}

    def frames_for(self, job):
        from .windows import window_cell_grid

        why = _DeviceFrames.refusal(job.ref, job.moving, job.commonCT, job.optim_params, job.vertex_col)
        if why is not None:
            raise ValueError(f"these frames cannot be held as device sections: {why}")
        cell_grid = window_cell_grid(job.grid, job.window_size, job.overlap)
        key = (tuple(job.commonCT), str(np.dtype(job.optim_params.get("hip_cost_dtype", "float64"))), cell_grid)
        if key not in self._frames:
            self._frames[key] = _DeviceFrames(job.ref, job.moving, job.commonCT, job.optim_params, cell_grid, ctx=self.ctx)
        frames = self._frames[key]
        frames.op = job.optim_params          # radius, k, penalties ... are per job; the sections do not depend on them
        return frames

    def close(self):
        for f in self._frames.values():
            f.close()
        self._frames = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def resident_frames(ref, moving, ctx=None):
    """See ResidentFrames."""
    return ResidentFrames(ref, moving, ctx=ctx)


class _WindowJob:
    """What sliding_window_matching settles before its loop (src/same.py:297-505): MetaCell unwrapping, parameters, the cell-type check,
    commonCT, the plan, the resume state and this rank's share of the windows."""

    def __init__(self, ref, moving, commonCT, outprefix, moving_delaunay, moving_delaunay_vertex_col, optim_params, gurobi_params,
                 ignore_precomputed_triangulation, shard, resident=None, mode=None):
        from .windows import window_grid, window_plan

        self.mode = mode                # how sliding_window_incumbent matches the job's windows (a WindowMode)

        # the caller's frames are on the device already (resident_frames): both arguments may name it
        if isinstance(ref, ResidentFrames):
            resident = ref
        if isinstance(moving, ResidentFrames):
            resident = moving
        if resident is not None:
            ref = resident.ref_arg if isinstance(ref, ResidentFrames) else ref
            moving = resident.moving_arg if isinstance(moving, ResidentFrames) else moving
            if ref is not resident.ref_arg or moving is not resident.moving_arg:
                raise ValueError("resident frames were made from other ref / moving objects than the ones passed")
        self.resident = resident

        ref_cell_type_col = moving_cell_type_col = "cell_type"
        optim_params = dict(optim_params or {})
        gurobi_params = dict(gurobi_params or {})
        if hasattr(ref, "metacell_df"):
            mc_ref = ref
            ref = mc_ref.metacell_df
            ref_cell_type_col = getattr(mc_ref, "cell_type_col", ref_cell_type_col)
            if (optim_params.get("cell_id_col") is None) and hasattr(mc_ref, "metacell_idx_col"):
                optim_params["cell_id_col"] = mc_ref.metacell_idx_col
        if hasattr(moving, "metacell_df") and hasattr(moving, "metacell_delaunay"):
            mc = moving
            moving = mc.metacell_df
            if moving_delaunay is None and not ignore_precomputed_triangulation:
                moving_delaunay = mc.metacell_delaunay
            if moving_delaunay_vertex_col is None and hasattr(mc, "metacell_idx_col"):
                moving_delaunay_vertex_col = mc.metacell_idx_col
            moving_cell_type_col = getattr(mc, "cell_type_col", moving_cell_type_col)
            if (optim_params.get("cell_id_col") is None) and hasattr(mc, "metacell_idx_col"):
                optim_params["cell_id_col"] = mc.metacell_idx_col
        self.optim_params = optim_params = init_optim_params(**(optim_params or {}))
        self.gurobi_params = gurobi_params = init_gurobi_params(**(gurobi_params or {}))
        self.window_size, self.overlap = optim_params["window_size"], optim_params["overlap"]
        min_cells = optim_params["min_cells_per_window"]

        ref_types = mov_types = None
        if ref_cell_type_col in ref.columns and moving_cell_type_col in moving.columns:
            if resident is not None and resident.type_sets.get((ref_cell_type_col, moving_cell_type_col)) is not None:
                ref_types, mov_types = resident.type_sets[(ref_cell_type_col, moving_cell_type_col)]
            else:
                ref_types = set(pd.Series(ref[ref_cell_type_col]).dropna().unique().tolist())
                mov_types = set(pd.Series(moving[moving_cell_type_col]).dropna().unique().tolist())
                if resident is not None:
                    resident.type_sets[(ref_cell_type_col, moving_cell_type_col)] = (ref_types, mov_types)
            if ref_types != mov_types:
                raise ValueError(
                    "Cell type categories differ between ref and moving.\n"
                    f"ref ({ref_cell_type_col}) has {len(ref_types)} types, moving ({moving_cell_type_col}) has {len(mov_types)} types.\n"
                    f"Only-in-ref: {sorted(ref_types - mov_types)[:20]}\nOnly-in-moving: {sorted(mov_types - ref_types)[:20]}")
        if commonCT is None:
            if ref_types is None:
                raise ValueError("commonCT is None, but cell_type columns were not found to infer it. Pass commonCT explicitly "
                                 f"or ensure both dataframes have '{ref_cell_type_col}'/'{moving_cell_type_col}'.")
            commonCT = sorted(ref_types)
            missing_ref = [c for c in commonCT if c not in ref.columns]
            missing_mov = [c for c in commonCT if c not in moving.columns]
            if missing_ref or missing_mov:
                raise ValueError("commonCT is None so it was inferred as the unique values of the cell_type column, but those "
                                 f"names are not present as probability/one-hot columns.\nMissing in ref columns (first 20): "
                                 f"{missing_ref[:20]}\nMissing in moving columns (first 20): {missing_mov[:20]}")
        self.ref, self.moving, self.commonCT = ref, moving, commonCT
        self.moving_delaunay, self.vertex_col = moving_delaunay, moving_delaunay_vertex_col
        self.ignore_pre = ignore_precomputed_triangulation
        self.caller_triangulation = moving_delaunay is not None and not ignore_precomputed_triangulation

        self.outprefix, self.output_file, self.all_matches = outprefix, None, []
        if outprefix:
            os.makedirs(outprefix, exist_ok=True)
            self.output_file = os.path.join(outprefix, "matchedDF.csv")
        plan_key = (self.window_size, self.overlap, min_cells)
        if resident is not None and plan_key in resident.plans:
            self.plan, self.grid = resident.plans[plan_key]
            plan = self.plan
        else:
            rxy, mxy = ref[["X", "Y"]].to_numpy(dtype=np.float64), moving[["X", "Y"]].to_numpy(dtype=np.float64)
            self.plan = plan = window_plan(rxy, mxy, self.window_size, self.overlap, min_cells)
            self.grid = window_grid(rxy, mxy, self.window_size, self.overlap)[:2] if plan else None
            if resident is not None:
                resident.plans[plan_key] = (plan, self.grid)
        done_ids = set()
        if self.output_file and os.path.exists(self.output_file):  # resume (src/helpers.py:21-70): skip windows already in the file
            existing = pd.read_csv(self.output_file)
            if "window_id" in existing.columns:
                done_ids = set(int(w) for w in existing["window_id"].unique())
                self.all_matches.append(existing)
        self.mine = self.owner = None
        if shard is not None:                    # (rank, world[, deal]): this process runs the windows the deal gives its rank
            from .windows import deal_windows
            self.owner = deal_windows(plan, int(shard[1]), shard[2] if len(shard) > 2 else "block")
            self.mine = set(np.flatnonzero(self.owner == int(shard[0])).tolist())
        self.todo = [(pos, w) for pos, w in enumerate(plan) if w["grid_id"] not in done_ids and (self.mine is None or pos in self.mine)]

    def window_outprefix(self, w):
        return os.path.join(self.outprefix, f"window_{w['window_id']}") if self.outprefix else None

    def device_frames(self, pipeline=None, ctx=None):
        """The two frames as device-resident sections, or None when this job runs the frame pipeline.  -> (frames, whether this job owns
        them: a caller's ResidentFrames stay up when the job is done)."""
        frames = self._device_frames(pipeline, ctx)
        return frames, (frames is not None and self.resident is None)

    def _device_frames(self, pipeline, ctx):
        if self.resident is not None:
            return self.resident.frames_for(self) if self.todo else None
        if window_pipeline(pipeline) != "device" or not self.todo:
            return None
        if _DeviceFrames.refusal(self.ref, self.moving, self.commonCT, self.optim_params, self.vertex_col) is not None:
            return None
        from .windows import window_cell_grid

        return _DeviceFrames(self.ref, self.moving, self.commonCT, self.optim_params,
                             window_cell_grid(self.grid, self.window_size, self.overlap), ctx=ctx)

    def collect(self, pos, w, window_matches):
        """Central trim + bookkeeping of one window's matches (src/same.py:565-590)."""
        if window_matches.shape[0] > 0:
            tx0, tx1, ty0, ty1 = w["trim"]
            x, y = window_matches["X"].to_numpy(), window_matches["Y"].to_numpy()       # the same comparisons on the columns' arrays
            central = window_matches[(x >= tx0) & (x < tx1) & (y >= ty0) & (y < ty1)].copy()
            central["window_id"] = w["window_id"]
            if self.mine is not None:
                central["__plan_pos"] = pos          # lets the sharded wrapper restore the single-process window order
            if len(central) > 0:
                self.all_matches.append(central)
                if self.outprefix:
                    pd.concat(self.all_matches, ignore_index=True).to_csv(self.output_file, index=False)

    def result(self):
        return pd.concat(self.all_matches, ignore_index=True) if self.all_matches else pd.DataFrame()


def _walk_windows(todo, frames, ref, moving, commonCT, optim_params, gurobi_params, *, verbose, ctx, moving_delaunay=None, vertex_col=None,
                  ignore_pre=False, fetch_triangles=False):
    """The one loop that turns windows into run_same's inputs: yields (pos, window, what) for every (pos, window) of `todo`, in order;
    `what` is a PreparedInputs, a _Staged (the caller's triangulation, or the frames pipeline: run_same's second half still to run) or
    the window's error (device pipeline; the frames pipeline's is inside its _Staged).  frames: _DeviceFrames -> the device pipeline on
    `ctx` (None: the frames' own); None -> the frames pipeline, windows n+1..n+k cut, pruned and handed to the Qhull helpers ahead."""
    caller_triangulation = moving_delaunay is not None and not ignore_pre
    if frames is not None:
        windows = frames.windows([w for _pos, w in todo], triangulate=not caller_triangulation, ctx=ctx, fetch_triangles=fetch_triangles)
        for (pos, w), dw in zip(todo, windows):
            if dw.error is not None:
                yield pos, w, _window_error(dw, optim_params)
            elif caller_triangulation:
                yield pos, w, _staged_from_device(dw, frames, commonCT, optim_params, gurobi_params, moving_delaunay, vertex_col,
                                                  verbose=verbose)
            else:
                yield pos, w, _prepared_from_device(dw, frames, optim_params, gurobi_params, verbose=verbose, vertex_col=vertex_col)
        return
    from . import qhull_pool

    depth = qhull_pool.lookahead()
    qhull_pool.warm(min(depth, len(todo)))      # helpers start (import scipy) while the first window is being pruned
    ref_rows, moving_rows = _WindowSubsetter(ref), _WindowSubsetter(moving)
    ahead = {}
    for q, (pos, w) in enumerate(todo):
        for nxt in range(q, min(q + 1 + depth, len(todo))):
            if nxt not in ahead:
                box = todo[nxt][1]["box"]
                ahead[nxt] = _stage_prune(ref_rows.subset(*box), moving_rows.subset(*box), commonCT, moving_delaunay, vertex_col,
                                          optim_params, gurobi_params, ignore_pre, verbose, ctx, prefetch=True, fresh_frames=True)
        yield pos, w, ahead.pop(q)


def iter_prepared_windows(ref, moving, commonCT, plan, optim_params=None, gurobi_params=None, verbose=False, ctx=None, pipeline=None):
    """Pre-MIP artefacts of every window of `plan` (windows.window_plan), in plan order: yields (window, PreparedInputs).
    Window n+1..n+k are staged ahead and triangulated by the Qhull helpers while the consumer works on window n (the same
    pipelining sliding_window_matching uses); a window whose prune leaves no pairs yields (window, the ValueError).
    pipeline: 'device' (default; both frames resident on the GPU, frames of a PreparedInputs made when read) or 'frames'."""
    op, gp = init_optim_params(**dict(optim_params or {})), init_gurobi_params(**dict(gurobi_params or {}))
    frames = None
    if window_pipeline(pipeline) == "device" and len(plan) and _DeviceFrames.refusal(ref, moving, commonCT, op) is None:
        frames = _DeviceFrames(ref, moving, commonCT, op, None, ctx=ctx)
    try:
        # (the frames pipeline's prune takes the parameters as given and completes them itself: op and gp are the same to it)
        for _pos, w, what in _walk_windows(list(enumerate(plan)), frames, ref, moving, commonCT, op, gp, verbose=verbose, ctx=ctx):
            if isinstance(what, _Staged):
                try:
                    what = prepare_same_inputs(None, None, commonCT, verbose=verbose, ctx=ctx, _staged=what)
                except ValueError as e:
                    what = e
            # only run_same's own ValueError is a window's answer; anything else ends the walk
            elif isinstance(what, Exception) and not isinstance(what, ValueError):
                raise what
            yield w, what
    finally:
        if frames is not None:
            frames.close()


def sliding_window_matching(ref, moving, commonCT=None, outprefix=None, moving_delaunay=None,
                            moving_delaunay_vertex_col=None, optim_params: Optional[Dict[str, Any]] = None,
                            gurobi_params: Optional[Dict[str, Any]] = None,
                            ignore_precomputed_triangulation: bool = False, _run_window=None, _shard=None, _pipeline=None, _solve=None,
                            _job=None):
    """Same contract as src/same.py:297-595.  `_run_window` (testing hook) replaces run_same; `_shard=(rank, world)` makes this
    call process only its share of the window plan (same_amd.dist.sharded_sliding_window_matching); `_pipeline` = 'device' | 'frames'
    (default: $SAME_WINDOW_PIPELINE, else 'device': both frames resident on the GPU for the whole loop, see the note above);
    `_solve(prep: PreparedInputs, outprefix) -> (matches_df, var_out)` stands in for the solver half of run_same (model assembly, solve,
    post-solve tables) behind the unchanged pre-MIP half -- how bench.py times this signature without a Gurobi licence.  `_job`: the
    job as a caller already settled it (dist.sharded_merged_window_matches reads its plan and deal afterwards)."""
    job = _job if _job is not None else _WindowJob(ref, moving, commonCT, outprefix, moving_delaunay, moving_delaunay_vertex_col,
                                                   optim_params,
                                                   gurobi_params, ignore_precomputed_triangulation, _shard)
    frames, own = job.device_frames(_pipeline)
    try:
        if _run_window is not None:
            _run_windows(job, frames, _run_window)
        else:
            _solver_windows(job, frames, _solve)
    finally:
        if own:
            frames.close()
    return job.result()


def _solver_windows(job, frames, solve=None):
    """The window loop: per window the pre-MIP half on either pipeline (`_walk_windows`; frames None: the frames pipeline), then the
    solver half -- run_same's own body, or the caller's stand-in (`_solve`) on the finished PreparedInputs.  A window whose prune finds
    no pair hands its error to the run_same body, which raises it where the reference does."""
    commonCT, op, gp = job.commonCT, job.optim_params, job.gurobi_params
    # the frames pipeline's prune always speaks; the device pipeline's only ahead of run_same's own body
    verbose = solve is None or frames is None
    for pos, w, what in _walk_windows(job.todo, frames, job.ref, job.moving, commonCT, op, gp, moving_delaunay=job.moving_delaunay,
                                      vertex_col=job.vertex_col, ignore_pre=job.ignore_pre, verbose=verbose, ctx=None):
        staged, prepared = (what, None) if isinstance(what, _Staged) else (None, what)
        if solve is None:
            window_matches, _ = _run_same(None, None, commonCT, job.window_outprefix(w), job.moving_delaunay, job.vertex_col, op, gp,
                                          job.ignore_pre, staged, prepared)
        elif isinstance(prepared, Exception):
            raise prepared
        else:
            prep = prepared if prepared is not None else prepare_same_inputs(None, None, commonCT, verbose=False, _staged=staged)
            window_matches, _ = solve(prep, job.window_outprefix(w))
        job.collect(pos, w, window_matches)


def _run_windows(job, frames, run_window):
    """The window loop with a stand-in for run_same (`_run_window`, testing): it takes the window's frames, subset_data of both -- from
    the device's row lists when the frames are resident, else cut on the host."""
    commonCT, op, gp = job.commonCT, job.optim_params, job.gurobi_params
    if frames is not None:
        from .windows import DeviceWindow

        state = DeviceWindow(frames.ctx)
        try:
            for pos, w in job.todo:
                rows_m, rows_r = frames.box_rows(w["box"], state)
                window_matches, _ = run_window(aligned_df=job.moving.iloc[rows_m], ref_df=job.ref.iloc[rows_r], commonCT=commonCT,
                                               optim_params=op, gurobi_params=gp, outprefix=job.window_outprefix(w),
                                               aligned_delaunay=job.moving_delaunay, aligned_delaunay_vertex_col=job.vertex_col,
                                               ignore_precomputed_triangulation=job.ignore_pre)
                job.collect(pos, w, window_matches)
        finally:
            state.close()
        return
    ref_rows, moving_rows = _WindowSubsetter(job.ref), _WindowSubsetter(job.moving)
    for pos, w in job.todo:
        ref_subset, moving_subset = ref_rows.subset(*w["box"]), moving_rows.subset(*w["box"])
        window_matches, _ = run_window(aligned_df=moving_subset, ref_df=ref_subset, commonCT=commonCT, optim_params=op, gurobi_params=gp,
                                       outprefix=job.window_outprefix(w), aligned_delaunay=job.moving_delaunay,
                                       aligned_delaunay_vertex_col=job.vertex_col, ignore_precomputed_triangulation=job.ignore_pre)
        job.collect(pos, w, window_matches)
