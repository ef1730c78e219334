"""Sliding-window tiler: the grid, merge-right / merge-down and central-trim rules of
sliding_window_matching (src/same.py:481-488, :509-582) as a plan of independent windows.

Windows are the shard unit for very large sections (BASELINE config 5).  Cell counts of every
box the merge logic can ask about (base, right-merged, down-merged, both) come from one
batched device pass (csrc/sweep.hip window_count_kernel) instead of one pandas boolean mask
per window; the sequential walk that decides merges is then pure host lookups."""
import ctypes
import os
from collections import deque, namedtuple

import numpy as np

from . import _lib, ops
from ._trace import stage as marked
from .delaunay import QHULL, QhullTriangulator, Ticket
from .window_mode import WindowMode


def window_grid(ref_xy, mov_xy, window_size, overlap):
    """src/same.py:481-488.  The reference takes the extent with pandas' min / max, which skip NaN (rows without coordinates are in no
    window; they do not stop the job): nanmin / nanmax here.  Infinite coordinates reach int() as they do there (OverflowError)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # an all-NaN column: NaN, and int(NaN) raises as in the reference
        x_min = min(np.nanmin(ref_xy[:, 0]), np.nanmin(mov_xy[:, 0]))
        x_max = max(np.nanmax(ref_xy[:, 0]), np.nanmax(mov_xy[:, 0]))
        y_min = min(np.nanmin(ref_xy[:, 1]), np.nanmin(mov_xy[:, 1]))
        y_max = max(np.nanmax(ref_xy[:, 1]), np.nanmax(mov_xy[:, 1]))
    step = window_size - overlap
    xs = list(range(int(x_min), int(x_max), step))
    ys = list(range(int(y_min), int(y_max), step))
    return xs, ys, (x_min, x_max, y_min, y_max)


def _candidate_boxes(xs, ys, ws):
    """All boxes the walk may query: variant 0 base, 1 right-merged, 2 down-merged, 3 both."""
    boxes = np.empty((len(xs), len(ys), 4, 4), np.float64)
    for i, x in enumerate(xs):
        xr = xs[i + 1] + ws if i + 1 < len(xs) else x + ws
        for j, y in enumerate(ys):
            yd = ys[j + 1] + ws if j + 1 < len(ys) else y + ws
            boxes[i, j, 0] = (x, x + ws, y, y + ws)
            boxes[i, j, 1] = (x, xr, y, y + ws)
            boxes[i, j, 2] = (x, x + ws, y, yd)
            boxes[i, j, 3] = (x, xr, y, yd)
    return boxes


def window_plan(ref_xy, mov_xy, window_size, overlap, min_cells, skip_ids=(), ctx=None):
    """The windows the reference's double while-loop would run, in order.

    Each entry: i0/j0 (grid cell where the window starts), i/j (after merges), grid_id
    (= len(xs)*j0+i0, what the resume check compares), window_id (= len(xs)*j+i, what is stored),
    box (x0,x1,y0,y1 half-open), trim (central region kept), n_ref, n_mov."""
    ref_xy = np.ascontiguousarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    mov_xy = np.ascontiguousarray(mov_xy, dtype=np.float64).reshape(-1, 2)
    xs, ys, (x_min, x_max, y_min, y_max) = window_grid(ref_xy, mov_xy, window_size, overlap)
    if not xs or not ys:
        return []
    boxes = _candidate_boxes(xs, ys, window_size)
    flat = boxes.reshape(-1, 4)
    n_ref = ops.window_count(ref_xy, flat, ctx=ctx).reshape(boxes.shape[:3])
    n_mov = ops.window_count(mov_xy, flat, ctx=ctx).reshape(boxes.shape[:3])
    skip_ids = set(skip_ids)

    plan = []
    i = 0
    while i < len(xs):
        j = 0
        while j < len(ys):
            if len(xs) * j + i in skip_ids:
                j += 1
                continue
            i0, j0 = i, j
            x, y = xs[i], ys[j]
            variant = 0
            nr, nm = n_ref[i0, j0, 0], n_mov[i0, j0, 0]
            if nr < min_cells or nm < min_cells:
                if i + 1 < len(xs):
                    variant = 1
                    nr, nm = n_ref[i0, j0, 1], n_mov[i0, j0, 1]
                    if nr >= min_cells and nm >= min_cells:
                        i += 1
                if (nr < min_cells or nm < min_cells) and j + 1 < len(ys):
                    variant |= 2
                    nr, nm = n_ref[i0, j0, variant], n_mov[i0, j0, variant]
                    if nr >= min_cells and nm >= min_cells:
                        j += 1
            if nr >= min_cells and nm >= min_cells:
                x0, x1, y0, y1 = (float(v) for v in boxes[i0, j0, variant])
                left, right = x == int(x_min), x1 >= int(x_max)
                top, bottom = y == int(y_min), y1 >= int(y_max)
                trim = (x0 if left else x0 + overlap / 2, x1 if right else x1 - overlap / 2,
                        y0 if top else y0 + overlap / 2, y1 if bottom else y1 - overlap / 2)
                plan.append({"i0": i0, "j0": j0, "i": i, "j": j, "grid_id": len(xs) * j0 + i0,
                             "window_id": len(xs) * j + i, "box": (x0, x1, y0, y1), "trim": trim,
                             "n_ref": int(nr), "n_mov": int(nm)})
            j += 1
        i += 1
    return plan


def assign_windows(plan, n_ranks):
    """Round-robin windows over ranks, heaviest first (windows are independent: no collective)."""
    order = sorted(range(len(plan)), key=lambda w: -(plan[w]["n_ref"] * plan[w]["n_mov"]))
    shards = [[] for _ in range(n_ranks)]
    for pos, w in enumerate(order):
        shards[pos % n_ranks].append(w)
    return [sorted(s) for s in shards]


def assign_window_blocks(plan, n_ranks):
    """Contiguous runs of the plan per rank, balanced by aligned cells (what a window costs: its triangulation and its pairs).
    The plan walks the window grid column by column (src/same.py:509-511), so a run is a strip of whole columns plus two partial ones:
    most overlaps between windows are then overlaps between windows of ONE rank, and the window merge (src/helpers.py:692-815) only
    has the strips' borders to settle between ranks (merge.seam_rows).  The ranks' tables laid end to end are in plan order."""
    weight = np.array([max(1, w["n_mov"]) for w in plan], dtype=np.float64)
    shards = [[] for _ in range(n_ranks)]
    if len(plan):
        middle = (np.cumsum(weight) - weight / 2) / weight.sum()              # where a window sits in the job's work, 0..1
        for w, q in enumerate(np.minimum((middle * n_ranks).astype(np.int64), n_ranks - 1).tolist()):
            shards[q].append(w)
    return shards


WINDOW_DEALS = ("block", "round_robin")


def deal_windows(plan, n_ranks, deal="block"):
    """-> owner[w] = the rank that runs window w of the plan: 'block' (assign_window_blocks) or 'round_robin' (assign_windows)."""
    if deal not in WINDOW_DEALS:
        raise ValueError(f"window deal must be one of {WINDOW_DEALS}, got {deal!r}")
    owner = np.zeros(len(plan), np.int32)
    for q, share in enumerate((assign_window_blocks if deal == "block" else assign_windows)(plan, n_ranks)):
        owner[share] = q
    return owner


class GridRows:
    """Row indices of the points inside half-open boxes [x0, x1) x [y0, y1), for many boxes of one point set: the points are
    binned once into a uniform grid (counting sort by cell), a box gathers the cells it touches (one contiguous run per grid
    row) and only those points are tested exactly.  Indices come back ascending -- `np.flatnonzero` of the reference's four
    comparisons (src/same.py:293-295); NaN / infinite coordinates fall outside every box either way."""

    GRID = 256

    def __init__(self, x, y):
        self.x, self.y = x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        finite = np.isfinite(x) & np.isfinite(y)
        ok = None if finite.all() else np.flatnonzero(finite)
        xo, yo = (x, y) if ok is None else (x[ok], y[ok])
        self.nx = self.ny = 1
        self.x0 = self.y0 = 0.0
        self.inv = 1.0
        if len(xo):
            self.x0, self.y0 = float(xo.min()), float(yo.min())
            extent = max(float(xo.max()) - self.x0, float(yo.max()) - self.y0)
            if extent > 0.0:
                self.inv = self.GRID / extent * (1.0 - 1e-12)
                self.nx = self.ny = self.GRID
        ix = ((xo - self.x0) * self.inv).astype(np.int32)
        iy = ((yo - self.y0) * self.inv).astype(np.int32)
        np.minimum(ix, self.nx - 1, out=ix)
        np.minimum(iy, self.ny - 1, out=iy)
        key = (iy * self.nx + ix).astype(np.uint16)     # GRID^2 cells fit 16 bits: numpy's stable sort of uint16 is a radix sort
        order = np.argsort(key, kind="stable")
        self.order = order if ok is None else ok[order]
        self.starts = np.concatenate(([0], np.cumsum(np.bincount(key, minlength=self.nx * self.ny))))

    def _cell(self, v, v0, n):
        c = np.floor((v - v0) * self.inv)
        return int(min(max(c, 0), n - 1)) if c == c else 0

    def rows(self, x_min, x_max, y_min, y_max):
        ix0, ix1 = self._cell(x_min, self.x0, self.nx), self._cell(x_max, self.x0, self.nx)
        iy0, iy1 = self._cell(y_min, self.y0, self.ny), self._cell(y_max, self.y0, self.ny)
        st, od = self.starts, self.order
        runs = [od[st[iy * self.nx + ix0]: st[iy * self.nx + ix1 + 1]] for iy in range(iy0, iy1 + 1)]
        cand = np.concatenate(runs) if runs else od[:0]
        xx, yy = self.x[cand], self.y[cand]
        return np.sort(cand[(xx >= x_min) & (xx < x_max) & (yy >= y_min) & (yy < y_max)])

    def positions(self, x_min, x_max, y_min, y_max, xs, ys):
        """As rows(), for data kept in GRID order: `xs`, `ys` are the coordinates permuted by `self.order`.  -> (rows ascending,
        pos) with order[pos] == rows, so `column_in_grid_order[pos]` is the column's values for `rows`.  The candidates of a box
        are a few contiguous runs of the grid-ordered arrays, so everything a window reads of a million-cell section comes from
        ~1 MB of neighbouring memory instead of 10^4 cache-missing rows scattered over the whole array."""
        ix0, ix1 = self._cell(x_min, self.x0, self.nx), self._cell(x_max, self.x0, self.nx)
        iy0, iy1 = self._cell(y_min, self.y0, self.ny), self._cell(y_max, self.y0, self.ny)
        st = self.starts
        runs = [np.arange(st[iy * self.nx + ix0], st[iy * self.nx + ix1 + 1]) for iy in range(iy0, iy1 + 1)]
        pos = np.concatenate(runs) if runs else np.zeros(0, np.int64)
        xx, yy = xs[pos], ys[pos]
        pos = pos[(xx >= x_min) & (xx < x_max) & (yy >= y_min) & (yy < y_max)]
        rows = self.order[pos]
        o = np.argsort(rows, kind="stable")
        return rows[o], pos[o]


class Section:
    """One tissue section as columns (no DataFrame): what the window pipeline reads of it.
    xy (n, 2) float64; types (n, T) float64, the commonCT columns in commonCT order; type_id (n,) int32 codes of the cell
    type (equal type <=> equal code); size (n,) (integer dtype kept: it decides the dtype of the triangle weights).
    The host-side grid and the grid-ordered copies of the columns (`grid`, `g_*`) are what the COLUMN pipeline subsets with; they are
    built on first use, so a section that only feeds a DeviceSection never pays for them."""

    def __init__(self, xy, types, type_id=None, size=None):
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        t = np.ascontiguousarray(types, dtype=np.float64)
        self.types = t if (t.ndim == 2 and len(t) == len(self.xy)) else t.reshape(len(self.xy), -1)      # (0, T) stays (0, T)
        self.type_id = None if type_id is None else np.ascontiguousarray(type_id, dtype=np.int32)
        self.size = np.ones(len(self.xy), np.int64) if size is None else np.asarray(size)
        self._host = None

    def _host_grid(self):
        if self._host is None:
            grid = GridRows(self.xy[:, 0], self.xy[:, 1])
            od = grid.order     # the same columns once more in GRID order (GridRows.positions): what the window loop gathers from
            g_xy = np.ascontiguousarray(self.xy[od])
            self._host = {"grid": grid, "g_xy": g_xy, "g_types": np.ascontiguousarray(self.types[od]), "g_size": self.size[od],
                          "g_x": np.ascontiguousarray(g_xy[:, 0]), "g_y": np.ascontiguousarray(g_xy[:, 1]),
                          "g_type_id": None if self.type_id is None else self.type_id[od]}
        return self._host

    grid = property(lambda self: self._host_grid()["grid"])
    g_xy = property(lambda self: self._host_grid()["g_xy"])
    g_types = property(lambda self: self._host_grid()["g_types"])
    g_size = property(lambda self: self._host_grid()["g_size"])
    g_x = property(lambda self: self._host_grid()["g_x"])
    g_y = property(lambda self: self._host_grid()["g_y"])
    g_type_id = property(lambda self: self._host_grid()["g_type_id"])

    def window(self, box):
        """-> (rows ascending, positions into the grid-ordered columns) of the section's points inside the half-open box."""
        return self.grid.positions(*box, self.g_x, self.g_y)

    @classmethod
    def from_frame(cls, df, commonCT):
        import pandas as pd

        type_id = pd.factorize(df["cell_type"].to_numpy(), use_na_sentinel=False)[0] if "cell_type" in df.columns else None
        return cls(df[["X", "Y"]].to_numpy(dtype=np.float64), df[list(commonCT)].to_numpy(dtype=np.float64), type_id,
                   df["size"].to_numpy() if "size" in df.columns else None)


class WindowArrays:
    """Pre-MIP artefacts of one window as flat arrays (what PreparedInputs holds, without the frames): `rows_m` / `rows_r` are
    the section rows of the window's compacted aligned / reference cells, `pairs` (P, 2) int64 index into them, `costs` (P,)
    float64 in pair order, `triangles` (Tr, 3) of compacted aligned rows in the reference's kept order, `weights`, `signs`."""

    __slots__ = ("window", "rows_m", "rows_r", "pairs", "costs", "triangles", "weights", "signs", "axy", "rxy", "size", "error")

    def __init__(self, window):
        self.window = window
        for name in self.__slots__[1:]:
            setattr(self, name, None)

    @property
    def n_aligned(self):
        return len(self.rows_m)

    @property
    def n_ref(self):
        return len(self.rows_r)


def iter_window_arrays(ref, moving, plan, radius=250, knn=8, dist_ct_coeff=1.0, min_angle_deg=15, ignore_same_type_triangles=True,
                       cost_dtype=np.float64, ctx=None):
    """The pre-MIP path of every window of `plan` on COLUMNS (two `Section`s), in plan order: yields one `WindowArrays` per
    window -- the same pairs, costs, kept triangles, weights and signs `api.iter_prepared_windows` computes from frames
    (tests/test_gpu_run_same.py::test_window_arrays_equal_prepared_windows), without building a DataFrame per window.  The
    frame pipeline spends ~90 % of a window in pandas `take`s that the reference's return types force at its boundary; a
    caller that feeds the artefacts straight to kernels (bench.py --workload cfg5) does not need them.  Windows n+1..n+k are
    subset, pruned and compacted ahead and triangulated by the Qhull helpers while window n runs, as in the frame pipeline.
    A window whose prune leaves no pairs yields a WindowArrays whose `.error` is the ValueError run_same would raise."""
    from . import qhull_pool
    from ._trace import stage as marked
    from .knn import pairs_from_padded
    from .triangles import filter_triangles_by_radius

    depth = qhull_pool.lookahead()
    qhull_pool.warm(min(depth, len(plan)))
    cost_dtype = np.dtype(cost_dtype)

    def stage(w):
        with marked("prune+compact"):
            return prune(w)

    def prune(w):
        out = WindowArrays(w)
        (rows_r, pos_r), (rows_m, pos_m) = ref.window(w["box"]), moving.window(w["box"])
        axy, rxy = moving.g_xy[pos_m], ref.g_xy[pos_r]
        # the argument checks cKDTree makes for the reference are moot here: GridRows only returns finite points
        r = float(radius)
        if r != r or int(knn) <= 0 or len(rxy) == 0 or len(axy) == 0:
            idx = np.full((len(axy), 1), -1, np.int32)
        else:
            idx, _, _ = ops.knn_prune(axy, rxy, abs(r), knn, want_d2=False, ctx=ctx)
        kp = pairs_from_padded(idx)
        if len(kp) == 0:
            out.error = ValueError("No valid_pairs after KNN filtering. Increase radius and/or knn.")
            return out, None
        used_a = np.zeros(len(axy), bool)
        used_a[kp[:, 0]] = True
        used_r = np.zeros(len(rxy), bool)
        used_r[kp[:, 1]] = True
        ua, ur = np.flatnonzero(used_a), np.flatnonzero(used_r)            # compaction (src/utils.py:734-742)
        out.pairs = np.column_stack(((np.cumsum(used_a) - 1)[kp[:, 0]], (np.cumsum(used_r) - 1)[kp[:, 1]])).astype(np.int64)
        out.rows_m, out.rows_r = rows_m[ua], rows_r[ur]
        out.axy, out.rxy = np.ascontiguousarray(axy[ua]), np.ascontiguousarray(rxy[ur])
        return out, (qhull_pool.pool().submit(out.axy), pos_m[ua], pos_r[ur])

    def finish(out, staged):
        ticket, pos_m, pos_r = staged
        with marked("triangulate (wait for helper)"):
            tris = ticket.result()
        with marked("triangle filter"):
            tid = moving.g_type_id[pos_m] if (ignore_same_type_triangles and moving.g_type_id is not None) else None
            out.triangles = filter_triangles_by_radius(out.axy, tris, radius, ignore_same_type_triangles=ignore_same_type_triangles,
                                                       min_angle_deg=min_angle_deg, verbose=False, ctx=ctx, _rows_as_array=True,
                                                       _type_id=tid)
        with marked("triangle weights + source signs"):
            out.size = moving.g_size[pos_m]
            sign, weight = ops.tri_sign_weight(out.axy, out.size.astype(np.float64), out.triangles, ctx=ctx)
            out.weights = weight.astype(np.int64) if np.issubdtype(out.size.dtype, np.integer) else weight
            out.signs = sign.astype(np.float64)
        with marked("pair costs"):
            out.costs = ops.pair_cost(moving.g_types[pos_m], ref.g_types[pos_r], out.axy, out.rxy, out.pairs, dist_ct_coeff,
                                      dtype=cost_dtype, ctx=ctx).astype(np.float64, copy=False)
        return out

    ahead = {}
    for q in range(len(plan)):
        for nxt in range(q, min(q + 1 + depth, len(plan))):
            if nxt not in ahead:
                ahead[nxt] = stage(plan[nxt])
        out, staged = ahead.pop(q)
        yield out if out.error is not None else finish(out, staged)


# ---- the window path with the sections resident on the device (csrc/window_stage.hip, csrc/window_finish.hip) -------------

_W_ALIGNED_XY, _W_ALIGNED_ROWS, _W_ROWS_M, _W_ROWS_R, _W_PAIRS, _W_COSTS, _W_KEPT, _W_SIGNS, _W_WEIGHTS, _W_MATCH, _W_TRIANGLES = range(11)
_W_CALLER_TRIANGLES, _W_STAGED_PAIRS = 11, 12      # SAME_WINDOW_CALLER_TRIANGLES, SAME_WINDOW_STAGED_PAIRS


def window_cell_grid(plan_or_grid, window_size, overlap):
    """(x0, y0, cell) of the grid on which every box of a window plan is a union of cells: the plan's boxes start at the grid
    origins int(x_min) + i * step and end window_size later (merged ones at a later origin + window_size: src/same.py:481-488,
    :527-542), so with cell = gcd(step, window_size) all their edges are cell edges (window sizes whose gcd with the step is small get
    quarter-window cells instead: correct for any box, only no longer test-free).  `plan_or_grid` = (xs, ys) of window_grid."""
    import math

    xs, ys = plan_or_grid
    step = int(window_size) - int(overlap)
    cell = float(math.gcd(step, int(window_size)))
    # a window of more than ~5 x 5 such cells (8 x 8 once merged) would leave the cell-run path (<= 64 cells):
    if window_size / cell > 5:
        # quarter windows instead -- boxes then cut through cells and their candidates are tested, still O(window)
        cell = window_size / 4.0
    return float(xs[0]), float(ys[0]), cell


class _DeviceHandle:
    """The owner of one library object made on a context, stated once for the classes below: the create call (`_ENTRY[0]`; a create
    that fails after it made something has that destroyed), `close()` through `_ENTRY[1]` and a `__del__` that cannot raise."""

    _ENTRY = (None, None)        # the library's create and destroy entry points

    def _create(self, ctx, *args):
        """`handle` = what create(context, *args, &handle) makes on `ctx`, which becomes `self.ctx`"""
        self.ctx = ctx = ops._ctx(ctx)
        create, destroy = self._ENTRY
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = getattr(ctx.lib, create)(ctx.handle, *args, ctypes.byref(h))
            if rc != 0 and h.value:
                getattr(ctx.lib, destroy)(h)
            ctx.check(rc, create)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:        # a context that is already gone took its device memory along
            with self.ctx.lock:
                getattr(self.ctx.lib, self._ENTRY[1])(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSection(_DeviceHandle):
    """A `Section`'s XY, type columns and sizes uploaded once (same_section_create) and binned into a grid of cells; every window
    reads them in place.  cost_dtype float32 keeps the cost operands as float (BASELINE cfg 5), float64 is the reference's
    arithmetic.  `bin(x0, y0, cell)` re-bins the rows on the window grid (window_cell_grid), on which a window's rows are
    whole cells: do it once, before the windows run."""

    _ENTRY = ("same_section_create", "same_section_destroy")

    def __init__(self, section, cost_dtype=np.float64, ctx=None):
        self.section = section
        self.cost_dtype = np.dtype(cost_dtype)
        if self.cost_dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError(f"cost_dtype must be float64 or float32, not {self.cost_dtype}")
        size = np.ascontiguousarray(section.size, dtype=np.float64)
        tid = None if section.type_id is None else np.ascontiguousarray(section.type_id, dtype=np.int32)
        self._create(ctx, section.xy.ctypes.data, section.types.ctypes.data, section.types.shape[1], size.ctypes.data,
                     None if tid is None else tid.ctypes.data, len(section.xy), int(self.cost_dtype == np.dtype(np.float32)))

    def bin(self, x0, y0, cell_w, cell_h=None):
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_section_bin(self.handle, float(x0), float(y0), float(cell_w),
                                                         float(cell_w if cell_h is None else cell_h)),
                           "same_section_bin")
        return self

    def set_codes(self, codes, n_codes):
        """codes[row] = rank of the row's cell id among the section's ids (what the window merge on the device compares and orders by);
        None: a row's code is its number."""
        c = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32)
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_section_set_codes(self.handle, None if c is None else c.ctypes.data, int(n_codes)),
                           "same_section_set_codes")

    def set_label_codes(self, codes):
        """codes[row] = the row's cell-type label code, made jointly over the two sections of a job (eval_utils._label_codes): what the
        cell-type-priority prune on the device compares (priority_windows).  A slot of its own, beside the merge's id codes."""
        ops.section_set_label_codes(self.ctx, self.handle, codes, len(self.section.xy))


class DeviceTypesLayer(_DeviceHandle):
    """One more (n, T) type matrix for the rows of a DeviceSection, resident beside it (same_types_layer_create): `types` float64, the
    commonCT columns in commonCT order, one row per section row; in a float32 section the float copy is made once, as the section's own.
    What `recost_windows` prices a staged window's pair list from and `MergeAccumulator.columns` reads a table's type columns from.
    Read-only: the worker contexts of the device share it.  Close it BEFORE its section."""

    _ENTRY = ("same_types_layer_create", "same_types_layer_destroy")

    def __init__(self, dsection, types, ctx=None):
        want = dsection.section.types.shape
        self.types = types = np.ascontiguousarray(types, dtype=np.float64)
        if types.shape != want:
            raise ValueError(f"a types layer of this section is {want}, not {types.shape}")
        self.dsection = dsection
        self._create(ctx, dsection.handle, types.ctypes.data if types.size else None)


class DeviceWindow(_DeviceHandle):
    """Device state of one window in flight (same_window): `stage` then `filter_finish` (or `finish` with triangles filtered by the
    caller), arrays of the state through `fetch`.  `stage_windows` / `filter_finish_windows` run a BATCH of windows per library call."""

    _ENTRY = ("same_window_create", "same_window_destroy")

    def __init__(self, ctx=None):
        self._create(ctx)
        self.counts = (0, 0, 0, 0)
        self.n_triangles = 0
        self.n_staged_pairs = self.n_selected = 0      # pairs as staged; the caller's triangles over the staged cells (caller_tris_windows)
        self.assignment = self.refine = None
        self.priority = None       # priority_windows: (pairs staged, pairs left, rows that kept one pair, rows that kept all)

    def stage(self, moving, ref, box, radius, knn, dist_ct_coeff):
        """-> (aligned rows in the box, reference rows in the box, aligned rows kept, pairs)"""
        return stage_windows([self], moving, ref, [box], radius, knn, dist_ct_coeff)[0]

    # what -> (dtype, which count gives the length: 0 aligned in box, 1 refs in box, 2 kept, 3 pairs, 4 triangles, 5 pairs as staged,
    # 6 the caller's triangles selected; trailing width)
    _FETCH = {_W_ALIGNED_XY: (np.float64, 2, 2), _W_ALIGNED_ROWS: (np.int32, 2, 0), _W_ROWS_M: (np.int32, 0, 0),
              _W_ROWS_R: (np.int32, 1, 0),
              _W_PAIRS: (np.int32, 3, 2), _W_COSTS: (np.float64, 3, 0), _W_KEPT: (np.int32, 2, 0), _W_SIGNS: (np.int8, 4, 0),
              _W_WEIGHTS: (np.float64, 4, 0), _W_MATCH: (np.int32, 2, 0), _W_TRIANGLES: (np.int32, 4, 3),
              _W_CALLER_TRIANGLES: (np.int32, 6, 3), _W_STAGED_PAIRS: (np.int32, 5, 2)}

    def fetch(self, what):
        dtype, which, width = self._FETCH[what]
        n = (self.n_triangles, self.n_staged_pairs, self.n_selected)[which - 4] if which >= 4 else self.counts[which]
        out = np.empty((n, width) if width else (n,), dtype)
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_window_fetch(self.handle, int(what), out.ctypes.data, out.nbytes), "same_window_fetch")
        return out

    STAT_NAMES = ("checked", "flipped", "xy_comparisons", "xy_violations", "xy_triangles", "area_flips", "greedy_rounds", "matched")

    def filter_finish(self, simplices, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, no_match_penalty,
                      ensure_min_triangle_per_node=True, mode=None):
        """filter_triangles_by_radius of the kept aligned cells' Delaunay simplices, then signs, weights, the incumbent and the three
        sweeps, in one call.  -> (kept, added back, near, match_row, flag, stats); with near != 0 (cosines within near_tol of the
        threshold) the last three are None and the caller filters on the host and calls finish() with its triangles.  `mode`: a
        WindowMode."""
        return filter_finish_windows([self], [simplices], radius, angle_enabled, cos_thr, near_tol, ignore_same_type, no_match_penalty,
                                     ensure_min_triangle_per_node, mode=mode)[0]

    def finish(self, triangles, no_match_penalty, mode=None):
        """The same with triangles the CALLER filtered (kept ones, in the reference's order).  -> (section row of the matched reference
        cell per kept aligned cell or -1, flag byte per kept cell: bit 0 = XY-order sweep, bit 1 = vertex of an area-flipped triangle;
        stats dict)."""
        return filter_finish_windows([self], [triangles], 0.0, 0, 0.0, 0.0, False, no_match_penalty, True, prefiltered=True,
                                     mode=mode)[0][3:]

    def refinish(self, match_pair, no_match_penalty, mode=None):
        """the finished window's matched rows and sweeps again under `match_pair` (pair index per kept cell, -1 = none), the search of
        `mode` (a WindowMode; its start is not run again) from it first -> (match_row, flag byte, stats dict) as `finish`
        (greedy_rounds 0); `refine` is set to the search's record (decoded with start=False: these stats hold no start's words)"""
        mode = WindowMode.default() if mode is None else mode
        n = self.counts[2]
        match_pair = np.ascontiguousarray(match_pair, dtype=np.int32)
        assert len(match_pair) == n
        match_row, flag, stats = np.empty(n, np.int32), np.empty(n, np.uint8), np.zeros(mode.refinish_width, np.int64)
        args = (self.handle, match_pair.ctypes.data, float(no_match_penalty), *mode.search_args)
        outs = (match_row.ctypes.data, flag.ctypes.data, stats.ctypes.data)
        with self.ctx.lock:
            if mode.refine != "capacity":
                self.ctx.check(self.ctx.lib.same_window_refinish(*args, *outs), "same_window_refinish")
            else:
                capacity = mode.c_capacity()
                self.ctx.check(self.ctx.lib.same_window_refinish_cap(*args, ctypes.byref(capacity), *outs), "same_window_refinish_cap")
        self.refine = mode.records(stats, start=False)[1]
        return match_row, flag, dict(zip(self.STAT_NAMES, stats[:8].tolist()))


# SAME_MERGE_REST
REST_RECORD = np.dtype([("row", "<i4"), ("ac", "<i4"), ("rc", "<i4"), ("wid", "<i4"), ("pos", "<i4"), ("cidx", "<i4"), ("flags", "<u4")])
# SAME_MERGE_FINAL
FINAL_RECORD = np.dtype([("a_row", "<i4"), ("r_row", "<i4"), ("cidx", "<i4"), ("wid", "<i4"), ("pos", "<i4"), ("flags", "<u4")])


class _PinnedBlocks:
    """Page-locked host blocks the device writes the merged table's columns into (same_host_alloc), handed out as numpy arrays.
    A block goes back to the pool when the last array made of it is gone (a result table is usually dropped before the next pass: the
    pool then serves every pass from the same block, and no pass pays the pinning again); at most KEEP blocks wait in the pool, and while
    more than LIMIT are out with callers (tables kept alive) `take` declines -- the caller then gathers on the host as before.
    A block comes back from a finalizer, i.e. wherever the interpreter happens to drop the last reference (possibly inside `take` itself,
    during a garbage collection): that path only moves entries between lists under a re-entrant lock; memory the pool does not keep is
    handed back to the driver by the next `take` / `drop`, never from the finalizer."""

    KEEP, LIMIT = 2, 4

    def __init__(self):
        import threading

        self.free, self.surplus, self.out, self.lock = [], [], 0, threading.RLock()

    def take(self, ctx, nbytes):
        """-> (ctypes char array over a pinned block of >= nbytes, address) or None"""
        import weakref

        self._release_surplus()
        with self.lock:
            if self.out >= self.LIMIT:
                return None
            fit = [q for q, (c, cap, _p) in enumerate(list(self.free)) if c is ctx and cap >= nbytes]
            got = self.free.pop(min(fit, key=lambda q: self.free[q][1])) if fit else None
            self.out += 1
        if got is not None:
            _c, cap, ptr = got
        else:
            cap, ptr = (int(nbytes * 1.1) + (1 << 20)) & ~((1 << 20) - 1), ctypes.c_void_p()
            with ctx.lock:
                rc = ctx.lib.same_host_alloc(ctx.handle, cap, ctypes.byref(ptr))
            if rc != 0:
                with self.lock:
                    self.out -= 1
                return None
            ptr = ptr.value
        buf = (ctypes.c_char * cap).from_address(ptr)
        weakref.finalize(buf, self._back, ctx, cap, ptr)          # when the last array over `buf` is gone
        return buf, ptr

    def _back(self, ctx, cap, ptr):
        with self.lock:
            self.out -= 1
            (self.free if len(self.free) < self.KEEP and ctx.handle else self.surplus).append((ctx, cap, ptr))

    def _release_surplus(self):
        with self.lock:
            gone, self.surplus = self.surplus, []
        for ctx, _cap, ptr in gone:
            self._release(ctx, ptr)

    @staticmethod
    def _release(ctx, ptr):
        try:
            if ctx.handle:
                with ctx.lock:
                    ctx.lib.same_host_free(ctx.handle, ptr)
        except Exception:
            pass

    def drop(self, ctx=None):
        """free the waiting blocks (of one context, or all)"""
        with self.lock:
            gone = [e for e in self.free if ctx is None or e[0] is ctx]
            self.free = [e for e in self.free if e not in gone]
        for c, _cap, ptr in gone:
            self._release(c, ptr)
        self._release_surplus()


PINNED_BLOCKS = _PinnedBlocks()


class MergeAccumulator(_DeviceHandle):
    """The rows of one pass over a window plan on one context (same_merge_acc, csrc/window_merge.hip): `collect` appends the matched cells
    of the windows' central regions where they are -- on the device --, `resolve_accumulators` / `finish` run the window merge on them."""

    _ENTRY = ("same_merge_acc_create", "same_merge_acc_destroy")

    def __init__(self, ctx=None):
        self._create(ctx)

    def begin(self, expected_rows, near=None, reach=0.0, all_seam=False):
        """A new pass.  near = (near_start int32[n_pos + 1], near_boxes float64[.., 4]): per plan position the central regions of OTHER
        ranks' windows close enough to share cells with it (merge.seam_tables); None: one rank."""
        ctx = self.ctx
        if near is None:
            n_pos, ns, nb = 0, None, None
        else:
            ns, nb = np.ascontiguousarray(near[0], dtype=np.int32), np.ascontiguousarray(near[1], dtype=np.float64).reshape(-1, 4)
            n_pos = len(ns) - 1
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_begin(self.handle, int(expected_rows), n_pos, None if ns is None else ns.ctypes.data,
                                                   None if nb is None or len(nb) == 0 else nb.ctypes.data, float(reach),
                                                   int(bool(all_seam))),
                      "same_merge_acc_begin")

    def collect(self, states, trims, window_ids, plan_pos):
        """Enqueue only: the matched cells of the finished windows `states` that lie in their central regions join the accumulator."""
        ctx, n = self.ctx, len(states)
        t = np.ascontiguousarray(trims, dtype=np.float64).reshape(n, 4)
        w, p = np.ascontiguousarray(window_ids, dtype=np.int32), np.ascontiguousarray(plan_pos, dtype=np.int32)
        with ctx.lock:
            ctx.check(ctx.lib.same_window_collect(_handles(states), n, self.handle, t.ctypes.data, w.ctypes.data, p.ctypes.data),
                      "same_window_collect")

    def load(self, a_code, r_code, flags, window_ids, pos, cidx, n_codes_a, n_codes_r):
        """Rows from the host instead of from windows (the ranks' seam rows after their exchange): the accumulator then holds exactly
        these rows, whose cells are named by codes; `resolve_accumulators([acc], None, None)` and `finish` follow."""
        ctx = self.ctx
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        a, r, w, p, c = i32(a_code), i32(r_code), i32(window_ids), i32(pos), i32(cidx)
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_load(self.handle, a.ctypes.data, r.ctypes.data, f.ctypes.data, w.ctypes.data, p.ctypes.data,
                                                  c.ctypes.data,
                                                  len(a), int(n_codes_a), int(n_codes_r)), "same_merge_acc_load")

    def finish(self, winner_rows, fetch=True):
        """The REST rows the host's matching kept (accumulator row numbers) -> the merged table's rows, aligned codes ascending: as
        FINAL_RECORDs, or (fetch=False) only their number -- they stay on the device for `columns`; `final_rows()` fetches them later."""
        ctx = self.ctx
        w = np.ascontiguousarray(winner_rows, dtype=np.int32)
        n = ctypes.c_int64(0)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_finish(self.handle, w.ctypes.data if len(w) else None, len(w), ctypes.byref(n)),
                      "same_merge_acc_finish")
        self.n_final = n.value
        return self.final_rows() if fetch else self.n_final

    def final_rows(self):
        out = np.empty(self.n_final, FINAL_RECORD)
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_merge_acc_fetch(self.handle, 1, out.ctypes.data, out.nbytes), "same_merge_acc_fetch")
        return out

    def score(self, dmoving, dref, tris=None, ignore_same_type=True, node_local=False, majority_threshold=0.5, min_flips=1):
        """After finish(): the merged rows reduced to same_merge_acc_score's eight counts (csrc/window_score.hip) -- final rows, rows whose
        two label codes agree, triangles resident in `tris` (a DeviceCallerTris of `dmoving`; None: no triangle counts), all matched, same
        type skipped, flipped, flipped among those not skipped, rows in a violating triangle -- as an int64 array.  Both sections carry
        label codes (DeviceSection.set_label_codes).  One wait; no table is made."""
        ctx, counts = self.ctx, np.zeros(8, np.int64)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_score(self.handle, dmoving.handle, dref.handle, None if tris is None else tris.handle,
                                                   int(bool(ignore_same_type)), int(bool(node_local)), float(majority_threshold),
                                                   int(min_flips), counts.ctypes.data), "same_merge_acc_score")
        return counts

    def score_detail(self, dmoving, dref, tris, detail, ignore_same_type=True, node_local=False, majority_threshold=0.5, min_flips=1):
        """After finish(): the merged rows binned by same_merge_acc_score_detail (csrc/window_score_detail.hip) under `detail`, a
        DeviceScoreDetail of `dmoving`; the other arguments are `score`'s.  -> the call's int64 words cut by `detail.split`: a dict of
        `confusion` (L, L), `unlabelled`, `groups` (G + 1, 8: `score`'s eight counts per group, the last row the cross bin),
        `strict` and `weak` (SCORE_RANKS + 1 each) and `untyped`.  One wait; leaves the accumulator as `score` does."""
        ctx, out = self.ctx, np.zeros(detail.n_words, np.int64)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_score_detail(self.handle, dmoving.handle, dref.handle, None if tris is None else tris.handle,
                                                          detail.handle, int(bool(ignore_same_type)), int(bool(node_local)),
                                                          float(majority_threshold), int(min_flips), out.ctypes.data, len(out)),
                      "same_merge_acc_score_detail")
        return detail.split(out)

    def score_map(self, dmoving, dref, tris, detail, score_map, ignore_same_type=True, node_local=False, majority_threshold=0.5,
                  min_flips=1, marks=True):
        """After finish(): `score`'s counts and, per row of the moving section, its mark (same_merge_acc_score_map,
        csrc/window_score_map.hip) -- folded into `score_map`, a DeviceScoreMap of the two sections, whose truth rows the marks are read
        against.  `detail`: a DeviceScoreDetail of `dmoving` whose label columns rank the rows (None: no ranks); the other arguments are
        `score`'s.  -> (ten int64 counts: `score`'s eight, matched rows with a known truth, those on it; the marks as a CELL_MARK array
        over a pooled page-locked block, or None with marks=False).  One wait; leaves the accumulator as `score` does."""
        ctx, counts = self.ctx, np.zeros(10, np.int64)
        n = len(dmoving.section.xy)
        out = None
        if marks:
            got = PINNED_BLOCKS.take(ctx, max(1, n * CELL_MARK.itemsize))
            out = np.empty(n, CELL_MARK) if got is None else np.frombuffer(got[0], dtype=CELL_MARK, count=n)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_score_map(self.handle, dmoving.handle, dref.handle, None if tris is None else tris.handle,
                                                       None if detail is None else detail.handle, score_map.handle,
                                                       int(bool(ignore_same_type)), int(bool(node_local)), float(majority_threshold),
                                                       int(min_flips), None if out is None or not n else out.ctypes.data,
                                                       counts.ctypes.data), "same_merge_acc_score_map")
        return counts, out

    def score_features(self, dmoving, dref, features, zone=None, d2=False):
        """After finish(): the merged rows read as feature sums (same_merge_acc_score_features, csrc/window_score_feature.hip) under
        `features`, a DeviceScoreFeatures of the two sections, and `zone`, a DeviceFeatureZone of it (None: no distance reading).
        -> (the call's int64 words cut by `split_score_features`: `counts`, `rows`, `sums` and with a zone `bin_rows`, `bin_sums`; with
        `d2` and a zone the float64 squared distance to the zone per moving row, NaN where the row has no subset pair, else None).
        Touches none of the other reader calls' buffers."""
        ctx = self.ctx
        B = 0 if zone is None else zone.n_bins
        out = np.zeros(score_feature_words(features.n_groups, features.n_columns, B), np.int64)
        dist = np.empty(features.n_rows, np.float64) if d2 and zone is not None else None
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_score_features(self.handle, dmoving.handle, dref.handle, features.handle,
                                                            None if zone is None else zone.handle, out.ctypes.data, len(out),
                                                            None if dist is None or not len(dist) else dist.ctypes.data),
                      "same_merge_acc_score_features")
        return split_score_features(out, features.n_groups, features.n_columns, B), dist

    def unpack(self, mov_members, ref_members, strategy, pairs=False):
        """After finish(): the merged metacell rows unpacked to cells (same_merge_acc_unpack, csrc/window_unpack.hip) under `strategy`
        ("distribute" / "nearest"; `mov_members`, `ref_members`: DeviceMembers of the sections the pass ran over) -> the int64 counts
        (final rows, pairs, pairs whose two label codes agree, largest member count met); with `pairs` (counts, per pair the flat index
        of its reference member in `ref_members`' CSR) -- the pairs in the order of the final rows and of each moving row's members.
        A merge names a moving row once, so the moving side's member count bounds the pairs: one call."""
        if strategy not in UNPACK_STRATEGIES:
            raise ValueError(f"strategy must be one of {tuple(UNPACK_STRATEGIES)}, not {strategy!r}")
        ctx, counts = self.ctx, np.zeros(4, np.int64)
        out = np.empty(mov_members.n_members, np.int64) if pairs else None
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_unpack(self.handle, mov_members.handle, ref_members.handle, UNPACK_STRATEGIES[strategy],
                                                    counts.ctypes.data, None if out is None else out.ctypes.data, 0 if out is None else len(out)),
                      "same_merge_acc_unpack")
        return (counts, out[:int(counts[1])]) if pairs else counts

    def unpack_detail(self, mov_members, ref_members, strategy, detail, groups=None):
        """After finish(): `unpack`'s pairs binned where they are made (same_merge_acc_unpack_detail, csrc/window_unpack_detail.hip) under
        `detail`, a DeviceUnpackDetail of `ref_members`, and `groups`, a DeviceScoreDetail of the moving section whose group codes a pair
        takes from its moving row (None: one group).  -> the call's int64 words by name (`split_unpack_detail`): `counts` -- `unpack`'s
        four --, `confusion` (L, L) over the cell-level label codes, `unlabelled`, `groups` (G + 1, 2: pairs and pairs whose codes agree,
        the last row the pairs of rows without a group), `strict` and `weak` (SCORE_RANKS + 1 each) and `untyped`.  Two waits; no pair
        comes to the host."""
        if strategy not in UNPACK_STRATEGIES:
            raise ValueError(f"strategy must be one of {tuple(UNPACK_STRATEGIES)}, not {strategy!r}")
        n_groups = 1 if groups is None else groups.n_groups
        ctx, out = self.ctx, np.zeros(unpack_detail_words(detail.n_labels, n_groups), np.int64)
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_unpack_detail(self.handle, mov_members.handle, ref_members.handle, UNPACK_STRATEGIES[strategy],
                                                           detail.handle, None if groups is None else groups.handle, out.ctypes.data,
                                                           len(out)), "same_merge_acc_unpack_detail")
        return split_unpack_detail(out, detail.n_labels, n_groups)

    def unpack_features(self, mov_members, ref_members, strategy, features, zone=None, d2=False, pairs=False):
        """After finish(): `unpack`'s pairs read as feature sums where they are made (same_merge_acc_unpack_features,
        csrc/window_unpack_feature.hip) under `features`, a DeviceUnpackFeatures of the two member lists, and `zone`, a DeviceUnpackZone
        of it (None: no distance reading).  -> (`unpack`'s four int64 counts; the feature words cut by `split_score_features`, "final
        row" read as "cell pair"; with `d2` the float64 squared distance to the zone per PAIR, NaN where it is no subset pair, else
        None; with `pairs` per pair the flat index of its reference member, else None) -- the pairs in `unpack`'s order.  A merge names
        a moving row once, so the moving side's member count bounds the pairs: one call."""
        if strategy not in UNPACK_STRATEGIES:
            raise ValueError(f"strategy must be one of {tuple(UNPACK_STRATEGIES)}, not {strategy!r}")
        ctx = self.ctx
        B = 0 if zone is None else zone.n_bins
        out = np.zeros(4 + score_feature_words(features.n_groups, features.n_columns, B), np.int64)
        cap = mov_members.n_members
        dist = np.empty(cap, np.float64) if d2 else None
        ref_member = np.empty(cap, np.int64) if pairs else None
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_unpack_features(self.handle, mov_members.handle, ref_members.handle, UNPACK_STRATEGIES[strategy],
                                                             features.handle, None if zone is None else zone.handle, out.ctypes.data, len(out),
                                                             None if dist is None else dist.ctypes.data,
                                                             None if ref_member is None else ref_member.ctypes.data, cap),
                      "same_merge_acc_unpack_features")
        n = int(out[1])
        return (out[:4], split_score_features(out[4:], features.n_groups, features.n_columns, B), None if dist is None else dist[:n],
                None if ref_member is None else ref_member[:n])

    def unpack_map(self, mov_members, ref_members, strategy, detail, unpack_map, marks=True):
        """After finish(): `unpack`'s counts and, per moving MEMBER, its mark (same_merge_acc_unpack_map, csrc/window_unpack_map.hip) --
        folded into `unpack_map`, a DeviceUnpackMap of the two member lists, whose truth members the marks are read against.  `detail`: a
        DeviceUnpackDetail of `ref_members` whose label columns and type rows rank the members (None: no ranks).  -> (six int64 counts:
        `unpack`'s four, matched members with a known truth, those on it; the marks as a MEMBER_MARK array, or None with marks=False).
        The device's copy of the marks lands in a page-locked block of the map; the array is written from it once the call succeeded.
        No wait beyond `unpack`'s; leaves the accumulator as `unpack` does."""
        if strategy not in UNPACK_STRATEGIES:
            raise ValueError(f"strategy must be one of {tuple(UNPACK_STRATEGIES)}, not {strategy!r}")
        ctx, counts = self.ctx, np.zeros(6, np.int64)
        n = mov_members.n_members
        out = np.empty(n, MEMBER_MARK) if marks else None
        with ctx.lock:
            ctx.check(ctx.lib.same_merge_acc_unpack_map(self.handle, mov_members.handle, ref_members.handle, UNPACK_STRATEGIES[strategy],
                                                        None if detail is None else detail.handle, unpack_map.handle,
                                                        None if out is None or not n else out.ctypes.data, counts.ctypes.data),
                      "same_merge_acc_unpack_map")
        return counts, out

    def columns(self, dmoving, dref, n_final, n_types, extra_moving=(), extra_ref=(), layer=None):
        """After finish(): the merged table's columns written by the device straight into page-locked host memory (enqueue only:
        `ctx.sync()` before reading): the moving section's type columns (`layer`: a DeviceTypesLayer of `dmoving` to read them from), X, Y, the reference's X, Y, the caller's extra 8-byte device
        columns (DeviceBuffers of 8-byte values per moving / reference row: ids, sizes), aligned_idx, window_id and plan position as int64,
        and the two flag columns.  -> (uint64 array (n_types + 4 + extras + 3, n_final), uint8 array (2, n_final)) over a pooled block,
        or None when no block is to be had (the caller gathers on the host)."""
        n8 = n_types + 4 + len(extra_moving) + len(extra_ref) + 3
        got = PINNED_BLOCKS.take(self.ctx, max(1, n8 * 8 * n_final + 2 * n_final)) if n_final else None
        if got is None:
            return None
        buf, ptr = got
        ctx = self.ctx
        em = (ctypes.c_void_p * max(1, len(extra_moving)))(*[b.ptr for b in extra_moving])
        er = (ctypes.c_void_p * max(1, len(extra_ref)))(*[b.ptr for b in extra_ref])
        with ctx.lock:
            if layer is None:
                ctx.check(ctx.lib.same_merge_acc_columns(self.handle, dmoving.handle, dref.handle, em, len(extra_moving), er,
                                                         len(extra_ref), ptr, int(n_final)), "same_merge_acc_columns")
            else:
                ctx.check(ctx.lib.same_merge_acc_columns_layer(self.handle, dmoving.handle, layer.handle, dref.handle, em,
                                                               len(extra_moving), er, len(extra_ref), ptr, int(n_final)),
                          "same_merge_acc_columns_layer")
        wide = np.frombuffer(buf, dtype=np.uint64, count=n8 * n_final).reshape(n8, n_final)
        flags = np.frombuffer(buf, dtype=np.uint8, count=2 * n_final, offset=n8 * 8 * n_final).reshape(2, n_final)
        return wide, flags


def plain_accumulators(accs):
    """The pass is over and its table is wanted WITHOUT the merge: every accumulated row is a row of the table, windows in the order they
    were collected.  -> accs[0], holding the rows (`.n_final`, `.final_rows()`, `.columns(...)`)."""
    ctx = accs[0].ctx
    n = ctypes.c_int64(0)
    handles = (ctypes.c_void_p * len(accs))(*[a.handle.value for a in accs])
    with ctx.lock:
        ctx.check(ctx.lib.same_merge_acc_plain(handles, len(accs), ctypes.byref(n)), "same_merge_acc_plain")
    accs[0].n_final = n.value
    return accs[0]


def resolve_accumulators(accs, dmoving, dref):
    """The pass is over: the accumulators of the worker contexts (in the order their runs of the plan have) -> ((rows, rows after the
    de-duplication, rest rows, rows final already), the REST rows as REST_RECORDs): what the device could not decide alone -- cells some
    window disagrees about, rows at a seam between ranks -- for merge.py's graph step; `accs[0].finish(winners)` completes the merge."""
    ctx = accs[0].ctx
    counts = np.zeros(4, np.int64)
    handles = (ctypes.c_void_p * len(accs))(*[a.handle.value for a in accs])
    with ctx.lock:
        ctx.check(ctx.lib.same_merge_acc_resolve(handles, len(accs), None if dmoving is None else dmoving.handle,
                                                 None if dref is None else dref.handle, counts.ctypes.data), "same_merge_acc_resolve")
        rest = np.empty(int(counts[2]), REST_RECORD)
        ctx.check(ctx.lib.same_merge_acc_fetch(accs[0].handle, 0, rest.ctypes.data, rest.nbytes), "same_merge_acc_fetch")
    return tuple(int(c) for c in counts), rest


WINDOW_BATCH_MAX = 64      # SAME_WINDOW_BATCH_MAX


def _handles(states):
    return (ctypes.c_void_p * len(states))(*[s.handle.value for s in states])


def _staged_anew(states, counts):
    """the states of windows a call left as a stage call leaves them (same_window_stage; same_window_knn_prefix): their counts, a pair
    list that is the list as staged, no triangles, no prune  -> [counts per window]"""
    for s, c in zip(states, counts.tolist()):
        s.counts, s.n_triangles = tuple(c), 0
        s.n_staged_pairs, s.priority = c[3], None
    return [s.counts for s in states]


def _compacted(states, counts):
    """the states of windows a call left without their unconstrained nodes (same_window_caller_tris; same_window_caller_pairs): the
    triangles selected, the kept cells and pairs left  -> [the call's six counts per window]"""
    out = []
    for s, c in zip(states, counts.tolist()):
        s.n_selected, s.n_triangles = c[0], 0
        s.counts = (s.counts[0], s.counts[1], c[3], c[4])
        out.append(tuple(c))
    return out


def stage_windows(states, moving, ref, boxes, radius, knn, dist_ct_coeff):
    """same_window_stage for a batch of windows of one context (one wait for all of them).  -> [counts per window]"""
    ctx, n = states[0].ctx, len(states)
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(n, 4)
    counts = np.zeros((n, 4), np.int64)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_stage(_handles(states), n, moving.handle, ref.handle, boxes.ctypes.data, float(radius), int(knn),
                                            float(dist_ct_coeff), counts.ctypes.data), "same_window_stage")
    for s in states:
        s.n_selected = 0
    return _staged_anew(states, counts)


def priority_windows(states):
    """same_window_priority_pairs for a batch of staged windows of one context (one wait): the cell-type-priority prune of every window's
    pair list (src/knn_utils.py:28-78; csrc/window_priority.hip).  -> [(pairs staged, pairs left, rows that kept one pair, rows that kept
    all) per window]; every state's pair count -- and _W_PAIRS, _W_COSTS -- are the filtered list's afterwards, _W_STAGED_PAIRS stays the
    list as staged.  The kept aligned cells do not change."""
    ctx, n = states[0].ctx, len(states)
    counts = ops.window_priority_pairs(ctx, _handles(states), n)
    out = []
    for s, c in zip(states, counts.tolist()):
        if s.counts[3]:
            s.counts = (s.counts[0], s.counts[1], s.counts[2], c[1])
        s.priority = tuple(c)
        out.append(s.priority)
    return out


def prefix_windows(states, k):
    """same_window_knn_prefix for a batch of staged windows of one context (one wait): every window's pair list cut to each row's first
    min(k, count) pairs (csrc/window_knn_prefix.hip) -- the window a stage call at `k` leaves, derived from the list as staged instead
    of staged again.  k at most the knn the windows were staged at (that value turns them back to the staged list); values may come in
    any order.  -> [counts per window]; every state's pair count -- and _W_PAIRS, _W_COSTS, _W_STAGED_PAIRS -- are the shorter list's
    afterwards, an earlier priority prune's result is gone.  The kept aligned cells, and a triangulation made for them, do not change."""
    ctx, n = states[0].ctx, len(states)
    counts = np.zeros((n, 4), np.int64)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_knn_prefix(_handles(states), n, int(k), counts.ctypes.data), "same_window_knn_prefix")
    return _staged_anew(states, counts)


def recost_windows(states, dmoving, dref, layer, dist_ct_coeff):
    """same_window_recost for a batch of staged windows of one context (one wait): the costs of every window's pair list AS STAGED written
    again with the moving rows' types read from `layer` (a DeviceTypesLayer of `dmoving`; None: the section's own) -- bit for bit the
    costs a stage call over a moving section made with that matrix computes (csrc/window_recost.hip).  `dmoving`, `dref`, `dist_ct_coeff`:
    what the windows were staged with.  Every window is afterwards what `prefix_windows` at the staged knn leaves: the list as staged, no
    priority prune, a caller's compaction turned back and held for `caller_pairs_windows`.  -> [counts per window]"""
    ctx, n = states[0].ctx, len(states)
    counts = np.zeros((n, 4), np.int64)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_recost(_handles(states), n, dmoving.handle, dref.handle, None if layer is None else layer.handle,
                                             float(dist_ct_coeff), counts.ctypes.data), "same_window_recost")
    return _staged_anew(states, counts)


class DeviceCallerTris(_DeviceHandle):
    """A caller's triangulation of a moving section resident on the device (same_caller_tris_create, csrc/window_caller.hip): `rows`
    int32 (Tr, 3) section rows in the caller's order (window_api.caller_triangulation_rows), uploaded once and binned by the grid the
    section has NOW -- bin the section on the window grid first.  Read-only: the worker contexts of the device share it."""

    _ENTRY = ("same_caller_tris_create", "same_caller_tris_destroy")

    def __init__(self, dsection, rows, ctx=None):
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
        self.n_triangles = len(rows)
        self._create(ctx, dsection.handle, rows.ctypes.data if len(rows) else None, len(rows))


class DeviceMembers(_DeviceHandle):
    """The members of a section's rows resident on the device (same_members_create, csrc/window_unpack.hip): `off` int64 (rows + 1) CSR
    offsets, `xy` float64 (m, 2) the members' ORIGINAL cells' coordinates, `codes` int32 (m) their joint label codes (negative: equals
    nothing).  Made on the section's context; read-only: the worker contexts of the device share it.  Close it before its section."""

    _ENTRY = (None, "same_members_destroy")

    def __init__(self, dsection, off, xy, codes):
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if len(xy) != len(codes):
            raise ValueError(f"{len(xy)} member coordinates, {len(codes)} member codes")
        if len(self.off) != len(dsection.section.xy) + 1:       # (the library reads off[rows]: nothing it was not given)
            raise ValueError(f"{len(self.off)} offsets for a section of {len(dsection.section.xy)} rows")
        self.n_members = len(codes)
        self.ctx = ctx = dsection.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_members_create(dsection.handle, self.off.ctypes.data, xy.ctypes.data if len(xy) else None,
                                             codes.ctypes.data if len(codes) else None, len(codes), ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_members_destroy(h)
            ctx.check(rc, "same_members_create")
        self.handle = h


SCORE_RANKS = _lib.SAME_SCORE_RANKS


def score_detail_words(n_labels, n_groups):
    """int64 words of same_merge_acc_score_detail's `out` (SAME_SCORE_DETAIL_WORDS)"""
    return n_labels * n_labels + 1 + (n_groups + 1) * 8 + 2 * (SCORE_RANKS + 1) + 1


def split_score_detail(out, n_labels, n_groups):
    """the words of same_merge_acc_score_detail's `out` by name, in the order include/same_hip.h states"""
    L, G, R = int(n_labels), int(n_groups), SCORE_RANKS
    out = np.asarray(out, np.int64)
    assert len(out) >= score_detail_words(L, G)
    at = np.cumsum([0, L * L, 1, (G + 1) * 8, R + 1, R + 1, 1])
    part = lambda q: out[at[q]:at[q + 1]]
    return {"confusion": part(0).reshape(L, L), "unlabelled": int(part(1)[0]), "groups": part(2).reshape(G + 1, 8), "strict": part(3),
            "weak": part(4), "untyped": int(part(5)[0])}


class DeviceScoreDetail(_DeviceHandle):
    """What same_merge_acc_score_detail bins by, resident beside a moving section (same_score_detail_create,
    csrc/window_score_detail.hip): `group_of` int32 per section row (negative: no group; None: every row in group 0) over `n_groups`
    groups, `col_of_label` int32 per joint label code, the type column the label names or -1 (None: no rank counts), `n_labels` codes.
    Made on the section's context; read-only: the worker contexts of the device share it.  Close it before its section."""

    _ENTRY = (None, "same_score_detail_destroy")

    def __init__(self, dsection, group_of, n_groups, n_labels, col_of_label):
        g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.int32)
        c = None if col_of_label is None else np.ascontiguousarray(col_of_label, dtype=np.int32)
        if g is not None and g.shape != (len(dsection.section.xy),):        # (the library reads one entry per row: nothing it was not given)
            raise ValueError(f"group_of has shape {g.shape} for a section of {len(dsection.section.xy)} rows")
        if c is not None and c.shape != (max(int(n_labels), 0),):
            raise ValueError(f"col_of_label has shape {c.shape} for {n_labels} labels")
        self.n_groups, self.n_labels = int(n_groups), int(n_labels)
        self.ctx = ctx = dsection.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_score_detail_create(dsection.handle, None if g is None or not len(g) else g.ctypes.data, self.n_groups,
                                                  self.n_labels, None if c is None or not len(c) else c.ctypes.data, ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_score_detail_destroy(h)
            ctx.check(rc, "same_score_detail_create")
        self.handle = h
        self.n_words = score_detail_words(self.n_labels, self.n_groups)

    def split(self, out):
        return split_score_detail(out, self.n_labels, self.n_groups)


# same_cell_mark (include/same_hip.h): one record per row of the moving section
CELL_MARK = np.dtype([("ref_row", np.int32), ("node_tri", np.uint32), ("node_flip", np.uint32), ("flags", np.uint8),
                      ("rank_strict", np.uint8), ("rank_weak", np.uint8), ("reserved", np.uint8)])
assert CELL_MARK.itemsize == 16
TALLY_COLUMNS = ("matched_in", "type_match_in", "violating_in", "on_truth_in")


class DeviceScoreMap(_DeviceHandle):
    """What same_merge_acc_score_map reads its marks against and folds them into, resident beside the two sections
    (same_score_map_create, csrc/window_score_map.hip): `truth_row` int32 per moving section row, the reference section row that is its
    true or baseline match, -1 unknown (None: every row unknown); with `tally` four uint32 counters per moving row over the results
    folded in.  The worker contexts of the device share it.  Close it before its sections."""

    _ENTRY = ("same_score_map_create", "same_score_map_destroy")

    def __init__(self, dmoving, dref, truth_row=None, tally=True, ctx=None):
        t = None if truth_row is None else np.ascontiguousarray(truth_row, dtype=np.int32)
        self.n_rows = len(dmoving.section.xy)
        if t is not None and t.shape != (self.n_rows,):             # (the library reads one entry per row: nothing it was not given)
            raise ValueError(f"truth_row has shape {t.shape} for a moving section of {self.n_rows} rows")
        self.has_tally = bool(tally)
        self._create(dmoving.ctx if ctx is None else ctx, dmoving.handle, dref.handle, None if t is None or not len(t) else t.ctypes.data,
                     int(self.has_tally))

    def tally(self):
        """-> (uint32 (rows, 4) over TALLY_COLUMNS, or None for a map without a tally; the results folded in since the creation or the
        last `reset`)"""
        ctx = self.ctx
        out = np.zeros((self.n_rows, 4), np.uint32) if self.has_tally else None
        n = ctypes.c_int64(0)
        with ctx.lock:
            ctx.check(ctx.lib.same_score_map_tally(self.handle, None if out is None or not len(out) else out.ctypes.data, ctypes.byref(n)),
                      "same_score_map_tally")
        return out, n.value

    def reset(self):
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_score_map_reset(self.handle), "same_score_map_reset")


def score_feature_words(n_groups, n_columns, n_bins=0):
    """int64 words of same_merge_acc_score_features' `out` (SAME_FEATURE_WORDS); n_bins: the zone's distance bins, 0 without a zone"""
    return 4 + (n_groups + 1) * (1 + n_columns) + ((n_bins + 1) * (1 + n_columns) if n_bins > 0 else 0)


def split_score_features(out, n_groups, n_columns, n_bins=0):
    """the words of same_merge_acc_score_features' `out` by name, in the order include/same_hip.h states: `counts` (4), `rows` (G + 1),
    `sums` (G + 1, F) and with a zone `bin_rows` (B + 1), `bin_sums` (B + 1, F)"""
    G, F, B = int(n_groups), int(n_columns), int(n_bins)
    out = np.asarray(out, np.int64)
    assert len(out) >= score_feature_words(G, F, B)
    at = np.cumsum([0, 4, G + 1, (G + 1) * F] + ([B + 1, (B + 1) * F] if B > 0 else []))
    part = lambda q: out[at[q]:at[q + 1]]
    got = {"counts": part(0), "rows": part(1), "sums": part(2).reshape(G + 1, F)}
    if B > 0:
        got.update(bin_rows=part(3), bin_sums=part(4).reshape(B + 1, F))
    return got


class DeviceScoreFeatures(_DeviceHandle):
    """What same_merge_acc_score_features sums, resident beside the two sections (same_score_features_create,
    csrc/window_score_feature.hip): `mov_q` int32 (moving rows, F_m) and `ref_q` int32 (reference rows, F_r), the fixed-point feature
    columns (|q| <= 2**30; None: the side has no column), `group_of` / `n_groups` as DeviceScoreDetail's.  Made on the moving section's
    context; read-only: the worker contexts of the device share it.  Close it before its sections."""

    _ENTRY = (None, "same_score_features_destroy")

    def __init__(self, dmoving, dref, mov_q, ref_q, group_of, n_groups):
        n_m, n_r = len(dmoving.section.xy), len(dref.section.xy)
        side = lambda q, n: np.zeros((n, 0), np.int32) if q is None else np.ascontiguousarray(q, dtype=np.int32)
        mq, rq = side(mov_q, n_m), side(ref_q, n_r)
        for q, n, name in ((mq, n_m, "mov_q"), (rq, n_r, "ref_q")):       # (the library reads rows x columns: nothing it was not given)
            if q.ndim != 2 or q.shape[0] != n:
                raise ValueError(f"{name} has shape {q.shape} for a section of {n} rows")
        g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.int32)
        if g is not None and g.shape != (n_m,):
            raise ValueError(f"group_of has shape {g.shape} for a section of {n_m} rows")
        self.F_m, self.F_r, self.n_groups = mq.shape[1], rq.shape[1], int(n_groups)
        self.n_columns, self.n_rows, self.n_ref_rows = self.F_m + self.F_r, n_m, n_r
        self.ctx = ctx = dmoving.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_score_features_create(dmoving.handle, dref.handle, mq.ctypes.data if mq.size else None, self.F_m,
                                                    rq.ctypes.data if rq.size else None, self.F_r,
                                                    None if g is None or not len(g) else g.ctypes.data, self.n_groups, ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_score_features_destroy(h)
            ctx.check(rc, "same_score_features_create")
        self.handle = h


class DeviceFeatureZone(_DeviceHandle):
    """The zone and the subset of a distance reading, resident beside a DeviceScoreFeatures (same_feature_zone_create): `mov_flags`,
    `ref_flags` uint8 per section row, bit 0 "zone side", bit 1 "subset side" (None: every bit set); `d2_edges` the thresholds on the
    SQUARED distance, non-decreasing, 2 .. 65 of them.  Close it before its features."""

    _ENTRY = (None, "same_feature_zone_destroy")

    def __init__(self, features, mov_flags, ref_flags, d2_edges):
        flags = lambda f: None if f is None else np.ascontiguousarray(f, dtype=np.uint8)
        mf, rf = flags(mov_flags), flags(ref_flags)
        for f, n, name in ((mf, features.n_rows, "mov_flags"), (rf, features.n_ref_rows, "ref_flags")):
            if f is not None and f.shape != (n,):                         # (the library reads one entry per row: nothing it was not given)
                raise ValueError(f"{name} has shape {f.shape} for a section of {n} rows")
        e = np.ascontiguousarray(d2_edges, dtype=np.float64).reshape(-1)
        self.features, self.n_bins = features, len(e) - 1
        self.ctx = ctx = features.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_feature_zone_create(features.handle, None if mf is None or not len(mf) else mf.ctypes.data,
                                                  None if rf is None or not len(rf) else rf.ctypes.data, e.ctypes.data if len(e) else None,
                                                  len(e), ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_feature_zone_destroy(h)
            ctx.check(rc, "same_feature_zone_create")
        self.handle = h


UNPACK_STRATEGIES = {"distribute": _lib.SAME_UNPACK_DISTRIBUTE, "nearest": _lib.SAME_UNPACK_NEAREST}


def unpack_detail_words(n_labels, n_groups):
    """int64 words of same_merge_acc_unpack_detail's `out` (SAME_UNPACK_DETAIL_WORDS)"""
    return 4 + n_labels * n_labels + 1 + (n_groups + 1) * 2 + 2 * (SCORE_RANKS + 1) + 1


def split_unpack_detail(out, n_labels, n_groups):
    """the words of same_merge_acc_unpack_detail's `out` by name, in the order include/same_hip.h states"""
    L, G, R = int(n_labels), int(n_groups), SCORE_RANKS
    out = np.asarray(out, np.int64)
    assert len(out) >= unpack_detail_words(L, G)
    at = np.cumsum([0, 4, L * L, 1, (G + 1) * 2, R + 1, R + 1, 1])
    part = lambda q: out[at[q]:at[q + 1]]
    return {"counts": part(0), "confusion": part(1).reshape(L, L), "unlabelled": int(part(2)[0]), "groups": part(3).reshape(G + 1, 2),
            "strict": part(4), "weak": part(5), "untyped": int(part(6)[0])}


class DeviceUnpackFeatures(_DeviceHandle):
    """What same_merge_acc_unpack_features sums, resident beside the two member lists (same_unpack_features_create,
    csrc/window_unpack_feature.hip): `mov_q` int32 (moving members, F_m) and `ref_q` int32 (reference members, F_r), one fixed-point
    feature row per MEMBER in CSR order (|q| <= 2**30; None: the side has no column); `member_group` int32 per moving member, the group
    of the moving CELL (negative: none; None: every cell in group 0) over `n_groups` groups.  Made on the moving members' context;
    read-only: the worker contexts of the device share it.  Close it before its members."""

    _ENTRY = (None, "same_unpack_features_destroy")

    def __init__(self, mov_members, ref_members, mov_q, ref_q, member_group, n_groups):
        n_m, n_r = mov_members.n_members, ref_members.n_members
        side = lambda q, n: np.zeros((n, 0), np.int32) if q is None else np.ascontiguousarray(q, dtype=np.int32)
        mq, rq = side(mov_q, n_m), side(ref_q, n_r)
        for q, n, name in ((mq, n_m, "mov_q"), (rq, n_r, "ref_q")):       # (the library reads members x columns: nothing it was not given)
            if q.ndim != 2 or q.shape[0] != n:
                raise ValueError(f"{name} has shape {q.shape} for {n} members")
        g = None if member_group is None else np.ascontiguousarray(member_group, dtype=np.int32)
        if g is not None and g.shape != (n_m,):
            raise ValueError(f"member_group has shape {g.shape} for {n_m} moving members")
        self.F_m, self.F_r, self.n_groups = mq.shape[1], rq.shape[1], int(n_groups)
        self.n_columns, self.n_rows, self.n_ref_rows = self.F_m + self.F_r, n_m, n_r
        self.ctx = ctx = mov_members.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_unpack_features_create(mov_members.handle, ref_members.handle, mq.ctypes.data if mq.size else None, self.F_m,
                                                     rq.ctypes.data if rq.size else None, self.F_r,
                                                     None if g is None or not len(g) else g.ctypes.data, self.n_groups, ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_unpack_features_destroy(h)
            ctx.check(rc, "same_unpack_features_create")
        self.handle = h


class DeviceUnpackZone(_DeviceHandle):
    """The zone and the subset of a cell-level distance reading, resident beside a DeviceUnpackFeatures (same_unpack_zone_create):
    `mov_flags`, `ref_flags` uint8 per MEMBER, bit 0 "zone side", bit 1 "subset side" (None: every bit set); `d2_edges` the thresholds
    on the SQUARED distance, non-decreasing, 2 .. 65 of them.  Close it before its features."""

    _ENTRY = (None, "same_unpack_zone_destroy")

    def __init__(self, features, mov_flags, ref_flags, d2_edges):
        flags = lambda f: None if f is None else np.ascontiguousarray(f, dtype=np.uint8)
        mf, rf = flags(mov_flags), flags(ref_flags)
        for f, n, name in ((mf, features.n_rows, "mov_flags"), (rf, features.n_ref_rows, "ref_flags")):
            if f is not None and f.shape != (n,):                         # (the library reads one entry per member: nothing it was not given)
                raise ValueError(f"{name} has shape {f.shape} for {n} members")
        e = np.ascontiguousarray(d2_edges, dtype=np.float64).reshape(-1)
        self.features, self.n_bins = features, len(e) - 1
        self.ctx = ctx = features.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_unpack_zone_create(features.handle, None if mf is None or not len(mf) else mf.ctypes.data,
                                                 None if rf is None or not len(rf) else rf.ctypes.data, e.ctypes.data if len(e) else None,
                                                 len(e), ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_unpack_zone_destroy(h)
            ctx.check(rc, "same_unpack_zone_create")
        self.handle = h


class DeviceUnpackDetail(_DeviceHandle):
    """What same_merge_acc_unpack_detail bins cell pairs by, resident beside the reference members (same_unpack_detail_create,
    csrc/window_unpack_detail.hip): `n_labels` cell-level joint label codes -- the codes the members were uploaded with --,
    `col_of_label` int32 per code, the type column the label names or -1 (None: no rank counts), `member_types` float64 (members, T),
    one type row per reference member in CSR order (None: none).  Made on the members' context; read-only: the worker contexts of the
    device share it.  Close it before its members."""

    _ENTRY = (None, "same_unpack_detail_destroy")

    def __init__(self, ref_members, n_labels, col_of_label, member_types):
        c = None if col_of_label is None else np.ascontiguousarray(col_of_label, dtype=np.int32)
        t = None if member_types is None else np.ascontiguousarray(member_types, dtype=np.float64)
        if c is not None and c.shape != (max(int(n_labels), 0),):            # (the library reads one entry per label: nothing it was not given)
            raise ValueError(f"col_of_label has shape {c.shape} for {n_labels} labels")
        if t is not None and (t.ndim != 2 or len(t) != ref_members.n_members):
            raise ValueError(f"member_types has shape {t.shape} for {ref_members.n_members} reference members")
        self.n_labels, self.n_types = int(n_labels), 0 if t is None else t.shape[1]
        self.ctx = ctx = ref_members.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_unpack_detail_create(ref_members.handle, self.n_labels, None if c is None or not len(c) else c.ctypes.data,
                                                   None if t is None else t.ctypes.data, self.n_types, ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_unpack_detail_destroy(h)
            ctx.check(rc, "same_unpack_detail_create")
        self.handle = h


# same_member_mark (include/same_hip.h): one record per moving member
MEMBER_MARK = np.dtype([("ref_member", np.int32), ("ref_row", np.int32), ("pair", np.int32), ("flags", np.uint8),
                        ("rank_strict", np.uint8), ("rank_weak", np.uint8), ("reserved", np.uint8)])
assert MEMBER_MARK.itemsize == 16
MEMBER_TALLY_COLUMNS = ("matched_in", "type_match_in", "on_truth_in")


class DeviceUnpackMap(_DeviceHandle):
    """What same_merge_acc_unpack_map reads its marks against and folds them into, resident beside the two member lists
    (same_unpack_map_create, csrc/window_unpack_map.hip): `truth_member` int32 per moving member, the flat reference member that is its
    true or baseline partner, -1 unknown (None: every member unknown); with `with_tally` three uint32 counters per moving member over
    the results folded in.  Made on the moving members' context; the worker contexts of the device share it.  Close it before its
    members."""

    _ENTRY = (None, "same_unpack_map_destroy")

    def __init__(self, moving_members, ref_members, truth_member=None, with_tally=True):
        t = None if truth_member is None else np.ascontiguousarray(truth_member, dtype=np.int32)
        self.n_members = moving_members.n_members
        if t is not None and t.shape != (self.n_members,):          # (the library reads one entry per member: nothing it was not given)
            raise ValueError(f"truth_member has shape {t.shape} for {self.n_members} moving members")
        self.has_tally = bool(with_tally)
        self.ctx = ctx = moving_members.ctx
        h = ctypes.c_void_p()
        with ctx.lock:
            rc = ctx.lib.same_unpack_map_create(moving_members.handle, ref_members.handle, None if t is None or not len(t) else t.ctypes.data,
                                                int(self.has_tally), ctypes.byref(h))
            if rc != 0 and h.value:
                ctx.lib.same_unpack_map_destroy(h)
            ctx.check(rc, "same_unpack_map_create")
        self.handle = h

    def tally(self):
        """-> (uint32 (members, 3) over MEMBER_TALLY_COLUMNS, or None for a map without a tally; the results folded in since the creation
        or the last `reset`)"""
        ctx = self.ctx
        out = np.zeros((self.n_members, 3), np.uint32) if self.has_tally else None
        n = ctypes.c_int64(0)
        with ctx.lock:
            ctx.check(ctx.lib.same_unpack_map_tally(self.handle, None if out is None or not len(out) else out.ctypes.data, ctypes.byref(n)),
                      "same_unpack_map_tally")
        return out, n.value

    def reset(self):
        with self.ctx.lock:
            self.ctx.check(self.ctx.lib.same_unpack_map_reset(self.handle), "same_unpack_map_reset")


def caller_tris_windows(states, caller, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, removed=None):
    """same_window_caller_tris for a batch of staged windows of one context (one wait): the caller's triangles of every window over its
    kept cells, the filter's node mask, and the window without its unconstrained nodes (src/same.py:1016-1085).  `removed`: per window a
    uint8 mask over its kept cells AS STAGED (the prefiltered form: the host filtered).  -> [(selected, removed, near, kept cells left,
    pairs left, triangles left) per window]; every state's counts are the smaller window's afterwards, unless its near is not 0."""
    ctx, n = states[0].ctx, len(states)
    counts = np.zeros((n, 6), np.int64)
    flat = offsets = None
    if removed is not None:
        masks = [np.ascontiguousarray(m, dtype=np.uint8) for m in removed]
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum([len(m) for m in masks], out=offsets[1:])
        flat = np.concatenate(masks) if masks else np.zeros(0, np.uint8)
        if len(flat) == 0:
            flat = np.zeros(1, np.uint8)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_caller_tris(_handles(states), n, caller.handle, _lib._ptr(flat), _lib._ptr(offsets), float(radius),
                                                  int(angle_enabled), float(cos_thr), float(near_tol), int(bool(ignore_same_type)),
                                                  counts.ctypes.data), "same_window_caller_tris")
    return _compacted(states, counts)


def caller_pairs_windows(states):
    """same_window_caller_pairs for a batch of windows of one context (one wait): every window `caller_tris_windows` compacted and
    `prefix_windows` [+ `priority_windows`] has since cut gets its CURRENT pair list pushed through the node mask it holds
    (csrc/window_caller.hip) -- the aligned side and the triangles are not made again.  -> [(selected, removed, 0, kept cells left, pairs
    left, triangles left) per window], as caller_tris_windows reports them; every state's counts are the smaller window's afterwards:
    the window is the one stage at that knn [+ prune] + caller_tris_windows leaves."""
    ctx, n = states[0].ctx, len(states)
    counts = np.zeros((n, 6), np.int64)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_caller_pairs(_handles(states), n, counts.ctypes.data), "same_window_caller_pairs")
    return _compacted(states, counts)


def _window_records(stats_words, mode):
    """WindowMode.records of a FINISH call's stats words (a re-finish's are narrower: `mode.records(s, start=False)`)"""
    return mode.records(stats_words)


def filter_finish_windows(states, simplices, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, no_match_penalty,
                          ensure_min_triangle_per_node=True, prefiltered=False, mode=None, from_caller=False):
    """same_window_filter_finish for a batch (one wait for all of them): `simplices[i]` are window i's Delaunay simplices, or with
    `prefiltered` its kept triangles; `simplices=None` takes the candidates `triangulate_windows` left on the device for every window
    (each state must have been answered since it was staged), or with `from_caller` the triangles `caller_tris_windows` left.
    `mode`: a WindowMode -- the start, the search on it and the model's reference capacities (None: the greedy start alone); one with a capacity goes through same_window_filter_finish_cap.
    -> [(kept, added back, near, match_row, flag byte, stats dict) per window]; a window with near != 0 has None for the last three.
    Every state's `order_ties` is set to the call's count of places where the answer hangs on the ORDER of the triangles or of their
    corners (include/same_hip.h; of consequence only when the simplices are not Qhull's own), its `assignment` and `refine` to the
    call's records of the two (_window_records; None when off)."""
    mode = WindowMode.default() if mode is None else mode
    ctx, n = states[0].ctx, len(states)
    if simplices is None:
        source, flat, offsets = _lib.SAME_TRIS_CALLER if from_caller else _lib.SAME_TRIS_DEVICE, None, None
    else:
        source = _lib.SAME_TRIS_KEPT if prefiltered else _lib.SAME_TRIS_SIMPLICES
        tris = [ops._tris(t) for t in simplices]
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum([len(t) for t in tris], out=offsets[1:])
        flat = tris[0] if n == 1 else np.concatenate(tris)
    capacity = mode.c_capacity()
    kept_cells = [s.counts[2] for s in states]
    cell_off = np.concatenate(([0], np.cumsum(kept_cells))).astype(np.int64)
    match_row, flag = np.empty(int(cell_off[-1]), np.int32), np.empty(int(cell_off[-1]), np.uint8)
    stats, counts = np.zeros((n, mode.finish_width), np.int64), np.zeros((n, 4), np.int64)
    args = (_handles(states), n, source, _lib._ptr(flat), _lib._ptr(offsets), float(radius), int(angle_enabled), float(cos_thr),
            float(near_tol), int(bool(ignore_same_type)), int(bool(ensure_min_triangle_per_node)), float(no_match_penalty),
            mode.incumbent_code, *mode.search_args)
    outs = (match_row.ctypes.data, flag.ctypes.data, stats.ctypes.data, counts.ctypes.data)
    with ctx.lock:
        if capacity is None:
            ctx.check(ctx.lib.same_window_filter_finish(*args, *outs), "same_window_filter_finish")
        else:
            ctx.check(ctx.lib.same_window_filter_finish_cap(*args, ctypes.byref(capacity), *outs), "same_window_filter_finish_cap")
    out = []
    for i, s in enumerate(states):
        kept, added, near, s.order_ties = (int(c) for c in counts[i])
        s.n_triangles = 0 if near else kept + added
        s.assignment, s.refine = _window_records(stats[i], mode)
        if near:
            out.append((kept, added, near, None, None, None))
        else:
            a, b = int(cell_off[i]), int(cell_off[i + 1])
            out.append((kept, added, near, match_row[a:b], flag[a:b], dict(zip(DeviceWindow.STAT_NAMES, stats[i, :8].tolist()))))
    return out


def triangulate_windows(states, radius, angle_enabled, cos_thr, guard):
    """same_window_delaunay for a batch of staged windows (one wait): -> (status per window: 0 answered, else a mask of
    _lib.SAME_DD_* reasons; candidate triangles per window); the candidates stay on the device for filter_finish_windows(states, None, ...)"""
    ctx, n = states[0].ctx, len(states)
    status, n_tris = np.zeros(n, np.int32), np.zeros(n, np.int64)
    with ctx.lock:
        ctx.check(ctx.lib.same_window_delaunay(_handles(states), n, float(abs(radius)), int(angle_enabled), float(cos_thr), float(guard),
                                               status.ctypes.data, n_tris.ctypes.data), "same_window_delaunay")
    return status, n_tris


def window_ref_limits(ref_size, pairs, capacity):
    """The model's match limit of every reference row of a window (src/helpers.py:102-161 as csrc/refine.hip's limits kernel reads it):
    `ref_size` the sizes of the window's reference rows, the frame = the references its `pairs` name; (max_matches, multiplier or None,
    penalty_coeff) -> int32 limits, at most 1001"""
    mm, mult, _pc = capacity
    ref_size = np.asarray(ref_size, dtype=np.float64)
    frame = ref_size[np.unique(np.asarray(pairs).reshape(-1, 2)[:, 1])]
    any_meta = bool((frame > 1).any())
    if mult is None:
        mult = int(frame.max()) if len(frame) else 0
    big, plain = min(int(mult) * int(mm), ops.MAX_REF_LIMIT), min(int(mm), ops.MAX_REF_LIMIT)
    return np.where(any_meta & (ref_size > 1), big, plain).astype(np.int32)


def _assignment_fallback(state, out, moving, no_match_penalty, mode, ref=None):
    """a window whose assignment the device's certificate refused: solved by scipy's sparse solver and finished again under that
    matching (counted as a fallback) -> (match_row, flag byte, stats dict); greedy_rounds stays the device's searches.  The transport
    start of `mode`: the host solves the transport problem within the window's limits (sizes from the section `ref`)."""
    from ._trace import stage as marked

    with marked("assignment fallback (host)"):
        pairs, costs = state.fetch(_W_PAIRS), state.fetch(_W_COSTS)
        unmatched = float(no_match_penalty) * moving.size[out.rows_m].astype(np.float64)
        if mode.incumbent != "transport":
            mp = ops.sparse_assign_host(pairs, costs, unmatched, len(unmatched), out.counts[1])
            record = dict(objective=ops.assign_objective(mp, costs, unmatched), fallback=1)
        else:
            # (the limits' frame is the prune's: the references the pair list named as staged, whatever the caller's triangulation removed)
            limits = window_ref_limits(ref.size[state.fetch(_W_ROWS_R)], state.fetch(_W_STAGED_PAIRS), mode.capacity)
            mp = ops.sparse_transport_host(pairs, costs, unmatched, len(unmatched), out.counts[1], limits, mode.capacity[2])
            obj, extra = ops.transport_objective(mp, pairs, costs, unmatched, out.counts[1], mode.capacity[2], with_extra=True)
            record = dict(objective=obj, ref_extra_matches_start=extra, fallback=1)
        match_row, cell_flags, stats = state.refinish(mp, no_match_penalty, mode)
        stats["greedy_rounds"] = out.assignment["rounds"]
        out.assignment.update(record)
    return match_row, cell_flags, stats


class DeviceWindowResult:
    """What one window of `iter_device_windows` leaves on the host: `rows_m` section rows of the kept aligned cells, `axy` their XY,
    `triangles` the kept Delaunay triangles over them (None unless asked for or filtered on the host; `n_triangles` always),
    `match_row` the section row of each cell's matched reference cell (-1 = none), `point_flag` the XY-order sweep's per-cell flag,
    `flip_flag` 1 for the vertices of triangles whose signed area flips, `stats` the sweeps' counters, `counts` (aligned in box, refs in
    box, kept, pairs); `state` is the live DeviceWindow until the generator is asked for the first window of the next batch (pairs,
    costs, signs ... through `state.fetch`).  `mode`: the WindowMode the window was finished under.  `assignment` (a start other than
    greedy only): {"objective", "fallback", "rounds"[, "ref_extra_matches_start"]}.  `refine` (with a search only): the search's record
    of the window's final finish ({"rounds", "moves", "settled", "objective_start", "objective"[, "ref_extra_matches"]}).
    With a caller's triangulation: `removed` the number of unconstrained nodes that went (everything above describes the window without
    them); `skipped` true for a window left without pairs, which contributes nothing (no error, nothing else set).
    With the priority prune on the device: `priority` = (pairs staged, pairs left, rows that kept one pair, rows that kept all); `counts`
    and everything later describe the filtered pair list.
    With `sets` (a parameter sweep): `set` = the index of the parameter set this result was finished under; `mode`, `counts`, `priority`
    and everything the finish call leaves are that set's, `rows_m` / `axy` are shared by the window's results; `variant` = the index of
    the set's type-matrix variant (`variants`; 0 without them)."""

    __slots__ = ("window", "error", "rows_m", "axy", "triangles", "n_triangles", "match_row", "point_flag", "flip_flag", "stats",
                 "counts", "state", "assignment", "refine", "mode", "skipped", "removed", "priority", "set", "variant")

    def __init__(self, window, mode=None):
        self.window = window
        for name in self.__slots__[1:]:
            setattr(self, name, None)
        self.mode = mode


class _StagedWindow:
    """What a batch's stage step of `iter_device_windows` leaves of one window, shared by the window's results: `window`; `error` (no
    pairs) or `skipped` / `removed` (a caller's triangulation); `rows_m`, `axy`; `triangles` a caller's, where the host filtered them;
    `state` and `ticket` of a window that goes on to the finish calls, else None and `counts`, `priority` what the stage step left."""

    __slots__ = ("window", "error", "skipped", "removed", "rows_m", "axy", "triangles", "counts", "priority", "state", "ticket")

    def __init__(self, window):
        self.window = window
        for name in self.__slots__[1:]:
            setattr(self, name, None)


class TriangulationCache(QhullTriangulator):
    """Delaunay simplices remembered per window (a DIAGNOSTIC: bench.py's "what would a pass cost if the triangulations were free").
    `submit(points, key)` hands back the simplices of `key` when it has seen the window before, else asks the helper pool and keeps
    the answer; the simplices are the pool's, i.e. scipy's, either way."""

    def __init__(self):
        self.known = {}

    @staticmethod
    def _tag(points, key):
        """What an entry is remembered under: the window's id AND its points (count + a checksum of the coordinates' bits), so that a
        cache reused with another plan or section whose windows reuse ids asks the pool again instead of answering with stale simplices."""
        p = np.ascontiguousarray(points, dtype=np.float64)
        return key, len(p), int(np.bitwise_xor.reduce(p.view(np.uint64).ravel())) if len(p) else 0

    def submit(self, points, key=None):
        from . import qhull_pool

        tag = None if key is None else self._tag(points, key)       # a window without an id cannot be remembered
        if tag in self.known:
            return Ticket(self, points, simplices=self.known[tag])
        return Ticket(self, points, pending=qhull_pool.pool().submit(points), key=tag)

    def _answered(self, ticket, simplices):
        if ticket.key is not None:
            self.known[ticket.key] = simplices
        return simplices, False


def batch_schedule(sets, layered, priority, caller):
    """THE ORDER OF A BATCH'S CALLS in `iter_device_windows`, as data: the steps a batch makes after its front calls (the stage call,
    [the priority prune], [`caller_tris_windows`], the tickets), a flat list of
        ("recost", v)  ("prefix", k)  ("priority",)  ("caller_pairs",)  ("finish", set index)
    -- `recost_windows` from variant v's layer, `prefix_windows` at k, `priority_windows`, `caller_pairs_windows`, and the filter +
    finish call of one set.  `sets`: the sets, of which only the first entry (knn) and the last (variant index) are read; `layered[v]`:
    variant v is a DeviceTypesLayer, not None (the section's own types); `priority`, `caller`: the prune is on, there is a caller's
    triangulation.  Needs no device and no library.
    The rule.  The front calls leave every window's pair list AT the staged knn (the largest of the sets), priced with the section's own
    types, pruned and pushed through the caller's node masks.  The variants that have sets are the outermost loop, None variants first
    -- that list is already theirs -- then by index.  A layered variant begins with ONE `recost`, which leaves the list at the staged
    knn, unpruned and uncompacted.  Within a variant the distinct knn come largest first, and ONE `prefix` stands where a group's knn
    is not the one the list is at (a batch sees at most one per variant and distinct value); it too hands back an unpruned,
    uncompacted list.  After a `recost` or a `prefix` -- once for the two together -- comes `priority` where the prune is on, then
    `caller_pairs` where there is a caller.  Then the group's finishes, in the order the sets were given.  So the first group of a
    None variant at the staged knn has nothing before its finishes, and a list of one set is its finish alone."""
    staged = max(st[0] for st in sets)
    steps, at, anew = [], staged, False
    for v in sorted({st[-1] for st in sets}, key=lambda v: (bool(layered[v]), v)):
        if layered[v]:
            steps.append(("recost", v))
            at, anew = staged, True
        for k in sorted({st[0] for st in sets if st[-1] == v}, reverse=True):
            if k != at:
                steps.append(("prefix", k))
                at, anew = k, True
            if anew:
                steps += [("priority",)] * bool(priority) + [("caller_pairs",)] * bool(caller)
                anew = False
            steps += [("finish", q) for q, st in enumerate(sets) if st[0] == k and st[-1] == v]
    return steps


def _checked_walk_sets(sets, variants, knn, mode, no_match_penalty, caller, triangulate):
    """`iter_device_windows`' sets and variants, checked and in one form -> ([(knn, WindowMode, no_match_penalty, variant index) per
    set], [DeviceTypesLayer or None per variant], [(`result.set`, what the collector is told beside the states and the windows) per
    set]).  The plain form (`sets` None) is the one set (`knn`, `mode`, `no_match_penalty`) of the one variant None; a set of three
    values is of variant 0."""
    tags = [(None, ())] if sets is None else [(q, (q,)) for q in range(len(sets))]
    if variants is not None and (sets is None or len(variants) == 0):
        raise ValueError("variants: at least one, and with sets that name them")
    variants = [None] if variants is None else list(variants)
    sets = [(knn, mode, no_match_penalty, 0)] if sets is None else [(int(st[0]), st[1], float(st[2]), int(st[3]) if len(st) > 3 else 0)
                                                                     for st in sets]
    if not sets or (len(sets) > 1 and ((caller is not None and not isinstance(caller, DeviceCallerTris)) or not triangulate)):
        raise ValueError("sets: at least one; several only with windows triangulated by the route or by a DeviceCallerTris")
    if any(not 0 <= v < len(variants) for _k, _m, _p, v in sets):
        raise ValueError("sets: a variant index outside `variants`")
    return [(k, WindowMode.default() if m is None else m, p, v) for k, m, p, v in sets], variants, tags


class _WindowStates:
    """The DeviceWindows of one pass of `iter_device_windows`, and how many windows go together.  Windows go to the library in batches
    of `batch` (`size`; default $SAME_WINDOW_BATCH, else 8), at most `ahead_max` are staged and not yet finished ($SAME_WINDOW_AHEAD
    beyond the route's `depth`).  `take(n)` hands out states -- the context's from earlier passes (`ctx._device_windows`) first, new
    ones after --, `give(states)` takes them back for the next batch.  `all` holds every state of the pass once, handed out or not,
    and `close()` leaves those with the context: whatever ended the pass -- a refused library call, a triangulator that raised, a
    consumer that walked away -- a state is in the context's cache once or closed, and no call site has a failure path of its own."""

    def __init__(self, ctx, n_windows, batch, depth):
        B = max(1, min(int(batch if batch is not None else os.environ.get("SAME_WINDOW_BATCH", "8")), WINDOW_BATCH_MAX, max(n_windows, 1)))
        if batch is None and depth > 0:
            # a rank with three helpers (eight ranks on a 16-CPU host) gains nothing from collecting eight tickets at once
            B = min(B, max(2, depth))
        # windows staged and not yet finished: one per helper BEYOND the batch being finished (a batch's tickets are collected together,
        # and nothing is handed over meanwhile: with only `depth` in flight, 12 helpers and batches of 8 ran 8 of 12 helpers -- 264
        # against 431 windows/s for one thread of a rank that shares its host with another)
        self.size, self.ahead_max = B, max(B, depth + int(os.environ.get("SAME_WINDOW_AHEAD", str(B))))
        # window states (their device buffers, grown once) are kept with the context from one call to the next: a pass over a plan
        # then makes no device allocation at all.  In use at once: the windows ahead + the batch being staged + the batch last yielded
        self.ctx, self.cache = ctx, ctx.__dict__.setdefault("_device_windows", [])
        self.want = min(self.ahead_max + 2 * B, max(n_windows, 1) + B)
        self.all = [self.cache.pop() for _ in range(min(self.want, len(self.cache)))]       # every state of the pass, each once
        self.free = list(self.all)

    def take(self, n):
        new = [DeviceWindow(self.ctx) for _ in range(n - len(self.free))]
        self.all += new
        self.free += new
        at = len(self.free) - n
        states, self.free[at:] = self.free[at:], []
        return states

    def give(self, states):
        self.free.extend(states)

    def close(self):
        self.cache.extend(self.all)
        for extra in self.cache[self.want:]:          # a context keeps what one pass needs, not every state it ever had
            extra.close()
        del self.cache[self.want:]


# what the calls of one pass of `iter_device_windows` read beside their windows; `filt`: the triangle filter's arguments (radius,
# angle_enabled, cos_thr, near_tol, ignore_same_type_triangles)
_WalkPass = namedtuple("_WalkPass", "ctx moving tri caller filt min_angle_deg")


def _host_filter(c, axy, rows, tris, **how):
    """the triangle filter of a window with a cosine at the threshold, re-decided on the host with the reference's literal expression
    (triangles.filter_triangles_by_radius over the aligned cells `axy`, section rows `rows`)"""
    from .triangles import filter_triangles_by_radius

    radius, _angle_enabled, _cos_thr, _near_tol, same_type = c.filt
    tid = c.moving.type_id[rows] if (same_type and c.moving.type_id is not None) else None
    return filter_triangles_by_radius(axy, tris, radius, ignore_same_type_triangles=same_type, min_angle_deg=c.min_angle_deg,
                                      verbose=False, ctx=c.ctx, _rows_as_array=True, _type_id=tid, **how)


def _caller_front(c, pairs_of):
    """the staged windows [(record, state)] that have pairs: their triangles from `c.caller`, their unconstrained nodes gone"""
    if not pairs_of:
        return
    got = caller_tris_windows([st for _o, st in pairs_of], c.caller, *c.filt)
    for q, (out, state) in enumerate(pairs_of):
        if got[q][2]:
            with marked("triangle filter (host: a cosine at the threshold)"):
                rows0 = state.fetch(_W_ALIGNED_ROWS)
                kept, gone = _host_filter(c, state.fetch(_W_ALIGNED_XY), rows0, state.fetch(_W_CALLER_TRIANGLES),
                                          remove_unconstrained_nodes=True)
                mask = np.zeros(len(rows0), np.uint8)
                mask[sorted(gone)] = 1
                got[q] = caller_tris_windows([state], c.caller, *c.filt, removed=[mask])[0]
                kept = np.asarray(kept).reshape(-1, 3)
                kept = kept[(mask[kept] == 0).all(axis=1)] if len(kept) else kept        # src/same.py:1076-1078
                out.triangles = (np.cumsum(mask == 0) - 1)[kept].astype(np.int32).reshape(-1, 3)
        out.removed = got[q][1]
        out.skipped = got[q][4] == 0          # every node unconstrained, or the removed ones held every pair


def _finish_callers(c, todo, states, no_match_penalty, mode):
    """the finish call over the caller's triangles, which are on the device (SAME_TRIS_CALLER); a window the host filtered
    (_caller_front) brings its kept list.  -> (result per window, no simplices)"""
    with marked("filter + signs + incumbent + sweeps (device)"):
        mine = [q for q, (o, _s, _t) in enumerate(todo) if o.triangles is None]
        res = dict(zip(mine, filter_finish_windows([states[q] for q in mine], None, *c.filt, no_match_penalty, mode=mode,
                                                   from_caller=True) if mine else []))
        for q, (o, st, _t) in enumerate(todo):
            if o.triangles is not None:
                res[q] = (len(o.triangles), 0, 0) + tuple(st.finish(o.triangles, no_match_penalty, mode))
    if any(r[2] for r in res.values()):        # (the node mask's kernel classifies the same corners with the same expressions)
        raise RuntimeError("a cosine at the angle threshold that same_window_caller_tris did not report")
    return res, [None] * len(todo)


def _finish_triangulated(c, states, tickets, no_match_penalty, mode, first):
    """the finish call over the triangulator's answers -> (result per window, simplices per window); `first`: the batch's first
    finish (the route's per-batch hook runs once; a ticket keeps its answer)"""
    args = c.filt + (no_match_penalty,)
    if first:
        c.tri.before_finish(states, tickets, *c.filt[:3])
    with marked("triangulate (wait for helper)"):
        tris = [ticket.result() for ticket in tickets]
    with marked("filter + signs + incumbent + sweeps (device)"):
        # candidates the device made stay there (simplices None); every other window brings its simplices
        mine = [q for q, t in enumerate(tris) if t is None]
        theirs = [q for q, t in enumerate(tris) if t is not None]
        res = dict(zip(mine, filter_finish_windows([states[q] for q in mine], None, *args, mode=mode) if mine else []))
        res.update(zip(theirs, filter_finish_windows([states[q] for q in theirs], [tris[q] for q in theirs], *args, mode=mode)
                       if theirs else []))
    # simplices that are not Qhull's own (delaunay.py: the same triangles in another order): where the window's numbers hang on that
    # order -- the device counted such places, or a cosine sits at the threshold and the host is about to re-decide the filter --
    # the window is finished again with scipy's
    for q, (state, ticket) in enumerate(zip(states, tickets)):
        if ticket.native and (state.order_ties or res[q][2]):
            with marked("order ties: the window again with Qhull's simplices"):
                tris[q] = ticket.qhull()
                res[q] = filter_finish_windows([state], [tris[q]], *args, mode=mode)[0]
    return res, tris


def _set_result(rec, mode, tag, variant):
    """-> the DeviceWindowResult of the staged window `rec` under one set, before that set's finish call: the staged record + the state
    as the set's knn group left it"""
    out = DeviceWindowResult(rec.window, mode)
    out.set, out.variant, out.error, out.skipped, out.removed = tag, variant, rec.error, rec.skipped, rec.removed
    out.rows_m, out.axy, out.triangles, out.state = rec.rows_m, rec.axy, rec.triangles, rec.state
    out.counts, out.priority = (rec.counts, rec.priority) if rec.state is None else (rec.state.counts, rec.state.priority)
    out.n_triangles = None if rec.state is None else 0
    return out


def iter_device_windows(ref, moving, dref, dmoving, plan, radius=250, knn=8, dist_ct_coeff=1.0, min_angle_deg=15,
                        ignore_same_type_triangles=True, no_match_penalty=100.0, ctx=None, fetch_triangles=False, triangulator=None,
                        triangulate=True, batch=None, collector=None, mode=None, caller=None, priority=False, sets=None, variants=None):
    """The window path of `iter_window_arrays` + the incumbent and the three sweeps, with both sections resident on the device (`dref`,
    `dmoving`: DeviceSections of `ref`, `moving`): per window the host only triangulates (Qhull helpers, windows ahead as before) and
    receives the match; the triangle filter runs on the device too, unless a cosine sits within 8 ulp of the angle threshold (then the
    host re-decides it with the reference's literal expression, as triangles.classify_triangles does).  The numbers are those of the
    column pipeline (tests/test_gpu_run_same.py::test_device_windows_equal_the_column_pipeline).
    YIELDS DeviceWindowResults.  What a window is finished under is a SET, a (knn, WindowMode, no_match_penalty) triple.  The plain form
    has one, (`knn`, `mode`, `no_match_penalty`), and yields one result per window in plan order, `result.set` and `result.variant` None;
    a window without pairs yields `.error`.  `sets=[...]` is a parameter sweep over ONE pass (then `knn`, `mode` and `no_match_penalty`
    are not read): every window is staged once, at the largest knn, triangulated once, and finished once per set.  Windows go to the
    library in BATCHES (`batch`; _WindowStates); per batch the results come set by set in the order of `batch_schedule`'s finishes --
    THE statement of which calls a batch makes and in which order -- one per window each, `result.set` the set's index; `mode`,
    `counts`, `priority` and everything the finish call leaves are that set's, `rows_m` / `axy` are shared by the window's results.  A list
    of one set makes the calls of the plain form; more than one does not go with `triangulate=False`, and with `caller` only when that
    is a DeviceCallerTris (its selection does not depend on knn: it is made once per batch and serves every set).
    `result.state` is the live DeviceWindow until the generator is asked for the first window of the next batch, and with several sets
    only until the next set's finish.
    `triangulator`: the route, a delaunay.Triangulator (default: delaunay.QHULL, the Qhull helper pool).  It says how many windows to
    stage ahead and whether to start the helpers first; each window is submitted when it is staged, and the route's per-batch hook runs
    right before the batch's first filter + finish call.  A ticket's `.result()` is the simplices, or None for candidates the device
    made; one whose `.native` is true after `.result()` brought simplices that are not scipy's own and has `.qhull()` for those
    (delaunay.py).  One ticket per window serves every set: scipy's simplices, once a set's order ties asked for them, are the ticket's
    answer for the sets after it.
    `triangulate=False` stops after the stage call (rows, prune, costs, compaction): the caller brings its own triangles
    (api.sliding_window_matching with a caller's triangulation) and reads pairs / costs through `state.fetch`.
    `collector(states, windows)` -- with `sets`: `collector(states, windows, set index)` -- is called once per finished batch and set
    with its windows' live states (the window merge's accumulator: MergeAccumulator.collect).
    `caller`: a DeviceCallerTris of `dmoving` -- the triangulation source that needs no triangulator (`triangulator`, and with it
    optim_params["hip_delaunay"], is irrelevant then).  Right after a batch's stage call ONE more call selects and remaps every window's
    triangles, works out the filter's node mask and leaves the window without its unconstrained nodes (caller_tris_windows;
    src/same.py:1016-1085); rows_m, axy, counts and everything later describe that smaller window.  A window left without pairs is
    yielded with `.skipped`; one with a cosine at the threshold has triangles AND mask re-decided on the host.
    `priority`: the cell-type-priority prune (optim_params["ignore_knn_if_matched"], src/knn_utils.py:28-78) on the device: right after a
    batch's stage call -- before anything is triangulated or selected, as the reference filters its pairs before it triangulates --
    ONE more call filters every window's pair list (priority_windows); both sections need their label codes
    (DeviceSection.set_label_codes).  `counts[3]`, the pairs and costs a state hands out and everything later are the filtered list's;
    the pair list as staged (or as cut) stays fetchable (_W_STAGED_PAIRS) and stays the frame of the reference limits.
    `variants=[layer or None, ...]` (with `sets`): TYPE-MATRIX VARIANTS of the moving section over the same pass -- each a
    DeviceTypesLayer of `dmoving`, or None for the section's own types -- and a set is then (knn, WindowMode, no_match_penalty, variant
    index); a set of three values is of variant 0.  Only the pair costs read the type columns, so staging, the tickets and the
    caller's selection happen once per batch whatever the number of variants.  `result.variant` carries the index.
    A set's WindowMode (None: the greedy start alone): a window whose optimal start the device does not certify is solved again on
    the host (ops.sparse_assign_host, ops.sparse_transport_host) and finished again under that matching; every later finish of a window
    (that fallback, a re-finish with scipy's simplices) runs the mode's search again: `result.refine` holds the last one's counts."""
    from . import qhull_pool
    from .triangles import cos_threshold

    ctx = ops._ctx(ctx)
    sets, variants, tags = _checked_walk_sets(sets, variants, knn, mode, no_match_penalty, caller, triangulate)
    knn = max(st[0] for st in sets)
    schedule = batch_schedule(sets, [layer is not None for layer in variants], priority, caller is not None)
    angle_enabled, cos_thr = cos_threshold(min_angle_deg)
    near_tol = float(8 * np.spacing(abs(cos_thr))) if (angle_enabled and np.isfinite(cos_thr)) else 0.0
    tri = QHULL if triangulator is None else triangulator
    c = _WalkPass(ctx, moving, tri, caller, (radius, angle_enabled, cos_thr, near_tol, ignore_same_type_triangles), min_angle_deg)
    depth = 0 if caller is not None else int(tri.lookahead())
    if tri.warm and caller is None:
        qhull_pool.warm(min(depth, len(plan)))
    pool = _WindowStates(ctx, len(plan), batch, depth)
    B, r = pool.size, float(radius)
    prune_possible = r == r and int(knn) > 0
    # a schedule step that is no finish: its stage label and its call over the batch's live states
    between = {"recost": ("pair lists priced from the variant's type matrix (device)",
                          lambda states, v: recost_windows(states, dmoving, dref, variants[v], dist_ct_coeff)),
               "prefix": ("pair lists cut to the set's knn (device)", lambda states, k: prefix_windows(states, k)),
               "priority": ("cell-type-priority prune of the pair lists (device)", lambda states: priority_windows(states)),
               "caller_pairs": ("caller's triangles: the cut pair lists through the held node masks (device)",
                                lambda states: caller_pairs_windows(states))}

    def stage_batch(windows):
        """-> a _StagedWindow per window of `windows`, staged by ONE library call.  No failure path of its own: a call that raises
        ends the walk, whose `pool.close()` takes back the states handed out here"""
        staged = [_StagedWindow(w) for w in windows]
        if not prune_possible:
            for rec in staged:
                rec.error = ValueError("No valid_pairs after KNN filtering. Increase radius and/or knn.")
            return staged
        states = pool.take(len(windows))
        with marked("subset + prune + costs + compaction (device)"):
            counts = stage_windows(states, dmoving, dref, [w["box"] for w in windows], abs(r), knn, dist_ct_coeff)
        if priority:                                  # the list as staged is pruned here; a list cut or priced later, by `schedule`
            with marked("cell-type-priority prune of the pair lists (device)"):
                priority_windows(states)
            counts = [st.counts for st in states]
        if caller is not None:
            with marked("caller's triangles: select + remap + node mask + second compaction (device)"):
                _caller_front(c, [(rec, st) for rec, st, n in zip(staged, states, counts) if n[3] != 0])
            counts = [st.counts for st in states]
        for rec, state, n in zip(staged, states, counts):
            rec.counts, rec.priority = n, state.priority          # (the prune's counts, or the None the stage call leaves)
            if rec.skipped:
                continue
            if rec.counts[3] == 0:
                rec.error = ValueError("No valid_pairs after KNN filtering. Increase radius and/or knn.")
                continue
            rec.rows_m, rec.axy = state.fetch(_W_ALIGNED_ROWS), state.fetch(_W_ALIGNED_XY)
            if triangulate and caller is None:
                with marked("triangulate (hand-over; waits for a free helper)"):
                    rec.ticket = tri.submit(rec.axy, key=rec.window.get("window_id"))
            rec.state = state
        pool.give(st for rec, st in zip(staged, states) if rec.state is None)      # skipped, or without pairs
        return staged

    def finish_set(group, which, first):
        """-> a DeviceWindowResult per staged window of `group` under set `which`: filter + signs + incumbent + sweeps of the windows
        that have a state, by ONE library call (+ one per window whose filter met a cosine at the threshold); `first`: the batch's
        first finish.  A result is _set_result's + what the call leaves."""
        _k, mode, no_match_penalty, variant = sets[which]
        tag, told = tags[which]
        outs = [_set_result(rec, mode, tag, None if tag is None else variant) for rec in group]
        todo = [(out, rec.state, rec.ticket) for out, rec in zip(outs, group) if rec.state is not None]
        if not triangulate or not todo:
            return outs
        states, tickets = [st for _o, st, _t in todo], [t for _o, _s, t in todo]
        res, tris = (_finish_callers(c, todo, states, no_match_penalty, mode) if caller is not None
                     else _finish_triangulated(c, states, tickets, no_match_penalty, mode, first))
        for q, (out, state, _t) in enumerate(todo):
            _kept, _added, near, match_row, cell_flags, stats = res[q]
            if near:
                with marked("triangle filter (host: a cosine at the threshold)"):
                    out.triangles = _host_filter(c, out.axy, out.rows_m, tris[q])
                with marked("signs + incumbent + sweeps (device)"):
                    match_row, cell_flags, stats = state.finish(out.triangles, no_match_penalty, mode)
            if mode.incumbent != "greedy":
                out.assignment = {k: v for k, v in state.assignment.items() if k != "flags"}
                out.assignment["fallback"] = 0
                if state.assignment["flags"]:
                    match_row, cell_flags, stats = _assignment_fallback(state, out, moving, no_match_penalty, mode, ref)
            out.refine = state.refine
            out.match_row, out.stats = match_row, stats
            # the library packs both per-cell flags into one byte
            out.point_flag, out.flip_flag = cell_flags & 1, (cell_flags >> 1) & 1
            out.n_triangles = state.n_triangles
            if fetch_triangles and out.triangles is None:
                out.triangles = state.fetch(_W_TRIANGLES)
        if collector is not None:
            with marked("central rows to the merge accumulator (device, enqueue only)"):
                collector(states, [o.window for o, _s, _t in todo], *told)
        return outs

    def finish_sets(group):
        """the staged windows of `group` taken through `schedule` -> yields every set's results; a batch without a live state makes
        none of the calls between the finishes"""
        states = [rec.state for rec in group if rec.state is not None]
        first = True
        for kind, *arg in schedule:
            if kind == "finish":
                yield from finish_set(group, arg[0], first)
                first = False
            elif states:
                label, call = between[kind]
                with marked(label):
                    call(states, *arg)

    pending, live, nxt = deque(), [], 0
    try:
        while nxt < len(plan) or pending:
            while nxt < len(plan) and (not pending or len(pending) + min(B, len(plan) - nxt) <= pool.ahead_max):
                windows = plan[nxt:nxt + B]
                nxt += len(windows)
                pending.extend(stage_batch(windows))
            pool.give(live)                       # the caller has moved on: the previous batch's states go back to the pool
            group = [pending.popleft() for _ in range(min(B, len(pending)))]
            live = [rec.state for rec in group if rec.state is not None]
            yield from finish_sets(group)
    finally:
        pool.close()
