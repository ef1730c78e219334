"""A study read as FEATURE MEANS of its matched pairs: `sliding_window_score_features` (at cell level, `unpack=`: §5.20).

Every study the reference's notebooks report ends the same way: the matches put two modalities' feature matrices side by side and the
result is read as means.  examples/luad/reproduce_figures.ipynb cells 16-22 gather the PCF rows and the Xenium rows of every matched
pair into one `combinedAD`, plot `sc.pl.matrixplot(..., groupby='pcf_Annotations', standard_scale='var')` -- the mean of every marker
per moving label (Fig 5) --, take `cdist(X_spatial, sftp_pos_coords).min(axis=1)`, the distance of every pair to the nearest pair of a
marked zone, `pd.cut` it at 0 / 15 / 30 / inf and plot the mean of the exhaustion markers per distance bin over a marked subset of the
pairs; examples/tongue builds the same table for Fig 4's matrixplot.

When a set's merge ends everything that reading needs is resident or constant over the study: the final rows and both sections' XY
are resident, the two feature matrices, the moving rows' groups and the zone / subset masks are constant.  One more call per result
beside the score call (csrc/window_score_feature.hip) sums there.

FIXED-POINT COLUMNS.  A float sum over pairs depends on its order and float atomics are not reproducible, so no host statement could be
held bit for bit.  Every feature column is therefore quantised once (`quantize_features`, after `ops.quantize_types`): with m the
column's largest magnitude and p = frexp(m)'s exponent, e = 30 - p and q = rint(ldexp(x, e)) as int32.  Sums of q are exact in int64,
the same from run to run and on every grid.  `means_from_sums` turns them into means for the device route and the host statement alike;
against the true mean it errs by at most 2**(-e-1) + 3 * 2**-53 * |mean|.  A column with one huge outlier loses its small values: a
value is rounded to a multiple of `resolution` = 2**-e, which is 2**-30 of the power of two above the column's largest magnitude (an
error of at most 2**-31 of it).

`score_table_features` is the same reading of a result TABLE with numpy: what the device must equal, and what inputs the device
refuses go through.

AT CELL LEVEL (`unpack=`).  The LUAD notebook never reads metacell pairs: cell 12 unpacks the metacell matches to cells and everything
after it is built on the cell pairs -- a metacell has no PCF or Xenium row, and its annotation is not a cell's.  With `unpack=` the
features, groups and masks are per ORIGINAL cell of the two MetaCell objects, reordered once into the member lists' CSR order, and one
call per result in the unpack call's place sums them over the cell pairs where the unpack phases make them
(csrc/window_unpack_feature.hip).  `score_unpacked_features` is its host statement, built from `score_unpacked`'s table and the same
numpy sums."""
import collections

import numpy as np
import pandas as pd

from . import _lib
from .score_details import _NoMetaCellObjects, checked_groups
from .scores import DeviceScores, _frame_rows, _scored_study, checked_score_params, checked_unpack, score_unpacked, unpack_record
from .variants import _frames_of

ScoreFeatures = collections.namedtuple("ScoreFeatures", "scores rows means sums resolution zones pairs")
TableFeatures = collections.namedtuple("TableFeatures", "rows means sums resolution zones pairs")
ZoneReading = collections.namedtuple("ZoneReading", "rows means sums zone_pairs subset_pairs")
FeatureZones = collections.namedtuple("FeatureZones", "zone_moving zone_ref subset_moving subset_ref edges labels", defaults=(None,))
NO_GROUP, NO_BIN = "(no group)", "(no bin)"       # the rows of the pairs whose moving row has no group / whose distance is in no bin
Q_BITS = 30


# ---- fixed point -------------------------------------------------------------------------------------------------------------------------
def quantize_features(x):
    """-> (int32 (n, F) fixed-point columns, int32 (F,) exponents e): per column m = max |x|, p = frexp(m)[1], e = 30 - p (0 for an
    all-zero or empty column), q = rint(ldexp(x, e)), so |q| <= 2**30.  `x`: a finite float64 (n, F) matrix."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    m = np.abs(x).max(axis=0) if x.shape[0] else np.zeros(x.shape[1])
    e = np.where(m > 0, Q_BITS - np.frexp(m)[1], 0).astype(np.int32)
    return np.rint(np.ldexp(x, e)).astype(np.int32), e


def means_from_sums(sums, n, e):
    """the means of the integer `sums` (..., F) over `n` (...) pairs each under the exponents `e` (F,): ldexp(float64(sum) / n, -e); NaN
    with no pair.  The one place where sums become means."""
    sums, n = np.asarray(sums, np.int64), np.asarray(n, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.ldexp(sums.astype(np.float64) / n[..., None].astype(np.float64), -np.asarray(e, np.int32))


def standard_scale_var(means):
    """scanpy's `standard_scale='var'` of a matrixplot (sc.pl.matrixplot: `values_df -= values_df.min(0)`, `values_df = (values_df /
    values_df.max(0)).fillna(0)`): per column subtract the minimum, divide by the maximum, NaN -> 0"""
    out = means - means.min(axis=0)
    return (out / out.max(axis=0)).fillna(0)


def d2_threshold(edge):
    """the largest float64 t with np.sqrt(t) <= edge -- so that `d2 <= t` is exactly `np.sqrt(d2) <= edge` for every d2 >= 0 --, found
    from edge * edge by stepping with nextafter; -inf for a negative edge (no distance is at or below it), ValueError for NaN"""
    e = float(edge)
    if e != e:
        raise ValueError("a distance edge is NaN")
    if e < 0:
        return float("-inf")
    with np.errstate(over="ignore"):                  # (an edge whose square overflows: the largest finite double)
        t = np.float64(e) * np.float64(e)
        while np.sqrt(t) > e:
            t = np.nextafter(t, -np.inf)
        while t < np.inf and np.sqrt(np.nextafter(t, np.inf)) <= e:
            t = np.nextafter(t, np.inf)
    return float(t)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def checked_features(features, frame, side):
    """-> (float64 (rows, F) matrix, the F column names prefixed `side`_), or (None, []) for None.  `features`: a DataFrame on the
    frame's index, an array of (rows, F) numbers or a list of the frame's own column names.  ValueError for anything else, a wrong
    length, values that are no numbers or not finite."""
    if features is None:
        return None, []
    n = len(frame)
    if isinstance(features, pd.DataFrame):
        if not features.index.equals(frame.index):
            raise ValueError(f"{side}_features is not on the {side} frame's index")
        names, values = [str(c) for c in features.columns], features.to_numpy()
    elif isinstance(features, (list, tuple)) and all(isinstance(c, str) for c in features) and len(features):
        lacking = [c for c in features if c not in frame.columns]
        if lacking:
            raise ValueError(f"{side}_features names columns the {side} frame lacks: {lacking}")
        names, values = list(features), frame[list(features)].to_numpy()
    else:
        if isinstance(features, (str, bytes, dict)) or not hasattr(features, "__len__"):
            raise ValueError(f"{side}_features must be a DataFrame, an (n, F) array or a list of column names, not {type(features).__name__}")
        values = np.asarray(features)
        if values.ndim != 2:
            raise ValueError(f"{side}_features must be an (n, F) array, not one of shape {values.shape}")
        names = [str(c) for c in range(values.shape[1])]
    if values.ndim != 2 or values.shape[0] != n:
        raise ValueError(f"{side}_features has {values.shape[0]} rows; the {side} frame has {n}")
    if values.dtype.kind not in "fiub":
        try:
            values = values.astype(np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{side}_features holds values that are no numbers") from None
    values = np.ascontiguousarray(values, dtype=np.float64)
    if not np.isfinite(values).all():
        raise ValueError(f"{side}_features holds values that are not finite")
    return values, [f"{side}_{c}" for c in names]


def checked_zones(zones, n_ref, n_mov):
    """-> (uint8 flags per moving row, per reference row -- bit 0 zone side, bit 1 subset side --, the float64 thresholds on the squared
    distance (`d2_threshold` per edge), the bin labels), or None for None.  ValueError unless `zones` is a FeatureZones whose masks are
    None or boolean arrays of their frame's length, whose edges are 2 .. 65 numbers, no NaN, non-decreasing, and whose labels, if
    given, are one per bin."""
    if zones is None:
        return None
    if not isinstance(zones, FeatureZones):
        raise ValueError(f"zones must be a FeatureZones, not {type(zones).__name__}")

    def mask(m, n, name):
        if m is None:
            return np.ones(n, bool)
        m = np.asarray(m)
        if m.shape != (n,) or m.dtype.kind != "b":
            raise ValueError(f"zones.{name} must be a boolean mask of {n} rows, not {m.dtype} of shape {m.shape}")
        return m

    zm, sm = mask(zones.zone_moving, n_mov, "zone_moving"), mask(zones.subset_moving, n_mov, "subset_moving")
    zr, sr = mask(zones.zone_ref, n_ref, "zone_ref"), mask(zones.subset_ref, n_ref, "subset_ref")
    try:
        edges = np.asarray(zones.edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("zones.edges must be numbers") from None
    if edges.ndim != 1 or not 2 <= len(edges) <= _lib.SAME_FEATURE_MAX_EDGES:
        raise ValueError(f"zones.edges must be 2 .. {_lib.SAME_FEATURE_MAX_EDGES} distances, as given to pd.cut")
    if np.isnan(edges).any() or (np.diff(edges) < 0).any():
        raise ValueError("zones.edges must not decrease and hold no NaN")
    B = len(edges) - 1
    if zones.labels is None:
        labels = [f"({edges[b]:g}, {edges[b + 1]:g}]" for b in range(B)]
    else:
        labels = list(zones.labels)
        if len(labels) != B:
            raise ValueError(f"zones.labels has {len(labels)} labels for {B} bins")
    thresholds = np.array([d2_threshold(e) for e in edges], np.float64)
    return (zm.astype(np.uint8) | (sm.astype(np.uint8) << 1)), (zr.astype(np.uint8) | (sr.astype(np.uint8) << 1)), thresholds, labels


class FeatureSpec:
    """What a study sums, checked and quantised once for the device route and the host statement: the two fixed-point matrices (None: the
    side has no column), their exponents and names, the moving rows' group codes and names, the zone's flags, thresholds and labels."""

    def __init__(self, ref_df, mov_df, moving_features, ref_features, group_by, zones, xy_cols=("X", "Y"), default_group="cell_type"):
        if moving_features is None and ref_features is None:
            raise ValueError("pass moving_features, ref_features or both: there is no feature to read")
        mov_x, mov_names = checked_features(moving_features, mov_df, "moving")
        ref_x, ref_names = checked_features(ref_features, ref_df, "ref")
        self.names = mov_names + ref_names
        if not self.names:
            raise ValueError("the features hold no column")
        self.mov_q, e_m = quantize_features(mov_x) if mov_x is not None else (None, np.zeros(0, np.int32))
        self.ref_q, e_r = quantize_features(ref_x) if ref_x is not None else (None, np.zeros(0, np.int32))
        self.e = np.concatenate((e_m, e_r)).astype(np.int32)
        if group_by is None:
            if default_group not in mov_df.columns:
                raise ValueError(f"group_by=None groups by the moving frame's '{default_group}': it has no such column")
            group_by = default_group
        self.group_codes, self.group_names = checked_groups(group_by, mov_df)
        self.n_groups = max(len(self.group_names), 1)
        self.zone = checked_zones(zones, len(ref_df), len(mov_df))
        self.ref_xy_finite = True
        if self.zone is not None:
            for c in xy_cols:
                if c not in ref_df.columns:
                    raise ValueError(f"zones measure distances between reference cells: the ref frame has no '{c}' column")
            self.ref_xy_finite = bool(np.isfinite(ref_df[list(xy_cols)].to_numpy(dtype=np.float64)).all())
        self.n_mov, self.n_ref = len(mov_df), len(ref_df)

    @property
    def device_ok(self):
        """within the library's caps, and no zone over non-finite reference XY (the library refuses those)"""
        return len(self.names) <= _lib.SAME_FEATURE_MAX_COLUMNS and self.n_groups <= _lib.SAME_SCORE_MAX_GROUPS and self.ref_xy_finite

    def resolution(self):
        return pd.Series(np.ldexp(1.0, -self.e), index=self.names, name="resolution")

    # the words of one result -> its frames: the one statement of them for the device's words and the host's
    def _by_bin(self, rows, sums, labels, rest_label):
        rows, sums = np.asarray(rows, np.int64), np.asarray(sums, np.int64)
        keep = len(labels) + (1 if rows[-1] else 0)              # (the rest row only where a pair is in it)
        index = pd.Index(list(labels) + [rest_label], dtype=object)[:keep]
        n = pd.Series(rows[:keep], index=index, name="pairs")
        return (n, pd.DataFrame(means_from_sums(sums[:keep], rows[:keep], self.e), index=index, columns=self.names),
                pd.DataFrame(sums[:keep], index=index, columns=self.names))

    def frames(self, words):
        """(rows, means, sums, zones) of the library's words (windows.split_score_features) or `host_words`' of one result"""
        G = self.n_groups
        rows, sums = np.asarray(words["rows"], np.int64), np.asarray(words["sums"], np.int64)
        if not self.group_names:                                 # (every value missing: the library's one group stays empty)
            rows, sums = rows[G:], sums[G:]
        n, means, total = self._by_bin(rows, sums, self.group_names, NO_GROUP)
        zone = None
        if self.zone is not None:
            zn, zmeans, zsums = self._by_bin(words["bin_rows"], words["bin_sums"], self.zone[3], NO_BIN)
            zone = ZoneReading(zn, zmeans, zsums, int(words["counts"][2]), int(words["counts"][3]))
        return n, means, total, zone

    def pair_frame(self, index, ref_ids, a_row, r_row, d2):
        """the per-pair frame of one result, indexed like the moving frame: `ref_id` of the reference cell the row was put on (<NA> /
        None: unmatched) and with a zone `distance_to_zone` = sqrt(d2), NaN where the row has no subset pair"""
        ref_row = np.full(len(index), -1, np.int64)
        ref_row[np.asarray(a_row, np.int64)] = np.asarray(r_row, np.int64)
        ids = pd.Series(np.asarray(ref_ids))
        if ids.dtype.kind in "iu":
            ids = ids.astype("Int64")
        ref_id = ids.take(np.maximum(ref_row, 0)).reset_index(drop=True).where(pd.Series(ref_row >= 0)) if len(ids) else pd.Series([None] * len(index))
        cols = {"ref_id": ref_id.to_numpy() if ref_id.dtype == object else ref_id.array}
        if self.zone is not None:
            cols["distance_to_zone"] = np.sqrt(np.asarray(d2, np.float64))
        return pd.DataFrame(cols, index=index)


# ---- the host statement ------------------------------------------------------------------------------------------------------------------
def _sum_by(bins, q, n_bins):
    """(rows per bin, int64 sums of q's rows per bin) over bins in [0, n_bins)"""
    rows = np.bincount(bins, minlength=n_bins).astype(np.int64)
    sums = np.zeros((n_bins, q.shape[1]), np.int64)
    for b in np.flatnonzero(rows):
        sums[b] = q[bins == b].sum(axis=0, dtype=np.int64)
    return rows, sums


def nearest_zone_d2(xy, zone_xy, chunk_elements=1 << 22):
    """per row of `xy` the minimum over `zone_xy` of dx*dx + dy*dy in float64 -- np.sqrt of it is cdist(xy, zone_xy).min(axis=1) --, the
    brute-force matrix in chunks of rows; NaN with no zone point"""
    xy, zone_xy = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(zone_xy, np.float64).reshape(-1, 2)
    out = np.full(len(xy), np.nan)
    if not len(zone_xy):
        return out
    step = max(1, chunk_elements // len(zone_xy))
    for lo in range(0, len(xy), step):
        dx = xy[lo:lo + step, None, 0] - zone_xy[None, :, 0]
        dy = xy[lo:lo + step, None, 1] - zone_xy[None, :, 1]
        out[lo:lo + step] = (dx * dx + dy * dy).min(axis=1)
    return out


def host_words(spec, a_row, r_row, ref_xy=None):
    """same_merge_acc_score_features' words of the pairs (moving row, reference row), with numpy: -> ({counts, rows, sums[, bin_rows,
    bin_sums]}, d2 per moving row or None without a zone)"""
    a, r = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    G, F_m = spec.n_groups, 0 if spec.mov_q is None else spec.mov_q.shape[1]
    g = spec.group_codes[a].astype(np.int64) if len(a) else np.zeros(0, np.int64)
    g = np.where(g < 0, G, g)
    sides = ([spec.mov_q[a]] if spec.mov_q is not None else []) + ([spec.ref_q[r]] if spec.ref_q is not None else [])
    q = np.concatenate(sides, axis=1) if len(a) else np.zeros((0, len(spec.names)), np.int32)      # (int32: summed in int64 below)
    assert q.shape[1] == len(spec.names) and F_m <= q.shape[1]
    rows, sums = _sum_by(g, q, G + 1)
    words = {"counts": np.array([len(a), len(a) - rows[G], 0, 0], np.int64), "rows": rows, "sums": sums}
    if spec.zone is None:
        return words, None
    mov_flags, ref_flags, thresholds, _labels = spec.zone
    f = mov_flags[a] & ref_flags[r]
    zone, subset = (f & 1) != 0, (f & 2) != 0
    xy = np.asarray(ref_xy, np.float64).reshape(-1, 2)[r]
    d2 = nearest_zone_d2(xy[subset], xy[zone])
    d2[zone[subset]] = 0.0                                        # a pair that is both: its own position is a zone position
    B = len(thresholds) - 1
    b = np.searchsorted(thresholds, d2, side="left") - 1          # thresholds[b] < d2 <= thresholds[b + 1]; NaN sorts last
    b = np.where((b < 0) | (b >= B) | np.isnan(d2), B, b)
    words["bin_rows"], words["bin_sums"] = _sum_by(b, q[subset], B + 1)
    words["counts"][2:] = int(zone.sum()), int(subset.sum())
    d2_mov = np.full(spec.n_mov, np.nan)
    d2_mov[a[subset]] = d2
    return words, d2_mov


def score_table_features(table, ref, moving, *, cell_id_col, moving_features=None, ref_features=None, group_by=None, zones=None,
                         per_pair=False, _spec=None):
    """The feature reading of ONE result table of `sliding_window_incumbent` / `_sweep` / `_variants` over the frames `ref` and `moving`
    (MetaCell objects: their `.metacell_df`), with numpy -- what `sliding_window_score_features`' frames of that result must equal, bit
    for bit: the same quantisation, the same `means_from_sums`, the distance as the brute-force minimum in chunks.  -> `TableFeatures`
      rows        pairs per group of the moving rows (`group_by`; None: the moving frame's `cell_type`), groups in pd.factorize order;
                  a last row "(no group)" where pairs have none;
      means, sums one frame each, groups as rows, the feature columns as `moving_<name>` then `ref_<name>`: the mean
                  (`means_from_sums`; the notebook's `groupby().mean()` within the error the module states) and the int64 fixed-point sum;
      resolution  per feature column 2**-e: what its values were rounded to a multiple of;
      zones       with `zones`: `ZoneReading(rows, means, sums, zone_pairs, subset_pairs)` -- the same three per distance bin over the
                  subset pairs (a last row "(no bin)" where pairs are in none), and the two pair counts; else None;
      pairs       with per_pair: indexed like the moving frame, `ref_id` and with `zones` `distance_to_zone`; else None.
    A pair's position is its reference cell's X, Y.  A pair is a zone pair iff zone_moving[its moving row] and zone_ref[its reference
    row], a subset pair likewise; `distance_to_zone` of a subset pair is `cdist(position, zone positions).min()` (0 for a pair that is
    both, NaN with no zone pair) and its bin `pd.cut(distance, edges)`'s."""
    ref, moving = getattr(ref, "metacell_df", ref), getattr(moving, "metacell_df", moving)
    spec = _spec if _spec is not None else FeatureSpec(ref, moving, moving_features, ref_features, group_by, zones)
    n = len(table)
    for df, name in ((ref, "ref"), (moving, "moving")):
        if cell_id_col not in getattr(df, "columns", ()):
            raise ValueError(f"the table names cells by '{cell_id_col}': the {name} frame has no such column")
    rows_m = _frame_rows(moving[cell_id_col].to_numpy(), table[f"Aligned_{cell_id_col}"].to_numpy(), "moving") if n else np.zeros(0, np.int64)
    rows_r = _frame_rows(ref[cell_id_col].to_numpy(), table[f"Ref_{cell_id_col}"].to_numpy(), "reference") if n else np.zeros(0, np.int64)
    words, d2 = host_words(spec, rows_m, rows_r, ref[["X", "Y"]].to_numpy(dtype=np.float64) if spec.zone is not None else None)
    rows, means, sums, zone = spec.frames(words)
    pairs = spec.pair_frame(moving.index, ref[cell_id_col].to_numpy(), rows_m, rows_r, d2) if per_pair else None
    return TableFeatures(rows, means, sums, spec.resolution(), zone, pairs)


def unpack_spec(ref_mc, moving_mc, moving_features, ref_features, group_by, zones):
    """the FeatureSpec of a cell-level reading: everything per row of the two objects' `original_df` -- features, the moving cells'
    groups (None: their `cell_type_col`), the masks; positions are the reference cells' `x_col`, `y_col`"""
    return FeatureSpec(ref_mc.original_df, moving_mc.original_df, moving_features, ref_features, group_by, zones,
                       xy_cols=(ref_mc.x_col, ref_mc.y_col), default_group=moving_mc.cell_type_col)


def _cell_frames(spec, ref_mc, moving_mc, rows_m, rows_r, words, d2, per_pair):
    """both routes' one statement of a cell-level result's frames and dtypes: `words` and the pairs' rows in the two `original_df`s"""
    rows, means, sums, zone = spec.frames(words)
    pairs = None
    if per_pair:
        pairs = spec.pair_frame(pd.Index(moving_mc.original_df[moving_mc.original_idx_col].to_numpy(), name=moving_mc.original_idx_col),
                                ref_mc.original_df[ref_mc.original_idx_col].to_numpy(), rows_m, rows_r, d2)
    return TableFeatures(rows, means, sums, spec.resolution(), zone, pairs)


def score_unpacked_features(table, ref_mc, moving_mc, strategy, *, moving_features=None, ref_features=None, group_by=None, zones=None,
                            per_pair=False, _spec=None):
    """The cell-level feature reading of ONE result table over the MetaCell objects `ref_mc` and `moving_mc`, with numpy -- what
    `sliding_window_score_features(..., unpack=strategy)`'s frames of that result must equal, bit for bit, and what serves everything
    the device refuses: `score_unpacked`'s cell pairs (examples/luad/reproduce_figures.ipynb cell 12), then `score_table_features`'
    sums over them -- the same quantisation of the ORIGINAL cells' columns, the same `means_from_sums`, `nearest_zone_d2` over the
    reference cells' own coordinates (cell 20), the bins of `pd.cut` (cells 21-22).  -> `TableFeatures`: `rows` count cell pairs per
    group of the moving CELL (`group_by`: a column of `moving_mc.original_df` or an array over its rows; None: its `cell_type_col`);
    `pairs` (per_pair) is indexed by the moving cell id and carries `ref_id`, the reference cell id, and with `zones`
    `distance_to_zone`.  `moving_features` / `ref_features`: a DataFrame on the object's `original_df` index, an (n_cells, F) array or
    a list of `original_df` column names; the masks of `zones` are per cell."""
    checked_unpack(strategy, ref_mc, moving_mc)
    if strategy is None:
        raise ValueError("strategy must be 'nearest' or 'distribute'")
    spec = _spec if _spec is not None else unpack_spec(ref_mc, moving_mc, moving_features, ref_features, group_by, zones)
    _rec, cells = score_unpacked(table, ref_mc, moving_mc, strategy)
    if len(cells):
        rows_m = _frame_rows(moving_mc.original_df[moving_mc.original_idx_col].to_numpy(), cells["Aligned_cell_id"].to_numpy(), "moving")
        rows_r = _frame_rows(ref_mc.original_df[ref_mc.original_idx_col].to_numpy(), cells["Ref_cell_id"].to_numpy(), "reference")
    else:
        rows_m = rows_r = np.zeros(0, np.int64)
    ref_xy = ref_mc.original_df[[ref_mc.x_col, ref_mc.y_col]].to_numpy(dtype=np.float64) if spec.zone is not None else None
    words, d2 = host_words(spec, rows_m, rows_r, ref_xy)
    return _cell_frames(spec, ref_mc, moving_mc, rows_m, rows_r, words, d2, per_pair)


# ---- on the device -------------------------------------------------------------------------------------------------------------------------
class FeatureScores(DeviceScores):
    """`scores.DeviceScores` whose `record` makes the feature call beside the score call (windows.MergeAccumulator.score_features):
    the words of every result (`words`, in the jobs' order) and with per_pair its rows and squared distances (`pairs`)."""

    def __init__(self, score_delaunay, vertex_col, params, spec, per_pair, unpack=None, ref_mc=None, moving_mc=None):
        super().__init__(score_delaunay, vertex_col, params, tables=False, unpack=unpack, ref_mc=ref_mc, moving_mc=moving_mc)
        self.spec, self.per_pair = spec, bool(per_pair)
        # windows.DeviceScoreFeatures, windows.DeviceFeatureZone (with `unpack`: DeviceUnpackFeatures, DeviceUnpackZone) once `prepare` agreed
        self.feats = self.zone = None
        self.words, self.pairs = [], []

    def prepare(self, frames, job):
        """`DeviceScores.prepare`, then the feature columns, groups and zone resident beside the sections; False beyond the library's
        caps and for a zone over non-finite reference XY"""
        if not self.spec.device_ok or not super().prepare(frames, job):
            return False
        s = self.spec
        if self.unpack is not None:
            # per original cell -> the member lists' CSR order, once (`prepare` made the members: `.rows` are their rows of original_df)
            mm, rm = self.members
            at = lambda x, rows: None if x is None else x[rows]
            zone = None if s.zone is None else (s.zone[0][mm.rows], s.zone[1][rm.rows], s.zone[2])
            self.feats, self.zone = frames.unpack_features(mm, rm, at(s.mov_q, mm.rows), at(s.ref_q, rm.rows), s.group_codes[mm.rows],
                                                           s.n_groups, zone)
            return True
        self.feats, self.zone = frames.score_features(s.mov_q, s.ref_q, s.group_codes, s.n_groups, None if s.zone is None else s.zone[:3])
        return True

    def unpacked(self, acc):
        """`DeviceScores.unpacked` by ONE call in the unpack call's place (windows.MergeAccumulator.unpack_features): its counts are the
        record's cell keys, its words the result's sums; with per_pair the pairs' rows in the two `original_df`s and d2 per moving cell"""
        mm, rm = self.members
        counts, words, d2, ref_member = self._infeasible_as_the_reference(
            lambda: acc.unpack_features(mm, rm, self.unpack, self.feats, self.zone, d2=self.per_pair and self.zone is not None,
                                        pairs=self.per_pair))
        self.words.append(words)
        if self.per_pair:
            a = acc.final_rows()["a_row"].astype(np.int64) if acc.n_final else np.zeros(0, np.int64)
            n_a = mm.off[a + 1] - mm.off[a]
            within = np.arange(int(n_a.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_a) - n_a, n_a)
            rows_m, rows_r = mm.rows[np.repeat(mm.off[a], n_a) + within], rm.rows[ref_member]
            d2_cell = None
            if d2 is not None:
                d2_cell = np.full(self.spec.n_mov, np.nan)
                d2_cell[rows_m] = d2
            self.pairs.append((rows_m, rows_r, d2_cell))
        return unpack_record(counts[1], counts[2])

    def record(self, frames, acc):
        rec = super().record(frames, acc)
        if self.unpack is not None:          # (`unpacked` made the call)
            return rec
        words, d2 = acc.score_features(frames.dmov, frames.dref, self.feats, self.zone, d2=self.per_pair)
        self.words.append(words)
        if self.per_pair:
            final = acc.final_rows() if acc.n_final else {"a_row": np.zeros(0, np.int32), "r_row": np.zeros(0, np.int32)}
            self.pairs.append((final["a_row"].astype(np.int64), final["r_row"].astype(np.int64), d2))
        return rec

    def finished(self, frames):
        """the resident objects closed with the study: the zone before its features"""
        held = frames.__dict__.get("_score_features" if self.unpack is None else "_unpack_features", [])
        for made in (self.zone, self.feats):
            if made is not None:
                if made in held:
                    held.remove(made)
                made.close()
        self.feats = self.zone = None


def sliding_window_score_features(ref, moving, commonCT=None, *, moving_features=None, ref_features=None, group_by=None, zones=None,
                                  per_pair=False, type_variants=None, param_sets=None, optim_params=None, gurobi_params=None,
                                  score_delaunay=None, score_delaunay_vertex_col=None, score_params=None, workers=None, triangulator=None,
                                  ctx=None, batch=None, moving_delaunay=None, moving_delaunay_vertex_col=None, unpack=None):
    """`sliding_window_scores` with every result read as feature means of its matched pairs as well, over the same one pass of the
    windows and without a table: -> `ScoreFeatures`
      scores      `sliding_window_scores`' frame for the same arguments;
      rows, means, sums   `rows[v][s]`, `means[v][s]`, `sums[v][s]`: `score_table_features`' of result (variant v, set s) -- pairs per
                  group, and one frame each with groups as rows and the feature columns `moving_<name>`, `ref_<name>`;
      resolution  per feature column what its values were rounded to a multiple of (2**-e; the module states the error of a mean);
      zones       with `zones`: `zones[v][s]` that result's `ZoneReading` per distance bin; else None;
      pairs       with per_pair: `pairs[v][s]`, indexed like the moving frame: `ref_id` and with `zones` `distance_to_zone`; else None.
    `moving_features`, `ref_features`: a DataFrame on the frame's index, an (n, F) array or a list of the frame's own column names, of
    any float or integer dtype; at least one side.  Without `unpack` MetaCell objects are read at metacell level: the features are per
    row of their `metacell_df`.  `group_by`: `score_details.checked_groups`'; None: the moving frame's `cell_type`.  `zones`: `FeatureZones(
    zone_moving, zone_ref, subset_moving, subset_ref, edges, labels=None)` -- four boolean masks per row (None: all), `edges` the
    distances as given to `pd.cut`.  The other keywords are `sliding_window_scores`' but for `tables`.  A value that is not
    finite, a wrong length, a mask of the wrong length, edges that decrease and what `sliding_window_scores` refuses raise ValueError
    before a job or a device is touched.
    A column with one huge outlier loses its small values: see `resolution`.
    On the device one call per result beside the score call sums the fixed-point columns where the merged rows are
    (csrc/window_score_feature.hip).  What `scores.DeviceScores.prepare` refuses, more columns or groups than the library's caps (4096,
    256), a job off the shared pass and non-finite reference XY with `zones` go through `score_table_features` on the tables: the same
    frames, nothing saved.
    `unpack` ("nearest" / "distribute"; `ref` and `moving` MetaCell objects, `scores.checked_unpack`): the reading at CELL level, as
    examples/luad/reproduce_figures.ipynb cells 12-22 make it.  `moving_features` and `ref_features` are then per ORIGINAL cell -- a
    DataFrame on the object's `original_df` index, an (n_cells, F) array or a list of `original_df` column names --, `group_by` is per
    moving cell (None: the cells' `cell_type_col`) and the masks of `zones` are per cell; a pair's position is its reference CELL's
    coordinates.  The rows are reordered into the member lists' CSR order once, before the upload.  Every frame counts cell pairs;
    `scores` carries `cells_matched`, `cell_type_matches` and `cell_accuracy`; `pairs[v][s]` is indexed by the moving cell id and
    carries `ref_id`, the reference cell id, and `distance_to_zone`.  One call per result in the unpack call's place sums where the
    unpack phases make the pairs (csrc/window_unpack_feature.hip); every frame equals `score_unpacked_features` of its table, which
    also serves what the device refuses: whatever `score_unpacked` serves, columns or groups over the caps, non-finite reference cell
    coordinates with `zones`, a job off the shared pass."""
    params = checked_score_params(score_params)
    ref_arg, moving_arg, ref_df, mov_df = _frames_of(ref, moving)
    for df, name in ((ref_df, "ref"), (mov_df, "moving")):
        if not isinstance(df, pd.DataFrame):
            raise ValueError(f"the {name} frame is no DataFrame")
    # (over plain frames: a ValueError that is a TypeError too, as the call raised for `unpack` before it had the keyword --
    # tests/test_score_features_cpu.py still asserts it; score_details does the same)
    checked_unpack(unpack, ref_arg, moving_arg, no_objects=_NoMetaCellObjects)
    if unpack is None:
        spec = FeatureSpec(ref_df, mov_df, moving_features, ref_features, group_by, zones)
    else:
        spec = unpack_spec(ref_arg, moving_arg, moving_features, ref_features, group_by, zones)
    hook = FeatureScores(score_delaunay, score_delaunay_vertex_col, params, spec, per_pair, unpack, ref_arg, moving_arg)
    scores, nested, hook = _scored_study(ref, moving, commonCT, type_variants=type_variants, param_sets=param_sets, optim_params=optim_params,
                                         gurobi_params=gurobi_params, score_delaunay=score_delaunay,
                                         score_delaunay_vertex_col=score_delaunay_vertex_col, score_params=params, tables=False,
                                         workers=workers, triangulator=triangulator, ctx=ctx, batch=batch, moving_delaunay=moving_delaunay,
                                         moving_delaunay_vertex_col=moving_delaunay_vertex_col, unpack=unpack, hook=hook)
    n_sets = len(nested[0])
    job = hook.job
    cid = job.optim_params["cell_id_col"]
    if hook.records is not None and unpack is not None:
        rows_of = lambda q: hook.pairs[q] if per_pair else (None, None, None)       # (rows in the two original_df, d2 per moving cell)
        got = [_cell_frames(spec, ref_arg, moving_arg, rows_of(q)[0], rows_of(q)[1], w, rows_of(q)[2], per_pair) for q, w in enumerate(hook.words)]
        flat = [(g.rows, g.means, g.sums, g.zones) for g in got]
        pairs = [g.pairs for g in got] if per_pair else None
    elif hook.records is not None:
        flat = [spec.frames(w) for w in hook.words]
        pairs = [spec.pair_frame(job.moving.index, job.ref[cid].to_numpy(), *p) for p in hook.pairs] if per_pair else None
    elif unpack is not None:                            # not read on the device: the host statement on every table
        got = [score_unpacked_features(t, ref_arg, moving_arg, unpack, per_pair=per_pair, _spec=spec) for per_set in nested for t in per_set]
        flat = [(g.rows, g.means, g.sums, g.zones) for g in got]
        pairs = [g.pairs for g in got] if per_pair else None
    else:
        got = [score_table_features(t, job.ref, job.moving, cell_id_col=cid, per_pair=per_pair, _spec=spec) for per_set in nested for t in per_set]
        flat = [(g.rows, g.means, g.sums, g.zones) for g in got]
        pairs = [g.pairs for g in got] if per_pair else None
    nest = lambda items: None if items is None else [items[q:q + n_sets] for q in range(0, len(items), n_sets)]
    part = lambda k: nest([f[k] for f in flat])
    return ScoreFeatures(scores, part(0), part(1), part(2), spec.resolution(), part(3) if spec.zone is not None else None, nest(pairs))
