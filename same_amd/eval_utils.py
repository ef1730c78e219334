"""eval_utils of the reference, same signatures.  check_triangle_violations (src/eval_utils.py:66-223): triangle orientation flips
after alignment, and which nodes sit in flipped triangles (optionally by a node-local majority rule); the triangle loop runs in
csrc/match.hip (tri_flip_stats_kernel); id bookkeeping and the per-node rule are host work on small arrays.  check_alignment
(src/eval_utils.py:6-53): the k-nearest-template label check, searched in csrc/align.hip."""
import numpy as np
import pandas as pd

from . import _lib, ops


def check_triangle_violations(outputDF, mc_align, aligned_id_col="aligned_metacell_index",
                              ref_id_col="matched_ref_index", mapped_x_col="mapped_x", mapped_y_col="mapped_y",
                              cell_type_col="cell_type", ignore_same_type_triangles=True, node_local=False,
                              majority_threshold=0.5, min_flips=1, verbose=False, ctx=None):
    outputDF = outputDF.copy()
    tri_ids = np.asarray(mc_align.metacell_delaunay)
    tri_ids = tri_ids.reshape(-1, 3) if tri_ids.size else np.zeros((0, 3), dtype=np.int64)
    mdf = mc_align.metacell_df
    n = len(mdf)
    node_index = pd.Index(mdf.index)
    # node = position in metacell_df; ids absent from it cannot be processed (the reference's `except: continue`)
    tri_pos = node_index.get_indexer(tri_ids.reshape(-1)).reshape(-1, 3)
    has_node = (tri_pos >= 0).all(axis=1)
    # rows of outputDF per aligned id; the dict comprehensions of the reference keep the LAST row per id
    ids = outputDF[aligned_id_col].to_numpy()
    out_pos = node_index.get_indexer(ids)
    matched = np.zeros(n, np.uint8)
    last_row = np.full(n, -1, np.int64)
    ok = out_pos >= 0
    last_row[out_pos[ok]] = np.flatnonzero(ok)
    matched[out_pos[ok]] = 1
    mapped = np.zeros((n, 2))
    rows = last_row[last_row >= 0]
    mapped[last_row >= 0, 0] = outputDF[mapped_x_col].to_numpy(dtype=np.float64)[rows]
    mapped[last_row >= 0, 1] = outputDF[mapped_y_col].to_numpy(dtype=np.float64)[rows]
    type_id = None
    if ignore_same_type_triangles:
        codes = pd.factorize(outputDF[cell_type_col].to_numpy(), use_na_sentinel=False)[0].astype(np.int32)
        type_id = np.full(n, -1, np.int32)
        type_id[last_row >= 0] = codes[rows]
    axy = mdf[["X", "Y"]].to_numpy(dtype=np.float64)

    tris = tri_pos[has_node].astype(np.int32)
    flag, node_tri, node_flip = ops.tri_flip_stats(axy, mapped, matched, tris, type_id, ctx=ctx)
    all_matched = (flag & 1).astype(bool)
    same = (flag & 2).astype(bool)
    flipped = (flag & 4).astype(bool)
    # triangles whose three ids are in outputDF but not all in metacell_df: counted, then skipped
    lost = ~has_node
    lost_matched = 0
    lost_same = 0
    if lost.any():
        full = np.isin(tri_ids[lost], ids).all(axis=1)
        lost_matched = int(full.sum())
        if ignore_same_type_triangles and lost_matched:
            ct = outputDF[cell_type_col].to_numpy()
            lastrow_of = {v: r for r, v in enumerate(ids)}
            for tri in tri_ids[lost][full]:
                t0, t1, t2 = (ct[lastrow_of[v]] for v in tri)
                lost_same += int(t0 == t1 == t2)

    considered = all_matched & ~same
    sign_flips = flipped[considered]
    unique_ids = outputDF[aligned_id_col].unique()
    upos = node_index.get_indexer(unique_ids)
    n_tri = np.where(upos >= 0, node_tri[np.maximum(upos, 0)], 0).astype(np.int64)
    n_flip = np.where(upos >= 0, node_flip[np.maximum(upos, 0)], 0).astype(np.int64)
    if node_local:
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = n_flip / n_tri
        viol = (n_tri > 0) & (n_flip >= min_flips) & (frac >= majority_threshold)
    else:
        viol = n_flip > 0
    node_in_violating_triangle = dict(zip(unique_ids.tolist(), viol.tolist()))
    outputDF["in_violating_triangle"] = outputDF[aligned_id_col].map(node_in_violating_triangle).fillna(False)
    stats = {
        "total_triangles": len(tri_ids),
        "triangles_with_all_matched": int(all_matched.sum()) + lost_matched,
        "triangles_processed": int(all_matched.sum()) + lost_matched,
        "triangles_same_type_skipped": int(same.sum()) + lost_same,
        "triangles_flipped": int(np.sum(sign_flips)) if len(sign_flips) else 0,
        "percent_flipped": (100.0 * np.sum(sign_flips) / len(sign_flips) if len(sign_flips) else 0.0),
        "nodes_in_violating_triangles": int(outputDF["in_violating_triangle"].sum()),
        "percent_nodes_violating": 100.0 * outputDF["in_violating_triangle"].mean(),
    }
    if verbose:
        print(stats)
    return outputDF, stats


def _knn_count(kNN):
    """the k that cKDTree.query(k=kNN) reads: an integral number >= 1"""
    if isinstance(kNN, (bool, np.bool_, int, np.integer)) or (isinstance(kNN, (float, np.floating)) and float(kNN).is_integer()):
        k = int(kNN)
        if k >= 1:
            return k
    raise ValueError(f"kNN must be an integer >= 1, got {kNN!r}")


def _label_codes(q_labels, t_labels):
    """int32 codes of the query and template labels whose equality is Python `==` of the labels: pd.factorize merges values that
    compare equal (1 == 1.0 == True, '1' != 1); None equals None; NaN and every other missing value equal nothing (-1 on the query
    side, -2 on the template side)."""
    both = pd.concat([pd.Series(q_labels).reset_index(drop=True), pd.Series(t_labels).reset_index(drop=True)], ignore_index=True)
    codes, uniques = pd.factorize(both)
    codes = codes.astype(np.int32)
    missing = np.flatnonzero(codes < 0)
    if len(missing):
        is_none = np.asarray(both.to_numpy(dtype=object)[missing] == None, dtype=bool)  # noqa: E711 (elementwise)
        codes[missing] = np.where(is_none, len(uniques), np.where(missing < len(q_labels), -1, -2))
    return codes[:len(q_labels)], codes[len(q_labels):]


def check_alignment(queryDF, templateDF, xcol, ycol, ctype_col="cell_type", kNN=1, *, ctx=None, return_stats=False):
    """eval_utils.check_alignment (src/eval_utils.py:6-53), same signature and result: is the query cell's label among the labels of
    its kNN nearest template cells (cKDTree.query(k=kNN))?  Returns (queryDF copy with `_{kNN}NN_match` -- and, for kNN == 1,
    `_1NN_match_ctype`, the nearest template cell's label --, the column's mean); return_stats=True adds a dict of row counts.

    The search runs in csrc/align.hip (same_check_alignment), which decides every row whose answer does not depend on how scipy
    orders (nearly) equidistant template points; the rows in doubt are asked of cKDTree itself, built as the reference builds it."""
    queryDF = queryDF.copy()
    required = {xcol, ycol, ctype_col}
    if not required.issubset(queryDF.columns) or not required.issubset(templateDF.columns):
        raise ValueError(f"Both DataFrames must contain the columns: {required}")
    txy = templateDF[[xcol, ycol]].to_numpy(dtype=np.float64)
    if not np.isfinite(txy).all():
        raise ValueError("data must be finite, check for nan or inf values")
    qxy = queryDF[[xcol, ycol]].to_numpy(dtype=np.float64)
    if not np.isfinite(qxy).all():
        raise ValueError("'x' must be finite, check for nan or inf values")
    k = _knn_count(kNN)
    if k > _lib.ALIGN_MAX_KNN:
        raise ValueError(f"kNN={kNN} exceeds the device cap SAME_ALIGN_MAX_KNN = {_lib.ALIGN_MAX_KNN}")
    n_q, n_t = len(qxy), len(txy)
    if n_q and k > n_t:   # the reference's .iloc of scipy's missing-neighbour index n_t
        raise IndexError("single positional indexer is out-of-bounds" if k == 1 else "positional indexers are out-of-bounds")
    ctx = ctx if ctx is not None else _lib.default_context()
    qcode, tcode = _label_codes(queryDF[ctype_col].to_numpy(), templateDF[ctype_col].to_numpy())
    col = "_" + str(kNN) + "NN_match"
    n_doubt = 0
    if n_q:
        flag, nearest = ops.check_alignment(qxy, qcode, txy, tcode, k, ctx=ctx)
        match = (flag & _lib.ALIGN_MATCH).astype(bool)
        doubt = np.flatnonzero((flag & _lib.ALIGN_DECIDED) == 0)
        n_doubt = len(doubt)
        if n_doubt:
            from scipy.spatial import cKDTree

            _, idx = cKDTree(templateDF[[xcol, ycol]]).query(qxy[doubt], k=k)
            if k == 1:
                nearest[doubt] = idx
                match[doubt] = tcode[idx] == qcode[doubt]
            else:
                match[doubt] = (tcode[idx] == qcode[doubt, None]).any(axis=1)
    else:
        match, nearest = [], np.zeros(0, np.intp)
    queryDF.loc[:, col] = match
    if kNN == 1:
        queryDF.loc[:, "_" + str(kNN) + "NN_match_ctype"] = templateDF[ctype_col].iloc[nearest].values
    alignment_score = queryDF[col].mean()
    if not return_stats:
        return queryDF, alignment_score
    return queryDF, alignment_score, {"rows": n_q, "rows_decided_on_device": n_q - n_doubt, "rows_resolved_on_host": n_doubt, "kNN": k}
