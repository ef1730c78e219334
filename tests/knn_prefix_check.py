"""A plain host statement of csrc/window_knn_prefix.hip (same_window_knn_prefix), for the tests: a staged window's pair list at a smaller
k, derived from the list as staged.  tests/test_window_sweep_cpu.py holds it against the reference's own prune at the smaller k
(oracle.knn_prune through tests/caller_check.host_stage) on the inputs the GPU tests use; tests/test_gpu_window_sweep.py holds the
library against a freshly staged window.  Not collected by pytest."""
import numpy as np

import caller_check as C


def prefix(rows, pairs, costs, ref_rows, k):
    """`rows` the ascending section rows of the window's kept aligned cells, `pairs` (P, 2) over (kept cell, reference of the window:
    its place among `ref_rows`, the reference rows in the box) with the rows ascending and every row's pairs in the prune's order,
    `costs` (P,) in pair order, all as staged at some k_staged >= `k`.  Every row keeps its first min(k, count) pairs; nothing else of
    the window changes: the kept cells (a row with a pair keeps one) and the reference rows in the box are those staged.
    -> dict: rows, ref_rows (as given), pairs, costs, prow (the rows' pair offsets), counts (cells kept, pairs), and the window's
    COMPACTED reference frame (src/utils.py:734-742: the references the kept pairs still name, ascending, renumbered) as frame_rows /
    frame_pairs -- what `ref_idx` under window_local_indices and the reference limits of "capacity" / "transport" are read over."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n, P = len(rows), len(pairs)
    per_row = np.bincount(pairs[:, 0], minlength=n)
    assert n == 0 or (per_row > 0).all()                                  # kept cells: every one has a pair
    assert P == 0 or (np.diff(pairs[:, 0]) >= 0).all()                    # rows ascending
    first = np.concatenate(([0], np.cumsum(per_row)))
    place = np.arange(P) - first[pairs[:, 0]]
    keep = place < int(k)
    out = pairs[keep]
    named = np.unique(out[:, 1])
    renumber = np.full(len(ref_rows), -1, np.int64)
    renumber[named] = np.arange(len(named))
    return dict(rows=np.asarray(rows), ref_rows=np.asarray(ref_rows), pairs=out, costs=np.asarray(costs)[keep],
                prow=np.concatenate(([0], np.cumsum(np.minimum(per_row, int(k))))), counts=(n, len(out)),
                frame_rows=np.asarray(ref_rows)[named], frame_pairs=np.column_stack((out[:, 0], renumber[out[:, 1]])))


def pair_d2(axy, rxy, pairs):
    """squared distance of every pair, the prune's expression (dx*dx + dy*dy in fp64)"""
    dx, dy = axy[pairs[:, 0], 0] - rxy[pairs[:, 1], 0], axy[pairs[:, 0], 1] - rxy[pairs[:, 1], 1]
    return dx * dx + dy * dy


# ---- the inputs of both test files: (family, box, radius, k_max, the smaller values of k) ---------------------------------------------
BASE_K, TIE_KMAX, CONTENTION_KMAX = 8, 200, 8


def smaller(k_max):
    """the values of k a list staged at k_max is cut to: 1, 2, k_max - 1, k_max, and 64 / 65 where k_max allows"""
    return sorted({k for k in (1, 2, 64, 65, k_max - 1, k_max) if 1 <= k <= k_max})


def families(oracle):
    """-> [(tag, case, box, radius, k_max)]: the base case's boxes (whole: 24 scan blocks; sliver: rows with one, two, three pairs;
    boxes that keep nothing), the tie family staged at 200 (the large-capacity prune path; four references exactly equidistant from every
    row), the contention family, and the sections whose kept-cell count is a scan block edge"""
    out = []
    base = C.base_case()
    for name, box in C.base_boxes(oracle).items():
        out.append((f"base/{name}", base, box, C.RADIUS, BASE_K))
    out.append(("base/empty", base, C.EMPTY_BOX, C.RADIUS, BASE_K))
    out.append(("tie", C.tie_case(), C.TIE_BOX, C.TIE_K[TIE_KMAX], TIE_KMAX))
    out.append(("contention", C.contention_case(), C.CONTENTION_BOX, C.CONTENTION_RADIUS, CONTENTION_KMAX))
    for n in C.EDGE_ROWS:
        case = C.edge_case(n)
        out.append((f"edge/{n}", case, case["box"], C.RADIUS, BASE_K))
    return out
