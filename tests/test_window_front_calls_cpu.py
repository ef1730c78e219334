"""The input families of tests/caller_check.py, checked WITHOUT a GPU: every family has the property a GPU test of the window
path's two front calls (same_window_caller_tris, same_window_priority_pairs) at the library needs of it -- a box of more than 64
cells, a scan sized to a block edge, a row of 64+ pairs with equal distances, a contended reference ... -- by proof, not by luck.
The two host statements are held against the reference's own flow on these inputs too: tests/priority_check.device_rule against
same_amd.knn.priority_filter, caller_check's window statement against reference_flow of tests/test_caller_triangulation_cpu.py."""
import numpy as np
import pytest

import caller_check as C
from priority_check import device_rule


def _staged(case, box, oracle, radius=C.RADIUS, k=C.KNN):
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, radius, k, oracle)
    return rows, rows_r, pairs, case["mov_xy"][rows], case["type_id"][rows]


def _statement_equals_the_reference_flow(case, tris, rows, pairs, xy, tid, angle, same, oracle):
    from test_caller_triangulation_cpu import reference_flow

    costs = np.arange(len(pairs), dtype=np.float64)
    sel, valid, n_left, pairs2, costs2, tris2 = C.window_statement(rows, tris, xy, tid, pairs, costs, C.RADIUS, angle, same, oracle)
    kept = C.filtered_after(xy, tid, valid, tris2, C.RADIUS, angle, same, oracle)
    # (reference_flow remaps by vertex id: a section row is its own id here)
    want_tris, want_gone, want_pairs, want_n, _before = reference_flow(rows, tris, xy, tid, pairs, C.RADIUS, angle, same, oracle)
    assert np.array_equal(kept, want_tris) and np.array_equal(np.flatnonzero(~valid), want_gone) and n_left == want_n
    assert np.array_equal(pairs2, want_pairs)
    assert np.array_equal(costs2, costs[valid[pairs[:, 0]]])           # the costs ride with their pairs
    assert C.near_count(xy, sel, C.RADIUS, angle, oracle) == 0           # near == 0: the call compacts
    return sel, valid, tris2


@pytest.mark.parametrize("angle,same", [(15, True), (15, False), (None, True), (None, False)])
def test_base_case_windows(oracle, angle, same):
    case = C.base_case()
    boxes = C.base_boxes(oracle)
    n_tris = len(case["tris"])
    for name, box in boxes.items():
        rows, rows_r, pairs, xy, tid = _staged(case, box, oracle)
        if name == "beside":
            assert len(C.in_box(case["mov_xy"], box)) == len(rows_r) == 0
            continue
        assert len(rows) > 0 and len(pairs) >= len(rows)
        sel, valid, tris2 = _statement_equals_the_reference_flow(case, case["tris"], rows, pairs, xy, tid, angle, same, oracle)
        if name == "no triangle":            # (by construction the family without a triangle: every kept cell goes)
            assert len(sel) == 0 and not valid.any()
        else:
            assert (~valid).any() and len(tris2) > 0                      # a node is removed, a triangle is left
        if name == "whole":
            # the list's last triangles are the window's: a candidate list cut short at the tail would lose them
            inside = np.isin(case["tris"], rows).all(axis=1)
            assert inside[n_tris - case["n_unbinned"]:].all() and not inside[:4].any()
            assert len(sel) > 256 * 30 and valid.sum() > 256 * 20       # every scan of the call crosses many blocks
    # which (grid, box) leave the cell-run path
    over = {(g, b) for g, grid in C.GRIDS.items() for b, box in boxes.items() if C.cells_covered(box, grid, case["mov_xy"]) > 64}
    assert {("cell 25", "whole"), ("cell 40 off origin", "whole"), ("60 x 17", "whole")} <= over
    assert not any(g in ("cell 75", "one cell") for g, _b in over) and not any(b != "whole" for _g, b in over)
    assert C.cells_covered(boxes["whole"], C.GRIDS["one cell"], case["mov_xy"]) == 1
    # the unbinned triangles: those whose FIRST corner has no finite coordinates
    assert np.count_nonzero(~np.isfinite(case["mov_xy"][case["tris"][:, 0]]).all(axis=1)) == case["n_unbinned"]


def test_mixed_launch_group(oracle):
    case = C.base_case()
    boxes = C.mixed_boxes(oracle)
    assert len(boxes) == 23
    for g in range(0, 23, 8):
        assert {k for k, _b in boxes[g:g + 8]} == {"job", "cells", "empty", "no triangle"}
    for kind, box in boxes:
        cells = C.cells_covered(box, C.GRIDS["cell 25"], case["mov_xy"])
        rows, rows_r, pairs, xy, tid = _staged(case, box, oracle)
        if kind == "empty":
            assert len(C.in_box(case["mov_xy"], box)) == 40 and len(rows_r) == 40 and len(rows) == 0 and cells <= 64
            continue
        assert (cells > 64) == (kind == "job")
        sel, valid, tris2 = _statement_equals_the_reference_flow(case, case["tris"], rows, pairs, xy, tid, 15, True, oracle)
        assert (len(sel) == 0) == (kind == "no triangle") and len(rows) > 0
        if kind != "no triangle":
            assert (~valid).any() and len(tris2) > 0


@pytest.mark.parametrize("n", C.EDGE_ROWS)
def test_scan_edge_sections(oracle, n):
    case = C.edge_case(n)
    assert C.cells_covered(case["box"], case["grid"], case["mov_xy"]) > 64
    rows, rows_r, pairs, xy, tid = _staged(case, case["box"], oracle)
    assert len(rows) == n and np.array_equal(rows, np.arange(n)) and len(rows_r) == n            # every row kept: n0 == n exactly
    counts = C.edge_counts(n)
    assert set(counts) >= {m for m in (1, 255, 256, 257) if m <= len(case["tris"])} and len(counts) >= 4
    if n == C.EDGE_ROWS[-1]:
        assert set(C.EDGE_TRIANGLES) <= set(counts) and counts[-1] == len(case["tris"]) > 120 * 256
    for m in counts:
        sel, valid, tris2 = _statement_equals_the_reference_flow(case, case["tris"][:m], rows, pairs, xy, tid, 15, True, oracle)
        assert len(sel) == m                                                                     # n_cand == selected == m exactly
        assert len(tris2) > 0 and (~valid).any()
    # the prune on the same section: rows that win their own copy, rows whose label differs and keep all
    out, one, all_ = device_rule(pairs, xy, case["ref_xy"], case["code_m"], case["code_r"])
    assert one > 0 and all_ > 0 and one + all_ == n and len(out) < len(pairs)


@pytest.mark.parametrize("k", sorted(C.TIE_K))
def test_tie_family(oracle, k):
    from same_amd.knn import priority_filter

    case = C.tie_case()
    assert 590 <= len(case["ref_xy"]) <= 610
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], C.TIE_BOX, C.TIE_K[k], k, oracle)
    assert len(rows) == len(case["mov_xy"]) and len(rows_r) == len(case["ref_xy"])
    axy, rxy = case["mov_xy"], case["ref_xy"]
    per_row = np.bincount(pairs[:, 0])
    assert per_row.max() == k and np.count_nonzero(per_row == k) > 100            # rows fill k
    d = np.sqrt((axy[pairs[:, 0], 0] - rxy[pairs[:, 1], 0]) ** 2 + (axy[pairs[:, 0], 1] - rxy[pairs[:, 1], 1]) ** 2)
    full = int(np.flatnonzero(per_row == k)[0])
    mine = d[pairs[:, 0] == full]
    assert len(np.unique(mine)) * 4 <= max(len(mine), 4)                         # many exactly equal distances in one row
    if k > 1:
        assert np.count_nonzero(mine == mine.min()) == 4                          # four references exactly equidistant
    got, one, all_ = device_rule(pairs, axy, rxy, case["code_m"], case["code_r"])
    want, w_one, w_all = priority_filter(pairs, axy, rxy, C.labels_of(case["code_m"]), C.labels_of(case["code_r"]))
    assert np.array_equal(got, want) and (one, all_) == (w_one, w_all)
    assert one > 0 and all_ > 0
    for side in ("code_m", "code_r"):
        assert (case[side] == -1).any() and (case[side] == 0).any() and (case[side] == 1).any()
    assert ((case["code_m"][pairs[:, 0]] == -1) & (case["code_r"][pairs[:, 1]] == -1)).any()       # -1 on both sides of a pair
    # exact duplicates among the moving points
    assert len(np.unique(axy, axis=0)) < len(axy)


def test_contention_and_batch_families(oracle):
    from same_amd.knn import priority_filter

    case = C.contention_case()
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], C.CONTENTION_BOX, C.CONTENTION_RADIUS, C.CONTENTION_K, oracle)
    assert len(rows) == C.CONTENTION_ROWS > 2 * 256 and len(pairs) == 4 * C.CONTENTION_ROWS
    got, one, all_ = device_rule(pairs, case["mov_xy"], case["ref_xy"], case["code_m"], case["code_r"])
    want, w_one, w_all = priority_filter(pairs, case["mov_xy"], case["ref_xy"], C.labels_of(case["code_m"]), C.labels_of(case["code_r"]))
    assert np.array_equal(got, want) and (one, all_) == (w_one, w_all) == (1, C.CONTENTION_ROWS - 1)
    assert np.array_equal(got[0], (0, 0)) and np.count_nonzero(got[:, 0] == 0) == 1          # the lowest row keeps the one pair
    # the batch of 23 on the base case
    base, codes = C.base_case(), C.base_codes()
    boxes = C.priority_boxes()
    assert len(boxes) == 23
    for g in range(0, 23, 8):
        kinds = [k for k, _b in boxes[g:g + 8]]
        assert kinds[0] == "pairs" and kinds[-1] == "pairs" and {"no pairs", "nothing"} <= set(kinds[1:-1])
    sizes = set()
    for kind, box in boxes:
        rows, rows_r, pairs = C.host_stage(base["mov_xy"], base["ref_xy"], box, C.RADIUS, C.KNN, oracle)
        n_m = len(C.in_box(base["mov_xy"], box))
        if kind == "nothing":
            assert n_m == 0 and len(rows_r) == 0
        elif kind == "no pairs":
            assert n_m > 0 and len(rows_r) > 0 and len(pairs) == 0
        else:
            assert len(pairs) > 0
            sizes.add(len(rows))
            axy, rxy = base["mov_xy"][rows], base["ref_xy"][rows_r]
            got, one, all_ = device_rule(pairs, axy, rxy, codes["code_m"][rows], codes["code_r"][rows_r])
            want, w_one, w_all = priority_filter(pairs, axy, rxy, C.labels_of(codes["code_m"][rows]), C.labels_of(codes["code_r"][rows_r]))
            assert np.array_equal(got, want) and (one, all_) == (w_one, w_all) and one > 0 and all_ > 0
    assert len(sizes) >= 8 and max(sizes) > 5000 and min(sizes) < 256 < sorted(sizes)[-2], sorted(sizes)
