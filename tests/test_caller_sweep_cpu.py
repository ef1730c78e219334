"""The parameter sweep over a CALLER's triangulation (same_amd.sliding_window_sweep under hip_caller_delaunay="device";
csrc/window_caller.hip: same_window_caller_pairs) without a GPU:
 * the rule itself, from the oracle -- the reference's second compaction (tests/caller_check.window_statement) of the list pruned at k
   equals the k-NN prefix (tests/knn_prefix_check.prefix) of the list pruned at the largest knn pushed through the node mask made THERE
   -- on the very inputs tests/test_gpu_caller_sweep.py drives the library with, and that these inputs hold the shapes the kernel can go
   wrong at;
 * the entry point's declaration and binding;
 * the call sequence of windows.iter_device_windows with several sets and a DeviceCallerTris (stand-ins, as tests/test_window_walk_cpu.py)."""
import os
import types

import numpy as np
import pytest

import caller_check as C
import knn_prefix_check as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE, SAME = 15, True


def pair_costs(rows, rows_r, pairs):
    """a cost that names its pair: a function of the two SECTION rows, so equal costs <=> the same pair whatever list it stands in"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    return rows[pairs[:, 0]].astype(np.float64) * 4099.0 + rows_r[pairs[:, 1]].astype(np.float64) / 8.0


def through_mask(valid, pairs, costs):
    """the pair half of the second compaction (src/same.py:1055-1075): pairs of removed rows go, rows renumbered by the mask's prefix sum"""
    new = np.cumsum(valid) - 1
    keep = valid[pairs[:, 0]] if len(pairs) else np.zeros(0, bool)
    return np.column_stack((new[pairs[keep, 0]], pairs[keep, 1])), np.asarray(costs)[keep]


def family_boxes(oracle):
    """-> [(tag, case, box)]: every box of C.base_boxes and C.mixed_boxes over the base case, the full box of every C.edge_case size"""
    base = C.base_case()
    out = [(f"base/{name}", base, box) for name, box in C.base_boxes(oracle).items()]
    out += [(f"mixed/{q}/{kind}", base, box) for q, (kind, box) in enumerate(C.mixed_boxes(oracle))]
    out += [(f"edge/{n}", C.edge_case(n), C.edge_case(n)["box"]) for n in C.EDGE_ROWS]
    return out


@pytest.fixture(scope="module")
def checked(oracle):
    """per (box, k): the statement at k against prefix + mask of the statement at C.KNN; -> the records the shape test reads"""
    records, seen = [], {}
    for tag, case, box in family_boxes(oracle):
        if box in seen:                                        # (C.mixed_boxes repeats its empty and its no-triangle box)
            records += [dict(r, tag=tag) for r in seen[box]]
            continue
        mov_xy, ref_xy, tris = case["mov_xy"], case["ref_xy"], case["tris"]
        rows, rows_r, pairs = C.host_stage(mov_xy, ref_xy, box, C.RADIUS, C.KNN, oracle)
        costs = pair_costs(rows, rows_r, pairs)
        tid = case["type_id"][rows]
        sel, valid, n_left, _pairs2, _costs2, tris2 = C.window_statement(rows, tris, mov_xy[rows], tid, pairs, costs, C.RADIUS, ANGLE, SAME, oracle)
        per_row = np.bincount(pairs[:, 0], minlength=len(rows))
        mine = []
        for k in K.smaller(C.KNN):
            cut = K.prefix(rows, pairs, costs, rows_r, k)
            want_pairs, want_costs = through_mask(valid, cut["pairs"], cut["costs"])
            # the reference's own: pruned at k, then its second compaction
            rows_k, rows_r_k, pairs_k = C.host_stage(mov_xy, ref_xy, box, C.RADIUS, k, oracle)
            assert np.array_equal(rows_k, rows) and np.array_equal(rows_r_k, rows_r), (tag, k)
            got = C.window_statement(rows_k, tris, mov_xy[rows_k], case["type_id"][rows_k], pairs_k, pair_costs(rows_k, rows_r_k, pairs_k),
                                     C.RADIUS, ANGLE, SAME, oracle)
            g_sel, g_valid, g_left, g_pairs, g_costs, g_tris = got
            assert np.array_equal(g_sel, sel) and np.array_equal(g_valid, valid) and g_left == n_left, (tag, k)
            assert g_pairs.shape == want_pairs.shape and np.array_equal(g_pairs, want_pairs), (tag, k)
            assert np.array_equal(g_costs, want_costs), (tag, k)
            assert np.array_equal(g_tris, tris2), (tag, k)
            removed_long = int(np.count_nonzero(~valid & (per_row > k)))
            mine.append(dict(tag=tag, k=k, rows=len(rows), removed=int((~valid).sum()), removed_long=removed_long, selected=len(sel),
                             left=n_left, pairs=len(want_pairs), pairs_cut=len(cut["pairs"])))
        seen[box] = mine
        records += mine
    return records


def test_second_compaction_commutes_with_the_knn_prefix(checked):
    tags = {r["tag"] for r in checked}
    assert {f"base/{n}" for n in ("whole", "interior", "sliver", "beside", "no triangle")} <= tags
    assert sum(t.startswith("mixed/") for t in tags) == 23 and {f"edge/{n}" for n in C.EDGE_ROWS} <= tags
    assert {r["k"] for r in checked} == set(K.smaller(C.KNN)) == {1, 2, 5, 6}


def test_inputs_hold_what_the_kernel_can_go_wrong_at(checked):
    by = {(r["tag"], r["k"]): r for r in checked}
    # removed nodes whose rows hold more than k pairs: whole rows go out of the middle of a list every row of which is cut
    for k in (1, 2, 5):
        assert by[("base/whole", k)]["removed_long"] > 0 and by[("base/interior", k)]["removed_long"] > 0, k
    whole = by[("base/whole", 2)]
    assert 0 < whole["removed"] < whole["rows"] and whole["pairs"] < whole["pairs_cut"] and whole["rows"] > 20 * 256
    # every node removed; a box without triangles (the same box: no triangle, no valid node); boxes without kept cells
    gone = by[("base/no triangle", 1)]
    assert gone["rows"] > 0 and gone["selected"] == 0 and gone["removed"] == gone["rows"] and gone["pairs"] == 0 and gone["pairs_cut"] > 0
    assert by[("base/beside", 1)]["rows"] == 0
    kinds = {t.split("/")[2] for t, _k in by if t.startswith("mixed/")}
    assert kinds == {"job", "cells", "empty", "no triangle"}
    assert all(by[(t, 1)]["rows"] == 0 for t, k in by if t.endswith("/empty") and k == 1)
    # the scan over the staged kept cells at block edges
    assert [by[(f"edge/{n}", 1)]["rows"] for n in C.EDGE_ROWS] == [255, 256, 257, 16385]
    assert all(by[(f"edge/{n}", 2)]["left"] > 0 for n in C.EDGE_ROWS)


def test_entry_point_is_declared_and_bound():
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "int same_window_caller_pairs(same_window *const *windows, int n_windows, int64_t *out_counts);" in header
    assert _lib._PROTOTYPES["same_window_caller_pairs"] == [_lib.c_vp, _lib.c_int, _lib.c_vp]
    assert hasattr(_lib.load(), "same_window_caller_pairs") and _lib.load().same_abi_version() == 9
    from same_amd import windows as W

    assert callable(W.caller_pairs_windows)


# ---- the walk's call sequence ----------------------------------------------------------------------------------------------------------
KEPT = (4, 5, 0, 7, 8)          # kept aligned cells per window as staged; a kept cell has `knn` pairs, so window 2 is staged without pairs
ALL_REMOVED = 1                 # the window whose every node is unconstrained: skipped
PLAN = [dict(box=(float(q), 0.0, 0.0, 0.0), window_id=q) for q in range(len(KEPT))]


class _State:
    def __init__(self, ctx=None):
        self.ctx, self.counts, self.n_triangles, self.n_staged_pairs, self.n_selected = ctx, (0, 0, 0, 0), 0, 0, 0
        self.assignment = self.refine = self.priority = None
        self.order_ties = 0

    def fetch(self, what):
        from same_amd import windows as W

        n = self.counts[2]
        return {W._W_ALIGNED_ROWS: np.arange(n, dtype=np.int32), W._W_ALIGNED_XY: np.zeros((n, 2))}[what]

    def close(self):
        pass


@pytest.fixture
def walk(monkeypatch):
    from same_amd import delaunay
    from same_amd import windows as W

    log = []

    def stage_windows(states, moving, ref, boxes, radius, knn, dist_ct_coeff):
        log.append(("stage", [int(b[0]) for b in boxes], knn))
        for s, box in zip(states, boxes):
            s.wid, s.kept, s.left, s.per_row = int(box[0]), KEPT[int(box[0])], None, knn
            s.counts, s.n_triangles, s.n_staged_pairs, s.priority = (s.kept + 3, s.kept + 2, s.kept, s.kept * knn), 0, s.kept * knn, None
        return [s.counts for s in states]

    def prefix_windows(states, k):
        log.append(("prefix", [s.wid for s in states], k))
        for s in states:
            s.per_row = k
            s.counts, s.n_triangles, s.n_staged_pairs, s.priority = s.counts[:2] + (s.kept, s.kept * k), 0, s.kept * k, None
        return [s.counts for s in states]

    def priority_windows(states):
        log.append(("priority", [s.wid for s in states], None))
        for s in states:
            staged = s.counts[3]
            s.per_row -= 0.5 if staged else 0
            s.counts = s.counts[:3] + (int(s.kept * s.per_row),)
            s.priority = (staged, s.counts[3], 1 if staged else 0, max(s.kept - 1, 0))
        return [s.priority for s in states]

    def compacted(s):
        s.left = 0 if s.wid == ALL_REMOVED else s.kept - 1
        s.n_selected, s.n_triangles = 3, 0
        s.counts = s.counts[:2] + (s.left, int(s.left * s.per_row))
        return (3, s.kept - s.left, 0, s.left, s.counts[3], 2)

    def caller_tris_windows(states, caller, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, removed=None):
        log.append(("caller_tris", [s.wid for s in states], None))
        assert removed is None
        return [compacted(s) for s in states]

    def caller_pairs_windows(states):
        log.append(("caller_pairs", [s.wid for s in states], None))
        assert all(s.left is not None and s.counts[2] == s.kept for s in states)       # compacted once, cut since
        return [compacted(s) for s in states]

    def filter_finish_windows(states, simplices, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, no_match_penalty,
                              ensure_min_triangle_per_node=True, prefiltered=False, mode=None, from_caller=False):
        log.append(("finish", [s.wid for s in states], no_match_penalty))
        assert simplices is None and from_caller and not prefiltered
        assert all(s.counts[2] == s.left for s in states)                               # the compacted window
        out = []
        for s in states:
            s.order_ties, s.n_triangles, s.assignment, s.refine = 0, 2, None, None
            out.append((2, 0, 0, np.zeros(s.left, np.int32), np.zeros(s.left, np.uint8), {"matched": s.left, "pairs": s.counts[3]}))
        return out

    class Caller(W.DeviceCallerTris):
        def __init__(self):
            self.handle = None

    monkeypatch.setattr(W, "DeviceWindow", _State)
    for stand_in in (stage_windows, prefix_windows, priority_windows, caller_tris_windows, caller_pairs_windows, filter_finish_windows):
        monkeypatch.setattr(W, stand_in.__name__, stand_in)

    def run(**kw):
        del log[:]
        kw.setdefault("caller", Caller())
        results = list(W.iter_device_windows(None, None, None, None, PLAN, ctx=types.SimpleNamespace(), batch=2,
                                             triangulator=delaunay.Triangulator(), **kw))
        return list(log), results

    return run


def _sets():
    from same_amd.window_mode import WindowMode

    search = WindowMode(refine="local", rounds=4, delaunay_penalty=5.0)
    return [(4, None, 100.0), (8, search, 100.0), (4, search, 30.0), (2, None, 100.0), (8, None, 30.0)]


def _expected(priority):
    """per batch: stage at 8, [priority], ONE caller_tris over the windows with pairs, the finishes of the knn-8 sets over the windows
    left with pairs; then per further knn: prefix, [priority], caller_pairs, its sets' finishes"""
    out = []
    for staged, with_pairs, live in (([0, 1], [0, 1], [0]), ([2, 3], [3], [3]), ([4], [4], [4])):
        out.append(("stage", staged, 8))
        out += [("priority", staged, None)] if priority else []
        out.append(("caller_tris", with_pairs, None))
        out += [("finish", live, 100.0), ("finish", live, 30.0)]                        # sets 1, 4
        out.append(("prefix", live, 4))
        out += [("priority", live, None)] if priority else []
        out.append(("caller_pairs", live, None))
        out += [("finish", live, 100.0), ("finish", live, 30.0)]                        # sets 0, 2
        out.append(("prefix", live, 2))
        out += [("priority", live, None)] if priority else []
        out += [("caller_pairs", live, None), ("finish", live, 100.0)]                   # set 3
    return out


@pytest.mark.parametrize("priority", [False, True], ids=["plain", "priority prune"])
def test_several_sets_over_a_callers_triangulation_share_the_selection(walk, priority):
    """fails without the feature: iter_device_windows refuses several sets with a caller's triangulation"""
    log, results = walk(sets=_sets(), priority=priority)
    assert log == _expected(priority)
    # per batch the results come set by set in the order the sets are taken, one per window each
    order = [1, 4, 0, 2, 3]
    want = [(q, w) for batch in ([0, 1], [2, 3], [4]) for q in order for w in batch]
    assert [(r.set, r.window["window_id"]) for r in results] == want
    for r in results:
        w, k = r.window["window_id"], _sets()[r.set][0]
        if w == 2:
            assert r.error is not None and r.state is None and not r.skipped
        elif w == ALL_REMOVED:                      # skipped for every set, in no later call, no state
            assert r.skipped and r.error is None and r.state is None and r.match_row is None and r.removed == KEPT[w]
        else:
            per_row = k - 0.5 if priority else k
            assert r.error is None and not r.skipped and r.removed == 1 and len(r.rows_m) == KEPT[w] - 1
            assert r.counts == (KEPT[w] + 3, KEPT[w] + 2, KEPT[w] - 1, int((KEPT[w] - 1) * per_row)) and r.stats["pairs"] == r.counts[3]
            assert (r.priority is not None) == priority and (not priority or r.priority[0] == KEPT[w] * k)
            assert len(r.match_row) == KEPT[w] - 1 and r.n_triangles == 2


def test_one_set_over_a_callers_triangulation_makes_the_plain_calls(walk):
    plain, _r = walk(knn=4, no_match_penalty=30.0)
    one, results = walk(sets=[(4, None, 30.0)])
    assert one == plain and all(r.set == 0 for r in results)
    assert not any(c[0] in ("prefix", "caller_pairs") for c in plain) and sum(c[0] == "caller_tris" for c in plain) == 3


def test_several_sets_need_a_device_triangulation_object(walk):
    with pytest.raises(ValueError):
        walk(sets=_sets(), caller=object())
    with pytest.raises(ValueError):
        walk(sets=_sets(), triangulate=False)
