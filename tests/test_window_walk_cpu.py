"""The call sequence of windows.iter_device_windows, without a device: the generator's control flow is plain Python over five names of
same_amd.windows (DeviceWindow, stage_windows, priority_windows, prefix_windows, filter_finish_windows) and a triangulator.  Stand-ins
for the five log (call, number of windows, knn or k, penalty, mode) and set the state fields the real ones set; the triangulator logs
the window id of every ticket.  A plan of five windows in batches of two whose third window is staged without pairs: one batch holds an
errored window, one batch is short.

Pinned: the plain form's sequence (with and without the priority prune), the `sets` form's, and that a list of one set makes the plain
form's calls.  With the priority prune a batch is pruned once right after its stage call -- over every staged window, the one without
pairs included -- and once after every prefix call: two prunes per batch for two knn groups.  The `variants` form (a `recost_windows`
stand-in beside the five) makes the steps of windows.batch_schedule batch by batch, and a batch without a live window makes its stage
call alone."""
import types

import numpy as np
import pytest

from same_amd import delaunay
from same_amd import windows as W
from same_amd.window_mode import WindowMode

KEPT = (4, 5, 0, 7, 8)          # kept aligned cells per window; a kept cell has `knn` pairs, so window 2 is staged without pairs
PLAN = [dict(box=(float(q), 0.0, 0.0, 0.0), window_id=q) for q in range(len(KEPT))]
DEFAULT = WindowMode.default()
SEARCH = WindowMode(refine="local", rounds=4, delaunay_penalty=5.0)


class _State:
    """what the walk reads of a DeviceWindow"""

    def __init__(self, ctx=None):
        self.ctx, self.counts, self.n_triangles, self.n_staged_pairs = ctx, (0, 0, 0, 0), 0, 0
        self.assignment = self.refine = self.priority = None
        self.order_ties = 0

    def fetch(self, what):
        n = self.counts[2]
        return {W._W_ALIGNED_ROWS: np.arange(n, dtype=np.int32), W._W_ALIGNED_XY: np.zeros((n, 2))}[what]

    def close(self):
        pass


@pytest.fixture
def walk(monkeypatch):
    """-> run(**arguments of iter_device_windows) -> (the calls in order, the results in order, the collector's argument tuples)"""
    log = []

    def stage_windows(states, moving, ref, boxes, radius, knn, dist_ct_coeff):
        log.append(("stage", len(states), knn, None, None))
        for s, box in zip(states, boxes):
            kept = KEPT[int(box[0])]
            s.kept, s.counts, s.n_triangles = kept, (kept + 3, kept + 2, kept, kept * knn), 0
            s.n_staged_pairs, s.priority, s.knn = kept * knn, None, knn
        return [s.counts for s in states]

    def recost_windows(states, dmoving, dref, layer, dist_ct_coeff):
        log.append(("recost", len(states), layer, None, None))
        return cut(states, states[0].knn)             # the window as a prefix call at the staged knn leaves it

    def prefix_windows(states, k):
        log.append(("prefix", len(states), k, None, None))
        return cut(states, k)

    def cut(states, k):
        for s in states:
            s.counts, s.n_triangles = s.counts[:3] + (s.kept * k,), 0
            s.n_staged_pairs, s.priority = s.kept * k, None
        return [s.counts for s in states]

    def priority_windows(states):
        log.append(("priority", len(states), None, None, None))
        for s in states:
            staged = s.counts[3]
            if staged:
                s.counts = s.counts[:3] + (staged - 1,)
            s.priority = (staged, max(staged - 1, 0), 1 if staged else 0, max(s.kept - 1, 0))
        return [s.priority for s in states]

    def filter_finish_windows(states, simplices, radius, angle_enabled, cos_thr, near_tol, ignore_same_type, no_match_penalty,
                              ensure_min_triangle_per_node=True, prefiltered=False, mode=None, from_caller=False):
        log.append(("finish", len(states), None, no_match_penalty, mode))
        assert simplices is not None and len(simplices) == len(states) and not prefiltered and not from_caller
        out = []
        for s in states:
            s.order_ties, s.n_triangles, s.assignment, s.refine = 0, 1, None, None
            out.append((1, 0, 0, np.zeros(s.kept, np.int32), np.zeros(s.kept, np.uint8), {"matched": s.kept, "pairs": s.counts[3]}))
        return out

    class Logging(delaunay.Triangulator):
        def submit(self, points, key=None):
            log.append(("ticket", key))
            return delaunay.Ticket(self, points, simplices=np.array([[0, 1, 2]], np.int32), native=False)

    monkeypatch.setattr(W, "DeviceWindow", _State)
    for stand_in in (stage_windows, recost_windows, prefix_windows, priority_windows, filter_finish_windows):
        monkeypatch.setattr(W, stand_in.__name__, stand_in)

    def run(plan=PLAN, ctx=None, triangulator=None, take=list, **kw):
        """`take`: what consumes the generator (tests/test_window_schedule_cpu.py abandons it)"""
        del log[:]
        collected = []
        kw.setdefault("collector", lambda *a: collected.append(a))
        results = take(W.iter_device_windows(None, None, None, None, plan, ctx=types.SimpleNamespace() if ctx is None else ctx, batch=2,
                                             triangulator=Logging() if triangulator is None else triangulator, **kw))
        return list(log), results, collected

    return run


def _batches(per_batch):
    """the three batches' calls: windows (0, 1), (2, 3) of which 2 has no pairs, (4,); per_batch(staged, with pairs, ids with pairs)"""
    return [c for staged, ids in ((2, (0, 1)), (2, (3,)), (1, (4,))) for c in per_batch(staged, len(ids), ids)]


def _plain_calls(knn=8, penalty=100.0, mode=DEFAULT, priority=False):
    return _batches(lambda staged, n, ids: [("stage", staged, knn, None, None)]
                    + ([("priority", staged, None, None, None)] if priority else [])
                    + [("ticket", q) for q in ids] + [("finish", n, None, penalty, mode)])


def test_plain_form(walk):
    """1: per batch `stage`, the tickets of the windows with pairs, one `finish`"""
    log, results, collected = walk()
    assert log == _plain_calls()
    assert [(r.window["window_id"], r.set, r.error is None) for r in results] == [(0, None, True), (1, None, True), (2, None, False),
                                                                                   (3, None, True), (4, None, True)]
    assert [r.counts[3] for r in results] == [8 * k for k in KEPT] and all(r.priority is None and r.mode is DEFAULT for r in results)
    assert all(r.state is not None and len(r.match_row) == KEPT[r.window["window_id"]] for r in results if r.error is None)
    assert results[2].state is None and results[2].match_row is None
    # the collector of the plain form takes two arguments: the states and the windows of the batch's finished windows
    assert [len(a) for a in collected] == [2, 2, 2]
    assert [[w["window_id"] for w in a[1]] for a in collected] == [[0, 1], [3], [4]]
    assert all(len(a[0]) == len(a[1]) for a in collected)


def test_plain_form_with_its_own_knn_mode_and_penalty(walk):
    log, results, _c = walk(knn=3, mode=SEARCH, no_match_penalty=30.0)
    assert log == _plain_calls(3, 30.0, SEARCH)
    assert all(r.mode is SEARCH and r.set is None for r in results)


def test_plain_form_with_the_priority_prune(walk):
    """2: per batch `stage`, `priority`, tickets, `finish` -- the prune comes before the tickets, over every staged window"""
    log, results, _c = walk(priority=True)
    assert log == _plain_calls(priority=True)
    assert [r.priority for r in results] == [(8 * k, max(8 * k - 1, 0), 1 if k else 0, max(k - 1, 0)) for k in KEPT]
    assert [r.counts[3] for r in results] == [max(8 * k - 1, 0) for k in KEPT]


SETS = [(2, None, 100.0), (8, None, 100.0), (2, SEARCH, 30.0), (1, None, 30.0)]


def test_sets(walk):
    """3: per batch `stage` at the largest knn, tickets, the knn-8 set's `finish`, `prefix 2`, two finishes, `prefix 1`, one finish;
    the results set by set in the order 1, 0, 2, 3, each with its own set's pair counts, the errored window once per set"""
    log, results, collected = walk(sets=SETS, knn=5, no_match_penalty=7.0, mode=SEARCH)        # (not read with `sets`)
    assert log == _batches(lambda staged, n, ids: [("stage", staged, 8, None, None)] + [("ticket", q) for q in ids]
                           + [("finish", n, None, 100.0, DEFAULT), ("prefix", n, 2, None, None), ("finish", n, None, 100.0, DEFAULT),
                              ("finish", n, None, 30.0, SEARCH), ("prefix", n, 1, None, None), ("finish", n, None, 30.0, DEFAULT)])
    order = [(s, q) for batch in ((0, 1), (2, 3), (4,)) for s in (1, 0, 2, 3) for q in batch]
    assert [(r.set, r.window["window_id"]) for r in results] == order
    for r in results:
        k, mode, _p = SETS[r.set]
        q = r.window["window_id"]
        assert r.mode is (DEFAULT if mode is None else mode) and r.priority is None
        assert (r.error is not None) == (q == 2) and not r.skipped
        if q != 2:
            assert r.counts[3] == KEPT[q] * k and r.stats["pairs"] == KEPT[q] * k and len(r.rows_m) == KEPT[q] == len(r.match_row)
    assert sum(r.error is not None for r in results) == len(SETS)
    # the collector of the `sets` form takes three: the states, the windows, the set's index
    assert [len(a) for a in collected] == [3] * 12 and [a[2] for a in collected] == [1, 0, 2, 3] * 3


def test_sets_with_the_priority_prune(walk):
    """4: per batch `stage`, `priority`, tickets, `finish`, `prefix`, `priority`, `finish`: two prunes for two groups, never three"""
    log, results, _c = walk(sets=[(8, None, 100.0), (2, None, 30.0)], priority=True)
    assert log == _batches(lambda staged, n, ids: [("stage", staged, 8, None, None), ("priority", staged, None, None, None)]
                           + [("ticket", q) for q in ids]
                           + [("finish", n, None, 100.0, DEFAULT), ("prefix", n, 2, None, None), ("priority", n, None, None, None),
                              ("finish", n, None, 30.0, DEFAULT)])
    for r in results:
        q, k = r.window["window_id"], (8, 2)[r.set]
        if q != 2:
            assert r.priority == (KEPT[q] * k, KEPT[q] * k - 1, 1, KEPT[q] - 1) and r.counts[3] == KEPT[q] * k - 1


def test_one_set_makes_the_calls_of_the_plain_form(walk):
    log, results, collected = walk(sets=[(8, None, 100.0)])
    assert log == _plain_calls()
    assert [(r.set, r.window["window_id"]) for r in results] == [(0, q) for q in range(5)]
    assert [len(a) for a in collected] == [3, 3, 3] and all(a[2] == 0 for a in collected)
    log, _r, _c = walk(sets=[(8, None, 100.0)], priority=True)
    assert log == _plain_calls(priority=True)


def test_several_sets_go_with_the_routes_own_triangulation_only(walk):
    with pytest.raises(ValueError):
        walk(sets=SETS, triangulate=False)
    with pytest.raises(ValueError):
        walk(sets=SETS, caller=object())
    with pytest.raises(ValueError):
        walk(sets=[])


VARIANTS = ["layer 0", None, "layer 2"]          # (the walk hands a layer to recost_windows and reads nothing of it)
VARIANT_SETS = [(8, None, 100.0, 0), (4, None, 100.0, 0), (8, SEARCH, 30.0, 1), (4, None, 100.0, 1), (4, None, 30.0, 2)]


def test_variants(walk):
    """5: per batch `stage 8`, the tickets, then the calls of windows.batch_schedule over the batch's live windows -- the None variant
    first, `recost` before each layered one, `prefix` where k differs --; the results in the schedule's finish order, one per window
    each, under their set's variant"""
    steps = W.batch_schedule([(8, 0), (4, 0), (8, 1), (4, 1), (4, 2)], [True, False, True], False, False)
    assert steps == [("finish", 2), ("prefix", 4), ("finish", 3), ("recost", 0), ("finish", 0), ("prefix", 4), ("finish", 1),
                     ("recost", 2), ("prefix", 4), ("finish", 4)]

    def call(n, kind, arg):
        if kind == "finish":
            _k, mode, penalty, _v = VARIANT_SETS[arg]
            return ("finish", n, None, penalty, DEFAULT if mode is None else mode)
        return (kind, n, VARIANTS[arg] if kind == "recost" else arg, None, None)

    log, results, collected = walk(sets=VARIANT_SETS, variants=VARIANTS)
    assert log == _batches(lambda staged, n, ids: [("stage", staged, 8, None, None)] + [("ticket", q) for q in ids]
                           + [call(n, *step) for step in steps])
    order = [(s, q) for batch in ((0, 1), (2, 3), (4,)) for s in (2, 3, 0, 1, 4) for q in batch]
    assert [(r.set, r.window["window_id"]) for r in results] == order
    for r in results:
        k, _m, _p, v = VARIANT_SETS[r.set]
        q = r.window["window_id"]
        assert r.variant == v and (r.error is not None) == (q == 2)
        if q != 2:
            assert r.counts[3] == KEPT[q] * k == r.stats["pairs"] and len(r.match_row) == KEPT[q]
    assert [a[2] for a in collected] == [2, 3, 0, 1, 4] * 3


def test_a_batch_without_a_live_window_makes_its_stage_call_alone(walk, monkeypatch):
    """6: windows 2 and 3 -- the second batch -- staged without pairs: `stage` and nothing else, no recost, prefix or prune over no
    window, no finish; every set still yields an errored result for each of the two"""
    monkeypatch.setitem(globals(), "KEPT", (4, 5, 0, 0, 8))
    for priority in (False, True):
        log, results, collected = walk(sets=VARIANT_SETS, variants=VARIANTS, priority=priority)
        at = log.index(("stage", 2, 8, None, None), 1)
        assert log[at + 1 + priority] == ("stage", 1, 8, None, None) and (not priority or log[at + 1] == ("priority", 2, None, None, None))
        second = results[10:20]
        assert [(r.set, r.window["window_id"]) for r in second] == [(s, q) for s in (2, 3, 0, 1, 4) for q in (2, 3)]
        assert all(r.error is not None and r.state is None and r.match_row is None for r in second)
        assert all(r.variant == VARIANT_SETS[r.set][3] and r.counts[3] == 0 for r in second)
        assert sum(r.error is not None for r in results) == 10 and len(results) == 25
        assert [[w["window_id"] for w in a[1]] for a in collected] == [[0, 1]] * 5 + [[4]] * 5
