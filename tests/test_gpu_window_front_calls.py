"""same_window_caller_tris (csrc/window_caller.hip) and same_window_priority_pairs (csrc/window_priority.hip) driven at the LIBRARY, as
iter_device_windows drives them (W.stage_windows, W.priority_windows, W.DeviceCallerTris, W.caller_tris_windows, DeviceWindow.fetch, the
finish call with the caller's source), against the plain host statements of both rules (tests/caller_check.window_statement,
tests/priority_check.device_rule, same_amd.knn.priority_filter) -- at the shapes the product route never produces: boxes over more than
64 cells of the section's grid (every triangle of the job a candidate), grids that cut through boxes, launch groups that mix the two
candidate paths with windows that keep nothing, scans sized to a block edge and past one look-back window, rows of 65 and 200 pairs
with exactly equal distances, one reference 700 rows bid for.  Every comparison is exact: counts are the statement's, a fetched cost is
the staged cost of the same pair bit for bit.  The inputs come from tests/caller_check.py; tests/test_window_front_calls_cpu.py proves
without a GPU that each of them has the property its test is about."""
import functools

import numpy as np
import pytest

import caller_check as C
from priority_check import device_rule

pytestmark = pytest.mark.gpu

PENALTY = 50.0
ARRAYS = ("rows", "xy", "pairs", "costs")


def _W():
    from same_amd import windows as W

    return W


def _what(W):
    return dict(rows=W._W_ALIGNED_ROWS, xy=W._W_ALIGNED_XY, pairs=W._W_PAIRS, costs=W._W_COSTS)


@functools.lru_cache(maxsize=None)
def _device(name, dtype="float64"):
    """(moving DeviceSection, reference DeviceSection, case) of one input family, uploaded once per cost type; label codes set where the
    family has them"""
    W = _W()
    case = {"base": C.base_case, "tie": C.tie_case, "contention": C.contention_case}[name]() if isinstance(name, str) else C.edge_case(name)
    mov = W.Section(case["mov_xy"], case["types_m"], case.get("type_id"), case.get("size"))
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov, dtype), W.DeviceSection(ref, dtype)
    codes = C.base_codes() if name == "base" else case
    if "code_m" in codes:
        dmov.set_label_codes(codes["code_m"])
        dref.set_label_codes(codes["code_r"])
    return dmov, dref, case


def _filter_args(angle, same):
    from same_amd.triangles import cos_threshold

    en, thr = cos_threshold(angle)
    tol = float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0
    return (C.RADIUS, en, thr, tol, same)


def _fetch(st, W):
    return {k: st.fetch(w) for k, w in _what(W).items()}


def _same_arrays(a, b, tag):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


def _stage(st, dmov, dref, box, radius=C.RADIUS, k=C.KNN):
    """stage one window -> (counts, its arrays as staged)"""
    W = _W()
    counts = st.stage(dmov, dref, box, radius, k, 1.0)
    staged = _fetch(st, W)
    assert np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"])
    return counts, staged


def _staged_as_on_the_host(case, box, staged, oracle, radius=C.RADIUS, k=C.KNN):
    """the kept rows and every row's pair count are the host's (tests/caller_check.host_stage): what the CPU test proved of the host's
    list holds for the list the device staged"""
    rows, _rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, radius, k, oracle)
    assert np.array_equal(staged["rows"], rows) and len(staged["pairs"]) == len(pairs)
    assert np.array_equal(np.bincount(staged["pairs"][:, 0], minlength=len(rows)), np.bincount(pairs[:, 0], minlength=len(rows)))


def _statement(case, tris, staged, angle, same, oracle):
    """-> dict of what the caller call must leave, from the arrays as staged"""
    rows0 = staged["rows"]
    tid = case["type_id"][rows0]
    sel, valid, n_left, pairs2, costs2, tris2 = C.window_statement(rows0, tris, staged["xy"], tid, staged["pairs"].astype(np.int64),
                                                                   staged["costs"], C.RADIUS, angle, same, oracle)
    kept = C.filtered_after(staged["xy"], tid, valid, tris2, C.RADIUS, angle, same, oracle) if len(tris2) else np.zeros((0, 3), np.int64)
    return dict(sel=sel, valid=valid, rows=rows0[valid], xy=staged["xy"][valid], pairs=pairs2, costs=costs2, tris2=tris2, kept=kept,
                counts=(len(sel), int((~valid).sum()), 0, n_left, len(pairs2), len(tris2)))


def _check_caller(st, got, want, staged, tag):
    """the window after same_window_caller_tris against the statement: six counts, selected triangles, the compacted arrays"""
    W = _W()
    assert tuple(got) == want["counts"], (tag, got, want["counts"])
    assert np.array_equal(st.fetch(W._W_CALLER_TRIANGLES), want["sel"]), tag
    after = _fetch(st, W)
    for k in ARRAYS:
        assert after[k].dtype == staged[k].dtype and np.array_equal(after[k], want[k]), (tag, k)
    assert st.counts[2:] == (want["counts"][3], want["counts"][4]), tag
    return after


def _finish(st, angle, same, want=None, tag=None):
    """the finish call over the caller's triangles -> the record (counts, match, flags, stats, triangles, signs)"""
    W = _W()
    kept, added, near, row, flag, stats = W.filter_finish_windows([st], None, *_filter_args(angle, same), PENALTY, from_caller=True)[0]
    assert near == 0, tag
    tris = st.fetch(W._W_TRIANGLES)
    if want is not None:
        assert np.array_equal(tris, want["kept"]) and kept + added == len(want["kept"]), tag
    return dict(counts=(kept, added), row=row, flag=flag, stats=stats, tris=tris, signs=st.fetch(W._W_SIGNS), match=st.fetch(W._W_MATCH))


def _same_record(a, b, tag):
    assert a["counts"] == b["counts"] and a["stats"] == b["stats"], tag
    for k in ("row", "flag", "tris", "signs", "match"):
        assert np.array_equal(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("angle", [15, None], ids=["angle rule", "no angle rule"])
@pytest.mark.parametrize("same", [True, False], ids=["same-type rule", "no same-type rule"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_caller_call_does_not_depend_on_the_section_grid(oracle, dtype, same, angle):
    """The triangles are binned by the cell of their first corner on the grid the section had when the DeviceCallerTris was made.  The same
    sections and the same triangulation on five grids -- the window grid, small cells (the whole box covers 144 of them: every triangle
    of the job is a candidate), an origin off the data that cuts through the boxes, one cell over everything, unequal cell sides --:
    selected triangles, compacted rows / XY / pairs / costs and the six counts are the host statement's on every grid, and the finish
    call's record over the caller's triangles is the one of the window grid."""
    from same_amd import _lib

    W = _W()
    dmov, dref, case = _device("base", dtype)
    boxes = C.base_boxes(oracle)
    st = W.DeviceWindow()
    wants, records, launches = {}, {}, {}
    ctx = st.ctx
    try:
        for gname, grid in C.GRIDS.items():
            dmov.bin(*grid)
            dref.bin(*grid)
            caller = W.DeviceCallerTris(dmov, case["tris"])
            try:
                for bname, box in boxes.items():
                    tag = (gname, bname)
                    counts, staged = _stage(st, dmov, dref, box)
                    if bname == "beside":
                        # no row of either section: not staged as far as the caller call is concerned -- refused, nothing launched
                        assert counts == (0, 0, 0, 0)
                        with pytest.raises(_lib.SameHipError) as e:
                            W.caller_tris_windows([st], caller, *_filter_args(angle, same))
                        assert e.value.code == _lib.SAME_EINVAL
                        continue
                    if bname not in wants:
                        _staged_as_on_the_host(case, box, staged, oracle)
                        wants[bname] = (staged, _statement(case, case["tris"], staged, angle, same, oracle))
                    first, want = wants[bname]
                    _same_arrays(staged, first, tag)                            # (the stage call's own independence of the grid)
                    before = ctx.stats()["launches"]
                    got = W.caller_tris_windows([st], caller, *_filter_args(angle, same))[0]
                    launches[tag] = ctx.stats()["launches"] - before
                    _check_caller(st, got, want, staged, tag)
                    assert np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"]), tag
                    if bname in ("whole", "interior", "sliver"):
                        # the branch the LIBRARY took is the one tests/caller_check.cells_covered predicts: a box over more than 64 cells
                        # makes every triangle of the job a candidate and launches no rows kernel -- one launch fewer than on the window grid
                        over = C.cells_covered(box, grid, case["mov_xy"]) > 64
                        assert launches[tag] == launches[("cell 75", bname)] - (1 if over else 0), (tag, launches[tag], over)
                    if want["counts"][4] == 0:
                        assert bname == "no triangle"
                        continue
                    rec = _finish(st, angle, same, want, tag)
                    _same_record(rec, records.setdefault(bname, rec), tag)
            finally:
                caller.close()
        whole = wants["whole"][1]
        assert whole["counts"][1] > 0 and whole["counts"][5] > 256 * 20 and set(records) == {"whole", "interior", "sliver"}
    finally:
        st.close()


def test_caller_call_with_both_candidate_paths_in_one_launch_group(oracle):
    """ONE call of 23 windows on the cell-25 grid: boxes over more than 64 cells (every triangle of the job a candidate, no rows kernel:
    empty RowsArgs), cell-run boxes, boxes that keep no cell (skipped: the surviving windows close ranks in the launch groups) and boxes
    that keep cells but no whole triangle, every group of 8 mixing them.  Every window gets what a call of its own gives, its counts
    at its own index, and what the statement says."""
    W = _W()
    dmov, dref, case = _device("base")
    grid = C.GRIDS["cell 25"]
    dmov.bin(*grid)
    dref.bin(*grid)
    kinds = C.mixed_boxes(oracle)
    boxes = [b for _k, b in kinds]
    caller = W.DeviceCallerTris(dmov, case["tris"])
    states = [W.DeviceWindow() for _ in boxes]
    solo = W.DeviceWindow()
    args = _filter_args(15, True)
    try:
        counts = W.stage_windows(states, dmov, dref, boxes, C.RADIUS, C.KNN, 1.0)
        staged = [_fetch(st, W) for st in states]
        got = W.caller_tris_windows(states, caller, *args)
        after = [_fetch(st, W) for st in states]
        live = []
        for q, ((kind, box), st) in enumerate(zip(kinds, states)):
            s_counts, s_staged = _stage(solo, dmov, dref, box)
            assert s_counts == counts[q]
            _same_arrays(staged[q], s_staged, q)
            s_got = W.caller_tris_windows([solo], caller, *args)[0]
            assert got[q] == s_got, (q, kind, got[q], s_got)
            _same_arrays(after[q], _fetch(solo, W), (q, kind))
            if kind == "empty":
                assert counts[q][0] > 0 and counts[q][1] > 0 and counts[q][2:] == (0, 0) and got[q] == (0,) * 6
                continue
            assert np.array_equal(st.fetch(W._W_CALLER_TRIANGLES), solo.fetch(W._W_CALLER_TRIANGLES)), (q, kind)
            want = _statement(case, case["tris"], staged[q], 15, True, oracle)
            _check_caller(st, got[q], want, staged[q], (q, kind))
            assert (got[q][0] == 0) == (kind == "no triangle")
            if got[q][4]:
                live.append((q, _finish(solo, 15, True, want, (q, kind))))
        # the finish call over the batch's survivors, 8 + 4 of them
        assert len(live) == 12
        res = W.filter_finish_windows([states[q] for q, _r in live], None, *args, PENALTY, from_caller=True)
        for (q, rec), (kept, added, near, row, flag, stats) in zip(live, res):
            assert (kept, added) == rec["counts"] and near == 0 and stats == rec["stats"], q
            assert np.array_equal(row, rec["row"]) and np.array_equal(flag, rec["flag"]), q
            assert np.array_equal(states[q].fetch(W._W_TRIANGLES), rec["tris"]), q
    finally:
        caller.close()
        for st in states + [solo]:
            st.close()


@pytest.mark.parametrize("n", C.EDGE_ROWS)
def test_caller_scan_edges(oracle, n):
    """The three chained scans of the caller call at block edges.  The reference is the moving section itself, so every row is kept: the
    cell scan runs over exactly n = 255 / 256 / 257 / 16 385 elements; the full box covers more than 64 cells, so the candidates are the
    list's first m triangles exactly: the two triangle scans run over m = 1, 255, 256, 257, 513, 16 384, 16 385 elements and over the whole
    list (~128 blocks: past one look-back window of 64)."""
    W = _W()
    dmov, dref, case = _device(n)
    dmov.bin(*case["grid"])
    dref.bin(*case["grid"])
    st = W.DeviceWindow()
    try:
        for m in C.edge_counts(n):
            tris = case["tris"][:m]
            caller = W.DeviceCallerTris(dmov, tris)
            try:
                counts, staged = _stage(st, dmov, dref, case["box"])
                assert counts[:3] == (n, n, n)
                print(f"rows {n}: {m} triangles, {counts[3]} pairs")
                want = _statement(case, tris, staged, 15, True, oracle)
                got = W.caller_tris_windows([st], caller, *_filter_args(15, True))[0]
                _check_caller(st, got, want, staged, (n, m))
                assert got[0] == m and got[5] > 0
                _finish(st, 15, True, want, (n, m))
            finally:
                caller.close()
    finally:
        st.close()


def test_caller_call_again_with_the_hosts_mask_restarts_from_the_staged_window(oracle):
    """After a first call the window is the compacted one.  A second call with a host `removed` mask (the statement's own) must start
    from the arrays as STAGED again and arrive at the first call's window, on both candidate paths."""
    W = _W()
    dmov, dref, case = _device("base")
    grid = C.GRIDS["cell 25"]
    dmov.bin(*grid)
    dref.bin(*grid)
    caller = W.DeviceCallerTris(dmov, case["tris"])
    st = W.DeviceWindow()
    boxes = C.base_boxes(oracle)
    try:
        for bname in ("whole", "interior"):
            _counts, staged = _stage(st, dmov, dref, boxes[bname])
            want = _statement(case, case["tris"], staged, 15, True, oracle)
            args = _filter_args(15, True)
            first = W.caller_tris_windows([st], caller, *args)[0]
            _check_caller(st, first, want, staged, (bname, "first"))
            assert first[1] > 0
            for again in range(2):
                second = W.caller_tris_windows([st], caller, *args, removed=[(~want["valid"]).astype(np.uint8)])[0]
                _check_caller(st, second, want, staged, (bname, "prefiltered", again))
            _finish(st, 15, True, want, bname)
    finally:
        caller.close()
        st.close()


def test_priority_then_caller_then_finish_on_a_box_of_more_than_64_cells(oracle):
    """The chain of the product route -- stage, priority prune, caller's triangles, finish -- on the whole box of the cell-25 grid equals
    the chain on the window grid, every link equals its statement, and _W_STAGED_PAIRS stays the staged list throughout."""
    from same_amd.knn import priority_filter

    W = _W()
    dmov, dref, case = _device("base")
    codes = C.base_codes()
    box = C.base_boxes(oracle)["whole"]
    st = W.DeviceWindow()
    records = []
    try:
        for gname in ("cell 75", "cell 25"):
            dmov.bin(*C.GRIDS[gname])
            dref.bin(*C.GRIDS[gname])
            caller = W.DeviceCallerTris(dmov, case["tris"])
            try:
                counts, staged = _stage(st, dmov, dref, box)
                rows_r = st.fetch(W._W_ROWS_R)
                pr = W.priority_windows([st])[0]
                pruned = _fetch(st, W)
                want_pairs, one, all_ = priority_filter(staged["pairs"].astype(np.int64), staged["xy"], case["ref_xy"][rows_r],
                                                        C.labels_of(codes["code_m"][staged["rows"]]), C.labels_of(codes["code_r"][rows_r]))
                assert pr == (counts[3], len(want_pairs), one, all_) and one > 0 and all_ > 0
                assert np.array_equal(pruned["pairs"], want_pairs)
                assert np.array_equal(pruned["costs"], C.costs_of(staged["pairs"], staged["costs"], want_pairs, len(rows_r)))
                assert np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"])
                want = _statement(case, case["tris"], pruned, 15, True, oracle)
                got = W.caller_tris_windows([st], caller, *_filter_args(15, True))[0]
                _check_caller(st, got, want, pruned, gname)
                assert got[1] > 0 and np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"])
                records.append(_finish(st, 15, True, want, gname))
                assert np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"])
            finally:
                caller.close()
        _same_record(records[1], records[0], "cell 25 against cell 75")
    finally:
        st.close()


# ---- the priority prune --------------------------------------------------------------------------------------------------------------
def _check_prune(st, case, staged, got, code_m, code_r, tag, rule=True):
    """the window after same_window_priority_pairs against both host statements: pairs, costs, the four counts"""
    from same_amd.knn import priority_filter

    W = _W()
    rows_r = st.fetch(W._W_ROWS_R)
    rxy, cm, cr = case["ref_xy"][rows_r], code_m[staged["rows"]], code_r[rows_r]
    before = staged["pairs"].astype(np.int64)
    want, one, all_ = priority_filter(before, staged["xy"], rxy, C.labels_of(cm), C.labels_of(cr))
    if rule:
        d_want, d_one, d_all = device_rule(before, staged["xy"], rxy, np.asarray(cm), np.asarray(cr))
        assert np.array_equal(d_want, want) and (d_one, d_all) == (one, all_), tag
    assert tuple(got) == (len(before), len(want), one, all_), (tag, got, (len(before), len(want), one, all_))
    after = _fetch(st, W)
    assert after["pairs"].dtype == staged["pairs"].dtype and np.array_equal(after["pairs"], want), tag
    assert np.array_equal(after["costs"], C.costs_of(staged["pairs"], staged["costs"], want, len(rows_r))), tag
    assert np.array_equal(after["rows"], staged["rows"]) and np.array_equal(after["xy"], staged["xy"]), tag
    assert np.array_equal(st.fetch(W._W_STAGED_PAIRS), staged["pairs"]) and st.counts[3] == len(want), tag
    return one, all_


@pytest.mark.parametrize("k", sorted(C.TIE_K))
def test_priority_prune_with_ties_and_large_k(oracle, k):
    """A lattice: four references exactly equidistant from every row and shells of equal distances behind them, exact duplicates among
    the rows, label codes -1 on one side or both.  k = 1, 4, 8, 64, 65 (the stage call's other kernel form), 200: the stable rank of
    rows of up to 200 pairs, the keep counts and the scatter against tests/priority_check.device_rule AND same_amd.knn.priority_filter."""
    W = _W()
    dmov, dref, case = _device("tie")
    st = W.DeviceWindow()
    try:
        counts, staged = _stage(st, dmov, dref, C.TIE_BOX, C.TIE_K[k], k)
        _staged_as_on_the_host(case, C.TIE_BOX, staged, oracle, C.TIE_K[k], k)
        assert counts[2] == len(case["mov_xy"]) and np.bincount(staged["pairs"][:, 0]).max() == k
        got = W.priority_windows([st])[0]
        one, all_ = _check_prune(st, case, staged, got, case["code_m"], case["code_r"], k)
        assert one > 0 and all_ > 0
    finally:
        st.close()


def test_priority_prune_when_700_rows_bid_for_one_reference(oracle):
    """every row's nearest is the one reference that carries their label: 700 bids in three scan blocks and eleven rank blocks meet in one
    atomicMin.  The lowest row wins it and keeps that pair; every other row keeps all four of its pairs."""
    W = _W()
    dmov, dref, case = _device("contention")
    st = W.DeviceWindow()
    try:
        counts, staged = _stage(st, dmov, dref, C.CONTENTION_BOX, C.CONTENTION_RADIUS, C.CONTENTION_K)
        _staged_as_on_the_host(case, C.CONTENTION_BOX, staged, oracle, C.CONTENTION_RADIUS, C.CONTENTION_K)
        n = C.CONTENTION_ROWS
        assert counts == (n, 9, n, 4 * n)
        got = W.priority_windows([st])[0]
        _check_prune(st, case, staged, got, case["code_m"], case["code_r"], "contention")
        assert got == (4 * n, 4 * n - 3, 1, n - 1)
        pairs = st.fetch(W._W_PAIRS)
        assert np.array_equal(pairs[0], (0, 0)) and pairs[1, 0] == 1 and np.array_equal(np.bincount(pairs[:, 0])[1:], np.full(n - 1, 4))
    finally:
        st.close()


@pytest.mark.parametrize("n", C.EDGE_ROWS)
def test_priority_scan_edges(oracle, n):
    """the prune's scan over exactly 255 / 256 / 257 / 16 385 kept rows (the caller call's scan-edge sections: every row is kept)"""
    W = _W()
    dmov, dref, case = _device(n)
    dmov.bin(*case["grid"])
    dref.bin(*case["grid"])
    st = W.DeviceWindow()
    try:
        counts, staged = _stage(st, dmov, dref, case["box"])
        assert counts[:3] == (n, n, n)
        got = W.priority_windows([st])[0]
        one, all_ = _check_prune(st, case, staged, got, case["code_m"], case["code_r"], n)
        assert one > 0 and all_ > 0 and one + all_ == n
    finally:
        st.close()


def test_priority_call_with_more_windows_than_a_launch_takes(oracle):
    """ONE call of 23 windows: in the middle of the launch groups windows whose box holds rows and no pair and windows whose box holds
    nothing -- both skipped, the windows with pairs close ranks.  Every window gets what a call of its own gives, its counts at its own
    index, and what the statements say."""
    W = _W()
    dmov, dref, case = _device("base")
    codes = C.base_codes()
    grid = C.GRIDS["cell 75"]
    dmov.bin(*grid)
    dref.bin(*grid)
    kinds = C.priority_boxes()
    boxes = [b for _k, b in kinds]
    states = [W.DeviceWindow() for _ in boxes]
    solo = W.DeviceWindow()
    try:
        counts = W.stage_windows(states, dmov, dref, boxes, C.RADIUS, C.KNN, 1.0)
        staged = [_fetch(st, W) for st in states]
        got = W.priority_windows(states)
        for q, ((kind, box), st) in enumerate(zip(kinds, states)):
            s_counts, s_staged = _stage(solo, dmov, dref, box)
            assert s_counts == counts[q]
            _same_arrays(staged[q], s_staged, q)
            assert W.priority_windows([solo])[0] == got[q], (q, kind)
            _same_arrays(_fetch(st, W), _fetch(solo, W), (q, kind))
            if kind != "pairs":
                assert got[q] == (0, 0, 0, 0) and counts[q][3] == 0 and (counts[q][0] > 0) == (kind == "no pairs"), (q, kind)
                continue
            one, all_ = _check_prune(st, case, staged[q], got[q], codes["code_m"], codes["code_r"], (q, kind), rule=counts[q][2] < 2000)
            assert one > 0 and all_ > 0
    finally:
        for st in states + [solo]:
            st.close()
