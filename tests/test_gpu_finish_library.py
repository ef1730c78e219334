"""same_window_filter_finish and same_window_refinish (csrc/window_finish.hip, with csrc/match.hip's greedy rounds behind them) driven at
the LIBRARY, as iter_device_windows drives them (W.Section, W.DeviceSection, W.stage_windows, W.filter_finish_windows with the host's
simplices and with prefiltered=True, DeviceWindow.finish / refinish / fetch), against the plain host statement of one window
(tests/finish_check.statement: the oracle and numpy) -- on triangle lists sized to a scan block's edge and past one look-back window,
lattices with exactly equal perimeters and equal costs, cosines on the angle threshold, degenerate triangles, matchings that put both
kinds of writer on every flag byte, a chain of 200 greedy rounds, rows exactly on the no-match penalty, and nine windows in one call.
Every comparison is exact: counts, emitted triangles, signs, weights bit for bit, matched rows, flag bytes, the eight stats with the
productive greedy rounds, the order-tie count.  The inputs come from tests/finish_check.py; tests/test_finish_check_cpu.py proves without a
GPU that each of them has the property its case is about, and that a kernel wrong in one of six ways would give another answer."""
import numpy as np
import pytest

import caller_check as C
import finish_check as F

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")
_DEVICE = {}


def _W():
    from same_amd import windows as W

    return W


def _device(case, dtype):
    """(moving DeviceSection, reference DeviceSection) of a family's section, uploaded once per cost type"""
    key = (id(case), dtype)
    if key not in _DEVICE:
        W = _W()
        mov = W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"])
        ref = W.Section(case["ref_xy"], case["types_r"], None, None)
        _DEVICE[key] = (W.DeviceSection(mov, dtype), W.DeviceSection(ref, dtype), case)       # (the case is held: its id stays its own)
    return _DEVICE[key][:2]


def _filter_args(filt, oracle):
    """the filter's arguments as the product passes them (the threshold is the oracle's)"""
    from same_amd.triangles import cos_threshold

    radius, angle, same = filt
    en, thr = cos_threshold(angle)
    assert (en, thr) == tuple(oracle.cos_threshold(angle))
    return (radius, en, thr, F.near_tol(angle, oracle)[2], same)


def _fetch_staged(st):
    W = _W()
    return dict(rows=st.fetch(W._W_ALIGNED_ROWS), rows_r=st.fetch(W._W_ROWS_R), xy=st.fetch(W._W_ALIGNED_XY), pairs=st.fetch(W._W_PAIRS),
                costs=st.fetch(W._W_COSTS))


def _as_on_the_host(case, box, staged, oracle):
    """the kept rows, the reference rows and every row's pair count are the host's (tests/caller_check.host_stage): what the CPU test
    proved of the host's list holds for the list the device staged"""
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, case["radius"], case["k"], oracle)
    assert np.array_equal(staged["rows"], rows) and np.array_equal(staged["rows_r"], rows_r) and len(staged["pairs"]) == len(pairs)
    assert np.array_equal(np.bincount(staged["pairs"][:, 0], minlength=len(rows)), np.bincount(pairs[:, 0], minlength=len(rows)))
    assert np.array_equal(staged["xy"], case["mov_xy"][rows])


def _stage(st, case, dtype, oracle):
    dmov, dref = _device(case, dtype)
    counts = st.stage(dmov, dref, case["box"], case["radius"], case["k"], case["coeff"])
    staged = _fetch_staged(st)
    _as_on_the_host(case, case["box"], staged, oracle)
    assert counts[2] == len(staged["rows"]) and counts[3] == len(staged["pairs"])
    return staged


def _record(st, res):
    """a finish call's answer for one window with what it left on the device"""
    W = _W()
    kept, added, near, row, flag, stats = res
    rec = dict(kept=kept, added=added, near=near, row=row, flag=flag, stats=stats, order_ties=st.order_ties)
    if not near and len(row):
        rec["match"] = st.fetch(W._W_MATCH)
        if kept + added:
            rec.update(tris=st.fetch(W._W_TRIANGLES), signs=st.fetch(W._W_SIGNS), weights=st.fetch(W._W_WEIGHTS))
    return rec


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _tail_is(rec, want, tag):
    """matched rows, flag bytes, the eight stats; signs and weights bit for bit"""
    assert rec["stats"] == want["stats"], (tag, rec["stats"], want["stats"])
    assert rec["row"].dtype == np.int32 and np.array_equal(rec["row"], want["row"]), tag
    assert rec["flag"].dtype == np.uint8 and np.array_equal(rec["flag"], want["flag"]), tag
    if "match" in rec:
        assert np.array_equal(rec["match"], want["match"]), tag
    if "signs" in rec:
        assert rec["signs"].dtype == np.int8 and np.array_equal(rec["signs"], want["signs"]), tag
        assert np.array_equal(_bits(rec["weights"]), _bits(want["weights"])), tag


def _is(rec, want, tag):
    """the filtered call's answer is the statement's"""
    print(tag, "kept", rec["kept"], "added", rec["added"], "near", rec["near"], "ties", rec["order_ties"], rec["stats"])
    assert (rec["kept"], rec["added"], rec["near"]) == (want["kept"], want["added"], want["near"]), (tag, rec["kept"], rec["added"], rec["near"])
    assert rec["order_ties"] == want["order_ties"], (tag, rec["order_ties"], want["order_ties"])
    if want["near"]:
        assert rec["row"] is None and rec["flag"] is None and rec["stats"] is None, tag
        return
    if want["kept"] + want["added"]:
        assert np.array_equal(rec["tris"], want["tris"]), tag
    _tail_is(rec, want, tag)


def _finish_and_check(st, case, staged, tris, filt, oracle, tag, start=None):
    """the filtered call on a staged window against the statement; again on the finished window (buffers reused, heads zeroed); then the
    statement's emitted triangles handed over as kept ones (prefiltered=True): the filtered call's rows, flags and stats again.
    -> the statement"""
    W = _W()
    penalty = case.get("penalty", F.PENALTY)
    want = F.of_case(case, staged, tris, filt, oracle, start=start)
    fargs = _filter_args(filt, oracle)
    for again in range(2):
        rec = _record(st, W.filter_finish_windows([st], [tris], *fargs, penalty)[0])
        _is(rec, want, (tag, "again" if again else "first"))
    row, flag, stats = st.finish(want["tris"], penalty)
    kept_call = F.of_case(case, staged, want["tris"], filt, oracle, prefiltered=True, start=want.get("start")) if want["near"] else want
    rec = _record(st, (len(want["tris"]), 0, 0, row, flag, stats))
    _tail_is(rec, kept_call, (tag, "prefiltered"))
    if len(want["tris"]):
        assert np.array_equal(rec["tris"], want["tris"]), tag
    assert st.order_ties == kept_call["order_ties"] - (0 if want["near"] else want["fc_ties"]), tag
    return want if not want["near"] else kept_call


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", F.TAGS)
def test_finish_call_is_the_statement(oracle, tag, dtype):
    """One window per family (tests/finish_check.TAGS): staged, checked against the host's stage, finished; the answer is the statement's.
    The knife window comes back with near > 0 and None for the last three results, and is finished from the host's kept triangles as the
    product does.  match/*: the finished window again under the chosen matchings (same_window_refinish).  greedy/chain: the rounds go on
    past the three enqueued up front in batches of 4, 8, ... 64, one read each.  degenerate: the whole list also handed over as kept."""
    W = _W()
    case, tris, filt = F.window_of(tag, oracle)
    st = W.DeviceWindow()
    try:
        staged = _stage(st, case, dtype, oracle)
        n = len(staged["rows"])
        assert n == len(case["mov_xy"])
        before = st.ctx.stats()["greedy_readbacks"]
        want = F.of_case(case, staged, tris, filt, oracle)
        rec = _record(st, W.filter_finish_windows([st], [tris], *_filter_args(filt, oracle), case.get("penalty", F.PENALTY))[0])
        reads = st.ctx.stats()["greedy_readbacks"] - before
        _is(rec, want, tag)
        assert (want["near"] > 0) == (tag in F.NEAR_TAGS)
        kept_call = _finish_and_check(st, case, staged, tris, filt, oracle, tag, start=want.get("start"))
        if tag == "greedy/chain":
            rounds = want["stats"]["greedy_rounds"]
            assert rounds >= 130 and 5 <= reads < rounds, (reads, rounds)
        else:
            assert (reads > 0) == (want["near"] == 0 and want["stats"]["greedy_rounds"] > F.WINDOW_GREEDY_ROUNDS), (tag, reads)
        if tag == "greedy/penalty":            # what the CPU test proved of the host's costs holds for the staged ones
            limit = case["penalty"] * case["size"]
            assert (staged["costs"] == limit).any() and (staged["costs"] < limit).any() and (staged["costs"] > limit).any()
            assert np.array_equal(want["row"] >= 0, staged["costs"] < limit)
        if tag == "greedy/ties":
            assert (staged["costs"] == 3.0).sum() == 4 * n
        if tag.startswith("degenerate"):
            whole = F.of_case(case, staged, tris, filt, oracle, prefiltered=True, start=kept_call["start"])
            row, flag, stats = st.finish(tris, F.PENALTY)
            _tail_is(_record(st, (len(tris), 0, 0, row, flag, stats)), whole, (tag, "the whole list as kept"))
            assert st.order_ties == whole["order_ties"] > 0
        if tag.startswith("match/"):
            st.finish(kept_call["tris"], F.PENALTY)
            for name in F.MATCHINGS:
                mp = F.matching(name, n, kept_call["tris"], staged["pairs"], len(staged["rows_r"]))
                under = F.of_case(case, staged, kept_call["tris"], filt, oracle, prefiltered=True, match_pair=mp)
                row, flag, stats = st.refinish(mp, F.PENALTY)
                _tail_is(dict(row=row, flag=flag, stats=stats, match=st.fetch(W._W_MATCH), signs=st.fetch(W._W_SIGNS),
                              weights=st.fetch(W._W_WEIGHTS)), under, (tag, name))
                if name == "mirror":
                    assert (flag == 3).all()
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_lists_on_one_window_then_a_small_one(oracle, dtype):
    """The triangle list cut to exactly 1 / 255 / 256 / 257 / 16 385 rows, an all-kept and a none-kept list, on ONE DeviceWindow over the
    16 385 kept cells of the edge section: filter_keep_kernel's scan and klist at block edges and past one look-back window,
    filter_emit_kernel's tail.  Then a small window (the lattice) on the same DeviceWindow, its buffers sized by the large one: its own
    statement's."""
    W = _W()
    case = F.edge_section()
    st = W.DeviceWindow()
    try:
        staged = _stage(st, case, dtype, oracle)
        assert len(staged["rows"]) == 16385
        start = None
        for name in F.EDGE_LISTS:
            _case, tris, filt = F.window_of(f"edge/{name}", oracle)
            want = _finish_and_check(st, case, staged, tris, filt, oracle, name, start=start)
            start = want["start"]
            if name.startswith("Tr="):
                assert want["kept"] + want["added"] <= len(tris) == int(name[3:])
        small, tris, filt = F.window_of("lattice/one type/15", oracle)
        staged = _stage(st, small, dtype, oracle)
        want = _finish_and_check(st, small, staged, tris, filt, oracle, "the lattice after 16 385")
        assert want["added"] > 0 and want["fc_ties"] > 0
    finally:
        st.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nine_windows_in_one_call(oracle, dtype):
    """ONE filter_finish_windows call over nine windows (two launch groups) at min_angle_deg = 45: the lattice in the middle comes back
    with near > 0 and None; a window without triangles, a window without a kept cell and the generic ones are each their own statement's,
    at their own index: counts, rows, flags, stats, fetched triangles / signs / weights."""
    W = _W()
    case = F.batch_section()
    dmov, dref = _device(case, dtype)
    states = [W.DeviceWindow() for _ in case["boxes"]]
    try:
        counts = W.stage_windows(states, dmov, dref, list(case["boxes"]), case["radius"], case["k"], case["coeff"])
        staged = [_fetch_staged(st) for st in states]
        tris = list(case["tris"])
        res = W.filter_finish_windows(states, tris, *_filter_args(F.BATCH_FILTER, oracle), F.PENALTY)
        for w, st in enumerate(states):
            _as_on_the_host(case, case["boxes"][w], staged[w], oracle)
            if w == F.BATCH_NO_KEPT:
                assert counts[w][0] > 0 and counts[w][1] > 0 and counts[w][2:] == (0, 0)
                kept, added, near, row, flag, stats = res[w]
                assert (kept, added, near) == (0, 0, 0) and len(row) == 0 and len(flag) == 0 and set(stats.values()) == {0}
                continue
            # the window's own cells are consecutive rows of the section: its triangles are over its kept cells
            assert np.array_equal(staged[w]["rows"], case["first"][w] + np.arange(len(staged[w]["rows"])))
            want = F.of_case(case, staged[w], tris[w], F.BATCH_FILTER, oracle)
            _is(_record(st, res[w]), want, ("window", w))
            assert (want["near"] > 0) == (w == F.BATCH_KNIFE)
    finally:
        for st in states:
            st.close()
