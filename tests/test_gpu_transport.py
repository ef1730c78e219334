"""The transport start on the device (optim_params["hip_incumbent"] = "transport", csrc/assign.hip's transport form): the optimum of
the model without its triangle term within the reference capacities.  The oracle is ops.sparse_transport_host (scipy's sparse matching
on the expanded graph, itself checked on the CPU against an enumeration and the dense solver: tests/test_transport_cpu.py); with every
limit 1 the answer is the one-to-one kernel's bit for bit, on host buffers and on the window path."""
import numpy as np
import pytest

import transport_check as T
from test_assign_cpu import random_problem
from test_gpu_assign import _family, _section

pytestmark = pytest.mark.gpu


def _check(ops, pairs, costs, unmatched, n_a, n_r, limit, pc, ties=False, tag=None):
    got, st = ops.sparse_transport(pairs, costs, unmatched, n_a, n_r, limit, pc)
    assert st["fallback"] == 0, tag
    count = T.within_limits(got, pairs, n_a, n_r, limit)
    assert st["ref_extra_matches"] == int(np.maximum(count - 1, 0).sum()), tag
    want = ops.sparse_transport_host(pairs, costs, unmatched, n_a, n_r, limit, pc)
    w_obj = ops.transport_objective(want, pairs, costs, unmatched, n_r, pc)
    assert st["objective"] == pytest.approx(ops.transport_objective(got, pairs, costs, unmatched, n_r, pc), rel=1e-12, abs=1e-12), tag
    assert st["objective"] == pytest.approx(w_obj, rel=1e-9, abs=1e-9), tag
    if not ties:
        assert np.array_equal(got, want), tag
    return got, st


def test_random_problems_equal_the_host_oracle():
    from same_amd import ops

    rng = np.random.default_rng(17)
    extra = 0
    for t in range(200):
        big = t % 25 == 0
        n_a = int(rng.integers(500, 2001)) if big else int(rng.integers(1, 120))
        n_r = int(rng.integers(max(1, n_a // 4), n_a + 2))          # fewer references than rows: the capacities matter
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 12)))
        limit = T.random_limits(rng, n_r)
        pc = [0.0, 0.25, 15.0][t % 3]                                 # none, small, above every no-match cost (<= 12)
        _got, st = _check(ops, pairs, costs, unmatched, n_a, n_r, limit, pc, ties=pc == 0.0, tag=t)
        extra += st["ref_extra_matches"]
        if pc == 15.0:
            assert st["ref_extra_matches"] == 0, t                    # a second match never pays
        # never worse than the greedy start (one-to-one: feasible here) under the same costs
        greedy, _r = ops.greedy_match(pairs, costs, n_a, n_r, ops.pair_rowmin(pairs, costs, n_a) < unmatched)
        assert st["objective"] <= ops.assign_objective(greedy, costs, unmatched) * (1 + 1e-12)
    assert extra > 1000


def _star_with_capacity(rng):
    """every row wants reference 0 at 0.5; it may take 40 of them, each after the first at penalty_coeff"""
    pairs, costs, unmatched, n_a, n_r = _family("star", rng)
    limit = np.ones(n_r, np.int32)
    limit[0] = 40
    return pairs, costs, unmatched, n_a, n_r, limit


@pytest.mark.parametrize("name", ["all_equal", "integer", "star", "no_match_cheaper", "one_pair", "no_pairs", "star_with_capacity"])
@pytest.mark.parametrize("pc", [0.0, 1.0])
def test_adversarial_families(name, pc):
    from same_amd import ops

    rng = np.random.default_rng(hash(name) % 1000)
    if name == "star_with_capacity":
        pairs, costs, unmatched, n_a, n_r, limit = _star_with_capacity(rng)
    else:
        pairs, costs, unmatched, n_a, n_r = _family(name, rng)
        limit = T.random_limits(rng, n_r)
    got, st = _check(ops, pairs, costs, unmatched, n_a, n_r, limit, pc, ties=True, tag=name)
    again, st2 = ops.sparse_transport(pairs, costs, unmatched, n_a, n_r, limit, pc)
    assert st2 == st and np.array_equal(got, again)
    if name == "star_with_capacity":
        assert np.bincount(pairs[got[got >= 0], 1], minlength=n_r)[0] == 40          # 0.5 + 1.0 is below every no-match cost


def test_every_limit_one_is_sparse_assign_bit_for_bit():
    from same_amd import ops

    rng = np.random.default_rng(23)
    for t in range(60):
        n_a = int(rng.integers(500, 2001)) if t % 20 == 0 else int(rng.integers(1, 120))
        n_r = int(rng.integers(max(1, n_a // 2), 2 * n_a + 2))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 12)))
        if t % 4 == 0:
            costs, unmatched = np.round(costs), np.round(unmatched)            # ties: the order among the columns is the same too
        want, wst = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r)
        got, st = ops.sparse_transport(pairs, costs, unmatched, n_a, n_r, np.ones(n_r, np.int32), [0.0, 2.5][t % 2])
        assert np.array_equal(got, want), t
        assert st["rounds"] == wst["rounds"] and st["fallback"] == wst["fallback"] == 0 and st["ref_extra_matches"] == 0
        assert np.float64(st["objective"]).tobytes() == np.float64(wst["objective"]).tobytes(), t


def test_cfg5_sized_window_equals_scipy_sparse():
    """one window of cfg 5's size: 11 300 kept aligned cells, 11 000 reference cells, knn 8, fp32 costs widened to double"""
    from scipy.spatial import cKDTree

    from same_amd import ops

    rng = np.random.default_rng(5)
    n_a, n_r, side = 11_300, 11_000, 1200.0
    rxy = rng.uniform(0, side, (n_r, 2))
    axy = rng.uniform(0, side, (n_a, 2))
    d, j = cKDTree(rxy).query(axy, k=8, distance_upper_bound=25.0)
    ok = np.isfinite(d)
    rows = np.repeat(np.arange(n_a), 8).reshape(n_a, 8)[ok]
    pairs = np.column_stack((rows, j[ok])).astype(np.int32)
    costs = (d[ok] + rng.uniform(0, 60, len(pairs))).astype(np.float32).astype(np.float64)
    unmatched = np.full(n_a, 100.0)
    _got, st = _check(ops, pairs, costs, unmatched, n_a, n_r, np.full(n_r, 2, np.int32), 10.0, tag="cfg5")
    assert st["ref_extra_matches"] > 100


def test_arguments_are_checked_before_any_device_work():
    from same_amd import _lib, ops

    ctx = _lib.default_context(0)
    pairs, costs, unmatched = random_problem(np.random.default_rng(1), 5, 4, 3)
    out, st = np.zeros(5, np.int32), np.zeros(5, np.int64)
    before = ctx.stats()

    def call(limit, pc):
        limit = np.ascontiguousarray(limit, np.int32)
        return ctx.lib.same_sparse_assign_cap(ctx.handle, pairs.ctypes.data, costs.ctypes.data, len(pairs), unmatched.ctypes.data, 5, 4,
                                              limit.ctypes.data, pc, out.ctypes.data, st.ctypes.data)

    for limit, pc in (([1, 0, 1, 1], 1.0), ([1, 1002, 1, 1], 1.0), ([1, 1, 1, 1], -1.0), ([1, 1, 1, 1], float("nan")),
                      ([1, 1, 1, 1], float("inf"))):
        assert call(limit, pc) == _lib.SAME_EINVAL
    assert ctx.lib.same_sparse_assign_cap(ctx.handle, pairs.ctypes.data, costs.ctypes.data, len(pairs), unmatched.ctypes.data, 5, 4, None,
                                          1.0, out.ctypes.data, st.ctypes.data) == _lib.SAME_EINVAL
    assert ctx.stats() == before
    with pytest.raises(ValueError):
        ops.sparse_transport(pairs, costs, unmatched, 5, 4, [1, 0, 1, 1], 1.0)
    assert ctx.stats() == before
    assert call([1, 2, 1001, 1], 0.0) == 0


def _run(r_df, m_df, cols, op, **k):
    import same_amd

    return same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op), return_stats=True, **k)


def _same_tables(got, want, tag):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), tag
    for c in want.columns:
        assert np.array_equal(got[c].to_numpy(), want[c].to_numpy()), (tag, c)


def test_window_path_with_max_matches_one_is_the_assignment_path():
    """max_matches = 1 and no metacells: every limit is 1, and the tables and stats are the "assignment" ones across routes, batch
    sizes, workers and triangulators"""
    r_df, m_df, cols, op = _section()
    A, Tp = dict(op, hip_incumbent="assignment"), dict(op, hip_incumbent="transport", penalty_coeff=3.0)
    want, stats = _run(r_df, m_df, cols, A, _route="device")
    assert len(stats) > 10
    for kw in (dict(_route="device"), dict(_route="device", batch=1), dict(_route="device", workers=1), dict(_route="device", workers=2),
               dict(_route="general", _pipeline="device"), dict(_route="general", _pipeline="frames")):
        got, st = _run(r_df, m_df, cols, Tp, **kw)
        _same_tables(got, want, kw)
        assert len(st) == len(stats)
        for a, b in zip(st, stats):
            assert a["ref_extra_matches_start"] == 0 and a["fallback"] == 0
            if kw["_route"] == "device":
                assert {k: v for k, v in a.items() if k not in ("ref_extra_matches_start", "transport_searches")} == b, kw
                assert np.float64(a["objective"]).tobytes() == np.float64(b["objective"]).tobytes()
            else:
                assert a["objective"] == pytest.approx(b["objective"], rel=1e-9)
    for tri in ("qhull", "native", "device"):
        got, _st = _run(r_df, m_df, cols, dict(Tp, hip_delaunay=tri), _route="device")
        assert got.equals(want), tri
    # under the search too ("capacity" with every limit 1 is "local" bit for bit)
    want, stats = _run(r_df, m_df, cols, dict(A, hip_refine="capacity", penalty_coeff=3.0), _route="device")
    got, st = _run(r_df, m_df, cols, dict(Tp, hip_refine="capacity"), _route="device")
    _same_tables(got, want, "capacity")
    for a, b in zip(st, stats):
        assert {k: v for k, v in a.items() if k not in ("ref_extra_matches_start", "transport_searches", "mip_gap")} == b
        assert a["mip_gap"] >= 0


def _crowded_section(seed=50):
    """`_section` with the moving side laid down twice (two jitters of the same reference): two aligned cells per reference cell whose
    type vectors equal its own.  On `_section` itself a cell's only pair below its no-match cost is its own counterpart (the type term of
    any other pair is four orders of magnitude above no_match_penalty), so no optimum shares a reference; here the second cell of a
    reference shares it whenever its pair cost + penalty_coeff is below its no-match cost."""
    import pandas as pd

    from same_amd import synth

    r_df, m_df, cols, op = _section(seed=seed)
    ref = synth.make_cells(30_000, 5, seed=seed)
    m_df = pd.concat([m_df, synth.to_frame(synth.make_jittered(ref, seed=seed + 2))], ignore_index=True)
    m_df["Cell_Num_Old"] = np.arange(len(m_df))
    m_df["size"] = np.where(np.arange(len(m_df)) % 3 == 0, 2, 1)
    return r_df, m_df, cols, dict(op, max_matches=2, penalty_coeff=0.001)


def _metacell_section():
    """the crowded section with metacells on both sides (sizes 1, 3, 5 on every fourth reference), multiplier 3: a metacell reference
    takes up to 6 cells, the others 2"""
    r_df, m_df, cols, op = _crowded_section(seed=60)
    r_df["size"] = np.where(np.arange(len(r_df)) % 4 == 0, 1 + np.arange(len(r_df)) % 6, 1)
    return r_df, m_df, cols, dict(op, ref_metacell_match_multiplier=3)


@pytest.mark.parametrize("section", ["plain", "crowded", "metacell"])
def test_routes_agree_and_the_objectives_are_ordered(section):
    """max_matches = 2: the device route's table is the general route's; per window the transport optimum is at most the assignment's
    and the greedy start's cost, and under hip_refine="capacity" it bounds the refined objective from below (mip_gap >= 0).  "plain" is
    `_section` as it is (no optimum shares a reference there: see _crowded_section); the other two use the capacities."""
    if section == "plain":
        r_df, m_df, cols, op = _section()
        op = dict(op, max_matches=2, penalty_coeff=0.001)
    elif section == "crowded":
        r_df, m_df, cols, op = _crowded_section()
    else:
        r_df, m_df, cols, op = _metacell_section()
    Tp = dict(op, hip_incumbent="transport")
    dev, dst = _run(r_df, m_df, cols, Tp, _route="device")
    gen, gst = _run(r_df, m_df, cols, Tp, _route="general")
    _same_tables(dev, gen, section)
    assert len(dst) == len(gst) > 10
    if section != "plain":          # the capacities are used
        assert sum(s["ref_extra_matches_start"] for s in dst) > 50
    for a, b in zip(dst, gst):
        assert set(a) == set(b) and a["fallback"] == b["fallback"] == 0
        for k in a:
            if k == "objective":
                assert a[k] == pytest.approx(b[k], rel=1e-9), k
            elif k != "transport_searches":          # (how many searches it took is the route's own: its pair order, its cost bits)
                assert a[k] == b[k], k
    # ordering: against the one-to-one optimum (max_matches = 1 so that the mode is accepted; the pairs and costs are the same)
    # and the greedy start, whose cost is its search record's starting objective at delaunay_penalty 0
    _a, ast = _run(r_df, m_df, cols, dict(op, hip_incumbent="assignment", max_matches=1), _route="device")
    _g, grs = _run(r_df, m_df, cols, dict(op, hip_refine="capacity", hip_refine_rounds=1, delaunay_penalty=0.0), _route="device")
    for t, a, g in zip(dst, ast, grs):
        assert t["objective"] <= a["objective"] * (1 + 1e-12)
        assert t["objective"] <= g["mip_objective_start"] * (1 + 1e-12)
    ref, rst = _run(r_df, m_df, cols, dict(Tp, hip_refine="capacity"), _route="device")
    gref, grst = _run(r_df, m_df, cols, dict(Tp, hip_refine="capacity"), _route="general")
    _same_tables(ref, gref, section + " refined")
    for s, t, g in zip(rst, dst, grst):
        assert s["objective"] == t["objective"] and s["ref_extra_matches_start"] == t["ref_extra_matches_start"]
        assert s["mip_objective"] >= s["objective"] * (1 - 1e-12) and s["mip_gap"] >= 0
        # (both routes' objectives agree to rel 1e-9 each, so their quotient of a difference agrees to about 2e-9 absolute)
        assert s["mip_gap"] == pytest.approx(g["mip_gap"], rel=1e-6, abs=1e-8)
    # a start that is not the model's own capacities carries no gap
    assert all("mip_gap" not in s for s in grs)


@pytest.mark.parametrize("refine", [None, "capacity"])
def test_device_route_fallback_equals_the_general_route(monkeypatch, refine):
    """a window whose certificate flag is up (forced, in the decoded record of its finish call) is solved by the host transport solver
    and finished again under that matching: its table rows and stats are the general route's, with fallback == 1"""
    from same_amd import windows as W

    r_df, m_df, cols, op = _metacell_section()
    A = dict(op, hip_incumbent="transport", **({} if refine is None else {"hip_refine": refine}))
    want, wst = _run(r_df, m_df, cols, A, _route="general")
    inner, forced = W._window_records, []

    def flagged(s, mode):
        asg, rfn = inner(s, mode)
        if asg is not None and s[7] > 0 and not forced:        # (word 7: matched cells)
            forced.append(asg)
            asg = dict(asg, flags=1)
        return asg, rfn

    monkeypatch.setattr(W, "_window_records", flagged)
    got, gst = _run(r_df, m_df, cols, A, _route="device")
    assert len(forced) == 1 and len(gst) == len(wst) > 10
    assert [s["fallback"] for s in gst].count(1) == 1 and all(s["fallback"] == 0 for s in wst)
    _same_tables(got, want, refine)
    for a, b in zip(gst, wst):
        assert set(a) == set(b)
        for k in a:
            if k == "mip_gap":           # (a quotient of a difference of two objectives that agree to rel 1e-9 each)
                assert a[k] == pytest.approx(b[k], rel=1e-6, abs=1e-8), k
            elif k in ("objective", "mip_objective_start", "mip_objective"):
                assert a[k] == pytest.approx(b[k], rel=1e-9, abs=1e-12), k
            elif k not in ("fallback", "transport_searches"):
                assert a[k] == b[k], k


def test_finish_call_refuses_transport_without_a_capacity(monkeypatch):
    """SAME_INCUMBENT_TRANSPORT through the library call that carries no capacity, or with a bad one: SAME_EINVAL and no device work.
    On the Python side no such call can be made: the VALUE refuses (a transport WindowMode without a capacity raises when it is built,
    before DeviceWindow.filter_finish is entered)."""
    import ctypes

    from same_amd import _lib, synth
    from same_amd import windows as W
    from same_amd.window_mode import WindowMode
    from scipy.spatial import Delaunay

    ctx = _lib.default_context(0)
    ref = synth.make_cells(2000, 4, seed=3)
    mov = synth.make_jittered(ref, seed=4)
    rs, ms = W.Section(ref["xy"], ref["types"], None, None), W.Section(mov["xy"], mov["types"], None, None)
    dref, dmov = W.DeviceSection(rs, np.float64, ctx), W.DeviceSection(ms, np.float64, ctx)
    st = W.DeviceWindow(ctx)
    try:
        W.stage_windows([st], dmov, dref, [(-1e9, 1e9, -1e9, 1e9)], 25.0, 8, 1.0)
        tris = np.ascontiguousarray(Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices, np.int32)
        offsets = np.array([0, len(tris)], np.int64)
        n = st.counts[2]
        row, flag = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        stats, counts = np.zeros(_lib.SAME_WINDOW_STATS_TRANSPORT, np.int64), np.zeros(4, np.int64)
        head = (W._handles([st]), 1, _lib.SAME_TRIS_SIMPLICES, tris.ctypes.data, offsets.ctypes.data, 25.0, 0, 0.0, 0.0, 1, 1, 6.0,
                _lib.SAME_INCUMBENT_TRANSPORT, 0, 0.0)
        outs = (row.ctypes.data, flag.ctypes.data, stats.ctypes.data, counts.ctypes.data)
        before = ctx.stats()
        assert ctx.lib.same_window_filter_finish(*head, *outs) == _lib.SAME_EINVAL
        assert ctx.lib.same_window_filter_finish_cap(*head, None, *outs) == _lib.SAME_EINVAL
        for bad in (_lib.WindowCapacity(0, 0, 1.0), _lib.WindowCapacity(2, -1, 1.0), _lib.WindowCapacity(2, 0, -1.0),
                    _lib.WindowCapacity(2, 0, float("nan"))):
            assert ctx.lib.same_window_filter_finish_cap(*head, ctypes.byref(bad), *outs) == _lib.SAME_EINVAL
        assert ctx.stats() == before
        with pytest.raises(ValueError):
            st.filter_finish(tris, 25.0, 0, 0.0, 0.0, True, 6.0, mode=WindowMode("transport"))
        assert ctx.stats() == before
        good = _lib.WindowCapacity(2, 0, 1.0)
        assert ctx.lib.same_window_filter_finish_cap(*head, ctypes.byref(good), *outs) == 0
        assert stats[8] == 0 and stats[7] > 0
    finally:
        st.close()
        dref.close()
        dmov.close()
