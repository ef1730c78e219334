"""The optimal-assignment incumbent on the device (optim_params["hip_incumbent"] = "assignment", csrc/assign.hip).  The oracle is scipy:
linear_sum_assignment on the reference's dense big-M matrix (ops.assign_matrix, src/init_helpers.py:150-158) for small problems,
min_weight_full_bipartite_matching on the shifted sparse problem (ops.sparse_assign_host) for large ones."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from test_assign_cpu import random_problem

pytestmark = pytest.mark.gpu

BIG_M = 1e9


def dense_call(ops, pairs, costs, unmatched, n_a, n_r):
    """the reference's call on the port's dense matrix -> pair index per row, -1 = unmatched"""
    cost_mat = ops.assign_matrix(pairs, costs, unmatched, n_a, n_r, BIG_M)
    rows, cols = linear_sum_assignment(cost_mat)
    lookup = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs.tolist())}
    out = np.full(n_a, -1, np.int32)
    for i, j in zip(rows.tolist(), cols.tolist()):
        if j < n_r and cost_mat[i, j] < BIG_M * 0.5:
            out[i] = lookup[(i, j)]
    return out


def valid_matching(pairs, mp, n_a):
    m = mp >= 0
    assert len(mp) == n_a and np.all(mp[m] < len(pairs))
    assert np.array_equal(pairs[mp[m], 0], np.flatnonzero(m))          # a row's pair is its own
    cols = pairs[mp[m], 1]
    assert len(np.unique(cols)) == len(cols)                              # one-to-one


def test_small_random_problems_equal_the_dense_reference():
    from same_amd import ops

    rng = np.random.default_rng(7)
    for t in range(200):
        big = t % 20 == 0
        n_a = int(rng.integers(500, 2001)) if big else int(rng.integers(1, 120))
        n_r = int(rng.integers(max(1, n_a // 2), 2 * n_a + 2))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 12)))
        got, st = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r)
        assert st["fallback"] == 0
        valid_matching(pairs, got, n_a)
        assert np.array_equal(got, dense_call(ops, pairs, costs, unmatched, n_a, n_r)), t
        assert st["objective"] == pytest.approx(ops.assign_objective(got, costs, unmatched), rel=1e-12)
        # never worse than the greedy start under the same costs
        prefer = ops.pair_rowmin(pairs, costs, n_a) < unmatched
        greedy, _r = ops.greedy_match(pairs, costs, n_a, n_r, prefer)
        assert st["objective"] <= ops.assign_objective(greedy, costs, unmatched) * (1 + 1e-12)


def _family(name, rng):
    n_a, n_r, k = 600, 500, 6
    pairs, costs, unmatched = random_problem(rng, n_a, n_r, k)
    if name == "all_equal":
        costs[:] = 3.0
        unmatched[:] = 5.0
    elif name == "integer":
        costs = rng.integers(0, 6, len(costs)).astype(np.float64)
        unmatched = rng.integers(3, 8, n_a).astype(np.float64)
    elif name == "star":
        star = np.column_stack((np.arange(n_a), np.zeros(n_a))).astype(np.int32)
        keep = pairs[:, 1] != 0
        pairs, costs = np.concatenate((pairs[keep], star)), np.concatenate((costs[keep], np.full(n_a, 0.5)))
    elif name == "no_match_cheaper":
        unmatched[:] = costs.min() - 1.0 if len(costs) else 0.0
    elif name == "one_pair":
        pairs = np.column_stack((np.arange(n_a), rng.integers(0, n_r, n_a))).astype(np.int32)
        costs = rng.uniform(0, 10, n_a)
    elif name == "no_pairs":
        pairs, costs = np.zeros((0, 2), np.int32), np.zeros(0)
    return pairs, costs, unmatched, n_a, n_r


@pytest.mark.parametrize("name", ["all_equal", "integer", "star", "no_match_cheaper", "one_pair", "no_pairs"])
def test_adversarial_families(name):
    from same_amd import ops

    pairs, costs, unmatched, n_a, n_r = _family(name, np.random.default_rng(hash(name) % 1000))
    got, st = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r)
    again, st2 = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r)
    assert st["fallback"] == 0 and st2 == st and np.array_equal(got, again)
    valid_matching(pairs, got, n_a)
    want = ops.assign_objective(dense_call(ops, pairs, costs, unmatched, n_a, n_r), costs, unmatched)
    assert ops.assign_objective(got, costs, unmatched) == pytest.approx(want, rel=1e-9, abs=1e-9)


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
    types = rng.uniform(0, 60, len(pairs))
    costs = (d[ok] + types).astype(np.float32).astype(np.float64)
    unmatched = np.full(n_a, 100.0)
    got, st = ops.sparse_assign(pairs, costs, unmatched, n_a, n_r)
    assert st["fallback"] == 0
    valid_matching(pairs, got, n_a)
    assert np.array_equal(got, ops.sparse_assign_host(pairs, costs, unmatched, n_a, n_r))


def _section(seed=30):
    from same_amd import synth

    ref = synth.make_cells(30_000, 5, seed=seed)
    mov = synth.make_jittered(ref, seed=seed + 1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    m_df["size"] = np.where(np.arange(len(m_df)) % 3 == 0, 2, 1)
    op = dict(radius=30, knn=6, min_angle_deg=12, dist_ct_coeff=1.5, hip_cost_dtype="float32", window_size=700, overlap=200,
              no_match_penalty=0.006, min_cells_per_window=10)
    return r_df, m_df, synth.type_columns(5), op


def test_window_tables_agree_over_routes_batches_workers_and_triangulators():
    import same_amd

    r_df, m_df, cols, op = _section()
    A = dict(op, hip_incumbent="assignment")
    run = lambda o, **k: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True, **k)
    want, stats = run(A, _route="device")
    assert len(stats) > 10 and all(s["fallback"] == 0 for s in stats)
    greedy, gstats = run(op, _route="device")
    plain, pstats = run(dict(op, hip_incumbent="greedy"), _route="device")
    assert plain.equals(greedy) and pstats == gstats and all("objective" not in s for s in gstats)
    for kw in (dict(_route="general", _pipeline="device"), dict(_route="general", _pipeline="frames")):
        got, st = run(A, **kw)
        assert list(got.columns) == list(want.columns) and len(got) == len(want), kw
        for c in want.columns:
            assert np.array_equal(got[c].to_numpy(), want[c].to_numpy()), (kw, c)
        assert [s["objective"] for s in st] == pytest.approx([s["objective"] for s in stats], rel=1e-9)
    for kw in (dict(batch=1), dict(workers=1), dict(workers=2)):
        got, st = run(A, _route="device", **kw)
        assert got.equals(want) and st == stats, kw
    for tri in ("qhull", "native", "device"):
        got, st = run(dict(A, hip_delaunay=tri), _route="device")
        assert got.equals(want), tri
    merged = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(A), merge=True)
    ref_merge = same_amd.merge_window_matches_unique_ref([want], cell_id_col="Cell_Num_Old")
    assert list(merged.columns) == list(ref_merge.columns) and len(merged) == len(ref_merge)
    for c in merged.columns:
        assert np.array_equal(merged[c].to_numpy(), ref_merge[c].to_numpy()), c


def test_every_window_is_scipys_optimum_and_never_worse_than_greedy(monkeypatch):
    """every window of the general route (whose tables the device route's equal, above): its matching is scipy's over the window's own
    pairs and costs, and its objective is never above the greedy start's; the device route reports the same objectives"""
    import same_amd
    from same_amd import ops

    r_df, m_df, cols, op = _section(seed=40)
    seen, inner = [], ops.sparse_assign

    def spy(pairs, costs, unmatched, n_a, n_r, ctx=None):
        out = inner(pairs, costs, unmatched, n_a, n_r, ctx=ctx)
        seen.append((np.array(pairs), np.array(costs), np.array(unmatched), n_a, n_r, out[0].copy(), out[1]))
        return out

    monkeypatch.setattr(ops, "sparse_assign", spy)
    A = dict(op, hip_incumbent="assignment")
    _t, st = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=A, return_stats=True, _route="general")
    monkeypatch.setattr(ops, "sparse_assign", inner)
    _d, dst = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=A, return_stats=True, _route="device")
    assert len(seen) == len(st) == len(dst) > 10
    assert [s["objective"] for s in dst] == pytest.approx([s["objective"] for s in st], rel=1e-9)
    for pairs, costs, unmatched, n_a, n_r, got, stats in seen:
        assert stats["fallback"] == 0
        assert np.array_equal(got, ops.sparse_assign_host(pairs, costs, unmatched, n_a, n_r))
        prefer = ops.pair_rowmin(pairs, costs, n_a) < unmatched
        greedy, _r = ops.greedy_match(pairs, costs, n_a, n_r, prefer)
        g = ops.assign_objective(greedy, costs, unmatched)
        assert stats["objective"] <= g * (1 + 1e-12)


def test_cfg5_1m_cells_merged_table_is_stable_without_fallbacks():
    """BASELINE config 5 at full size through the product function, window merge included: two assignment passes give the same merged
    table, every window reports a finite objective and none falls back to the host"""
    import same_amd
    from same_amd import synth

    T = 8
    ref = synth.make_cells(1_000_000, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)
    A = dict(op, hip_incumbent="assignment")
    with same_amd.resident_frames(r_df, m_df) as res:
        first, st1 = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(A), merge=True, return_stats=True)
        second, st2 = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(A), merge=True, return_stats=True)
    assert len(first) > 900_000 and first.equals(second) and st1 == st2
    assert len(st1) > 100 and sum(s["fallback"] for s in st1) == 0
    assert all(np.isfinite(s["objective"]) for s in st1)


@pytest.fixture
def staged():
    """one window staged over a whole 4 000-cell section, with scipy's simplices of its kept cells"""
    from scipy.spatial import Delaunay

    from same_amd import _lib, synth
    from same_amd import windows as W

    ctx = _lib.default_context(0)
    ref = synth.make_cells(4000, 4, seed=3)
    mov = synth.make_jittered(ref, seed=4)
    tid = np.unique(mov["cell_type"], return_inverse=True)[1].astype(np.int32)
    size = np.where(np.arange(len(mov["xy"])) % 3 == 0, 2, 1)
    rs, ms = W.Section(ref["xy"], ref["types"], None, None), W.Section(mov["xy"], mov["types"], tid, size)
    dref, dmov = W.DeviceSection(rs, np.float64, ctx), W.DeviceSection(ms, np.float64, ctx)
    st = W.DeviceWindow(ctx)
    try:
        W.stage_windows([st], dmov, dref, [(-1e9, 1e9, -1e9, 1e9)], 25.0, 8, 1.0)
        yield st, rs, ms, Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices
    finally:
        st.close()
        dref.close()
        dmov.close()


PENALTY = 6.0
REFINE = (256, 4.0)


def _finish(st, simplices, mode=None):
    from same_amd.triangles import cos_threshold

    en, thr = cos_threshold(15)
    _k0, _k1, near, row, flag, stats = st.filter_finish(simplices, 25.0, en, thr, 0.0, True, PENALTY, mode=mode)
    assert near == 0
    return row, flag, stats


@pytest.mark.parametrize("refine", [None, REFINE])
def test_refinish_under_its_own_matching_repeats_the_finish(staged, refine):
    """same_window_refinish with the window's own matching (pair per kept cell from its match and pairs) gives back what the finish
    call gave: matched rows, flag bytes, every counter but the incumbent's rounds; with the search on, a settled search moves no more"""
    from same_amd import windows as W
    from same_amd.window_mode import WindowMode

    st, _rs, _ms, simplices = staged
    for incumbent in ("greedy", "assignment"):
        mode = WindowMode(incumbent) if refine is None else WindowMode(incumbent, "local", *refine)
        row, flag, stats = _finish(st, simplices, mode)
        first = st.refine
        if refine is not None:
            assert first["settled"] == 1 and first["rounds"] < refine[0], first
        pair_of = {tuple(p): q for q, p in enumerate(st.fetch(W._W_PAIRS).tolist())}
        mp = np.array([pair_of[(i, m)] if m >= 0 else -1 for i, m in enumerate(st.fetch(W._W_MATCH).tolist())], np.int32)
        row2, flag2, stats2 = st.refinish(mp, PENALTY, mode)
        assert np.array_equal(row2, row) and np.array_equal(flag2, flag), incumbent
        assert stats2["greedy_rounds"] == 0 and stats["matched"] > 0 and (stats["greedy_rounds"] > 0 or incumbent == "assignment")
        assert {k: v for k, v in stats2.items() if k != "greedy_rounds"} == {k: v for k, v in stats.items() if k != "greedy_rounds"}
        if refine is None:
            assert st.refine is None
        else:
            assert st.refine["moves"] == 0 and st.refine["settled"] == 1, st.refine
            assert st.refine["objective"] == pytest.approx(first["objective"], rel=1e-12)


@pytest.mark.parametrize("other", ["scipy", "unmatched"])
def test_refinish_under_another_matching_equals_the_host_sweeps(staged, other):
    """same_window_refinish under a matching the device did not make (scipy's optimum, or no cell matched): the matched rows, flag bytes
    and counters are those of the host-buffer sweeps for that matching, as incumbent.incumbent_of_prepared computes them"""
    from same_amd import ops
    from same_amd import windows as W
    from same_amd.window_mode import WindowMode

    st, rs, ms, simplices = staged
    _finish(st, simplices, WindowMode("assignment"))
    pairs, costs, rows_r = st.fetch(W._W_PAIRS), st.fetch(W._W_COSTS), st.fetch(W._W_ROWS_R)
    axy, rows_m, tris, signs = st.fetch(W._W_ALIGNED_XY), st.fetch(W._W_ALIGNED_ROWS), st.fetch(W._W_TRIANGLES), st.fetch(W._W_SIGNS)
    n_a, rxy = len(axy), rs.xy[rows_r]
    unmatched = PENALTY * ms.size[rows_m].astype(np.float64)
    if other == "scipy":
        mp = ops.sparse_assign_host(pairs, costs, unmatched, n_a, len(rows_r))
    else:
        mp = np.full(n_a, -1, np.int32)
    row, flag, stats = st.refinish(mp, PENALTY)
    match = np.where(mp >= 0, pairs[np.maximum(mp, 0), 1], -1).astype(np.int32)
    sw = ops.BoundSweep(tris, signs, rxy, n_a)
    try:
        checked, viol = sw.sweep_match(match)
    finally:
        sw.close()
    _edge, _tflag, pflag, counts = ops.xyorder_sweep(axy, rxy, tris, match)
    _before, _after, _m3, flipped = ops.area_flip(axy, rxy, tris, match)
    flip_node = np.zeros(n_a, np.uint8)
    flip_node[tris[flipped.astype(bool)].reshape(-1)] = 1
    assert np.array_equal(row, np.where(match >= 0, rows_r[np.maximum(match, 0)], -1))
    assert np.array_equal(flag & 1, pflag) and np.array_equal(flag >> 1, flip_node)
    assert stats == {"checked": checked, "flipped": len(viol), "xy_comparisons": int(counts[0]), "xy_violations": int(counts[1]),
                     "xy_triangles": int(counts[2]), "area_flips": int(np.count_nonzero(flipped)), "greedy_rounds": 0,
                     "matched": int(np.count_nonzero(mp >= 0))}
    assert (stats["matched"] > 0 and stats["xy_comparisons"] > 0) == (other == "scipy")


@pytest.mark.parametrize("refine", [None, "local"])
def test_device_route_fallback_equals_the_general_route(monkeypatch, refine):
    """a window whose certificate flag is up (forced here, in the decoded record of its finish call) is solved by scipy and finished
    again under that matching (same_window_refinish): its table rows and stats are the general route's, with fallback == 1"""
    import same_amd
    from same_amd import windows as W

    r_df, m_df, cols, op = _section()
    A = dict(op, hip_incumbent="assignment", **({} if refine is None else {"hip_refine": refine}))
    run = lambda **k: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(A), return_stats=True, **k)
    want, wst = run(_route="general")
    inner, forced = W._window_records, []

    def flagged(s, mode):
        asg, rfn = inner(s, mode)
        if asg is not None and s[7] > 0 and not forced:        # (word 7: matched cells)
            forced.append(asg)
            asg = dict(asg, flags=1)
        return asg, rfn

    monkeypatch.setattr(W, "_window_records", flagged)
    got, gst = run(_route="device")
    assert len(forced) == 1 and len(gst) == len(wst) > 10
    assert [s["fallback"] for s in gst].count(1) == 1 and all(s["fallback"] == 0 for s in wst)
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in want.columns:
        assert np.array_equal(got[c].to_numpy(), want[c].to_numpy()), c
    for a, b in zip(gst, wst):
        assert set(a) == set(b)
        for k in a:
            if k in ("objective", "mip_objective_start", "mip_objective"):
                assert a[k] == pytest.approx(b[k], rel=1e-9), k
            elif k != "fallback":
                assert a[k] == b[k], k


def test_finish_arguments_are_checked_before_any_device_work(staged):
    """a bad incumbent mode, a negative round cap, a NaN penalty, NULL simplices with a host source (and host simplices with the
    device's): SAME_EINVAL, and not one launch, fill, copy or wait"""
    from same_amd import _lib
    from same_amd import windows as W

    st, _rs, _ms, simplices = staged
    _finish(st, simplices)                              # (a finished window: same_window_refinish would take it)
    ctx = st.ctx
    n = st.counts[2]
    tris = np.ascontiguousarray(simplices, dtype=np.int32)
    offsets = np.array([0, len(tris)], np.int64)
    row, flag = np.empty(n, np.int32), np.empty(n, np.uint8)
    stats, counts = np.zeros(_lib.SAME_WINDOW_STATS, np.int64), np.zeros(4, np.int64)
    good = dict(source=_lib.SAME_TRIS_SIMPLICES, tris=tris.ctypes.data, offsets=offsets.ctypes.data, incumbent=_lib.SAME_INCUMBENT_GREEDY,
                cap=0, dp=0.0)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.same_window_filter_finish(W._handles([st]), 1, a["source"], a["tris"], a["offsets"], 25.0, 0, 0.0, 0.0, 1, 1,
                                                 PENALTY, a["incumbent"], a["cap"], a["dp"], row.ctypes.data, flag.ctypes.data,
                                                 stats.ctypes.data, counts.ctypes.data)

    mp = np.full(n, -1, np.int32)
    before = ctx.stats()
    assert call(incumbent=2) == _lib.SAME_EINVAL
    assert call(incumbent=-1) == _lib.SAME_EINVAL
    assert call(cap=-1) == _lib.SAME_EINVAL
    assert call(cap=8, dp=float("nan")) == _lib.SAME_EINVAL
    assert call(cap=8, dp=-1.0) == _lib.SAME_EINVAL
    assert call(source=3) == _lib.SAME_EINVAL
    for source in (_lib.SAME_TRIS_SIMPLICES, _lib.SAME_TRIS_KEPT):
        assert call(source=source, tris=None, offsets=None) == _lib.SAME_EINVAL
        assert call(source=source, tris=None) == _lib.SAME_EINVAL
    assert call(source=_lib.SAME_TRIS_DEVICE) == _lib.SAME_EINVAL
    for cap, dp in ((-1, 0.0), (8, float("nan"))):
        assert ctx.lib.same_window_refinish(st.handle, mp.ctypes.data, PENALTY, cap, dp, row.ctypes.data, flag.ctypes.data,
                                            stats.ctypes.data) == _lib.SAME_EINVAL
    after = ctx.stats()
    assert {k: after[k] for k in ("launches", "fills", "copies", "waits")} == {k: before[k] for k in ("launches", "fills", "copies", "waits")}
    assert call() == 0                                   # the same call with good arguments runs
