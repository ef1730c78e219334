"""optim_params["hip_priority_prune"] = "device": sliding_window_incumbent keeps a job with ignore_knn_if_matched (the cell-type-priority
prune, src/knn_utils.py:5-78) on the device route (csrc/window_priority.hip).  The oracle is the general route on the same inputs, whose
filter tests/test_host_rows.py pins to the reference.  Tables: the same rows in the same order, every column bit for bit.  Stats: key by
key -- the device route adds `pairs_staged`, `priority_rows`, `keep_all_rows` --, every integer equal; the float objectives of the
optimal starts and of the search are sums the two routes add up in different orders, so they agree to rel 1e-9, the bound of
tests/test_gpu_transport.py::test_routes_agree_and_the_objectives_are_ordered (and `mip_gap`, a quotient of their difference, to its rel
1e-6 / abs 1e-8); `transport_searches` is the route's own."""
import functools

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

KEY = {"hip_priority_prune": "device"}
EXTRA = {"pairs_staged", "priority_rows", "keep_all_rows"}
WIN = dict(window_size=200, overlap=50, min_cells_per_window=20)
OP = dict(radius=30, knn=4, ignore_knn_if_matched=True, **WIN)
FLOAT_STATS = ("objective", "mip_objective_start", "mip_objective")


def _run(ref, mov, cols, op, **k):
    import same_amd

    return same_amd.sliding_window_incumbent(ref, mov, commonCT=cols, optim_params=dict(op), return_stats=True, **k)


def _same_tables(got, want, tag=None):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), tag
    for c in want.columns:
        a, b = got[c].to_numpy(), want[c].to_numpy()
        assert a.dtype == b.dtype, (tag, c)
        if a.dtype.kind == "f":
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), (tag, c)


def _same_stats(got, want, tag=None):
    assert len(got) == len(want), tag
    for a, b in zip(got, want):
        assert set(a) == set(b) | EXTRA, (tag, set(a) ^ set(b))
        assert a["pairs_staged"] >= a["pairs"] and a["priority_rows"] + a["keep_all_rows"] > 0, tag
        for k in b:
            if k == "mip_gap":
                # (objective's rel 1e-9 does not carry over to a QUOTIENT of the two objectives' difference, which is small against
                # either: the bound tests/test_gpu_transport.py sets for this key, rel 1e-6 / abs 1e-8)
                assert a[k] == pytest.approx(b[k], rel=1e-6, abs=1e-8), (tag, k)
            elif k in FLOAT_STATS:
                assert a[k] == pytest.approx(b[k], rel=1e-9, abs=1e-12), (tag, k)
            elif k != "transport_searches":
                assert a[k] == b[k], (tag, k, a[k], b[k])


def _both(ref, mov, cols, op, tag=None, **k):
    """device route with the key == general route -> (table, stats)"""
    want, wst = _run(ref, mov, cols, op, _route="general", **{q: v for q, v in k.items() if q not in ("batch", "workers")})
    got, gst = _run(ref, mov, cols, dict(op, **KEY), _route="device", **k)
    _same_tables(got, want, tag)
    _same_stats(gst, wst, tag)
    return got, gst


@functools.lru_cache(maxsize=None)
def _plain(n=2400, seed=31):
    """(reference frame, moving frame, type columns): ~400 cells a window, so a window's rows span two scan blocks"""
    from same_amd import synth

    cells = synth.make_cells(n, 3, seed=seed)
    return synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=seed + 1)), tuple(synth.type_columns(3))


def _frame(xy, label, seed, types=3):
    """a frame over given coordinates and labels (the type columns random)"""
    from same_amd import synth

    rng = np.random.default_rng(seed)
    t = rng.dirichlet(np.ones(types), len(xy))
    cells = {"xy": np.ascontiguousarray(xy, dtype=np.float64), "types": t, "cell_type": np.zeros(len(xy), np.int32), "size": np.ones(len(xy)),
             "side": float(np.max(xy)) + 1.0}
    df = synth.to_frame(cells)
    df["cell_type"] = label
    return df


def test_the_device_route_gives_the_general_routes_table():
    """fails without the feature: `_route="device"` refuses ignore_knn_if_matched"""
    r_df, m_df, cols = _plain()
    cols = list(cols)
    got, st = _both(r_df, m_df, cols, OP, "plain")
    assert 4 <= len(st) <= 16 and len(got) > 1000
    assert max(s["priority_rows"] + s["keep_all_rows"] for s in st) > 256            # a window's scan crosses blocks
    assert sum(s["priority_rows"] for s in st) > 500 and sum(s["keep_all_rows"] for s in st) > 50
    assert all(s["pairs"] < s["pairs_staged"] for s in st)
    # without _route the key alone picks the device route
    auto, ast = _run(r_df, m_df, cols, dict(OP, **KEY))
    _same_tables(auto, got, "auto")
    assert all("pairs_staged" in s for s in ast) and ast == st
    # the key is ignored when the flag is off
    off = dict(OP, ignore_knn_if_matched=False)
    plain, pst = _run(r_df, m_df, cols, off, _route="device")
    keyed, kst = _run(r_df, m_df, cols, dict(off, **KEY), _route="device")
    _same_tables(keyed, plain, "flag off")
    assert kst == pst and not any("pairs_staged" in s for s in kst)


def test_without_the_key_the_device_route_still_refuses():
    r_df, m_df, cols = _plain()
    for op in (OP, dict(OP, hip_priority_prune="host"), dict(OP, hip_priority_prune=None)):
        with pytest.raises(ValueError, match="device route does not apply"):
            _run(r_df, m_df, list(cols), op, _route="device")
    with pytest.raises(ValueError, match="hip_priority_prune"):
        _run(r_df, m_df, list(cols), dict(OP, hip_priority_prune="gpu"))
    # ... and without _route such a job takes the general route as before
    quiet, qst = _run(r_df, m_df, list(cols), dict(OP, hip_priority_prune="host"))
    assert not any("pairs_staged" in s for s in qst) and len(quiet) > 1000


@pytest.mark.parametrize("knn", [1, 4, 8])
def test_claim_contention(knn):
    """all cells of one type and two jittered copies as suitors: every row bids, many rows share a nearest reference"""
    from same_amd import synth

    cells = synth.make_cells(1800, 3, seed=41)
    r_df = synth.to_frame(cells)
    m_df = pd.concat([synth.to_frame(synth.make_jittered(cells, seed=42, drop=0.0)), synth.to_frame(synth.make_jittered(cells, seed=43, drop=0.0))],
                     ignore_index=True)
    m_df["Cell_Num_Old"] = np.arange(len(m_df)) * 3 + 1
    r_df["cell_type"], m_df["cell_type"] = "c1", "c1"
    op = dict(OP, knn=knn, ignore_same_type_triangles=False)
    _got, st = _both(r_df, m_df, list(synth.type_columns(3)), op, ("one type", knn))
    assert sum(s["priority_rows"] for s in st) > 1000
    if knn > 1:
        assert sum(s["keep_all_rows"] for s in st) > 500          # the losers of a shared nearest reference
    else:
        assert all(s["pairs"] == s["pairs_staged"] for s in st)   # one pair a row: nothing to drop


def test_no_label_equals_any_label_the_filter_is_the_identity():
    """No moving label among the reference labels.  (The job's own check wants the two frames' label SETS equal, so the case is stated
    with labels that equal nothing: NaN on both sides, both sets empty.)  Every row keeps all its pairs, in distance order."""
    r_df, m_df, cols = _plain()
    r_df, m_df = r_df.copy(), m_df.copy()
    r_df["cell_type"], m_df["cell_type"] = np.nan, np.nan
    _got, st = _both(r_df, m_df, list(cols), dict(OP, ignore_same_type_triangles=False), "nan labels")
    assert all(s["pairs"] == s["pairs_staged"] and s["priority_rows"] == 0 for s in st)


def test_disjoint_label_codes_leave_every_pair():
    """No moving label among the reference labels, stated where it can be: at the library, with codes that are non-negative on both
    sides and share no value (a job refuses frames whose label SETS differ before any window runs).  No row bids: every row keeps all
    its pairs, re-sorted by distance with the staged order breaking ties."""
    from same_amd import windows as W
    from same_amd.params import init_optim_params
    from same_amd.window_api import _DeviceFrames, _WindowJob

    r_df, m_df, cols = _plain()
    job = _WindowJob(r_df, m_df, list(cols), None, None, None, OP, None, False, None)
    frames = _DeviceFrames(r_df, m_df, list(cols), init_optim_params(**OP), W.window_cell_grid(job.grid, job.window_size, job.overlap))
    states = [W.DeviceWindow(frames.ctx) for _ in range(3)]
    try:
        rng = np.random.default_rng(3)
        frames.dmov.set_label_codes(rng.integers(0, 4, len(m_df)))
        frames.dref.set_label_codes(rng.integers(4, 8, len(r_df)))
        staged = W.stage_windows(states, frames.dmov, frames.dref, [w["box"] for w in job.plan[:3]], 30.0, 8, 1.0)
        for st, c, got in zip(states, staged, W.priority_windows(states)):
            assert c[2] > 256 and got == (c[3], c[3], 0, c[2]) and st.counts == c
            before, after = st.fetch(W._W_STAGED_PAIRS), st.fetch(W._W_PAIRS)
            axy, rxy = st.fetch(W._W_ALIGNED_XY), frames.ref_sec.xy[st.fetch(W._W_ROWS_R)]
            d = np.sqrt((axy[before[:, 0], 0] - rxy[before[:, 1], 0]) ** 2 + (axy[before[:, 0], 1] - rxy[before[:, 1], 1]) ** 2)
            assert np.array_equal(after, before[np.lexsort((np.arange(len(d)), d, before[:, 0]))])
    finally:
        for st in states:
            st.close()
        frames.close()


def test_two_workers_upload_the_label_codes_once():
    """the codes go up before the worker threads start: one upload per section for a fresh frames object, none for the next job on
    resident frames (a second upload would free the codes a running prune reads)"""
    import same_amd
    from same_amd import windows as W

    r_df, m_df, cols = _plain()
    calls = []
    inner = W.DeviceSection.set_label_codes

    def spy(self, codes):
        import threading

        calls.append(threading.current_thread() is threading.main_thread())
        return inner(self, codes)

    W.DeviceSection.set_label_codes = spy
    try:
        want, _wst = _run(r_df, m_df, list(cols), OP, _route="general")
        got, _gst = _run(r_df, m_df, list(cols), dict(OP, **KEY), _route="device", workers=2, batch=1)
        assert calls == [True, True]
        _same_tables(got, want, "fresh frames, two workers")
        with same_amd.resident_frames(r_df, m_df) as held:
            for _ in range(2):
                again, _ast = _run(held, held, list(cols), dict(OP, **KEY), _route="device", workers=2, batch=1)
                _same_tables(again, want, "resident frames, two workers")
        assert calls == [True] * 4
    finally:
        W.DeviceSection.set_label_codes = inner


def test_lattice_with_two_labels():
    """equal distances everywhere: a moving cell half way between two reference cells of a lattice, labels in stripes -- the stable rank
    decides which of two equidistant references is the nearest"""
    g = np.arange(0.0, 400.0, 10.0)
    rx, ry = (v.ravel() for v in np.meshgrid(g, g))
    rxy = np.column_stack((rx, ry))
    mxy = np.vstack((rxy + (5.0, 0.0), rxy + (0.0, 5.0), rxy + (5.0, 5.0)))
    lab = lambda xy: np.where((np.floor(xy[:, 0] / 10.0) + np.floor(xy[:, 1] / 20.0)) % 2 == 0, "c1", "c2")
    r_df, m_df = _frame(rxy, lab(rxy), 1), _frame(mxy, lab(mxy), 2)
    for knn in (2, 4, 8):
        _got, st = _both(r_df, m_df, [f"c{q + 1}" for q in range(3)], dict(OP, radius=12, knn=knn, ignore_same_type_triangles=False),
                         ("lattice", knn))
        assert sum(s["priority_rows"] for s in st) > 200 and sum(s["keep_all_rows"] for s in st) > 200


@pytest.mark.parametrize("kind", ["nan and None", "int against float"])
def test_labels(kind):
    r_df, m_df, cols = _plain()
    r_df, m_df = r_df.copy(), m_df.copy()
    rng = np.random.default_rng(5)
    if kind == "nan and None":
        for df in (r_df, m_df):
            lab = df["cell_type"].to_numpy().astype(object)
            u = rng.random(len(df))
            lab[u < 0.15] = np.nan
            lab[(u >= 0.15) & (u < 0.3)] = None
            df["cell_type"] = lab
    else:
        code = {c: q + 1 for q, c in enumerate(cols)}
        r_df["cell_type"] = r_df["cell_type"].map(code).astype(np.int64)
        m_df["cell_type"] = m_df["cell_type"].map(code).astype(np.float64)
    _got, st = _both(r_df, m_df, list(cols), dict(OP, ignore_same_type_triangles=False), kind)
    assert sum(s["priority_rows"] for s in st) > 300


def test_a_frame_without_cell_type_fails_as_before():
    r_df, m_df, cols = _plain()
    op = dict(OP, ignore_same_type_triangles=False)
    errors = []
    for o in (op, dict(op, **KEY)):
        with pytest.raises(Exception) as e:
            _run(r_df.drop(columns=["cell_type"]), m_df, list(cols), o)
        errors.append((type(e.value), str(e.value)))
    assert errors[0] == errors[1]
    with pytest.raises(ValueError, match="device route does not apply"):
        _run(r_df.drop(columns=["cell_type"]), m_df, list(cols), dict(op, **KEY), _route="device")


MODES = [dict(hip_incumbent="greedy"), dict(hip_incumbent="assignment", max_matches=1),
         dict(hip_incumbent="transport", max_matches=2, penalty_coeff=0.5),
         dict(hip_refine="local"), dict(hip_refine="capacity", max_matches=2, penalty_coeff=0.5),
         dict(hip_incumbent="transport", hip_refine="capacity", max_matches=2, penalty_coeff=0.5),
         dict(hip_cost_dtype="float32"), dict(hip_delaunay="native"), dict(hip_delaunay="device")]


@pytest.mark.parametrize("extra", MODES, ids=lambda m: ",".join(f"{k}={v}" for k, v in m.items()))
def test_modes_behind_the_prune(extra):
    r_df, m_df, cols = _plain()
    _both(r_df, m_df, list(cols), dict(OP, **extra), extra)


@pytest.mark.parametrize("kw", [dict(window_local_indices=True), dict(batch=1), dict(batch=8), dict(workers=1), dict(workers=2),
                                dict(merge=True), dict(merge=True, workers=2, batch=3)], ids=str)
def test_walks_behind_the_prune(kw):
    r_df, m_df, cols = _plain()
    got, _st = _both(r_df, m_df, list(cols), OP, kw, **kw)
    assert ("ref_idx" in got.columns) == bool(kw.get("window_local_indices"))


def test_a_metacell_reference_named_only_by_dropped_pairs_still_sets_the_limits():
    """The first window by hand.  In the corner x, y < 60 every moving cell sits on its own reference cell and has its label: it wins that
    reference and keeps that one pair.  The LARGEST references (size 3) are extra cells of the corner, 5.7 away from a moving cell each:
    never a nearest, named only by pairs the filter drops.  Elsewhere three jittered copies of the section are the suitors and every second
    reference has size 1.5.  With the multiplier None the general route reads int(largest size) = 3 from the prune's frame (which
    src/knn_utils.py:78 does not compact again): a size-1.5 reference may take 2 * 3 cells.  Were the limits read from the filtered pair
    list, int(1.5) = 1 would hold it to 2."""
    from same_amd import synth
    from same_amd import windows as W

    cells = synth.make_cells(1500, 3, seed=91)
    r_df = synth.to_frame(cells)
    rx, ry = r_df["X"].to_numpy(), r_df["Y"].to_numpy()
    corner = (rx < 60) & (ry < 60)
    assert corner.sum() >= 3
    on_top = r_df[corner].copy()
    on_top[["X", "Y"]] += 0.01
    copies = [synth.to_frame(synth.make_jittered(cells, seed=s, drop=0.0)) for s in (92, 93, 94)]
    copies = [c[~((c["X"] < 75) & (c["Y"] < 75))] for c in copies]
    m_df = pd.concat([on_top] + copies, ignore_index=True)
    m_df["Cell_Num_Old"] = np.arange(len(m_df)) * 3 + 1
    big = r_df[corner].iloc[:3].copy()
    big[["X", "Y"]] += 4.0
    r_df["size"] = np.where(np.arange(len(r_df)) % 2 == 0, 1.5, 1.0)
    big["size"] = 3.0
    r_all = pd.concat([r_df, big], ignore_index=True)
    r_all["Cell_Num_Old"] = np.arange(len(r_all)) * 5 + 2
    is_big = r_all["size"].to_numpy() > 2
    seen = []
    inner = W.priority_windows

    def spy(states):
        out = inner(states)
        for st in states:
            rows_r = st.fetch(W._W_ROWS_R)
            seen.append((bool(is_big[rows_r[st.fetch(W._W_STAGED_PAIRS)[:, 1]]].any()), bool(is_big[rows_r[st.fetch(W._W_PAIRS)[:, 1]]].any())))
        return out

    cols = list(synth.type_columns(3))
    for mult in (None, 3):
        for inc, refine in (("transport", None), ("transport", "capacity"), ("greedy", "capacity")):
            op = dict(OP, max_matches=2, ref_metacell_match_multiplier=mult, penalty_coeff=0.5, hip_incumbent=inc)
            if refine:
                op["hip_refine"] = refine
            del seen[:]
            W.priority_windows = spy
            try:
                _got, st = _both(r_all, m_df, cols, op, (mult, inc, refine), workers=1)
            finally:
                W.priority_windows = inner
            assert seen[0] == (True, False), seen[0]          # the first window: size 3 in the staged list only
            assert st[0]["ref_extra_matches" if refine else "ref_extra_matches_start"] > 0, (mult, inc, refine)


@functools.lru_cache(maxsize=None)
def _metacells():
    import same_amd
    from same_amd import synth

    cells = synth.make_cells(2400, 3, seed=71)
    r_c = synth.to_frame(cells)
    a_c = synth.to_frame(synth.make_jittered(cells, seed=72))
    a_c["Cell_Num_Old"] = np.arange(len(a_c)) * 2 + 7
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True,
                                                            verbose=False)
    return collapse(r_c), collapse(a_c), tuple(synth.type_columns(3))


def test_with_a_callers_triangulation_on_the_device():
    ref, mc, cols = _metacells()
    cols = list(cols)
    both = dict(OP, hip_caller_delaunay="device")
    # MetaCell objects on both sides
    want, wst = _run(ref, mc, cols, both, _route="general")
    got, gst = _run(ref, mc, cols, dict(both, **KEY), _route="device")
    _same_tables(got, want, "metacells")
    _same_stats(gst, wst, "metacells")
    assert len(got) > 300 and sum(s["priority_rows"] for s in gst) > 100
    for kw in (dict(batch=3, workers=2), dict(window_local_indices=True), dict(merge=True)):
        w2, _ = _run(ref, mc, cols, both, _route="general", **{k: v for k, v in kw.items() if k not in ("batch", "workers")})
        g2, _ = _run(ref, mc, cols, dict(both, **KEY), _route="device", **kw)
        _same_tables(g2, w2, kw)
    # a moving_delaunay= array with a vertex column, the capacities behind it
    mdf = mc.metacell_df
    kw = dict(moving_delaunay=np.asarray(mc.metacell_delaunay), moving_delaunay_vertex_col=mc.metacell_idx_col)
    op = dict(both, max_matches=2, penalty_coeff=0.5, hip_incumbent="transport", hip_refine="capacity")
    want, wst = _run(ref, mdf, cols, op, _route="general", **kw)
    got, gst = _run(ref, mdf, cols, dict(op, **KEY), _route="device", **kw)
    _same_tables(got, want, "array")
    _same_stats(gst, wst, "array")
    # without hip_priority_prune the same job silently takes the general route, as before
    quiet, qst = _run(ref, mc, cols, both)
    assert not any("pairs_staged" in s for s in qst)
    with pytest.raises(ValueError, match="device route does not apply"):
        _run(ref, mc, cols, both, _route="device")


def test_a_window_without_pairs_raises_what_the_general_route_raises():
    """a clump of aligned cells and a clump of reference cells that share a window far away, farther apart than the radius"""
    r_df, m_df, cols = _plain()
    rng = np.random.default_rng(5)
    far = m_df.copy()
    far.loc[far.index[:300], ["X", "Y"]] = 50_000.0 + rng.uniform(0, 150, (300, 2))
    near_refs = r_df.iloc[:30].copy()
    near_refs[["X", "Y"]] = 50_190.0 + rng.uniform(0, 9, (30, 2))
    r_far = pd.concat([r_df, near_refs], ignore_index=True)
    r_far["Cell_Num_Old"] = np.arange(len(r_far))
    for op, kw in ((dict(OP, **KEY), dict(_route="device")), (OP, dict(_route="general")), (OP, dict(_route="general", _pipeline="frames"))):
        with pytest.raises(ZeroDivisionError):
            _run(r_far, far, list(cols), op, **kw)


def test_library_refusals():
    """SAME_EINVAL before any device work: the context's counts of launches, copies and waits do not move"""
    from same_amd import _lib
    from same_amd import windows as W
    from same_amd.eval_utils import _label_codes
    from same_amd.params import init_optim_params
    from same_amd.window_api import _DeviceFrames, _WindowJob

    r_df, m_df, cols = _plain()
    op = init_optim_params(**OP)
    job = _WindowJob(r_df, m_df, list(cols), None, None, None, OP, None, False, None)
    grid = W.window_cell_grid(job.grid, job.window_size, job.overlap)
    frames = _DeviceFrames(r_df, m_df, list(cols), op, grid)
    state = W.DeviceWindow(frames.ctx)
    try:
        ctx = frames.ctx

        def refused():
            before = ctx.stats()
            with pytest.raises(_lib.SameHipError) as e:
                W.priority_windows([state])
            assert e.value.code == _lib.SAME_EINVAL and ctx.stats() == before

        stage = lambda: state.stage(frames.dmov, frames.dref, job.plan[0]["box"], 30.0, 4, 1.0)
        refused()                                   # a window not staged
        staged = stage()
        assert staged[3] > 256
        refused()                                   # sections without label codes
        mc, rc = _label_codes(m_df["cell_type"].to_numpy(), r_df["cell_type"].to_numpy())
        frames.dmov.set_label_codes(mc)
        refused()                                   # ... one of them still without
        frames.dref.set_label_codes(rc)
        with pytest.raises(ValueError, match="one label code per section row"):
            frames.dref.set_label_codes(rc[:-1])
        frames.dmov.bin(*grid)
        refused()                                   # staged before the moving section was binned again
        stage()
        p_staged, p_left, one, all_ = W.priority_windows([state])[0]
        assert p_staged == staged[3] and state.counts == staged[:3] + (p_left,) and one + all_ == staged[2] and one > 0
        assert len(state.fetch(W._W_PAIRS)) == p_left and len(state.fetch(W._W_STAGED_PAIRS)) == p_staged
        refused()                                   # a second call on a filtered window
        # what the call left is the host filter's list, with the staged costs
        from same_amd.knn import priority_filter

        rows_r, rows_m = state.fetch(W._W_ROWS_R), state.fetch(W._W_ALIGNED_ROWS)
        before_pairs = state.fetch(W._W_STAGED_PAIRS).astype(np.int64)
        want, w_one, w_all = priority_filter(before_pairs, state.fetch(W._W_ALIGNED_XY), frames.ref_sec.xy[rows_r],
                                             m_df["cell_type"].to_numpy()[rows_m], r_df["cell_type"].to_numpy()[rows_r])
        assert np.array_equal(state.fetch(W._W_PAIRS), want) and (one, all_) == (w_one, w_all)
    finally:
        state.close()
        frames.close()


@pytest.mark.parametrize("seed", range(8))
def test_fuzz(seed):
    """random frames, random settings and modes, route equality"""
    from same_amd import synth

    rng = np.random.default_rng(500 + seed)
    n = int(rng.integers(1500, 3000))
    types = int(rng.integers(2, 5))
    cells = synth.make_cells(n, types, seed=600 + seed)
    r_df = synth.to_frame(cells)
    copies = [synth.to_frame(synth.make_jittered(cells, seed=700 + seed + 10 * q, sigma=float(rng.choice([0.5, 2.0, 6.0])),
                                                 drop=float(rng.uniform(0.0, 0.3)))) for q in range(1 + seed % 2)]
    m_df = pd.concat(copies, ignore_index=True)
    m_df["Cell_Num_Old"] = rng.permutation(len(m_df)) * 3 + 1
    mode = [dict(), dict(hip_incumbent="assignment", max_matches=1), dict(hip_incumbent="transport", max_matches=2, penalty_coeff=0.5),
            dict(hip_refine="local"), dict(hip_incumbent="transport", hip_refine="capacity", max_matches=3, penalty_coeff=0.25),
            dict(hip_cost_dtype="float32"), dict(hip_delaunay="native"), dict(hip_refine="capacity", max_matches=2, penalty_coeff=1.0)][seed]
    op = dict(OP, radius=float(rng.choice([15, 25, 35])), knn=int(rng.integers(1, 9)), min_angle_deg=[15, None, 25][seed % 3],
              ignore_same_type_triangles=bool(seed % 2), **mode)
    _both(r_df, m_df, list(synth.type_columns(types)), op, seed, batch=[1, 3, 8, 20][seed % 4], workers=1 + seed % 2,
          merge=seed % 5 == 0, window_local_indices=seed % 5 == 1)
