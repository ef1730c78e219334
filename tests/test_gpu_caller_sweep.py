"""same_window_caller_pairs (csrc/window_caller.hip) and same_window_knn_prefix on a window a caller's triangulation has compacted, at the
LIBRARY; and same_amd.sliding_window_sweep over MetaCell objects / `moving_delaunay=` under hip_caller_delaunay="device" as a product.
Library: stage at k_max, caller's triangles, prefix to k [, priority prune], caller_pairs leaves -- array by array, costs bit by bit,
count by count -- the window that stage at k [, prune], caller's triangles leaves, on the inputs of tests/caller_check.py and
tests/knn_prefix_check.py, which tests/test_caller_sweep_cpu.py proves (without a GPU) to hold the shapes the rule can go wrong at and on
which it proves the rule itself from the reference's prune.  Product: every table and stats list of a sweep is the stand-alone job's,
exactly; and the sweep stages and selects what ONE job does."""
import functools

import numpy as np
import pandas as pd
import pytest

import caller_check as C
import knn_prefix_check as K

pytestmark = pytest.mark.gpu

PENALTY = 50.0


def _W():
    from same_amd import windows as W

    return W


def _filter_args(radius=C.RADIUS, angle=15, same=True):
    from same_amd.triangles import cos_threshold

    en, thr = cos_threshold(angle)
    tol = float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0
    return (radius, en, thr, tol, same)


def _fetch(st):
    W = _W()
    what = dict(rows=W._W_ALIGNED_ROWS, xy=W._W_ALIGNED_XY, rows_m=W._W_ROWS_M, rows_r=W._W_ROWS_R, kept=W._W_KEPT, pairs=W._W_PAIRS,
                costs=W._W_COSTS, staged=W._W_STAGED_PAIRS, caller=W._W_CALLER_TRIANGLES)
    out = {k: st.fetch(w) for k, w in what.items()}
    out["python"] = np.array(st.counts + (st.n_staged_pairs, st.n_selected), np.int64)      # what the binding keeps of the window
    return out


def _same_arrays(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (tag, k, a[k].shape, b[k].shape)
        x, y = (a[k].view(np.int64), b[k].view(np.int64)) if a[k].dtype == np.float64 else (a[k], b[k])
        assert np.array_equal(x, y), (tag, k)


def _tie_triangles():
    """the half-step lattice of C.tie_case (24 x 23 points, row i * 23 + j) cut into right triangles, 30 % of them dropped: lattice
    points without a triangle and every duplicate (rows past the lattice) are unconstrained and go, with rows of up to 200 pairs"""
    i, j = np.meshgrid(np.arange(23), np.arange(22), indexing="ij")
    p = (i * 23 + j).ravel()
    tris = np.vstack((np.column_stack((p, p + 23, p + 1)), np.column_stack((p + 23, p + 24, p + 1))))
    rng = np.random.default_rng(5)
    keep = tris[rng.random(len(tris)) >= 0.3]
    return np.ascontiguousarray(keep[rng.permutation(len(keep))], np.int32)


@functools.lru_cache(maxsize=None)
def _device(name, dtype="float64"):
    """(moving DeviceSection, reference DeviceSection, DeviceCallerTris, case, triangles) of one input family, uploaded once per cost
    type, binned (base: the cell-25 grid, on which boxes take both candidate paths), label codes set"""
    W = _W()
    if isinstance(name, int):
        case = C.edge_case(name)
        grid, tris = case["grid"], case["tris"]
    else:
        case = {"base": C.base_case, "tie": C.tie_case, "contention": C.contention_case}[name]()
        grid = C.GRIDS["cell 25"]
        tris = (case["tris"] if name == "base" else _tie_triangles() if name == "tie"
                else C.shuffled_triangulation(case["mov_xy"], np.random.default_rng(11), thin=0.6))
    mov = W.Section(case["mov_xy"], case["types_m"], case.get("type_id"), case.get("size"))
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov, dtype), W.DeviceSection(ref, dtype)
    codes = C.base_codes() if name == "base" else case
    dmov.set_label_codes(codes["code_m"])
    dref.set_label_codes(codes["code_r"])
    dmov.bin(*grid)
    dref.bin(*grid)
    return dmov, dref, W.DeviceCallerTris(dmov, tris), case, tris


def _fresh(st, dev, box, radius, k, args, prune=False):
    """stage at k [, prune], caller's triangles -> the call's six counts"""
    W = _W()
    dmov, dref, caller = dev[:3]
    st.stage(dmov, dref, box, radius, k, 1.0)
    if prune:
        W.priority_windows([st])
    got = W.caller_tris_windows([st], caller, *args)[0]
    assert got[2] == 0
    return got


def _derive(st, k, prune=False):
    """prefix to k [, prune], the cut list through the held mask -> the call's six counts"""
    W = _W()
    W.prefix_windows([st], k)
    if prune:
        W.priority_windows([st])
    return W.caller_pairs_windows([st])[0]


def _same_window(st, got, fresh, want, tag):
    assert got == want and st.priority == fresh.priority, (tag, got, want)
    _same_arrays(_fetch(st), _fetch(fresh), tag)


# ---- 1. the window is the fresh window -------------------------------------------------------------------------------------------------
BOXES = ("whole", "interior", "sliver", "no triangle")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", [f"base/{b}" for b in BOXES] + [f"edge/{n}" for n in C.EDGE_ROWS])
def test_prefix_and_caller_pairs_leave_the_window_the_calls_at_k_leave(oracle, tag, dtype):
    """fails without the feature: the library has no same_window_caller_pairs"""
    W = _W()
    family, which = tag.split("/")
    dev = _device("base" if family == "base" else int(which), dtype)
    box = C.base_boxes(oracle)[which] if family == "base" else dev[3]["box"]
    args = _filter_args()
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        first = _fresh(st, dev, box, C.RADIUS, C.KNN, args)
        compacted = _fetch(st)
        assert first[3] > 0 or which == "no triangle"
        ks = K.smaller(C.KNN)
        for k in ks[::-1] + ks + [1, 1, C.KNN, 2, C.KNN]:          # descending, ascending, repeated, back to the staged k and again
            before = st.ctx.stats()
            W.prefix_windows([st], k)
            cut = _fetch_plain(st)
            after = st.ctx.stats()
            if k == C.KNN:
                assert after["launches"] == before["launches"]       # the staged k: the list as staged, no launch
            fresh.stage(*dev[:2], box, C.RADIUS, k, 1.0)
            _same_arrays(cut, _fetch_plain(fresh), (tag, k, "as staged at k"))
            after = st.ctx.stats()
            got = W.caller_pairs_windows([st])[0]
            assert st.ctx.stats()["waits"] == after["waits"] + 1, (tag, k)          # one wait for the batch
            want = W.caller_tris_windows([fresh], dev[2], *args)[0]
            _same_window(st, got, fresh, want, (tag, k))
            assert got[:3] == first[:3] and got[3] == first[3] and got[5] == first[5]      # the selection is the first one's
            if k == C.KNN:
                assert got == first
                _same_arrays(_fetch(st), compacted, (tag, "back"))
        if which == "whole":
            assert first[1] > 0 and first[3] > 20 * 256 and first[5] > 256
    finally:
        st.close()
        fresh.close()


def _fetch_plain(st):
    """a window that is as a stage call leaves it (no selection to fetch)"""
    W = _W()
    what = dict(rows=W._W_ALIGNED_ROWS, xy=W._W_ALIGNED_XY, rows_m=W._W_ROWS_M, rows_r=W._W_ROWS_R, kept=W._W_KEPT, pairs=W._W_PAIRS,
                costs=W._W_COSTS, staged=W._W_STAGED_PAIRS)
    out = {k: st.fetch(w) for k, w in what.items()}
    out["python"] = np.array(st.counts + (st.n_staged_pairs,), np.int64)
    return out


# ---- 2. with the priority prune --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, k", [("base", 1), ("base", 2), ("base", 5), ("tie", 2), ("tie", 65), ("tie", 199), ("contention", 1),
                                     ("contention", 3)])
def test_with_the_priority_prune_between_the_two_calls(oracle, name, k):
    W = _W()
    dev = _device(name)
    box, radius, k_max = {"base": (C.base_boxes(oracle)["interior"], C.RADIUS, C.KNN), "tie": (C.TIE_BOX, C.TIE_K[K.TIE_KMAX], K.TIE_KMAX),
                          "contention": (C.CONTENTION_BOX, C.CONTENTION_RADIUS, K.CONTENTION_KMAX)}[name]
    args = _filter_args(radius)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        first = _fresh(st, dev, box, radius, k_max, args, prune=True)
        compacted = _fetch(st)
        assert 0 < first[1] and first[4] > 0 and st.priority[2] > 0, (first, st.priority)       # nodes went, rows kept one pair
        got = _derive(st, k, prune=True)
        want = _fresh(fresh, dev, box, radius, k, args, prune=True)
        _same_window(st, got, fresh, want, (name, k))
        assert got[4] < first[4] and st.priority[0] < compacted["staged"].shape[0]
        # the staged list stays the frame: all the pairs as staged at k, rows of removed nodes included
        assert len(st.fetch(W._W_STAGED_PAIRS)) == st.priority[0] >= st.priority[1] >= got[4]
        got = _derive(st, k_max, prune=True)
        assert got == first
        _same_arrays(_fetch(st), compacted, (name, "back"))
    finally:
        st.close()
        fresh.close()


# ---- 3. a batch larger than a launch ---------------------------------------------------------------------------------------------------
def test_a_batch_of_more_windows_than_a_launch_takes(oracle):
    """ONE prefix call and ONE caller_pairs call over 23 windows on the cell-25 grid: windows on both candidate paths, windows that keep
    no cell (they hold nothing and are passed over) and windows whose every node is removed, every launch group of 8 mixing them"""
    W = _W()
    dev = _device("base")
    kinds = C.mixed_boxes(oracle)
    boxes = [b for _k, b in kinds]
    args = _filter_args()
    states, fresh = [W.DeviceWindow() for _ in boxes], [W.DeviceWindow() for _ in boxes]
    try:
        W.stage_windows(states, *dev[:2], boxes, C.RADIUS, C.KNN, 1.0)
        first = W.caller_tris_windows(states, dev[2], *args)
        for k in (2, 5, 1, C.KNN):
            before = states[0].ctx.stats()
            W.prefix_windows(states, k)
            mid = states[0].ctx.stats()
            got = W.caller_pairs_windows(states)
            after = states[0].ctx.stats()
            assert mid["waits"] - before["waits"] == 1 and after["waits"] - mid["waits"] == 1
            W.stage_windows(fresh, *dev[:2], boxes, C.RADIUS, k, 1.0)
            want = W.caller_tris_windows(fresh, dev[2], *args)
            assert got == want, k
            for q, (kind, _box) in enumerate(kinds):
                if kind == "empty":
                    assert got[q] == (0,) * 6
                    _same_arrays(_fetch_plain(states[q]), _fetch_plain(fresh[q]), (k, q, kind))
                    continue
                _same_arrays(_fetch(states[q]), _fetch(fresh[q]), (k, q, kind))
                assert (got[q][3] == 0) == (kind == "no triangle") and (got[q][4] == 0) == (kind == "no triangle")
            if k == C.KNN:
                assert got == first
        assert sum(kind != "empty" for kind, _b in kinds) == 17
    finally:
        for st in states + fresh:
            st.close()


# ---- 4. the prefiltered form -----------------------------------------------------------------------------------------------------------
def _knife_edge():
    """the input of test_gpu_caller_triangulation.py::test_a_cosine_at_the_threshold_is_decided_on_the_host: three cells of one triangle
    moved so that its smallest angle is min_angle_deg to within 1 ulp of the cosine -> (reference frame, moving frame, triangles, type
    columns, the moved corner)"""
    import math
    from fractions import Fraction

    from same_amd.triangles import cos_threshold
    from test_gpu_caller_triangulation import _plain

    r_df, m_df, tri, cols = _plain()
    m_df = m_df.copy()
    _en, thr = cos_threshold(15)
    a, b, c = tri[np.argmin(np.abs(m_df["X"].to_numpy()[tri].mean(axis=1) - 300) + np.abs(m_df["Y"].to_numpy()[tri].mean(axis=1) - 300))]
    ax, ay = m_df.loc[a, "X"], m_df.loc[a, "Y"]
    ang = np.arccos(thr)
    fma = lambda p, q, r: float(Fraction(p) * Fraction(q) + Fraction(r))

    def corner_cos(p1, p2, p3):
        v1x, v1y, v2x, v2y = p1[0] - p2[0], p1[1] - p2[1], p3[0] - p2[0], p3[1] - p2[1]
        n1, n2 = math.sqrt(fma(v1y, v1y, v1x * v1x)), math.sqrt(fma(v2y, v2y, v2x * v2x))
        return fma(v1y, v2y, v1x * v2x) / (n1 * n2)

    for scale in np.linspace(8.0, 12.0, 4001):
        bx, by, cx, cy = float(ax + scale), float(ay), float(ax + scale * np.cos(ang)), float(ay + scale * np.sin(ang))
        if abs(corner_cos((bx, by), (float(ax), float(ay)), (cx, cy)) - thr) <= np.spacing(abs(thr)):
            break
    else:
        raise AssertionError("no scale puts the cosine at the threshold")
    m_df.loc[b, ["X", "Y"]] = (bx, by)
    m_df.loc[c, ["X", "Y"]] = (cx, cy)
    return r_df, m_df, tri, cols, (float(ax), float(ay))


def test_the_prefiltered_form_holds_the_hosts_mask(oracle):
    """A window left as staged because a cosine sits at the threshold, called again with the host's mask (the prefiltered form): prefix +
    caller_pairs equal the fresh window at k given the same two calls, and the finish with SAME_TRIS_KEPT over the host's list agrees."""
    from same_amd.triangles import filter_triangles_by_radius

    W = _W()
    r_df, m_df, tri, cols, (ax, ay) = _knife_edge()
    mov, ref = W.Section.from_frame(m_df, list(cols)), W.Section.from_frame(r_df, list(cols))
    dmov, dref = W.DeviceSection(mov), W.DeviceSection(ref)
    radius, k_max = 30.0, 4
    args = _filter_args(radius)
    box = (ax - 100.0, ax + 100.0, ay - 100.0, ay + 100.0)
    dmov.bin(0.0, 0.0, 50.0)
    dref.bin(0.0, 0.0, 50.0)
    caller = W.DeviceCallerTris(dmov, tri)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()

    def two_calls(s, k):
        """stage at k, the call that reports near, the host's filter, the call again with its mask -> (counts, the host's kept list)"""
        s.stage(dmov, dref, box, radius, k, 1.0)
        got = W.caller_tris_windows([s], caller, *args)[0]
        assert got[2] > 0 and got[3:5] == s.counts[2:]                    # near: left as staged
        axy0, rows0, tris0 = s.fetch(W._W_ALIGNED_XY), s.fetch(W._W_ALIGNED_ROWS), s.fetch(W._W_CALLER_TRIANGLES)
        tid = mov.type_id[rows0] if mov.type_id is not None else None
        kept, gone = filter_triangles_by_radius(axy0, tris0, radius, ignore_same_type_triangles=True, remove_unconstrained_nodes=True,
                                                min_angle_deg=15, verbose=False, ctx=s.ctx, _rows_as_array=True, _type_id=tid)
        mask = np.zeros(len(rows0), np.uint8)
        mask[sorted(gone)] = 1
        kept = np.asarray(kept).reshape(-1, 3)
        kept = kept[(mask[kept] == 0).all(axis=1)]
        return W.caller_tris_windows([s], caller, *args, removed=[mask])[0], (np.cumsum(mask == 0) - 1)[kept].astype(np.int32).reshape(-1, 3)

    try:
        first, kept0 = two_calls(st, k_max)
        assert first[1] > 0 and first[2] == 0 and len(kept0) > 20
        compacted = _fetch(st)
        for k in (2, 1, 3, k_max):
            got = _derive(st, k)
            want, kept = two_calls(fresh, k)
            assert np.array_equal(kept, kept0)
            _same_window(st, got, fresh, want, k)
            a, b = st.finish(kept0, PENALTY), fresh.finish(kept, PENALTY)
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
            assert a[2]["matched"] > 20
            for what in (W._W_TRIANGLES, W._W_SIGNS, W._W_MATCH):
                assert np.array_equal(st.fetch(what), fresh.fetch(what)), (k, what)
        _same_arrays(_fetch(st), compacted, "back")
    finally:
        for h in (st, fresh, caller, dmov, dref):
            h.close()


def test_sweep_over_the_knife_edge_input_equals_the_jobs():
    r_df, m_df, tri, cols, _a = _knife_edge()
    op = dict(radius=30, knn=4, window_size=200, overlap=50, min_cells_per_window=20, **KEY)
    _sweep_equals_the_jobs(r_df, m_df, list(cols), op, [{"knn": 2}, {}, {"knn": 3, "no_match_penalty": 30}], "near", moving_delaunay=tri)


# ---- 5. finish on it -------------------------------------------------------------------------------------------------------------------
def _modes(mult):
    from same_amd.window_mode import WindowMode

    return {"greedy": WindowMode(), "assignment + local": WindowMode("assignment", "local", 32, 5.0),
            "transport + capacity": WindowMode("transport", "capacity", 32, 5.0, (2, mult, 0.5))}


@functools.lru_cache(maxsize=None)
def _metacell_reference():
    """the base case with a reference of metacells (sizes 1 .. 3) -> (dmov, dref, caller)"""
    W = _W()
    case = C.base_case()
    size_r = np.random.default_rng(3).integers(1, 4, len(case["ref_xy"])).astype(np.float64)
    mov = W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"])
    ref = W.Section(case["ref_xy"], case["types_r"], None, size_r)
    dmov, dref = W.DeviceSection(mov), W.DeviceSection(ref)
    dmov.bin(*C.GRIDS["cell 75"])
    dref.bin(*C.GRIDS["cell 75"])
    return dmov, dref, W.DeviceCallerTris(dmov, case["tris"])


def _finish(st, args, mode):
    W = _W()
    kept, added, near, row, flag, stats = W.filter_finish_windows([st], None, *args, PENALTY, mode=mode, from_caller=True)[0]
    assert near == 0
    return dict(counts=(kept, added), row=row, flag=flag, stats=stats, assignment=st.assignment, refine=st.refine, tris=st.fetch(W._W_TRIANGLES),
                signs=st.fetch(W._W_SIGNS), weights=st.fetch(W._W_WEIGHTS), match=st.fetch(W._W_MATCH))


def _same_record(a, b, tag):
    for k in ("counts", "stats", "assignment", "refine"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for k in ("row", "flag", "tris", "signs", "weights", "match"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("mult", [None, 3])
@pytest.mark.parametrize("name", ["greedy", "assignment + local", "transport + capacity"])
def test_finish_on_the_derived_window_is_the_finish_on_the_fresh_one(oracle, name, mult):
    W = _W()
    dev = _metacell_reference()
    mode = _modes(mult)[name]
    box = C.base_boxes(oracle)["interior"]
    args = _filter_args()
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        _fresh(st, dev, box, C.RADIUS, C.KNN, args)
        first = _finish(st, args, mode)                      # a finish of the first compaction: the prefix starts over
        for k in (2, 5, 1):
            _derive(st, k)
            _fresh(fresh, dev, box, C.RADIUS, k, args)
            a, b = _finish(st, args, mode), _finish(fresh, args, mode)
            _same_record(a, b, (name, mult, k))
            assert a["stats"]["matched"] > 100
        _derive(st, C.KNN)
        _same_record(_finish(st, args, mode), first, (name, mult, "back"))
    finally:
        st.close()
        fresh.close()


def test_limits_are_read_over_the_prefix_as_staged_where_only_removed_cells_name_a_metacell():
    """the input of test_a_metacell_reference_named_only_by_removed_cells_still_sets_the_limits, its sets cut to knn 2: the largest
    references are reachable only from cells the triangulation leaves unconstrained, so only the pair list AS STAGED at that knn -- rows
    of removed cells included -- grants the other references their capacity"""
    from scipy.spatial import Delaunay
    from same_amd import synth

    cells = synth.make_cells(1500, 3, seed=91)
    r_df = synth.to_frame(cells)
    m_df = pd.concat([synth.to_frame(synth.make_jittered(cells, seed=92, drop=0.0)),
                      synth.to_frame(synth.make_jittered(cells, seed=93, drop=0.0))], ignore_index=True)
    m_df["Cell_Num_Old"] = np.arange(len(m_df)) * 3 + 1
    rx, ry = r_df["X"].to_numpy(), r_df["Y"].to_numpy()
    corner = (rx < 60) & (ry < 60)
    r_df["size"] = np.where(corner, 3.0, np.where(np.arange(len(r_df)) % 2 == 0, 1.5, 1.0))
    tri = Delaunay(m_df[["X", "Y"]].to_numpy()).simplices
    mx, my = m_df["X"].to_numpy(), m_df["Y"].to_numpy()
    tri = tri[~((mx[tri] < 100) & (my[tri] < 100)).any(axis=1)]
    op = dict(OP, max_matches=1, ref_metacell_match_multiplier=None, penalty_coeff=0.5, hip_incumbent="transport", hip_refine="capacity", **KEY)
    sets = [{"knn": 2}, {}, {"knn": 2, "ref_metacell_match_multiplier": 3}, {"knn": 3, "hip_incumbent": "greedy"}]
    got = _sweep_equals_the_jobs(r_df, m_df, list(synth.type_columns(3)), op, sets, "limits", moving_delaunay=tri, workers=1)
    for q in (0, 2):
        assert got[q][1][0]["ref_extra_matches"] > 0, q          # the first window uses the capacity that only the staged frame grants


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_caller_pairs_refuses_what_holds_no_selection(oracle):
    from scipy.spatial import Delaunay

    from same_amd import _lib

    W = _W()
    dev = _device("base")
    box = C.base_boxes(oracle)["interior"]
    args = _filter_args()
    st, other, fresh = W.DeviceWindow(), W.DeviceWindow(), W.DeviceWindow()

    def refused(states):
        with pytest.raises(_lib.SameHipError) as e:
            W.caller_pairs_windows(states)
        assert e.value.code == _lib.SAME_EINVAL

    try:
        refused([st])                                          # not staged
        st.stage(*dev[:2], box, C.RADIUS, C.KNN, 1.0)
        staged = _fetch_plain(st)
        refused([st])                                          # never given the caller's triangles
        _same_arrays(_fetch_plain(st), staged, "never selected")
        W.prefix_windows([st], 3)
        refused([st])                                          # ... cut or not
        W.prefix_windows([st], C.KNN)
        _same_arrays(_fetch_plain(st), staged, "never selected, back")
        W.caller_tris_windows([st], dev[2], *args)
        compacted = _fetch(st)
        refused([st])                                          # compacted, not cut since: nothing is held, the window is the compaction
        _same_arrays(_fetch(st), compacted, "not cut")
        W.prefix_windows([st], 2)
        cut = _fetch_plain(st)
        # finished since its prefix (the window as staged at 2, over scipy's simplices)
        tris = Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices.astype(np.int32)
        W.filter_finish_windows([st], [tris], *args, PENALTY)
        refused([st])
        _same_arrays(_fetch_plain(st), cut, "finished")
        # the next prefix starts over; one bad window refuses the batch and leaves the good one as it was
        W.prefix_windows([st], 2)
        refused([st, other])
        other.stage(*dev[:2], box, C.RADIUS, C.KNN, 1.0)
        refused([other, st])
        _same_arrays(_fetch_plain(st), cut, "batch")
        got = W.caller_pairs_windows([st])[0]
        want = _fresh(fresh, dev, box, C.RADIUS, 2, args)
        _same_window(st, got, fresh, want, "after the refusals")
        refused([st])                                          # a second call without a prefix between
        # a caller_tris call on a window that holds a selection works from the cut list and replaces what is held
        W.prefix_windows([st], 5)
        got = W.caller_tris_windows([st], dev[2], *args)[0]
        want = _fresh(fresh, dev, box, C.RADIUS, 5, args)
        _same_window(st, got, fresh, want, "selected again")
    finally:
        for h in (st, other, fresh):
            h.close()


# ---- 7. the product --------------------------------------------------------------------------------------------------------------------
KEY = {"hip_caller_delaunay": "device"}
OP = dict(radius=30, knn=6, window_size=200, overlap=50, min_cells_per_window=20)
# three knn values, two no-match penalties, the capacity-aware start and search, a multiplier of its own; not in the order the pass takes them
SETS = [{"knn": 4, "hip_incumbent": "assignment", "hip_refine": "local"},
        {},
        {"knn": 2, "no_match_penalty": 30},
        {"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2, "penalty_coeff": 0.5},
        {"knn": 4, "hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2, "penalty_coeff": 0.5, "ref_metacell_match_multiplier": 2}]


def _metacells(kind):
    from test_gpu_caller_triangulation import _metacells as made

    return made(kind)


def _sweep_equals_the_jobs(ref, mov, cols, op, sets, tag, **kw):
    import same_amd

    got = same_amd.sliding_window_sweep(ref, mov, sets, commonCT=cols, optim_params=dict(op), return_stats=True, **kw)
    assert len(got) == len(sets)
    out = []
    for q, ps in enumerate(sets):
        want, wst = same_amd.sliding_window_incumbent(ref, mov, commonCT=cols, optim_params={**op, **ps}, return_stats=True, **kw)
        table, st = got[q]
        pd.testing.assert_frame_equal(table, want, check_exact=True, obj=f"{tag} set {q}")
        assert [list(s) for s in st] == [list(s) for s in wst] and st == wst, (tag, q)
        out.append((table, st))
    return out


def _removed_per_window(run):
    """the `removed` counts the caller calls of `run()` report (the tables alone do not show that nodes went)"""
    W = _W()
    seen, inner = [], W.caller_tris_windows

    def spy(states, *a, **k):
        out = inner(states, *a, **k)
        seen.extend(o[1] for o in out)
        return out

    W.caller_tris_windows = spy
    try:
        run()
    finally:
        W.caller_tris_windows = inner
    return seen


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
@pytest.mark.parametrize("kind", ["ms3", "ms1", "aligned_only"])
def test_sweep_over_metacell_objects_is_the_stand_alone_jobs(kind, merge):
    ref, mc, cols = _metacells(kind)
    got = _sweep_equals_the_jobs(ref, mc, list(cols), dict(OP, **KEY), SETS, (kind, merge), merge=merge)
    st0 = got[1][1]
    assert len(st0) >= 9 and all(len(t) > 100 for t, _s in got)
    # the sets differ: fewer pairs at a smaller knn
    assert all(a["pairs"] < b["pairs"] for a, b in zip(got[2][1], st0)) and all(a["pairs"] <= b["pairs"] for a, b in zip(got[0][1], st0))
    assert "mip_objective" in got[0][1][0] and "mip_gap" in got[3][1][0] and "objective" not in st0[0]


def test_sweep_over_metacells_with_window_local_indices_and_two_workers():
    ref, mc, cols = _metacells("ms3")
    got = _sweep_equals_the_jobs(ref, mc, list(cols), dict(OP, **KEY), SETS[:3], "local indices", window_local_indices=True, workers=2, batch=3)
    assert all("ref_idx" in t.columns for t, _s in got)


def test_sweep_over_metacells_over_resident_frames():
    import same_amd

    ref, mc, cols = _metacells("ms3")
    with same_amd.resident_frames(ref, mc) as frames:
        _sweep_equals_the_jobs(frames, mc, list(cols), dict(OP, **KEY), SETS[1:4], "resident")


def test_sweep_over_metacells_with_the_priority_prune_on_the_device():
    ref, mc, cols = _metacells("ms3")
    op = dict(OP, ignore_knn_if_matched=True, hip_priority_prune="device", **KEY)
    got = _sweep_equals_the_jobs(ref, mc, list(cols), op, SETS[:4], "priority")
    for _t, st in got:
        assert all(s["pairs_staged"] > s["pairs"] and s["priority_rows"] > 0 for s in st)
    assert all(a["pairs_staged"] < b["pairs_staged"] for a, b in zip(got[2][1], got[1][1]))      # `pairs_staged` is the set's own knn's


def test_sweep_with_a_moving_delaunay_array_on_plain_frames():
    """ids offset by 10^6 in a column of their own; the triangulation thinned by half (nodes go in every window) and with no triangle over
    the first window's box (every node of it goes: skipped for every set)"""
    import same_amd
    from test_gpu_caller_triangulation import _plain, _thinned

    r_df, m_df, tri, cols = _plain()
    x, y = m_df["X"].to_numpy(), m_df["Y"].to_numpy()
    hole = tri[~((x[tri] < 205) & (y[tri] < 205)).any(axis=1)]
    ids = m_df["vid"].to_numpy()[_thinned(hole, len(m_df), 9, 0.5)]
    kw = dict(moving_delaunay=ids, moving_delaunay_vertex_col="vid")
    got = _sweep_equals_the_jobs(r_df, m_df, list(cols), dict(OP, **KEY), SETS[:3], "array", **kw)
    assert all(a["pairs"] < b["pairs"] for a, b in zip(got[2][1], got[1][1])) and all(len(t) > 100 for t, _s in got)
    removed = _removed_per_window(lambda: same_amd.sliding_window_sweep(r_df, m_df, SETS[:3], commonCT=list(cols), optim_params=dict(OP, **KEY),
                                                                       workers=1, **kw))
    assert len(removed) == len(got[1][1]) + 1 and sum(r > 0 for r in removed) >= 2, removed      # one window more than the stats: the skipped one


# ---- 8. the sharing is real ------------------------------------------------------------------------------------------------------------
def test_a_sweep_over_metacells_stages_and_selects_what_one_job_does(monkeypatch):
    """fails without the feature: the sweep over MetaCell inputs makes every job's stage calls.  The binding's calls are counted where
    the walk makes them: a sweep of S sets over G knn values makes ONE job's stage and caller_tris calls, (G - 1) prefix and as many
    caller_pairs calls per batch, and the jobs' sum of finish calls."""
    import same_amd

    W = _W()
    names = {"stage_windows": "stage", "caller_tris_windows": "caller_tris", "prefix_windows": "prefix", "caller_pairs_windows": "caller_pairs",
             "filter_finish_windows": "finish"}
    seen = dict.fromkeys(names.values(), 0)

    def counting(name, key):
        inner = getattr(W, name)

        def call(*a, **k):
            seen[key] += 1
            return inner(*a, **k)

        monkeypatch.setattr(W, name, call)

    for name, key in names.items():
        counting(name, key)
    ref, mc, cols = _metacells("ms3")
    kw = dict(commonCT=list(cols), workers=1, batch=4)
    op = dict(OP, **KEY)

    def spent(run):
        for k in seen:
            seen[k] = 0
        run()
        return dict(seen)

    jobs = [spent(lambda ps=ps: same_amd.sliding_window_incumbent(ref, mc, optim_params={**op, **ps}, **kw)) for ps in SETS]
    sweep = spent(lambda: same_amd.sliding_window_sweep(ref, mc, SETS, optim_params=dict(op), **kw))
    one = jobs[1]
    assert one["stage"] >= 3 and one["caller_tris"] == one["stage"] and one["prefix"] == 0 and one["caller_pairs"] == 0
    assert all(j["stage"] == one["stage"] and j["caller_tris"] == one["caller_tris"] and j["finish"] == one["finish"] for j in jobs)
    assert sweep["stage"] == one["stage"] and sweep["caller_tris"] == one["caller_tris"]
    assert sweep["prefix"] == sweep["caller_pairs"] == 2 * one["stage"]        # knn 6 is the list as staged; 4 and 2: one call each per batch
    assert sweep["finish"] == sum(j["finish"] for j in jobs) == len(SETS) * one["finish"]
