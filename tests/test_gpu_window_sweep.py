"""same_window_knn_prefix (csrc/window_knn_prefix.hip) at the LIBRARY and same_amd.sliding_window_sweep as a product.
Library: a window staged at k_max and cut to k is, array by array and bit by bit, the window a stage call at k leaves -- on the input
families of tests/knn_prefix_check.py, which tests/test_window_sweep_cpu.py proves (without a GPU) to hold the shapes the rule can go wrong
at, and whose prefix statement it proves equal to the reference's prune at k.  Layering: the priority prune and the finish calls on a cut
window are those on the fresh one.  Product: every table and stats list of a sweep is the stand-alone job's, exactly; and the sweep stages
and triangulates what ONE job does."""
import functools

import numpy as np
import pandas as pd
import pytest

import caller_check as C
import knn_prefix_check as K

pytestmark = pytest.mark.gpu


def _W():
    from same_amd import windows as W

    return W


def _what(W):
    return dict(rows=W._W_ALIGNED_ROWS, xy=W._W_ALIGNED_XY, rows_m=W._W_ROWS_M, rows_r=W._W_ROWS_R, kept=W._W_KEPT, pairs=W._W_PAIRS,
                costs=W._W_COSTS, staged=W._W_STAGED_PAIRS)


def _fetch(st):
    W = _W()
    return {k: st.fetch(w) for k, w in _what(W).items()}


def _same_arrays(a, b, tag):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (tag, k)
        assert np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]), (tag, k)


def _sections(tag, dtype):
    """(moving DeviceSection, reference DeviceSection) of one family's case, uploaded once per case and cost type, label codes set where
    it has them"""
    return _uploaded(tag if tag.startswith("edge") else tag.split("/")[0], dtype)


@functools.lru_cache(maxsize=None)
def _uploaded(tag, dtype):
    W = _W()
    name = tag.split("/")[0]
    case = {"base": C.base_case, "tie": C.tie_case, "contention": C.contention_case}[name]() if name != "edge" else C.edge_case(int(tag.split("/")[1]))
    mov = W.Section(case["mov_xy"], case["types_m"], case.get("type_id"), case.get("size"))
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov, dtype), W.DeviceSection(ref, dtype)
    codes = C.base_codes() if name == "base" else case
    if "code_m" in codes:
        dmov.set_label_codes(codes["code_m"])
        dref.set_label_codes(codes["code_r"])
    return dmov, dref


def _family(oracle, tag):
    return next(f for f in K.families(oracle) if f[0] == tag)


FAMILY_TAGS = ("base/whole", "base/interior", "base/sliver", "base/beside", "base/no triangle", "base/empty", "tie", "contention",
               "edge/255", "edge/256", "edge/257", "edge/16385")


# ---- 1. the library, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", FAMILY_TAGS)
def test_prefix_leaves_the_window_a_stage_call_at_k_leaves(oracle, tag, dtype):
    """fails without the feature: the library has no same_window_knn_prefix"""
    W = _W()
    assert {f[0] for f in K.families(oracle)} == set(FAMILY_TAGS)
    _tag, case, box, radius, k_max = _family(oracle, tag)
    dmov, dref = _sections(tag, dtype)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        counts0 = st.stage(dmov, dref, box, radius, k_max, 1.0)
        staged0 = _fetch(st)
        rows, _rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, radius, k_max, oracle)
        assert np.array_equal(staged0["rows"], rows) and np.array_equal(staged0["pairs"], pairs)      # the list the CPU test reasoned about
        ks = K.smaller(k_max)
        order = ks[::2] + ks[1::2][::-1] + [k_max, 1, k_max]             # up, down, back to the staged list, and once more
        for k in order:
            got = W.prefix_windows([st], k)[0]
            want = fresh.stage(dmov, dref, box, radius, k, 1.0)
            assert got == want and st.counts == fresh.counts and st.n_staged_pairs == fresh.n_staged_pairs, (tag, k, got, want)
            _same_arrays(_fetch(st), _fetch(fresh), (tag, k))
            if k == k_max:
                assert got == counts0
                _same_arrays(_fetch(st), staged0, (tag, "back"))
            if len(pairs):       # ... and the host statement's, whose equality with the reference's prune the CPU test proves
                state = K.prefix(rows, pairs.astype(np.int64), staged0["costs"], staged0["rows_r"], k)
                assert np.array_equal(st.fetch(W._W_PAIRS), state["pairs"]) and np.array_equal(st.fetch(W._W_COSTS), state["costs"]), (tag, k)
    finally:
        st.close()
        fresh.close()


def test_prefix_of_a_batch_of_more_windows_than_a_launch_takes(oracle):
    """ONE call over 23 windows of very different sizes, among them windows whose box holds rows and no pair and windows whose box holds
    nothing: every window is the one a batch staged at k leaves, its counts at its own index"""
    W = _W()
    dmov, dref = _sections("base/whole", "float64")
    kinds = C.priority_boxes()
    boxes = [b for _k, b in kinds]
    states, fresh = [W.DeviceWindow() for _ in boxes], [W.DeviceWindow() for _ in boxes]
    try:
        W.stage_windows(states, dmov, dref, boxes, C.RADIUS, K.BASE_K, 1.0)
        for k in (3, 1, K.BASE_K, 7):
            got = W.prefix_windows(states, k)
            want = W.stage_windows(fresh, dmov, dref, boxes, C.RADIUS, k, 1.0)
            assert got == want, k
            for q, (kind, _box) in enumerate(kinds):
                _same_arrays(_fetch(states[q]), _fetch(fresh[q]), (k, q, kind))
                assert (got[q][3] == 0) == (kind != "pairs")
        sizes = sorted(c[2] for c in got if c[3])
        assert len(sizes) >= 8 and sizes[0] < 256 < sizes[-2] and sizes[-1] > 5000
    finally:
        for st in states + fresh:
            st.close()


def test_prefix_refuses_what_it_cannot_derive(oracle):
    from same_amd import _lib

    W = _W()
    dmov, dref = _sections("base/whole", "float64")
    box = C.base_boxes(oracle)["interior"]
    st, other = W.DeviceWindow(), W.DeviceWindow()
    try:
        with pytest.raises(_lib.SameHipError) as e:          # not staged
            W.prefix_windows([st], 1)
        assert e.value.code == _lib.SAME_EINVAL
        counts = st.stage(dmov, dref, box, C.RADIUS, 6, 1.0)
        before = _fetch(st)
        W.prefix_windows([st], 3)
        cut = _fetch(st)
        for k in (7, 449, 0, -1):                            # above the staged k, below 1: nothing changes
            with pytest.raises(_lib.SameHipError) as e:
                W.prefix_windows([st], k)
            assert e.value.code == _lib.SAME_EINVAL
            _same_arrays(_fetch(st), cut, k)
        with pytest.raises(_lib.SameHipError):               # one bad window refuses the batch, the good one is untouched
            W.prefix_windows([st, other], 2)
        _same_arrays(_fetch(st), cut, "batch")
        assert W.prefix_windows([st], 6)[0] == counts
        _same_arrays(_fetch(st), before, "back")
    finally:
        st.close()
        other.close()


# ---- 2. layering -----------------------------------------------------------------------------------------------------------------------
def _filter_args(radius, angle, same):
    from same_amd.triangles import cos_threshold

    en, thr = cos_threshold(angle)
    tol = float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0
    return (radius, en, thr, tol, same)


def _finish(st, radius, same, penalty, mode):
    """the finish call over scipy's simplices of the window's kept cells -> everything it leaves"""
    from scipy.spatial import Delaunay

    W = _W()
    tris = Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices.astype(np.int32)
    kept, added, near, row, flag, stats = W.filter_finish_windows([st], [tris], *_filter_args(radius, 15, same), penalty, mode=mode)[0]
    assert near == 0
    return dict(counts=(kept, added), row=row, flag=flag, stats=stats, assignment=st.assignment, refine=st.refine, tris=st.fetch(W._W_TRIANGLES),
                signs=st.fetch(W._W_SIGNS), weights=st.fetch(W._W_WEIGHTS), match=st.fetch(W._W_MATCH))


def _same_record(a, b, tag):
    for k in ("counts", "stats", "assignment", "refine"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for k in ("row", "flag", "tris", "signs", "weights", "match"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


def _modes():
    from same_amd.window_mode import WindowMode

    return {"greedy": WindowMode(), "assignment + local": WindowMode("assignment", "local", 32, 5.0),
            "transport + capacity": WindowMode("transport", "capacity", 32, 5.0, (2, None, 0.5))}


@pytest.mark.parametrize("tag, k", [("base/interior", 3), ("base/interior", 1), ("tie", 65), ("tie", 2)])
def test_priority_prune_on_a_prefix_is_the_prune_on_the_fresh_window(oracle, tag, k):
    W = _W()
    _tag, _case, box, radius, k_max = _family(oracle, tag)
    dmov, dref = _sections(tag, "float64")
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        st.stage(dmov, dref, box, radius, k_max, 1.0)
        W.priority_windows([st])                             # a prune of the staged list first: the prefix must forget it
        W.prefix_windows([st], k)
        fresh.stage(dmov, dref, box, radius, k, 1.0)
        got, want = W.priority_windows([st])[0], W.priority_windows([fresh])[0]
        assert got == want and st.counts == fresh.counts and got[1] <= got[0], (got, want)
        if tag != "tie" or k > 1:
            assert got[2] > 0 and got[3] > 0
        _same_arrays(_fetch(st), _fetch(fresh), (tag, k))
        for name, mode in list(_modes().items())[:2] if tag.startswith("base") else []:      # (the lattice has no Delaunay triangulation)
            _same_record(_finish(st, radius, False, 50.0, mode), _finish(fresh, radius, False, 50.0, mode), (tag, k, name))
        # and back to the staged list, pruned: the first prune's own result
        W.prefix_windows([st], k_max)
        fresh.stage(dmov, dref, box, radius, k_max, 1.0)
        assert W.priority_windows([st])[0] == W.priority_windows([fresh])[0]
        _same_arrays(_fetch(st), _fetch(fresh), (tag, "back"))
    finally:
        st.close()
        fresh.close()


@pytest.mark.parametrize("name", ["greedy", "assignment + local", "transport + capacity"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_finish_on_a_prefix_is_the_finish_on_the_fresh_window(oracle, name, k):
    W = _W()
    mode = _modes()[name]
    _tag, _case, box, radius, k_max = _family(oracle, "base/interior")
    dmov, dref = _sections("base/interior", "float64")
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        st.stage(dmov, dref, box, radius, k_max, 1.0)
        first = _finish(st, radius, True, 50.0, mode)       # a finish of the staged list first: the prefix starts over
        W.prefix_windows([st], k)
        fresh.stage(dmov, dref, box, radius, k, 1.0)
        a, b = _finish(st, radius, True, 50.0, mode), _finish(fresh, radius, True, 50.0, mode)
        _same_record(a, b, (name, k))
        assert a["stats"]["matched"] > 100
        W.prefix_windows([st], k_max)
        _same_record(_finish(st, radius, True, 50.0, mode), first, (name, "back"))
    finally:
        st.close()
        fresh.close()


def test_reference_limits_are_read_over_the_prefix_list(oracle):
    """700 rows around ONE reference of size 2, two references of size 5 on the ring behind it.  Staged at 8 the list names the ring, so
    the frame's largest size is 5 and the centre may take 2 * 5 rows; cut to k = 1 the list names the centre alone, the largest size is 2
    and it takes 2 * 2 -- what a window staged at 1 gives.  A limit read over the list as staged would match 10 rows."""
    from same_amd.window_mode import WindowMode

    W = _W()
    case = C.contention_case()
    size_r = np.array([2, 5, 1, 1, 5, 1, 1, 1, 1], np.float64)
    dmov = W.DeviceSection(W.Section(case["mov_xy"], case["types_m"], None, None))
    dref = W.DeviceSection(W.Section(case["ref_xy"], case["types_r"], None, size_r))
    mode = WindowMode("transport", "capacity", 32, 5.0, (2, None, 0.01))
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        box, radius = C.CONTENTION_BOX, C.CONTENTION_RADIUS
        st.stage(dmov, dref, box, radius, K.CONTENTION_KMAX, 1.0)
        wide = st.fetch(W._W_PAIRS)
        matched, certified = {}, True       # (a start the device does not certify is the host's to solve: its numbers prove nothing here)
        for k in (1, 2, K.CONTENTION_KMAX):
            W.prefix_windows([st], k)
            fresh.stage(dmov, dref, box, radius, k, 1.0)
            pairs = st.fetch(W._W_PAIRS)
            limits = W.window_ref_limits(size_r, pairs, mode.capacity)
            a, b = _finish(st, radius, False, 1.0e6, mode), _finish(fresh, radius, False, 1.0e6, mode)
            _same_record(a, b, k)
            took = np.bincount(a["match"][a["match"] >= 0], minlength=9)
            assert (took <= limits).all(), (k, took, limits)
            matched[k] = a["stats"]["matched"]
            certified = certified and a["assignment"]["flags"] == 0
            print(f"k={k}: limits {limits.tolist()} took {took.tolist()} matched {matched[k]} start flags {a['assignment']['flags']}")
            if k == 1:
                assert limits[0] == 4 and W.window_ref_limits(size_r, wide, mode.capacity)[0] == 10
                assert took[0] == matched[1] <= 4 and (matched[1] == 4 or not certified)
        assert matched[K.CONTENTION_KMAX] > matched[1] or not certified
    finally:
        st.close()
        fresh.close()
        dmov.close()
        dref.close()


# ---- 3. the product ----------------------------------------------------------------------------------------------------------------------
WIN = dict(window_size=300, overlap=75, min_cells_per_window=20)
OP = dict(radius=30, knn=8, **WIN)
# three knn values, two no-match penalties, the three start / search combinations; not in the order the pass takes them
SETS = [{"knn": 4, "hip_incumbent": "assignment", "hip_refine": "local"},
        {},
        {"knn": 2, "no_match_penalty": 30},
        {"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2, "penalty_coeff": 0.5},
        {"knn": 4, "hip_refine": "local", "delaunay_penalty": 25},
        {"no_match_penalty": 30}]


@functools.lru_cache(maxsize=None)
def _frames(n=4000, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1)), tuple(synth.type_columns(6))


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


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
@pytest.mark.parametrize("route", [None, "native", "device"])
def test_sweep_tables_and_stats_are_the_stand_alone_jobs(route, merge):
    """fails without the feature: same_amd has no sliding_window_sweep"""
    ref, mov, cols = _frames()
    op = dict(OP) if route is None else dict(OP, hip_delaunay=route)
    got = _sweep_equals_the_jobs(ref, mov, list(cols), op, SETS, (route, merge), merge=merge)
    st0 = got[1][1]
    assert 6 <= len(st0) <= 12 and min(s["pairs"] for s in st0) > 2000 and len(got[1][0]) > 2500
    # the sets differ: fewer pairs at a smaller knn, another matching at another penalty / start
    assert all(a["pairs"] < b["pairs"] for a, b in zip(got[2][1], st0))
    assert [s["matched"] for s in got[5][1]] != [s["matched"] for s in st0] or not got[5][0].equals(got[1][0])
    assert "mip_objective" in got[0][1][0] and "mip_gap" in got[3][1][0] and "objective" not in st0[0]


def test_sweep_with_window_local_indices_and_two_workers():
    ref, mov, cols = _frames()
    got = _sweep_equals_the_jobs(ref, mov, list(cols), OP, SETS[:3], "local indices", window_local_indices=True, workers=2, batch=3)
    assert all("ref_idx" in t.columns for t, _s in got)


def test_sweep_over_resident_frames():
    import same_amd

    ref, mov, cols = _frames()
    with same_amd.resident_frames(ref, mov) as frames:
        _sweep_equals_the_jobs(frames, mov, list(cols), OP, SETS[1:4], "resident")


def test_sweep_with_the_priority_prune_on_the_device():
    ref, mov, cols = _frames()
    op = dict(OP, ignore_knn_if_matched=True, hip_priority_prune="device")
    got = _sweep_equals_the_jobs(ref, mov, list(cols), op, SETS, "priority")
    for _t, st in got:
        assert all(s["pairs_staged"] > s["pairs"] and s["priority_rows"] > 0 for s in st)
    assert all(a["pairs_staged"] < b["pairs_staged"] for a, b in zip(got[2][1], got[1][1]))      # `pairs_staged` is the set's own knn's


def test_sweep_over_metacell_objects_runs_set_by_set():
    import same_amd
    from same_amd import synth

    cells = synth.make_cells(2400, 3, seed=71)
    r_c, a_c = synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=72))
    a_c["Cell_Num_Old"] = np.arange(len(a_c)) * 2 + 7
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    op = dict(radius=30, knn=4, window_size=200, overlap=50, min_cells_per_window=20)
    got = _sweep_equals_the_jobs(collapse(r_c), collapse(a_c), list(synth.type_columns(3)), op, [{"knn": 2}, {"no_match_penalty": 30}], "metacells")
    assert all(len(t) > 100 for t, _s in got)


# ---- 4. the sharing is real ------------------------------------------------------------------------------------------------------------
def test_a_sweep_stages_and_triangulates_what_one_job_does(monkeypatch):
    """The binding's stage calls, the tickets asked of the triangulator and the prefix calls of a sweep against ONE job's; its finish
    calls against the jobs' sum.  (include/same_hip_diag.h counts launches, copies and waits, not calls: the calls are counted where the
    binding makes them.)"""
    import same_amd
    from same_amd import delaunay

    W = _W()
    seen = {"stage": 0, "prefix": 0, "finish": 0, "tickets": 0}

    def counting(name, key):
        inner = getattr(W, name)

        def call(*a, **k):
            seen[key] += 1
            return inner(*a, **k)

        monkeypatch.setattr(W, name, call)

    counting("stage_windows", "stage")
    counting("prefix_windows", "prefix")
    counting("filter_finish_windows", "finish")

    class Counting(delaunay.QhullTriangulator):
        def submit(self, points, key=None):
            seen["tickets"] += 1
            return super().submit(points, key)

    ref, mov, cols = _frames()
    kw = dict(commonCT=list(cols), workers=1, batch=4, triangulator=Counting())

    def spent(run):
        for k in seen:
            seen[k] = 0
        run()
        return dict(seen)

    jobs = [spent(lambda ps=ps: same_amd.sliding_window_incumbent(ref, mov, optim_params={**OP, **ps}, **kw)) for ps in SETS]
    sweep = spent(lambda: same_amd.sliding_window_sweep(ref, mov, SETS, optim_params=dict(OP), **kw))
    one = jobs[1]
    assert one["stage"] >= 2 and one["tickets"] >= 6 and one["prefix"] == 0
    assert all(j["stage"] == one["stage"] and j["tickets"] == one["tickets"] for j in jobs)
    assert sweep["stage"] == one["stage"] and sweep["tickets"] == one["tickets"]
    assert sweep["finish"] == sum(j["finish"] for j in jobs) == len(SETS) * one["finish"]
    assert sweep["prefix"] == 2 * one["stage"]              # knn 8 is the list as staged; 4 and 2: one call each per batch
