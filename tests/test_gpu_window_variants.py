"""same_window_recost (csrc/window_recost.hip) at the LIBRARY and same_amd.sliding_window_variants as a product.
Library: a staged window priced again from a types layer is, array by array and bit by bit, the window a stage call over a moving section
MADE with the layer's matrix leaves -- on the input families of tests/variant_check.py, which tests/test_window_variants_cpu.py proves
(without a GPU) to hold the shapes the kernel can go wrong at, and against that file's host statement.  Layering: the prefix, the priority
prune, the caller calls and the finish calls on a recost window are those on the fresh one.  Product: every table and stats list of a
variants pass is the stand-alone job's on a moving frame the test builds itself, exactly; and the pass stages and triangulates what ONE
job does."""
import functools

import numpy as np
import pandas as pd
import pytest

import caller_check as C
import knn_prefix_check as K
import variant_check as V

pytestmark = pytest.mark.gpu


def _W():
    from same_amd import windows as W

    return W


def _fetch(st):
    W = _W()
    what = dict(rows=W._W_ALIGNED_ROWS, xy=W._W_ALIGNED_XY, rows_m=W._W_ROWS_M, rows_r=W._W_ROWS_R, kept=W._W_KEPT, pairs=W._W_PAIRS,
                costs=W._W_COSTS, staged=W._W_STAGED_PAIRS)
    return {k: st.fetch(w) for k, w in what.items()}


def _same_arrays(a, b, tag):
    bits = lambda v: v.view(np.int64) if v.dtype == np.float64 else v
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (tag, k)
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)


def _case_of(tag):
    """the sections' key of a family: its case, not its box"""
    head = tag.split("/")
    return head[0] if head[0].startswith("T") else ("K/edge/" + head[2] if head[1] == "edge" else "K/" + head[1])


@functools.lru_cache(maxsize=None)
def _uploaded(key, dtype):
    """of one case and cost type, uploaded once: the moving and the reference section, the two variants as layers of the moving section
    and as moving sections of their own (the fresh windows' source), label codes set where the case has them"""
    W = _W()
    if key.startswith("T"):
        case = V.t_case(int(key[1:]))
    else:
        name = key.split("/")[1]
        case = {"base": C.base_case, "tie": C.tie_case, "contention": C.contention_case}[name]() if name != "edge" else C.edge_case(int(key.split("/")[2]))
    codes = C.base_codes() if key == "K/base" else case
    l1, l2 = V.variants_of(case["types_m"], 5)

    def moving(types):
        d = W.DeviceSection(W.Section(case["mov_xy"], types, case.get("type_id"), case.get("size")), dtype)
        if "code_m" in codes:
            d.set_label_codes(codes["code_m"])
        return d

    dmov, dref = moving(case["types_m"]), W.DeviceSection(W.Section(case["ref_xy"], case["types_r"], None, None), dtype)
    if "code_r" in codes:
        dref.set_label_codes(codes["code_r"])
    return dict(case=case, dmov=dmov, dref=dref, types={None: case["types_m"], "L1": l1, "L2": l2},
                layer={None: None, "L1": W.DeviceTypesLayer(dmov, l1), "L2": W.DeviceTypesLayer(dmov, l2)},
                made={None: dmov, "L1": moving(l1), "L2": moving(l2)})


# ---- 1. the library, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", V.tags())
def test_recost_leaves_the_window_a_stage_call_over_the_variant_leaves(oracle, tag, dtype):
    """fails without the feature: the library has no same_window_recost"""
    W = _W()
    _tag, case, box, radius, k = V.family(oracle, tag)
    up = _uploaded(_case_of(tag), dtype)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        counts0 = st.stage(up["dmov"], up["dref"], box, radius, k, 1.0)
        staged0 = _fetch(st)
        rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, radius, k, oracle)
        assert np.array_equal(staged0["rows"], rows) and np.array_equal(staged0["pairs"], pairs)      # the list the CPU test reasoned about
        seen = {}
        for name in ("L1", "L2", None, "L1", None):                       # L1, L2, back to the section's own, and once more
            got = W.recost_windows([st], up["dmov"], up["dref"], up["layer"][name], 1.0)[0]
            want = fresh.stage(up["made"][name], up["dref"], box, radius, k, 1.0)
            assert got == want == counts0 and st.counts == fresh.counts and st.n_staged_pairs == fresh.n_staged_pairs, (tag, name, got, want)
            now = _fetch(st)
            _same_arrays(now, _fetch(fresh), (tag, name))
            if name is None:
                _same_arrays(now, staged0, (tag, "back"))
            # ... and the host statement's
            host = V.recost(case["mov_xy"], case["ref_xy"], up["types"][name], case["types_r"], rows, rows_r, pairs, 1.0, dtype, oracle)
            assert np.array_equal(now["costs"].view(np.int64), host.view(np.int64)), (tag, name)
            seen[name] = now["costs"]
        if len(pairs):
            assert (seen["L1"] != seen["L2"]).any() and (seen["L1"] != seen[None]).any()
    finally:
        st.close()
        fresh.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_recost_of_a_batch_of_more_windows_than_a_launch_takes(oracle, dtype):
    """ONE call over 23 windows of very different sizes, among them windows whose box holds rows and no pair and windows whose box holds
    nothing: every window is the one a batch staged over the variant leaves, its counts at its own index"""
    W = _W()
    up = _uploaded("K/base", dtype)
    kinds = C.priority_boxes()
    boxes = [b for _k, b in kinds]
    states, fresh = [W.DeviceWindow() for _ in boxes], [W.DeviceWindow() for _ in boxes]
    try:
        first = W.stage_windows(states, up["dmov"], up["dref"], boxes, C.RADIUS, K.BASE_K, 1.0)
        for name in ("L2", "L1", None):
            got = W.recost_windows(states, up["dmov"], up["dref"], up["layer"][name], 1.0)
            want = W.stage_windows(fresh, up["made"][name], up["dref"], boxes, C.RADIUS, K.BASE_K, 1.0)
            assert got == want == first, name
            for q, (kind, _box) in enumerate(kinds):
                _same_arrays(_fetch(states[q]), _fetch(fresh[q]), (name, q, kind))
                assert (got[q][3] == 0) == (kind != "pairs")
        assert sum(1 for c in got if c[3] >= V.LDS_MIN_PAIRS) >= 2 and sum(1 for c in got if 0 < c[3] < V.LDS_MIN_PAIRS) >= 2
    finally:
        for st in states + fresh:
            st.close()


def test_recost_refuses_what_it_cannot_price(oracle):
    from same_amd import _lib

    W = _W()
    up, other = _uploaded("K/base", "float64"), _uploaded("T4", "float64")
    box = C.base_boxes(oracle)["interior"]
    st, unstaged = W.DeviceWindow(), W.DeviceWindow()
    try:
        st.stage(up["dmov"], up["dref"], box, C.RADIUS, 6, 1.0)
        before = _fetch(st)
        for states, dmov, dref, layer in (([unstaged], up["dmov"], up["dref"], None),                # not staged
                                          ([st], other["dmov"], up["dref"], None),                    # other sections than staged from
                                          ([st], up["dmov"], other["dref"], None),
                                          ([st], up["dmov"], up["dref"], other["layer"]["L1"]),       # a layer of another section
                                          ([st, unstaged], up["dmov"], up["dref"], up["layer"]["L1"])):
            with pytest.raises(_lib.SameHipError) as e:
                W.recost_windows(states, dmov, dref, layer, 1.0)
            assert e.value.code == _lib.SAME_EINVAL
            _same_arrays(_fetch(st), before, "refused")
        with pytest.raises(ValueError):                                                               # a matrix of another shape
            W.DeviceTypesLayer(up["dmov"], up["types"]["L1"][:, :-1])
    finally:
        st.close()
        unstaged.close()


# ---- 2. layering -----------------------------------------------------------------------------------------------------------------------
def _filter_args(radius, angle, same):
    from same_amd.triangles import cos_threshold

    en, thr = cos_threshold(angle)
    tol = float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0
    return (radius, en, thr, tol, same)


def _finish(st, radius, same, penalty, mode, from_caller=False):
    """the finish call over scipy's simplices of the window's kept cells (or the caller's triangles the window holds) -> what it leaves"""
    from scipy.spatial import Delaunay

    W = _W()
    tris = None if from_caller else [Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices.astype(np.int32)]
    kept, added, near, row, flag, stats = W.filter_finish_windows([st], tris, *_filter_args(radius, 15, same), penalty, mode=mode,
                                                                  from_caller=from_caller)[0]
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


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", ["K/base/interior", "K/tie"])
def test_prefix_and_priority_prune_on_a_recost_window_are_those_on_the_fresh_one(oracle, tag, dtype):
    W = _W()
    _tag, _case, box, radius, k_max = V.family(oracle, tag)
    up = _uploaded(_case_of(tag), dtype)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        st.stage(up["dmov"], up["dref"], box, radius, k_max, 1.0)
        W.priority_windows([st])                             # a prune and a cut of the staged list first: the recost must forget both
        W.prefix_windows([st], 2)
        W.recost_windows([st], up["dmov"], up["dref"], up["layer"]["L1"], 1.0)
        for k in (3, 1, k_max):                              # smaller k, and back
            got = W.prefix_windows([st], k)[0]
            assert got == fresh.stage(up["made"]["L1"], up["dref"], box, radius, k, 1.0), k
            _same_arrays(_fetch(st), _fetch(fresh), (tag, k))
            got, want = W.priority_windows([st])[0], W.priority_windows([fresh])[0]
            assert got == want and st.counts == fresh.counts and got[1] <= got[0] and (k == 1 or got[1] < got[0]), (k, got, want)
            _same_arrays(_fetch(st), _fetch(fresh), (tag, k, "pruned"))
        # a recost of the pruned window: the prune is gone, the list is the staged one under the other variant
        got = W.recost_windows([st], up["dmov"], up["dref"], up["layer"]["L2"], 1.0)[0]
        assert got == fresh.stage(up["made"]["L2"], up["dref"], box, radius, k_max, 1.0) and st.priority is None
        _same_arrays(_fetch(st), _fetch(fresh), (tag, "L2"))
    finally:
        st.close()
        fresh.close()


@pytest.mark.parametrize("name", ["greedy", "assignment + local", "transport + capacity"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_finish_on_a_recost_window_is_the_finish_on_the_fresh_window(oracle, name, dtype):
    W = _W()
    mode = _modes()[name]
    _tag, _case, box, radius, k_max = V.family(oracle, "K/base/interior")
    up = _uploaded("K/base", dtype)
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    try:
        st.stage(up["dmov"], up["dref"], box, radius, k_max, 1.0)
        first = _finish(st, radius, True, 50.0, mode)        # a finish of the staged list first: the recost starts over
        records = {}
        for variant in ("L1", "L2"):
            W.recost_windows([st], up["dmov"], up["dref"], up["layer"][variant], 1.0)
            fresh.stage(up["made"][variant], up["dref"], box, radius, k_max, 1.0)
            a, b = _finish(st, radius, True, 50.0, mode), _finish(fresh, radius, True, 50.0, mode)
            _same_record(a, b, (name, variant))
            assert a["stats"]["matched"] > 100
            records[variant] = a
        assert not np.array_equal(records["L1"]["match"], records["L2"]["match"]) and not np.array_equal(records["L1"]["match"], first["match"])
        W.recost_windows([st], up["dmov"], up["dref"], None, 1.0)
        _same_record(_finish(st, radius, True, 50.0, mode), first, (name, "back"))
    finally:
        st.close()
        fresh.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_caller_calls_on_a_recost_window_are_those_on_the_fresh_window(oracle, dtype):
    """both orders: caller's triangles AFTER the recost (then a cut and caller_pairs), and a recost of a window the caller's triangles
    have compacted (turned back and held: caller_pairs alone puts the priced list through the mask)"""
    W = _W()
    _tag, case, box, radius, k_max = V.family(oracle, "K/base/interior")
    up = _uploaded("K/base", dtype)
    filt = _filter_args(radius, 15, True)
    callers = {name: W.DeviceCallerTris(up["made"][name], case["tris"]) for name in (None, "L1")}
    st, fresh = W.DeviceWindow(), W.DeviceWindow()
    mode = _modes()["assignment + local"]

    def fresh_at(k):
        fresh.stage(up["made"]["L1"], up["dref"], box, radius, k, 1.0)
        return W.caller_tris_windows([fresh], callers["L1"], *filt)[0]

    try:
        st.stage(up["dmov"], up["dref"], box, radius, k_max, 1.0)
        W.recost_windows([st], up["dmov"], up["dref"], up["layer"]["L1"], 1.0)
        got = W.caller_tris_windows([st], callers[None], *filt)[0]
        assert got == fresh_at(k_max) and got[2] == 0 and got[0] > 0 and st.counts == fresh.counts
        _same_arrays(_fetch(st), _fetch(fresh), "caller after recost")
        W.prefix_windows([st], 3)
        assert W.caller_pairs_windows([st])[0] == fresh_at(3) and st.counts == fresh.counts
        _same_arrays(_fetch(st), _fetch(fresh), "cut after recost")
        _same_record(_finish(st, radius, True, 50.0, mode, from_caller=True), _finish(fresh, radius, True, 50.0, mode, from_caller=True), "cut")
        # the compacted window priced again: under L2 (nothing to compare but the counts), then under L1 against the fresh one
        for name in ("L2", "L1"):
            staged = W.recost_windows([st], up["dmov"], up["dref"], up["layer"][name], 1.0)[0]
            assert staged[3] >= got[4] and staged[2] >= got[3]  # the staged list again, rows of removed nodes included
            assert W.caller_pairs_windows([st])[0] == got
        assert fresh_at(k_max) == got and st.counts == fresh.counts
        _same_arrays(_fetch(st), _fetch(fresh), "recost of a compacted window")
        _same_record(_finish(st, radius, True, 50.0, mode, from_caller=True), _finish(fresh, radius, True, 50.0, mode, from_caller=True), "held")
    finally:
        st.close()
        fresh.close()
        for c in callers.values():
            c.close()


# ---- 3. what one recost call asks of the runtime ------------------------------------------------------------------------------------------
# (launches, fills, copies, waits) of ONE recost call over the nine boxes of tests/test_gpu_window_call_counts.py -- one launch group of
# the 8 windows that have pairs: the kernel and the group's hand-back -- as observed with this very test body on an MI355X on the commit
# that added the call (the one after 2aae868)
RECOST_CALLS = (2, 0, 0, 1)


def test_one_recost_call_has_one_wait_and_no_copy(oracle):
    from test_gpu_window_call_counts import BOXES

    W = _W()
    case = C.base_case()
    dmov = W.DeviceSection(W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"]), np.float64)
    dref = W.DeviceSection(W.Section(case["ref_xy"], case["types_r"], None, None), np.float64)
    dmov.bin(*C.GRIDS["cell 25"])
    dref.bin(*C.GRIDS["cell 25"])
    layer = W.DeviceTypesLayer(dmov, V.variants_of(case["types_m"], 5)[0])
    states = [W.DeviceWindow() for _ in BOXES]
    ctx = states[0].ctx
    try:
        staged = W.stage_windows(states, dmov, dref, BOXES, C.RADIUS, C.KNN, 1.0)
        assert [c[3] > 0 for c in staged] == [b != C.EMPTY_BOX for b in BOXES]
        seen = []
        for lay in (layer, None):
            before = ctx.stats()
            assert W.recost_windows(states, dmov, dref, lay, 1.0) == staged
            after = ctx.stats()
            seen.append(tuple(after[w] - before[w] for w in ("launches", "fills", "copies", "waits")))
    finally:
        for s in states:
            s.close()
        layer.close()
        dmov.close()
        dref.close()
    print("observed:", seen)
    assert seen == [RECOST_CALLS, RECOST_CALLS]
    assert seen[0][3] == 1 and seen[0][1] == 0 and seen[0][2] == 0


# ---- 4. the product ----------------------------------------------------------------------------------------------------------------------
WIN = dict(window_size=300, overlap=75, min_cells_per_window=20)
OP = dict(radius=30, knn=8, **WIN)
SETS = [{"knn": 4, "hip_incumbent": "assignment", "hip_refine": "local"}, {}, {"knn": 4}, {"hip_incumbent": "transport", "hip_refine": "capacity",
                                                                                        "max_matches": 2, "penalty_coeff": 0.5}]


@functools.lru_cache(maxsize=None)
def _frames(n=4000, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1)), tuple(synth.type_columns(6))


def _variants_of(frame, cols, seed=11):
    """None, a noised matrix (an array), a column permutation of the frame's own (a DataFrame under an index of its own)"""
    own = frame[list(cols)].to_numpy(dtype=np.float64)
    rng = np.random.default_rng(seed)
    noised = np.abs(own + 0.35 * rng.standard_normal(own.shape))
    noised /= np.maximum(noised.sum(axis=1, keepdims=True), 1e-12)
    permuted = pd.DataFrame(np.roll(own, 1, axis=1), columns=list(cols), index=np.arange(len(frame))[::-1])
    return [None, noised, permuted]


def _moving_v(moving, cols, variant):
    """the test's own moving_v: a copy of the frame (of the object, for a MetaCell) with the commonCT columns assigned"""
    import copy

    if variant is None:
        return moving
    m = np.asarray(variant[list(cols)] if isinstance(variant, pd.DataFrame) else variant, dtype=np.float64)
    frame = (moving.metacell_df if hasattr(moving, "metacell_df") else moving).copy()
    for t, c in enumerate(cols):
        frame[c] = m[:, t]
    if not hasattr(moving, "metacell_df"):
        return frame
    out = copy.copy(moving)
    out.metacell_df = frame
    return out


def _variants_equal_the_jobs(ref, mov, cols, op, tag, sets=None, variants=None, ref_alone=None, **kw):
    import same_amd

    frame = mov.metacell_df if hasattr(mov, "metacell_df") else mov
    variants = _variants_of(frame, cols) if variants is None else variants
    got = same_amd.sliding_window_variants(ref, mov, variants, commonCT=list(cols), param_sets=sets, optim_params=dict(op), return_stats=True, **kw)
    assert len(got) == len(variants)
    ref_alone = ref if ref_alone is None else ref_alone
    for v, variant in enumerate(variants):
        mov_v = _moving_v(mov, cols, variant)
        for q, ps in enumerate([{}] if sets is None else sets):
            want, wst = same_amd.sliding_window_incumbent(ref_alone, mov_v, commonCT=list(cols), optim_params={**op, **ps}, return_stats=True, **kw)
            table, st = got[v] if sets is None else got[v][q]
            pd.testing.assert_frame_equal(table, want, check_exact=True, obj=f"{tag} variant {v} set {q}")
            assert [list(s) for s in st] == [list(s) for s in wst] and st == wst, (tag, v, q)
    tables = [g[0] if sets is None else g[0][0] for g in got]
    for a in range(len(tables)):                              # not vacuous: every two variants differ in a table row
        for b in range(a + 1, len(tables)):
            assert len(tables[a]) > 100 and not tables[a].equals(tables[b]), (tag, a, b)
    return got


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
@pytest.mark.parametrize("route", [None, "native", "device"])
def test_variant_tables_and_stats_are_the_stand_alone_jobs(route, merge):
    """fails without the feature: same_amd has no sliding_window_variants"""
    import same_amd

    ref, mov, cols = _frames()
    op = dict(OP) if route is None else dict(OP, hip_delaunay=route)
    n_windows = len(same_amd.window_plan(ref[["X", "Y"]].to_numpy(), mov[["X", "Y"]].to_numpy(), WIN["window_size"], WIN["overlap"],
                                         WIN["min_cells_per_window"]))
    batch = next(b for b in (4, 3, 5) if n_windows % b)                                             # a partial last batch
    got = _variants_equal_the_jobs(ref, mov, cols, op, (route, merge), merge=merge, batch=batch, workers=1)
    st0 = got[0][1]
    assert 6 <= len(st0) <= 12 and len(st0) == n_windows and min(s["pairs"] for s in st0) > 2000
    assert [s["pairs"] for s in got[1][1]] == [s["pairs"] for s in st0]                           # the pair lists are geometry
    assert [s["matched"] for s in got[1][1]] != [s["matched"] for s in st0] or not got[1][0].equals(got[0][0])


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
def test_variants_in_float_costs(merge):
    ref, mov, cols = _frames()
    _variants_equal_the_jobs(ref, mov, cols, dict(OP, hip_cost_dtype="float32"), ("float32", merge), merge=merge)


def test_variants_under_param_sets_with_window_local_indices_and_two_workers():
    ref, mov, cols = _frames()
    got = _variants_equal_the_jobs(ref, mov, cols, OP, "sets", sets=SETS, window_local_indices=True, workers=2, batch=3)
    assert all("ref_idx" in t.columns for per_set in got for t, _s in per_set)
    assert all(a["pairs"] < b["pairs"] for a, b in zip(got[1][2][1], got[1][1][1]))                 # knn 4 against knn 8, within a variant


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
def test_variants_with_the_priority_prune_on_the_device(merge):
    ref, mov, cols = _frames()
    op = dict(OP, ignore_knn_if_matched=True, hip_priority_prune="device")
    got = _variants_equal_the_jobs(ref, mov, cols, op, "priority", sets=SETS[1:3], merge=merge)
    for per_set in got:
        for _t, st in per_set:
            assert all(s["pairs_staged"] > s["pairs"] and s["priority_rows"] > 0 for s in st)


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merged"])
@pytest.mark.parametrize("kind", ["ms3", "aligned_only"])
def test_variants_over_metacell_objects_on_the_device_route(kind, merge):
    from test_gpu_caller_triangulation import _metacells

    ref, mc, cols = _metacells(kind)
    op = dict(radius=30, knn=6, window_size=200, overlap=50, min_cells_per_window=20, hip_caller_delaunay="device")
    got = _variants_equal_the_jobs(ref, mc, cols, op, (kind, merge), sets=[{}, {"knn": 3, "hip_incumbent": "assignment"}], merge=merge)
    assert len(got[0][0][1]) >= 9


def test_variants_over_resident_frames_upload_a_variant_once():
    import same_amd

    ref, mov, cols = _frames()
    variants = _variants_of(mov, cols)
    with same_amd.resident_frames(ref, mov) as frames:
        _variants_equal_the_jobs(frames, mov, cols, OP, "resident", variants=variants, ref_alone=ref)
        held = [f._types_layers for f in frames._frames.values()]
        assert len(held) == 1 and len(held[0]) == 2
        layers = [layer for _v, layer in held[0].values()]
        same_amd.sliding_window_variants(frames, mov, variants[::-1], commonCT=list(cols), optim_params=dict(OP))
        assert [layer for _v, layer in held[0].values()] == layers and all(layer.handle for layer in layers)
    assert all(layer.handle is None for layer in layers)                                            # closed with the frames


@pytest.mark.parametrize("why", ["host prune", "caller on the host"])
def test_inputs_the_device_route_refuses_give_the_same_results_variant_by_variant(monkeypatch, why):
    W = _W()
    monkeypatch.setattr(W, "recost_windows", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the shared pass ran")))
    if why == "host prune":
        ref, mov, cols = _frames(1500, 3)
        _variants_equal_the_jobs(ref, mov, cols, dict(OP, ignore_knn_if_matched=True), why, sets=[{}, {"knn": 4}])
    else:
        from test_gpu_caller_triangulation import _metacells

        ref, mc, cols = _metacells("ms3")
        _variants_equal_the_jobs(ref, mc, cols, dict(radius=30, knn=6, window_size=200, overlap=50, min_cells_per_window=20), why)


# ---- 5. the sharing is real ------------------------------------------------------------------------------------------------------------
def test_a_variants_pass_stages_and_triangulates_what_one_job_does(monkeypatch):
    """The binding's stage calls and the tickets asked of the triangulator over a pass of three variants x two knn values against ONE
    job's; its finish calls against the jobs' sum; its recost calls against batches x the variants that are not None."""
    import same_amd
    from same_amd import delaunay

    W = _W()
    seen = {"stage": 0, "prefix": 0, "finish": 0, "recost": 0, "tickets": 0}

    def counting(name, key):
        inner = getattr(W, name)

        def call(*a, **k):
            seen[key] += 1
            return inner(*a, **k)

        monkeypatch.setattr(W, name, call)

    counting("stage_windows", "stage")
    counting("prefix_windows", "prefix")
    counting("recost_windows", "recost")
    counting("filter_finish_windows", "finish")

    class Counting(delaunay.QhullTriangulator):
        def submit(self, points, key=None):
            seen["tickets"] += 1
            return super().submit(points, key)

    ref, mov, cols = _frames()
    variants, sets = _variants_of(mov, cols), [{}, {"knn": 4}]
    kw = dict(commonCT=list(cols), workers=1, batch=4, triangulator=Counting())

    def spent(run):
        for k in seen:
            seen[k] = 0
        run()
        return dict(seen)

    one = spent(lambda: same_amd.sliding_window_incumbent(ref, mov, optim_params=dict(OP), **kw))
    shared = spent(lambda: same_amd.sliding_window_variants(ref, mov, variants, param_sets=sets, optim_params=dict(OP), **kw))
    batches = one["stage"]
    assert batches >= 2 and one["tickets"] >= 6 and one["prefix"] == one["recost"] == 0
    assert shared["stage"] == batches and shared["tickets"] == one["tickets"]
    assert shared["recost"] == batches * 2                      # at most batches x (variants that are not None): here every batch has pairs
    assert shared["finish"] == len(variants) * len(sets) * one["finish"]
    assert shared["prefix"] == batches * len(variants)          # per batch and variant: knn 8 is the list as staged / priced, 4 one cut
    only_none = spent(lambda: same_amd.sliding_window_variants(ref, mov, [None, None], optim_params=dict(OP), **kw))
    assert only_none["recost"] == 0 and only_none["stage"] == batches and only_none["tickets"] == one["tickets"]
