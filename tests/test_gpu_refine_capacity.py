"""The local search within the model's reference capacities on the device (optim_params["hip_refine"] = "capacity", csrc/refine.hip).
The oracle is the host statement (tests/refine_capacity_check.py): the same matching, rounds and moves; with every limit 1 it is
hip_refine="local" bit for bit."""
import numpy as np
import pytest

import refine_capacity_check as rcc
import refine_check as rc

pytestmark = pytest.mark.gpu


def _device(kw, start, cap=32, limit=None, pc=None):
    from same_amd import ops

    limit = kw["limit"] if limit is None else limit
    pc = kw["penalty_coeff"] if pc is None else pc
    return ops.refine_matching_cap(kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"], kw["triangles"], kw["axy"],
                                   kw["ref_xy"], kw["size"], kw["delaunay_penalty"], limit, pc, cap, start)


FAMILIES = [(kind, seed, pc, {}) for kind in ("uniform", "clustered", "lattice") for seed, pc in ((0, 0.0), (1, 1.0), (2, 100.0))] + [
    ("uniform", 10, 1.0, dict(equal_costs=True)), ("clustered", 12, 0.0, dict(equal_costs=True)),
    ("uniform", 13, 1.0, dict(delaunay_penalty=0.0)), ("lattice", 14, 100.0, dict(delaunay_penalty=0.0)),
    ("clustered", 15, 0.5, dict(no_match_penalty=40.0)),
]


@pytest.mark.parametrize("kind, seed, pc, extra", FAMILIES)
def test_host_form_equals_the_host_statement(kind, seed, pc, extra):
    kw, start = rcc.make_cap_problem(kind, 300, seed=seed, penalty_coeff=pc, **extra)
    want, wst = rcc.refine(rcc.CapProblem(**kw), start, 32)
    got, st = _device(kw, start)
    assert np.array_equal(got, want)
    assert (st["rounds"], st["moves"], st["settled"], st["ref_extra_matches"]) == \
           (wst["rounds"], wst["moves"], wst["settled"], wst["ref_extra_matches"])
    assert st["objective_start"] == pytest.approx(wst["objective_start"], rel=1e-12)
    assert st["objective"] == pytest.approx(wst["objective"], rel=1e-12)
    again, st2 = _device(kw, start)
    assert np.array_equal(again, got) and st2 == st


def test_host_form_uses_capacity_and_round_caps_match():
    kw, start = rcc.make_cap_problem("clustered", 300, seed=21, penalty_coeff=0.5, no_match_penalty=40.0)
    _m, full = rcc.refine(rcc.CapProblem(**kw), start, 32)
    assert full["ref_extra_matches"] > 0
    for cap in (1, 2, 3):
        want, wst = rcc.refine(rcc.CapProblem(**kw), start, cap)
        got, st = _device(kw, start, cap)
        assert np.array_equal(got, want)
        assert (st["rounds"], st["moves"], st["settled"]) == (wst["rounds"], wst["moves"], wst["settled"])


@pytest.mark.parametrize("kind, seed", [("uniform", 0), ("clustered", 1), ("lattice", 2), ("uniform", 3)])
def test_every_limit_one_is_the_local_search_bit_for_bit(kind, seed):
    from same_amd import ops

    kw, start = rc.make_problem(kind, 400, seed=seed)
    for cap in (1, 2, 32):
        want, wst = ops.refine_matching(kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"], kw["triangles"], kw["axy"],
                                        kw["ref_xy"], kw["size"], kw["delaunay_penalty"], cap, start)
        for pc in (0.0, 100.0):
            got, st = _device(kw, start, cap, limit=np.ones(kw["n_r"], np.int32), pc=pc)
            assert np.array_equal(got, want)
            assert st.pop("ref_extra_matches") == 0
            assert st == wst            # objectives compared as floats: the same bits


# ---- the window path
def _section(seed=60, meta=True, n=6000):
    from same_amd import synth

    cells = synth.make_cells(n, 5, seed=seed)
    r_df = synth.to_frame(cells).iloc[::2].reset_index(drop=True)       # half the cells as references: they are contended
    m_df = synth.to_frame(synth.make_jittered(cells, seed=seed + 1))
    if meta:
        r_df["size"] = np.random.default_rng(seed).integers(1, 5, len(r_df)).astype(np.float64)
    op = dict(radius=30, knn=6, min_angle_deg=12, dist_ct_coeff=1.5, window_size=900, overlap=200, no_match_penalty=100.0,
              penalty_coeff=1.0, min_cells_per_window=10)
    return r_df, m_df, synth.type_columns(5), op


def _same(got, want, what):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), what
    for c in want.columns:
        assert np.array_equal(got[c].to_numpy(), want[c].to_numpy()), (what, c)


@pytest.mark.parametrize("tri", [None, "native"])
def test_sliding_window_capacity_with_every_limit_one_is_local(tri):
    import same_amd

    r_df, m_df, cols, op = _section(seed=70, meta=False)
    op = dict(op, max_matches=1)
    if tri:
        op["hip_delaunay"] = tri
    run = lambda o: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True)
    want, wst = run(dict(op, hip_refine="local"))
    got, st = run(dict(op, hip_refine="capacity"))
    _same(got, want, tri)
    assert len(st) == len(wst) > 3
    for a, b in zip(st, wst):
        assert a.pop("ref_extra_matches") == 0
        assert a == b


def _window_checks(r_df, m_df, cols, op):
    """per window of the device route: counts within the model's limits, the objective never up, the reported objective = the model's
    formula on the window's own arrays, the final matching = the host statement from the window's start -> windows holding a reference
    more than once"""
    from same_amd import windows as W
    from same_amd.api import ref_match_limits
    from same_amd.window_api import _WindowJob
    from same_amd.window_mode import WindowMode

    import pandas as pd

    mode = WindowMode.from_params(op)
    job = _WindowJob(r_df, m_df, cols, None, None, None, op, None, False, None)
    frames, own = job.device_frames(None)
    plan = [w for _p, w in job.todo]
    try:
        starts = {}
        for w, dw in zip(plan, frames.windows(plan, batch=1)):
            if dw.error is None:
                starts[id(w)] = dw.state.fetch(W._W_MATCH).copy()
        multi = 0
        n_win = 0
        for w, dw in zip(plan, frames.windows(plan, batch=1, mode=mode)):
            if dw.error is not None:
                continue
            st = dw.state
            pairs, costs = st.fetch(W._W_PAIRS), st.fetch(W._W_COSTS)
            rows_r, match = st.fetch(W._W_ROWS_R), st.fetch(W._W_MATCH)
            tris = st.fetch(W._W_TRIANGLES)
            n, n_r = len(dw.rows_m), len(rows_r)
            size = np.asarray(m_df["size"].to_numpy(dtype=np.float64) if "size" in m_df.columns else np.ones(len(m_df)))[dw.rows_m]
            axy = np.asarray(m_df[["X", "Y"]].to_numpy(dtype=np.float64))[dw.rows_m]
            rxy = np.asarray(r_df[["X", "Y"]].to_numpy(dtype=np.float64))[rows_r]
            # the model's frame: the references the pairs name, ascending (the post-KNN ref_df)
            used = np.unique(pairs[:, 1])
            frame = pd.DataFrame({"size": r_df["size"].to_numpy()[rows_r[used]]}) if "size" in r_df.columns else pd.DataFrame(index=used)
            lim = np.ones(n_r, np.int32)
            lim[used] = np.minimum(ref_match_limits(frame, op.get("max_matches", 1), op.get("ref_metacell_match_multiplier")), 1001)
            cnt = np.bincount(match[match >= 0], minlength=n_r)
            assert np.all(cnt <= lim)
            rec = dw.refine
            assert rec["objective"] <= rec["objective_start"]
            assert rec["ref_extra_matches"] == int(np.maximum(cnt - 1, 0).sum())
            pair_of = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs)}
            mp = np.array([pair_of[(i, int(match[i]))] if match[i] >= 0 else -1 for i in range(n)], np.int32)
            obj, extra = rcc.model_objective(pairs, costs, n, tris, axy, rxy, size, mp, op["no_match_penalty"], op["delaunay_penalty"],
                                             op["penalty_coeff"])
            assert extra == rec["ref_extra_matches"]
            assert rec["objective"] == pytest.approx(obj, rel=1e-9)
            s0 = starts[id(w)]
            start = np.array([pair_of[(i, int(s0[i]))] if s0[i] >= 0 else -1 for i in range(n)], np.int32)
            prob = rcc.CapProblem(pairs, costs, op["no_match_penalty"] * size, n, n_r, tris, axy, rxy, size, op["delaunay_penalty"],
                                  limit=lim, penalty_coeff=op["penalty_coeff"])
            want, wst = rcc.refine(prob, start, mode.rounds)
            assert np.array_equal(want, mp), w
            assert (wst["rounds"], wst["moves"], wst["settled"]) == (rec["rounds"], rec["moves"], rec["settled"])
            multi += int(cnt.max(initial=0) > 1)
            n_win += 1
    finally:
        if own:
            frames.close()
    assert n_win > 3
    return multi


@pytest.mark.parametrize("variant", ["metacells", "max_matches_2"])
def test_window_capacity_is_used_and_respected(variant):
    if variant == "metacells":
        r_df, m_df, cols, op = _section(seed=80, meta=True)
        op = dict(op, ref_metacell_match_multiplier=3, hip_refine="capacity", delaunay_penalty=5.0)
    else:
        r_df, m_df, cols, op = _section(seed=81, meta=False)
        op = dict(op, max_matches=2, hip_refine="capacity", delaunay_penalty=5.0)
    multi = _window_checks(r_df, m_df, cols, op)
    assert multi > 0, "the fixture must make some window hold a reference more than once"


def test_capacity_routes_agree_and_merge():
    import same_amd
    from same_amd.merge import merge_window_matches_unique_ref

    r_df, m_df, cols, op = _section(seed=90, meta=True)
    op = dict(op, ref_metacell_match_multiplier=3, hip_refine="capacity")
    run = lambda o, **k: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True, **k)
    want, stats = run(op, _route="device")
    assert sum(s["ref_extra_matches"] for s in stats) > 0
    for kw in (dict(_route="general", _pipeline="device"), dict(_route="general", _pipeline="frames")):
        got, st = run(op, **kw)
        _same(got, want, kw)
        for a, b in zip(st, stats):
            for k in ("flipped", "matched", "refine_rounds", "refine_moves", "refine_settled", "ref_extra_matches"):
                assert a[k] == b[k], (kw, k)
            assert a["mip_objective"] == pytest.approx(b["mip_objective"], rel=1e-9)
    merged = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op), merge=True)
    plain = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op))
    want_merged = merge_window_matches_unique_ref([plain])
    assert list(merged.columns) == list(want_merged.columns) and merged.equals(want_merged)


def test_assignment_start_with_capacity_and_refinish():
    import same_amd
    from same_amd import windows as W
    from same_amd.window_api import _WindowJob
    from same_amd.window_mode import WindowMode

    r_df, m_df, cols, op = _section(seed=100, meta=True)
    op = dict(op, ref_metacell_match_multiplier=3, hip_refine="capacity", hip_incumbent="assignment")
    table, st = same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(op), return_stats=True)
    assert len(table) and len(st) > 3
    assert all(s["mip_objective"] <= s["mip_objective_start"] for s in st)
    assert sum(s["ref_extra_matches"] for s in st) > 0
    # a window sent through same_window_refinish_cap from its assignment gives what the finish call gave
    mode = WindowMode.from_params(op)
    job = _WindowJob(r_df, m_df, cols, None, None, None, op, None, False, None)
    frames, own = job.device_frames(None)
    try:
        plan = [w for _p, w in job.todo]
        for w, dw in zip(plan, frames.windows(plan, batch=1, mode=mode)):
            if dw.error is not None:
                continue
            first = dw.state.fetch(W._W_MATCH).copy()
            pairs = dw.state.fetch(W._W_PAIRS)
            rec = dict(dw.refine)
            # the search's own result as the start: nothing left to improve, the same matching and record
            pair_of = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs)}
            mp = np.array([pair_of[(i, int(first[i]))] if first[i] >= 0 else -1 for i in range(len(first))], np.int32)
            match_row, _flag, _stats = dw.state.refinish(mp, op["no_match_penalty"], mode)
            again = dw.state.refine
            assert np.array_equal(match_row, dw.match_row)
            assert again["moves"] == 0 and again["settled"] == 1
            assert again["ref_extra_matches"] == rec["ref_extra_matches"]
            assert again["objective"] == rec["objective"]
            break
    finally:
        if own:
            frames.close()


@pytest.mark.parametrize("op", [{"penalty_coeff": -1.0}, {"penalty_coeff": float("nan")}, {"ref_metacell_match_multiplier": 0},
                                {"max_matches": 0}])
def test_bad_capacity_arguments_raise(op):
    import same_amd

    r_df, m_df, cols, base = _section(seed=110, meta=True, n=800)
    with pytest.raises(ValueError):
        same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(base, hip_refine="capacity", **op))
