"""The local search on the lazy model's objective on the device (optim_params["hip_refine"] = "local", csrc/refine.hip).  The oracle is
the host statement of the round rule (tests/refine_check.py): the same matching, rounds and moves."""
import numpy as np
import pytest

import refine_check as rc

pytestmark = pytest.mark.gpu


def _device(kw, start, cap=32):
    from same_amd import ops

    return ops.refine_matching(kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"], kw["triangles"], kw["axy"], kw["ref_xy"],
                               kw["size"], kw["delaunay_penalty"], cap, start)


FAMILIES = [(kind, seed, {}) for kind in ("uniform", "clustered", "lattice") for seed in range(4)] + [
    ("uniform", 10, dict(equal_costs=True)), ("lattice", 11, dict(equal_costs=True)), ("clustered", 12, dict(equal_costs=True)),
    ("uniform", 13, dict(delaunay_penalty=0.0)), ("clustered", 14, dict(delaunay_penalty=0.0)),
    ("uniform", 15, dict(jitter=2.0, k=8)), ("lattice", 16, dict(jitter=0.05)),
]


@pytest.mark.parametrize("kind, seed, extra", FAMILIES)
def test_host_form_equals_the_host_statement(kind, seed, extra):
    kw, start = rc.make_problem(kind, 400, seed=seed, **extra)
    want, wst = rc.refine(rc.Problem(**kw), start, 32)
    got, st = _device(kw, start)
    assert np.array_equal(got, want)
    assert (st["rounds"], st["moves"], st["settled"]) == (wst["rounds"], wst["moves"], wst["settled"])
    assert st["objective_start"] == pytest.approx(wst["objective_start"], rel=1e-12)
    assert st["objective"] == pytest.approx(wst["objective"], rel=1e-12)
    again, st2 = _device(kw, start)
    assert np.array_equal(again, got) and st2 == st


def test_round_cap_and_tiny_caps_match_the_host_statement():
    kw, start = rc.make_problem("uniform", 400, seed=21)
    for cap in (1, 2, 3):
        want, wst = rc.refine(rc.Problem(**kw), start, cap)
        got, st = _device(kw, start, cap)
        assert np.array_equal(got, want) and (st["rounds"], st["moves"], st["settled"]) == (wst["rounds"], wst["moves"], wst["settled"])


def test_zero_penalty_from_the_assignment_makes_no_move():
    from same_amd import ops

    for seed in range(3):
        kw, _start = rc.make_problem("clustered", 500, seed=seed, delaunay_penalty=0.0)
        opt, ast = ops.sparse_assign(kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"])
        assert ast["fallback"] == 0
        got, st = _device(kw, opt)
        assert st["moves"] == 0 and st["rounds"] == 0 and st["settled"] == 1 and np.array_equal(got, opt)


def _section(seed=30):
    from same_amd import synth

    ref = synth.make_cells(30_000, 5, seed=seed)
    mov = synth.make_jittered(ref, seed=seed + 1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    m_df["size"] = np.where(np.arange(len(m_df)) % 3 == 0, 2, 1)
    op = dict(radius=30, knn=6, min_angle_deg=12, dist_ct_coeff=1.5, hip_cost_dtype="float32", window_size=700, overlap=200,
              no_match_penalty=0.006, min_cells_per_window=10)
    return r_df, m_df, synth.type_columns(5), op


REFINE_KEYS = ("mip_objective_start", "mip_objective", "refine_rounds", "refine_moves", "refine_settled")


def _same(got, want, what):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), what
    for c in want.columns:
        assert np.array_equal(got[c].to_numpy(), want[c].to_numpy()), (what, c)


@pytest.mark.parametrize("incumbent", ["greedy", "assignment"])
def test_window_tables_agree_over_routes_batches_workers_and_triangulators(incumbent):
    import same_amd

    r_df, m_df, cols, op = _section()
    R = dict(op, hip_incumbent=incumbent, hip_refine="local")
    run = lambda o, **k: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True, **k)
    want, stats = run(R, _route="device")
    assert len(stats) > 10 and all(set(REFINE_KEYS) <= set(s) for s in stats)
    for kw in (dict(_route="general", _pipeline="device"), dict(_route="general", _pipeline="frames")):
        got, st = run(R, **kw)
        _same(got, want, kw)
        for a, b in zip(st, stats):
            assert {k: a[k] for k in ("flipped", "matched", "refine_rounds", "refine_moves", "refine_settled")} == \
                   {k: b[k] for k in ("flipped", "matched", "refine_rounds", "refine_moves", "refine_settled")}, kw
            assert a["mip_objective"] == pytest.approx(b["mip_objective"], rel=1e-9)
            assert a["mip_objective_start"] == pytest.approx(b["mip_objective_start"], rel=1e-9)
    for kw in (dict(batch=1), dict(batch=3), dict(workers=1), dict(workers=2)):
        got, st = run(R, _route="device", **kw)
        assert got.equals(want) and st == stats, kw
    for tri in ("qhull", "native", "device"):
        got, st = run(dict(R, hip_delaunay=tri), _route="device")
        assert got.equals(want) and st == stats, tri


@pytest.mark.parametrize("incumbent", ["greedy", "assignment"])
def test_refinement_lowers_the_objective_and_the_flips(incumbent):
    import same_amd

    r_df, m_df, cols, op = _section(seed=40)
    op = dict(op, hip_incumbent=incumbent, no_match_penalty=0.05)
    run = lambda o: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True, _route="device")
    _base, bst = run(op)
    assert sum(s["flipped"] for s in bst) > 0, "the start must have flips for this test to say anything"
    _t, st = run(dict(op, hip_refine="local"))
    assert len(st) == len(bst)
    for s in st:
        assert s["mip_objective"] <= s["mip_objective_start"]
    assert sum(s["mip_objective"] for s in st) < sum(s["mip_objective_start"] for s in st)
    assert sum(s["flipped"] for s in st) < sum(s["flipped"] for s in bst)
    assert sum(s["refine_moves"] for s in st) > 0


def test_without_the_key_nothing_changes():
    import same_amd

    r_df, m_df, cols, op = _section(seed=50)
    run = lambda o, **k: same_amd.sliding_window_incumbent(r_df, m_df, commonCT=cols, optim_params=dict(o), return_stats=True, **k)
    for route in ("device", "general"):
        base, bst = run(op, _route=route)
        none, nst = run(dict(op, hip_refine=None), _route=route)
        assert none.equals(base) and nst == bst and all(not set(REFINE_KEYS) & set(s) for s in bst), route
    # a refining pass on the same context leaves nothing behind in the window states it reuses
    run(dict(op, hip_refine="local"), _route="device")
    again, ast = run(op, _route="device")
    assert again.equals(base) and ast == bst


def test_cfg5_1m_cells_merged_pass_with_refinement():
    """BASELINE config 5 at full size through the product function with the search on, window merge included: it completes, is stable
    over two passes, never raises a window's objective; the windows that stopped at the round cap are reported"""
    import same_amd
    from same_amd import synth

    T = 8
    ref = synth.make_cells(1_000_000, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10,
              hip_refine="local")
    with same_amd.resident_frames(r_df, m_df) as res:
        first, st1 = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op), merge=True, return_stats=True)
        second, st2 = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op), merge=True, return_stats=True)
    assert len(first) > 900_000 and first.equals(second) and st1 == st2
    assert len(st1) > 100 and all(s["mip_objective"] <= s["mip_objective_start"] for s in st1)
    capped = sum(1 for s in st1 if not s["refine_settled"])
    rounds = [s["refine_rounds"] for s in st1]
    print(f"cfg 5 with refinement: {len(st1)} windows, {capped} at the round cap, rounds mean {np.mean(rounds):.2f} max {max(rounds)}")
