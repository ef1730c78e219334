"""The local search on the lazy model's objective (optim_params["hip_refine"] = "local", csrc/refine.hip) on the CPU: the ABI surface, the
argument checks that must run before anything reaches a device, and the host statement of the round rule (tests/refine_check.py)
against what the rule promises: the objective never goes up, a settled result admits no improving move, it lies between the optimum
and the start, it depends on the triangle set alone, and its objective is src/same.py:1191-1196 evaluated directly."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import refine_check as rc

NEW = ("same_window_filter_finish", "same_window_refinish", "same_refine_matching")
GONE = ("same_window_filter_finish_device", "same_window_set_incumbent", "same_window_incumbent_result", "same_window_set_refine",
        "same_window_refine_result")     # folded into same_window_filter_finish (ABI 9)


def test_abi9_entry_points_declared_exported_and_built():
    from same_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert f"int {name}(" in header
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    for name in GONE:
        assert name not in _lib.EXPORTS and not hasattr(lib, name)


def _frames(n=400, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1))


@pytest.mark.parametrize("op, message", [
    ({"hip_refine": "global"}, "hip_refine"),
    ({"hip_refine": "Local"}, "hip_refine"),
    ({"hip_refine": True}, "hip_refine"),
    ({"hip_refine": "local", "hip_refine_rounds": 0}, "hip_refine_rounds"),
    ({"hip_refine": "local", "hip_refine_rounds": -3}, "hip_refine_rounds"),
    ({"hip_refine": "local", "hip_refine_rounds": 2.5}, "hip_refine_rounds"),
    ({"hip_refine": "local", "hip_refine_rounds": True}, "hip_refine_rounds"),
    ({"hip_refine": "local", "delaunay_penalty": -1.0}, "delaunay_penalty"),
    ({"hip_refine": "local", "delaunay_penalty": float("nan")}, "delaunay_penalty"),
    ({"hip_refine": "local", "delaunay_penalty": float("inf")}, "delaunay_penalty"),
    ({"hip_refine": "local", "hip_incumbent": "assignment", "delaunay_penalty": -2}, "delaunay_penalty"),
])
def test_invalid_arguments_raise_before_any_device_call(monkeypatch, op, message):
    from same_amd import incumbent, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    monkeypatch.setattr(window_api, "_WindowJob", no_job)
    monkeypatch.setattr(incumbent, "_WindowJob", no_job)
    ref, mov = _frames()
    with pytest.raises(ValueError) as e:
        incumbent.sliding_window_incumbent(ref, mov, optim_params=op)
    assert message in str(e.value)


def test_valid_modes_pass_the_checks():
    from same_amd.incumbent import REFINE_ROUNDS, refine_mode

    assert refine_mode(None) is None and refine_mode({}) is None and refine_mode({"hip_refine": None}) is None
    assert refine_mode({"hip_refine": "local"}) == (REFINE_ROUNDS, 5.0)
    assert refine_mode({"hip_refine": "local", "hip_refine_rounds": 3, "delaunay_penalty": 0}) == (3, 0.0)
    assert refine_mode({"hip_refine": "local", "hip_refine_rounds": np.int64(7), "delaunay_penalty": 2}) == (7, 2.0)


CASES = [(kind, seed) for kind in ("uniform", "clustered", "lattice") for seed in range(3)]


@pytest.mark.parametrize("kind, seed", CASES)
def test_objective_never_increases_and_settles_at_a_local_optimum(kind, seed):
    kw, start = rc.make_problem(kind, 120, seed=seed)
    prob = rc.Problem(**kw)
    assert rc.improving_moves(prob, start), "the start should leave something to improve"
    m, st = rc.refine(prob, start, 1000)
    assert st["settled"] == 1 and st["moves"] >= st["rounds"] > 0
    assert all(b <= a for a, b in zip(st["trace"], st["trace"][1:]))
    assert st["objective"] < st["objective_start"]
    assert rc.improving_moves(prob, m) == []
    assert len({int(prob.col(p)) for p in m if p >= 0}) == int(np.count_nonzero(m >= 0))        # one-to-one


def test_round_cap_stops_the_search():
    kw, start = rc.make_problem("uniform", 120, seed=4)
    prob = rc.Problem(**kw)
    _m, full = rc.refine(prob, start, 1000)
    assert full["rounds"] >= 2
    _m, capped = rc.refine(prob, start, 1)
    assert capped["rounds"] == 1 and capped["settled"] == 0 and capped["objective"] >= full["objective"]


def _brute_force(prob):
    best = np.inf
    options = [[-1] + prob.rows[i] for i in range(prob.n)]
    for m in itertools.product(*options):
        cols = [prob.col(p) for p in m if p >= 0]
        if len(cols) == len(set(cols)):
            best = min(best, prob.objective(list(m)))
    return best


@pytest.mark.parametrize("seed", range(6))
def test_tiny_windows_lie_between_the_optimum_and_the_start(seed):
    kw, start = rc.make_problem("uniform", 6, seed=seed, k=3, jitter=0.8)
    prob = rc.Problem(**kw)
    _m, st = rc.refine(prob, start, 100)
    opt = _brute_force(prob)
    assert opt - 1e-9 <= st["objective"] <= st["objective_start"]


@pytest.mark.parametrize("kind, seed", CASES[:5])
def test_only_the_triangle_set_matters(kind, seed):
    kw, start = rc.make_problem(kind, 100, seed=seed)
    m0, st0 = rc.refine(rc.Problem(**kw), start, 32)
    rng = np.random.default_rng(seed + 100)
    tris = np.asarray(kw["triangles"])[rng.permutation(len(kw["triangles"]))]
    tris = np.array([t[rng.permutation(3)] for t in tris])
    m1, st1 = rc.refine(rc.Problem(**dict(kw, triangles=tris)), start, 32)
    assert np.array_equal(m0, m1)
    assert (st0["rounds"], st0["moves"], st0["objective"]) == (st1["rounds"], st1["moves"], st1["objective"])


@pytest.mark.parametrize("kind, seed", CASES[:5])
def test_objective_is_the_models(kind, seed):
    kw, start = rc.make_problem(kind, 100, seed=seed)
    m, st = rc.refine(rc.Problem(**kw), start, 32)
    for match, value in ((start, st["objective_start"]), (m, st["objective"])):
        direct = rc.lazy_objective(kw["pairs"], kw["costs"], kw["n"], kw["triangles"], kw["axy"], kw["ref_xy"], kw["size"], match,
                                   3.0, kw["delaunay_penalty"])
        assert direct == pytest.approx(value, rel=1e-12)


def test_zero_delaunay_penalty_from_the_optimal_assignment_moves_nothing():
    from same_amd.ops import sparse_assign_host

    kw, _start = rc.make_problem("uniform", 80, seed=2, delaunay_penalty=0.0)
    opt = sparse_assign_host(kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"])
    _m, st = rc.refine(rc.Problem(**kw), opt, 32)
    assert st["moves"] == 0 and st["settled"] == 1
