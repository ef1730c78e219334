"""The transport start (optim_params["hip_incumbent"] = "transport", csrc/assign.hip) on the CPU: the ABI surface, the argument checks
that run before anything reaches a device, and the host solver the device's answers are measured against
(ops.sparse_transport_host: scipy's sparse matching on the expanded graph) -- against an exhaustive enumeration, against scipy's
dense solver on the expanded matrix, and against ops.sparse_assign_host where every limit is 1 (tests/transport_check.py)."""
import ctypes
import os

import numpy as np
import pytest

import transport_check as T
from test_assign_cpu import _frames, random_problem

NEW = ("same_sparse_assign_cap",)


def test_abi9_transport_symbols_declared_exported_and_built():
    from same_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "#define SAME_INCUMBENT_TRANSPORT 2" in header and _lib.SAME_INCUMBENT_TRANSPORT == 2
    assert "#define SAME_WINDOW_STATS_TRANSPORT 17" in header and _lib.SAME_WINDOW_STATS_TRANSPORT == 17
    assert "#define SAME_WINDOW_STATS_CAP 16" in header and "#define SAME_WINDOW_STATS 15" in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert f"int {name}(" in header
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert len(_lib._PROTOTYPES["same_sparse_assign_cap"]) == len(_lib._PROTOTYPES["same_sparse_assign"]) + 2


def test_transport_mode_passes_the_checks():
    from same_amd.incumbent import INCUMBENTS, incumbent_mode, transport_capacity

    _ref, mov = _frames()
    assert "transport" in INCUMBENTS
    assert incumbent_mode({"hip_incumbent": "transport", "max_matches": 2}, None, mov) == "transport"
    assert incumbent_mode({"hip_incumbent": "transport"}, None, mov) == "transport"
    op = {"hip_incumbent": "transport", "max_matches": 3, "ref_metacell_match_multiplier": 4, "penalty_coeff": 7}
    assert incumbent_mode(op, None, mov) == "transport" and transport_capacity(op) == (3, 4, 7.0)
    assert transport_capacity({"hip_incumbent": "assignment"}) is None and transport_capacity(None) is None
    # the one-to-one start keeps refusing what the reference's Hungarian start refuses, in its words
    with pytest.raises(ValueError, match="init_method='hungarian' requires max_matches == 1."):
        incumbent_mode({"hip_incumbent": "assignment", "max_matches": 2}, None, mov)


@pytest.mark.parametrize("op, message", [
    ({"penalty_coeff": -1.0}, "penalty_coeff"),
    ({"penalty_coeff": float("nan")}, "penalty_coeff"),
    ({"penalty_coeff": float("inf")}, "penalty_coeff"),
    ({"penalty_coeff": True}, "penalty_coeff"),
    ({"max_matches": 0}, "max_matches"),
    ({"max_matches": 1.5}, "max_matches"),
    ({"max_matches": True}, "max_matches"),
    ({"ref_metacell_match_multiplier": 0}, "ref_metacell_match_multiplier"),
    ({"ref_metacell_match_multiplier": 2.0}, "ref_metacell_match_multiplier"),
    ({"hip_refine": "local", "max_matches": 2}, "hip_refine='local'"),
])
def test_invalid_transport_arguments_raise_before_any_device_call(monkeypatch, op, message):
    from same_amd import incumbent, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    monkeypatch.setattr(window_api, "_WindowJob", no_job)
    monkeypatch.setattr(incumbent, "_WindowJob", no_job)
    ref, mov = _frames()
    with pytest.raises(ValueError) as e:
        incumbent.sliding_window_incumbent(ref, mov, optim_params=dict(op, hip_incumbent="transport"))
    assert message in str(e.value) and "transport" in str(e.value)


@pytest.mark.parametrize("bad", [dict(limit=0), dict(limit=1002), dict(pc=-1.0), dict(pc=float("nan")), dict(short=True)])
def test_host_solver_checks_its_arguments(bad):
    from same_amd import ops

    pairs, costs, unmatched = random_problem(np.random.default_rng(1), 5, 4, 3)
    limit = np.full(4, bad.get("limit", 2), np.int32)
    if bad.get("short"):
        limit = limit[:3]
    with pytest.raises(ValueError, match="transport"):
        ops.sparse_transport_host(pairs, costs, unmatched, 5, 4, limit, bad.get("pc", 1.0))
    with pytest.raises(ValueError, match="transport"):          # the device form checks first, by the same rule: no context is made
        ops.sparse_transport(pairs, costs, unmatched, 5, 4, limit, bad.get("pc", 1.0), ctx=object())


def test_host_solver_equals_exhaustive_enumeration():
    from same_amd import ops

    rng = np.random.default_rng(20261017)
    shared = 0
    for t in range(150):
        n_a, n_r = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 5)))
        limit = rng.integers(1, 4, n_r).astype(np.int32)
        pc = [0.0, 0.75, 20.0][t % 3]
        if t % 5 == 0:          # ties
            costs, unmatched = np.round(costs), np.round(unmatched)
        got = ops.sparse_transport_host(pairs, costs, unmatched, n_a, n_r, limit, pc)
        count = T.within_limits(got, pairs, n_a, n_r, limit)
        shared += int(np.maximum(count - 1, 0).sum())
        best, best_mp = T.brute_force(pairs, costs, unmatched, n_a, n_r, limit, pc)
        obj, _c = T.objective(got, pairs, costs, unmatched, n_r, pc)
        assert obj == pytest.approx(best, rel=1e-12, abs=1e-12), t
        assert ops.transport_objective(got, pairs, costs, unmatched, n_r, pc) == pytest.approx(obj, rel=1e-12, abs=1e-12)
        if t % 5 and pc > 0:    # continuous costs: the optimum is one matching
            assert np.array_equal(got, best_mp), t
    assert shared > 20          # the capacities were used


@pytest.mark.parametrize("family", ["continuous", "integer", "all_equal"])
def test_host_solver_equals_dense_solver_on_the_expanded_matrix(family):
    from same_amd import ops

    rng = np.random.default_rng({"continuous": 3, "integer": 4, "all_equal": 5}[family])
    for t in range(60):
        n_a, n_r = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 8)))
        if family == "integer":
            costs, unmatched = rng.integers(0, 6, len(costs)).astype(np.float64), rng.integers(3, 8, n_a).astype(np.float64)
        elif family == "all_equal":
            costs[:], unmatched[:] = 3.0, 5.0
        limit = T.random_limits(rng, n_r)
        pc = [0.0, 0.5, 13.0][t % 3] if family == "continuous" else float(t % 3)
        got = ops.sparse_transport_host(pairs, costs, unmatched, n_a, n_r, limit, pc)
        want = T.dense_transport(pairs, costs, unmatched, n_a, n_r, limit, pc)
        T.within_limits(got, pairs, n_a, n_r, limit)
        T.within_limits(want, pairs, n_a, n_r, limit)
        a, b = (T.objective(m, pairs, costs, unmatched, n_r, pc)[0] for m in (got, want))
        assert a == pytest.approx(b, rel=1e-12, abs=1e-12), t
        if family == "continuous" and pc > 0:
            assert np.array_equal(got, want), t


def test_every_limit_one_is_the_assignment():
    from same_amd import ops

    rng = np.random.default_rng(11)
    for t in range(100):
        n_a, n_r = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 8)))
        got = ops.sparse_transport_host(pairs, costs, unmatched, n_a, n_r, np.ones(n_r, np.int32), [0.0, 3.0][t % 2])
        assert np.array_equal(got, ops.sparse_assign_host(pairs, costs, unmatched, n_a, n_r)), t
        assert ops.transport_objective(got, pairs, costs, unmatched, n_r, 3.0) == ops.assign_objective(got, costs, unmatched)


def test_window_limits_follow_the_models_rule():
    """windows.window_ref_limits (the fallback's limits on the device route) against api.ref_match_limits over the frame of the
    references the pairs name"""
    import pandas as pd

    from same_amd.api import ref_match_limits
    from same_amd.windows import window_ref_limits

    rng = np.random.default_rng(2)
    for t in range(40):
        n_r = int(rng.integers(2, 30))
        size = np.where(rng.random(n_r) < [0.0, 0.4][t % 2], rng.integers(2, 9, n_r), 1)
        used = np.flatnonzero(rng.random(n_r) < 0.7)
        if not len(used):
            continue
        pairs = np.column_stack((np.zeros(len(used), np.int64), used))
        for mm, mult in ((1, None), (2, None), (2, 3), (400, 5)):
            got = window_ref_limits(size, pairs, (mm, mult, 1.0))
            want = np.minimum(ref_match_limits(pd.DataFrame({"size": size[used]}), mm, mult), 1001)
            assert np.array_equal(got[used], want), (t, mm, mult)
