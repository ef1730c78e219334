"""The optimal-assignment incumbent (optim_params["hip_incumbent"] = "assignment", csrc/assign.hip) on the CPU: the ABI surface, the
argument checks that must run before anything reaches a device, and the test oracle itself -- scipy's sparse solver on the shifted
problem (ops.sparse_assign_host) against the reference's own call, linear_sum_assignment on the dense big-M matrix
(src/init_helpers.py:150-158)."""
import ctypes
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

NEW = ("same_sparse_assign", "same_window_filter_finish", "same_window_refinish")
GONE = ("same_window_filter_finish_device", "same_window_set_incumbent", "same_window_incumbent_result", "same_window_set_refine",
        "same_window_refine_result")     # folded into same_window_filter_finish (ABI 9)


def test_abi9_entry_points_declared_exported_and_built():
    from same_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "#define SAME_INCUMBENT_GREEDY 0" in header and "#define SAME_INCUMBENT_ASSIGNMENT 1" in header
    assert (_lib.SAME_INCUMBENT_GREEDY, _lib.SAME_INCUMBENT_ASSIGNMENT) == (0, 1)
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


@pytest.mark.parametrize("op, gp, message", [
    ({"hip_incumbent": "hungarian"}, None, "hip_incumbent"),
    ({"hip_incumbent": "Assignment"}, None, "hip_incumbent"),
    ({"hip_incumbent": None}, None, "hip_incumbent"),
    ({"hip_incumbent": "assignment", "max_matches": 2}, None, "init_method='hungarian' requires max_matches == 1."),
    ({"hip_incumbent": "assignment", "no_match_penalty": 100}, {"init_big_m": 200.0}, "init_big_m / 2"),
])
def test_invalid_arguments_raise_before_any_device_call(monkeypatch, op, gp, message):
    from same_amd import incumbent, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    monkeypatch.setattr(window_api, "_WindowJob", no_job)
    monkeypatch.setattr(incumbent, "_WindowJob", no_job)
    ref, mov = _frames()
    with pytest.raises(ValueError) as e:
        incumbent.sliding_window_incumbent(ref, mov, optim_params=op, gurobi_params=gp)
    assert message in str(e.value)


def test_valid_modes_pass_the_checks():
    from same_amd.incumbent import incumbent_mode

    _ref, mov = _frames()
    assert incumbent_mode(None, None, mov) == "greedy"
    assert incumbent_mode({"hip_incumbent": "greedy", "max_matches": 3}, None, mov) == "greedy"      # greedy: nothing new is checked
    assert incumbent_mode({"hip_incumbent": "assignment"}, None, mov) == "assignment"
    # 100 * 1 is below 1e9 / 2; just below the bound is still the reference's problem
    assert incumbent_mode({"hip_incumbent": "assignment"}, {"init_big_m": 200.000001}, mov) == "assignment"


def dense_reference(pairs, costs, unmatched, n_a, n_r, big_m=1e9):
    """the reference's dense problem and call (src/init_helpers.py:150-175) -> pair index per row, -1 = unmatched"""
    cost_mat = np.full((n_a, n_r + n_a), big_m)
    cost_mat[pairs[:, 0], pairs[:, 1]] = costs
    cost_mat[np.arange(n_a), n_r + np.arange(n_a)] = unmatched
    rows, cols = linear_sum_assignment(cost_mat)
    lookup = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs.tolist())}
    out = np.full(n_a, -1, np.int32)
    for i, j in zip(rows.tolist(), cols.tolist()):
        if j < n_r and cost_mat[i, j] < big_m * 0.5:
            out[i] = lookup[(i, j)]
    return out


def random_problem(rng, n_a, n_r, k):
    rows, cols = [], []
    for i in range(n_a):
        m = int(rng.integers(0, min(k, n_r) + 1))
        c = rng.choice(n_r, size=m, replace=False)
        rows += [i] * m
        cols += c.tolist()
    pairs = np.column_stack((rows, cols)).astype(np.int32).reshape(-1, 2)
    perm = rng.permutation(len(pairs))
    pairs = pairs[perm]
    costs = rng.uniform(0.0, 10.0, len(pairs))
    unmatched = rng.uniform(2.0, 12.0, n_a)
    return pairs, costs, unmatched


def test_sparse_checker_equals_dense_reference_call():
    from same_amd.ops import assign_objective, sparse_assign_host

    rng = np.random.default_rng(20261015)
    for _ in range(200):
        n_a, n_r = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        pairs, costs, unmatched = random_problem(rng, n_a, n_r, int(rng.integers(1, 8)))
        ours = sparse_assign_host(pairs, costs, unmatched, n_a, n_r)
        ref = dense_reference(pairs, costs, unmatched, n_a, n_r)
        assert np.array_equal(ours, ref)
        assert assign_objective(ours, costs, unmatched) == pytest.approx(assign_objective(ref, costs, unmatched), rel=1e-12)
