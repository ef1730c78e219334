"""The local search within the model's reference capacities (optim_params["hip_refine"] = "capacity", csrc/refine.hip) on the CPU: the
ABI surface, the argument checks that run before anything reaches a device, the per-reference limits against the reference's own
model builder, and the host statement (tests/refine_capacity_check.py) against what it promises."""
import ctypes
import os

import numpy as np
import pytest

import refine_capacity_check as rcc
import refine_check as rc

NEW = ("same_window_filter_finish_cap", "same_window_refinish_cap", "same_refine_matching_cap")


def test_capacity_entry_points_declared_exported_and_built():
    from same_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "#define SAME_WINDOW_STATS_CAP 16" in header and _lib.SAME_WINDOW_STATS_CAP == 16
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert f"int {name}(" in header
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def test_refine_mode_capacity():
    from same_amd.incumbent import REFINES, refine_mode

    assert REFINES == ("local", "capacity")
    assert refine_mode({"hip_refine": "local"}) == (32, 5.0)
    assert refine_mode({"hip_refine": "capacity"}) == (32, 5.0, (1, None, 100.0))
    assert refine_mode({"hip_refine": "capacity", "max_matches": 3, "ref_metacell_match_multiplier": 2, "penalty_coeff": 0,
                        "hip_refine_rounds": 4}) == (4, 5.0, (3, 2, 0.0))


def _frames(n=300, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1))


@pytest.mark.parametrize("op, message", [
    ({"penalty_coeff": -1.0}, "penalty_coeff"),
    ({"penalty_coeff": float("nan")}, "penalty_coeff"),
    ({"penalty_coeff": float("inf")}, "penalty_coeff"),
    ({"max_matches": 0}, "max_matches"),
    ({"max_matches": 1.5}, "max_matches"),
    ({"max_matches": True}, "max_matches"),
    ({"ref_metacell_match_multiplier": 0}, "ref_metacell_match_multiplier"),
    ({"ref_metacell_match_multiplier": 2.0}, "ref_metacell_match_multiplier"),
    ({"ref_metacell_match_multiplier": -3}, "ref_metacell_match_multiplier"),
])
def test_invalid_capacity_arguments_raise_before_any_device_call(monkeypatch, op, message):
    from same_amd import incumbent, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    monkeypatch.setattr(window_api, "_WindowJob", no_job)
    monkeypatch.setattr(incumbent, "_WindowJob", no_job)
    ref, mov = _frames()
    with pytest.raises(ValueError, match=message):
        incumbent.sliding_window_incumbent(ref, mov, optim_params={"hip_refine": "capacity", **op})


# ---- the limits against the reference's add_basic_constraints_optimized (tests/golden/ref_match_limits.npz, tools/gen_ref_limits.py)
def test_ref_match_limits_match_the_reference():
    import pandas as pd

    from conftest import load_golden
    from same_amd.api import ref_match_limits

    g = load_golden("ref_match_limits")
    seen_meta = seen_plain = 0
    for name in g["frames"]:
        name = str(name)
        size = g[f"{name}_size"]
        r_df = pd.DataFrame({"X": np.zeros(len(size))})
        if bool(g[f"{name}_has_size"]):
            r_df["size"] = size
        for mm in g["max_matches"]:
            for mult in g["multipliers"]:
                rows = g[f"{name}_mm{int(mm)}_mult{mult}"]
                lim = ref_match_limits(r_df, int(mm), None if str(mult) == "None" else int(mult))
                assert len(rows) == len(np.unique(g[f"{name}_pairs"][:, 1]))
                for j, want in rows:
                    assert lim[int(j)] == want, (name, mm, mult, int(j))
                    seen_meta += want != mm
                    seen_plain += want == mm
    assert seen_meta and seen_plain


# ---- the host statement
FAMILIES = [("uniform", dict()), ("clustered", dict()), ("lattice", dict()), ("uniform", dict(equal_costs=True)),
            ("clustered", dict(delaunay_penalty=0.0))]


@pytest.mark.parametrize("kind, kw", FAMILIES)
@pytest.mark.parametrize("pc", [0.0, 1.0, 100.0])
def test_statement_rounds_lower_the_objective_and_respect_limits(kind, kw, pc):
    args, start = rcc.make_cap_problem(kind, n=48, seed=3, penalty_coeff=pc, **kw)
    prob = rcc.CapProblem(**args)
    m, st = rcc.refine(prob, start, 50)
    assert all(b < a for a, b in zip(st["trace"], st["trace"][1:]))
    assert st["settled"] == 1
    count = prob.counts(m)                                   # asserts count <= limit
    assert all(c <= l for c, l in zip(count, prob.limit))
    assert st["ref_extra_matches"] == sum(max(0, c - 1) for c in count)
    want, extra = rcc.model_objective(args["pairs"], args["costs"], args["n"], args["triangles"], args["axy"], args["ref_xy"],
                                      args["size"], m, 3.0, args["delaunay_penalty"], pc)
    assert extra == st["ref_extra_matches"]
    assert st["objective"] == pytest.approx(want, rel=1e-12, abs=1e-9)
    assert st["objective"] == prob.cap_objective(m)


def test_statement_uses_capacity():
    """with room, a cheap penalty and a high no-match cost, some reference ends up held more than once"""
    args, start = rcc.make_cap_problem("clustered", n=60, seed=5, limits=(3,), penalty_coeff=0.01, no_match_penalty=50.0)
    prob = rcc.CapProblem(**args)
    m, st = rcc.refine(prob, start, 50)
    assert st["ref_extra_matches"] > 0 and st["objective"] < st["objective_start"]


@pytest.mark.parametrize("kind, kw", FAMILIES)
@pytest.mark.parametrize("cap", [1, 2, 50])
def test_statement_with_every_limit_one_is_the_local_search(kind, kw, cap):
    kwargs, start = rc.make_problem(kind, n=50, seed=11, **kw)
    m0, st0 = rc.refine(rc.Problem(**kwargs), start, cap)
    for pc in (0.0, 7.0):
        m1, st1 = rcc.refine(rcc.CapProblem(**kwargs, penalty_coeff=pc), start, cap)
        assert np.array_equal(m0, m1)
        for k in ("rounds", "moves", "settled", "objective_start", "objective", "trace"):
            assert st0[k] == st1[k], k
        assert st1["ref_extra_matches"] == 0
