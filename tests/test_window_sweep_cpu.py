"""The parts of the parameter sweep (same_amd.sliding_window_sweep, csrc/window_knn_prefix.hip) that need no GPU: the entry point's
declaration, the argument checks, and -- on the very inputs tests/test_gpu_window_sweep.py drives the library with -- the proof that the
host statement of the prefix rule (tests/knn_prefix_check.prefix) over the list pruned at k_max IS the reference's prune at the smaller k
(oracle.knn_prune through tests/caller_check.host_stage), and that the inputs hold the shapes the rule can go wrong at."""
import os

import numpy as np
import pytest

import caller_check as C
import knn_prefix_check as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_exported():
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "int same_window_knn_prefix(" in header and "same_window_knn_prefix" in _lib.EXPORTS
    assert _lib._PROTOTYPES["same_window_knn_prefix"] == [_lib.c_vp, _lib.c_int, _lib.c_int, _lib.c_vp]
    assert hasattr(_lib.load(), "same_window_knn_prefix") and _lib.load().same_abi_version() == 9
    assert (_lib.SAME_WINDOW_STATS, _lib.SAME_WINDOW_STATS_CAP, _lib.SAME_WINDOW_STATS_TRANSPORT) == (15, 16, 17)
    srcs = open(os.path.join(ROOT, "same_amd", "csrc", "Makefile")).read()
    assert "window_knn_prefix.hip" in srcs


def test_public_function_is_exported():
    import same_amd
    from same_amd import sweep

    assert same_amd.sliding_window_sweep is sweep.sliding_window_sweep and "sliding_window_sweep" in same_amd.__all__
    assert sweep.SWEEP_KEYS == ("knn", "no_match_penalty", "delaunay_penalty", "penalty_coeff", "max_matches",
                                "ref_metacell_match_multiplier", "hip_incumbent", "hip_refine", "hip_refine_rounds")


@pytest.fixture(scope="module")
def checked(oracle):
    """per (family, k): the statement over the list pruned at k_max, held against the reference's prune at k; -> the records the shape
    test reads"""
    records = []
    for tag, case, box, radius, k_max in K.families(oracle):
        axy_all, rxy_all = case["mov_xy"], case["ref_xy"]
        rows, rows_r, pairs = C.host_stage(axy_all, rxy_all, box, radius, k_max, oracle)
        costs = np.arange(len(pairs), dtype=np.float64) * 0.5 + 1.0
        d2 = K.pair_d2(axy_all[rows], rxy_all[rows_r], pairs) if len(pairs) else np.zeros(0)
        per_row = np.bincount(pairs[:, 0], minlength=len(rows))
        first = np.concatenate(([0], np.cumsum(per_row)))
        for k in K.smaller(k_max):
            got = K.prefix(rows, pairs, costs, rows_r, k)
            w_rows, w_rows_r, w_pairs = C.host_stage(axy_all, rxy_all, box, radius, k, oracle)
            assert np.array_equal(got["rows"], w_rows) and np.array_equal(got["ref_rows"], w_rows_r), (tag, k)
            assert got["pairs"].dtype == w_pairs.dtype and np.array_equal(got["pairs"], w_pairs), (tag, k)
            assert got["counts"] == (len(w_rows), len(w_pairs)), (tag, k)
            assert np.array_equal(got["prow"], np.concatenate(([0], np.cumsum(np.bincount(w_pairs[:, 0], minlength=len(w_rows)))))), (tag, k)
            if len(pairs):
                assert np.array_equal(got["costs"], C.costs_of(pairs, costs, w_pairs, len(rows_r))), (tag, k)     # the costs ride with their pairs
            # the compacted reference frame (src/utils.py:734-742) of the reference's own list at k
            used = np.zeros(len(w_rows_r), bool)
            used[w_pairs[:, 1]] = True
            assert np.array_equal(got["frame_rows"], w_rows_r[used]), (tag, k)
            assert np.array_equal(got["frame_pairs"], np.column_stack((w_pairs[:, 0], (np.cumsum(used) - 1)[w_pairs[:, 1]]))), (tag, k)
            if k == k_max:
                assert np.array_equal(got["pairs"], pairs) and np.array_equal(got["costs"], costs), (tag, k)
            full = np.flatnonzero(per_row > k)          # rows cut at k: is the pair at place k as far as the one at place k - 1?
            straddle = int(np.count_nonzero(d2[first[full] + k] == d2[first[full] + k - 1])) if len(full) else 0
            named_all, named_k = np.unique(pairs[:, 1]), np.unique(got["pairs"][:, 1])
            gone = np.setdiff1d(named_all, named_k)
            shifted = bool(len(gone)) and bool((named_k > gone.min()).any())      # a later reference moves down in the frame
            records.append(dict(tag=tag, k=k, k_max=k_max, fewer=int(np.count_nonzero((per_row > 0) & (per_row < k))),
                                exact=int(np.count_nonzero(per_row == k)), more=len(full), straddle=straddle, gone=len(gone),
                                shifted=shifted, rows=len(rows), pairs=len(pairs)))
    return records


def test_statement_is_the_reference_prune_at_the_smaller_k(checked):
    tags = {r["tag"] for r in checked}
    assert {"base/whole", "base/sliver", "base/empty", "base/beside", "tie", "contention"} <= tags
    assert {f"edge/{n}" for n in C.EDGE_ROWS} <= tags
    assert {r["k"] for r in checked if r["tag"] == "tie"} == {1, 2, 64, 65, 199, 200}
    assert {r["k"] for r in checked if r["tag"] == "base/whole"} == {1, 2, 7, 8}


def test_inputs_hold_the_shapes_the_rule_can_go_wrong_at(checked):
    by = {(r["tag"], r["k"]): r for r in checked}
    # a row with fewer than k pairs, one with exactly k, one with more -- in ONE window at one k
    sliver = by[("base/sliver", 2)]
    assert sliver["fewer"] > 0 and sliver["exact"] > 0 and sliver["more"] > 0, sliver
    assert by[("base/sliver", 1)]["more"] > 0 and by[("base/sliver", 7)]["fewer"] > 0
    assert by[("base/whole", 7)]["more"] > 20 * 256                       # (a dense window: nearly every row is cut)
    # a distance tie straddling position k: the four exactly equidistant nearest references of the tie family at k = 1, 2; whole shells at 64, 65
    for k in (1, 2, 64, 65, 199):
        assert by[("tie", k)]["straddle"] > 100, by[("tie", k)]
    # the tie family's source is the large-capacity prune: rows of 200 pairs, rows of 65 and more
    assert by[("tie", 200)]["exact"] > 100 and by[("tie", 65)]["more"] > 100
    # a reference named only by pairs beyond k: it leaves the compacted frame and the numbering of later references shifts
    for key in (("base/whole", 1), ("base/whole", 2), ("base/interior", 1)):
        assert by[key]["gone"] > 0 and by[key]["shifted"], by[key]
    assert by[("contention", 1)]["gone"] == 8 and by[("contention", 7)]["more"] == C.CONTENTION_ROWS     # 9 references, every row sees all
    # windows that keep nothing, and scans over one block, a block edge, and more blocks than one look-back reads (64)
    assert by[("base/empty", 1)]["rows"] == 0 and by[("base/beside", 1)]["rows"] == 0
    assert [by[(f"edge/{n}", 1)]["rows"] for n in C.EDGE_ROWS] == list(C.EDGE_ROWS) and C.EDGE_ROWS[-1] > 64 * 256
    assert by[("base/whole", 8)]["rows"] > 20 * 256


def _frames(n=400, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1))


@pytest.mark.parametrize("sets, op, message", [
    ([{"knn": 4}, {"radius": 30}], None, "radius"),
    ([{"window_size": 500}], None, "window_size"),
    ([{"hip_delaunay": "device"}], None, "hip_delaunay"),
    ([], None, "non-empty"),
    (None, None, "non-empty"),
    ({"knn": 4}, None, "non-empty"),
    ([{"knn": 4}, ("knn", 2)], None, "dict"),
    ([{"knn": 4}, {"hip_refine": "local", "hip_incumbent": "transport"}], None, "hip_refine='local'"),
    ([{"hip_refine": "local"}], {"hip_incumbent": "transport"}, "hip_refine='local'"),
    ([{"knn": 8}, {"knn": 0}], None, "knn"),
    ([{"knn": -2}], None, "knn"),
    ([{"knn": 2.5}], None, "knn"),
    ([{"knn": True}], None, "knn"),
    ([{}], {"knn": 0}, "knn"),
    ([{"hip_incumbent": "hungarian"}], None, "hip_incumbent"),
    ([{"hip_refine": "local", "hip_refine_rounds": 0}], None, "hip_refine_rounds"),
    ([{"hip_refine": "capacity", "max_matches": 0}], None, "max_matches"),
])
def test_invalid_arguments_raise_before_any_device_call(monkeypatch, sets, op, message):
    from same_amd import incumbent, sweep, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    for module in (window_api, incumbent, sweep):
        monkeypatch.setattr(module, "_WindowJob", no_job)
    ref, mov = _frames()
    with pytest.raises(ValueError) as e:
        sweep.sliding_window_sweep(ref, mov, sets, optim_params=op)
    assert message in str(e.value)


def test_valid_sets_pass_the_checks():
    from same_amd.sweep import _checked_sets

    ref, mov = _frames()
    got = _checked_sets([{"knn": 4}, {}, {"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2}], {"knn": 6, "radius": 30},
                        None, mov)
    assert [op.get("knn") for op, _m in got] == [4, 6, 6] and all(op["radius"] == 30 for op, _m in got)
    assert [(m.incumbent, m.refine) for _op, m in got] == [("greedy", None), ("greedy", None), ("transport", "capacity")]
    assert got[2][1].capacity[0] == 2
