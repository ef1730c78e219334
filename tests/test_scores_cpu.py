"""The parts of same_amd.sliding_window_scores (scores.py, csrc/window_score.hip) that need no GPU: the entry point's declaration, the one
function that turns counts into percentages, and every refusal that has to come before a job or a device is touched."""
import math
import os

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_score_call_is_declared_and_the_abi_stays_at_9():
    """fails without the feature: no same_merge_acc_score"""
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "int same_merge_acc_score(same_merge_acc *acc, const same_section *moving, const same_section *ref," in header
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "same_merge_acc_score" in _lib.EXPORTS and len(_lib._PROTOTYPES["same_merge_acc_score"]) == 9
    lib = _lib.load()
    assert hasattr(lib, "same_merge_acc_score") and lib.same_abi_version() == 9


COUNTS = dict(matched=7, type_matches=3, total_triangles=11, triangles_with_all_matched=6, triangles_same_type_skipped=2, triangles_flipped=1,
              nodes_in_violating_triangles=3)


def test_record_from_counts_uses_the_expressions_of_check_triangle_violations():
    from same_amd import record_from_counts
    from same_amd.scores import RECORD_KEYS

    rec = record_from_counts(COUNTS)
    assert tuple(rec) == RECORD_KEYS
    assert rec["accuracy"] == 100 * (3 / 7) and rec["percent_flipped"] == 100.0 * 1 / 4 and rec["violations"] == 100 * 1 / 11
    assert rec["percent_nodes_violating"] == 100.0 * (3 / 7)
    assert all(isinstance(rec[k], int) for k in RECORD_KEYS if "percent" not in k and k not in ("accuracy", "violations"))
    # no triangulation: the triangle keys are left out
    assert tuple(record_from_counts(dict(matched=7, type_matches=3))) == ("matched", "type_matches", "accuracy")
    assert tuple(record_from_counts(dict(matched=7, type_matches=3, total_triangles=None))) == ("matched", "type_matches", "accuracy")
    # none considered: every matched triangle has one type
    none = record_from_counts(dict(COUNTS, triangles_same_type_skipped=6, triangles_flipped=0, nodes_in_violating_triangles=0))
    assert none["percent_flipped"] == 0.0 and none["violations"] == 0.0 and none["percent_nodes_violating"] == 0.0
    # an empty table: counts 0, percent_flipped 0.0, the quotients over its rows NaN
    empty = record_from_counts(dict(matched=0, type_matches=0, total_triangles=11, triangles_with_all_matched=0,
                                    triangles_same_type_skipped=0, triangles_flipped=0, nodes_in_violating_triangles=0))
    assert empty["percent_flipped"] == 0.0 and math.isnan(empty["accuracy"]) and math.isnan(empty["percent_nodes_violating"])
    assert empty["violations"] == 0.0 and empty["matched"] == empty["triangles_flipped"] == 0
    # ... and no triangles at all
    assert math.isnan(record_from_counts(dict(empty, total_triangles=0))["violations"])


def test_the_node_local_rule_at_its_thresholds():
    """per table row (triangles not skipped, flipped ones): the rule of src/eval_utils.py:199-211, `>=` on both thresholds"""
    from same_amd import record_from_counts

    base = {k: v for k, v in COUNTS.items() if k != "nodes_in_violating_triangles"}
    n_tri, n_flip = [0, 2, 2, 4, 3, 3, 5], [0, 1, 2, 1, 0, 3, 2]
    nodes = lambda **p: record_from_counts(dict(base, node_triangles=n_tri, node_flips=n_flip), p)["nodes_in_violating_triangles"]
    assert nodes() == 5                                                        # any flip
    assert nodes(node_local=True) == 3                                         # 1/2, 2/2, 3/3 reach 0.5; 1/4 and 2/5 do not
    assert nodes(node_local=True, majority_threshold=1.0) == 2                 # equality at 1.0: 2/2 and 3/3
    assert nodes(node_local=True, majority_threshold=0.25) == 5                # equality at 0.25: 1/4 joins, and 2/5
    assert nodes(node_local=True, majority_threshold=0.25, min_flips=2) == 3   # equality at min_flips: 2 and 3 flips stay
    assert nodes(node_local=True, majority_threshold=0.0, min_flips=0) == 6    # a cell without triangles is never violating


def _frames(n=40):
    rng = np.random.default_rng(5)
    df = pd.DataFrame({"X": rng.random(n) * 100, "Y": rng.random(n) * 100, "c1": 1.0, "c2": 0.0, "cell_type": ["c1", "c2"] * (n // 2),
                       "Cell_Num_Old": np.arange(n)})
    return df, df.copy()


@pytest.fixture
def no_device(monkeypatch):
    """a device, a window job's sections or a library call would raise"""
    from same_amd import _lib, window_api

    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was touched"))
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(window_api._DeviceFrames, "__init__", boom)
    monkeypatch.setattr(window_api._WindowJob, "device_frames", boom)


@pytest.mark.parametrize("score_params", [{"min_flip": 1}, {"verbose": True}, ["node_local"], {"majority_threshold": "0.5"},
                                          {"majority_threshold": None}, {"majority_threshold": True}, {"majority_threshold": float("nan")},
                                          {"min_flips": 1.0}, {"min_flips": "1"}, {"min_flips": False}, {"node_local": 1},
                                          {"ignore_same_type_triangles": "yes"}])
def test_score_params_are_refused_before_a_device_is_touched(no_device, score_params):
    import same_amd

    ref, mov = _frames()
    with pytest.raises(ValueError, match="score_params"):
        same_amd.sliding_window_scores(ref, mov, ["c1", "c2"], score_params=score_params)
    with pytest.raises(ValueError, match="score_params"):
        same_amd.score_table(pd.DataFrame(), ref, mov, cell_id_col="Cell_Num_Old", score_params=score_params)
    with pytest.raises(ValueError, match="score_params"):
        same_amd.record_from_counts(COUNTS, score_params)


def test_good_score_params_are_taken():
    from same_amd.scores import SCORE_PARAMS, checked_score_params

    assert checked_score_params(None) == SCORE_PARAMS == dict(ignore_same_type_triangles=True, node_local=False, majority_threshold=0.5,
                                                               min_flips=1)
    got = checked_score_params({"majority_threshold": 1, "min_flips": np.int64(3), "node_local": np.bool_(True)})
    assert got == dict(SCORE_PARAMS, majority_threshold=1.0, min_flips=3, node_local=True)
    assert type(got["majority_threshold"]) is float and type(got["min_flips"]) is int and type(got["node_local"]) is bool


@pytest.mark.parametrize("side", ["ref", "moving"])
def test_a_frame_without_cell_type_is_refused(no_device, side):
    import same_amd

    ref, mov = _frames()
    (ref if side == "ref" else mov).drop(columns="cell_type", inplace=True)
    with pytest.raises(ValueError, match=f"the {side} frame has no 'cell_type'"):
        same_amd.sliding_window_scores(ref, mov, ["c1", "c2"])
    with pytest.raises(ValueError, match=f"the {side} frame has no 'cell_type'"):
        same_amd.score_table(pd.DataFrame(), ref, mov, cell_id_col="Cell_Num_Old")


def test_the_variants_and_the_sets_own_refusals_come_first(no_device):
    import same_amd

    ref, mov = _frames()
    run = lambda **kw: same_amd.sliding_window_scores(ref, mov, ["c1", "c2"], **kw)
    with pytest.raises(ValueError, match="type_variants must be a non-empty list"):
        run(type_variants=[])
    with pytest.raises(ValueError, match="type_variants must be a non-empty list"):
        run(type_variants={"a": None})
    with pytest.raises(ValueError, match=r"type_variants\[1\] has shape"):
        run(type_variants=[None, np.zeros((len(mov), 3))])
    with pytest.raises(ValueError, match="param_sets must be a non-empty list"):
        run(param_sets=[])
    with pytest.raises(ValueError, match=r"param_sets\[0\] overrides \['radius'\]"):
        run(param_sets=[{"radius": 3}])
    with pytest.raises(ValueError, match="knn must be an int"):
        run(param_sets=[{"knn": 0}])
    with pytest.raises(ValueError, match=r"shape \(n, 3\)"):
        run(score_delaunay=np.zeros((4, 2), int))


def test_score_table_of_an_empty_table_needs_no_device(no_device):
    import same_amd

    ref, mov = _frames()
    rec = same_amd.score_table(pd.DataFrame(), ref, mov, cell_id_col="Cell_Num_Old", score_delaunay=np.array([[0, 1, 2], [1, 2, 99]]))
    assert rec["matched"] == 0 and rec["total_triangles"] == 2 and rec["triangles_with_all_matched"] == 0 and math.isnan(rec["accuracy"])
    assert "total_triangles" not in same_amd.score_table(pd.DataFrame(), ref, mov, cell_id_col="Cell_Num_Old")
