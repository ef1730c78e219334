"""The cell-type-priority prune on the device route (optim_params["hip_priority_prune"] = "device", csrc/window_priority.hip), the parts
that need no GPU: the device rule as a host statement (tests/priority_check.py) against same_amd.knn.priority_filter -- which
tests/test_host_rows.py pins to the reference -- the key's validation, and the two entry points' declarations."""
import inspect
import os
import re

import numpy as np
import pytest

from priority_check import device_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _codes(at, rt):
    from same_amd.eval_utils import _label_codes

    return _label_codes(np.asarray(at), np.asarray(rt))


def _agree(pairs, axy, rxy, at, rt, tag):
    from same_amd.knn import priority_filter

    want, one, all_ = priority_filter(pairs, axy, rxy, at, rt)
    cm, cr = _codes(at, rt)
    got, g_one, g_all = device_rule(pairs, axy, rxy, cm, cr)
    assert np.array_equal(got, want) and (g_one, g_all) == (one, all_), tag
    return one, all_


def test_device_rule_equals_the_filter_on_the_golden_fixtures():
    from conftest import frames_from_golden, load_golden

    for case in ("synthetic_example", "cfg1_500", "cfg2_small"):
        g = load_golden(case)
        a_df, r_df, _ = frames_from_golden(g)
        na = a_df.iloc[g["kept_aligned"]].reset_index(drop=True)
        nr = r_df.iloc[g["kept_ref"]].reset_index(drop=True)
        axy, rxy = na[["X", "Y"]].to_numpy(), nr[["X", "Y"]].to_numpy()
        cm, cr = _codes(na["cell_type"].to_numpy(), nr["cell_type"].to_numpy())
        got, one, all_ = device_rule(g["pairs"], axy, rxy, cm, cr)
        assert np.array_equal(got, g["pairs_priority"]) and one > 0 and one + all_ == len(np.unique(g["pairs"][:, 0])), case


def test_device_rule_equals_the_filter_on_random_sets():
    """300 seeded sets of at most 40 x 40 cells with 2-4 labels: lattice coordinates (many equal distances), rows whose pairs are NOT in
    distance order, NaN / None labels, 1 against 1.0"""
    rng = np.random.default_rng(7)
    seen_one = seen_ties = seen_missing = seen_unordered = 0
    for trial in range(300):
        n_m, n_r = (int(v) for v in rng.integers(1, 41, 2))
        P = int(rng.integers(1, 300))
        pairs = np.unique(np.column_stack((rng.integers(0, n_m, P), rng.integers(0, n_r, P))), axis=0).reshape(-1, 2)
        rng.shuffle(pairs)                                        # any order inside a row ...
        pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]     # ... rows ascending, as staged
        if trial % 3 == 0:
            axy, rxy = rng.uniform(0, 6, (n_m, 2)), rng.uniform(0, 6, (n_r, 2))
        else:
            axy, rxy = rng.integers(0, 5, (n_m, 2)).astype(float), rng.integers(0, 5, (n_r, 2)).astype(float)
        n_lab = int(rng.integers(2, 5))
        kind = trial % 4
        if kind == 0:
            at, rt = rng.integers(0, n_lab, n_m), rng.integers(0, n_lab, n_r)
        elif kind == 1:                                           # strings with NaN and None
            pool = np.array(["a", "b", "c", "d"][:n_lab] + [np.nan, None], dtype=object)
            at, rt = pool[rng.integers(0, len(pool), n_m)], pool[rng.integers(0, len(pool), n_r)]
            seen_missing += 1
        elif kind == 2:                                           # int against float labels
            at, rt = rng.integers(0, n_lab, n_m), rng.integers(0, n_lab, n_r).astype(float)
        else:                                                     # float labels with NaN on both sides
            at, rt = rng.integers(0, n_lab, n_m).astype(float), rng.integers(0, n_lab, n_r).astype(float)
            at[rng.random(n_m) < 0.2], rt[rng.random(n_r) < 0.2] = np.nan, np.nan
        one, _all = _agree(pairs, axy, rxy, at, rt, trial)
        seen_one += one
        d = np.hypot(axy[pairs[:, 0], 0] - rxy[pairs[:, 1], 0], axy[pairs[:, 0], 1] - rxy[pairs[:, 1], 1])
        same_row = pairs[1:, 0] == pairs[:-1, 0]
        seen_ties += int(np.count_nonzero(same_row & (d[1:] == d[:-1])))
        seen_unordered += int(np.count_nonzero(same_row & (d[1:] < d[:-1])))
    assert seen_one > 300 and seen_ties > 300 and seen_unordered > 300 and seen_missing > 50


def test_missing_labels_equal_nothing_and_one_equals_one_point_zero():
    axy, rxy = np.array([[0.0, 0.0], [0.0, 1.0]]), np.array([[0.0, 0.1], [5.0, 5.0]])
    pairs = np.array([[0, 0], [0, 1], [1, 0], [1, 1]])
    for at, rt, want_one in (([np.nan, np.nan], [np.nan, 1.0], 0), (np.array([None, None], dtype=object), np.array([None, 1], dtype=object), 1),
                             ([1, 1], [1.0, 2.0], 1), (np.array(["1", "1"], dtype=object), np.array([1, 1], dtype=object), 0)):
        one, all_ = _agree(pairs, axy, rxy, np.asarray(at), np.asarray(rt), (at, rt))
        assert (one, all_) == (want_one, 2 - want_one)


def test_key_validation():
    from same_amd.window_mode import WindowMode, priority_prune_route

    assert priority_prune_route(None) == priority_prune_route({}) == priority_prune_route({"hip_priority_prune": None}) == "host"
    assert priority_prune_route({"hip_priority_prune": "host"}) == "host"
    assert priority_prune_route({"hip_priority_prune": "device"}) == "device"
    for bad in ("gpu", "Device", 1, True, b"device", ("device",)):
        with pytest.raises(ValueError, match="hip_priority_prune"):
            priority_prune_route({"hip_priority_prune": bad})
        with pytest.raises(ValueError, match="hip_priority_prune"):          # ... and before anything reaches a device
            WindowMode.from_params({"hip_priority_prune": bad})
    # the key does not change the mode, with the flag or without
    for flag in (False, True):
        assert WindowMode.from_params({"hip_priority_prune": "device", "ignore_knn_if_matched": flag}) == WindowMode.default()


def test_the_refusal_reason_follows_the_key():
    import pandas as pd
    from same_amd.params import init_optim_params
    from same_amd.window_api import caller_triangulation_refusal

    df = pd.DataFrame({"X": [0.0, 1.0, 0.0], "Y": [0.0, 0.0, 1.0], "t0": [1.0, 0.0, 0.0], "cell_type": ["a", "b", "a"], "cell_id": [0, 1, 2]})
    tri = np.array([[0, 1, 2]])
    op = init_optim_params(ignore_knn_if_matched=True)
    assert caller_triangulation_refusal(df, df, ["t0"], op, tri) == "ignore_knn_if_matched"
    assert caller_triangulation_refusal(df, df, ["t0"], dict(op, hip_priority_prune="host"), tri) == "ignore_knn_if_matched"
    assert caller_triangulation_refusal(df, df, ["t0"], dict(op, hip_priority_prune="device"), tri) is None
    assert caller_triangulation_refusal(df, df, ["t0"], dict(op, ignore_knn_if_matched=False, hip_priority_prune="device"), tri) is None


def test_entry_points_are_declared_and_bound():
    from same_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    for name in ("same_section_set_label_codes", "same_window_priority_pairs"):
        decl = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib._PROTOTYPES[name]), name
        assert name in _lib.EXPORTS
    assert "same_section_set_label_codes" in inspect.getsource(ops.section_set_label_codes)
    assert "same_window_priority_pairs" in inspect.getsource(ops.window_priority_pairs)
    srcs = open(os.path.join(ROOT, "same_amd", "csrc", "Makefile")).read()
    assert "window_priority.hip" in srcs
