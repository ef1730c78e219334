"""same_amd.score_maps without a GPU: `score_table_maps` on the parts that need no kernel (no triangulation: matches, labels, truth,
ranks), every argument check of `sliding_window_score_maps` before a job or a device is touched, and the new entry points in the
header, the ctypes table and the built library at ABI 9."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = "Cell_Num_Old"
NEW = ("same_score_map_create", "same_score_map_destroy", "same_score_map_tally", "same_score_map_reset", "same_merge_acc_score_map")


def _frames():
    cols = ["A", "B", "C"]
    ref = pd.DataFrame({"X": [0.0, 1.0, 2.0, 3.0], "Y": [0.0, 0.0, 0.0, 0.0], "A": [0.7, 0.5, 0.1, np.nan], "B": [0.2, 0.5, 0.1, 0.5],
                        "C": [0.1, 0.0, 0.8, 0.5], "cell_type": ["A", "B", "C", "A"], CID: [10, 11, 12, 13]})
    mov = pd.DataFrame({"X": [0.1, 1.1, 2.1, 3.1, 4.1], "Y": [0.0] * 5, "A": [1.0, 0, 0, 0, 0], "B": [0, 1.0, 0, 0, 0], "C": [0, 0, 1.0, 1.0, 1.0],
                        "cell_type": ["A", "A", "C", "B", "nothing"], CID: [100, 101, 102, 103, 104]}, index=list("vwxyz"))
    table = pd.DataFrame({f"Aligned_{CID}": [103, 100, 101, 104], f"Ref_{CID}": [13, 10, 11, 12], "ref_X": [3.0, 0.0, 1.0, 2.0], "ref_Y": [0.0] * 4})
    return ref, mov, cols, table


def test_score_table_maps_without_a_triangulation():
    import same_amd

    ref, mov, cols, table = _frames()
    truth = {100: 10, 101: 12, 102: 12, 104: 12}
    c = same_amd.score_table_maps(table, ref, mov, cell_id_col=CID, commonCT=cols, truth=truth, ranks=True)
    assert c.index.equals(mov.index) and list(c.columns) == ["ref_row", "ref_id", "matched", "type_match", "node_triangles", "node_flips",
                                                             "considered", "in_violating_triangle", "truth_known", "on_truth", "rank_strict",
                                                             "rank_weak", "ranked"]
    assert c["ref_row"].tolist() == [0, 1, -1, 3, 2] and c["ref_row"].dtype == np.int64
    assert c["ref_id"].tolist()[:2] == [10, 11] and pd.isna(c["ref_id"].iloc[2]) and c["ref_id"].tolist()[3:] == [13, 12]
    assert c["matched"].tolist() == [True, True, False, True, True] and c["type_match"].tolist() == [True, False, False, False, False]
    assert not c["considered"].any() and not c["in_violating_triangle"].any() and not c["node_triangles"].any() and not c["node_flips"].any()
    assert c["truth_known"].tolist() == [True, True, True, False, True] and c["on_truth"].tolist() == [True, False, False, False, True]
    # v: A in (0.7, 0.2, 0.1) ranks first; w: A ties B at 0.5 (strict 0 < weak 1); y: a NaN in the row; z: its label names no column
    assert c["rank_strict"].tolist() == [0, 0, 255, 255, 255] and c["rank_weak"].tolist() == [0, 1, 255, 255, 255]
    assert c["ranked"].tolist() == [True, True, False, False, False] and c["rank_weak"].dtype == np.uint8
    plain = same_amd.score_table_maps(table, ref, mov, cell_id_col=CID)
    pd.testing.assert_frame_equal(plain, c[plain.columns], check_exact=True)
    empty = same_amd.score_table_maps(table.iloc[:0], ref, mov, cell_id_col=CID, commonCT=cols, ranks=True)
    assert not empty["matched"].any() and (empty["ref_row"] == -1).all() and empty["ref_id"].isna().all() and (empty["rank_weak"] == 255).all()
    record = same_amd.score_table(table, ref, mov, cell_id_col=CID)
    assert (record["matched"], record["type_matches"]) == (int(c["matched"].sum()), int(c["type_match"].sum()))


def test_score_table_maps_on_the_golden_tables_host_only_parts():
    """tests/golden/eval_tri.npz without its triangulation: a moving id the table names twice keeps its LAST row, as the reference's dicts"""
    import same_amd
    import score_map_check as M
    from test_oracle_golden import load_golden

    g = load_golden("eval_tri")
    table, ref, moving, _tri, cid, rows = M.golden_eval_study(g)
    cells = same_amd.score_table_maps(table, ref, moving, cell_id_col=cid)
    assert len(np.unique(rows)) < len(rows)                                     # the duplicate is there
    last = dict(zip(g["o_id"].tolist(), g["o_ref"].tolist()))
    named = np.isin(moving[cid].to_numpy(), g["o_id"])
    assert np.array_equal(cells["matched"].to_numpy(), named) and cells["matched"].sum() == len(last)
    assert cells["ref_id"][named].tolist() == [last[i] for i in moving[cid][named].tolist()] and cells["ref_id"][~named].isna().all()
    assert cells["ref_row"][named].tolist() == cells["ref_id"][named].tolist() and not cells["considered"].any()


def test_truth_as_a_series_an_array_and_a_dict_is_one_thing():
    from same_amd.score_maps import checked_truth

    ref, mov, _cols, _t = _frames()
    want = [0, 2, -1, -1, 3]
    as_dict = {100: 10, 101: 12, 104: 13}
    series = pd.Series({"z": 13, "v": 10, "w": 12, "y": None})
    array = np.array([10, 12, None, np.nan, 13], dtype=object)
    for truth in (as_dict, series, array, list(array)):
        got = checked_truth(truth, ref, mov, CID)
        assert got.dtype == np.int32 and got.tolist() == want, type(truth)
    assert checked_truth(None, ref, mov, CID) is None
    twice = ref.assign(**{CID: [10, 11, 10, 13]})                               # an id that names two rows: the last, as the tables' ids
    assert checked_truth({100: 10}, twice, mov, CID).tolist() == [2, -1, -1, -1, -1]


def test_every_argument_check_raises_before_a_device_is_touched(monkeypatch):
    import same_amd
    from same_amd import _lib, window_api

    def touched(*_a, **_k):
        raise AssertionError("a job or a device was touched")

    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.setattr(_lib, "Context", touched)
    monkeypatch.setattr(window_api._WindowJob, "__init__", touched)
    ref, mov, cols, _t = _frames()
    call = lambda **kw: same_amd.sliding_window_score_maps(ref, mov, kw.pop("commonCT", cols), optim_params={"cell_id_col": CID}, **kw)
    with pytest.raises(ValueError, match="not in the reference frame"):
        call(truth={100: 10, 101: 999})
    with pytest.raises(ValueError, match="not in the reference frame"):
        call(truth=["10", "11", "12", "13", "10"])
    with pytest.raises(ValueError, match="4 values; the moving frame has 5 rows"):
        call(truth=[10, 11, 12, 13])
    with pytest.raises(ValueError, match="truth must be"):
        call(truth="10")
    with pytest.raises(ValueError, match="pass commonCT"):
        call(ranks=True, commonCT=None)
    with pytest.raises(ValueError, match="score_params"):
        call(score_params={"nodes": 1})
    with pytest.raises(ValueError, match="no 'cell_type' column"):
        same_amd.sliding_window_score_maps(ref.drop(columns="cell_type"), mov, cols, optim_params={"cell_id_col": CID})
    with pytest.raises(ValueError, match="has no such column"):
        same_amd.sliding_window_score_maps(ref, mov, cols, truth={100: 10}, optim_params={"cell_id_col": "nowhere"})
    for refused in ("unpack", "tables"):                                        # cell-level maps and tables are not this call's
        with pytest.raises(TypeError, match=refused):
            call(**{refused: "nearest"})
    with pytest.raises(ValueError, match="pass commonCT"):
        same_amd.score_table_maps(_t, ref, mov, cell_id_col=CID, ranks=True)


def test_the_new_entry_points_are_declared_bound_and_exported_at_abi_9():
    from same_amd import _lib
    from same_amd import windows as W

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.same_abi_version() == _lib.ABI_VERSION == 9 and "#define SAME_ABI_VERSION 9" in header
    assert len(_lib._PROTOTYPES["same_merge_acc_score_map"]) == 12 and lib.same_score_map_destroy.restype is None
    assert "uint8_t flags, rank_strict, rank_weak, reserved; } same_cell_mark;" in code and W.CELL_MARK.itemsize == 16
    assert (_lib.SAME_MARK_MATCHED, _lib.SAME_MARK_TYPE_MATCH, _lib.SAME_MARK_CONSIDERED, _lib.SAME_MARK_VIOLATING, _lib.SAME_MARK_TRUTH_KNOWN,
            _lib.SAME_MARK_ON_TRUTH, _lib.SAME_MARK_RANKED) == (1, 2, 4, 8, 16, 32, 64)
    # null handles are refused, not followed: no device is needed to be told so
    out = np.zeros(10, np.int64)
    assert lib.same_merge_acc_score_map(None, None, None, None, None, None, 1, 0, 0.5, 1, None, out.ctypes.data) == _lib.SAME_EINVAL
    assert lib.same_score_map_tally(None, None, None) == _lib.SAME_EINVAL and lib.same_score_map_reset(None) == _lib.SAME_EINVAL
    assert lib.same_score_map_create(None, None, None, None, 1, ctypes.byref(ctypes.c_void_p())) == _lib.SAME_EINVAL
    lib.same_score_map_destroy(None)
