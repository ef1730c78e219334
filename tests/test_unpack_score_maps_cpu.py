"""The parts of the cell-level maps (same_amd/score_maps.py, csrc/window_unpack_map.hip) that need no GPU: `score_unpacked_maps` under
"distribute" (which touches no kernel) on tests/test_unpack_check_cpu.py's hand-made objects, against the reference's notebook cells
written out in pandas -- examples/tongue/reproduce_figures.ipynb cell 16's `cell_type == pred_cell_type` per cell, examples/luad cell
13's np.argpartition top k --; every argument check of `sliding_window_score_maps(unpack=, cell_truth=)`, raised before a job or a device
is touched; the plain-frames refusal; the ABI surface.  Every test fails without the feature: the names do not exist."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from test_unpack_check_cpu import _objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ["a", "b", "c"]


def _typed_objects(distinct=True, missing_label=False):
    """`_objects` with type columns on the reference cells: distinct values per row (no tie at any place) or small integers"""
    ref, mov, table = _objects(missing_label)
    rng = np.random.default_rng(12)
    n = len(ref.original_df)
    values = np.argsort(rng.random((n, 3)), axis=1) + rng.random((n, 1)) if distinct else rng.integers(0, 2, (n, 3))
    for q, c in enumerate(COLS):
        ref.original_df[c] = values[:, q].astype(np.float64)
    return ref, mov, table


def _unpacked(table, ref, mov):
    from same_amd.metacell_utils import unpack_metacell_matches

    return unpack_metacell_matches(table, mov.metacell_df, ref.metacell_df, aligned_df=mov.original_df, ref_df=ref.original_df,
                                   strategy="distribute", aligned_original_idx_col=mov.original_idx_col,
                                   ref_original_idx_col=ref.original_idx_col)


@pytest.mark.parametrize("missing_label", [False, True])
def test_score_unpacked_maps_distribute_is_the_tongue_notebook_cell(missing_label):
    """every moving CELL takes the label of the reference cell the unpacked matches put it on; the panel's colour is
    cell_type == pred_cell_type"""
    import same_amd

    ref, mov, table = _typed_objects(missing_label=missing_label)
    table = table.iloc[:20]                                             # eight moving metacells stay unmatched
    got = same_amd.score_unpacked_maps(table, ref, mov, "distribute")
    expanded = _unpacked(table, ref, mov)
    protein = mov.original_df.set_index("Cell_Num_Old", drop=False)
    rna = ref.original_df.set_index("Cell_Num_Old", drop=False)
    new_pcf = protein.loc[expanded["Aligned_cell_id"].to_numpy()].copy()
    new_mer = rna.loc[expanded["Ref_cell_id"].to_numpy()]
    new_pcf["pred_cell_type"] = new_mer["cell_type"].to_numpy()
    new_pcf["SAME_X"], new_pcf["SAME_Y"] = new_mer["X"].to_numpy(), new_mer["Y"].to_numpy()
    correct = new_pcf["cell_type"] == new_pcf["pred_cell_type"]
    assert list(got.columns) == ["ref_id", "ref_cell_row", "metacell_row", "ref_metacell_row", "pair", "matched", "type_match"]
    assert got.index.name == "Cell_Num_Old" and got.index.tolist() == mov.original_df["Cell_Num_Old"].tolist()
    assert got["matched"].sum() == len(expanded) and 0 < len(expanded) < len(got)
    m = got[got["matched"]]
    assert m["type_match"].reindex(new_pcf.index).tolist() == correct.tolist() and 0 < correct.sum() < len(correct)
    assert f"{correct.mean():.1%}" == f"{m['type_match'].mean():.1%}"
    assert m["ref_id"].reindex(new_pcf.index).astype(np.int64).tolist() == expanded["Ref_cell_id"].tolist()
    assert m["pair"].reindex(new_pcf.index).tolist() == list(range(len(expanded)))
    # the reference cell's row: where the cell's SAME coordinates are read
    xy = ref.original_df[["X", "Y"]].to_numpy()[m["ref_cell_row"].reindex(new_pcf.index).to_numpy()]
    assert np.array_equal(xy, new_pcf[["SAME_X", "SAME_Y"]].to_numpy())
    # a cell finds its metacell, matched or not; its reference metacell is the table's
    owner = {c: q for q, members in enumerate(mov.metacell_df["members"]) for c in members}
    assert got["metacell_row"].tolist() == [owner[c] for c in got.index]
    by_meta = dict(zip(table["Aligned_metacell_id"], table["Ref_metacell_id"]))
    assert got["ref_metacell_row"].tolist() == [by_meta.get(q, -1) for q in got["metacell_row"]]
    u = got[~got["matched"]]
    assert len(u) and (u[["ref_cell_row", "ref_metacell_row", "pair"]] == -1).all().all() and u["ref_id"].isna().all() and not u["type_match"].any()
    assert got["ref_id"].dtype == "Int64" and got.dtypes[["ref_cell_row", "metacell_row", "ref_metacell_row", "pair"]].eq(np.int64).all()
    if missing_label:
        both_none = new_pcf["cell_type"].isna() & new_pcf["pred_cell_type"].isna()
        assert both_none.any() and not correct[both_none].any()
    # no row in the table, and a cell in no list
    empty = same_amd.score_unpacked_maps(table.iloc[:0], ref, mov, "distribute", commonCT=COLS, ranks=True, cell_truth={7: 1000})
    assert not empty["matched"].any() and empty["truth_known"].sum() == 1 and (empty["rank_weak"] == 255).all() and (empty["pair"] == -1).all()
    assert (empty["metacell_row"] >= 0).all()
    members = [list(x) for x in mov.metacell_df["members"]]
    dropped = members[3].pop()
    loose = type(mov)(**dict(vars(mov), metacell_df=mov.metacell_df.assign(members=members)))
    alone = same_amd.score_unpacked_maps(table, ref, loose, "distribute").loc[dropped]
    assert alone["metacell_row"] == -1 and not alone["matched"] and alone["pair"] == -1


@pytest.mark.parametrize("distinct", [True, False])
def test_ranks_against_the_luad_notebook_cell(distinct):
    """cell 13: the moving cell's label among the k largest type columns of the reference cell (np.argpartition) -- `rank_weak < k` where no
    tie decides, and between `rank_weak < k` and `rank_strict < k` where one does"""
    import same_amd

    ref, mov, table = _typed_objects(distinct)
    got = same_amd.score_unpacked_maps(table, ref, mov, "distribute", commonCT=COLS, ranks=True)
    assert list(got.columns[-3:]) == ["rank_strict", "rank_weak", "ranked"] and got["rank_weak"].dtype == np.uint8
    expanded = _unpacked(table, ref, mov)
    dom_types = expanded["Aligned_cell_id"].map(mov.original_df.set_index("Cell_Num_Old")["cell_type"]).to_numpy()
    ref_rows = ref.original_df.set_index("Cell_Num_Old").loc[expanded["Ref_cell_id"].to_numpy(), COLS].to_numpy()
    ct_array = np.array(COLS)
    m = got.loc[expanded["Aligned_cell_id"].to_numpy()]
    assert m["ranked"].all() and m["matched"].all()
    tied = 0
    for k in (1, 2, 3):
        top_k_idx = np.argpartition(ref_rows, -k, axis=1)[:, -k:]
        hits = np.any(ct_array[top_k_idx] == dom_types[:, None], axis=1)
        sure, may = (m["rank_weak"] < k).to_numpy(), (m["rank_strict"] < k).to_numpy()
        assert (sure <= hits).all() and (hits <= may).all(), k
        if distinct:
            assert np.array_equal(sure, may) and np.array_equal(hits, sure)
        tied += int((sure != may).sum())
    assert (m["rank_weak"] < 3).all() and (tied > 0) == (not distinct)
    assert 0 < (m["rank_weak"] < 1).sum() < len(m)
    # a label that names no column, a NaN in the type row: not ranked
    mov.original_df.loc[mov.original_df.index[::6], "cell_type"] = "z"
    ref.original_df.loc[ref.original_df.index[::5], "b"] = np.nan
    holes = same_amd.score_unpacked_maps(table, ref, mov, "distribute", commonCT=COLS, ranks=True)
    no_column = (mov.original_df["cell_type"] == "z").to_numpy()
    nan_row = ref.original_df["b"].isna().to_numpy()[np.maximum(holes["ref_cell_row"].to_numpy(), 0)] & holes["matched"].to_numpy()
    assert np.array_equal(holes["ranked"].to_numpy(), holes["matched"].to_numpy() & ~no_column & ~nan_row) and nan_row.any()
    assert (holes["rank_strict"][~holes["ranked"]] == 255).all() and (holes["rank_weak"][holes["ranked"]] < 3).all()


def test_cell_truth_as_dict_series_and_array():
    import same_amd

    ref, mov, table = _typed_objects()
    base = same_amd.score_unpacked_maps(table, ref, mov, "distribute")
    ids_m = mov.original_df["Cell_Num_Old"].to_numpy()
    want_id = base["ref_id"].to_numpy(dtype=object).copy()
    want_id[::3] = None                                                 # unknown
    want_id[1::3] = int(ref.original_df["Cell_Num_Old"].iloc[5])        # known, and wrong for all but the cells put on that cell
    as_dict = {int(a): int(b) for a, b in zip(ids_m, want_id) if not pd.isna(b)}
    as_series = pd.Series(want_id, index=mov.original_df.index)
    frames = [same_amd.score_unpacked_maps(table, ref, mov, "distribute", cell_truth=t) for t in (as_dict, as_series, want_id)]
    for f in frames[1:]:
        pd.testing.assert_frame_equal(f, frames[0], check_exact=True)
    f = frames[0]
    assert list(f.columns[-2:]) == ["truth_known", "on_truth"]
    assert f["truth_known"].tolist() == [not pd.isna(b) for b in want_id]
    assert f["on_truth"].tolist() == [bool(m) and not pd.isna(b) and int(r) == int(b) for m, r, b in zip(f["matched"], base["ref_id"], want_id)]
    assert 0 < f["on_truth"].sum() < (f["matched"] & f["truth_known"]).sum()
    # the objects may name their id columns differently
    renamed = type(ref)(**dict(vars(ref), original_df=ref.original_df.rename(columns={"Cell_Num_Old": "rna_id"}), original_idx_col="rna_id"))
    other = same_amd.score_unpacked_maps(table, renamed, mov, "distribute", cell_truth=as_dict)
    pd.testing.assert_frame_equal(other, f, check_exact=True)
    tally = same_amd.score_maps.cell_tally_from_cells([f, base], f.index)
    assert list(tally.columns) == ["results", "matched_in", "type_match_in", "on_truth_in"] and tally["results"].eq(2).all()
    assert np.array_equal(tally["matched_in"], 2 * f["matched"].astype(np.int64)) and np.array_equal(tally["on_truth_in"], f["on_truth"].astype(np.int64))
    with pytest.raises(ValueError, match="not in the reference frame's 'Cell_Num_Old'"):
        same_amd.score_unpacked_maps(table, ref, mov, "distribute", cell_truth={7: 5})
    with pytest.raises(ValueError, match="pass commonCT"):
        same_amd.score_unpacked_maps(table, ref, mov, "distribute", ranks=True)


def test_every_argument_is_checked_before_a_job_or_a_device_is_touched(monkeypatch):
    import same_amd
    from same_amd import _lib, window_api

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(window_api, "_WindowJob", lambda *a, **k: pytest.fail("a job was made"))
    ref, mov, _table = _typed_objects()
    for df in (ref.metacell_df, mov.metacell_df):
        df["cell_type"] = "a"
    call = lambda *a, **kw: same_amd.sliding_window_score_maps(*(a or (ref, mov, COLS)), **kw)
    for bad in ("closest", "Nearest", 1, True):
        with pytest.raises(ValueError, match="unpack must be None or one of"):
            call(unpack=bad)
    with pytest.raises(ValueError, match="cell_truth names the true reference CELLS"):
        call(cell_truth={7: 1000})
    with pytest.raises(ValueError, match="pass commonCT"):
        call(ref, mov, None, unpack="nearest", ranks=True)
    bare = type(ref)(**dict(vars(ref), original_df=ref.original_df.drop(columns=["b", "c"])))
    with pytest.raises(ValueError, match=r"ref.original_df has no \['b', 'c'\]"):
        call(bare, mov, COLS, unpack="nearest", ranks=True)
    with pytest.raises(ValueError, match="not in the reference frame's 'Cell_Num_Old'"):
        call(unpack="distribute", cell_truth={7: 5})
    with pytest.raises(ValueError, match="cell_truth|truth has 3 values"):
        call(unpack="distribute", cell_truth=[1000, 1003, 1006])
    with pytest.raises(ValueError, match="truth must be a Series"):
        call(unpack="distribute", cell_truth="1000")
    no_lists = type(ref)(**dict(vars(ref), metacell_df=ref.metacell_df.drop(columns="members")))
    with pytest.raises(ValueError, match="ref.metacell_df has no 'members' column of lists"):
        call(no_lists, mov, COLS, unpack="distribute")
    with pytest.raises(ValueError, match="score_params"):
        call(unpack="distribute", score_params={"nodes": 1})


def test_plain_frames_are_refused_with_an_error_that_is_both(monkeypatch):
    """callers are told ValueError, as for every refusal; tests/test_score_maps_cpu.py still expects the TypeError the call raised for
    the keyword before it had it -- and it fires before any other check can"""
    import same_amd
    from same_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    ref, mov, _table = _typed_objects()
    for frames in ((ref.metacell_df, mov.metacell_df), (ref, mov.metacell_df), (ref.metacell_df, mov)):
        for expected in (TypeError, ValueError):
            with pytest.raises(expected, match="unpack='nearest' reads MetaCell objects on both sides"):
                # (ranks without commonCT, a cell_truth naming nothing: the refusal comes first)
                same_amd.sliding_window_score_maps(*frames, None, unpack="nearest", ranks=True, cell_truth={7: 5})


def test_the_abi_surface_and_the_exports():
    """additions do not bump the version; the five entry points are declared, bound and exported"""
    import same_amd
    from same_amd import _lib, windows

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert re.search(r"^#define SAME_ABI_VERSION 9$", header, re.M) and _lib.ABI_VERSION == 9
    lib = _lib.load()
    for name in ("same_unpack_map_create", "same_unpack_map_destroy", "same_unpack_map_tally", "same_unpack_map_reset",
                 "same_merge_acc_unpack_map"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(rf"\b{name}\(", header), name
    assert "same_member_mark" in header and windows.MEMBER_MARK.itemsize == 16
    assert windows.MEMBER_MARK.names == ("ref_member", "ref_row", "pair", "flags", "rank_strict", "rank_weak", "reserved")
    for name in ("CellScoreMaps", "score_unpacked_maps"):
        assert name in same_amd.__all__ and hasattr(same_amd, name)
    assert same_amd.CellScoreMaps._fields == ("scores", "cells", "tally", "cell_cells", "cell_tally")
    for name in ("DeviceUnpackMap",):
        assert hasattr(windows, name) and hasattr(windows.MergeAccumulator, "unpack_map")
