"""`same_amd.sliding_window_score_details(unpack=...)` as a product: every cell-level frame the device bins from a result's unpacked pairs
(csrc/window_unpack_detail.hip) equals `score_unpacked_details` of that result's table -- `unpack_metacell_matches`, np.bincount over
the joint label codes and `top_k_counts` --, the notebook cells of examples/luad/reproduce_figures.ipynb written out here as well; the
first five fields are `sliding_window_score_details`' own; what the device does not unpack or bin comes back the same through the
tables.  Every comparison is exact."""
import copy

import numpy as np
import pandas as pd
import pytest

from test_gpu_score_details import _regions, _rows_of
from test_gpu_scores import MC_OP
from test_gpu_unpack_scores import CELL_KEYS, SETS, _changed, _notebook_cell, _objects

pytestmark = pytest.mark.gpu

TOP_K = (1, 2, 3)
CELL_FIELDS = ("cell_confusion", "cell_groups", "cell_cross", "cell_top_k")


@pytest.fixture
def calls(monkeypatch):
    """which of the two unpack calls ran, in order"""
    from same_amd import windows as W

    seen = []
    for name in ("unpack", "unpack_detail"):
        def counted(self, *a, _inner=getattr(W.MergeAccumulator, name), _name=name, **kw):
            seen.append(_name)
            return _inner(self, *a, **kw)

        monkeypatch.setattr(W.MergeAccumulator, name, counted)
    return seen


def _no_tables(mp):
    from same_amd import incumbent
    from same_amd import windows as W

    refuse = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a table was built"))
    mp.setattr(W.MergeAccumulator, "columns", refuse)
    mp.setattr(W.MergeAccumulator, "final_rows", refuse)
    mp.setattr(incumbent._TableBuilder, "gather", refuse)
    mp.setattr(incumbent._TableBuilder, "table_from_device", refuse)


def _same_cell_frames(got, want, s, tag):
    eq = lambda a, b, what: pd.testing.assert_frame_equal(a, b, check_exact=True, obj=f"{tag} set {s} {what}")
    eq(got.cell_confusion.loc[(0, s)], want.cell_confusion, "cell_confusion")
    for what in CELL_FIELDS[1:]:
        g, w = getattr(got, what), getattr(want, what)
        assert (g is None) == (w is None), (tag, what)
        if w is not None:
            eq(_rows_of(g, 0, s), w, what)


def _held_against_the_host(got, mc_ref, mc_mov, cols, strategy, regions, op, tag):
    """every cell frame == score_unpacked_details of the result's table == the notebook's cells 12 and 13; .scores is
    sliding_window_scores(unpack=)'s frame"""
    import same_amd

    assert isinstance(got, same_amd.CellScoreDetails)
    scores, tables, _cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, param_sets=SETS,
                                                                  optim_params=dict(op), tables=True)
    pd.testing.assert_frame_equal(got.scores, scores, check_exact=True)
    assert list(got.scores.columns[-3:]) == list(CELL_KEYS)
    for s, table in enumerate(tables[0]):
        want = same_amd.score_unpacked_details(table, mc_ref, mc_mov, strategy, commonCT=list(cols), group_by=regions, top_k=TOP_K)
        _same_cell_frames(got, want, s, tag)
        n, k, accuracy, cells = _notebook_cell(table, mc_ref, mc_mov, strategy)
        groups, cross, top = _rows_of(got.cell_groups, 0, s), _rows_of(got.cell_cross, 0, s), _rows_of(got.cell_top_k, 0, s).iloc[0]
        assert groups["cells_matched"].sum() + cross["cells_matched"].iloc[0] == n == got.cell_confusion.loc[(0, s)].to_numpy().sum()
        assert groups["cell_type_matches"].sum() + cross["cell_type_matches"].iloc[0] == k
        assert k == np.trace(got.cell_confusion.loc[(0, s)].to_numpy()) and 0 < k < n
        assert (got.scores["cells_matched"].iloc[s], got.scores["cell_type_matches"].iloc[s], got.scores["cell_accuracy"].iloc[s]) == (n, k, accuracy)
        # cell 13: the moving cell's label among the k largest type columns of the reference cell (np.argpartition), where no tie decides
        aligned_ct = cells["Aligned_cell_id"].map(mc_mov.original_df.set_index("Cell_Num_Old")["cell_type"]).to_numpy()
        xen = mc_ref.original_df.set_index("Cell_Num_Old").loc[cells["Ref_cell_id"].to_numpy(), list(cols)].to_numpy()
        at = np.array([list(cols).index(v) for v in aligned_ct])
        for kk in TOP_K:
            hits = int((np.argpartition(-xen, kk - 1, axis=1)[:, :kk] == at[:, None]).any(axis=1).sum())
            assert top[f"top{kk}_matches"] <= hits <= top[f"top{kk}_matches"] + top[f"top{kk}_tied"], (tag, s, kk)
            if top[f"top{kk}_tied"] == 0:
                assert hits == top[f"top{kk}_matches"] and top[f"top{kk}_accuracy"] == 100 * (hits / n)
        assert top["typed_rows"] == n and top["top1_matches"] < top["top3_matches"] <= n
        assert cross["cells_matched"].iloc[0] > 0 and (groups["cell_type_matches"] < groups["cells_matched"]).all()
    return tables


@pytest.mark.parametrize("kind", ["ms3", "5 against 4"])
@pytest.mark.parametrize("strategy", ["distribute", "nearest"])
def test_cell_level_frames_equal_the_host_statement_and_the_notebook(monkeypatch, calls, strategy, kind):
    import same_amd

    mc_ref, mc_mov, cols = _objects(kind)
    regions = _regions(mc_mov.metacell_df, seed=8)
    kw = dict(group_by=regions, top_k=TOP_K, param_sets=SETS, optim_params=dict(MC_OP))
    with monkeypatch.context() as mp:
        _no_tables(mp)
        got = same_amd.sliding_window_score_details(mc_ref, mc_mov, list(cols), unpack=strategy, **kw)
    assert calls == ["unpack_detail"] * len(SETS)                      # ONE call per result in the unpack call's place, and no table
    _held_against_the_host(got, mc_ref, mc_mov, cols, strategy, regions, MC_OP, (kind, strategy))
    # the first five fields: the call without `unpack`, but for the added cell keys
    del calls[:]
    plain = same_amd.sliding_window_score_details(mc_ref, mc_mov, list(cols), **kw)
    assert isinstance(plain, same_amd.ScoreDetails) and not isinstance(plain, same_amd.CellScoreDetails) and calls == []
    pd.testing.assert_frame_equal(got.scores.drop(columns=list(CELL_KEYS)), plain.scores, check_exact=True)
    for what in ("confusion", "groups", "cross", "top_k"):
        pd.testing.assert_frame_equal(getattr(got, what), getattr(plain, what), check_exact=True, obj=what)
    # the cell level is another number than the metacell level's rank count
    assert got.cell_top_k["typed_rows"].tolist() != got.top_k["typed_rows"].tolist()
    # without group_by / top_k: None
    bare = same_amd.sliding_window_score_details(mc_ref, mc_mov, list(cols), unpack=strategy, param_sets=SETS[:1], optim_params=dict(MC_OP))
    assert bare.cell_groups is None and bare.cell_cross is None and bare.cell_top_k is None and bare.groups is None
    pd.testing.assert_frame_equal(bare.cell_confusion.loc[(0, 0)], got.cell_confusion.loc[(0, 0)], check_exact=True)


@pytest.mark.parametrize("why", ["permuted metacell ids", "a list of 65 members", "65 cell labels"])
def test_what_the_device_does_not_bin_comes_back_the_same_through_the_tables(monkeypatch, why):
    import same_amd
    from same_amd import windows as W

    monkeypatch.setattr(W.MergeAccumulator, "unpack_detail", lambda *a, **k: (_ for _ in ()).throw(AssertionError("binned on the device")))
    mc_ref, mc_mov, cols = _objects("ms3")
    if why == "permuted metacell ids":
        ids = mc_ref.metacell_df[mc_ref.metacell_idx_col].to_numpy().copy()
        ids[[3, 11]] = ids[[11, 3]]
        mc_ref = _changed(mc_ref, ids=ids)
    elif why == "a list of 65 members":
        members = [list(m) for m in mc_ref.metacell_df["members"]]
        members[5] = mc_ref.original_df["Cell_Num_Old"].to_numpy()[:65].tolist()
        mc_ref = _changed(mc_ref, members=members)
    else:
        mc_mov = copy.copy(mc_mov)
        mc_mov.original_df = mc_mov.original_df.copy()
        labels = mc_mov.original_df["cell_type"].to_numpy().astype(object)
        labels[5::17] = [f"rare{q % 62}" for q in range(len(labels[5::17]))]
        mc_mov.original_df["cell_type"] = labels
        assert len(set(labels) | set(mc_ref.original_df["cell_type"])) == 65
    regions = _regions(mc_mov.metacell_df, seed=8)
    got = same_amd.sliding_window_score_details(mc_ref, mc_mov, list(cols), unpack="nearest", group_by=regions, top_k=TOP_K, param_sets=SETS,
                                                optim_params=dict(MC_OP))
    scores, tables, _c = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack="nearest", param_sets=SETS,
                                                        optim_params=dict(MC_OP), tables=True)
    pd.testing.assert_frame_equal(got.scores, scores, check_exact=True)
    for s, table in enumerate(tables[0]):
        want = same_amd.score_unpacked_details(table, mc_ref, mc_mov, "nearest", commonCT=list(cols), group_by=regions, top_k=TOP_K)
        _same_cell_frames(got, want, s, why)
    if why == "65 cell labels":
        assert got.cell_confusion.shape[1] == 65 and (got.cell_top_k["typed_rows"] < got.scores["cells_matched"]).all()


def test_non_finite_member_coordinates_under_nearest():
    """the reference's own error from the device's flag, as sliding_window_scores(unpack=) raises it; 'distribute' does not read them"""
    import same_amd

    mc_ref, mc_mov, cols = _objects("ms3")
    bad = copy.copy(mc_mov)
    bad.original_df = mc_mov.original_df.copy()
    bad.original_df["X"] = np.nan
    kw = dict(param_sets=SETS[:1], optim_params=dict(MC_OP), top_k=TOP_K)
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        same_amd.sliding_window_score_details(mc_ref, bad, list(cols), unpack="nearest", **kw)
    got = same_amd.sliding_window_score_details(mc_ref, bad, list(cols), unpack="distribute", **kw)
    want = same_amd.sliding_window_score_details(mc_ref, mc_mov, list(cols), unpack="distribute", **kw)
    for what in ("scores",) + CELL_FIELDS[:1] + CELL_FIELDS[3:]:
        pd.testing.assert_frame_equal(getattr(got, what), getattr(want, what), check_exact=True, obj=what)
