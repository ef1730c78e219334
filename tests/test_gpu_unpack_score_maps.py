"""`same_amd.sliding_window_score_maps(unpack=...)` as a product: every per-CELL frame the device marks from a result's unpacked pairs
(csrc/window_unpack_map.hip) equals `score_unpacked_maps` of that result's table -- `unpack_metacell_matches`, the two label maps and
`label_ranks` --; the cell tally is the sum of the frames; `scores`' cell keys are `sliding_window_scores(unpack=)`'s; the first three
fields are the call's own without `unpack`; what the device does not unpack or rank comes back the same through the tables.  Every
comparison is exact."""
import copy

import numpy as np
import pandas as pd
import pytest

from test_gpu_scores import MC_OP
from test_gpu_unpack_scores import CELL_KEYS, SETS, _changed, _objects
from test_gpu_window_variants import _variants_of

pytestmark = pytest.mark.gpu

SETS3 = SETS + [{"knn": 4}]
CELL_TRUTH_KEYS = ("cell_truth_rows", "cell_truth_matches", "cell_truth_accuracy")


@pytest.fixture
def calls(monkeypatch):
    """the strategies of the cell-level map calls, in order"""
    from same_amd import windows as W

    seen, inner = [], W.MergeAccumulator.unpack_map

    def counted(self, *a, **kw):
        seen.append(a[2])
        return inner(self, *a, **kw)

    monkeypatch.setattr(W.MergeAccumulator, "unpack_map", counted)
    return seen


def _not_on_the_device(monkeypatch):
    from same_amd import windows as W

    monkeypatch.setattr(W.MergeAccumulator, "unpack_map", lambda *a, **k: (_ for _ in ()).throw(AssertionError("mapped on the device")))


def _truth_of(mc_ref, mc_mov, met=None, seed=3):
    """a cell truth by hand, as a dict: per original moving cell a reference cell's id drawn at random, a third of them unknown; `met`:
    an unpacked table (`sliding_window_scores(tables=True, unpack=)`'s) whose every second pair is taken as the truth, so that results meet
    some of it"""
    rng = np.random.default_rng(seed)
    ids_m, ids_r = mc_mov.original_df["Cell_Num_Old"].to_numpy(), mc_ref.original_df["Cell_Num_Old"].to_numpy()
    truth = {int(a): int(b) for a, b, u in zip(ids_m, rng.choice(ids_r, len(ids_m)), rng.random(len(ids_m))) if u > 0.33}
    if met is not None:
        truth.update({int(a): int(b) for a, b in zip(met["Aligned_cell_id"].to_numpy()[::2], met["Ref_cell_id"].to_numpy()[::2])})
    return truth


def _tally_of(frames):
    flat = [c for per_set in frames for c in per_set]
    total = lambda col: sum(c[col].to_numpy().astype(np.int64) for c in flat)
    return pd.DataFrame({"results": np.full(len(flat[0]), len(flat), np.int64), "matched_in": total("matched"), "type_match_in": total("type_match"),
                         "on_truth_in": total("on_truth") if "on_truth" in flat[0].columns else np.zeros(len(flat[0]), np.int64)},
                        index=flat[0].index)


def _held_against_the_host(got, mc_ref, mc_mov, cols, strategy, kw, cell_truth, ranks, tag, all_ranked=True):
    """every cell frame == score_unpacked_maps of the result's table; the tally their sum; the cell keys sliding_window_scores(unpack=)'s"""
    import same_amd

    assert isinstance(got, same_amd.CellScoreMaps)
    scores, tables, cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, tables=True, **kw)
    pd.testing.assert_frame_equal(got.scores[list(scores.columns)], scores, check_exact=True)
    n_cells = len(mc_mov.original_df)
    for v, per_set in enumerate(tables):
        for s, table in enumerate(per_set):
            want = same_amd.score_unpacked_maps(table, mc_ref, mc_mov, strategy, commonCT=list(cols), cell_truth=cell_truth, ranks=ranks)
            g = got.cell_cells[v][s]
            pd.testing.assert_frame_equal(g, want, check_exact=True, obj=f"{tag} cell_cells[{v}][{s}]")
            assert len(g) == n_cells and g.index.name == "Cell_Num_Old" and g.index.equals(pd.Index(mc_mov.original_df["Cell_Num_Old"].to_numpy()))
            rec = scores.iloc[v * len(per_set) + s]
            assert g["matched"].sum() == rec["cells_matched"] and g["type_match"].sum() == rec["cell_type_matches"]
            assert 0 < g["type_match"].sum() < g["matched"].sum() <= n_cells, tag
            # the pair column names the unpacked table's rows, which name the cell and the reference cell
            m = g[g["matched"]]
            cells = cell_tables[v][s]
            assert np.array_equal(cells["Aligned_cell_id"].to_numpy()[m["pair"].to_numpy()], m.index.to_numpy())
            assert np.array_equal(cells["Ref_cell_id"].to_numpy()[m["pair"].to_numpy()], m["ref_id"].to_numpy(dtype=np.int64))
            assert sorted(m["pair"].tolist()) == list(range(len(cells)))
            assert np.array_equal(mc_ref.original_df["Cell_Num_Old"].to_numpy()[m["ref_cell_row"].to_numpy()], m["ref_id"].to_numpy(dtype=np.int64))
            by_meta = dict(zip(table["Aligned_metacell_id"].tolist(), table["Ref_metacell_id"].tolist()))
            assert [by_meta[a] for a in m["metacell_row"].tolist()] == m["ref_metacell_row"].tolist()
            if ranks and all_ranked:
                assert m["ranked"].all() and (m["rank_strict"] <= m["rank_weak"]).all() and (g["rank_weak"][~g["matched"]] == 255).all()
    if got.cell_tally is not None:
        pd.testing.assert_frame_equal(got.cell_tally, _tally_of(got.cell_cells), check_exact=True, obj=f"{tag} cell_tally")
    return scores, tables


@pytest.mark.parametrize("strategy", ["distribute", "nearest"])
def test_cell_frames_equal_the_host_statement_and_the_first_fields_do_not_move(calls, strategy):
    import same_amd

    mc_ref, mc_mov, cols = _objects("5 against 4")
    variants = _variants_of(mc_mov.metacell_df, cols)[:2]
    kw = dict(type_variants=variants, param_sets=SETS3, optim_params=dict(MC_OP))
    met = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, tables=True, **kw)[2][0][0]
    truth = _truth_of(mc_ref, mc_mov, met)
    got = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), unpack=strategy, cell_truth=truth, ranks=True, **kw)
    assert calls == [strategy] * 6                                      # ONE call per result in the unpack call's place
    scores, _tables = _held_against_the_host(got, mc_ref, mc_mov, cols, strategy, kw, truth, True, strategy)
    assert list(got.scores.columns[-6:]) == list(CELL_KEYS) + list(CELL_TRUTH_KEYS)
    flat = [c for per_set in got.cell_cells for c in per_set]
    for q, c in enumerate(flat):
        rec = got.scores.iloc[q]
        assert rec["cell_truth_rows"] == (c["matched"] & c["truth_known"]).sum() and rec["cell_truth_matches"] == c["on_truth"].sum()
        assert 0 < rec["cell_truth_matches"] < rec["cell_truth_rows"] < rec["cells_matched"]
        assert rec["cell_truth_accuracy"] == 100 * (int(rec["cell_truth_matches"]) / int(rec["cell_truth_rows"]))
        assert c["truth_known"].sum() == len(truth)
    assert any(not a.equals(b) for a, b in zip(flat, flat[1:]))
    assert got.cell_tally["results"].eq(6).all() and got.cell_tally["matched_in"].max() == 6 and got.cell_tally["on_truth_in"].max() > 0
    # the first three fields: the call without `unpack`, but for the added cell keys
    del calls[:]
    plain = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), ranks=True, **kw)
    assert isinstance(plain, same_amd.ScoreMaps) and not isinstance(plain, same_amd.CellScoreMaps) and calls == []
    pd.testing.assert_frame_equal(got.scores[list(plain.scores.columns)], plain.scores, check_exact=True)
    pd.testing.assert_frame_equal(got.tally, plain.tally, check_exact=True)
    for per_set, want in zip(got.cells, plain.cells):
        for c, w in zip(per_set, want):
            pd.testing.assert_frame_equal(c, w, check_exact=True)


def test_cell_truth_as_dict_series_and_array_and_a_baseline_study(calls):
    import same_amd

    mc_ref, mc_mov, cols = _objects("ms3")
    kw = dict(param_sets=SETS, optim_params=dict(MC_OP))
    first = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), unpack="nearest", **kw)
    assert "truth_known" not in first.cell_cells[0][0].columns and not first.cell_tally["on_truth_in"].any()
    assert not any(k in first.scores.columns for k in CELL_TRUTH_KEYS)
    base = first.cell_cells[0][0]["ref_id"]                            # set 0's reference cell per moving cell: the baseline
    assert base.isna().any() and base.notna().sum() == first.scores["cells_matched"].iloc[0]
    as_dict = {int(a): int(b) for a, b in base.dropna().items()}
    as_series = pd.Series(base.to_numpy(), index=mc_mov.original_df.index)
    as_array = base.to_numpy()
    runs = [same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), unpack="nearest", cell_truth=t, **kw) for t in (as_dict, as_series, as_array)]
    assert calls == ["nearest"] * 8
    for run in runs[1:]:
        pd.testing.assert_frame_equal(run.scores, runs[0].scores, check_exact=True)
        pd.testing.assert_frame_equal(run.cell_tally, runs[0].cell_tally, check_exact=True)
        for a, b in zip(run.cell_cells[0], runs[0].cell_cells[0]):
            pd.testing.assert_frame_equal(a, b, check_exact=True)
    _held_against_the_host(runs[0], mc_ref, mc_mov, cols, "nearest", kw, as_dict, False, "baseline")
    c0, c1 = runs[0].cell_cells[0]
    assert c0["on_truth"].equals(c0["matched"]) and c0["truth_known"].equals(c0["matched"])      # set 0 against itself: every match on its truth
    assert runs[0].scores["cell_truth_accuracy"].iloc[0] == 100.0 and runs[0].scores["cell_truth_rows"].iloc[0] == c0["matched"].sum()
    assert 0 < c1["on_truth"].sum() < (c1["matched"] & c1["truth_known"]).sum()                 # another set moved some cells
    assert runs[0].scores["cell_truth_matches"].iloc[1] == c1["on_truth"].sum()


def test_per_result_false_and_tally_false(calls):
    import same_amd

    mc_ref, mc_mov, cols = _objects("ms3")
    kw = dict(param_sets=SETS, optim_params=dict(MC_OP), unpack="distribute", cell_truth=_truth_of(mc_ref, mc_mov))
    full = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), **kw)
    no_frames = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), per_result=False, **kw)
    no_tally = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), tally=False, **kw)
    assert calls == ["distribute"] * 6
    assert no_frames.cell_cells is None and no_frames.cells is None and no_tally.cell_tally is None and no_tally.tally is None
    pd.testing.assert_frame_equal(no_frames.cell_tally, full.cell_tally, check_exact=True)
    pd.testing.assert_frame_equal(no_frames.scores, full.scores, check_exact=True)
    pd.testing.assert_frame_equal(no_tally.scores, full.scores, check_exact=True)
    for a, b in zip(no_tally.cell_cells[0], full.cell_cells[0]):
        pd.testing.assert_frame_equal(a, b, check_exact=True)
    pd.testing.assert_frame_equal(full.cell_tally, _tally_of(full.cell_cells), check_exact=True)


@pytest.mark.parametrize("why", ["permuted metacell ids", "65 cell labels", "a truth cell in no list"])
def test_what_the_device_does_not_map_comes_back_the_same_through_the_tables(monkeypatch, why):
    import same_amd

    _not_on_the_device(monkeypatch)
    mc_ref, mc_mov, cols = _objects("ms3")
    truth = _truth_of(mc_ref, mc_mov)
    if why == "permuted metacell ids":
        ids = mc_ref.metacell_df[mc_ref.metacell_idx_col].to_numpy().copy()
        ids[[3, 11]] = ids[[11, 3]]
        mc_ref = _changed(mc_ref, ids=ids)
    elif why == "65 cell labels":
        mc_mov = copy.copy(mc_mov)
        mc_mov.original_df = mc_mov.original_df.copy()
        labels = mc_mov.original_df["cell_type"].to_numpy().astype(object)
        labels[5::17] = [f"rare{q % 62}" for q in range(len(labels[5::17]))]
        mc_mov.original_df["cell_type"] = labels
        assert len(set(labels) | set(mc_ref.original_df["cell_type"])) == 65
    else:
        members = [list(m) for m in mc_ref.metacell_df["members"]]
        q = next(q for q, m in enumerate(members) if len(m) > 1)
        lost = members[q].pop()                                        # a reference cell no metacell lists, which a truth names
        mc_ref = _changed(mc_ref, members=members)
        truth[int(mc_mov.original_df["Cell_Num_Old"].iloc[0])] = int(lost)
    kw = dict(param_sets=SETS, optim_params=dict(MC_OP))
    got = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), unpack="nearest", cell_truth=truth, ranks=True, **kw)
    _held_against_the_host(got, mc_ref, mc_mov, cols, "nearest", kw, truth, True, why, all_ranked=why != "65 cell labels")
    if why == "65 cell labels":
        c = got.cell_cells[0][0]
        assert (c["matched"] & ~c["ranked"]).any() and c["ranked"].any()      # a rare label names no column


def test_non_finite_member_coordinates_under_nearest():
    """the reference's own error from the device's flag, as sliding_window_scores(unpack=) raises it; 'distribute' does not read them"""
    import same_amd

    mc_ref, mc_mov, cols = _objects("ms3")
    bad = copy.copy(mc_mov)
    bad.original_df = mc_mov.original_df.copy()
    bad.original_df["X"] = np.nan
    kw = dict(param_sets=SETS[:1], optim_params=dict(MC_OP))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        same_amd.sliding_window_score_maps(mc_ref, bad, list(cols), unpack="nearest", **kw)
    got = same_amd.sliding_window_score_maps(mc_ref, bad, list(cols), unpack="distribute", **kw)
    want = same_amd.sliding_window_score_maps(mc_ref, mc_mov, list(cols), unpack="distribute", **kw)
    pd.testing.assert_frame_equal(got.scores, want.scores, check_exact=True)
    pd.testing.assert_frame_equal(got.cell_cells[0][0], want.cell_cells[0][0], check_exact=True)
    pd.testing.assert_frame_equal(got.cell_tally, want.cell_tally, check_exact=True)
