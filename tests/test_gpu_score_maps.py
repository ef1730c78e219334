"""same_amd.sliding_window_score_maps as a product: every per-cell frame the device marks from a result's merged rows equals
`score_table_maps` of that result's table -- the host statement, made of check_triangle_violations' own column, ops.tri_flip_stats'
node counters, a comparison of labels and `label_ranks` --, frame for frame and exactly; `scores` is sliding_window_scores' frame; the
tally is the sum over the frames.  Every test here fails without the feature: same_amd has no sliding_window_score_maps."""
import numpy as np
import pandas as pd
import pytest

from test_gpu_scores import CID, MC_OP, OP, SETS, _frames, _plain_tris
from test_gpu_window_variants import _variants_of

pytestmark = pytest.mark.gpu

TALLY = {"matched_in": "matched", "type_match_in": "type_match", "violating_in": "in_violating_triangle", "on_truth_in": "on_truth"}


def _study(ref, mov, cols, op, *, cid=CID, truth=None, host_truth="same", ranks=True, variants=None, sets=None, score_delaunay=None,
           host_delaunay="same", score_params=None, frame=None):
    """sliding_window_score_maps against sliding_window_scores(tables=True) + score_table_maps per table -> (the maps, the host's frames)"""
    import same_amd

    kw = dict(type_variants=variants, param_sets=sets, optim_params=dict(op), score_delaunay=score_delaunay, score_params=score_params)
    maps = same_amd.sliding_window_score_maps(ref, mov, list(cols), truth=truth, ranks=ranks, **kw)
    scores, tables = same_amd.sliding_window_scores(ref, mov, list(cols), tables=True, **kw)
    n_v, n_s = len(variants or [None]), len(sets or [{}])
    assert isinstance(maps, same_amd.ScoreMaps) and len(maps.cells) == n_v and all(len(c) == n_s for c in maps.cells)
    pd.testing.assert_frame_equal(maps.scores[scores.columns], scores, check_exact=True)
    frame = mov if frame is None else frame
    host_tri = score_delaunay if isinstance(host_delaunay, str) else host_delaunay
    host = [[same_amd.score_table_maps(t, ref, mov, cell_id_col=cid, commonCT=list(cols), truth=truth if isinstance(host_truth, str) else host_truth,
                                       ranks=ranks, score_delaunay=host_tri, score_params=score_params) for t in per_set] for per_set in tables]
    for v in range(n_v):
        for s in range(n_s):
            got, want = maps.cells[v][s], host[v][s]
            assert got.index.equals(frame.index) and len(got) == len(frame)
            pd.testing.assert_frame_equal(got, want, check_exact=True, obj=f"cells[{v}][{s}]")
            ref_ids = getattr(ref, "metacell_df", ref)[cid].to_numpy()
            assert np.array_equal(got["ref_id"][got["matched"]].to_numpy(), ref_ids[got["ref_row"][got["matched"]]])
    flat = [c for per_set in maps.cells for c in per_set]
    assert maps.tally.index.equals(frame.index) and (maps.tally["results"] == len(flat)).all()
    for k, col in TALLY.items():
        want = sum((c[col].to_numpy().astype(np.int64) for c in flat if col in c.columns), np.zeros(len(frame), np.int64))
        assert maps.tally[k].dtype == np.int64 and np.array_equal(maps.tally[k].to_numpy(), want), k
    if truth is not None:
        for q, c in enumerate(flat):
            rows, hits = int((c["matched"] & c["truth_known"]).sum()), int(c["on_truth"].sum())
            assert (maps.scores["truth_rows"].iloc[q], maps.scores["truth_matches"].iloc[q]) == (rows, hits)
            assert maps.scores["truth_accuracy"].iloc[q] == 100 * (hits / rows)
    lean = same_amd.sliding_window_score_maps(ref, mov, list(cols), truth=truth, ranks=ranks, per_result=False, **kw)
    assert lean.cells is None
    pd.testing.assert_frame_equal(lean.scores, maps.scores, check_exact=True)
    pd.testing.assert_frame_equal(lean.tally, maps.tally, check_exact=True)
    return maps, host


def _baseline(ref, mov, cols, op, cid, **kw):
    """a truth for the study: the first result of a study without one (its `ref_id` per moving row), one row in five forgotten"""
    import same_amd

    first = same_amd.sliding_window_score_maps(ref, mov, list(cols), optim_params=dict(op), tally=False, **kw).cells[0][0]
    truth = first["ref_id"].copy()
    truth.iloc[::5] = pd.NA
    return truth


def test_the_cells_of_a_study_equal_the_host_statement_of_their_tables():
    ref, mov, cols = _frames()
    variants = _variants_of(mov, cols)[:2]
    maps, _host = _study(ref, mov, cols, OP, variants=variants, sets=SETS[:2], score_delaunay=_plain_tris())
    flat = [c for per_set in maps.cells for c in per_set]
    assert len(flat) == 4 and list(flat[0].columns) == ["ref_row", "ref_id", "matched", "type_match", "node_triangles", "node_flips", "considered",
                                                        "in_violating_triangle", "rank_strict", "rank_weak", "ranked"]
    for c in flat:                                  # not vacuous: every column has both values
        assert 0 < c["matched"].sum() < len(c) and 0 < c["type_match"].sum() < c["matched"].sum()
        assert 0 < c["in_violating_triangle"].sum() < c["considered"].sum() <= c["matched"].sum()
        assert 0 < c["ranked"].sum() and not (c["ranked"] & ~c["matched"]).any() and (c["rank_strict"][~c["ranked"]] == 255).all()
        assert (c["rank_weak"][c["ranked"]] == 0).sum() > 0 and (c["rank_weak"][c["ranked"]] > 0).sum() > 0
    assert any(not a.equals(b) for a, b in zip(flat, flat[1:]))
    assert (maps.tally["matched_in"] == 4).any() and (maps.tally["matched_in"] < 4).any()


@pytest.mark.parametrize("how", ["series", "dict", "array"])
def test_truth_as_a_series_a_dict_and_an_array(how):
    ref, mov, cols = _frames()
    base = _baseline(ref, mov, cols, OP, CID)
    assert base.index.equals(mov.index) and base.isna().sum() >= len(mov) // 5
    if how == "series":
        truth = base.sample(frac=1.0, random_state=3)                        # aligned by label, not by position
    elif how == "dict":
        truth = {m: r for m, r in zip(mov[CID].tolist(), base.tolist()) if not pd.isna(r)}
    else:
        truth = base.to_numpy(dtype=object)
    maps, _host = _study(ref, mov, cols, OP, truth=truth, host_truth=base, ranks=False, sets=SETS[:2], score_delaunay=_plain_tris())
    first, second = maps.cells[0]
    assert list(first.columns)[-2:] == ["truth_known", "on_truth"] and np.array_equal(first["truth_known"].to_numpy(), base.notna().to_numpy())
    assert np.array_equal(first["on_truth"].to_numpy(), (first["matched"] & first["truth_known"]).to_numpy())   # the baseline IS the first set's result
    assert 0 < second["on_truth"].sum() < (second["matched"] & second["truth_known"]).sum()
    assert maps.scores["truth_accuracy"].iloc[0] == 100.0 > maps.scores["truth_accuracy"].iloc[1] > 0


def test_metacell_objects_on_the_device_route():
    from test_gpu_caller_triangulation import _metacells

    ref, mc, cols = _metacells("ms3")
    cid = mc.metacell_idx_col
    base = _baseline(ref, mc, cols, MC_OP, cid)
    variants = _variants_of(mc.metacell_df, cols)[:2]
    maps, _host = _study(ref, mc, cols, MC_OP, cid=cid, truth=base, variants=variants, sets=SETS[:2], host_delaunay=mc.metacell_delaunay,
                         frame=mc.metacell_df)
    for c in (c for per_set in maps.cells for c in per_set):
        assert c["in_violating_triangle"].sum() > 0 and 0 < c["on_truth"].sum()


@pytest.mark.parametrize("why", ["duplicate cell ids", "a missing cell_type label"])
def test_inputs_the_device_refuses_give_the_same_frames_through_the_host_path(why, monkeypatch):
    from same_amd import windows as W

    ref, mov, cols = _frames()
    mov = mov.copy()
    if why == "duplicate cell ids":
        ids = mov[CID].to_numpy().copy()
        ids[7] = ids[3]
        mov[CID] = ids
    else:
        labels = mov["cell_type"].to_numpy().astype(object)
        labels[11] = None
        mov["cell_type"] = labels
    made = []
    monkeypatch.setattr(W.MergeAccumulator, "score_map", lambda *a, **k: made.append(1))
    truth = np.where(np.arange(len(mov)) % 4 == 0, None, ref[CID].to_numpy()[np.arange(len(mov)) % len(ref)].astype(object))
    maps, _host = _study(ref, mov, cols, OP, truth=truth, sets=SETS[:2], score_delaunay=_plain_tris())
    assert not made and maps.cells[0][0]["matched"].sum() > 0                          # the map call was never made


def test_in_violating_triangle_is_the_references_recorded_column_on_the_golden_inputs():
    """tests/golden/eval_tri.npz: duplicate ids, a NaN coordinate, a triangle that names an unknown id -- under every recorded rule"""
    import same_amd
    import score_map_check as M
    from test_oracle_golden import EVAL_CASES, load_golden

    g = load_golden("eval_tri")
    table, ref, moving, tri, cid, rows = M.golden_eval_study(g)
    for tag, kw in EVAL_CASES:
        cells = same_amd.score_table_maps(table, ref, moving, cell_id_col=cid, score_delaunay=tri, score_delaunay_vertex_col=cid, score_params=kw)
        got = cells["in_violating_triangle"].to_numpy()[rows].astype(np.uint8)
        assert np.array_equal(got, g[f"viol_{tag}"]), (tag, int(got.sum()), int(g[f"viol_{tag}"].sum()))
        assert int(got.sum()) == int(g[f"stats_{tag}"][6])                      # nodes_in_violating_triangles, per table row
        assert (cells["considered"] | ~cells["in_violating_triangle"]).all() and cells["matched"].sum() == len(np.unique(rows))
