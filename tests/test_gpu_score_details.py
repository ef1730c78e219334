"""same_amd.sliding_window_score_details as a product: every frame the device bins from a result's merged rows
(csrc/window_score_detail.hip) equals `score_table_details` of that result's table -- the host statement, made of
check_triangle_violations on the triangulation restricted to each group, a comparison of label codes and `top_k_counts` -- frame for
frame, integers exact and floats bit for bit; `.scores` is `sliding_window_scores`' frame; inputs the device refuses take the host route
to the same frames.  And, because check_triangle_violations' triangle kernel runs on the device, `score_table_details` WITH a
triangulation against the reference's recorded output (tests/golden/score_details.npz) and for additivity against `score_table`.
Every test here fails without the feature: same_amd has no sliding_window_score_details."""
import types

import numpy as np
import pandas as pd
import pytest

from test_gpu_scores import CID, MC_OP, OP, _frames, _simplices
from test_gpu_window_variants import _variants_of
from test_score_details_cpu import FLAGGED, QUADRANTS, _small_study, golden

pytestmark = pytest.mark.gpu

SETS = [{}, {"knn": 3, "hip_incumbent": "assignment"}]
TOP_K = (1, 2, 3)


def _regions(frame, seed=5):
    """four regions by the medians of X and Y, one row in thirteen without one"""
    rng = np.random.default_rng(seed)
    x, y = frame["X"].to_numpy(), frame["Y"].to_numpy()
    names = np.array(["sw", "se", "nw", "ne"], dtype=object)[(x > np.median(x)).astype(int) + 2 * (y > np.median(y)).astype(int)]
    names[rng.choice(len(frame), len(frame) // 13, replace=False)] = None
    return names


@pytest.fixture
def detail_calls(monkeypatch):
    """how often the detail call ran"""
    from same_amd import windows as W

    seen, inner = [], W.MergeAccumulator.score_detail

    def counted(self, *a, **kw):
        seen.append(1)
        return inner(self, *a, **kw)

    monkeypatch.setattr(W.MergeAccumulator, "score_detail", counted)
    return seen


def _rows_of(frame, v, s):
    return frame[(frame["variant"] == v) & (frame["set"] == s)].drop(columns=["variant", "set"]).reset_index(drop=True)


def _same_frames(got, want, v, s, tag):
    """the study's frames at (variant, set) against one table's ScoreDetails"""
    eq = lambda a, b, what: pd.testing.assert_frame_equal(a, b, check_exact=True, obj=f"{tag} variant {v} set {s} {what}")
    eq(_rows_of(got.scores, v, s), want.scores, "scores")
    eq(got.confusion.loc[(v, s)], want.confusion, "confusion")
    for what in ("groups", "cross", "top_k"):
        g, w = getattr(got, what), getattr(want, what)
        assert (g is None) == (w is None), (tag, what)
        if w is not None:
            eq(_rows_of(g, v, s), w, what)


def _study(ref, mov, cols, op, tag, *, cid=CID, variants=None, sets=None, group_by=None, score_delaunay=None, host_delaunay=None, **kw):
    """sliding_window_score_details against score_table_details of every table of sliding_window_variants(merge=True) -> the details"""
    import same_amd

    got = same_amd.sliding_window_score_details(ref, mov, list(cols), group_by=group_by, top_k=TOP_K, type_variants=variants, param_sets=sets,
                                                optim_params=dict(op), score_delaunay=score_delaunay, **kw)
    assert isinstance(got, same_amd.ScoreDetails)
    tables = same_amd.sliding_window_variants(ref, mov, [None] if variants is None else variants, list(cols), param_sets=sets,
                                              optim_params=dict(op), merge=True)
    tables = [[t] if sets is None else list(t) for t in tables]
    for v, per_set in enumerate(tables):
        for s, table in enumerate(per_set):
            want = same_amd.score_table_details(table, ref, mov, cell_id_col=cid, commonCT=list(cols), group_by=group_by, top_k=TOP_K,
                                                score_delaunay=score_delaunay if host_delaunay is None else host_delaunay, **kw)
            _same_frames(got, want, v, s, tag)
    return got


# ---- 1. the device's frames equal the host statement of every table ------------------------------------------------------------------------
@pytest.mark.parametrize("with_tris", [True, False], ids=["a score_delaunay", "no triangulation"])
def test_details_of_plain_frames_equal_the_host_statement_of_every_table(detail_calls, with_tris):
    import same_amd

    ref, mov, cols = _frames(1500, 3)
    mov = mov.assign(region=_regions(mov))
    variants = _variants_of(mov, cols)[:2]
    tris = _simplices(mov) if with_tris else None
    got = _study(ref, mov, cols, OP, "plain", variants=variants, sets=SETS, group_by="region", score_delaunay=tris)
    assert len(detail_calls) == 4                                     # one per (variant, set): the device route
    assert got.scores[["variant", "set"]].to_numpy().tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert got.groups["group"].tolist() == list(pd.unique(pd.Series(mov["region"]).dropna())) * 4 and len(got.cross) == len(got.top_k) == 4
    assert ("total_triangles" in got.groups.columns) == with_tris and "nodes_in_violating_triangles" not in got.cross.columns
    # not vacuous: rows without a group, wrong labels, ranked rows beyond the first place, and with triangles flips within and across
    assert (got.cross["matched"] > 0).all() and (got.groups["type_matches"] < got.groups["matched"]).all()
    off_diagonal = got.confusion.to_numpy().sum() - sum(np.trace(got.confusion.loc[(v, s)].to_numpy()) for v in (0, 1) for s in (0, 1))
    assert off_diagonal > 0 and (got.top_k["top1_matches"] < got.top_k["top3_matches"]).any() and (got.top_k["typed_rows"] > 0).all()
    if with_tris:
        assert (got.cross["total_triangles"] > 0).all() and got.groups["triangles_flipped"].sum() > 0
        assert got.groups["nodes_in_violating_triangles"].sum() > 0
        for v in (0, 1):
            for s in (0, 1):
                assert _rows_of(got.groups, v, s)["total_triangles"].sum() + _rows_of(got.cross, v, s)["total_triangles"].iloc[0] == len(tris)
    # .scores is sliding_window_scores' frame
    scores = same_amd.sliding_window_scores(ref, mov, list(cols), type_variants=variants, param_sets=SETS, optim_params=dict(OP),
                                            score_delaunay=tris)
    pd.testing.assert_frame_equal(got.scores, scores, check_exact=True)


def test_details_of_metacell_objects_equal_the_host_statement(detail_calls):
    """the job's own caller triangulation, an array as group_by, node-local scoring"""
    from test_gpu_caller_triangulation import _metacells

    ref, mc, cols = _metacells("ms3")
    regions = _regions(mc.metacell_df, seed=8)
    params = dict(node_local=True, majority_threshold=0.5)
    got = _study(ref, mc, cols, MC_OP, "metacells", cid=mc.metacell_idx_col, sets=SETS, group_by=regions, host_delaunay=mc.metacell_delaunay,
                 score_params=params)
    assert len(detail_calls) == 2 and got.groups["total_triangles"].sum() > 0
    assert (got.groups.groupby("set")["total_triangles"].sum() + got.cross["total_triangles"].to_numpy() == len(mc.metacell_delaunay)).all()


def test_a_missing_label_takes_the_host_route_to_the_same_frames(detail_calls):
    ref, mov, cols = _frames(1500, 3)
    labels = mov["cell_type"].to_numpy().astype(object)
    labels[7::41] = np.nan
    mov = mov.assign(region=_regions(mov), cell_type=labels)
    got = _study(ref, mov, cols, OP, "missing label", sets=SETS[:1], group_by="region", score_delaunay=_simplices(mov))
    assert len(detail_calls) == 0                                     # DeviceScores.prepare refused: score_table_details on the tables
    n_missing = int(pd.isna(labels).sum())
    assert got.confusion.to_numpy().sum() < got.scores["matched"].iloc[0] <= got.confusion.to_numpy().sum() + n_missing


# ---- 2. score_table_details with a triangulation: the golden, additivity ---------------------------------------------------------------------
def _golden_study():
    g = golden()
    frame = lambda side: pd.DataFrame({"cell_id": np.arange(len(g[f"{side}_xy"])), "X": g[f"{side}_xy"][:, 0], "Y": g[f"{side}_xy"][:, 1],
                                       "cell_type": g[f"{side}_cell_type"], "quadrant": g[f"{side}_quadrant"],
                                       **{c: g[f"{side}_types"][:, q] for q, c in enumerate(g["commonCT"])}})
    ref, mov = frame("ref"), frame("mov")
    table = pd.DataFrame({"Aligned_cell_id": g["a_row"].astype(np.int64), "Ref_cell_id": g["r_row"].astype(np.int64),
                          "ref_X": g["ref_xy"][g["r_row"], 0], "ref_Y": g["ref_xy"][g["r_row"], 1]})
    return g, ref, mov, table


def test_the_golden_per_quadrant_counts_and_rows_are_the_references():
    """score_table_details(group_by="quadrant", ignore_same_type_triangles=False) gives, per quadrant, the count of rows the reference's
    check_triangle_violations_within_quadrants flags, and check_triangle_violations on each quadrant's triangles -- the call it is made
    of -- flags those very rows and none outside the quadrant"""
    import same_amd

    g, ref, mov, table = _golden_study()
    params = {"ignore_same_type_triangles": False}
    got = same_amd.score_table_details(table, ref, mov, cell_id_col="cell_id", commonCT=list(g["commonCT"]), group_by="quadrant", top_k=TOP_K,
                                       score_delaunay=g["tris"], score_params=params)
    assert got.groups["group"].tolist() == list(QUADRANTS)
    assert got.groups["nodes_in_violating_triangles"].tolist() == [FLAGGED[q] for q in QUADRANTS]
    assert got.cross["total_triangles"].tolist() == [81] and got.groups["total_triangles"].sum() == 728 - 81
    assert got.groups["matched"].sum() == 372 and got.cross["matched"].tolist() == [0]
    quadrant = g["mov_quadrant"]
    q3 = quadrant[g["tris"]]
    flagged = np.zeros(len(table), bool)
    for q in QUADRANTS:
        within = (q3 == q).all(axis=1)
        out = table.assign(cell_type=mov["cell_type"].to_numpy()[g["a_row"]])
        carrier = types.SimpleNamespace(metacell_df=mov[["X", "Y"]], metacell_delaunay=g["tris"][within])
        rows, _stats = same_amd.check_triangle_violations(out, carrier, aligned_id_col="Aligned_cell_id", ref_id_col="Ref_cell_id",
                                                          mapped_x_col="ref_X", mapped_y_col="ref_Y", **params)
        mine = rows["in_violating_triangle"].to_numpy(dtype=bool)
        assert not mine[quadrant[g["a_row"]] != q].any()
        flagged |= mine
    assert np.array_equal(flagged, g["triangle_violation"])


@pytest.mark.parametrize("seed", [0, 1])
def test_groups_and_cross_add_up_to_score_tables_record(seed):
    """random small tables: rows without a group, triangles across groups and triangles naming ids the frame lacks"""
    import same_amd

    ref, mov, cols, table, _a, _r = _small_study(seed)
    rng = np.random.default_rng(seed + 40)
    tris = np.vstack((_simplices(mov), rng.integers(0, len(mov), (40, 3)), np.column_stack((rng.integers(0, len(mov), (9, 2)), np.full(9, 9999)))))
    tris = tris[(tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])]
    for params in ({}, {"ignore_same_type_triangles": False}):
        got = same_amd.score_table_details(table, ref, mov, cell_id_col=CID, commonCT=cols, group_by="region", score_delaunay=tris,
                                           score_params=params)
        record = same_amd.score_table(table, ref, mov, cell_id_col=CID, score_delaunay=tris, score_params=params)
        assert got.scores.iloc[0].to_dict() == record
        for k in ("matched", "type_matches", "total_triangles", "triangles_with_all_matched", "triangles_same_type_skipped", "triangles_flipped"):
            assert got.groups[k].sum() + got.cross[k].iloc[0] == record[k], (k, params)
        assert got.cross["total_triangles"].iloc[0] >= 9 and got.groups["nodes_in_violating_triangles"].sum() <= record["nodes_in_violating_triangles"]
        assert got.groups["triangles_flipped"].sum() > 0 and got.cross["triangles_flipped"].iloc[0] > 0
