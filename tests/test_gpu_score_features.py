"""same_amd.sliding_window_score_features as a product: every frame the device sums from a result's merged rows equals
`score_table_features` of that result's table -- the host statement: numpy sums of the same fixed-point columns, the brute-force
minimum, thresholds on the squared distance --, frame for frame and exactly, distances bit for bit; `scores` is sliding_window_scores'
frame.  Every test here fails without the feature: same_amd has no sliding_window_score_features."""
import numpy as np
import pandas as pd
import pytest

from test_gpu_scores import CID, MC_OP, OP, SETS, _frames, _plain_tris
from test_gpu_window_variants import _variants_of

pytestmark = pytest.mark.gpu

EDGES = [0, 15, 30, np.inf]


def _inputs(ref_df, mov_df, cols, seed=0, n_ref_columns=5):
    """what a study reads: the moving frame's own type columns by name, a frame of markers on the reference index, regions of the moving
    rows with some in none, a zone of about a fifth of the reference rows and a subset of about half the moving rows"""
    import same_amd

    rng = np.random.default_rng(seed)
    markers = pd.DataFrame(rng.lognormal(0.0, 1.5, (len(ref_df), n_ref_columns)), index=ref_df.index,
                           columns=[f"m{q}" for q in range(n_ref_columns)])
    markers["m0"] = 0.0                                                           # an all-zero column
    region = np.where(rng.random(len(mov_df)) < 0.1, None, rng.integers(0, 4, len(mov_df)).astype(object))
    zones = same_amd.FeatureZones(None, rng.random(len(ref_df)) < 0.2, rng.random(len(mov_df)) < 0.5, None, EDGES, labels=["near", "mid", "far"])
    return dict(moving_features=list(cols)[:3], ref_features=markers, group_by=region, zones=zones)


def _same_reading(got, want, tag):
    rows, means, sums, zones, pairs = got
    pd.testing.assert_series_equal(rows, want.rows, check_exact=True, obj=f"rows{tag}")
    pd.testing.assert_frame_equal(means, want.means, check_exact=True, obj=f"means{tag}")
    pd.testing.assert_frame_equal(sums, want.sums, check_exact=True, obj=f"sums{tag}")
    assert (zones is None) == (want.zones is None)
    if zones is not None:
        assert (zones.zone_pairs, zones.subset_pairs) == (want.zones.zone_pairs, want.zones.subset_pairs), tag
        pd.testing.assert_series_equal(zones.rows, want.zones.rows, check_exact=True, obj=f"zone rows{tag}")
        pd.testing.assert_frame_equal(zones.means, want.zones.means, check_exact=True, obj=f"zone means{tag}")
        pd.testing.assert_frame_equal(zones.sums, want.zones.sums, check_exact=True, obj=f"zone sums{tag}")
    assert (pairs is None) == (want.pairs is None)
    if pairs is not None:
        pd.testing.assert_frame_equal(pairs, want.pairs, check_exact=True, obj=f"pairs{tag}")
        if "distance_to_zone" in pairs.columns:
            a, b = pairs["distance_to_zone"].to_numpy(), want.pairs["distance_to_zone"].to_numpy()
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)), tag


def _study(ref, mov, cols, op, inputs, *, cid=CID, variants=None, sets=None, per_pair=True, **kw):
    """sliding_window_score_features against sliding_window_scores(tables=True) + score_table_features per table -> the device's result"""
    import same_amd

    common = dict(type_variants=variants, param_sets=sets, optim_params=dict(op), **kw)
    got = same_amd.sliding_window_score_features(ref, mov, list(cols), per_pair=per_pair, **inputs, **common)
    scores, tables = same_amd.sliding_window_scores(ref, mov, list(cols), tables=True, **common)
    n_v, n_s = len(variants or [None]), len(sets or [{}])
    assert isinstance(got, same_amd.ScoreFeatures) and len(got.means) == n_v and all(len(m) == n_s for m in got.means)
    pd.testing.assert_frame_equal(got.scores, scores, check_exact=True)
    for v in range(n_v):
        for s in range(n_s):
            want = same_amd.score_table_features(tables[v][s], ref, mov, cell_id_col=cid, per_pair=per_pair, **inputs)
            _same_reading((got.rows[v][s], got.means[v][s], got.sums[v][s], None if got.zones is None else got.zones[v][s],
                           None if got.pairs is None else got.pairs[v][s]), want, f"[{v}][{s}]")
            assert got.rows[v][s].sum() == len(tables[v][s]) == scores["matched"].iloc[v * n_s + s]
            pd.testing.assert_series_equal(got.resolution, want.resolution, check_exact=True)
    return got


@pytest.mark.parametrize("route", ["default", "triangulations given"])
def test_a_study_of_two_variants_and_two_sets_equals_the_host_statement_of_its_tables(route):
    ref, mov, cols = _frames()
    variants = _variants_of(mov, cols)[:2]
    op, kw = (OP, {}) if route == "default" else (dict(OP, hip_caller_delaunay="device"), dict(moving_delaunay=_plain_tris()))
    got = _study(ref, mov, cols, op, _inputs(ref, mov, cols), variants=variants, sets=SETS[:2], **kw)
    flat = [(got.rows[v][s], got.means[v][s], got.zones[v][s], got.pairs[v][s]) for v in range(2) for s in range(2)]
    for rows, means, zone, pairs in flat:                           # not vacuous
        assert list(rows.index) == list(pd.factorize(_inputs(ref, mov, cols)["group_by"])[1]) + ["(no group)"] and (rows > 0).all()
        assert list(means.columns) == [f"moving_{c}" for c in list(cols)[:3]] + [f"ref_m{q}" for q in range(5)]
        assert not means["ref_m0"].any() and (means["ref_m1"] > 0).all() and means.notna().all().all()
        assert list(zone.rows.index)[:3] == ["near", "mid", "far"] and (zone.rows.iloc[:3] > 0).all() and 0 < zone.zone_pairs < rows.sum()
        assert zone.rows.sum() == zone.subset_pairs and pairs["distance_to_zone"].notna().sum() == zone.subset_pairs
        assert pairs.index.equals(mov.index) and pairs["ref_id"].notna().sum() == rows.sum()
    assert any(not a[1].equals(b[1]) for a, b in zip(flat, flat[1:]))
    lean = _study(ref, mov, cols, op, dict(_inputs(ref, mov, cols), zones=None), per_pair=False, **kw)
    assert lean.zones is None and lean.pairs is None


def test_metacell_objects_on_the_device_route():
    from test_gpu_caller_triangulation import _metacells

    ref, mc, cols = _metacells("ms3")
    frame = mc.metacell_df
    ref_df = getattr(ref, "metacell_df", ref)
    got = _study(ref, mc, cols, MC_OP, _inputs(ref_df, frame, cols, seed=2), cid=mc.metacell_idx_col, variants=_variants_of(frame, cols)[:2],
                 sets=SETS[:2])
    for v in range(2):
        for s in range(2):
            assert got.pairs[v][s].index.equals(frame.index) and got.rows[v][s].sum() > 0 and got.zones[v][s].subset_pairs > 0


def test_more_columns_than_the_cap_go_through_the_host_statement(monkeypatch):
    from same_amd import _lib
    from same_amd import windows as W

    ref, mov, cols = _frames(1500, 3)
    made = []
    monkeypatch.setattr(W.MergeAccumulator, "score_features", lambda *a, **k: made.append(1))
    inputs = _inputs(ref, mov, cols, n_ref_columns=_lib.SAME_FEATURE_MAX_COLUMNS - 2)       # with the three moving columns: one over
    got = _study(ref, mov, cols, OP, inputs, sets=SETS[:2])
    assert not made and got.means[0][0].shape[1] == _lib.SAME_FEATURE_MAX_COLUMNS + 1 and got.rows[0][0].sum() > 0


def test_the_device_is_what_reads_a_study_within_the_caps(monkeypatch):
    from same_amd import windows as W

    ref, mov, cols = _frames(1500, 3)
    calls = []
    real = W.MergeAccumulator.score_features
    monkeypatch.setattr(W.MergeAccumulator, "score_features", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    _study(ref, mov, cols, OP, _inputs(ref, mov, cols), sets=SETS[:2])
    assert len(calls) == 2
