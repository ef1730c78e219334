"""`same_amd.sliding_window_score_features(unpack=...)` as a product: every frame the device sums from a result's unpacked cell pairs
(csrc/window_unpack_feature.hip) equals `score_unpacked_features` of that result's table -- `unpack_metacell_matches`, numpy sums of the
same fixed-point columns of the ORIGINAL cells, the brute-force minimum over the reference cells' own coordinates --, frame for frame
and exactly, distances bit for bit; `scores` is sliding_window_scores(unpack=)'s frame.  Every test here fails without the feature:
sliding_window_score_features takes no `unpack`."""
import numpy as np
import pandas as pd
import pytest

from test_gpu_score_features import EDGES, _same_reading
from test_gpu_scores import MC_OP
from test_gpu_unpack_scores import CELL_KEYS, SETS, _changed, _objects
from test_gpu_window_variants import _variants_of

pytestmark = pytest.mark.gpu


def _inputs(mc_ref, mc_mov, cols, form="frame", seed=0, n_ref_columns=5):
    """what a cell-level study reads, everything per ORIGINAL cell: the moving cells' own type columns (by name, as an array or as a
    frame), markers of the reference cells, regions of the moving cells with some in none, a zone of about a fifth of the reference
    cells and a subset of about half the moving cells"""
    import same_amd

    ref_c, mov_c = mc_ref.original_df, mc_mov.original_df
    rng = np.random.default_rng(seed)
    markers = pd.DataFrame(rng.lognormal(0.0, 1.5, (len(ref_c), n_ref_columns)), index=ref_c.index, columns=[f"m{q}" for q in range(n_ref_columns)])
    markers["m0"] = 0.0
    own = list(cols)[:3]
    moving = {"names": own, "array": mov_c[own].to_numpy(), "frame": mov_c[own]}[form]
    region = np.where(rng.random(len(mov_c)) < 0.1, None, rng.integers(0, 4, len(mov_c)).astype(object))
    zones = same_amd.FeatureZones(None, rng.random(len(ref_c)) < 0.2, rng.random(len(mov_c)) < 0.5, None, EDGES, labels=["near", "mid", "far"])
    return dict(moving_features=moving, ref_features=markers if form != "array" else markers.to_numpy(), group_by=region, zones=zones)


def _study(mc_ref, mc_mov, cols, strategy, inputs, *, op=MC_OP, variants=None, sets=None, per_pair=True):
    """sliding_window_score_features(unpack=) against sliding_window_scores(tables=True, unpack=) + score_unpacked_features per table"""
    import same_amd

    common = dict(type_variants=variants, param_sets=sets, optim_params=dict(op), unpack=strategy)
    got = same_amd.sliding_window_score_features(mc_ref, mc_mov, list(cols), per_pair=per_pair, **inputs, **common)
    scores, tables, cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), tables=True, **common)
    n_v, n_s = len(variants or [None]), len(sets or [{}])
    assert isinstance(got, same_amd.ScoreFeatures) and len(got.means) == n_v and all(len(m) == n_s for m in got.means)
    pd.testing.assert_frame_equal(got.scores, scores, check_exact=True)
    assert list(got.scores.columns[-3:]) == list(CELL_KEYS)
    for v in range(n_v):
        for s in range(n_s):
            want = same_amd.score_unpacked_features(tables[v][s], mc_ref, mc_mov, strategy, per_pair=per_pair, **inputs)
            _same_reading((got.rows[v][s], got.means[v][s], got.sums[v][s], None if got.zones is None else got.zones[v][s],
                           None if got.pairs is None else got.pairs[v][s]), want, f"[{v}][{s}] {strategy}")
            # the frames count CELL pairs: the unpacked table's rows, the record's cells_matched
            assert got.rows[v][s].sum() == len(cell_tables[v][s]) == scores["cells_matched"].iloc[v * n_s + s] > scores["matched"].iloc[v * n_s + s]
            pd.testing.assert_series_equal(got.resolution, want.resolution, check_exact=True)
    return got, cell_tables


@pytest.mark.parametrize("strategy", ["distribute", "nearest"])
def test_a_study_of_two_variants_and_two_sets_equals_the_host_statement_of_its_tables(monkeypatch, strategy):
    from same_amd import windows as W

    mc_ref, mc_mov, cols = _objects("5 against 4")
    calls, real = [], W.MergeAccumulator.unpack_features
    monkeypatch.setattr(W.MergeAccumulator, "unpack_features", lambda self, *a, **k: calls.append(a[2]) or real(self, *a, **k))
    monkeypatch.setattr(W.MergeAccumulator, "score_features", lambda *a, **k: pytest.fail("the section-level call was made"))
    inputs = _inputs(mc_ref, mc_mov, cols)
    variants = _variants_of(mc_mov.metacell_df, cols)[:2]
    got, cell_tables = _study(mc_ref, mc_mov, cols, strategy, inputs, variants=variants, sets=SETS)
    assert calls == [strategy] * 4                                  # the device read every result, by one call each
    ids = pd.Index(mc_mov.original_df["Cell_Num_Old"].to_numpy())
    flat = [(got.rows[v][s], got.means[v][s], got.zones[v][s], got.pairs[v][s], cell_tables[v][s]) for v in range(2) for s in range(2)]
    for rows, means, zone, pairs, cells in flat:                    # not vacuous
        assert list(rows.index) == list(pd.factorize(inputs["group_by"])[1]) + ["(no group)"] and (rows > 0).all()
        assert list(means.columns) == [f"moving_{c}" for c in list(cols)[:3]] + [f"ref_m{q}" for q in range(5)]
        assert not means["ref_m0"].any() and (means["ref_m1"] > 0).all() and means.notna().all().all()
        assert list(zone.rows.index)[:3] == ["near", "mid", "far"] and (zone.rows.iloc[:3] > 0).all() and 0 < zone.zone_pairs < rows.sum()
        assert zone.rows.sum() == zone.subset_pairs and pairs["distance_to_zone"].notna().sum() == zone.subset_pairs
        # indexed by the moving CELL id; ref_id is the reference CELL the unpacked table gave it
        assert pairs.index.equals(ids) and pairs["ref_id"].notna().sum() == rows.sum() == len(cells)
        assert pairs["ref_id"].loc[cells["Aligned_cell_id"].to_numpy()].to_numpy().astype(np.int64).tolist() == cells["Ref_cell_id"].tolist()
    assert any(not a[1].equals(b[1]) for a, b in zip(flat, flat[1:]))
    lean, _t = _study(mc_ref, mc_mov, cols, strategy, dict(inputs, zones=None), per_pair=False)
    assert lean.zones is None and lean.pairs is None


@pytest.mark.parametrize("form", ["names", "array"])
def test_features_given_as_column_names_and_as_an_array(form):
    """(a DataFrame on the original index: the test above) -- the same frames but for the array's column names"""
    mc_ref, mc_mov, cols = _objects("ms3")
    got, _t = _study(mc_ref, mc_mov, cols, "nearest", _inputs(mc_ref, mc_mov, cols, form), sets=SETS)
    ref, _t = _study(mc_ref, mc_mov, cols, "nearest", _inputs(mc_ref, mc_mov, cols, "frame"), sets=SETS)
    for s in range(2):
        assert np.array_equal(got.sums[0][s].to_numpy(), ref.sums[0][s].to_numpy()) and got.rows[0][s].equals(ref.rows[0][s])
    if form == "array":
        assert list(got.means[0][0].columns) == [f"moving_{q}" for q in range(3)] + [f"ref_{q}" for q in range(5)]


def test_the_group_means_are_the_notebooks_groupby_mean_over_the_nearest_cell_pairs():
    """examples/luad/reproduce_figures.ipynb cells 12, 16, 18 on the device's 'nearest' pairs: mean per annotation of the moving cell of
    the gathered (quantised) columns"""
    import same_amd
    from same_amd.score_features import quantize_features

    mc_ref, mc_mov, cols = _objects("ms3")
    got = same_amd.sliding_window_score_features(mc_ref, mc_mov, list(cols), unpack="nearest", moving_features=list(cols)[:2],
                                                 ref_features=list(cols)[1:], optim_params=dict(MC_OP))
    _scores, tables, cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack="nearest", tables=True, optim_params=dict(MC_OP))
    cells = cell_tables[0][0]
    pcf, xen = mc_mov.original_df.set_index("Cell_Num_Old"), mc_ref.original_df.set_index("Cell_Num_Old")
    (q_m, e_m), (q_r, e_r) = quantize_features(pcf[list(cols)[:2]].to_numpy()), quantize_features(xen[list(cols)[1:]].to_numpy())
    combined = pd.concat([pd.DataFrame(np.ldexp(q_m.astype(np.float64), -e_m), index=pcf.index).loc[cells["Aligned_cell_id"]].reset_index(drop=True),
                          pd.DataFrame(np.ldexp(q_r.astype(np.float64), -e_r), index=xen.index).loc[cells["Ref_cell_id"]].reset_index(drop=True)],
                         axis=1, ignore_index=True)
    combined["pcf_Annotations"] = pcf["cell_type"].loc[cells["Aligned_cell_id"]].to_numpy()
    by = combined.groupby("pcf_Annotations", sort=False)
    assert got.rows[0][0].to_dict() == by.size().to_dict() and len(got.rows[0][0]) >= 2
    # every value is a multiple of 2**-e below 2**31 steps and there are fewer than 2**20 pairs: pandas' float sum is exact, as the
    # device's integer sum is, and each mean is that sum rounded once by the division -- a few ulps cover the order of the two scalings
    np.testing.assert_allclose(got.means[0][0].to_numpy(), by.mean().loc[got.means[0][0].index].to_numpy(), rtol=4 * 2.0**-53, atol=0)


@pytest.mark.parametrize("why", ["forced", "more columns than the cap", "permuted metacell ids", "non-finite reference cell XY"])
def test_what_the_device_does_not_read_comes_back_the_same_through_the_host_statement(monkeypatch, why):
    import copy

    import same_amd
    from same_amd import _lib
    from same_amd import windows as W
    from same_amd.score_features import FeatureSpec

    monkeypatch.setattr(W.MergeAccumulator, "unpack_features", lambda *a, **k: pytest.fail("read on the device"))
    mc_ref, mc_mov, cols = _objects("ms3")
    strategy, n_ref_columns = "distribute", 5
    if why == "forced":
        monkeypatch.setattr(FeatureSpec, "device_ok", property(lambda self: False))
    elif why == "more columns than the cap":
        n_ref_columns = _lib.SAME_FEATURE_MAX_COLUMNS - 2
    elif why == "permuted metacell ids":
        ids = mc_ref.metacell_df[mc_ref.metacell_idx_col].to_numpy().copy()
        ids[[3, 11]] = ids[[11, 3]]
        mc_ref = _changed(mc_ref, ids=ids)
    else:
        mc_ref = copy.copy(mc_ref)
        mc_ref.original_df = mc_ref.original_df.copy()
        mc_ref.original_df.loc[mc_ref.original_df.index[5], "X"] = np.inf       # ('distribute' reads no XY; the zone would)
    inputs = _inputs(mc_ref, mc_mov, cols, n_ref_columns=n_ref_columns)
    got, _t = _study(mc_ref, mc_mov, cols, strategy, inputs, sets=SETS)
    assert got.rows[0][0].sum() > 0 and got.means[0][0].shape[1] == 3 + n_ref_columns
