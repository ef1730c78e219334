"""same_amd.score_features without a GPU: `score_table_features` on a small table against the notebook's own expressions --
`groupby().mean()` within the derived bound, `cdist(...).min(axis=1)` and `pd.cut` exactly --, `standard_scale_var` against scanpy's
formula, every argument check of `sliding_window_score_features` before a job or a device is touched, and the new entry points in the
header, the ctypes table and the built library at ABI 9."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import cdist

import feature_check as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = "Cell_Num_Old"
NEW = ("same_score_features_create", "same_score_features_destroy", "same_feature_zone_create", "same_feature_zone_destroy",
       "same_merge_acc_score_features")


def _study(n_ref=300, n_mov=260, n=200, seed=0):
    """frames with ids that are not their rows, markers on both sides, and a table of n pairs in no particular order"""
    rng = np.random.default_rng(seed)
    ref = pd.DataFrame({"X": rng.random(n_ref) * 400, "Y": rng.random(n_ref) * 400, "cell_type": rng.choice(list("ABC"), n_ref),
                        CID: 1000 + rng.permutation(n_ref), "SFTPC": rng.lognormal(0, 2, n_ref), "PDCD1": rng.poisson(2.0, n_ref)})
    mov = pd.DataFrame({"X": rng.random(n_mov) * 400, "Y": rng.random(n_mov) * 400, "cell_type": rng.choice(list("ABCD"), n_mov),
                        CID: 5000 + rng.permutation(n_mov), "CD8": rng.normal(0, 3, n_mov).astype(np.float32), "PanCK": rng.integers(0, 9, n_mov)},
                       index=[f"m{i}" for i in range(n_mov)])
    rows_m, rows_r = rng.choice(n_mov, n, replace=False), rng.choice(n_ref, n, replace=False)
    table = pd.DataFrame({f"Aligned_{CID}": mov[CID].to_numpy()[rows_m], f"Ref_{CID}": ref[CID].to_numpy()[rows_r],
                          "ref_X": ref["X"].to_numpy()[rows_r], "ref_Y": ref["Y"].to_numpy()[rows_r]})
    return ref, mov, table, rows_m, rows_r


def test_means_per_group_against_groupby_mean_within_the_bound():
    import same_amd

    ref, mov, table, rows_m, rows_r = _study()
    got = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, moving_features=["CD8", "PanCK"], ref_features=["SFTPC", "PDCD1"])
    names = ["moving_CD8", "moving_PanCK", "ref_SFTPC", "ref_PDCD1"]
    assert list(got.means.columns) == names == list(got.sums.columns) == list(got.resolution.index) and got.zones is None and got.pairs is None
    # the notebook: the two sides' rows of every pair side by side, grouped by the moving label
    combined = pd.DataFrame(np.column_stack((mov[["CD8", "PanCK"]].to_numpy(np.float64)[rows_m], ref[["SFTPC", "PDCD1"]].to_numpy(np.float64)[rows_r])),
                            columns=names)
    combined["label"] = mov["cell_type"].to_numpy()[rows_m]
    want = combined.groupby("label", sort=False).mean()
    order = list(pd.factorize(mov["cell_type"].to_numpy())[1])
    assert list(got.means.index) == order == list(got.rows.index) and got.rows.tolist() == combined["label"].value_counts()[order].tolist()
    e = -np.log2(got.resolution.to_numpy()).astype(np.int32)
    values = combined[names].to_numpy()
    for label in order:
        rows = np.flatnonzero((combined["label"] == label).to_numpy())
        mine = got.means.loc[label].to_numpy()
        # against the true mean: the derived bound and nothing more
        true = C.fsum_means(values, rows)
        assert (np.abs(mine - true) <= C.mean_bound(e, true)).all(), label
        # against pandas' own mean, a float sum of n terms: each of its n - 1 additions rounds a partial sum of at most n * max |x| by
        # 2**-53 of it, the division once more -- so it is within n * 2**-53 * max |x| of the true mean, whatever the order of its sum
        allowance = len(rows) * 2.0**-53 * np.abs(values[rows]).max(axis=0)
        assert (np.abs(mine - want.loc[label].to_numpy()) <= C.mean_bound(e, true) + allowance).all(), label
    assert got.sums.to_numpy().dtype == np.int64 and got.sums.to_numpy().sum() != 0
    # the same sums from the statement, and an array or a DataFrame is the same thing as the names
    q_m, e_m = C.quantize(mov[["CD8", "PanCK"]].to_numpy(np.float64))
    q_r, e_r = C.quantize(ref[["SFTPC", "PDCD1"]].to_numpy(np.float64))
    codes = pd.factorize(mov["cell_type"].to_numpy())[0].astype(np.int32)
    out, _d2 = C.host_features(rows_m, rows_r, len(mov), q_m, q_r, codes, len(order))
    assert np.array_equal(out[4 + len(order) + 1:].reshape(len(order) + 1, 4)[:len(order)], got.sums.to_numpy())
    assert np.array_equal(np.ldexp(1.0, -np.concatenate((e_m, e_r))), got.resolution.to_numpy())
    other = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, moving_features=mov[["CD8", "PanCK"]],
                                          ref_features=ref[["SFTPC", "PDCD1"]].to_numpy())
    assert np.array_equal(other.sums.to_numpy(), got.sums.to_numpy()) and list(other.sums.columns) == names[:2] + ["ref_0", "ref_1"]


def test_groups_with_missing_values_and_one_side_only():
    import same_amd

    ref, mov, table, rows_m, _rows_r = _study()
    region = np.where(np.arange(len(mov)) % 5 == 0, None, np.arange(len(mov)) % 3).astype(object)
    got = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, moving_features=["PanCK"], group_by=region)
    assert list(got.rows.index) == [1, 2, 0, "(no group)"] and got.rows.sum() == len(table)
    sel = np.array([v is None for v in region[rows_m]])
    assert got.rows["(no group)"] == sel.sum() and got.means.loc["(no group)", "moving_PanCK"] == mov["PanCK"].to_numpy()[rows_m][sel].mean()
    empty = same_amd.score_table_features(table.iloc[:0], ref, mov, cell_id_col=CID, ref_features=["PDCD1"])
    assert not empty.rows.any() and empty.means.isna().all().all() and not empty.sums.to_numpy().any()


def test_distance_to_the_zone_against_cdist_and_pd_cut():
    import same_amd
    from same_amd import FeatureZones

    ref, mov, table, rows_m, rows_r = _study()
    rng = np.random.default_rng(9)
    zone_ref, subset_mov = rng.random(len(ref)) < 0.2, rng.random(len(mov)) < 0.6
    edges = [0, 15, 30, np.inf]
    zones = FeatureZones(None, zone_ref, subset_mov, None, edges, labels=["near", "mid", "far"])
    got = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, ref_features=["PDCD1"], zones=zones, per_pair=True)
    # the notebook's own expressions over the pairs
    X_spatial = ref[["X", "Y"]].to_numpy()[rows_r]
    is_zone, is_subset = zone_ref[rows_r], subset_mov[rows_m]
    dist = cdist(X_spatial[is_subset], X_spatial[is_zone]).min(axis=1)
    want = np.full(len(mov), np.nan)
    want[rows_m[is_subset]] = dist
    assert C.same_bits(got.pairs["distance_to_zone"].to_numpy(), want) and got.pairs.index.equals(mov.index)
    cut = pd.cut(dist, edges, labels=["near", "mid", "far"])
    z = got.zones
    assert (z.zone_pairs, z.subset_pairs) == (int(is_zone.sum()), int(is_subset.sum()))
    counts = pd.Series(cut).value_counts()
    assert z.rows.loc[["near", "mid", "far"]].tolist() == [int(counts[k]) for k in ("near", "mid", "far")]
    assert z.rows.get("(no bin)", 0) == int(pd.isna(cut).sum()) == int((dist == 0).sum()) > 0              # the pairs that are both: 0 is in no bin
    marker = ref["PDCD1"].to_numpy(np.float64)[rows_r][is_subset]
    e = -np.log2(got.resolution.to_numpy()).astype(np.int32)
    for k in ("near", "mid", "far"):
        rows = np.flatnonzero(np.asarray(cut == k))
        true = C.fsum_means(marker[:, None], rows)
        assert abs(z.means.loc[k, "ref_PDCD1"] - true[0]) <= C.mean_bound(e, true)[0], k             # the derived bound
        allowance = len(rows) * 2.0**-53 * np.abs(marker[rows]).max()                                  # numpy's own float sum (as above)
        assert abs(z.means.loc[k, "ref_PDCD1"] - marker[rows].mean()) <= C.mean_bound(e, true)[0] + allowance, k
    matched = np.zeros(len(mov), bool)
    matched[rows_m] = True
    assert got.pairs["ref_id"][matched].tolist() == ref[CID].to_numpy()[rows_r][np.argsort(rows_m)].tolist() and got.pairs["ref_id"][~matched].isna().all()
    # no zone pair: every distance NaN, every subset pair in no bin
    none = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, ref_features=["PDCD1"], per_pair=True,
                                         zones=FeatureZones(np.zeros(len(mov), bool), None, None, None, edges))
    assert none.pairs["distance_to_zone"].isna().all() and none.zones.rows.tolist() == [0, 0, 0, len(table)] and none.zones.zone_pairs == 0
    assert list(none.zones.rows.index) == ["(0, 15]", "(15, 30]", "(30, inf]", "(no bin)"]


def test_reference_xy_that_is_not_finite_goes_to_the_host_statement_which_reads_it_as_cdist_does():
    import same_amd
    from same_amd import FeatureZones
    from same_amd.score_features import FeatureSpec

    ref, mov, table, rows_m, rows_r = _study()
    rng = np.random.default_rng(9)
    zone_ref = rng.random(len(ref)) < 0.2
    zones = FeatureZones(None, zone_ref, None, None, [0, 15, 30, np.inf])
    assert FeatureSpec(ref, mov, None, ["PDCD1"], None, zones).device_ok and FeatureSpec(ref, mov, None, ["PDCD1"], None, None).device_ok
    plain = same_amd.score_table_features(table, ref, mov, cell_id_col=CID, ref_features=["PDCD1"], zones=zones, per_pair=True)
    # a matched reference cell outside the zone without an X: its own pair has no distance, every other pair keeps its own
    lone = int(rows_r[np.flatnonzero(~zone_ref[rows_r])[0]])
    bad = ref.copy()
    bad.loc[bad.index[lone], "X"] = np.nan
    assert not FeatureSpec(bad, mov, None, ["PDCD1"], None, zones).device_ok           # the device is not asked
    assert FeatureSpec(bad, mov, None, ["PDCD1"], None, None).device_ok                # (without a zone nothing reads the XY)
    got = same_amd.score_table_features(table, bad, mov, cell_id_col=CID, ref_features=["PDCD1"], zones=zones, per_pair=True)
    X = bad[["X", "Y"]].to_numpy()[rows_r]
    want = np.full(len(mov), np.nan)
    want[rows_m] = cdist(X, X[zone_ref[rows_r]]).min(axis=1)
    want[rows_m[zone_ref[rows_r]]] = 0.0
    assert C.same_bits(got.pairs["distance_to_zone"].to_numpy(), want)
    row = rows_m[list(rows_r).index(lone)]
    assert np.isnan(got.pairs["distance_to_zone"].iloc[row]) and not np.isnan(plain.pairs["distance_to_zone"].iloc[row])
    assert got.zones.rows["(no bin)"] == plain.zones.rows["(no bin)"] + 1 and got.zones.rows.sum() == plain.zones.rows.sum() == len(table)
    # a zone cell without an X: no pair outside the zone has a distance, as cdist(...).min(axis=1) has none
    worst = ref.copy()
    worst.loc[worst.index[int(rows_r[np.flatnonzero(zone_ref[rows_r])[0]])], "X"] = np.nan
    got = same_amd.score_table_features(table, worst, mov, cell_id_col=CID, ref_features=["PDCD1"], zones=zones, per_pair=True)
    in_zone = int(zone_ref[rows_r].sum())
    assert got.zones.rows.tolist() == [0, 0, 0, len(table)] and int(got.pairs["distance_to_zone"].isna().sum()) == len(mov) - in_zone


def test_standard_scale_var_is_scanpys_formula():
    from same_amd import standard_scale_var

    means = pd.DataFrame({"a": [1.0, 3.0, 2.0], "b": [5.0, 5.0, 5.0], "c": [np.nan, 1.0, 0.0]}, index=list("xyz"))
    values_df = means.copy()
    values_df -= values_df.min(0)
    values_df = (values_df / values_df.max(0)).fillna(0)
    got = standard_scale_var(means)
    pd.testing.assert_frame_equal(got, values_df, check_exact=True)
    assert got["a"].tolist() == [0.0, 1.0, 0.5] and got["b"].tolist() == [0.0, 0.0, 0.0] and means["a"].tolist() == [1.0, 3.0, 2.0]


def test_every_argument_check_raises_before_a_device_is_touched(monkeypatch):
    import same_amd
    from same_amd import FeatureZones, _lib, window_api

    def touched(*_a, **_k):
        raise AssertionError("a job or a device was touched")

    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.setattr(_lib, "Context", touched)
    monkeypatch.setattr(window_api._WindowJob, "__init__", touched)
    ref, mov, _table, _m, _r = _study()
    call = lambda **kw: same_amd.sliding_window_score_features(ref, mov, list("ABC"), optim_params={"cell_id_col": CID}, **kw)
    with pytest.raises(ValueError, match="moving_features, ref_features or both"):
        call()
    with pytest.raises(ValueError, match="not finite"):
        call(ref_features=ref[["SFTPC"]].to_numpy() * np.where(np.arange(len(ref)) == 7, np.nan, 1.0)[:, None])
    with pytest.raises(ValueError, match="not finite"):
        call(moving_features=pd.DataFrame({"x": np.where(np.arange(len(mov)) == 3, np.inf, 1.0)}, index=mov.index))
    with pytest.raises(ValueError, match="has 5 rows"):
        call(moving_features=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="not on the moving frame's index"):
        call(moving_features=pd.DataFrame({"x": np.zeros(len(mov))}))
    with pytest.raises(ValueError, match="lacks"):
        call(ref_features=["SFTPC", "nowhere"])
    with pytest.raises(ValueError, match="no numbers"):
        call(moving_features=np.array([["a"]] * len(mov), dtype=object))
    with pytest.raises(ValueError, match="must be a DataFrame"):
        call(moving_features="CD8")
    with pytest.raises(ValueError, match="group_by"):
        call(moving_features=["CD8"], group_by="nowhere")
    ok = dict(moving_features=["CD8"])
    with pytest.raises(ValueError, match="FeatureZones"):
        call(zones=(None, None, None, None, [0, 1]), **ok)
    with pytest.raises(ValueError, match="boolean mask of"):
        call(zones=FeatureZones(np.ones(len(mov) - 1, bool), None, None, None, [0, 1]), **ok)
    with pytest.raises(ValueError, match="boolean mask of"):
        call(zones=FeatureZones(None, np.ones(len(ref), np.int64), None, None, [0, 1]), **ok)
    with pytest.raises(ValueError, match="must not decrease"):
        call(zones=FeatureZones(None, None, None, None, [0, 30, 15]), **ok)
    with pytest.raises(ValueError, match="must not decrease"):
        call(zones=FeatureZones(None, None, None, None, [0, np.nan]), **ok)
    with pytest.raises(ValueError, match="2 .. 65"):
        call(zones=FeatureZones(None, None, None, None, [0]), **ok)
    with pytest.raises(ValueError, match="2 .. 65"):
        call(zones=FeatureZones(None, None, None, None, np.arange(67.0)), **ok)
    with pytest.raises(ValueError, match="labels for 2 bins"):
        call(zones=FeatureZones(None, None, None, None, [0, 1, 2], labels=["a"]), **ok)
    with pytest.raises(ValueError, match="score_params"):
        call(score_params={"nodes": 1}, **ok)
    for refused in ("unpack", "tables"):
        with pytest.raises(TypeError, match=refused):
            call(**{refused: "nearest"}, **ok)


def test_quantisation_and_means_are_the_statements():
    from same_amd.score_features import means_from_sums, quantize_features

    x = C.float_columns(400, 12, 3)
    q, e = quantize_features(x)
    want_q, want_e = C.quantize(x)
    assert q.dtype == np.int32 and np.array_equal(q, want_q) and np.array_equal(e, want_e)
    sums = q.astype(np.int64).sum(axis=0)
    assert C.same_bits(means_from_sums(sums[None, :], np.array([400]), e)[0], C.means(sums, 400, e))
    assert np.isnan(means_from_sums(np.zeros((1, 12), np.int64), np.array([0]), e)).all()
    q0, e0 = quantize_features(np.zeros((0, 3)))
    assert q0.shape == (0, 3) and not e0.any()


def test_the_new_entry_points_are_declared_bound_and_exported_at_abi_9():
    from same_amd import _lib
    from same_amd import windows as W

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code) and name in _lib.EXPORTS and hasattr(lib, name), name
        decl = re.search(rf"\b{name}\s*\((.*?)\);", code, flags=re.S)
        assert len(decl.group(1).split(",")) == len(_lib._PROTOTYPES[name]), name
    assert lib.same_abi_version() == _lib.ABI_VERSION == 9 and "#define SAME_ABI_VERSION 9" in header
    assert "#define SAME_FEATURE_MAX_COLUMNS 4096" in header and _lib.SAME_FEATURE_MAX_COLUMNS == 4096 >= 1024
    assert "#define SAME_FEATURE_MAX_EDGES 65" in header and _lib.SAME_FEATURE_MAX_EDGES == 65
    assert W.score_feature_words(3, 5) == 4 + 4 * 6 and W.score_feature_words(3, 5, 2) == 4 + 4 * 6 + 3 * 6
    parts = W.split_score_features(np.arange(W.score_feature_words(2, 3, 1)), 2, 3, 1)
    assert parts["counts"].tolist() == [0, 1, 2, 3] and parts["rows"].tolist() == [4, 5, 6] and parts["sums"].shape == (3, 3)
    assert parts["bin_rows"].tolist() == [16, 17] and parts["bin_sums"].tolist() == [[18, 19, 20], [21, 22, 23]]
    # null handles are refused, not followed: no device is needed to be told so
    out = np.zeros(8, np.int64)
    h = ctypes.c_void_p()
    assert lib.same_merge_acc_score_features(None, None, None, None, None, out.ctypes.data, 8, None) == _lib.SAME_EINVAL
    assert lib.same_score_features_create(None, None, None, 1, None, 0, None, 1, ctypes.byref(h)) == _lib.SAME_EINVAL and not h.value
    assert lib.same_feature_zone_create(None, None, None, None, 2, ctypes.byref(h)) == _lib.SAME_EINVAL and not h.value
    lib.same_score_features_destroy(None)
    lib.same_feature_zone_destroy(None)
