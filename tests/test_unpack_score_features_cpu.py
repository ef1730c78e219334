"""`same_amd.score_unpacked_features` and the argument checks of `sliding_window_score_features(unpack=...)` without a GPU: the host
statement over hand-made MetaCell-like objects under 'distribute' (which touches no kernel) against the notebook's cells written out in
pandas -- cdist over the reference CELLS' own coordinates, pd.cut, groupby().mean() --, and every bad argument raised before a job or a
device is touched."""
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import cdist

from test_unpack_check_cpu import _objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("same_unpack_features_create", "same_unpack_features_destroy", "same_unpack_zone_create", "same_unpack_zone_destroy",
       "same_merge_acc_unpack_features")


def _study(seed=4):
    ref, mov, table = _objects()
    rng = np.random.default_rng(seed)
    mov.original_df["CD8"] = rng.normal(0, 3, len(mov.original_df)).astype(np.float32)
    mov.original_df["PanCK"] = rng.integers(0, 9, len(mov.original_df))
    ref.original_df["SFTPC"] = rng.lognormal(0, 2, len(ref.original_df))
    return ref, mov, table


def test_distance_to_the_zone_is_cdist_over_the_reference_cells_and_the_bins_are_pd_cuts():
    """cells 20-22: sftp_pos_coords are the coordinates of the reference CELLS of the zone pairs, the distance of a subset pair is
    cdist(its reference cell, those).min(), the bins pd.cut's; `pairs` is indexed by the moving cell id"""
    import same_amd

    ref, mov, table = _study()
    rng = np.random.default_rng(1)
    zone_ref, subset_mov = rng.random(len(ref.original_df)) < 0.3, rng.random(len(mov.original_df)) < 0.6
    edges = [0, 4, 9, np.inf]
    zones = same_amd.FeatureZones(None, zone_ref, subset_mov, None, edges)
    got = same_amd.score_unpacked_features(table, ref, mov, "distribute", moving_features=["CD8", "PanCK"], ref_features=["SFTPC"],
                                           zones=zones, per_pair=True)
    _rec, cells = same_amd.score_unpacked(table, ref, mov, "distribute")
    xen = ref.original_df.set_index("Cell_Num_Old")
    is_zone = pd.Series(zone_ref, index=xen.index).loc[cells["Ref_cell_id"]].to_numpy()
    is_subset = pd.Series(subset_mov, index=mov.original_df["Cell_Num_Old"]).loc[cells["Aligned_cell_id"]].to_numpy()
    X_spatial = xen.loc[cells["Ref_cell_id"], ["X", "Y"]].to_numpy()
    dist = cdist(X_spatial[is_subset], X_spatial[is_zone]).min(axis=1)
    assert got.zones.zone_pairs == is_zone.sum() > 0 and got.zones.subset_pairs == is_subset.sum() > 0
    pairs = got.pairs
    assert pairs.index.tolist() == mov.original_df["Cell_Num_Old"].tolist() and pairs.index.name == "Cell_Num_Old"
    at = cells["Aligned_cell_id"].to_numpy()
    assert pairs["ref_id"].loc[at].astype(np.int64).tolist() == cells["Ref_cell_id"].tolist() and pairs["ref_id"].isna().sum() == len(pairs) - len(cells)
    assert np.array_equal(pairs["distance_to_zone"].loc[at[is_subset]].to_numpy().view(np.uint64), dist.view(np.uint64))
    assert pairs["distance_to_zone"].notna().sum() == is_subset.sum()
    cut = pd.cut(dist, edges)
    want = pd.Series(cut).value_counts(sort=False)
    n_none = int(np.asarray(pd.isna(cut)).sum())                   # distance 0: a subset pair on a zone cell is in no bin of (0, ...]
    assert got.zones.rows.iloc[:3].tolist() == want.tolist() and (n_none == 0 or got.zones.rows.iloc[3] == n_none) and len(want) == 3
    assert np.count_nonzero(got.zones.rows.to_numpy()) >= 2
    # the bin means: groupby(bin).mean() of the quantised values
    from same_amd.score_features import quantize_features

    q, e = quantize_features(mov.original_df[["CD8"]].to_numpy())
    cd8 = pd.Series(np.ldexp(q[:, 0].astype(np.float64), -e[0]), index=mov.original_df["Cell_Num_Old"]).loc[at[is_subset]]
    by_bin = cd8.groupby(np.asarray(cut.codes)).mean()
    for b in range(3):
        if b in by_bin.index:
            assert got.zones.means["moving_CD8"].iloc[b] == by_bin.loc[b]


def test_both_sides_one_side_and_groups_given_as_an_array():
    import same_amd

    ref, mov, table = _study()
    region = np.where(np.arange(len(mov.original_df)) % 5 == 0, None, (np.arange(len(mov.original_df)) % 3).astype(object))
    got = same_amd.score_unpacked_features(table, ref, mov, "distribute", ref_features=ref.original_df[["SFTPC"]], group_by=region)
    assert list(got.rows.index) == [1, 2, 0, "(no group)"] and got.rows.sum() == 100 and list(got.means.columns) == ["ref_SFTPC"]
    arr = same_amd.score_unpacked_features(table, ref, mov, "distribute", ref_features=ref.original_df[["SFTPC"]].to_numpy(), group_by=region)
    assert np.array_equal(arr.sums.to_numpy(), got.sums.to_numpy()) and list(arr.means.columns) == ["ref_0"]
    default = same_amd.score_unpacked_features(table, ref, mov, "distribute", moving_features=["CD8"])
    assert sorted(default.rows.index) == ["a", "b", "c"]            # the cells' own cell_type
    empty = same_amd.score_unpacked_features(table.iloc[:0], ref, mov, "distribute", moving_features=["CD8"], per_pair=True)
    assert empty.rows.sum() == 0 and empty.pairs["ref_id"].isna().all() and len(empty.pairs) == len(mov.original_df)


def test_every_argument_check_raises_before_a_device_is_touched(monkeypatch):
    import same_amd
    from same_amd import FeatureZones, _lib, window_api

    def touched(*_a, **_k):
        raise AssertionError("a job or a device was touched")

    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.setattr(_lib, "Context", touched)
    monkeypatch.setattr(window_api._WindowJob, "__init__", touched)
    ref, mov, _table = _study()
    for df in (ref.metacell_df, mov.metacell_df):
        df["cell_type"], df["X"], df["Y"] = "a", 0.0, 0.0
    n_ref, n_mov = len(ref.original_df), len(mov.original_df)
    call = lambda r=ref, m=mov, unpack="nearest", **kw: same_amd.sliding_window_score_features(r, m, list("abc"), unpack=unpack, **kw)
    for bad in ("closest", "Nearest", 1, True):
        with pytest.raises(ValueError, match="unpack must be None or one of"):
            call(unpack=bad, moving_features=["CD8"])
    with pytest.raises(ValueError, match="MetaCell objects on both sides: ref has no"):
        call(r=ref.metacell_df, moving_features=["CD8"])
    with pytest.raises(ValueError, match="MetaCell objects on both sides: moving has no"):
        call(m=mov.metacell_df, moving_features=["CD8"])
    with pytest.raises(ValueError, match="moving_features, ref_features or both"):
        call()
    # the features are per ORIGINAL cell: a matrix of the metacells' length is refused
    with pytest.raises(ValueError, match=f"has {len(mov.metacell_df)} rows; the moving frame has {n_mov}"):
        call(moving_features=np.zeros((len(mov.metacell_df), 2)))
    with pytest.raises(ValueError, match="not on the ref frame's index"):
        call(ref_features=pd.DataFrame({"x": np.zeros(n_ref)}, index=np.arange(n_ref) + 5))
    with pytest.raises(ValueError, match="lacks"):
        call(moving_features=["CD8", "SFTPC"])                       # a column of the OTHER object's cells
    with pytest.raises(ValueError, match="not finite"):
        call(ref_features=np.where(np.arange(n_ref) == 7, np.nan, 1.0)[:, None])
    with pytest.raises(ValueError, match="group_by"):
        call(moving_features=["CD8"], group_by=np.zeros(len(mov.metacell_df)))
    ok = dict(moving_features=["CD8"])
    with pytest.raises(ValueError, match=f"boolean mask of {n_mov} rows"):
        call(zones=FeatureZones(np.ones(len(mov.metacell_df), bool), None, None, None, [0, 1]), **ok)
    with pytest.raises(ValueError, match=f"boolean mask of {n_ref} rows"):
        call(zones=FeatureZones(None, np.ones(n_ref + 1, bool), None, None, [0, 1]), **ok)
    with pytest.raises(ValueError, match="must not decrease"):
        call(zones=FeatureZones(None, None, None, None, [0, 30, 15]), **ok)
    with pytest.raises(ValueError, match="score_params"):
        call(score_params={"nodes": 1}, **ok)
    with pytest.raises(ValueError, match="unpack must be None or one of"):
        same_amd.score_unpacked_features(_table, ref, mov, "closest", **ok)
    with pytest.raises(ValueError, match="strategy must be"):
        same_amd.score_unpacked_features(_table, ref, mov, None, **ok)


def test_the_new_entry_points_are_declared_bound_and_exported_at_abi_9():
    import same_amd
    from same_amd import _lib
    from same_amd import windows as W

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert re.search(r"^#define SAME_ABI_VERSION 9$", header, re.M)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\b{name}\(", header), name
    assert header.index("same_merge_acc_unpack_detail(") < header.index("same_unpack_features_create(")
    assert "SAME_UNPACK_FEATURE_WORDS" in header
    for name in ("DeviceUnpackFeatures", "DeviceUnpackZone"):
        assert hasattr(W, name)
    assert hasattr(W.MergeAccumulator, "unpack_features") and "score_unpacked_features" in same_amd.__all__
    code = open(os.path.join(ROOT, "same_amd", "csrc", "window_unpack_feature.hip")).read()
    assert "__global__" not in code                                  # the kernels are stated once, in feature_kernels.h
    assert open(os.path.join(ROOT, "same_amd", "csrc", "window_score_feature.hip")).read().count("__global__") == 0
