"""tests/unpack_feature_check.py without a GPU: the means the statement's sums give stay within §5.19's bound of math.fsum's over the
cell pairs, sqrt(d2) is scipy's cdist(...).min(axis=1) over the reference members' XY bit for bit, the bins are pd.cut's, the group means
are `groupby().mean()` of the quantised values over `score_unpacked`'s table, and every family has the properties its tests rely on."""
import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import cdist

import feature_check as C
import unpack_check as U
import unpack_feature_check as UF
from test_unpack_check_cpu import _objects

N_MOV, N_REF, N_FINAL = 400, 380, 300


@pytest.fixture(scope="module")
def rows():
    return U.synthetic_rows(N_MOV, N_REF, N_FINAL, 5)


@pytest.fixture(scope="module")
def fams(rows):
    return U.families(*rows, N_MOV, N_REF, seed=11)


def test_means_of_the_statements_sums_stay_within_the_bound_of_fsum(rows, fams):
    a_row, r_row = rows
    for name, fam in fams[:2] + fams[-2:]:
        x_m, x_r = C.float_columns(len(fam.mov_code), 6, 1), C.float_columns(len(fam.ref_code), 7, 2)
        x_r[5, 5] = 1e9                                   # one huge outlier: the bound grows with it, and holds
        (mov_q, e_m), (ref_q, e_r) = C.quantize(x_m), C.quantize(x_r)
        e = np.concatenate((e_m, e_r))
        g = UF.member_groups(fam, 3, 2)
        for s in U.STRATEGIES:
            want = UF.host_unpack_features(a_row, r_row, fam, s, mov_q, ref_q, g, 3)
            p = UF.parts(want.out, 3, 13)
            gp = np.where(g[want.mov_member] < 0, 3, g[want.mov_member])
            for b in range(4):
                at = np.flatnonzero(gp == b)
                assert len(at) == p["rows"][b] > 0
                got = C.means(p["sums"][b], len(at), e)
                true = np.concatenate((C.fsum_means(x_m, want.mov_member[at]), C.fsum_means(x_r, want.ref_member[at])))
                err, bound = np.abs(got - true), C.mean_bound(e, true)
                assert (err <= bound).all(), (name, s, b, (err / bound).max())


def test_sqrt_of_d2_is_cdist_min_over_the_reference_members_bit_for_bit_and_the_bins_are_pd_cuts(rows, fams):
    from same_amd.score_features import d2_threshold

    a_row, r_row = rows
    fam = fams[0][1]
    mov_q, ref_q = np.zeros((len(fam.mov_code), 1), np.int32), np.zeros((len(fam.ref_code), 1), np.int32)
    seen = 0
    for name, zfam, zone in UF.member_zone_families(a_row, r_row, fam):
        dist_edges = np.sqrt(np.asarray(zone[2]))
        thresholds = np.array([d2_threshold(e) for e in dist_edges])
        for s in U.STRATEGIES:
            want = UF.host_unpack_features(a_row, r_row, zfam, s, mov_q, ref_q, None, 1, (zone[0], zone[1], thresholds))
            i, j = want.mov_member, want.ref_member
            f = (np.full(len(i), 3, np.uint8) if zone[0] is None else zone[0][i]) & (np.full(len(j), 3, np.uint8) if zone[1] is None else zone[1][j])
            is_zone, only_subset = (f & 1) != 0, (f & 3) == 2
            assert np.isnan(want.d2[(f & 2) == 0]).all() and not want.d2[is_zone & ((f & 2) != 0)].any()
            B = len(thresholds) - 1
            if is_zone.any() and only_subset.any():
                nearest = cdist(zfam.ref_xy[j[only_subset]], zfam.ref_xy[j[is_zone]]).min(axis=1)     # the notebook's cell 20
                assert C.same_bits(np.sqrt(want.d2[only_subset]), nearest), (name, s)
                codes = pd.cut(nearest, dist_edges).codes.astype(np.int64)                             # cells 21-22
                codes = np.where(codes < 0, B, codes)
                both = int((is_zone & ((f & 2) != 0)).sum())                                           # d2 = 0: pd.cut(0, (0, ...]) is in no bin
                want_rows = np.bincount(codes, minlength=B + 1)
                want_rows[B] += both
                assert UF.parts(want.out, 1, 2, B)["bin_rows"].tolist() == want_rows.tolist(), (name, s)
                seen += name == "lattice ties" and len(np.unique(nearest)) < len(nearest) / 4
    assert seen == 2                                      # lattice ties under both strategies


def test_every_family_has_the_properties_its_tests_rely_on(rows, fams):
    a_row, r_row = rows
    for name, fam in fams:
        mov_q, ref_q = UF.member_features(fam, 2, 3, 4)
        g = UF.member_groups(fam, 3, 5)
        for s in U.STRATEGIES:
            UF.check_not_vacuous(UF.host_unpack_features(a_row, r_row, fam, s, mov_q, ref_q, g, 3), fam, a_row, r_row, 3, 5)
        zones = UF.member_zone_families(a_row, r_row, fam)
        assert [n for n, _f, _z in zones] == ["scattered", "no zone pair", "one zone point", "every pair both", "NULL flags", "coincident zone",
                                              "lattice ties", "far corner", "3-4-5", "B = 1", "B = 64", "reference flags"]
        for zname, zfam, zone in zones:
            want = UF.host_unpack_features(a_row, r_row, zfam, U.DISTRIBUTE, mov_q, ref_q, g, 3, zone)
            UF.check_not_vacuous(want, zfam, a_row, r_row, 3, 5, len(zone[2]) - 1, zname)
            p = UF.parts(want.out, 3, 5, len(zone[2]) - 1)
            assert p["bin_rows"].sum() == p["counts"][3] and p["rows"].sum() == p["counts"][0] == want.out[1], (name, zname)
            if zname == "no zone pair":
                assert p["counts"][2] == 0 and p["counts"][3] > 0 and np.isnan(want.d2).all() and p["bin_rows"][-1] == p["counts"][3]
            if zname in ("every pair both", "NULL flags"):
                assert p["counts"][2] == p["counts"][3] == want.out[1] and not want.d2.any()


def test_the_statement_on_a_case_small_enough_to_read():
    """two final rows: (moving row 0: members 0, 1, 2; reference row 1: member 2) and (moving row 1: member 3; reference row 0: members
    0, 1).  DISTRIBUTE: pairs (0, 2), (1, 2), (2, 2), (3, 0).  Cell 1 has no group; member 3's pair is the zone, the others the subset"""
    fam = U.Members(np.array([0, 3, 4]), np.zeros((4, 2)), np.array([0, 1, 0, 1], np.int32), np.array([0, 2, 3]),
                    np.array([[30.0, 40.0], [9.0, 9.0], [27.0, 44.0]]), np.array([1, 1, 0], np.int32))
    mov_q, ref_q = np.array([[1], [10], [100], [1000]], np.int32), np.array([[7], [-1], [-2]], np.int32)
    zone = (np.array([2, 2, 2, 1], np.uint8), None, np.array([0.0, 25.0, 100.0]))
    want = UF.host_unpack_features([0, 1], [1, 0], fam, U.DISTRIBUTE, mov_q, ref_q, np.array([0, -1, 1, 1], np.int32), 2, zone)
    assert want.out.tolist() == [2, 4, 3, 3,   4, 3, 1, 3,   1, 2, 1,   1, -2, 1100, 5, 10, -2,   3, 0, 0,   111, -6, 0, 0, 0, 0]
    assert C.same_bits(want.d2, [25.0, 25.0, 25.0, np.nan]) and want.ref_member.tolist() == [2, 2, 2, 0] and want.mov_member.tolist() == [0, 1, 2, 3]


def test_the_group_means_are_groupby_mean_of_the_quantised_values_over_score_unpackeds_table(strategy="distribute"):
    """examples/luad/reproduce_figures.ipynb cells 12, 16, 18 in pandas over hand-made objects: the cell pairs of `score_unpacked`, both
    sides' rows gathered, the mean per annotation of the moving cell -- of the quantised values, so the comparison is exact up to the
    one division.  ('nearest' solves on the device: tests/test_gpu_unpack_score_features.py holds it to the same cells.)"""
    import same_amd
    from same_amd.score_features import quantize_features

    ref, mov, table = _objects()
    rng = np.random.default_rng(3)
    mov.original_df["CD8"] = rng.lognormal(0, 2, len(mov.original_df))
    ref.original_df["SFTPC"], ref.original_df["PDCD1"] = rng.normal(0, 3, len(ref.original_df)), rng.poisson(2.0, len(ref.original_df))
    got = same_amd.score_unpacked_features(table, ref, mov, strategy, moving_features=["CD8"], ref_features=["SFTPC", "PDCD1"])
    _rec, cells = same_amd.score_unpacked(table, ref, mov, strategy)
    pcf, xen = mov.original_df.set_index("Cell_Num_Old"), ref.original_df.set_index("Cell_Num_Old")
    (q_m, e_m), (q_r, e_r) = quantize_features(pcf[["CD8"]].to_numpy()), quantize_features(xen[["SFTPC", "PDCD1"]].to_numpy())
    combined = pd.concat([pd.DataFrame(np.ldexp(q_m.astype(np.float64), -e_m), index=pcf.index, columns=["moving_CD8"])
                          .loc[cells["Aligned_cell_id"]].reset_index(drop=True),
                          pd.DataFrame(np.ldexp(q_r.astype(np.float64), -e_r), index=xen.index, columns=["ref_SFTPC", "ref_PDCD1"])
                          .loc[cells["Ref_cell_id"]].reset_index(drop=True)], axis=1)
    combined["pcf_Annotations"] = pcf["cell_type"].loc[cells["Aligned_cell_id"]].to_numpy()
    by = combined.groupby("pcf_Annotations", sort=False)
    assert got.rows.sum() == len(cells) == 100 and len(got.rows) >= 2
    assert got.rows.to_dict() == by.size().to_dict()
    want = by.mean().loc[got.means.index]
    np.testing.assert_allclose(got.means.to_numpy(), want.to_numpy(), rtol=4 * 2.0**-53 * len(cells), atol=0)
    assert list(got.means.columns) == ["moving_CD8", "ref_SFTPC", "ref_PDCD1"] and got.zones is None and got.pairs is None
