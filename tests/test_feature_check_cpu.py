"""tests/feature_check.py without a GPU: every family has the property it is named for, the means the statement's sums give stay within
the derived bound of math.fsum's, sqrt(d2) is scipy's cdist(...).min(axis=1) bit for bit, and the edge helper of the package
(score_features.d2_threshold) bins squared distances exactly as pd.cut bins the distances."""
import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import cdist

import feature_check as C


def _pairs(n=600, n_mov=700, n_ref=650, seed=1):
    """pairs with every moving row and every reference row named at most once, as a merge's final rows name them"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n_mov, n, replace=False)), rng.choice(n_ref, n, replace=False), n_mov, n_ref


def test_feature_families_have_their_properties():
    x = C.float_columns(500, 11, 0)
    assert np.isfinite(x).all() and not x[:, 0].any() and (x[:, 3] < 1e-199).all() and (x[:, 4] < 0).any()
    assert np.array_equal(x[:, 1], x[:, 1].astype(np.float32)) and np.array_equal(x[:, 2], np.rint(x[:, 2]))
    q, e = C.quantize(x)
    assert q.dtype == np.int32 and np.abs(q.astype(np.int64)).max() <= C.Q_MAX and e[0] == 0 and not q[:, 0].any()
    assert (np.abs(q.astype(np.int64)).max(axis=0)[1:] >= C.Q_MAX // 2).all()          # every column uses its top bit
    assert e[3] > 600                                                                    # the tiny column keeps 30 bits
    q = C.int_columns(64, 3, 1)
    assert q.max() == C.Q_MAX and q.min() == -C.Q_MAX
    g = C.groups(100, 4, 2)
    assert (g == -1).any() and (g == -2**31).any() and set(g[g >= 0].tolist()) == {0, 1, 2, 3}
    # a power of two sits on the upper end: frexp(2**k) = (0.5, k + 1), so q = 2**29, never above 2**30
    q, e = C.quantize(np.array([[1.0], [-2.0], [1.999999]]))
    assert e[0] == 28 and q[:, 0].tolist() == [2**28, -2**29, round(1.999999 * 2**28)]


def test_means_of_the_statements_sums_stay_within_the_derived_bound_of_fsum():
    x = C.float_columns(5000, 20, 4)
    x[17, 5] = 1e9                                        # one huge outlier: the bound grows with it, and holds
    q, e = C.quantize(x)
    for rows in (np.arange(5000), np.arange(0, 5000, 7), np.array([3])):
        got = C.means(q[rows].astype(np.int64).sum(axis=0), len(rows), e)
        want = C.fsum_means(x, rows)
        err, bound = np.abs(got - want), C.mean_bound(e, want)
        assert (err <= bound).all(), (err / bound).max()
    # the outlier column's small values are lost to its resolution, as the package says
    assert np.ldexp(1.0, -int(e[5])) > 0.5


def test_sqrt_of_d2_is_cdist_min_bit_for_bit():
    rng = np.random.default_rng(5)
    for scale in (1.0, 1e-3, 1e6):
        xy, zone = rng.random((900, 2)) * 2000 * scale, rng.random((400, 2)) * 2000 * scale
        zone[::9] = np.rint(zone[::9] / (8 * scale)) * 8 * scale              # lattice ties among the zone points
        xy[::4] = np.rint(xy[::4] / (8 * scale)) * 8 * scale
        assert C.same_bits(np.sqrt(C.zone_d2(xy, zone)), cdist(xy, zone).min(axis=1)), scale
    assert np.isnan(C.zone_d2(rng.random((5, 2)), np.zeros((0, 2)))).all()


def test_zone_families_have_their_properties():
    a, r, n_mov, n_ref = _pairs()
    fams = dict(C.zone_families(a, r, n_mov, n_ref))
    assert list(fams) == ["scattered", "no zone pair", "one zone point", "every pair both", "NULL flags", "coincident zone", "lattice ties",
                          "far corner", "3-4-5", "B = 1", "B = 64", "reference flags"]
    zero_m, zero_r = np.zeros((n_mov, 1), np.int32), np.zeros((n_ref, 1), np.int32)

    def read(name):
        z = fams[name]
        assert np.isfinite(z.ref_xy).all() and z.ref_xy.shape == (n_ref, 2) and (np.diff(z.d2_edges) >= 0).all()
        out, d2 = C.host_features(a, r, n_mov, zero_m, zero_r, None, 1, z.ref_xy, (z.mov_flags, z.ref_flags, z.d2_edges))
        B = len(z.d2_edges) - 1
        at = 4 + 2 + 2 * 2                                   # counts, rows of one group and the rest, their sums over two columns
        return out[2], out[3], out[at:at + B + 1], d2[a]

    nz, ns, bins, d2 = read("scattered")
    assert 0 < nz < ns < len(a) and bins.sum() == ns and (bins[1:3] > 0).all() and np.isnan(d2).sum() == len(a) - ns
    nz, ns, bins, d2 = read("no zone pair")
    assert nz == 0 and ns > 0 and bins.tolist() == [0, 0, 0, ns] and np.isnan(d2).all()
    nz, ns, bins, d2 = read("one zone point")
    assert nz == 1 and ns == len(a) and (d2 == 0).sum() == 1 and bins[3] == 1          # d2 = 0 is in no bin of (0, ...]
    for name in ("every pair both", "NULL flags"):
        nz, ns, bins, d2 = read(name)
        assert nz == ns == len(a) and not d2.any() and bins.tolist() == [0, 0, 0, len(a)]
    nz, ns, bins, d2 = read("coincident zone")
    z = fams["coincident zone"]
    assert nz > 1 and len(np.unique(z.ref_xy[r[(z.mov_flags[a] & 1) != 0]], axis=0)) == 1 and nz + ns == len(a)
    nz, ns, bins, d2 = read("lattice ties")
    sub = d2[~np.isnan(d2)]
    assert set(sub.tolist()) <= {64.0 * k for k in range(400)} and (sub == 64.0).sum() > 10 and bins[0] == (sub == 64.0).sum()
    nz, ns, bins, d2 = read("far corner")
    assert nz >= 1 and np.nanmin(d2) > 1e9 and bins[3] + bins[4] < ns
    nz, ns, bins, d2 = read("3-4-5")
    sub = d2[~np.isnan(d2)]
    assert (sub == 25.0).sum() >= 4 * (len(sub) // 6) and (sub > 25.0).any() and bins[0] == (sub == 25.0).sum() and bins[2] == 0
    assert 25.0 < sorted(set(sub.tolist()))[1] < 25.0 + 1e-10                           # just above the edge: the next bin
    nz, ns, bins, d2 = read("B = 1")
    assert len(bins) == 2 and bins.sum() == ns and bins[0] > 0 and bins[1] > 0
    nz, ns, bins, d2 = read("B = 64")
    assert len(bins) == 65 and bins.sum() == ns and (bins[:64] > 0).sum() > 20
    assert read("reference flags")[:2] == read("scattered")[:2]                         # (unique reference rows: the same classes)
    # an empty set of pairs goes through every family
    for name, z in C.zone_families(a[:0], r[:0], n_mov, n_ref):
        out, d2 = C.host_features(a[:0], r[:0], n_mov, np.zeros((n_mov, 1), np.int32), np.zeros((n_ref, 1), np.int32), None, 1, z.ref_xy,
                                  (z.mov_flags, z.ref_flags, z.d2_edges))
        assert not out.any() and np.isnan(d2).all(), name


def test_the_statement_on_a_case_small_enough_to_read():
    """three pairs, two groups, one column a side: pair 0 is zone, pair 1 subset at distance 5, pair 2 subset and in no group"""
    a, r = np.array([0, 2, 3]), np.array([1, 0, 2])
    mov_q, ref_q = np.array([[1], [50], [10], [100]], np.int32), np.array([[7], [-2], [1000]], np.int32)
    ref_xy = np.array([[3.0, 4.0], [0.0, 0.0], [30.0, 40.0]])
    out, d2 = C.host_features(a, r, 4, mov_q, ref_q, np.array([0, 1, 1, -1], np.int32), 2, ref_xy,
                              (np.array([1, 0, 2, 2], np.uint8), None, np.array([0.0, 25.0, 100.0])))
    assert out.tolist() == [3, 2, 1, 2,   1, 1, 1,   1, -2, 10, 7, 100, 1000,   1, 0, 1,   10, 7, 0, 0, 100, 1000]
    assert C.same_bits(d2, [np.nan, np.nan, 25.0, 2500.0])


@pytest.mark.parametrize("edges", [(0, 15, 30, np.inf), (0, 0.1, 1 / 3, 7.3), (1e-160, 1.0), (2.5, 2.5000000000000004, 1e200)])
def test_the_edge_helper_bins_squares_as_pd_cut_bins_distances(edges):
    from same_amd.score_features import d2_threshold

    edges = np.asarray(edges, np.float64)
    t = np.array([d2_threshold(e) for e in edges])
    cand = []
    for e in edges[np.isfinite(edges)]:
        for d in (np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)):           # distances on, one ulp below and above the edge ...
            sq = np.float64(d) * np.float64(d)
            for _ in range(4):
                sq = np.nextafter(sq, -np.inf)
            for _ in range(9):                                                       # ... and the squares around theirs
                cand.append(sq)
                sq = np.nextafter(sq, np.inf)
    d2 = np.array([c for c in cand if c >= 0] + [0.0, np.inf, np.nan])
    for e, th in zip(edges, t):
        assert np.array_equal(d2 <= th, np.sqrt(d2) <= e), e
    got = C.bins_of(d2, t)
    want = pd.cut(np.sqrt(d2), edges).codes.astype(np.int64)
    assert np.array_equal(got, np.where(want < 0, len(edges) - 1, want))
    assert d2_threshold(-1.0) == -np.inf and d2_threshold(0.0) == 0.0 and d2_threshold(np.inf) == np.inf
    with pytest.raises(ValueError):
        d2_threshold(np.nan)
