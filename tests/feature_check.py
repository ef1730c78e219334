"""same_merge_acc_score_features (csrc/window_score_feature.hip) stated in plain numpy -- nothing of the library in it -- and the inputs
its tests run over.  Not collected by pytest; tests/test_feature_check_cpu.py proves every family has its property without a GPU.

The statement: fixed-point columns (per column m = max |x|, p = frexp(m)[1], e = 30 - p, q = rint(ldexp(x, e))), their int64 sums per
group of the moving rows and per distance bin of the subset pairs, the squared distance of a subset pair to the nearest zone pair as
the minimum of dx*dx + dy*dy in float64, the bin by thresholds on that square (edges[b] < d2 <= edges[b+1])."""
import collections
import math

import numpy as np

Q_MAX = 1 << 30
Zone = collections.namedtuple("Zone", "ref_xy mov_flags ref_flags d2_edges")     # a zone family: the reference XY it needs, the call's inputs


# ---- the statement -------------------------------------------------------------------------------------------------------------------------
def quantize(x):
    """-> (int32 (n, F), int32 e (F,)) of the float64 matrix x"""
    x = np.asarray(x, np.float64)
    m = np.abs(x).max(axis=0) if len(x) else np.zeros(x.shape[1])
    e = np.where(m > 0, 30 - np.frexp(m)[1], 0).astype(np.int32)
    return np.rint(np.ldexp(x, e)).astype(np.int32), e


def means(sums, n, e):
    """ldexp(float64(sum) / n, -e)"""
    return np.ldexp(np.asarray(sums, np.int64).astype(np.float64) / float(n), -np.asarray(e, np.int32))


def mean_bound(e, mean):
    """the derived bound on |means(...) - true mean|: half a step per value, three roundings (the sum's conversion, the division, none
    in ldexp short of underflow)"""
    return np.ldexp(1.0, -np.asarray(e, np.int32) - 1) + 3 * 2.0**-53 * np.abs(mean)


def zone_d2(xy, zone_xy):
    """min over zone_xy of dx*dx + dy*dy per row of xy, float64; NaN without a zone point"""
    xy, zone_xy = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(zone_xy, np.float64).reshape(-1, 2)
    out = np.full(len(xy), np.nan)
    if len(zone_xy):
        for lo in range(0, len(xy), 512):
            dx = xy[lo:lo + 512, None, 0] - zone_xy[None, :, 0]
            dy = xy[lo:lo + 512, None, 1] - zone_xy[None, :, 1]
            out[lo:lo + 512] = (dx * dx + dy * dy).min(axis=1)
    return out


def bins_of(d2, d2_edges):
    """bin b with d2_edges[b] < d2 <= d2_edges[b+1]; B (= len - 1) for a d2 in none, NaN among them"""
    d2, e = np.asarray(d2, np.float64), np.asarray(d2_edges, np.float64)
    B = len(e) - 1
    out = np.full(len(d2), B, np.int64)
    for b in range(B - 1, -1, -1):
        out[(d2 > e[b]) & (d2 <= e[b + 1])] = b
    return out


def _sums(bins, q, n_bins):
    rows = np.bincount(bins, minlength=n_bins).astype(np.int64)
    sums = np.zeros((n_bins, q.shape[1]), np.int64)
    np.add.at(sums, bins, q)
    return rows, sums


def host_features(a_row, r_row, n_mov, mov_q, ref_q, group_of, n_groups, ref_xy=None, zone=None):
    """-> (the call's `out` as one int64 array in the header's order, out_d2 per moving row or None without a zone).  mov_q / ref_q:
    int32 (rows, F_m) / (rows, F_r); group_of: int32 per moving row or None; zone: (mov_flags or None, ref_flags or None, d2_edges)"""
    a, r = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    G = int(n_groups)
    g = np.zeros(len(a), np.int64) if group_of is None else np.asarray(group_of, np.int64)[a]
    g = np.where((g < 0) | (g >= G), G, g)
    q = np.concatenate((np.asarray(mov_q, np.int64)[a], np.asarray(ref_q, np.int64)[r]), axis=1)
    rows, sums = _sums(g, q, G + 1)
    counts = np.array([len(a), len(a) - rows[G], 0, 0], np.int64)
    if zone is None:
        return np.concatenate((counts, rows, sums.reshape(-1))), None
    mov_flags, ref_flags, d2_edges = zone
    mf = np.full(len(a), 3, np.uint8) if mov_flags is None else np.asarray(mov_flags, np.uint8)[a]
    rf = np.full(len(a), 3, np.uint8) if ref_flags is None else np.asarray(ref_flags, np.uint8)[r]
    f = mf & rf
    is_zone, is_subset = (f & 1) != 0, (f & 2) != 0
    xy = np.asarray(ref_xy, np.float64).reshape(-1, 2)[r]
    d2 = zone_d2(xy[is_subset], xy[is_zone])
    d2[is_zone[is_subset]] = 0.0
    B = len(d2_edges) - 1
    bin_rows, bin_sums = _sums(bins_of(d2, d2_edges), q[is_subset], B + 1)
    counts[2:] = int(is_zone.sum()), int(is_subset.sum())
    out_d2 = np.full(int(n_mov), np.nan)
    out_d2[a[is_subset]] = d2
    return np.concatenate((counts, rows, sums.reshape(-1), bin_rows, bin_sums.reshape(-1))), out_d2


def same_bits(x, y):
    """float64 arrays equal bit for bit, every NaN counted as one value"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and bool(np.array_equal(np.where(np.isnan(x), np.nan, x).view(np.uint64), np.where(np.isnan(y), np.nan, y).view(np.uint64)))


# ---- feature families ----------------------------------------------------------------------------------------------------------------------
def float_columns(n, F, seed):
    """float64 (n, F): lognormal, float32-valued, count, tiny-valued and signed columns in turn; column 0 of three or more is all zero"""
    rng = np.random.default_rng(seed)
    x = np.empty((n, F))
    for c in range(F):
        kind = c % 5
        if kind == 0:
            x[:, c] = rng.lognormal(0.0, 2.0, n)
        elif kind == 1:
            x[:, c] = rng.random(n).astype(np.float32)
        elif kind == 2:
            x[:, c] = rng.poisson(3.0, n)
        elif kind == 3:
            x[:, c] = rng.random(n) * 1e-200
        else:
            x[:, c] = rng.normal(0.0, 50.0, n)
    if F >= 3:
        x[:, 0] = 0.0
    return x


def int_columns(n, F, seed):
    """int32 (n, F) over the whole fixed-point range, both ends among them"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-Q_MAX, Q_MAX + 1, (n, F)).astype(np.int32)
    if n and F:
        q[0, 0], q[-1, -1] = Q_MAX, -Q_MAX
    return q


def groups(n, G, seed, none_every=7):
    """int32 group per row in [0, G), every `none_every`-th row without one (-1, or -2**31 on every other of those)"""
    g = np.random.default_rng(seed).integers(0, G, n).astype(np.int32)
    g[::none_every] = -1
    g[::2 * none_every] = -2**31
    return g


# ---- zone families -------------------------------------------------------------------------------------------------------------------------
# Each makes the reference XY of a reference section of n_ref rows -- finite everywhere -- and the flags over n_mov / n_ref rows; the
# pairs are (a_row[i], r_row[i]).  What decides a pair's class is stated in the moving flags, the reference flags are all set unless
# said otherwise, so a reference row that two moving rows share cannot blur it.
EDGES = np.array([0.0, 15.0 * 15.0, 30.0 * 30.0, np.inf])


def _flags(n_mov, a_row, is_zone, is_subset):
    f = np.zeros(n_mov, np.uint8)
    f[a_row] = is_zone.astype(np.uint8) | (is_subset.astype(np.uint8) << 1)
    return f


def _scattered(n_ref, seed, extent=2000.0):
    return np.random.default_rng(seed).random((n_ref, 2)) * extent


def zone_families(a_row, r_row, n_mov, n_ref, seed=3):
    """[(name, Zone)] over the pairs"""
    a, r = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    n = len(a)
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    ones_r = np.full(n_ref, 3, np.uint8)
    out = []
    xy = _scattered(n_ref, seed)
    fifth, tenth = rng.random(n) < 0.2, rng.random(n) < 0.5
    out.append(("scattered", Zone(xy, _flags(n_mov, a, fifth, tenth), ones_r, EDGES)))
    out.append(("no zone pair", Zone(xy, _flags(n_mov, a, np.zeros(n, bool), tenth), ones_r, EDGES)))
    one = np.zeros(n, bool)
    one[n // 2:n // 2 + 1] = True
    out.append(("one zone point", Zone(xy, _flags(n_mov, a, one, np.ones(n, bool)), ones_r, EDGES)))
    out.append(("every pair both", Zone(xy, _flags(n_mov, a, np.ones(n, bool), np.ones(n, bool)), ones_r, EDGES)))
    out.append(("NULL flags", Zone(xy, None, None, EDGES)))
    same = xy.copy()
    same[r[fifth]] = (777.0, 333.0)                               # all zone points coincident
    out.append(("coincident zone", Zone(same, _flags(n_mov, a, fifth, ~fifth), ones_r, EDGES)))
    lattice = np.zeros((n_ref, 2))
    lattice[r] = np.column_stack((i % 71, i // 71)) * 8.0         # an 8-unit lattice: every distance tied many times over
    out.append(("lattice ties", Zone(lattice, _flags(n_mov, a, i % 5 == 0, i % 5 != 0), ones_r, np.array([0.0, 64.0, 128.0, 1e4, np.inf]))))
    corner = xy.copy()
    far = i < max(1, n // 50)
    corner[r[far]] = 2000.0 + rng.random((int(far.sum()), 2)) * 5.0 + (1e5, 1e5)       # the zone in one far corner: the walk crosses the grid
    out.append(("far corner", Zone(corner, _flags(n_mov, a, far, ~far), ones_r, np.array([0.0, 1e9, 1e10, 3e10, np.inf]))))
    # 3-4-5: subset pair i sits (3, 4), (4, 3), (5, 0), (0, 5), (3, 4 + 2**-40) or (6, 8) off its zone point; an edge exactly at 25
    t345 = np.zeros((n_ref, 2))
    is_z = i % 2 == 0
    base = np.column_stack(((i // 2) * 100.0, np.zeros(n)))
    offs = np.array([(3.0, 4.0), (4.0, 3.0), (5.0, 0.0), (0.0, 5.0), (3.0, 4.0 + 2.0**-40), (6.0, 8.0)])[(i // 2) % 6]
    t345[r] = np.where(is_z[:, None], base, base + offs)
    out.append(("3-4-5", Zone(t345, _flags(n_mov, a, is_z, ~is_z), ones_r, np.array([0.0, 25.0, 100.0]))))
    out.append(("B = 1", Zone(xy, _flags(n_mov, a, fifth, tenth), ones_r, np.array([100.0, 4e4]))))
    out.append(("B = 64", Zone(xy, _flags(n_mov, a, fifth, tenth), ones_r, np.concatenate(([0.0], np.linspace(5.0, 300.0, 63) ** 2, [np.inf])))))
    # the reference flags decide: moving flags all set, a pair's class is its reference row's
    rf = np.zeros(n_ref, np.uint8)
    rf[r] = _flags(n, i, fifth, tenth)                            # (a reference row two pairs share keeps the later pair's)
    out.append(("reference flags", Zone(xy, np.full(n_mov, 3, np.uint8), rf, EDGES)))
    return out


def fsum_means(x, rows):
    """the true means of the float64 columns over `rows`, by math.fsum"""
    return np.array([math.fsum(x[rows, c].tolist()) / len(rows) for c in range(x.shape[1])])
