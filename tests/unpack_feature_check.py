"""same_merge_acc_unpack_features (csrc/window_unpack_feature.hip) stated in plain numpy over tests/unpack_check.py's pairs -- nothing of
the library in it -- and the inputs its tests run over.  Not collected by pytest; tests/test_unpack_feature_check_cpu.py proves every
family has its property without a GPU.

The statement: `host_unpack`'s pairs (scipy's cdist, np.tile and linear_sum_assignment from the reference's text); per pair the moving
MEMBER's and the reference MEMBER's int32 fixed-point rows side by side; their int64 sums per group of the moving member and per
distance bin of the subset pairs; the squared distance of a subset pair to the nearest zone pair as the minimum of dx*dx + dy*dy in
float64 over the reference members' XY; the bin by thresholds on that square (edges[b] < d2 <= edges[b+1]).  d2 and the reference member
are per PAIR, in `host_unpack`'s pair order."""
import collections

import numpy as np

import feature_check as C
import unpack_check as U

Want = collections.namedtuple("Want", "out d2 ref_member mov_member")
# families that hold one distance bin by their definition: without a zone pair every d2 is NaN (bin B); a pair that is both has d2 = 0,
# which (0, ...] leaves out (bin B) -- NULL flags make every pair both; the far corner's zone lies 1e5 away from every subset pair in
# both coordinates, so every d2 is about 2e10, between the family's edges 1e10 and 3e10 (the family is there for the walk across the grid)
ONE_BIN_FAMILIES = ("no zone pair", "every pair both", "NULL flags", "far corner")


def moving_members(a_row, mov_off):
    """the flat moving member of every pair, in the pairs' order: final row by final row, the moving row's members in their order"""
    a = np.asarray(a_row, np.int64)
    mov_off = np.asarray(mov_off, np.int64)
    n_a = mov_off[a + 1] - mov_off[a]
    within = np.arange(int(n_a.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_a) - n_a, n_a)
    return np.repeat(mov_off[a], n_a) + within


def out_words(G, F, B=0):
    """SAME_UNPACK_FEATURE_WORDS"""
    return 4 + 4 + (G + 1) * (1 + F) + ((B + 1) * (1 + F) if B > 0 else 0)


def host_unpack_features(a_row, r_row, fam, strategy, mov_q, ref_q, member_group, n_groups, zone=None, unpacked=None):
    """-> Want(the call's `out` as one int64 array in the header's order, d2 per pair (None without a zone), the reference member per
    pair, the moving member per pair).  mov_q / ref_q: int32 (members, F_m) / (members, F_r); member_group: int32 per moving member or
    None; zone: (moving member flags or None, reference member flags or None, d2_edges); `unpacked`: host_unpack's answer, if the
    caller has it"""
    counts, ref_member = unpacked if unpacked is not None else U.host_unpack(a_row, r_row, *fam, strategy)
    i, j = moving_members(a_row, fam.mov_off), np.asarray(ref_member, np.int64)
    assert len(i) == len(j) == counts[1]
    G, n = int(n_groups), len(i)
    g = np.zeros(n, np.int64) if member_group is None else np.asarray(member_group, np.int64)[i]
    g = np.where((g < 0) | (g >= G), G, g)
    q = np.concatenate((np.asarray(mov_q, np.int64)[i], np.asarray(ref_q, np.int64)[j]), axis=1)
    rows = np.bincount(g, minlength=G + 1).astype(np.int64)
    sums = np.zeros((G + 1, q.shape[1]), np.int64)
    np.add.at(sums, g, q)
    head = np.array([n, n - rows[G], 0, 0], np.int64)
    if zone is None:
        return Want(np.concatenate((counts, head, rows, sums.reshape(-1))), None, j, i)
    mov_flags, ref_flags, d2_edges = zone
    mf = np.full(n, 3, np.uint8) if mov_flags is None else np.asarray(mov_flags, np.uint8)[i]
    rf = np.full(n, 3, np.uint8) if ref_flags is None else np.asarray(ref_flags, np.uint8)[j]
    f = mf & rf
    is_zone, is_subset = (f & 1) != 0, (f & 2) != 0
    xy = np.asarray(fam.ref_xy, np.float64).reshape(-1, 2)[j]
    d2 = C.zone_d2(xy[is_subset], xy[is_zone])
    d2[is_zone[is_subset]] = 0.0
    B = len(d2_edges) - 1
    b = C.bins_of(d2, d2_edges)
    bin_rows = np.bincount(b, minlength=B + 1).astype(np.int64)
    bin_sums = np.zeros((B + 1, q.shape[1]), np.int64)
    np.add.at(bin_sums, b, q[is_subset])
    head[2:] = int(is_zone.sum()), int(is_subset.sum())
    d2_pair = np.full(n, np.nan)
    d2_pair[is_subset] = d2
    return Want(np.concatenate((counts, head, rows, sums.reshape(-1), bin_rows, bin_sums.reshape(-1))), d2_pair, j, i)


def parts(out, G, F, B=0):
    """the words by name"""
    out = np.asarray(out, np.int64)
    assert len(out) == out_words(G, F, B)
    at = np.cumsum([0, 4, 4, G + 1, (G + 1) * F] + ([B + 1, (B + 1) * F] if B > 0 else []))
    p = lambda k: out[at[k]:at[k + 1]]
    got = {"unpack": p(0), "counts": p(1), "rows": p(2), "sums": p(3).reshape(G + 1, F)}
    if B > 0:
        got.update(bin_rows=p(4), bin_sums=p(5).reshape(B + 1, F))
    return got


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def member_features(fam, F_m, F_r, seed, floats=True):
    """(int32 (moving members, F_m), int32 (reference members, F_r)): quantised float columns, or integers over the whole range"""
    m_m, m_r = len(fam.mov_code), len(fam.ref_code)
    if floats:
        return C.quantize(C.float_columns(m_m, F_m, seed))[0], C.quantize(C.float_columns(m_r, F_r, seed + 1))[0]
    return C.int_columns(m_m, F_m, seed), C.int_columns(m_r, F_r, seed + 1)


def member_groups(fam, G, seed):
    """int32 group per moving member in [0, G), every seventh without one"""
    return C.groups(len(fam.mov_code), G, seed)


def member_zone_families(a_row, r_row, fam, seed=3):
    """§5.19's zone families restated on members: [(name, the family with the reference members' XY the zone needs, (moving member flags,
    reference member flags, d2_edges))].  The families are laid over the DISTRIBUTE pairs (which read no XY); under NEAREST the new XY
    moves the pairs, and the statement follows them."""
    _counts, j = U.host_unpack(a_row, r_row, *fam, U.DISTRIBUTE)
    i = moving_members(a_row, fam.mov_off)
    out = []
    for name, z in C.zone_families(i, j, len(fam.mov_code), len(fam.ref_code), seed=seed):
        assert z.ref_xy.shape == fam.ref_xy.shape and np.isfinite(z.ref_xy).all()
        out.append((name, fam._replace(ref_xy=np.ascontiguousarray(z.ref_xy, np.float64)), (z.mov_flags, z.ref_flags, z.d2_edges)))
    return out


def check_not_vacuous(want, fam, a_row, r_row, G, F, B=0, zone_name=None):
    """the properties a family's answer must have for its test to test anything"""
    p = parts(want.out, G, F, B)
    if G >= 2:
        assert np.count_nonzero(p["rows"][:G]) >= 2, "pairs in fewer than two groups"
    assert p["rows"][G] > 0, "no pair in the rest bin"
    na, nr = U.row_sizes(fam, a_row, r_row)
    assert (na > nr).any(), "no row with more moving than reference members: the tiling is not exercised"
    if B > 0 and zone_name not in ONE_BIN_FAMILIES:
        assert np.count_nonzero(p["bin_rows"]) >= 2, (zone_name, "pairs in fewer than two distance bins", p["bin_rows"].tolist())
