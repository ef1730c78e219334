"""The host statement of same_merge_acc_unpack (csrc/window_unpack.hip) and the member lists its tests run on.

`host_unpack` is written from the reference's text (src/metacell_utils.py:695-761) in plain numpy and scipy -- `cdist`, `np.tile`,
`linear_sum_assignment`, `i % nr` -- and nothing of libsame_hip is in it.  The families put hostile member lists on the rows a merged
accumulator's final rows name: tests/test_unpack_check_cpu.py checks each family has its property and holds the statement against the
reference and the oracle, tests/test_gpu_unpack_library.py holds the library call against the statement."""
import collections
import fractions

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

DISTRIBUTE, NEAREST = 0, 1
STRATEGIES = (DISTRIBUTE, NEAREST)

# the members of the two sections' rows: CSR offsets, per member XY and label code
Members = collections.namedtuple("Members", "mov_off mov_xy mov_code ref_off ref_xy ref_code")


def host_unpack(a_row, r_row, mov_off, mov_xy, mov_code, ref_off, ref_xy, ref_code, strategy):
    """-> (int64 counts [final rows, pairs, pairs whose codes are equal and non-negative, largest member count met], int64 per pair the
    flat index of its reference member).  ValueError: members against an empty reference list; scipy's own for an infeasible matrix."""
    picks, agree, most = [], 0, 0
    for a, r in zip(np.asarray(a_row).tolist(), np.asarray(r_row).tolist()):
        a0, a1, r0, r1 = int(mov_off[a]), int(mov_off[a + 1]), int(ref_off[r]), int(ref_off[r + 1])
        na, nr = a1 - a0, r1 - r0
        most = max(most, na, nr)
        if na == 0:
            continue
        if nr == 0:
            raise ValueError("members against an empty reference list")
        if strategy == DISTRIBUTE:
            local = np.arange(na) % nr
        else:
            distances = cdist(mov_xy[a0:a1], ref_xy[r0:r1])
            if na <= nr:
                row_ind, col_ind = linear_sum_assignment(distances)
            else:
                n_copies = int(np.ceil(na / nr))
                row_ind, col_ind = linear_sum_assignment(np.tile(distances, (1, n_copies)))
            assert row_ind.tolist() == list(range(na))
            local = col_ind % nr
        member = r0 + local
        cm, cr = mov_code[a0:a1], ref_code[member]
        agree += int(np.count_nonzero((cm >= 0) & (cm == cr)))
        picks.append(member)
    ref_member = np.concatenate(picks).astype(np.int64) if picks else np.zeros(0, np.int64)
    return np.array([len(a_row), len(ref_member), agree, most], np.int64), ref_member


def call(fam, a_row, r_row, strategy):
    return host_unpack(a_row, r_row, *fam, strategy)


def synthetic_rows(n_mov, n_ref, n_final, seed):
    """final rows as a merge leaves them: every moving row at most once, ascending; reference rows of their own"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.permutation(n_mov)[:n_final]).astype(np.int32), rng.permutation(n_ref)[:n_final].astype(np.int32)


# ---- the families -------------------------------------------------------------------------------------------------------------------------
def _build(rng, na_of, nr_of, xy=None, codes=None):
    """Members with `na_of[row]` / `nr_of[row]` members per moving / reference row; xy(rng, m) and codes(rng, m) make a side's arrays"""
    xy = xy or (lambda g, m: g.uniform(0.0, 50.0, (m, 2)))
    codes = codes or (lambda g, m: g.integers(0, 4, m).astype(np.int32))
    mov_off = np.concatenate(([0], np.cumsum(na_of))).astype(np.int64)
    ref_off = np.concatenate(([0], np.cumsum(nr_of))).astype(np.int64)
    m_m, m_r = int(mov_off[-1]), int(ref_off[-1])
    return Members(mov_off, np.ascontiguousarray(xy(rng, m_m), np.float64), codes(rng, m_m), ref_off,
                   np.ascontiguousarray(xy(rng, m_r), np.float64), codes(rng, m_r))


def _sizes(rng, a_row, r_row, n_mov, n_ref, na_final, nr_final):
    """member counts per row: 1 .. 3 on the rows no final row names, `na_final[i]` / `nr_final[i]` on final row i's two rows (a
    reference row two final rows name keeps the later one's)"""
    na_of, nr_of = rng.integers(1, 4, n_mov), rng.integers(1, 4, n_ref)
    na_of[a_row] = na_final
    nr_of[r_row] = nr_final
    return na_of, nr_of


def grid_sizes(n_final, seed=0):
    """every (na, nr) of 1..6 x 1..6, in a fixed shuffled order, repeated over the final rows"""
    combos = np.array([(na, nr) for na in range(1, 7) for nr in range(1, 7)])
    combos = combos[np.random.default_rng(seed).permutation(len(combos))]
    at = np.arange(n_final) % len(combos)
    return combos[at, 0], combos[at, 1]


def families(a_row, r_row, n_mov, n_ref, seed=0, library_only=False):
    """[(name, Members)] over sections of n_mov / n_ref rows whose merge left the final rows (a_row, r_row)"""
    a_row, r_row = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    n = len(a_row)
    rng = np.random.default_rng(seed)
    out = []
    na6, nr6 = grid_sizes(n)
    sizes6 = lambda: _sizes(rng, a_row, r_row, n_mov, n_ref, na6, nr6)
    out.append(("grid", _build(rng, *sizes6())))
    out.append(("lattice", _build(rng, *sizes6(), xy=lambda g, m: g.integers(0, 4, (m, 2)).astype(np.float64))))
    out.append(("coincident", _build(rng, *sizes6(), xy=lambda g, m: np.full((m, 2), 7.25))))
    out.append(("offset", _build(rng, *sizes6(), xy=lambda g, m: 1e9 + g.uniform(0.0, 50.0, (m, 2)))))
    out.append(("negative codes", _build(rng, *sizes6(), codes=lambda g, m: g.integers(-2, 2, m).astype(np.int32))))
    na0 = na6.copy()
    na0[::3] = 0
    na_of, nr_of = _sizes(rng, a_row, r_row, n_mov, n_ref, na0, nr6)
    unnamed = np.setdiff1d(np.arange(n_ref), r_row)
    nr_of[unnamed[::2]] = 0                     # reference rows without members that no final row names
    out.append(("empty moving rows", _build(rng, na_of, nr_of)))
    nab, nrb = na6.copy(), nr6.copy()
    big = [(64, 64), (64, 5), (5, 64)] + ([(96, 40)] if library_only else [])
    spots = _distinct_spots(r_row, len(big))
    for q, (na, nr) in zip(spots, big):
        nab[q], nrb[q] = na, nr
    out.append(("large lists" + (" and 96 x 40" if library_only else ""), _build(rng, *_sizes(rng, a_row, r_row, n_mov, n_ref, nab, nrb))))
    return out


def _distinct_spots(r_row, count):
    """final rows whose reference row no other final row names (so the size put there stays)"""
    _u, first, counts = np.unique(r_row, return_index=True, return_counts=True)
    spots = np.sort(first[counts == 1])[:count]
    assert len(spots) == count, "too few final rows with a reference row of their own"
    return spots.tolist()


# ---- the families' properties ---------------------------------------------------------------------------------------------------------------
def row_sizes(fam, a_row, r_row):
    return np.diff(fam.mov_off)[np.asarray(a_row)], np.diff(fam.ref_off)[np.asarray(r_row)]


def tied_rows(fam, a_row, r_row):
    """final rows whose (untiled) distance matrix holds a value twice"""
    n = 0
    for a, r in zip(np.asarray(a_row).tolist(), np.asarray(r_row).tolist()):
        d = cdist(fam.mov_xy[fam.mov_off[a]:fam.mov_off[a + 1]], fam.ref_xy[fam.ref_off[r]:fam.ref_off[r + 1]])
        n += d.size > 1 and len(np.unique(d)) < d.size
    return n


def rounded_squares(fam, a_row, r_row, limit=50):
    """pairs (of the first `limit` final rows) whose dx*dx + dy*dy is not the exact sum: the operation order is visible there"""
    n = 0
    for a, r in list(zip(np.asarray(a_row).tolist(), np.asarray(r_row).tolist()))[:limit]:
        for p in fam.mov_xy[fam.mov_off[a]:fam.mov_off[a + 1]]:
            for q in fam.ref_xy[fam.ref_off[r]:fam.ref_off[r + 1]]:
                dx, dy = float(p[0]) - float(q[0]), float(p[1]) - float(q[1])
                exact = fractions.Fraction(dx) ** 2 + fractions.Fraction(dy) ** 2
                n += fractions.Fraction(dx * dx + dy * dy) != exact
    return n
