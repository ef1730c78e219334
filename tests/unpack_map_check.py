"""The host statement of same_merge_acc_unpack_map (csrc/window_unpack_map.hip) and what its tests read the marks against.

`host_unpack_map` is built on tests/unpack_check.py's `host_unpack` -- scipy's cdist, np.tile and linear_sum_assignment from the
reference's text -- with numpy for the marks; nothing of libsame_hip is in it.  A spec (tests/unpack_detail_check.py's `Spec`, its group
fields unused) says what the members are ranked by: the number of cell-level labels, the member codes (negative ones and codes at or
above the label count among them), the labels' type columns, the reference members' type rows.  A truth names per moving member a
reference member or -1.  tests/test_unpack_map_check_cpu.py checks that the specs and truths hold what they are made to hold and holds
the statement against a per-member Python loop; tests/test_gpu_unpack_map_library.py holds the library call against the statement."""
import collections

import numpy as np

import unpack_check as U
import unpack_detail_check as D

MATCHED, TYPE_MATCH, CONSIDERED, VIOLATING, TRUTH_KNOWN, ON_TRUTH, RANKED = 1, 2, 4, 8, 16, 32, 64       # SAME_MARK_*
UNRANKED, RANK_TOP = 255, 254
# same_member_mark
MARK = np.dtype([("ref_member", "<i4"), ("ref_row", "<i4"), ("pair", "<i4"), ("flags", "u1"), ("rank_strict", "u1"), ("rank_weak", "u1"),
                 ("reserved", "u1")])
assert MARK.itemsize == 16

# marks: MARK per moving member; counts: int64[6]; tally: uint32 (members, 3), what ONE call adds (matched, type-matched, on its truth)
MapAnswer = collections.namedtuple("MapAnswer", "marks counts tally")


def unmatched_marks(m_mov, truth_member=None):
    """{-1, -1, -1, TRUTH_KNOWN or 0, 255, 255, 0} per moving member"""
    marks = np.zeros(m_mov, MARK)
    marks["ref_member"] = marks["ref_row"] = marks["pair"] = -1
    marks["rank_strict"] = marks["rank_weak"] = UNRANKED
    if truth_member is not None:
        marks["flags"] = np.where(np.asarray(truth_member) >= 0, TRUTH_KNOWN, 0)
    return marks


def host_unpack_map(a_row, r_row, fam, strategy, spec=None, truth_member=None, unpacked=None):
    """-> MapAnswer for the final rows (a_row, r_row) and the family's lists -- under the spec's codes, ranked by its columns and type rows
    (None: the family's own codes, no ranks) --, read against `truth_member` (None: every member unknown).  `unpacked`: `host_unpack`'s
    answer for these lists and XY where it is known already (the pairs do not depend on the codes)."""
    if spec is not None:
        fam = D.with_codes(fam, spec)
    counts4, ref_member = unpacked if unpacked is not None else U.call(fam, a_row, r_row, strategy)
    mov_member, _row = D.pairs_of(a_row, fam, ref_member)
    m_mov = len(fam.mov_code)
    assert len(np.unique(mov_member)) == len(mov_member), "a merge's final rows name a moving row at most once"
    marks = unmatched_marks(m_mov, truth_member)
    tally = np.zeros((m_mov, 3), np.uint32)
    P = len(mov_member)
    cm, cr = fam.mov_code[mov_member].astype(np.int64), fam.ref_code[ref_member].astype(np.int64)
    agree = (cm >= 0) & (cm == cr)
    truth = np.full(m_mov, -1, np.int64) if truth_member is None else np.asarray(truth_member, np.int64)
    known = truth[mov_member] >= 0
    on = ref_member == truth[mov_member]
    flags = MATCHED | np.where(agree, TYPE_MATCH, 0) | np.where(known, TRUTH_KNOWN, 0) | np.where(on, ON_TRUTH, 0)
    strict_b, weak_b = np.full(P, UNRANKED, np.int64), np.full(P, UNRANKED, np.int64)
    if spec is not None and spec.col_of_label is not None and spec.ref_types is not None and P:
        L, T = spec.n_labels, spec.ref_types.shape[1]
        lm = (cm >= 0) & (cm < L)
        c = np.where(lm, spec.col_of_label[np.where(lm, cm, 0)], -1).astype(np.int64) if L else np.full(P, -1)
        rows = spec.ref_types[ref_member]
        typed = (c >= 0) & ~np.isnan(rows).any(axis=1)
        v = rows[np.arange(P), np.maximum(c, 0)]
        strict, weak = np.zeros(P, np.int64), np.zeros(P, np.int64)
        with np.errstate(invalid="ignore"):
            for t in range(T):
                other = c != t
                strict += other & (rows[:, t] > v)
                weak += other & (rows[:, t] >= v)
        strict_b = np.where(typed, np.minimum(strict, RANK_TOP), UNRANKED)
        weak_b = np.where(typed, np.minimum(weak, RANK_TOP), UNRANKED)
        flags = flags | np.where(typed, RANKED, 0)
    marks["ref_member"][mov_member] = ref_member
    # the reference row that owns the member: the last row whose list starts at or before it (rows without members own nothing)
    marks["ref_row"][mov_member] = np.searchsorted(fam.ref_off, ref_member, side="right") - 1
    marks["pair"][mov_member] = np.arange(P)
    marks["flags"][mov_member] = flags
    marks["rank_strict"][mov_member], marks["rank_weak"][mov_member] = strict_b, weak_b
    tally[mov_member, 0] = 1
    tally[mov_member, 1] = agree
    tally[mov_member, 2] = on
    counts = np.array([counts4[0], P, int(agree.sum()), counts4[3], int(known.sum()), int(on.sum())], np.int64)
    return MapAnswer(marks, counts, tally)


# ---- the specs -----------------------------------------------------------------------------------------------------------------------------
def specs(fam, seed=0):
    """[Spec] for the marks: tests/unpack_detail_check.py's -- T 1; L 5, T 2 with ties; L 64, T 17 with infinities, signed zeros and NaN
    rows; no label names a column -- and a T = 300 spec whose rows are 300 distinct values, so that ranks beyond 254 saturate"""
    rng = np.random.default_rng(1000 + seed)
    base = D.specs(fam, 1, seed=seed)
    out = [base[0], base[1], base[2], base[4]]
    m_m, m_r = len(fam.mov_code), len(fam.ref_code)
    side = lambda m: np.where(rng.random(m) < 0.1, -1, rng.integers(0, 6, m)).astype(np.int32)          # (5: at the label count)
    wide = np.argsort(rng.random((m_r, 300)), axis=1).astype(np.float64)                                # a permutation of 0 .. 299 per row
    out.append(D.Spec("L 5, T 300, ranks beyond 254", 5, side(m_m), side(m_r), np.array([0, 299, -1, 150, 7], np.int32), wide, None, 1,
                      {"pairs", "saturated"}))
    return out


def truths(fam, a_row, r_row, seed=0):
    """int32 per moving member.  On a final row (a, r) member k of a's list cycles through: -1; member k % nr of r's list (the member
    DISTRIBUTE gives it); member (k + 1) % nr of r's list (the right row, with nr > 1 another member); a member of another reference
    row.  Members of rows no final row names: every other one a random member, the others -1."""
    rng = np.random.default_rng(2000 + seed)
    m_m, m_r = len(fam.mov_code), len(fam.ref_code)
    truth = np.where(np.arange(m_m) % 2 == 0, rng.integers(0, max(m_r, 1), m_m), -1).astype(np.int32) if m_r else np.full(m_m, -1, np.int32)
    q = 0
    for a, r in zip(np.asarray(a_row).tolist(), np.asarray(r_row).tolist()):
        a0, a1, r0, r1 = int(fam.mov_off[a]), int(fam.mov_off[a + 1]), int(fam.ref_off[r]), int(fam.ref_off[r + 1])
        nr = r1 - r0
        for k in range(a1 - a0):
            kind, q = q % 4, q + 1
            if kind == 0 or nr == 0:
                truth[a0 + k] = -1
            elif kind == 1:
                truth[a0 + k] = r0 + k % nr
            elif kind == 2:
                truth[a0 + k] = r0 + (k + 1) % nr
            else:
                other = (r1 + int(rng.integers(0, max(m_r - nr, 1)))) % m_r      # a member outside [r0, r1) unless the row owns them all
                truth[a0 + k] = other
    return truth


def check_not_vacuous(answer, fam, a_row, spec, truth_member, few=False):
    """what the spec and the truth were made to show is in the answer (few: a handful of pairs, of which only the identities are asked)"""
    marks, counts = answer.marks, answer.counts
    f = marks["flags"]
    matched = (f & MATCHED) != 0
    assert counts[1] == matched.sum() > 0 and counts[2] == ((f & TYPE_MATCH) != 0).sum(), spec.name
    assert not (f & (CONSIDERED | VIOLATING)).any() and not marks["reserved"].any()
    named = np.zeros(len(fam.mov_off) - 1, bool)
    named[np.asarray(a_row)] = True
    on_named = np.repeat(named, np.diff(fam.mov_off))
    assert np.array_equal(matched, on_named)
    if few:
        return
    if truth_member is not None:
        if (~on_named).any():
            assert (~matched & ((f & TRUTH_KNOWN) != 0)).any() and (~matched & ((f & TRUTH_KNOWN) == 0)).any(), "unmatched, truth known and not"
        on = (f & ON_TRUTH) != 0
        assert 0 < counts[5] == on.sum() < counts[4] < counts[1], counts
        wrong = matched & ((f & TRUTH_KNOWN) != 0) & ~on
        same_row = marks["ref_row"][wrong] == np.searchsorted(fam.ref_off, np.asarray(truth_member)[wrong], side="right") - 1
        assert same_row.any() and (~same_row).any(), "a truth in the right row and one in the wrong row, both missed"
    ranked = (f & RANKED) != 0
    if "tied" in spec.expects:
        assert (marks["rank_strict"][ranked] < marks["rank_weak"][ranked]).any(), spec.name
    if "nan" in spec.expects:
        assert (matched & ~ranked).any() and ranked.any(), spec.name
    if "all untyped" in spec.expects:
        assert not ranked.any() and (marks["rank_weak"] == UNRANKED).all(), spec.name
    if "saturated" in spec.expects:
        assert (marks["rank_strict"][ranked] == RANK_TOP).any() and (marks["rank_strict"][ranked] < RANK_TOP).any(), spec.name
    assert (marks["rank_strict"][~ranked] == UNRANKED).all() and (marks["rank_weak"][~ranked] == UNRANKED).all()
    assert (marks["rank_strict"][ranked] <= RANK_TOP).all() and (marks["rank_strict"][ranked] <= marks["rank_weak"][ranked]).all()
