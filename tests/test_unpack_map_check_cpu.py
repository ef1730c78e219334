"""tests/unpack_map_check.py held without a GPU: the statement tests/test_gpu_unpack_map_library.py holds same_merge_acc_unpack_map
(csrc/window_unpack_map.hip) against, checked against a per-member Python loop and `score_details.label_ranks`; and that the specs, the
truths and the member families hold what they are made to hold -- members on rows no final row names (some with a known truth), moving
rows without members, codes that are negative and at or above the label count, labels that name no column, type rows with a NaN, with
tied columns (strict != weak), 300 columns of which some rank exceeds 254, one column; truths that name a member of the right reference
row, one of a wrong row, and none."""
import numpy as np
import pytest

import unpack_check as U
import unpack_detail_check as D
import unpack_map_check as M

N_MOV, N_REF, N_FINAL = 90, 80, 60
A_ROW, R_ROW = U.synthetic_rows(N_MOV, N_REF, N_FINAL, seed=5)
FAMILIES = U.families(A_ROW, R_ROW, N_MOV, N_REF, seed=2)


def _loop(fam, spec, truth, ref_member):
    """the marks, the six counts and the tally update member by member, in plain Python"""
    m_mov = len(fam.mov_code)
    marks, tally = M.unmatched_marks(m_mov, truth), np.zeros((m_mov, 3), np.uint32)
    pairs = agreeing = known = on_truth = most = 0
    for a, r in zip(A_ROW.tolist(), R_ROW.tolist()):
        most = max(most, int(fam.mov_off[a + 1] - fam.mov_off[a]), int(fam.ref_off[r + 1] - fam.ref_off[r]))
        for i in range(int(fam.mov_off[a]), int(fam.mov_off[a + 1])):
            j = int(ref_member[pairs])
            assert fam.ref_off[r] <= j < fam.ref_off[r + 1]
            cm, cr = int(spec.mov_code[i]), int(spec.ref_code[j])
            t = -1 if truth is None else int(truth[i])
            flags = M.MATCHED | (M.TRUTH_KNOWN if t >= 0 else 0)
            tally[i, 0] += 1
            if cm >= 0 and cm == cr:
                flags |= M.TYPE_MATCH
                agreeing += 1
                tally[i, 1] += 1
            known += t >= 0
            if j == t:
                flags |= M.ON_TRUTH
                on_truth += 1
                tally[i, 2] += 1
            strict = weak = M.UNRANKED
            c = int(spec.col_of_label[cm]) if spec.col_of_label is not None and 0 <= cm < spec.n_labels else -1
            row = None if spec.ref_types is None else spec.ref_types[j].tolist()
            if c >= 0 and row is not None and not any(x != x for x in row):
                flags |= M.RANKED
                strict = min(sum(1 for q, x in enumerate(row) if q != c and x > row[c]), M.RANK_TOP)
                weak = min(sum(1 for q, x in enumerate(row) if q != c and x >= row[c]), M.RANK_TOP)
            marks[i] = (j, r, pairs, flags, strict, weak, 0)
            pairs += 1
    return marks, np.array([len(A_ROW), pairs, agreeing, most, known, on_truth], np.int64), tally


@pytest.mark.parametrize("which", range(len(FAMILIES)))
def test_the_statement_equals_a_loop_over_the_members(which):
    name, fam = FAMILIES[which]
    truth = M.truths(fam, A_ROW, R_ROW, seed=which)
    for strategy in U.STRATEGIES:
        unpacked = U.call(fam, A_ROW, R_ROW, strategy)
        for spec in M.specs(fam, seed=which):
            for t in (truth, None):
                got = M.host_unpack_map(A_ROW, R_ROW, fam, strategy, spec, t, unpacked=unpacked)
                marks, counts, tally = _loop(fam, spec, t, unpacked[1])
                assert got.marks.dtype == M.MARK and got.marks.tobytes() == marks.tobytes(), (name, spec.name, strategy)
                assert got.counts.tolist() == counts.tolist() and np.array_equal(got.tally, tally), (name, spec.name, strategy)
                assert got.counts[:4].tolist() == U.call(D.with_codes(fam, spec), A_ROW, R_ROW, strategy)[0].tolist()
            M.check_not_vacuous(M.host_unpack_map(A_ROW, R_ROW, fam, strategy, spec, truth, unpacked=unpacked), fam, A_ROW, spec, truth)
        # without a spec: the family's own codes, no ranks; the same pairs
        plain = M.host_unpack_map(A_ROW, R_ROW, fam, strategy, None, truth)
        assert plain.counts[:4].tolist() == unpacked[0].tolist() and not (plain.marks["flags"] & M.RANKED).any()
        assert np.array_equal(plain.marks["ref_member"][plain.marks["pair"] >= 0][np.argsort(plain.marks["pair"][plain.marks["pair"] >= 0])],
                              unpacked[1])


def test_the_families_specs_and_truths_hold_what_they_are_made_to_hold():
    by_name = dict(FAMILIES)
    fam = by_name["grid"]
    named = np.zeros(N_MOV, bool)
    named[A_ROW] = True
    on_named = np.repeat(named, np.diff(fam.mov_off))
    truth = M.truths(fam, A_ROW, R_ROW, seed=0)
    # members on rows that no final row names, some of them with a known truth
    assert (~on_named).sum() > 20 and (truth[~on_named] >= 0).any() and (truth[~on_named] < 0).any()
    # moving rows without members, on final rows
    empty = by_name["empty moving rows"]
    assert (np.diff(empty.mov_off)[A_ROW] == 0).sum() >= N_FINAL // 3
    # truths of every kind on the pairs: none, the right row (DISTRIBUTE's member and another of the row), a wrong row
    ref_row_of = lambda j: np.searchsorted(fam.ref_off, j, side="right") - 1
    row_of_final = np.full(N_MOV, -1)
    row_of_final[A_ROW] = R_ROW
    want_row = np.repeat(row_of_final, np.diff(fam.mov_off))[on_named]
    t = truth[on_named]
    assert (t < 0).any() and ((t >= 0) & (ref_row_of(t) == want_row)).any() and ((t >= 0) & (ref_row_of(t) != want_row)).any()
    dist = M.host_unpack_map(A_ROW, R_ROW, fam, U.DISTRIBUTE, None, truth)
    assert 0 < dist.counts[5] < dist.counts[4]
    by_spec = {s.name: s for s in M.specs(fam, seed=0)}
    assert [s.ref_types.shape[1] for s in by_spec.values() if s.ref_types is not None] == [1, 2, 17, 300]
    for spec in by_spec.values():
        L = spec.n_labels
        assert (spec.mov_code < 0).any() and (spec.mov_code >= L).any() and (spec.ref_code < 0).any(), spec.name
    assert (by_spec["L 5, G 3, T 2, ties"].col_of_label < 0).any() and (by_spec["L 5, T 300, ranks beyond 254"].col_of_label < 0).any()
    assert by_spec["no label names a column"].col_of_label is None
    assert np.isnan(by_spec["L 64, G 256, T 17, hostile rows"].ref_types).any(axis=1).any()
    for strategy in U.STRATEGIES:
        got = {name: M.host_unpack_map(A_ROW, R_ROW, fam, strategy, spec, truth) for name, spec in by_spec.items()}
        ranked = lambda g: (g.marks["flags"] & M.RANKED) != 0
        tied = got["L 5, G 3, T 2, ties"]
        assert (tied.marks["rank_strict"][ranked(tied)] != tied.marks["rank_weak"][ranked(tied)]).any()
        wide = got["L 5, T 300, ranks beyond 254"]
        assert (wide.marks["rank_weak"][ranked(wide)] == M.RANK_TOP).sum() > 3 and (wide.marks["rank_weak"][ranked(wide)] < M.RANK_TOP).any()
        one = got["L 1, no groups, T 1"]
        assert ranked(one).any() and not one.marks["rank_weak"][ranked(one)].any()          # one column: nothing ranks above it
        hostile = got["L 64, G 256, T 17, hostile rows"]
        matched = (hostile.marks["flags"] & M.MATCHED) != 0
        assert (matched & ~ranked(hostile)).any() and ranked(hostile).any()
        assert not ranked(got["no label names a column"]).any()


def test_the_ranks_are_label_ranks_saturated():
    from same_amd.score_details import label_ranks

    name, fam = FAMILIES[0]
    for spec in M.specs(fam, seed=4):
        if spec.col_of_label is None:
            continue
        L, T = spec.n_labels, spec.ref_types.shape[1]
        got = M.host_unpack_map(A_ROW, R_ROW, fam, U.NEAREST, spec, None)
        at = np.flatnonzero(got.marks["pair"] >= 0)
        columns = [f"col{t}" for t in range(T)]
        name_of = lambda code: columns[spec.col_of_label[code]] if 0 <= code < L and spec.col_of_label[code] >= 0 else f"none{code}"
        labels = np.array([name_of(int(c)) for c in spec.mov_code[at]], dtype=object)
        strict, weak, typed = label_ranks(labels, spec.ref_types[got.marks["ref_member"][at]], columns)
        assert np.array_equal(typed, (got.marks["flags"][at] & M.RANKED) != 0)
        assert np.array_equal(got.marks["rank_strict"][at], np.where(typed, np.minimum(strict, M.RANK_TOP), M.UNRANKED))
        assert np.array_equal(got.marks["rank_weak"][at], np.where(typed, np.minimum(weak, M.RANK_TOP), M.UNRANKED))
