"""tests/score_map_check.py without a GPU: `host_marks` agrees with score_check's counts and with the package's own host statement of the
rank rule (`score_details.label_ranks`), and each family has the property it was made for."""
import numpy as np
import pytest

import score_check as S
import score_map_check as M


@pytest.fixture(scope="module")
def job():
    return S.synthetic_job()


def test_the_mark_is_sixteen_bytes_in_the_headers_order():
    assert M.MARK.itemsize == 16 and M.MARK.names == ("ref_row", "node_tri", "node_flip", "flags", "rank_strict", "rank_weak", "reserved")
    assert [M.MARK.fields[k][1] for k in M.MARK.names] == [0, 4, 8, 12, 13, 14, 15]
    header = open(__file__.replace("tests/test_score_map_check_cpu.py", "include/same_hip.h")).read()
    for name, bit in (("MATCHED", M.MATCHED), ("TYPE_MATCH", M.TYPE_MATCH), ("CONSIDERED", M.CONSIDERED), ("VIOLATING", M.VIOLATING),
                      ("TRUTH_KNOWN", M.TRUTH_KNOWN), ("ON_TRUTH", M.ON_TRUTH), ("RANKED", M.RANKED)):
        assert f"#define SAME_MARK_{name}" in header and int(header.split(f"#define SAME_MARK_{name}")[1].split()[0]) == bit


def test_host_marks_sums_to_score_checks_counts_and_its_own_tally(job):
    inp = S.own(job)
    n_ref = len(inp.ref_xy)
    types = M.type_rows(n_ref, 20)
    cols = M.label_columns(6, 20)
    for name, truth in M.truths(job, len(inp.mov_xy), n_ref):
        for rule in ((False, 0.5, 1), (True, 0.5, 1), (True, 1.0 / 3.0, 2)):
            marks, counts, tally = M.host_marks(job.a_row, job.r_row, *inp, truth, cols, types, True, *rule)
            want, node_tri, node_flip = S.host_counts(job.a_row, job.r_row, *inp, True, *rule)
            assert counts[:8].tolist() == want.tolist(), (name, rule)
            f = marks["flags"]
            matched = (f & M.MATCHED) != 0
            assert matched.sum() == counts[0] and ((f & M.TYPE_MATCH) != 0).sum() == counts[1] and ((f & M.VIOLATING) != 0).sum() == counts[7]
            assert (matched & ((f & M.TRUTH_KNOWN) != 0)).sum() == counts[8] and ((f & M.ON_TRUTH) != 0).sum() == counts[9]
            assert np.array_equal(marks["node_tri"][matched], node_tri[matched]) and np.array_equal(marks["node_flip"][matched], node_flip[matched])
            assert np.array_equal(marks["ref_row"][job.a_row], job.r_row) and (marks["ref_row"][~matched] == -1).all()
            assert np.array_equal(tally, np.column_stack([(f & b) != 0 for b in (M.MATCHED, M.TYPE_MATCH, M.VIOLATING, M.ON_TRUTH)]))
            lost = marks[~matched]
            assert (lost["node_tri"] == 0).all() and (lost["node_flip"] == 0).all() and (lost["rank_strict"] == 255).all()
            assert (lost["rank_weak"] == 255).all() and (lost["reserved"] == 0).all() and ((lost["flags"] & ~np.uint8(M.TRUTH_KNOWN)) == 0).all()
    assert counts[7] > 0 and 0 < counts[1] < counts[0]


def test_the_rank_rule_is_the_packages_own_host_statement(job):
    """`score_details.label_ranks` (what `top_k_counts` and the notebook's cell 13 are stated with) on the same pairs"""
    from same_amd.score_details import label_ranks

    inp = S.own(job)
    for T in (1, 2, 20):
        types = M.type_rows(len(inp.ref_xy), T)
        cols = M.label_columns(6, T)
        marks, _c, _t = M.host_marks(job.a_row, job.r_row, *inp, None, cols, types)
        columns = [f"c{t}" for t in range(T)]
        labels = np.array([columns[cols[c]] if cols[c] >= 0 else "none" for c in inp.code_m[job.a_row]], dtype=object)
        strict, weak, typed = label_ranks(labels, types[job.r_row], columns)
        got = marks[job.a_row]
        assert np.array_equal((got["flags"] & M.RANKED) != 0, typed), T
        assert np.array_equal(got["rank_strict"][typed], strict[typed]) and np.array_equal(got["rank_weak"][typed], weak[typed]), T
        assert (got["rank_strict"][~typed] == 255).all() and 0 < typed.sum() < len(typed)


def test_the_sizes_put_unmatched_rows_at_the_wave_and_block_edges(job):
    least = M.smallest_rows(job)
    assert least == job.a_row.max() + 1 and least > len(job.a_row)         # unmatched rows inside the smallest section already
    got = M.sizes(job)
    assert [len(inp.mov_xy) for _n, inp in got] == [least + k for k in M.SIZE_STEPS]
    for name, inp in got:
        assert len(inp.code_m) == len(inp.mov_xy) and inp.tris.max() < len(inp.mov_xy) and len(inp.tris) > 0, name
        marks, counts, _t = M.host_marks(job.a_row, job.r_row, *inp)
        assert counts[0] == len(job.a_row) and (marks["ref_row"][least:] == -1).all(), name
    assert len(got[0][1].tris) <= len(got[-1][1].tris) == len(S.own(job).tris)    # a cut drops triangles; the grown sections keep them all
    cut = M.resized(S.grown(job), job, least)                                    # a section that had rows beyond: cut back to the smallest
    assert len(cut.mov_xy) == least and len(cut.tris) < len(S.grown(job).tris) and cut.tris.max() < least
    assert got[-1][1].mov_xy.shape[0] > len(S.grown(job).mov_xy) - 1       # larger than any section the score tests lay the buffer for


def test_the_truths_are_unknown_right_wrong_and_the_last_row(job):
    inp = S.own(job)
    n_mov, n_ref = len(inp.mov_xy), len(inp.ref_xy)
    got = dict(M.truths(job, n_mov, n_ref))
    per = {name: M.host_marks(job.a_row, job.r_row, *inp, truth)[1] for name, truth in got.items()}
    n = len(job.a_row)
    assert per["all unknown"][8:].tolist() == [0, 0]
    assert per["the match"][8:].tolist() == [n, n] and (got["the match"] >= 0).all()     # known on unmatched rows too
    assert per["shifted by one"][8:].tolist() == [n, 0]
    assert per["the last row"][8] == n and per["the last row"][9] == np.count_nonzero(job.r_row == n_ref - 1)
    assert all(t.dtype == np.int32 and t.min() >= -1 and t.max() < n_ref for t in got.values()) and got["the last row"].max() == n_ref - 1


def test_the_type_rows_hold_ties_signed_zeros_infinities_nan_and_saturate():
    for T in M.TYPE_COUNTS:
        rows = M.type_rows(64, T)
        assert rows.shape == (64, T) and rows.dtype == np.float64
        assert np.isnan(rows[6::8]).any(axis=1).all() and not np.isnan(rows[np.arange(64) % 8 != 6]).any()
        assert np.isposinf(rows[4::8]).any(axis=1).all() and np.isneginf(rows[5::8]).any(axis=1).all()
        if T > 1:
            assert M.host_ranks(0, rows[1]) == (0, T - 1)                  # all ties
            assert M.host_ranks(T - 1, rows[7]) == (T - 1, T - 1)          # strictly descending: the last column ranks last
        assert M.host_ranks(0, rows[6]) is None and M.host_ranks(-1, rows[0]) is None and M.host_ranks(T, rows[0]) is None
    rows = M.type_rows(64, 20)
    ties = [M.host_ranks(c, rows[2]) for c in range(20)]
    assert any(s < w for s, w in ties)
    zeros = rows[3]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all() and all(M.host_ranks(c, zeros) == (0, 19) for c in range(20))   # -0.0 == 0.0
    assert M.host_ranks(299, M.type_rows(8, 300)[7]) == (299, 299) and min(299, M.RANK_TOP) == 254
    cols = M.label_columns(6, 300)
    assert cols[0] == 299 and cols[-1] == -1 and cols.min() >= -1 and cols.max() < 300
