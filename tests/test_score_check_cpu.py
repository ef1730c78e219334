"""tests/score_check.py without a GPU: `host_counts` -- the statement tests/test_gpu_score_library.py holds same_merge_acc_score against --
equals the oracle's C triangle loop flag for flag and counter for counter on every input family, states the negative-code rule as a
hand-written loop does and the node-local rule as `record_from_counts` does; and every family has the property it was made for, on
synthetic final rows (a random injective match of 1200 of 1500 rows)."""
import functools
import types

import numpy as np
import pandas as pd
import pytest

import score_check as S


@functools.lru_cache(maxsize=None)
def _job():
    return S.synthetic_job()


@functools.lru_cache(maxsize=None)
def _families():
    return S.all_families(_job())


def _triangles(inp, ignore_same=True):
    job = _job()
    return S.host_triangles(job.a_row, job.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.tris, ignore_same)


def _counts(inp, *rule, ignore_same=True):
    job = _job()
    return S.host_counts(job.a_row, job.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.code_r, inp.tris, ignore_same, *rule)


# ---- the statement against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore_same", [True, False])
def test_flags_and_node_counters_equal_the_oracles_triangle_loop_on_every_family(oracle, ignore_same):
    job = _job()
    for name, inp in _families():
        if inp.tris is None:
            continue
        n = len(inp.mov_xy)
        matched = np.zeros(n, np.uint8)
        matched[job.a_row] = 1
        mapped = np.zeros((n, 2))
        mapped[job.a_row] = inp.ref_xy[job.r_row]
        # the oracle's same-type rule is plain equality: a code that equals nothing becomes a code no other row has
        type_id = np.where(inp.code_m < 0, 10**6 + np.arange(n), inp.code_m).astype(np.int32)
        flag, nt, nf = oracle.tri_flip_stats(inp.mov_xy, mapped, matched, inp.tris, type_id if ignore_same else None)
        m, same, flipped, _b, _a = _triangles(inp, ignore_same)
        # (the oracle computes `flipped` for skipped triangles too, as the statement does)
        assert np.array_equal(flag & 1, m) and np.array_equal((flag >> 1) & 1, same) and np.array_equal((flag >> 2) & 1, flipped), name
        counts, node_tri, node_flip = _counts(inp, ignore_same=ignore_same)
        assert np.array_equal(node_tri, nt) and np.array_equal(node_flip, nf), name
        assert counts[2:7].tolist() == [len(inp.tris), m.sum(), same.sum(), flipped.sum(), (flipped & ~same).sum()], name


@pytest.mark.parametrize("rule", [(False, 0.5, 1), (True, 0.5, 1), (True, 0.25, 2)])
def test_the_eight_counts_are_check_triangle_violations_stats_on_own(oracle, rule):
    job, inp = _job(), S.own(_job())
    out = pd.DataFrame({"a": job.a_row, "r": job.r_row, "mx": inp.ref_xy[job.r_row, 0], "my": inp.ref_xy[job.r_row, 1],
                        "cell_type": inp.code_m[job.a_row]})
    carrier = types.SimpleNamespace(metacell_df=pd.DataFrame({"X": inp.mov_xy[:, 0], "Y": inp.mov_xy[:, 1]}), metacell_delaunay=inp.tris)
    _df, stats = oracle.check_triangle_violations(out, carrier, aligned_id_col="a", ref_id_col="r", mapped_x_col="mx", mapped_y_col="my",
                                                  cell_type_col="cell_type", ignore_same_type_triangles=True, node_local=rule[0],
                                                  majority_threshold=rule[1], min_flips=rule[2])
    counts, _nt, _nf = _counts(inp, *rule)
    assert counts[0] == len(out) and counts[1] == np.count_nonzero(inp.code_m[job.a_row] == inp.code_r[job.r_row])
    assert [int(c) for c in counts[[2, 3, 4, 6, 7]]] == [stats[k] for k in ("total_triangles", "triangles_with_all_matched",
                                                                           "triangles_same_type_skipped", "triangles_flipped",
                                                                           "nodes_in_violating_triangles")]
    assert counts[6] > 0 and counts[7] > 0 and counts[4] > 0


def test_a_negative_code_equals_nothing():
    """a dozen rows, by hand: the row comparison and the same-type rule"""
    code_m = np.array([0, 1, -1, -1, 2, -2, 0, 0, 0, -1, -1, -1], np.int32)
    code_r = np.array([0, 2, -1, 1, -2, -2, 0, -1, 0, -1, 5, -1], np.int32)
    a_row = r_row = np.arange(12, dtype=np.int32)
    xy = np.column_stack((np.arange(12.0), np.arange(12.0) ** 2))
    tris = np.array([[6, 7, 8], [9, 10, 11], [2, 3, 9], [0, 6, 7], [0, 6, 2], [5, 5, 5], [8, 8, 8]], np.int32)
    agree = 0
    for cm, cr in zip(code_m.tolist(), code_r.tolist()):
        if cm >= 0 and cr >= 0 and cm == cr:
            agree += 1
    same = 0
    for t in tris.tolist():
        c = [int(code_m[v]) for v in t]
        if min(c) >= 0 and c[0] == c[1] == c[2]:
            same += 1
    assert (agree, same) == (3, 3)
    counts, _nt, _nf = S.host_counts(a_row, r_row, xy, xy, code_m, code_r, tris)
    assert (counts[1], counts[4]) == (agree, same) and counts[3] == 7
    # without the rule the three rows of -1 on both sides and the triangles of -1 and -2 alone would count
    assert np.count_nonzero(code_m == code_r) == agree + 4 and sum(len({int(code_m[v]) for v in t}) == 1 for t in tris.tolist()) == same + 3


# ---- the families hold what they are for ---------------------------------------------------------------------------------------------------
def _family(name):
    return dict(_families())[name]


def test_mirrored_turns_every_triangle_of_two_areas_over():
    (m, _s, f_own, b, a_own), (_m, _s2, f_mir, _b, a_mir) = _triangles(_family("own")), _triangles(_family("mirrored"))
    assert np.array_equal(a_mir[m], -a_own[m])                                    # exactly
    two = m & (b != 0) & (a_own != 0)
    assert two.sum() > 1000 and np.array_equal(f_mir[two], ~f_own[two]) and f_own.sum() > 0


def test_line_has_after_areas_that_are_exactly_zero_and_others_left_to_the_roundings():
    m, _s, f, _b, a = _triangles(_family("line"))
    zero, tiny = m & (a == 0), m & (a != 0) & (np.abs(a) < 1e-9)
    print("line: after-areas exactly 0:", zero.sum(), "non-zero below 1e-9:", tiny.sum(), "of", m.sum(), "flipped:", f.sum())
    assert zero.sum() >= 100 and tiny.sum() >= 100 and not f[zero].any() and 0 < f[tiny].sum() < tiny.sum()


def test_degenerate_has_before_areas_that_are_exactly_zero_a_triangle_300_times_and_unmatched_triangles():
    inp = _family("degenerate")
    m, _s, f, b, _a = _triangles(inp)
    print("degenerate: before-areas exactly 0:", (m & (b == 0)).sum(), "triangles not all matched:", (~m).sum())
    assert (m & (b == 0)).sum() >= 50
    twice = (inp.tris[:, 0] == inp.tris[:, 1]) | (inp.tris[:, 0] == inp.tris[:, 2])
    assert twice.sum() >= 100 and m[twice].all() and not f[twice].any()
    _u, times = np.unique(inp.tris, axis=0, return_counts=True)
    assert times.max() == 301 and f[np.all(inp.tris == _u[times.argmax()], axis=1)].all()          # own's, and 300 more: flipped
    lost = ~np.isin(inp.tris, _job().a_row).any(axis=1)
    assert lost.sum() >= 50 and not m[lost].any()
    _c, node_tri, node_flip = _counts(inp, ignore_same=False)
    assert node_flip.max() >= 300 and node_tri[inp.tris[twice][0, 0]] >= 2           # a repeated corner: once per occurrence


def test_nonfinite_has_nan_areas_on_each_side_and_signed_zeros():
    m, _s, f, b, a = _triangles(_family("nonfinite"))
    print("nonfinite: NaN areas before:", (m & np.isnan(b)).sum(), "after:", (m & np.isnan(a)).sum(),
          "infinite:", (m & np.isinf(b)).sum(), (m & np.isinf(a)).sum(), "-0.0:", (m & (b == 0) & np.signbit(b)).sum(),
          (m & (a == 0) & np.signbit(a)).sum())
    assert (m & np.isnan(b)).sum() >= 20 and (m & np.isnan(a)).sum() >= 20
    assert (m & np.isinf(b)).sum() >= 5 and (m & np.isinf(a)).sum() >= 5
    for v in (b, a):
        assert (m & (v == 0) & np.signbit(v)).sum() >= 5 and (m & (v == 0) & ~np.signbit(v)).sum() >= 5
    assert f[m & (np.isnan(b) | np.isnan(a))].sum() >= 20 and not f[m & ((b == 0) | (a == 0))].any()
    assert f[m & np.isnan(b) & np.isnan(a)].all()                                  # NaN is unequal to NaN


def test_cancellation_is_decided_by_the_operation_order():
    inp = _family("cancellation")
    m, _s, f, b, a = _triangles(inp)
    assert m.all() and len(inp.tris) >= 300
    mapped = np.zeros_like(inp.mov_xy)
    mapped[_job().a_row] = inp.ref_xy[_job().r_row]
    exact_b = np.array([S.exact_sign(*inp.mov_xy[t]) for t in inp.tris])
    exact_a = np.array([S.exact_sign(*mapped[t]) for t in inp.tris])
    differ = (np.sign(b) != exact_b) | (np.sign(a) != exact_a)
    both = (b != 0) & (a != 0)
    print(f"cancellation: {len(inp.tris)} triangles, plain-order sign differs from the exact one for {differ.mean():.1%} "
          f"(before {np.mean(np.sign(b) != exact_b):.1%}, after {np.mean(np.sign(a) != exact_a):.1%}), "
          f"non-zero in both areas {both.mean():.1%}, flipped {f.mean():.1%}")
    assert differ.mean() >= 0.2 and both.mean() >= 0.2 and 0 < f.sum() < both.sum()


def test_hub_ratios_are_exact():
    inp, hubs = S.hub(_job())
    counts, node_tri, node_flip = _counts(inp)
    assert counts[2] == counts[3] == 2 * S.FAN and counts[4] == 0
    assert node_tri[list(hubs)].tolist() == [S.FAN, S.FAN] and node_flip[list(hubs)].tolist() == [S.FAN // 2, S.FAN // 3]
    assert node_flip[hubs[0]] / node_tri[hubs[0]] == 0.5 and node_flip[hubs[1]] / node_tri[hubs[1]] == 1.0 / 3.0
    at = lambda thr: int(_counts(inp, True, thr, 1)[0][7])
    assert at(0.5) - at(float(np.nextafter(0.5, 1.0))) == 1 and at(1.0 / 3.0) - at(float(np.nextafter(1.0 / 3.0, 1.0))) == 1


def test_every_codes_variant_changes_a_count():
    base = _counts(_family("own"))[0]
    for name, inp in S.codes(_job()):
        c = _counts(inp)[0]
        print("codes:", name, "[1], [4] =", int(c[1]), int(c[4]), "own:", int(base[1]), int(base[4]))
        assert c[1] != base[1] or c[4] != base[4], name
        assert np.array_equal(c[[0, 2, 3, 5]], base[[0, 2, 3, 5]]), name          # the codes touch nothing else
    neg = dict(S.codes(_job()))["negative"]
    job = _job()
    assert np.count_nonzero((neg.code_m[job.a_row] == -1) & (neg.code_r[job.r_row] == -1)) >= 200
    assert np.count_nonzero((neg.code_m[neg.tris] == -1).all(axis=1)) >= 40 and (neg.code_m < 0).mean() >= 0.2 and (neg.code_r < 0).mean() >= 0.2
    assert dict(S.codes(_job()))["largest"].code_m.max() == 2**31 - 1


def test_no_family_passes_a_kernel_that_returns_zeros():
    for name, inp in _families():
        c = _counts(inp)[0]
        print(f"{name}: {c.tolist()}")
        assert c[0] == 1200
        if name.startswith("tri_counts"):
            assert c[2] == (0 if inp.tris is None else len(inp.tris))
            continue
        if name == "codes: all equal":      # every matched triangle is skipped, by construction: [6] is 0 of [5] > 0; the chain without the rule
            assert c[6] == 0 < c[5] and c[4] == c[3]
            c = _counts(inp, ignore_same=False)[0]
        assert 0 < c[6] <= c[5] <= c[3] <= c[2] and (c[6] < c[5] or c[5] < c[3] or c[3] < c[2]) and c[7] > 0, (name, c)
    g = _family("grown")
    assert len(g.mov_xy) == 1500 + S.GROWN_ROWS and not np.isin(_job().a_row, np.arange(1500, len(g.mov_xy))).any()
    new = (g.tris >= 1500).any(axis=1)
    assert new.sum() >= 3000 and not _triangles(g)[0][new].any() and g.tris.max() == len(g.mov_xy) - 1
    assert [len(i.tris) for n, i in S.tri_counts(_job()) if i.tris is not None] == list(S.TRI_COUNTS)


# ---- the node-local rule ---------------------------------------------------------------------------------------------------------------------
def test_the_node_local_rule_at_its_edges_and_against_record_from_counts():
    from same_amd.scores import record_from_counts

    job = _job()
    inp, hubs = S.hub(job)
    default, node_tri, node_flip = _counts(inp)
    seen = {}
    for thr in S.THRESHOLDS:
        for min_flips in S.MIN_FLIPS:
            counts, nt, nf = _counts(inp, True, thr, min_flips)
            assert np.array_equal(nt, node_tri) and np.array_equal(nf, node_flip) and np.array_equal(counts[:7], default[:7])
            rec = record_from_counts({"matched": counts[0], "type_matches": counts[1], "total_triangles": counts[2],
                                      "triangles_with_all_matched": counts[3], "triangles_same_type_skipped": counts[4],
                                      "triangles_flipped": counts[6], "node_triangles": nt[job.a_row], "node_flips": nf[job.a_row]},
                                     {"node_local": True, "majority_threshold": thr, "min_flips": min_flips})
            assert rec["nodes_in_violating_triangles"] == counts[7], (thr, min_flips)
            seen[thr, min_flips] = int(counts[7])
    rec = record_from_counts({"matched": default[0], "type_matches": default[1], "total_triangles": default[2],
                              "triangles_with_all_matched": default[3], "triangles_same_type_skipped": default[4],
                              "triangles_flipped": default[6], "node_triangles": node_tri[job.a_row], "node_flips": node_flip[job.a_row]})
    assert rec["nodes_in_violating_triangles"] == default[7] == np.count_nonzero(node_flip[job.a_row] > 0)
    with_tri, with_flip = int(np.count_nonzero(node_tri[job.a_row] > 0)), int(default[7])
    half = float(np.nextafter(0.5, 1.0))
    print("hub: rows with triangles", with_tri, "with flips", with_flip, {k: v for k, v in seen.items() if k[1] == 1})
    # every row of the fans is a corner of flipped triangles alone or of none, but the hubs (1/2 and 1/3)
    assert seen[0.5, 1] == with_flip - 1 and seen[half, 1] == with_flip - 2 and seen[1.0 / 3.0, 1] == with_flip and seen[1.0, 1] == with_flip - 2
    for min_flips in (0, -3):              # no flip needed: a threshold at or below 0 takes every row that has a triangle
        assert seen[0.0, min_flips] == seen[-1.0, min_flips] == with_tri > with_flip
        assert seen[0.5, min_flips] == with_flip - 1
    assert seen[0.0, 1] == seen[-1.0, 1] == seen[0.0, 2] == with_flip
    assert all(seen[thr, 2**62 - 1] == 0 for thr in S.THRESHOLDS) and all(seen[t, m] == 0 for t in (1.5, float("inf")) for m in S.MIN_FLIPS)
