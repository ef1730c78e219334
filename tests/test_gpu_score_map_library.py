"""same_merge_acc_score_map and the same_score_map_* calls (csrc/window_score_map.hip) driven at the library against
tests/score_map_check.py's `host_marks` -- plain numpy, nothing of libsame_hip in it -- on one merged accumulator
(tests/test_gpu_score_library.py's `_merged` recipe) over sections the tests make themselves.  Every assertion is exact equality: the
16-byte marks field for field, the ten int64 counts, the uint32 tally.

The inputs: score_check's own families (zero, NaN and infinite areas, negative and extreme codes, the 3000-triangle hubs under every
rule, the triangle counts at the wave and block edges); moving sections from the smallest that holds the final rows to 5000 rows more;
truth arrays all unknown, all right, all wrong and naming the last reference row; type rows of 1, 2, 20 and 300 columns with ties,
signed zeros, infinities and NaN; no detail object; and the protocol -- the call twice, between score and detail calls, without marks,
without a tally, after a reset -- with the runtime calls include/same_hip.h states."""
import contextlib
import ctypes

import numpy as np
import pytest

import score_check as S
import score_map_check as M
from test_gpu_score_library import RULES, _merged, _spent, large, tiny  # noqa: F401 (the fixtures are made here again, for this module)

pytestmark = pytest.mark.gpu

N_LABELS = 6            # the jobs' label codes are 0 .. 5; the families' other codes name no label
FEW_RULES = RULES[:3]   # any flip; the node-local rule at 0.0 with min_flips 0 and 1


@contextlib.contextmanager
def _resident(m, inp, truth=None, cols=None, types=None, tally=True, n_types=1):
    """the inputs as sections of their own on the accumulator's context -- the reference one with `types` as its type rows --, their label
    codes set, the triangles resident, the label columns as a DeviceScoreDetail (None: none) and a DeviceScoreMap over `truth`"""
    from same_amd import windows as W

    T = n_types if types is None else types.shape[1]
    made = []
    try:
        mov = W.DeviceSection(W.Section(inp.mov_xy, np.zeros((len(inp.mov_xy), T))), np.float64, m.ctx)
        made.append(mov)
        ref = W.DeviceSection(W.Section(inp.ref_xy, np.zeros((len(inp.ref_xy), T)) if types is None else types), np.float64, m.ctx)
        made.append(ref)
        mov.set_label_codes(np.ascontiguousarray(inp.code_m, np.int32))
        ref.set_label_codes(np.ascontiguousarray(inp.code_r, np.int32))
        tris = detail = None
        if inp.tris is not None:
            tris = W.DeviceCallerTris(mov, inp.tris, m.ctx)
            made.append(tris)
        if cols is not None:
            detail = W.DeviceScoreDetail(mov, None, 1, len(cols), cols)
            made.append(detail)
        smap = W.DeviceScoreMap(mov, ref, truth, tally, m.ctx)
        made.append(smap)
        yield mov, ref, tris, detail, smap
    finally:
        for h in reversed(made):                  # everything before its sections
            h.close()


def _same_marks(got, want, tag):
    assert got.dtype == M.MARK and len(got) == len(want), tag
    for field in M.MARK.names:
        bad = np.flatnonzero(got[field] != want[field])
        assert len(bad) == 0, (tag, field, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _check(m, name, inp, rules=FEW_RULES, truth=None, cols=None, types=None, both_type_rules=True):
    """the map call on `inp` under every rule: marks, counts and the tally's growth equal to `host_marks` -> the last counts"""
    folded = np.zeros((len(inp.mov_xy), 4), np.int64)
    calls = 0
    with _resident(m, inp, truth, cols, types) as (dmov, dref, tris, detail, smap):
        for ignore_same in ((True, False) if both_type_rules else (True,)):
            for rule in rules:
                counts, marks = m.acc.score_map(dmov, dref, tris, detail, smap, ignore_same, *rule)
                want_marks, want_counts, add = M.host_marks(m.job.a_row, m.job.r_row, *inp, truth, cols, types, ignore_same, *rule)
                tag = (name, ignore_same, rule)
                assert counts.dtype == np.int64 and counts.tolist() == want_counts.tolist(), (tag, counts.tolist(), want_counts.tolist())
                _same_marks(marks, want_marks, tag)
                folded += add
                calls += 1
        tally, results = smap.tally()
        assert results == calls and tally.dtype == np.uint32 and np.array_equal(tally, folded), name
    return counts


@pytest.fixture(scope="module")
def typed(large):
    """own's inputs with 20 type columns, the label columns and a truth that is right on every second matched row"""
    inp = S.own(large.job)
    truth = np.full(len(inp.mov_xy), -1, np.int32)
    truth[large.job.a_row] = np.where(np.arange(len(large.job.a_row)) % 2 == 0, large.job.r_row, 0)
    return inp, truth, M.label_columns(N_LABELS, 20), M.type_rows(len(inp.ref_xy), 20)


# ---- 1. score_check's families -----------------------------------------------------------------------------------------------------------
N_LARGE = 6 + 1 + 4 + (len(S.TRI_COUNTS) + 1) + 1


@pytest.mark.parametrize("which", range(N_LARGE))
def test_every_family_of_the_score_call(large, which):
    if not hasattr(large, "families"):
        large.families = S.all_families(large.job)
    assert len(large.families) == N_LARGE
    name, inp = large.families[which]
    n_mov, n_ref = len(inp.mov_xy), len(inp.ref_xy)
    truth = dict(M.truths(large.job, n_mov, n_ref))["the match"]
    truth[::3] = -1
    counts = _check(large, name, inp, RULES if name == "hub" else FEW_RULES, truth, M.label_columns(N_LABELS, 20), M.type_rows(n_ref, 20),
                    both_type_rules=name != "hub")
    print(name, counts.tolist())


def test_the_tiny_accumulator(tiny):
    for name, inp in S.small_families(tiny.job):
        print(name, _check(tiny, name, inp, FEW_RULES, None, M.label_columns(N_LABELS, 2), M.type_rows(len(inp.ref_xy), 2)).tolist())


# ---- 2. the moving section's size --------------------------------------------------------------------------------------------------------
def test_moving_sections_from_the_smallest_to_five_thousand_rows_more(large):
    """unmatched rows at the wave and block edges of the kernel's one lane per MOVING row; the largest lays the work buffer anew"""
    least = M.smallest_rows(large.job)
    for name, inp in M.sizes(large.job):
        truth = np.full(len(inp.mov_xy), len(inp.ref_xy) - 1, np.int32)
        counts = _check(large, name, inp, FEW_RULES[:2], truth, M.label_columns(N_LABELS, 2), M.type_rows(len(inp.ref_xy), 2),
                        both_type_rules=False)
        print(name, len(inp.mov_xy), counts.tolist())
        assert counts[0] == large.n_final and len(inp.mov_xy) >= least


# ---- 3. truth ----------------------------------------------------------------------------------------------------------------------------
def test_truth_arrays_and_the_refusal_of_rows_outside_the_reference(large):
    from same_amd import _lib
    from same_amd import windows as W

    inp = S.own(large.job)
    n_mov, n_ref, n = len(inp.mov_xy), len(inp.ref_xy), large.n_final
    seen = {}
    for name, truth in M.truths(large.job, n_mov, n_ref):
        seen[name] = _check(large, name, inp, FEW_RULES[:1], truth, both_type_rules=False)[8:].tolist()
    print(seen)
    assert seen["all unknown"] == [0, 0] and seen["the match"] == [n, n] and seen["shifted by one"] == [n, 0] and seen["the last row"][0] == n
    with _resident(large, inp) as (dmov, dref, _t, _d, _m):
        for bad in (n_ref, -2, 2**31 - 1, -2**31):
            truth = np.full(n_mov, -1, np.int32)
            truth[n_mov // 2] = bad
            h = ctypes.c_void_p()
            with large.ctx.lock:
                rc = large.ctx.lib.same_score_map_create(large.ctx.handle, dmov.handle, dref.handle, truth.ctypes.data, 1, ctypes.byref(h))
            assert rc == _lib.SAME_EINVAL == -22 and not h.value, (bad, rc)
            with pytest.raises(_lib.SameHipError):
                W.DeviceScoreMap(dmov, dref, truth, True, large.ctx)


# ---- 4. type rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", M.TYPE_COUNTS)
def test_type_rows_with_ties_signed_zeros_infinities_nan_and_saturation(large, T):
    inp = S.own(large.job)
    types, cols = M.type_rows(len(inp.ref_xy), T), M.label_columns(N_LABELS, T)
    _check(large, f"T = {T}", inp, FEW_RULES[:1], None, cols, types, both_type_rules=False)
    marks = M.host_marks(large.job.a_row, large.job.r_row, *inp, None, cols, types)[0][large.job.a_row]
    ranked = (marks["flags"] & M.RANKED) != 0
    assert 0 < ranked.sum() < len(marks)                          # NaN rows and the label without a column are among the final rows
    if T > 1:
        assert (marks["rank_strict"][ranked] < marks["rank_weak"][ranked]).any()          # exact ties
    if T == 300:
        assert (marks["rank_weak"][ranked] == 254).any() and marks["rank_weak"][ranked].max() == 254     # saturated, never 255


def test_no_detail_and_a_detail_without_columns_rank_nothing(large, typed):
    from same_amd import windows as W

    inp, truth, cols, types = typed
    with _resident(large, inp, truth, cols, types) as (dmov, dref, tris, detail, smap):
        with_ranks = large.acc.score_map(dmov, dref, tris, detail, smap)[1].copy()
        bare = W.DeviceScoreDetail(dmov, None, 1, N_LABELS, None)
        try:
            for d in (None, bare):
                counts, marks = large.acc.score_map(dmov, dref, tris, d, smap)
                assert (marks["rank_strict"] == 255).all() and (marks["rank_weak"] == 255).all() and not (marks["flags"] & M.RANKED).any()
                want = M.host_marks(large.job.a_row, large.job.r_row, *inp, truth)
                _same_marks(marks, want[0], "no ranks")
                assert counts.tolist() == want[1].tolist()
        finally:
            bare.close()
    assert (with_ranks["flags"] & M.RANKED).any()


# ---- 5. the protocol ---------------------------------------------------------------------------------------------------------------------
def test_the_call_twice_between_score_and_detail_calls_without_marks_without_a_tally_and_after_a_reset(large, typed):
    from same_amd import _lib
    from same_amd import windows as W

    inp, truth, cols, types = typed
    rule = (True, 0.5, 1)
    want_marks, want_counts, add = M.host_marks(large.job.a_row, large.job.r_row, *inp, truth, cols, types, True, *rule)
    with _resident(large, inp, truth, cols, types) as (dmov, dref, tris, detail, smap):
        score0 = large.acc.score(dmov, dref, tris, True, *rule)
        detail0 = large.acc.score_detail(dmov, dref, tris, detail, True, *rule)
        assert score0.tolist() == want_counts[:8].tolist()
        log = []
        for q in range(2):
            s0 = large.ctx.stats()
            counts, marks = large.acc.score_map(dmov, dref, tris, detail, smap, True, *rule)
            log.append(_spent(large.ctx, s0))
            _same_marks(marks, want_marks, ("call", q))
            assert counts.tolist() == want_counts.tolist()
        tally, results = smap.tally()
        assert results == 2 and np.array_equal(tally, 2 * add)                       # exactly doubled
        # the work buffer is idle again: the score and detail calls return their unchanged words, and no call lays it again
        s0 = large.ctx.stats()
        assert large.acc.score(dmov, dref, tris, True, *rule).tolist() == score0.tolist()
        again = large.acc.score_detail(dmov, dref, tris, detail, True, *rule)
        assert all(np.array_equal(again[k], detail0[k]) for k in detail0)
        assert _spent(large.ctx, s0)[1] == 0
        # without marks: the same counts and tally, one copy less
        s0 = large.ctx.stats()
        counts, marks = large.acc.score_map(dmov, dref, tris, detail, smap, True, *rule, marks=False)
        log.append(_spent(large.ctx, s0))
        assert marks is None and counts.tolist() == want_counts.tolist()
        tally, results = smap.tally()
        assert results == 3 and np.array_equal(tally, 3 * add)
        # what the header states of the runtime: (launches, fills, copies, waits)
        print(log)
        assert log == [(3, 0, 2, 1), (3, 0, 2, 1), (3, 0, 1, 1)]
        s0 = large.ctx.stats()
        smap.reset()
        assert _spent(large.ctx, s0) == (0, 1, 0, 1)
        s0 = large.ctx.stats()
        tally, results = smap.tally()
        assert _spent(large.ctx, s0) == (0, 0, 1, 1) and results == 0 and not tally.any()
        large.acc.score_map(dmov, dref, tris, detail, smap, True, *rule)
        assert np.array_equal(smap.tally()[0], add)
        # a map without a tally leaves nothing to read; its marks and counts are the same
        bare = W.DeviceScoreMap(dmov, dref, truth, False, large.ctx)
        try:
            counts, marks = large.acc.score_map(dmov, dref, tris, detail, bare, True, *rule)
            _same_marks(marks, want_marks, "no tally")
            assert counts.tolist() == want_counts.tolist() and bare.tally() == (None, 1)
            out = np.zeros((len(inp.mov_xy), 4), np.uint32)
            with large.ctx.lock:
                rc = large.ctx.lib.same_score_map_tally(bare.handle, out.ctypes.data, None)
            assert rc == _lib.SAME_EINVAL and not out.any()
        finally:
            bare.close()
        assert np.array_equal(smap.tally()[0], add)                                  # the other map's call left this one alone


def test_without_triangles_two_launches_and_a_map_of_other_sections_is_refused(large, typed):
    from same_amd import _lib

    inp, truth, cols, types = typed
    flat = inp._replace(tris=None)
    want_marks, want_counts, _add = M.host_marks(large.job.a_row, large.job.r_row, *flat, truth, cols, types)
    with _resident(large, flat, truth, cols, types) as (dmov, dref, tris, detail, smap):
        large.acc.score_map(dmov, dref, tris, detail, smap)
        s0 = large.ctx.stats()
        counts, marks = large.acc.score_map(dmov, dref, tris, detail, smap)
        assert _spent(large.ctx, s0) == (2, 0, 2, 1)
        _same_marks(marks, want_marks, "no triangulation")
        assert counts.tolist() == want_counts.tolist() and counts[7] == 0 and not (marks["flags"] & (M.CONSIDERED | M.VIOLATING)).any()
        with _resident(large, flat, truth) as (dmov2, dref2, _t, _d, other):
            out = np.full(10, -7, np.int64)
            for mov_h, ref_h, map_h in ((dmov, dref, other), (dmov2, dref, smap), (dmov, dref2, smap)):
                with large.ctx.lock:
                    rc = large.ctx.lib.same_merge_acc_score_map(large.acc.handle, mov_h.handle, ref_h.handle, None, None, map_h.handle, 1, 0, 0.5, 1,
                                                                None, out.ctypes.data)
                assert rc == _lib.SAME_EINVAL and out.tolist() == [-7] * 10
            assert other.tally()[1] == 0 and not other.tally()[0].any()
        assert large.acc.score_map(dmov, dref, tris, detail, smap)[0].tolist() == want_counts.tolist()
