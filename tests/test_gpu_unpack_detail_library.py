"""same_merge_acc_unpack_detail (csrc/window_unpack_detail.hip) driven at the library against tests/unpack_detail_check.py's
`host_unpack_detail` -- `host_unpack`'s scipy statement with numpy bins, nothing of libsame_hip in it -- over the merged accumulators
and the hostile member lists of tests/test_gpu_unpack_library.py.  Every assertion is exact equality."""
import ctypes

import numpy as np
import pytest

import unpack_check as U
import unpack_detail_check as D
from test_gpu_score_library import ONE_WINDOW, _synthetic
from test_gpu_unpack_library import N_FAMILIES, NAMES, _close, _families, _merged, _slice_units, _spent, large, tiny  # noqa: F401

pytestmark = pytest.mark.gpu


def _specs(m, which):
    """the specs over family `which` of this accumulator -- made once, never changed"""
    held = m.made.setdefault("specs", {})
    if which not in held:
        held[which] = D.specs(_families(m)[which][1], m.n_mov, seed=100 + which)
    return held[which]


def _want(m, which, spec, strategy):
    """the statement's words (the pairs are the family's own: `_families` solved them once)"""
    held = m.made.setdefault("want words", {})
    key = (which, spec.name, strategy)
    if key not in held:
        name, fam, want = _families(m)[which]
        held[key] = D.host_unpack_detail(m.a_row, m.r_row, fam, strategy, spec, unpacked=want[strategy])
    return held[key]


def _resident(m, which, spec):
    """(moving members, reference members) of the family under the spec's codes: kept with the accumulator's other members, so the
    fixture's `_close` closes them before the sections"""
    from same_amd import windows as W

    held = m.made.setdefault("members", {})
    key = ("detail", which, spec.name)
    if key not in held:
        fam = D.with_codes(_families(m)[which][1], spec)
        held[key] = (fam, W.DeviceMembers(m.frames.dmov, fam.mov_off, fam.mov_xy, fam.mov_code),
                     W.DeviceMembers(m.frames.dref, fam.ref_off, fam.ref_xy, fam.ref_code))
    return held[key][1:]


class _Bound:
    """a spec's detail and groups objects beside the members, closed on exit (before the members)"""

    def __init__(self, m, which, spec):
        from same_amd import windows as W

        self.mm, self.rm = _resident(m, which, spec)
        self.detail = W.DeviceUnpackDetail(self.rm, spec.n_labels, spec.col_of_label, spec.ref_types)
        self.groups = None if spec.group_of is None else W.DeviceScoreDetail(m.frames.dmov, spec.group_of, spec.n_groups, 0, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.detail.close()
        if self.groups is not None:
            self.groups.close()


def _words(d):
    """split_unpack_detail's dict back as the call's words"""
    return np.concatenate([d["counts"], d["confusion"].reshape(-1), [d["unlabelled"]], d["groups"].reshape(-1), d["strict"], d["weak"],
                           [d["untyped"]]]).astype(np.int64)


def _raw(m, b, strategy, out, out_words=None, detail=None, groups="own", acc=None, mm=None, rm=None):
    acc = m.acc if acc is None else acc
    g = b.groups if groups == "own" else groups
    with acc.ctx.lock:
        return acc.ctx.lib.same_merge_acc_unpack_detail(acc.handle, (mm or b.mm).handle, (rm or b.rm).handle, strategy,
                                                        (detail or b.detail).handle, None if g is None else g.handle, out.ctypes.data,
                                                        len(out) if out_words is None else out_words)


# ---- 1. the families x the specs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(N_FAMILIES))
@pytest.mark.parametrize("size", ["large", "tiny"])
def test_every_family_under_every_spec(request, size, which):
    m = request.getfixturevalue(size)
    name = _families(m)[which][0]
    for spec in _specs(m, which):
        with _Bound(m, which, spec) as b:
            for s in U.STRATEGIES:
                want = _want(m, which, spec, s)
                got = m.acc.unpack_detail(b.mm, b.rm, NAMES[s], b.detail, b.groups)
                assert np.array_equal(_words(got), want), (size, name, spec.name, NAMES[s])
                # counts: exactly the unpack call's for the same arguments
                assert m.acc.unpack(b.mm, b.rm, NAMES[s]).tolist() == want[:4].tolist(), (size, name, spec.name, NAMES[s])
                D.check_not_vacuous(D.parts(want, spec.n_labels, spec.n_groups), spec)
    print(size, name, [(s.name, _want(m, which, s, U.NEAREST)[:4].tolist()) for s in _specs(m, which)])


def test_every_pair_is_binned_once_whatever_the_slice_budget(large, monkeypatch):
    name, fam, _w = _families(large)[6]
    na, nr = U.row_sizes(fam, large.a_row, large.r_row)
    units = int(_slice_units(na, nr).sum())
    spec = _specs(large, 6)[2]
    want = _want(large, 6, spec, U.NEAREST)
    with _Bound(large, 6, spec) as b:
        for budget in (None, 7, units - 1, units):
            if budget is None:
                monkeypatch.delenv("SAME_UNPACK_BUDGET_UNITS", raising=False)
            else:
                monkeypatch.setenv("SAME_UNPACK_BUDGET_UNITS", str(budget))
            s0 = large.ctx.stats()
            got = large.acc.unpack_detail(b.mm, b.rm, "nearest", b.detail, b.groups)
            launches = _spent(large.ctx, s0)[0]
            assert np.array_equal(_words(got), want), budget
            assert launches == 1 + (1 if budget is None else -(-units // budget)) + 1, (budget, launches)


# ---- 2. the work buffers' life -----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_history_and_the_other_reader_calls_are_not_disturbed(large):
    """one accumulator: small lists, the large lists, small again, both strategies, specs of few and of many words, with unpack, score
    and score_detail in between -- every answer the statement's, every other call's answer what it was before"""
    from same_amd import windows as W

    frames = large.frames
    frames.label_codes_on_device()
    plain = W.DeviceScoreDetail(frames.dmov, None, 1, 4, None)
    try:
        score = lambda: large.acc.score(frames.dmov, frames.dref).tolist()
        detail = lambda: {k: np.asarray(v).tolist() for k, v in large.acc.score_detail(frames.dmov, frames.dref, None, plain).items()}
        before, before_detail = score(), detail()
        assert before[0] == large.n_final and 0 < before[1] <= before[0]
        for which, at in ((0, 2), (6, 0), (0, 1), (5, 2), (6, 2), (0, 0)):
            spec = _specs(large, which)[at]
            with _Bound(large, which, spec) as b:
                for s in (U.NEAREST, U.DISTRIBUTE, U.NEAREST, U.NEAREST, U.DISTRIBUTE):
                    want = _want(large, which, spec, s)
                    got = large.acc.unpack_detail(b.mm, b.rm, NAMES[s], b.detail, b.groups)
                    assert np.array_equal(_words(got), want), (which, spec.name, s)
                    counts, ref_member = large.acc.unpack(b.mm, b.rm, NAMES[s], pairs=True)
                    assert counts.tolist() == want[:4].tolist() and np.array_equal(ref_member, _families(large)[which][2][s][1])
                    assert score() == before and detail() == before_detail, (which, spec.name, s)
                    assert np.array_equal(_words(large.acc.unpack_detail(b.mm, b.rm, NAMES[s], b.detail, b.groups)), want)
    finally:
        plain.close()


def test_what_the_calls_ask_of_the_runtime(monkeypatch):
    """(launches, fills, copies, waits) as include/same_hip.h states them, on the 200-cell one-window accumulator: one launch more than
    same_merge_acc_unpack for the same rows, three copies, two waits, a fill only where a buffer is laid; the unpack call's own counts in
    the same sequence as tests/test_gpu_unpack_library.py has them; the score and the detail call in between without a fill"""
    from same_amd import windows as W

    ref, mov, cols = _synthetic(200, 7)
    with _merged(ref, mov, cols, ONE_WINDOW) as m:
        assert 64 < m.n_final < 256
        try:
            fam = _families(m)[0][1]
            na, nr = U.row_sizes(fam, m.a_row, m.r_row)
            units = int(_slice_units(na, nr).sum())
            assert units > 40
            small, big = _specs(m, 0)[0], _specs(m, 0)[2]
            m.frames.label_codes_on_device()
            plain = W.DeviceScoreDetail(m.frames.dmov, None, 1, 4, None)
            with _Bound(m, 0, small) as bs, _Bound(m, 0, big) as bb:
                # (strategy, bound spec, budget) -> fills: the unpack buffer and the bins' on the first call, the bins' alone when they grow
                steps = [(U.DISTRIBUTE, bs, small, None, 2), (U.NEAREST, bs, small, None, 0), (U.NEAREST, bb, big, None, 1),
                         (U.NEAREST, bs, small, 7, 0), (U.DISTRIBUTE, bb, big, 7, 0), (U.NEAREST, bb, big, units - 1, 0)]
                for s, b, spec, budget, fills in steps:
                    if budget is None:
                        monkeypatch.delenv("SAME_UNPACK_BUDGET_UNITS", raising=False)
                    else:
                        monkeypatch.setenv("SAME_UNPACK_BUDGET_UNITS", str(budget))
                    chunks = 1 if s == U.DISTRIBUTE or budget is None else -(-units // budget)
                    want = _want(m, 0, spec, s)
                    s0 = m.ctx.stats()
                    got = m.acc.unpack_detail(b.mm, b.rm, NAMES[s], b.detail, b.groups)
                    spent = _spent(m.ctx, s0)
                    print(NAMES[s], spec.name, budget, spent)
                    assert np.array_equal(_words(got), want)
                    assert spent == (1 + chunks + 1, fills, 3, 2), (NAMES[s], spec.name, budget, spent)
                    # the existing call, counts only and with the pairs: as its own test has it, no fill
                    for with_pairs in (False, True):
                        s0 = m.ctx.stats()
                        m.acc.unpack(b.mm, b.rm, NAMES[s], pairs=with_pairs)
                        assert _spent(m.ctx, s0) == (1 + chunks, 0, 3 if with_pairs else 2, 3 if with_pairs else 2)
                    # score and score_detail alternate with both: no fill after their own first
                    m.acc.score(m.frames.dmov, m.frames.dref)
                    m.acc.score_detail(m.frames.dmov, m.frames.dref, None, plain)
                    s0 = m.ctx.stats()
                    m.acc.score(m.frames.dmov, m.frames.dref)
                    m.acc.score_detail(m.frames.dmov, m.frames.dref, None, plain)
                    assert _spent(m.ctx, s0)[1] == 0
                # rows without members on the moving side only: no pair, what the unpack call asks, zeros behind the counts
                monkeypatch.delenv("SAME_UNPACK_BUDGET_UNITS", raising=False)
                none = W.DeviceMembers(m.frames.dmov, np.zeros(m.n_mov + 1, np.int64), np.zeros((0, 2)), np.zeros(0, np.int32))
                try:
                    s0 = m.ctx.stats()
                    got = _words(m.acc.unpack_detail(none, bs.rm, "nearest", bs.detail, bs.groups))
                    assert _spent(m.ctx, s0) == (1, 0, 1, 1)
                    assert got[:4].tolist() == [m.n_final, 0, 0, int(nr.max())] and not got[4:].any()
                finally:
                    none.close()
            plain.close()
        finally:
            _close(m)


# ---- 3. what the calls refuse ------------------------------------------------------------------------------------------------------------------
def test_unpack_detail_create_checks_its_arguments(tiny):
    from same_amd import _lib, windows as W

    spec = _specs(tiny, 0)[1]
    mm, rm = _resident(tiny, 0, spec)
    types2 = np.ascontiguousarray(spec.ref_types)

    def rc_of(n_labels, col, types, T):
        h = ctypes.c_void_p()
        col = None if col is None else np.ascontiguousarray(col, np.int32)
        with rm.ctx.lock:
            rc = rm.ctx.lib.same_unpack_detail_create(rm.handle, n_labels, None if col is None else col.ctypes.data,
                                                      None if types is None else types.ctypes.data, T, ctypes.byref(h))
            if h.value:
                rm.ctx.lib.same_unpack_detail_destroy(h)
        return rc

    ok = np.array([0, 1, -1, 0, 1])
    assert rc_of(5, ok, types2, 2) == 0 and rc_of(0, None, None, 0) == 0 and rc_of(64, None, types2, 2) == 0 and rc_of(5, None, None, 7) == 0
    assert rc_of(-1, None, None, 0) == _lib.SAME_EINVAL and rc_of(65, None, None, 0) == _lib.SAME_EINVAL
    assert rc_of(5, None, types2, -1) == _lib.SAME_EINVAL
    assert rc_of(5, ok, None, 2) == _lib.SAME_EINVAL and rc_of(5, ok, types2, 0) == _lib.SAME_EINVAL
    for bad in (np.array([0, 1, 2, 0, 1]), np.array([0, 1, -2, 0, 1])):
        assert rc_of(5, bad, types2, 2) == _lib.SAME_ERANGE
    with pytest.raises(ValueError, match="col_of_label has shape"):
        W.DeviceUnpackDetail(rm, 5, ok[:4], types2)
    with pytest.raises(ValueError, match="member_types has shape"):
        W.DeviceUnpackDetail(rm, 5, ok, types2[:-1])


def test_each_refusal_returns_its_code_with_out_untouched_and_the_next_call_answers(large):
    from same_amd import _lib, windows as W

    which = 0
    spec, other_spec = _specs(large, which)[1], _specs(large, which)[3]
    fam = D.with_codes(_families(large)[which][1], spec)
    words = D.out_words(spec.n_labels, spec.n_groups)
    with _Bound(large, which, spec) as b, _Bound(large, which, other_spec) as other:
        out = np.full(words + 3, -5, np.int64)
        untouched = lambda rc, code: rc == code and (out == -5).all()
        good = lambda: np.array_equal(_words(large.acc.unpack_detail(b.mm, b.rm, "nearest", b.detail, b.groups)),
                                      _want(large, which, spec, U.NEAREST))
        assert good()
        # out_words too small; a detail made for other members; groups made for the other section; the unpack call's own refusals
        assert untouched(_raw(large, b, U.NEAREST, out, words - 1), _lib.SAME_EINVAL)
        assert untouched(_raw(large, b, U.NEAREST, out, detail=other.detail), _lib.SAME_EINVAL)
        ref_groups = W.DeviceScoreDetail(large.frames.dref, None, 3, 0, None)
        try:
            assert untouched(_raw(large, b, U.NEAREST, out, groups=ref_groups), _lib.SAME_EINVAL)
        finally:
            ref_groups.close()
        assert untouched(_raw(large, b, 2, out), _lib.SAME_EINVAL)
        assert untouched(_raw(large, b, U.DISTRIBUTE, out, mm=b.rm), _lib.SAME_EINVAL)
        fresh = W.MergeAccumulator(large.ctx)
        try:
            fresh.begin(16)
            assert untouched(_raw(large, b, U.DISTRIBUTE, out, acc=fresh), _lib.SAME_EINVAL)
        finally:
            fresh.close()
        assert good()
        # one member's X is NaN, on a row a final row names: infeasible under NEAREST alone -- its pairs are never read
        xy = fam.mov_xy.copy()
        xy[fam.mov_off[int(large.a_row[9])], 0] = np.nan
        nan = W.DeviceMembers(large.frames.dmov, fam.mov_off, xy, fam.mov_code)
        # a final row's members against an empty reference list
        counts = np.diff(fam.ref_off)
        keep = np.ones(len(fam.ref_xy), bool)
        r = int(large.r_row[5])
        keep[fam.ref_off[r]:fam.ref_off[r + 1]] = False
        counts[r] = 0
        hollow = W.DeviceMembers(large.frames.dref, np.concatenate(([0], np.cumsum(counts))), fam.ref_xy[keep], fam.ref_code[keep])
        hollow_detail = W.DeviceUnpackDetail(hollow, spec.n_labels, spec.col_of_label, spec.ref_types[keep])
        try:
            assert untouched(_raw(large, b, U.NEAREST, out, mm=nan), _lib.SAME_ERANGE)
            assert good()                                    # the bins the refused call counted into are cleared
            for s in U.STRATEGIES:
                assert untouched(_raw(large, b, s, out, rm=hollow, detail=hollow_detail), _lib.SAME_ERANGE), s
            assert good()
            rc = _raw(large, b, U.DISTRIBUTE, out, words, mm=nan)
            assert rc == 0 and np.array_equal(out[:words], _want(large, which, spec, U.DISTRIBUTE)) and (out[words:] == -5).all()
            with pytest.raises(_lib.SameHipError, match="infeasible") as e:
                large.acc.unpack_detail(nan, b.rm, "nearest", b.detail, b.groups)
            assert e.value.code == _lib.SAME_ERANGE
        finally:
            hollow_detail.close()
            hollow.close()
            nan.close()
        assert good()
        with pytest.raises(ValueError, match="strategy must be one of"):
            large.acc.unpack_detail(b.mm, b.rm, "closest", b.detail, b.groups)
