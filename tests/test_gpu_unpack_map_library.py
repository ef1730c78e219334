"""same_merge_acc_unpack_map and the same_unpack_map_* calls (csrc/window_unpack_map.hip) driven at the library against
tests/unpack_map_check.py's `host_unpack_map` -- `host_unpack`'s scipy statement with numpy marks, nothing of libsame_hip in it -- on
merged accumulators made as tests/test_gpu_unpack_feature_library.py makes them.  Every assertion is exact equality: the marks as bytes,
the six counts, the tally's words.

The inputs: 0, 1, 63, 64, 65, 257 and about 5000 final rows; member lists of 1, 2, 63 and 64 on either side and every (na, nr) of
1..6 x 1..6; moving rows without members; both strategies, and tests/unpack_check.py's tied families under "nearest"; with and without
`detail`, `truth_member`, `with_tally`, `out_marks`; the tally after three calls and after a reset; the call twice and between score,
detail, map, feature, unpack, unpack-detail and unpack-feature calls, with the runtime calls include/same_hip.h states; every refusal
it states (but a map on another device: one device here), with the outputs untouched.  No test passes a non-finite XY on purpose to
anything but the refusal that names it."""
import ctypes
import itertools

import numpy as np
import pytest

import feature_check as C
import unpack_check as U
import unpack_detail_check as D
import unpack_feature_check as UF
import unpack_map_check as M
from test_gpu_unpack_feature_library import _accumulator, _lists, big, mid  # noqa: F401
from test_gpu_unpack_library import NAMES, _close, _families, _spent, large  # noqa: F401

pytestmark = pytest.mark.gpu


class _Resident:
    """a family's members under a spec's codes, the spec's detail (None: no detail) and a map beside the accumulator's sections, closed
    on exit in the order the header asks"""

    def __init__(self, m, fam, spec=None, truth=None, tally=True, detail=True):
        from same_amd import windows as W

        self.made = []
        self.fam = fam = fam if spec is None else D.with_codes(fam, spec)
        try:
            self.mm = self._keep(W.DeviceMembers(m.frames.dmov, fam.mov_off, fam.mov_xy, fam.mov_code))
            self.rm = self._keep(W.DeviceMembers(m.frames.dref, fam.ref_off, fam.ref_xy, fam.ref_code))
            self.detail = None
            if spec is not None and detail:
                self.detail = self._keep(W.DeviceUnpackDetail(self.rm, spec.n_labels, spec.col_of_label, spec.ref_types))
            self.map = self._keep(W.DeviceUnpackMap(self.mm, self.rm, truth, tally))
        except BaseException:
            self.close()
            raise

    def _keep(self, h):
        self.made.append(h)
        return h

    def close(self):
        for h in reversed(self.made):
            h.close()
        self.made = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _same(got, want, tag, marks=True):
    counts, got_marks = got
    assert counts.dtype == np.int64 and counts.tolist() == want.counts.tolist(), (tag, counts.tolist(), want.counts.tolist())
    if not marks:
        assert got_marks is None
        return
    assert got_marks.dtype.itemsize == 16 and len(got_marks) == len(want.marks), tag
    if got_marks.tobytes() != want.marks.tobytes():
        bad = np.flatnonzero(got_marks.view(M.MARK) != want.marks)
        raise AssertionError((tag, bad[:6].tolist(), got_marks[bad[:6]].tolist(), want.marks[bad[:6]].tolist()))


def _check(m, fam, spec, truth, tag, strategies=U.STRATEGIES, calls=1, few=False, unpacked=None):
    """the call on these inputs against the statement, per strategy `calls` times; the tally is what the calls add up to -> the answers"""
    wants = {}
    with _Resident(m, fam, spec, truth) as r:
        total, n = np.zeros((len(fam.mov_code), 3), np.uint32), 0
        for s in strategies:
            wants[s] = want = M.host_unpack_map(m.a_row, m.r_row, fam, s, spec, truth, unpacked=None if unpacked is None else unpacked[s])
            for q in range(calls):
                _same(m.acc.unpack_map(r.mm, r.rm, NAMES[s], r.detail, r.map), want, (tag, NAMES[s], q))
                total, n = total + want.tally, n + 1
            # the first four counts: exactly the unpack call's for the same arguments, and its pairs the marks'
            counts, ref_member = m.acc.unpack(r.mm, r.rm, NAMES[s], pairs=True)
            assert counts.tolist() == want.counts[:4].tolist(), (tag, NAMES[s])
            at = np.flatnonzero(want.marks["pair"] >= 0)
            assert np.array_equal(ref_member[want.marks["pair"][at]], want.marks["ref_member"][at])
            if spec is not None and len(m.a_row):
                M.check_not_vacuous(want, r.fam, m.a_row, spec, truth, few=few)
        words, results = r.map.tally()
        assert results == n and words.dtype == np.uint32 and np.array_equal(words, total), tag
    return wants


# ---- 1. final rows, lists, specs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_final_rows_at_the_wave_edges_and_none(n):
    with _accumulator(n) as m:
        assert m.n_final == n == len(m.a_row)
        fam = _lists(m)
        truth = M.truths(fam, m.a_row, m.r_row, seed=n)
        for spec in M.specs(fam, seed=n):
            w = _check(m, fam, spec, truth, (spec.name, n), calls=2, few=n < 63)
            assert w[U.NEAREST].counts[0] == n and (n == 0 or w[U.NEAREST].counts[1] > 0)
        _check(m, fam, None, None, ("no spec, no truth", n))


@pytest.mark.parametrize("size", ["mid", "big"])
def test_lists_of_1_2_63_64_on_257_rows_and_every_spec_on_five_thousand(request, size):
    m = request.getfixturevalue(size)
    fam = _lists(m, list(itertools.product((1, 2, 63, 64), (1, 2, 63, 64))) if size == "mid" else None)
    truth = M.truths(fam, m.a_row, m.r_row, seed=1)
    unpacked = {s: U.call(fam, m.a_row, m.r_row, s) for s in U.STRATEGIES}      # (the pairs do not depend on the codes: solved once)
    for spec in M.specs(fam, seed=3):
        w = _check(m, fam, spec, truth, (spec.name, size), unpacked=unpacked)
        assert w[U.DISTRIBUTE].counts[1] == w[U.NEAREST].counts[1] > m.n_final
    if size == "mid":
        na, nr = U.row_sizes(fam, m.a_row, m.r_row)
        assert {1, 2, 63, 64} <= set(na.tolist()) and {1, 2, 63, 64} <= set(nr.tolist())


def test_moving_rows_without_members(mid, big):
    for m in (mid, big):
        fam = _lists(m, empty_every=3)
        spec = M.specs(fam, seed=5)[1]
        w = _check(m, fam, spec, M.truths(fam, m.a_row, m.r_row, seed=2), ("empty moving rows", m.n_final))
        na = np.diff(fam.mov_off)[np.asarray(m.a_row, np.int64)]
        assert (na == 0).sum() >= m.n_final // 3 and 0 < w[U.NEAREST].counts[1] == na.sum()


@pytest.mark.parametrize("which", range(7))
def test_the_hostile_families_with_unmatched_members_and_ties(large, which):
    """tests/unpack_check.py's families over a windowed accumulator whose final rows leave moving rows unnamed: lattice and coincident
    members tie under "nearest" (the solver's tie order is the statement's), members of unnamed rows keep the unmatched mark"""
    name, fam, want = _families(large)[which]
    if name in ("lattice", "coincident"):
        assert U.tied_rows(fam, large.a_row, large.r_row) > 0
    assert large.n_final < large.n_mov
    truth = M.truths(fam, large.a_row, large.r_row, seed=which)
    spec = M.specs(fam, seed=which)[which % 5]
    w = _check(large, fam, spec, truth, name, unpacked=want)
    unmatched = w[U.NEAREST].marks[w[U.NEAREST].marks["pair"] < 0]
    assert len(unmatched) > 0 and set(unmatched["flags"].tolist()) == {0, M.TRUTH_KNOWN}


def test_with_and_without_detail_truth_tally_and_marks(mid):
    m = mid
    fam = _lists(m)
    spec = M.specs(fam, seed=2)[2]
    truth = M.truths(fam, m.a_row, m.r_row, seed=3)
    for with_detail, with_truth, with_tally, with_marks in itertools.product((True, False), repeat=4):
        t = truth if with_truth else None
        with _Resident(m, fam, spec, t, with_tally, detail=with_detail) as r:
            for s in U.STRATEGIES:
                want = M.host_unpack_map(m.a_row, m.r_row, fam, s, spec if with_detail else spec._replace(col_of_label=None), t)
                got = m.acc.unpack_map(r.mm, r.rm, NAMES[s], r.detail, r.map, marks=with_marks)
                _same(got, want, (with_detail, with_truth, with_tally, with_marks, s), marks=with_marks)
                assert with_detail or not (want.marks["flags"] & M.RANKED).any()
            words, results = r.map.tally()
            assert results == 2 and (words is None) == (not with_tally)
            if with_tally:
                assert np.array_equal(words, sum(M.host_unpack_map(m.a_row, m.r_row, fam, s, spec, t).tally for s in U.STRATEGIES))
    # a detail without type rows or without columns ranks nothing
    from same_amd import windows as W

    with _Resident(m, fam, spec, truth, detail=False) as r:
        for col, types in ((None, spec.ref_types), (None, None)):
            bare = W.DeviceUnpackDetail(r.rm, spec.n_labels, col, types)
            try:
                _same(m.acc.unpack_map(r.mm, r.rm, "nearest", bare, r.map),
                      M.host_unpack_map(m.a_row, m.r_row, fam, U.NEAREST, spec._replace(col_of_label=None), truth), "bare detail")
            finally:
                bare.close()


def test_the_tally_after_three_calls_and_after_a_reset(mid):
    m = mid
    fam = _lists(m)
    spec = M.specs(fam, seed=7)[1]
    truth = M.truths(fam, m.a_row, m.r_row, seed=7)
    want = {s: M.host_unpack_map(m.a_row, m.r_row, fam, s, spec, truth) for s in U.STRATEGIES}
    with _Resident(m, fam, spec, truth) as r:
        words, results = r.map.tally()
        assert results == 0 and not words.any() and words.shape == (len(fam.mov_code), 3)
        for s in (U.NEAREST, U.DISTRIBUTE, U.NEAREST):
            m.acc.unpack_map(r.mm, r.rm, NAMES[s], r.detail, r.map, marks=False)
        words, results = r.map.tally()
        assert results == 3 and np.array_equal(words, 2 * want[U.NEAREST].tally + want[U.DISTRIBUTE].tally)
        assert words[:, 0].max() == 3 and (words[:, 2] > 0).any() and (words[:, 1] <= words[:, 0]).all()
        s0 = m.ctx.stats()
        r.map.reset()
        assert _spent(m.ctx, s0) == (0, 1, 0, 1)
        s0 = m.ctx.stats()
        words, results = r.map.tally()
        assert _spent(m.ctx, s0) == (0, 0, 1, 1) and results == 0 and not words.any()
        m.acc.unpack_map(r.mm, r.rm, "distribute", r.detail, r.map)
        words, results = r.map.tally()
        assert results == 1 and np.array_equal(words, want[U.DISTRIBUTE].tally)
    with _Resident(m, fam, spec, truth, tally=False) as r:
        from same_amd import _lib

        out = np.full(3 * len(fam.mov_code), 7, np.uint32)
        with r.map.ctx.lock:
            rc = r.map.ctx.lib.same_unpack_map_tally(r.map.handle, out.ctypes.data, None)
        assert rc == _lib.SAME_EINVAL and (out == 7).all()
        r.map.reset()
        assert r.map.tally() == (None, 0)


# ---- 2. the protocol ---------------------------------------------------------------------------------------------------------------------------
def test_the_call_twice_between_the_other_reader_calls_and_what_it_asks_of_the_runtime(big):
    """(launches, fills, copies, waits) as include/same_hip.h states them: two launches and one 16-byte copy more than
    same_merge_acc_unpack, with out_marks one copy more, no wait more; no fill once the context's slot of the map is laid"""
    from same_amd import windows as W

    m = big
    fam = _lists(m)
    spec = M.specs(fam, seed=4)[2]
    truth = M.truths(fam, m.a_row, m.r_row, seed=4)
    frames = m.frames
    frames.label_codes_on_device()
    mov_q, ref_q = UF.member_features(fam, 3, 2, 1)
    sec_q = C.quantize(C.float_columns(m.n_mov, 3, 1))[0], C.quantize(C.float_columns(m.n_ref, 2, 2))[0]
    others = []
    with _Resident(m, fam, spec, truth) as r:
        try:
            detail = W.DeviceScoreDetail(frames.dmov, None, 1, 4, None)
            others.append(detail)
            smap = W.DeviceScoreMap(frames.dmov, frames.dref, None, True, m.ctx)
            others.append(smap)
            sfeat = W.DeviceScoreFeatures(frames.dmov, frames.dref, sec_q[0], sec_q[1], None, 1)
            others.append(sfeat)
            ufeat = W.DeviceUnpackFeatures(r.mm, r.rm, mov_q, ref_q, None, 1)
            others.append(ufeat)
            flat = lambda d: [np.asarray(v).tolist() for _k, v in sorted(d.items())]
            readers = {
                "score": lambda: m.acc.score(frames.dmov, frames.dref, None).tolist(),
                "detail": lambda: flat(m.acc.score_detail(frames.dmov, frames.dref, None, detail)),
                "map": lambda: [np.asarray(x).tolist() for x in m.acc.score_map(frames.dmov, frames.dref, None, detail, smap)],
                "features": lambda: flat(m.acc.score_features(frames.dmov, frames.dref, sfeat)[0]),
                "unpack": lambda: [x.tolist() for x in m.acc.unpack(r.mm, r.rm, "nearest", pairs=True)],
                "unpack detail": lambda: flat(m.acc.unpack_detail(r.mm, r.rm, "nearest", r.detail, detail)),
                "unpack features": lambda: [np.asarray(x).tolist() for x in m.acc.unpack_features(r.mm, r.rm, "nearest", ufeat)[:1]],
            }
            before = {k: f() for k, f in readers.items()}
            want = {s: M.host_unpack_map(m.a_row, m.r_row, fam, s, spec, truth) for s in U.STRATEGIES}
            s0 = m.ctx.stats()
            m.acc.unpack_map(r.mm, r.rm, "nearest", r.detail, r.map)        # (the context's slot of this map is laid here: two fills)
            assert _spent(m.ctx, s0) == (4, 2, 4, 2)
            log = []
            steps = [(U.NEAREST, True, True), (U.NEAREST, True, True), (U.DISTRIBUTE, False, True), (U.DISTRIBUTE, True, False),
                     (U.NEAREST, False, False), (U.NEAREST, True, True)]
            for q, (s, marks, with_detail) in enumerate(steps):
                s0 = m.ctx.stats()
                got = m.acc.unpack_map(r.mm, r.rm, NAMES[s], r.detail if with_detail else None, r.map, marks=marks)
                log.append(_spent(m.ctx, s0))
                _same(got, want[s] if with_detail else M.host_unpack_map(m.a_row, m.r_row, fam, s, spec._replace(col_of_label=None), truth),
                      q, marks=marks)
                # the unpack call for the same rows, counts only: what this call is measured against
                s0 = m.ctx.stats()
                m.acc.unpack(r.mm, r.rm, NAMES[s])
                base = _spent(m.ctx, s0)
                assert base == (2, 0, 2, 2), base
                extra = tuple(a - b for a, b in zip(log[-1], base))
                assert extra == (2, 0, 1 + marks, 0), (q, extra)
                # the other readers between the calls: their answers unchanged, and nothing laid again
                s0 = m.ctx.stats()
                for k, f in readers.items():
                    assert f() == before[k], (q, k)
                assert _spent(m.ctx, s0)[1] == 0
            print(log)
            words, results = r.map.tally()
            n_near = 1 + sum(1 for s, _m, _d in steps if s == U.NEAREST)
            assert results == 1 + len(steps)
            assert np.array_equal(words, n_near * want[U.NEAREST].tally + (len(steps) + 1 - n_near) * want[U.DISTRIBUTE].tally)
        finally:
            for h in reversed(others):
                h.close()


def test_no_final_row_and_no_pair_ask_what_the_unpack_call_asks():
    from same_amd import windows as W

    with _accumulator(0) as m:
        fam = _lists(m)
        truth = M.truths(fam, m.a_row, m.r_row, seed=0)
        assert (truth >= 0).any() and (truth < 0).any()
        with _Resident(m, fam, M.specs(fam)[1], truth) as r:
            for q in range(2):
                s0 = m.ctx.stats()
                counts, marks = m.acc.unpack_map(r.mm, r.rm, "nearest", r.detail, r.map)
                assert _spent(m.ctx, s0) == (0, 0, 0, 0) and counts.tolist() == [0] * 6
                assert marks.tobytes() == M.unmatched_marks(len(truth), truth).tobytes()
            words, results = r.map.tally()
            assert results == 2 and not words.any()
    with _accumulator(64) as m:
        fam = _lists(m)
        none = U.Members(np.zeros(m.n_mov + 1, np.int64), np.zeros((0, 2)), np.zeros(0, np.int32), fam.ref_off, fam.ref_xy, fam.ref_code)
        with _Resident(m, none) as r:
            m.acc.unpack_map(r.mm, r.rm, "nearest", None, r.map)       # (the unpack buffer and the slot are laid here)
            s0 = m.ctx.stats()
            counts, marks = m.acc.unpack_map(r.mm, r.rm, "nearest", None, r.map)
            assert _spent(m.ctx, s0) == (1, 0, 1, 1)
            assert counts[0] == 64 and not counts[[1, 2, 4, 5]].any() and len(marks) == 0
        # members, but none on a row a final row names... cannot be: identical frames name every row.  One member each instead, and a
        # truth for all: every mark comes from the device
        fam1 = _lists(m, [(1, 1)])
        truth = M.truths(fam1, m.a_row, m.r_row, seed=1)
        _check(m, fam1, M.specs(fam1)[0], truth, "one member each", few=True)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_the_create_call_refuses_what_the_header_states(mid):
    from same_amd import _lib
    from same_amd import windows as W

    m = mid
    fam = _lists(m)
    with _Resident(m, fam) as r:
        lib, ctx = m.ctx.lib, m.ctx
        m_m, m_r = len(fam.mov_code), len(fam.ref_code)

        def create(truth, tally=1, mm=r.mm, rm=r.rm):
            h = ctypes.c_void_p()
            t = None if truth is None else np.ascontiguousarray(truth, np.int32)
            with ctx.lock:
                rc = lib.same_unpack_map_create(mm.handle, rm.handle, None if t is None else t.ctypes.data, tally, ctypes.byref(h))
                if h.value:
                    lib.same_unpack_map_destroy(h)
            return rc

        ok = np.full(m_m, -1, np.int32)
        ok[0], ok[-1] = m_r - 1, 0
        assert create(None) == 0 and create(ok) == 0 and create(ok, 0) == 0
        for bad in (-2, m_r, 2**31 - 1):
            t = ok.copy()
            t[m_m // 2] = bad
            assert create(t) == _lib.SAME_EINVAL, bad
        with pytest.raises(ValueError, match="truth_member has shape"):
            W.DeviceUnpackMap(r.mm, r.rm, ok[:-1])


def _raw(m, r, strategy, marks, counts, acc=None, mm=None, rm=None, detail="own", map_=None):
    acc = m.acc if acc is None else acc
    d = r.detail if detail == "own" else detail
    with acc.ctx.lock:
        return acc.ctx.lib.same_merge_acc_unpack_map(acc.handle, (mm or r.mm).handle, (rm or r.rm).handle, strategy,
                                                     None if d is None else d.handle, (map_ or r.map).handle,
                                                     None if marks is None else marks.ctypes.data, counts.ctypes.data)


def test_the_call_refuses_what_the_header_states_and_leaves_the_outputs_untouched(big):
    from same_amd import _lib
    from same_amd import windows as W

    m = big
    fam = _lists(m)
    spec = M.specs(fam, seed=6)[1]
    truth = M.truths(fam, m.a_row, m.r_row, seed=6)
    want = {s: M.host_unpack_map(m.a_row, m.r_row, fam, s, spec, truth) for s in U.STRATEGIES}
    n = len(fam.mov_code)
    with _Resident(m, fam, spec, truth) as r, _Resident(m, fam, spec, truth) as other:
        marks, counts = np.full(n * 16 + 16, 0xA5, np.uint8), np.full(8, -5, np.int64)

        def refused(code, **kw):
            rc = _raw(m, r, kw.pop("strategy", U.NEAREST), marks, counts, **kw)
            return rc == code and (marks == 0xA5).all() and (counts == -5).all()

        def good(s=U.NEAREST):
            _same(m.acc.unpack_map(r.mm, r.rm, NAMES[s], r.detail, r.map), want[s], ("good", s))
            return True

        assert good()
        assert refused(_lib.SAME_EINVAL, map_=other.map)                     # a map made for other members
        assert refused(_lib.SAME_EINVAL, detail=other.detail)                # a detail made for other reference members
        assert refused(_lib.SAME_EINVAL, strategy=2)                         # the unpack call's own: an unknown strategy,
        assert refused(_lib.SAME_EINVAL, mm=r.rm)                            # members of the other section (and not the map's),
        fresh = W.MergeAccumulator(m.ctx)
        try:
            fresh.begin(16)
            assert refused(_lib.SAME_EINVAL, acc=fresh)                      # an accumulator before its finish
        finally:
            fresh.close()
        assert good() and good(U.DISTRIBUTE)
        made = []
        try:
            # one moving member's X is NaN, on a row a final row names: infeasible under NEAREST alone -- known only after the last
            # wait, when the marks' copy has landed in the map's own block: the caller's marks are not written
            xy = fam.mov_xy.copy()
            xy[fam.mov_off[int(m.a_row[9])], 0] = np.nan
            nan_m = W.DeviceMembers(m.frames.dmov, fam.mov_off, xy, r.fam.mov_code)
            made.append(nan_m)
            nan_map = W.DeviceUnpackMap(nan_m, r.rm, truth, True)
            made.append(nan_map)
            assert refused(_lib.SAME_ERANGE, mm=nan_m, map_=nan_map)
            assert good()
            nan_map.reset()                                                  # (the header: after SAME_ERANGE reset the tally)
            words, results = nan_map.tally()
            assert results == 0 and not words.any()
            _same(m.acc.unpack_map(nan_m, r.rm, "distribute", r.detail, nan_map), want[U.DISTRIBUTE], "distribute reads no XY")
            with pytest.raises(_lib.SameHipError, match="infeasible") as e:
                m.acc.unpack_map(nan_m, r.rm, "nearest", r.detail, nan_map)
            assert e.value.code == _lib.SAME_ERANGE
            # a final row's members against an empty reference list
            sizes = np.diff(fam.ref_off)
            keep = np.ones(len(fam.ref_xy), bool)
            row = int(m.r_row[5])
            keep[fam.ref_off[row]:fam.ref_off[row + 1]] = False
            sizes[row] = 0
            hollow = W.DeviceMembers(m.frames.dref, np.concatenate(([0], np.cumsum(sizes))), fam.ref_xy[keep], r.fam.ref_code[keep])
            made.append(hollow)
            hollow_map = W.DeviceUnpackMap(r.mm, hollow, None, True)
            made.append(hollow_map)
            for s in U.STRATEGIES:
                assert refused(_lib.SAME_ERANGE, strategy=s, rm=hollow, detail=None, map_=hollow_map), s
            assert good() and good(U.DISTRIBUTE)
        finally:
            for h in reversed(made):
                h.close()
        # the counts are asked for
        with m.acc.ctx.lock:
            rc = m.acc.ctx.lib.same_merge_acc_unpack_map(m.acc.handle, r.mm.handle, r.rm.handle, U.NEAREST, None, r.map.handle, None, None)
        assert rc == _lib.SAME_EINVAL
        with pytest.raises(ValueError, match="strategy must be one of"):
            m.acc.unpack_map(r.mm, r.rm, "closest", r.detail, r.map)
        assert good()
