"""same_merge_acc_unpack (csrc/window_unpack.hip) driven at the library against tests/unpack_check.py's `host_unpack` -- scipy's cdist,
np.tile and linear_sum_assignment from the reference's text, nothing of libsame_hip in it -- over merged accumulators made as
tests/test_gpu_score_library.py makes them.  The call asks that the members were made for the sections the pass ran over, so the
families' hostile lists are laid over those sections' rows.  Every assertion is exact equality."""
import contextlib
import ctypes
import types

import numpy as np
import pytest

import unpack_check as U
from test_gpu_score_library import ONE_WINDOW, _synthetic
from test_gpu_scores import OP, _frames

pytestmark = pytest.mark.gpu

NAMES = {U.DISTRIBUTE: "distribute", U.NEAREST: "nearest"}
N_FAMILIES = 7


@contextlib.contextmanager
def _merged(ref, mov, cols, op):
    """a merged accumulator over the frames, without a table (tests/test_gpu_score_library.py:29-54), and the frames it ran over"""
    from same_amd.incumbent import _begin_accumulators, _merge_on_device
    from same_amd.window_api import _WindowJob

    job = _WindowJob(ref, mov, list(cols), None, None, None, dict(op), None, False, None)
    frames, own = job.device_frames("device")
    try:
        accs = _begin_accumulators(job, frames, frames.worker_contexts(1), [0, len(job.todo)], None)
        pos_of = {id(w): pos for pos, w in job.todo}
        collector = lambda states, windows, *_s: accs[0].collect(states, [w["trim"] for w in windows], [w["window_id"] for w in windows],
                                                                 [pos_of[id(w)] for w in windows])
        for dw in frames.windows([w for _p, w in job.todo], collector=collector):
            assert dw.error is None
        done = _merge_on_device(job, frames, accs, None)
        final = done.final_rows()
        yield types.SimpleNamespace(acc=done, ctx=done.ctx, frames=frames, n_windows=len(job.todo), n_final=done.n_final,
                                    a_row=final["a_row"].copy(), r_row=final["r_row"].copy(), n_mov=len(mov), n_ref=len(ref), made={})
    finally:
        if own:
            frames.close()


@pytest.fixture(scope="module")
def large():
    ref, mov, cols = _frames(1500, 3)
    with _merged(ref, mov, cols, OP) as m:
        print("large:", len(mov), "cells,", m.n_windows, "windows, n_final", m.n_final)
        assert m.n_windows > 1 and m.n_final > 512 and m.n_final % 64 != 0
        yield m
        _close(m)


@pytest.fixture(scope="module")
def tiny():
    ref, mov, cols = _synthetic(70, 5)
    mov = mov.copy()
    mov.loc[mov.index[::7], "Y"] += 1500.0             # ten cells with no reference cell within the radius: at most sixty rows
    with _merged(ref, mov, cols, ONE_WINDOW) as m:
        print("tiny:", m.n_mov, "moving cells,", m.n_windows, "window, n_final", m.n_final)
        assert m.n_windows == 1 and 0 < m.n_final < 64
        yield m
        _close(m)


def _families(m):
    """the families over this accumulator's final rows, the statement's answer per strategy -- made once, never changed"""
    if "families" not in m.made:
        fams = U.families(m.a_row, m.r_row, m.n_mov, m.n_ref, seed=11, library_only=True)
        assert len(fams) == N_FAMILIES
        m.made["families"] = [(name, fam, {s: U.call(fam, m.a_row, m.r_row, s) for s in U.STRATEGIES}) for name, fam in fams]
    return m.made["families"]


def _members(m, fam):
    """the family's lists resident beside the accumulator's sections (kept until the accumulator goes)"""
    from same_amd import windows as W

    held = m.made.setdefault("members", {})
    if id(fam) not in held:
        held[id(fam)] = (fam, W.DeviceMembers(m.frames.dmov, fam.mov_off, fam.mov_xy, fam.mov_code),
                         W.DeviceMembers(m.frames.dref, fam.ref_off, fam.ref_xy, fam.ref_code))
    return held[id(fam)][1:]


def _close(m):
    for _fam, mm, rm in m.made.pop("members", {}).values():        # before the sections
        mm.close()
        rm.close()


def _raw(m, mm, rm, strategy, out=None, capacity=0, acc=None):
    """the call itself -> (rc, counts); counts start as -7"""
    counts = np.full(4, -7, np.int64)
    acc = m.acc if acc is None else acc
    with acc.ctx.lock:
        rc = acc.ctx.lib.same_merge_acc_unpack(acc.handle, mm.handle, rm.handle, strategy, counts.ctypes.data,
                                               None if out is None else out.ctypes.data, capacity)
    return rc, counts


def _spent(ctx, s0):
    s1 = ctx.stats()
    return tuple(s1[k] - s0[k] for k in ("launches", "fills", "copies", "waits"))


def _slice_units(na, nr):
    """the solver slice of a final row in 128-byte units (csrc/assign_solve.h: slice_words), as include/same_hip.h's budget counts them"""
    nc = np.where(na <= nr, nr, nr * -(-na // np.maximum(nr, 1)))
    words = na * nc + na + 2 * nc + (3 * nc + na + 1) // 2 + (na + nc + 7) // 8
    return np.where((na > 0) & (nr > 0), -(-words // 16), 0)


# ---- 1. the families -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(N_FAMILIES))
@pytest.mark.parametrize("size", ["large", "tiny"])
def test_every_family_with_pairs_and_without(request, size, which):
    m = request.getfixturevalue(size)
    name, fam, want = _families(m)[which]
    mm, rm = _members(m, fam)
    for s in U.STRATEGIES:
        counts, ref_member = m.acc.unpack(mm, rm, NAMES[s], pairs=True)
        assert counts.dtype == np.int64 and counts.tolist() == want[s][0].tolist(), (name, s, counts.tolist(), want[s][0].tolist())
        assert ref_member.dtype == np.int64 and np.array_equal(ref_member, want[s][1]), (name, s)
        assert m.acc.unpack(mm, rm, NAMES[s]).tolist() == want[s][0].tolist(), (name, s, "counts only")
    print(size, name, {NAMES[s]: want[s][0].tolist() for s in U.STRATEGIES})
    assert want[U.DISTRIBUTE][0][1] > 0


def test_an_array_too_small_is_left_alone_and_the_counts_filled(large):
    from same_amd import _lib

    name, fam, want = _families(large)[0]
    mm, rm = _members(large, fam)
    for s in U.STRATEGIES:
        pairs = int(want[s][0][1])
        out = np.full(pairs + 3, -5, np.int64)
        for capacity in (0, pairs - 1):
            rc, counts = _raw(large, mm, rm, s, out, capacity)
            assert rc == _lib.SAME_EINVAL and counts.tolist() == want[s][0].tolist() and (out == -5).all(), (s, capacity, rc, counts.tolist())
        rc, counts = _raw(large, mm, rm, s, out, pairs)
        assert rc == 0 and counts.tolist() == want[s][0].tolist() and np.array_equal(out[:pairs], want[s][1]) and (out[pairs:] == -5).all()


# ---- 2. the work buffers' life -----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_history_and_the_score_call_is_not_disturbed(large):
    """one accumulator: small lists, the large lists, small again, strategies alternating, same_merge_acc_score in between -- every
    answer the statement's, the score call's counts the same before, between and after"""
    fams = _families(large)
    small, big = fams[0], fams[6]
    assert big[2][U.NEAREST][0][3] == 96 > small[2][U.NEAREST][0][3] == 6
    frames = large.frames
    frames.label_codes_on_device()
    score = lambda: large.acc.score(frames.dmov, frames.dref).tolist()
    before = score()
    assert before[0] == large.n_final and 0 < before[1] <= before[0]
    for name, fam, want in (small, big, small, fams[5], big, small):
        mm, rm = _members(large, fam)
        for s in (U.NEAREST, U.DISTRIBUTE, U.NEAREST, U.NEAREST, U.DISTRIBUTE):
            counts, ref_member = large.acc.unpack(mm, rm, NAMES[s], pairs=True)
            assert counts.tolist() == want[s][0].tolist() and np.array_equal(ref_member, want[s][1]), (name, s)
            assert score() == before, (name, s)
            assert large.acc.unpack(mm, rm, NAMES[s]).tolist() == want[s][0].tolist(), (name, s)


def test_what_a_call_asks_of_the_runtime(monkeypatch):
    """(launches, fills, copies, waits) as include/same_hip.h states them: a fresh accumulator's first call lays its buffer (one fill),
    every later call none; one launch more per started slice budget, the same answer whatever the budget"""
    ref, mov, cols = _synthetic(200, 7)
    with _merged(ref, mov, cols, ONE_WINDOW) as m:
        assert 64 < m.n_final < 256
        try:
            name, fam, want = _families(m)[0]
            mm, rm = _members(m, fam)
            na, nr = U.row_sizes(fam, m.a_row, m.r_row)
            units = int(_slice_units(na, nr).sum())
            assert units > 40
            log = []
            for step, (s, with_pairs, budget) in enumerate([(U.DISTRIBUTE, False, None), (U.DISTRIBUTE, True, None), (U.NEAREST, False, None),
                                                            (U.NEAREST, True, None), (U.NEAREST, True, 7), (U.NEAREST, False, units),
                                                            (U.NEAREST, False, units - 1), (U.DISTRIBUTE, False, 7)]):
                if budget is None:
                    monkeypatch.delenv("SAME_UNPACK_BUDGET_UNITS", raising=False)
                else:
                    monkeypatch.setenv("SAME_UNPACK_BUDGET_UNITS", str(budget))
                s0 = m.ctx.stats()
                got = m.acc.unpack(mm, rm, NAMES[s], pairs=with_pairs)
                spent = _spent(m.ctx, s0)
                log.append((NAMES[s], with_pairs, budget, spent))
                counts, ref_member = got if with_pairs else (got, None)
                assert counts.tolist() == want[s][0].tolist() and (ref_member is None or np.array_equal(ref_member, want[s][1])), log[-1]
                chunks = 1 if s == U.DISTRIBUTE or budget is None else -(-units // budget)
                assert spent == (1 + chunks, 1 if step == 0 else 0, 3 if with_pairs else 2, 3 if with_pairs else 2), log[-1]
            for entry in log:
                print(entry)
            # rows without members on the moving side only: no pair, no second launch
            empty = U.Members(np.zeros(m.n_mov + 1, np.int64), np.zeros((0, 2)), np.zeros(0, np.int32), fam.ref_off, fam.ref_xy, fam.ref_code)
            from same_amd import windows as W

            none = W.DeviceMembers(m.frames.dmov, empty.mov_off, empty.mov_xy, empty.mov_code)
            try:
                s0 = m.ctx.stats()
                counts, ref_member = m.acc.unpack(none, rm, "nearest", pairs=True)
                assert _spent(m.ctx, s0) == (1, 0, 1, 1) and counts.tolist() == [m.n_final, 0, 0, int(nr.max())] and len(ref_member) == 0
            finally:
                none.close()
        finally:
            _close(m)


# ---- 3. what the calls refuse ------------------------------------------------------------------------------------------------------------------
def test_members_create_checks_its_lists(tiny):
    from same_amd import _lib, windows as W

    sec, n = tiny.frames.dmov, tiny.n_mov
    ones = np.arange(n + 1, dtype=np.int64)
    xy, code = np.zeros((3 * n + 600, 2)), np.zeros(3 * n + 600, np.int32)

    def rc_of(off, m):
        h = ctypes.c_void_p()
        with sec.ctx.lock:
            rc = sec.ctx.lib.same_members_create(sec.handle, off.ctypes.data, xy.ctypes.data, code.ctypes.data, m, ctypes.byref(h))
            if h.value:
                sec.ctx.lib.same_members_destroy(h)
        return rc

    assert rc_of(ones, n) == 0
    assert rc_of(ones + 1, n + 1) == _lib.SAME_EINVAL                       # off[0] != 0
    assert rc_of(ones, n + 1) == _lib.SAME_EINVAL and rc_of(ones, n - 1) == _lib.SAME_EINVAL        # off[n] != m
    dip = ones.copy()
    dip[5] = 7                                                              # row 4 has three members, row 5 minus one
    assert rc_of(dip, n) == _lib.SAME_EINVAL
    longest = ones.copy()
    longest[1:] += 511
    assert rc_of(longest, n + 511) == 0                                     # SAME_ASSIGN_MAX_MEMBERS members in one row
    longest[1:] += 1
    assert rc_of(longest, n + 512) == _lib.SAME_EINVAL
    with pytest.raises(ValueError, match="offsets for a section"):
        W.DeviceMembers(sec, ones[:-1], xy[:n - 1], code[:n - 1])


def test_each_refusal_returns_its_code_with_the_outputs_untouched(large):
    from same_amd import _lib, windows as W

    name, fam, want = _families(large)[0]
    mm, rm = _members(large, fam)
    out = np.full(int(want[U.NEAREST][0][1]), -5, np.int64)
    untouched = lambda rc, counts, code: rc == code and counts.tolist() == [-7] * 4 and (out == -5).all()
    # an unknown strategy; members of the other section on either side
    for args in ((mm, rm, 2), (mm, rm, -1), (rm, rm, U.NEAREST), (mm, mm, U.DISTRIBUTE), (rm, mm, U.DISTRIBUTE)):
        assert untouched(*_raw(large, *args, out, len(out)), _lib.SAME_EINVAL), args[2]
    # before the finish, after plain, after load
    fresh = W.MergeAccumulator(large.ctx)
    try:
        fresh.begin(16)
        assert untouched(*_raw(large, mm, rm, U.DISTRIBUTE, out, len(out), acc=fresh), _lib.SAME_EINVAL)
        W.plain_accumulators([fresh])
        assert untouched(*_raw(large, mm, rm, U.DISTRIBUTE, out, len(out), acc=fresh), _lib.SAME_EINVAL)
        z = np.zeros(4, np.int32)
        fresh.load(np.arange(4), np.arange(4), np.zeros(4, np.uint8), z, z, z, 4, 4)
        _counts, rest = W.resolve_accumulators([fresh], None, None)
        fresh.finish(rest["row"])
        assert fresh.n_final == 4
        assert untouched(*_raw(large, mm, rm, U.DISTRIBUTE, out, len(out), acc=fresh), _lib.SAME_EINVAL)
    finally:
        fresh.close()
    # a final row's members against an empty reference list: both strategies
    counts = np.diff(fam.ref_off)
    keep = np.ones(len(fam.ref_xy), bool)
    r = int(large.r_row[5])
    keep[fam.ref_off[r]:fam.ref_off[r + 1]] = False
    counts[r] = 0
    hollow = W.DeviceMembers(large.frames.dref, np.concatenate(([0], np.cumsum(counts))), fam.ref_xy[keep], fam.ref_code[keep])
    # one member's X is NaN, on a row a final row names: infeasible under NEAREST alone
    xy = fam.mov_xy.copy()
    xy[fam.mov_off[int(large.a_row[9])], 0] = np.nan
    nan = W.DeviceMembers(large.frames.dmov, fam.mov_off, xy, fam.mov_code)
    try:
        for s in U.STRATEGIES:
            assert untouched(*_raw(large, mm, hollow, s, out, len(out)), _lib.SAME_ERANGE), s
        assert untouched(*_raw(large, nan, rm, U.NEAREST, out, len(out)), _lib.SAME_ERANGE)
        assert untouched(*_raw(large, nan, rm, U.NEAREST), _lib.SAME_ERANGE)
        rc, got = _raw(large, nan, rm, U.DISTRIBUTE, out, len(out))
        assert rc == 0 and got.tolist() == want[U.DISTRIBUTE][0].tolist() and np.array_equal(out, want[U.DISTRIBUTE][1])
        with pytest.raises(_lib.SameHipError, match="infeasible") as e:
            large.acc.unpack(nan, rm, "nearest")
        assert e.value.code == _lib.SAME_ERANGE
    finally:
        hollow.close()
        nan.close()
    # and the accumulator answers as ever
    for s in U.STRATEGIES:
        counts, ref_member = large.acc.unpack(mm, rm, NAMES[s], pairs=True)
        assert counts.tolist() == want[s][0].tolist() and np.array_equal(ref_member, want[s][1])
    with pytest.raises(ValueError, match="strategy must be one of"):
        large.acc.unpack(mm, rm, "closest")
