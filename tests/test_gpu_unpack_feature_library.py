"""same_merge_acc_unpack_features and the same_unpack_features_* / same_unpack_zone_* calls (csrc/window_unpack_feature.hip) driven at the
library against tests/unpack_feature_check.py's `host_unpack_features` -- `host_unpack`'s scipy statement with numpy sums, nothing of
libsame_hip in it -- on merged accumulators made as tests/test_gpu_unpack_library.py makes them (the members must belong to the sections
the pass ran over).  Every assertion is exact equality: the int64 words of `out`, the bits of out_d2, the entries of out_ref_member.

The inputs: 0, 1, 63, 64, 65, 257 and about 5000 final rows; member lists of 1, 2, 63 and 64 on either side; moving rows without
members; both strategies; every pair of column counts from 0, 1, 63, 64, 65, 300; 1, 2, 64 and 256 groups with cells in none, and no
group array; a bin summing more than 5000 values of +2**30 and of -2**30; §5.19's zone families restated on members; the call twice
and between score, detail, map, feature, unpack and unpack-detail calls, with the runtime calls include/same_hip.h states; the
small-capacity protocol; every refusal it states, with the outputs untouched.  No test passes a non-finite XY on purpose to anything but
the refusal that names it."""
import contextlib
import ctypes
import itertools
import types

import numpy as np
import pandas as pd
import pytest

import feature_check as C
import unpack_check as U
import unpack_feature_check as UF
from test_gpu_feature_library import COLUMN_COUNTS, _flat
from test_gpu_score_library import ONE_WINDOW, _relabelled, _synthetic
from test_gpu_unpack_library import NAMES, _merged, _spent

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _merged_without_a_window(ref, mov, cols, op):
    """`_merged`'s recipe with no window collected: an accumulator whose merge ends with no final row"""
    from same_amd.incumbent import _begin_accumulators, _merge_on_device
    from same_amd.window_api import _WindowJob

    job = _WindowJob(ref, mov, list(cols), None, None, None, dict(op), None, False, None)
    frames, own = job.device_frames("device")
    try:
        accs = _begin_accumulators(job, frames, frames.worker_contexts(1), [0, len(job.todo)], None)
        done = _merge_on_device(job, frames, accs, None)
        empty = np.zeros(0, np.int32)
        yield types.SimpleNamespace(acc=done, ctx=done.ctx, frames=frames, n_final=done.n_final, a_row=empty, r_row=empty, n_mov=len(mov),
                                    n_ref=len(ref), made={})
    finally:
        if own:
            frames.close()


@contextlib.contextmanager
def _accumulator(n):
    """a merged accumulator of n final rows and the frames it ran over (tests/test_gpu_feature_library.py's recipes): identical frames
    of n cells under one neighbour keep every cell on itself; one row: seventy moving copies around one reference cell; none: no window"""
    if n == 0:
        ref, mov, cols = _synthetic(70, 5)
        with _merged_without_a_window(ref, mov, cols, ONE_WINDOW) as m:
            yield m
        return
    if n == 1:
        ref, _mov, cols = _synthetic(70, 5)
        ref = ref.copy()
        ref.loc[ref.index[0], ["X", "Y"]] = (1000.0, 1000.0)
        mov = pd.concat([ref.iloc[[0]]] * 70, ignore_index=True)
        blob = np.random.default_rng(6).uniform(-5.0, 5.0, (70, 2))
        mov["X"], mov["Y"], mov["Cell_Num_Old"] = 1000.0 + blob[:, 0], 1000.0 + blob[:, 1], np.arange(70)
        mov["cell_type"] = np.asarray(cols)[np.arange(70) % len(cols)]
        op = ONE_WINDOW
    else:
        ref, _mov, cols = _synthetic(n, 9)
        mov, op = _relabelled(ref), dict(ONE_WINDOW, knn=1)
    with _merged(ref, mov, cols, op) as m:
        yield m


@pytest.fixture(scope="module")
def big():
    with _accumulator(5000) as m:
        print("big: n_final", m.n_final)
        assert 4000 < m.n_final <= 5000
        yield m


@pytest.fixture(scope="module")
def mid():
    with _accumulator(257) as m:
        assert m.n_final == 257
        yield m


def _lists(m, sizes=None, seed=21, empty_every=0):
    """member lists over the accumulator's sections: `sizes` (na, nr) cycled over the final rows (None: every (na, nr) of 1..6 x 1..6),
    1 .. 3 members on the rows no final row names; empty_every: every so-manieth final row's moving row without members"""
    rng = np.random.default_rng(seed)
    n = m.n_final
    if sizes is None:
        na, nr = U.grid_sizes(n)
    else:
        combos = np.array(sizes)
        at = np.arange(n) % len(combos)
        na, nr = combos[at, 0], combos[at, 1]
    if empty_every:
        na = na.copy()
        na[::empty_every] = 0
    return U._build(rng, *U._sizes(rng, np.asarray(m.a_row, np.int64), np.asarray(m.r_row, np.int64), m.n_mov, m.n_ref, na, nr))


class _Resident:
    """a family's members and its features (and zone) beside the accumulator's sections, closed on exit in the order the header asks"""

    def __init__(self, m, fam, mov_q, ref_q, g, G, zone=None):
        from same_amd import windows as W

        self.made = []
        try:
            self.mm = self._keep(W.DeviceMembers(m.frames.dmov, fam.mov_off, fam.mov_xy, fam.mov_code))
            self.rm = self._keep(W.DeviceMembers(m.frames.dref, fam.ref_off, fam.ref_xy, fam.ref_code))
            self.feats = self._keep(W.DeviceUnpackFeatures(self.mm, self.rm, mov_q if mov_q.shape[1] else None,
                                                           ref_q if ref_q.shape[1] else None, g, G))
            self.zone = None if zone is None else self._keep(W.DeviceUnpackZone(self.feats, *zone))
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


def _same(got, want, tag):
    """the call's answer (windows.MergeAccumulator.unpack_features with d2 and pairs) against the statement's"""
    counts, words, d2, ref_member = got
    flat = np.concatenate((counts, _flat(words)))
    assert flat.dtype == np.int64 and flat.shape == want.out.shape, (tag, flat.shape, want.out.shape)
    bad = np.flatnonzero(flat != want.out)
    assert len(bad) == 0, (tag, bad[:8].tolist(), flat[bad[:8]].tolist(), want.out[bad[:8]].tolist())
    assert ref_member.dtype == np.int64 and np.array_equal(ref_member, want.ref_member), tag
    want_d2 = np.full(len(want.ref_member), np.nan) if want.d2 is None else want.d2
    assert C.same_bits(d2, want_d2), (tag, np.flatnonzero(~(np.isnan(d2) & np.isnan(want_d2)) & (d2 != want_d2))[:8].tolist())


def _check(m, fam, mov_q, ref_q, g, G, zone=None, tag="", strategies=U.STRATEGIES, calls=1, vacuity=None):
    """the call on these inputs against the statement, for the strategies, `calls` times each -> the statement's answers"""
    wants = {}
    with _Resident(m, fam, mov_q, ref_q, g, G, zone) as r:
        for s in strategies:
            wants[s] = want = UF.host_unpack_features(m.a_row, m.r_row, fam, s, mov_q, ref_q, g, G, zone)
            for q in range(calls):
                _same(m.acc.unpack_features(r.mm, r.rm, NAMES[s], r.feats, r.zone, d2=True, pairs=True), want, (tag, NAMES[s], q))
            # the first four words: exactly the unpack call's for the same arguments
            assert m.acc.unpack(r.mm, r.rm, NAMES[s]).tolist() == want.out[:4].tolist(), (tag, NAMES[s])
            if vacuity is not None:
                UF.check_not_vacuous(want, fam, m.a_row, m.r_row, G, mov_q.shape[1] + ref_q.shape[1], 0 if zone is None else len(zone[2]) - 1,
                                     vacuity)
    return wants


def _features(fam, F_m=3, F_r=2, seed=1):
    return UF.member_features(fam, F_m, F_r, seed)


# ---- 1. final rows, lists, zones ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_final_rows_at_the_wave_edges_and_none(n):
    with _accumulator(n) as m:
        assert m.n_final == n == len(m.a_row)
        fam = _lists(m)
        mov_q, ref_q = _features(fam)
        g = UF.member_groups(fam, 2, 4)
        w = _check(m, fam, mov_q, ref_q, g, 2, tag=("no zone", n), calls=2)
        assert w[U.NEAREST].out[0] == n and (n == 0 or w[U.NEAREST].out[1] > 0)
        for name, zfam, zone in UF.member_zone_families(m.a_row, m.r_row, fam):
            _check(m, zfam, mov_q, ref_q, g, 2, zone, tag=(name, n))


@pytest.mark.parametrize("size", ["mid", "big"])
def test_all_zone_families_on_257_rows_with_lists_of_1_2_63_64_and_on_five_thousand(request, size):
    """257 rows: lists of 1, 2, 63 and 64 on either side, every family under both strategies; 5000 rows: lists of 1 .. 6, every family
    under DISTRIBUTE and three of them under NEAREST too (the statement's 5000 scipy solves per family are what a case costs)"""
    m = request.getfixturevalue(size)
    fam = _lists(m, list(itertools.product((1, 2, 63, 64), (1, 2, 63, 64))) if size == "mid" else None)
    mov_q, ref_q = _features(fam)
    g = UF.member_groups(fam, 3, 5)
    _check(m, fam, mov_q, ref_q, g, 3, tag=("no zone", m.n_final), vacuity="")
    for name, zfam, zone in UF.member_zone_families(m.a_row, m.r_row, fam):
        both = size == "mid" or name in ("scattered", "lattice ties", "far corner")
        w = _check(m, zfam, mov_q, ref_q, g, 3, zone, tag=(name, m.n_final), strategies=U.STRATEGIES if both else (U.DISTRIBUTE,))
        # the family has its property on the pairs it was laid over
        UF.check_not_vacuous(w[U.DISTRIBUTE], zfam, m.a_row, m.r_row, 3, 5, len(zone[2]) - 1, name)


def test_moving_rows_without_members(mid, big):
    for m in (mid, big):
        fam = _lists(m, empty_every=3)
        mov_q, ref_q = _features(fam)
        zone = UF.member_zone_families(m.a_row, m.r_row, fam)[0]
        w = _check(m, zone[1], mov_q, ref_q, UF.member_groups(fam, 4, 1), 4, zone[2], tag=("empty moving rows", m.n_final))
        na = np.diff(fam.mov_off)[np.asarray(m.a_row, np.int64)]
        assert (na == 0).sum() >= m.n_final // 3 and 0 < w[U.NEAREST].out[1] == na.sum()


# ---- 2. columns, groups, the range ---------------------------------------------------------------------------------------------------------------
def test_every_pair_of_column_counts(mid):
    fam = _lists(mid)
    zone = dict((n, (f, z)) for n, f, z in UF.member_zone_families(mid.a_row, mid.r_row, fam))["scattered"]
    g = UF.member_groups(fam, 5, 3)
    for q, (F_m, F_r) in enumerate(itertools.product(COLUMN_COUNTS, COLUMN_COUNTS)):
        if F_m + F_r == 0:
            continue
        mov_q, ref_q = UF.member_features(fam, F_m, F_r, 10 + q, floats=bool(q % 2))
        _check(mid, zone[0], mov_q, ref_q, g, 5, zone[1] if q % 3 == 0 else None, tag=(F_m, F_r), strategies=(U.STRATEGIES[q % 2],))


def test_column_counts_across_the_tiles_on_five_thousand_rows_with_a_zone(big):
    fam = _lists(big)
    zone = dict((n, (f, z)) for n, f, z in UF.member_zone_families(big.a_row, big.r_row, fam))["scattered"]
    mov_q, ref_q = UF.member_features(fam, 65, 300, 7, floats=False)
    _check(big, zone[0], mov_q, ref_q, UF.member_groups(fam, 70, 3), 70, zone[1], tag="65 + 300", strategies=(U.NEAREST,))


@pytest.mark.parametrize("G", [1, 2, 64, 256, None])
def test_groups_with_cells_in_none_and_no_group_array(big, G):
    fam = _lists(big)
    mov_q, ref_q = _features(fam, 2, 66)
    g = None if G is None else UF.member_groups(fam, G, G)
    w = _check(big, fam, mov_q, ref_q, g, 1 if G is None else G, tag=("groups", G), strategies=(U.DISTRIBUTE,))
    rows = UF.parts(w[U.DISTRIBUTE].out, 1 if G is None else G, 68)["rows"]
    assert (rows[-1] > 0) == (G is not None) and rows.sum() == w[U.DISTRIBUTE].out[1]


@pytest.mark.parametrize("sign", [1, -1])
def test_every_value_at_the_end_of_the_range_in_one_bin(big, sign):
    fam = _lists(big)
    mov_q = np.full((len(fam.mov_code), 2), sign * C.Q_MAX, np.int32)
    ref_q = np.full((len(fam.ref_code), 65), -sign * C.Q_MAX, np.int32)
    w = _check(big, fam, mov_q, ref_q, np.zeros(len(fam.mov_code), np.int32), 1, tag=("range", sign))
    p = UF.parts(w[U.NEAREST].out, 1, 67)
    assert p["rows"][0] > 5000 and p["sums"][0, 0] == sign * C.Q_MAX * p["rows"][0] and abs(int(p["sums"][0, 0])) > 2**42


# ---- 3. the protocol ---------------------------------------------------------------------------------------------------------------------------
def test_the_call_twice_between_the_other_reader_calls_and_what_it_asks_of_the_runtime(big):
    """(launches, fills, copies, waits) as include/same_hip.h states them: without a zone one launch more than same_merge_acc_unpack and
    no wait more; with one four launches, one 32-byte copy and one wait more; an array asked for is one copy more; no fill once laid"""
    from same_amd import windows as W

    m = big
    fam0 = _lists(m)
    name, fam, zone = UF.member_zone_families(m.a_row, m.r_row, fam0)[0]
    assert name == "scattered"
    mov_q, ref_q = _features(fam, 70, 3)
    g = UF.member_groups(fam, 6, 2)
    frames = m.frames
    frames.label_codes_on_device()
    n_mov, n_ref = m.n_mov, m.n_ref
    sec_q = C.quantize(C.float_columns(n_mov, 3, 1))[0], C.quantize(C.float_columns(n_ref, 2, 2))[0]
    others = []
    with _Resident(m, fam, mov_q, ref_q, g, 6, zone) as r:
        try:
            detail = W.DeviceScoreDetail(frames.dmov, None, 1, 4, None)
            others.append(detail)
            smap = W.DeviceScoreMap(frames.dmov, frames.dref, None, True, m.ctx)
            others.append(smap)
            sfeat = W.DeviceScoreFeatures(frames.dmov, frames.dref, sec_q[0], sec_q[1], None, 1)
            others.append(sfeat)
            szone = W.DeviceFeatureZone(sfeat, None, None, C.EDGES)
            others.append(szone)
            cell = W.DeviceUnpackDetail(r.rm, 4, None, None)
            others.append(cell)
            flat = lambda d: [np.asarray(v).tolist() for _k, v in sorted(d.items())]
            readers = {
                "score": lambda: m.acc.score(frames.dmov, frames.dref, None).tolist(),
                "detail": lambda: flat(m.acc.score_detail(frames.dmov, frames.dref, None, detail)),
                "map": lambda: [np.asarray(x).tolist() for x in m.acc.score_map(frames.dmov, frames.dref, None, detail, smap)],
                "features": lambda: flat(m.acc.score_features(frames.dmov, frames.dref, sfeat, szone)[0]),
                "unpack": lambda: [x.tolist() for x in m.acc.unpack(r.mm, r.rm, "nearest", pairs=True)],
                "unpack detail": lambda: flat(m.acc.unpack_detail(r.mm, r.rm, "nearest", cell, detail)),
            }
            before = {k: f() for k, f in readers.items()}
            want = {(s, z): UF.host_unpack_features(m.a_row, m.r_row, fam, s, mov_q, ref_q, g, 6, zone if z else None)
                    for s in U.STRATEGIES for z in (True, False)}
            m.acc.unpack_features(r.mm, r.rm, "nearest", r.feats, r.zone, d2=True, pairs=True)      # (whatever this first call lays is laid)
            log = []
            steps = [(U.NEAREST, True, True, True), (U.NEAREST, True, True, True), (U.DISTRIBUTE, False, False, False),
                     (U.DISTRIBUTE, True, False, False), (U.NEAREST, False, False, True), (U.NEAREST, True, False, True)]
            for q, (s, z, d2, pairs) in enumerate(steps):
                s0 = m.ctx.stats()
                counts, words, dist, ref_member = m.acc.unpack_features(r.mm, r.rm, NAMES[s], r.feats, r.zone if z else None, d2=d2, pairs=pairs)
                log.append(_spent(m.ctx, s0))
                w = want[(s, z)]
                assert np.array_equal(np.concatenate((counts, _flat(words))), w.out), q
                assert dist is None if not d2 else C.same_bits(dist, w.d2), q
                assert ref_member is None if not pairs else np.array_equal(ref_member, w.ref_member), q
                # the unpack call for the same rows, counts only: what this call is measured against
                s0 = m.ctx.stats()
                m.acc.unpack(r.mm, r.rm, NAMES[s])
                base = _spent(m.ctx, s0)
                assert base == (2, 0, 2, 2), base
                extra = tuple(a - b for a, b in zip(log[-1], base))
                assert extra == ((4, 0, 2 + d2 + pairs, 1) if z else (1, 0, 1 + pairs, 0)), (q, extra)
                # the other readers between the calls: their answers unchanged, and nothing laid again
                s0 = m.ctx.stats()
                for k, f in readers.items():
                    assert f() == before[k], (q, k)
                assert _spent(m.ctx, s0)[1] == 0
            print(log)
            # more words than any call before: the sums' buffer is laid again, one fill; the zone's and the unpack buffer are not
            with _Resident(m, fam, *UF.member_features(fam, 301, 302, 5, floats=False), UF.member_groups(fam, 256, 1), 256, zone) as wide:
                s0 = m.ctx.stats()
                m.acc.unpack_features(wide.mm, wide.rm, "distribute", wide.feats, wide.zone)
                assert _spent(m.ctx, s0) == (6, 1, 4, 3)
            s0 = m.ctx.stats()
            got = m.acc.unpack_features(r.mm, r.rm, "nearest", r.feats, r.zone, d2=True, pairs=True)
            assert _spent(m.ctx, s0) == (6, 0, 6, 3)
            _same(got, want[(U.NEAREST, True)], "after the wide call")
        finally:
            for h in reversed(others):
                h.close()


def test_no_final_row_and_no_pair_ask_what_the_unpack_call_asks():
    from same_amd import windows as W

    with _accumulator(0) as m:
        fam = _lists(m)
        mov_q, ref_q = _features(fam)
        with _Resident(m, fam, mov_q, ref_q, None, 1, (None, None, C.EDGES)) as r:
            for z in (None, r.zone):
                s0 = m.ctx.stats()
                counts, words, d2, ref_member = m.acc.unpack_features(r.mm, r.rm, "nearest", r.feats, z, d2=True, pairs=True)
                assert _spent(m.ctx, s0) == (0, 0, 0, 0) and not counts.any() and not _flat(words).any() and len(d2) == len(ref_member) == 0
    with _accumulator(64) as m:
        fam = _lists(m)
        rm_xy = fam.ref_xy
        none = U.Members(np.zeros(m.n_mov + 1, np.int64), np.zeros((0, 2)), np.zeros(0, np.int32), fam.ref_off, rm_xy, fam.ref_code)
        with _Resident(m, none, np.zeros((0, 3), np.int32), UF.member_features(fam, 3, 2, 1)[1], None, 1, (None, None, C.EDGES)) as r:
            m.acc.unpack_features(r.mm, r.rm, "nearest", r.feats, r.zone)      # (the unpack buffer and the sums' are laid here: two fills)
            s0 = m.ctx.stats()
            counts, words, d2, ref_member = m.acc.unpack_features(r.mm, r.rm, "nearest", r.feats, r.zone, d2=True, pairs=True)
            assert _spent(m.ctx, s0) == (1, 0, 1, 1)
            assert counts[0] == 64 and counts[1] == 0 and not _flat(words).any() and len(d2) == 0


def _raw(m, r, strategy, out, out_words=None, d2=None, ref_member=None, capacity=0, acc=None, mm=None, rm=None, feats=None, zone="own"):
    acc = m.acc if acc is None else acc
    z = r.zone if zone == "own" else zone
    with acc.ctx.lock:
        return acc.ctx.lib.same_merge_acc_unpack_features(acc.handle, (mm or r.mm).handle, (rm or r.rm).handle, strategy,
                                                          (feats or r.feats).handle, None if z is None else z.handle, out.ctypes.data,
                                                          len(out) if out_words is None else out_words,
                                                          None if d2 is None else d2.ctypes.data,
                                                          None if ref_member is None else ref_member.ctypes.data, capacity)


def test_arrays_too_small_are_left_alone_and_the_four_counts_filled(mid):
    from same_amd import _lib

    m = mid
    fam0 = _lists(m)
    _name, fam, zone = UF.member_zone_families(m.a_row, m.r_row, fam0)[0]
    mov_q, ref_q = _features(fam)
    g = UF.member_groups(fam, 2, 4)
    with _Resident(m, fam, mov_q, ref_q, g, 2, zone) as r:
        for s in U.STRATEGIES:
            want = UF.host_unpack_features(m.a_row, m.r_row, fam, s, mov_q, ref_q, g, 2, zone)
            pairs = int(want.out[1])
            for capacity in (0, pairs - 1):
                out = np.full(len(want.out) + 2, -5, np.int64)
                d2, ref_member = np.full(pairs + 3, -5.0), np.full(pairs + 3, -5, np.int64)
                rc = _raw(m, r, s, out, d2=d2, ref_member=ref_member, capacity=capacity)
                assert rc == _lib.SAME_EINVAL and out[:4].tolist() == want.out[:4].tolist() and (out[4:] == -5).all(), (s, capacity, rc)
                assert (d2 == -5.0).all() and (ref_member == -5).all()
            out = np.full(len(want.out) + 2, -5, np.int64)
            rc = _raw(m, r, s, out, d2=d2, ref_member=ref_member, capacity=pairs)
            assert rc == 0 and np.array_equal(out[:-2], want.out) and (out[-2:] == -5).all()
            assert C.same_bits(d2[:pairs], want.d2) and (d2[pairs:] == -5.0).all()
            assert np.array_equal(ref_member[:pairs], want.ref_member) and (ref_member[pairs:] == -5).all()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_the_create_calls_refuse_what_the_header_states(mid):
    from same_amd import _lib
    from same_amd import windows as W

    m = mid
    fam = _lists(m)
    m_m, m_r = len(fam.mov_code), len(fam.ref_code)
    mov_q, ref_q = _features(fam)
    with _Resident(m, fam, mov_q, ref_q, None, 1) as r:
        lib, ctx = m.ctx.lib, m.ctx

        def create(mq, F_m, rq, F_r, g, G, mm=r.mm, rm=r.rm):
            h = ctypes.c_void_p()
            ptr = lambda x: None if x is None else x.ctypes.data
            with ctx.lock:
                rc = lib.same_unpack_features_create(mm.handle, rm.handle, ptr(mq), F_m, ptr(rq), F_r, ptr(g), G, ctypes.byref(h))
                if h.value:
                    lib.same_unpack_features_destroy(h)
            return rc

        assert create(mov_q, 3, ref_q, 2, None, 1) == 0 and create(None, 0, ref_q, 2, None, 1) == 0 and create(mov_q, 3, None, 0, None, 256) == 0
        assert create(None, 0, None, 0, None, 1) == _lib.SAME_EINVAL
        assert create(mov_q, -1, ref_q, 2, None, 1) == _lib.SAME_EINVAL and create(mov_q, 3, ref_q, -1, None, 1) == _lib.SAME_EINVAL
        assert create(None, 3, ref_q, 2, None, 1) == _lib.SAME_EINVAL and create(mov_q, 3, None, 2, None, 1) == _lib.SAME_EINVAL
        assert create(mov_q, 3, ref_q, 2, None, 0) == _lib.SAME_EINVAL and create(mov_q, 3, ref_q, 2, None, 257) == _lib.SAME_EINVAL
        wide = np.zeros((m_m, _lib.SAME_FEATURE_MAX_COLUMNS), np.int32)
        assert create(wide, wide.shape[1], None, 0, None, 1) == 0 and create(wide, wide.shape[1], ref_q, 2, None, 1) == _lib.SAME_EINVAL
        for bad in (C.Q_MAX + 1, -C.Q_MAX - 1):
            q = mov_q.copy()
            q[-1, -1] = bad
            assert create(q, 3, ref_q, 2, None, 1) == _lib.SAME_ERANGE
            q = ref_q.copy()
            q[0, 0] = bad
            assert create(mov_q, 3, q, 2, None, 1) == _lib.SAME_ERANGE
        g = np.zeros(m_m, np.int32)
        g[5] = 2
        assert create(mov_q, 3, ref_q, 2, g, 2) == _lib.SAME_ERANGE and create(mov_q, 3, ref_q, 2, g, 3) == 0
        g[5] = -2**31
        assert create(mov_q, 3, ref_q, 2, g, 1) == 0

        def zone_create(mf, rf, e, n_edges=None):
            h = ctypes.c_void_p()
            e = None if e is None else np.ascontiguousarray(e, np.float64)
            ptr = lambda x: None if x is None else x.ctypes.data
            with ctx.lock:
                rc = lib.same_unpack_zone_create(r.feats.handle, ptr(mf), ptr(rf), ptr(e), len(e) if n_edges is None else n_edges, ctypes.byref(h))
                if h.value:
                    lib.same_unpack_zone_destroy(h)
            return rc

        mf, rf = np.full(m_m, 3, np.uint8), np.full(m_r, 3, np.uint8)
        assert zone_create(mf, rf, C.EDGES) == 0 and zone_create(None, None, [0.0, 0.0]) == 0 and zone_create(None, rf, np.arange(65.0)) == 0
        assert zone_create(mf, rf, [1.0]) == _lib.SAME_EINVAL and zone_create(mf, rf, np.arange(66.0)) == _lib.SAME_EINVAL
        assert zone_create(mf, rf, None, 3) == _lib.SAME_EINVAL
        assert zone_create(mf, rf, [0.0, np.nan, 2.0]) == _lib.SAME_EINVAL and zone_create(mf, rf, [0.0, 2.0, 1.0]) == _lib.SAME_EINVAL
        with pytest.raises(ValueError, match="mov_q has shape"):
            W.DeviceUnpackFeatures(r.mm, r.rm, mov_q[:-1], ref_q, None, 1)
        with pytest.raises(ValueError, match="member_group has shape"):
            W.DeviceUnpackFeatures(r.mm, r.rm, mov_q, ref_q, np.zeros(m_m + 1, np.int32), 1)
        with pytest.raises(ValueError, match="ref_flags has shape"):
            W.DeviceUnpackZone(r.feats, mf, rf[:-1], C.EDGES)


def test_the_call_refuses_what_the_header_states_and_leaves_the_outputs_untouched(big):
    from same_amd import _lib
    from same_amd import windows as W

    m = big
    fam0 = _lists(m)
    _name, fam, zone = UF.member_zone_families(m.a_row, m.r_row, fam0)[0]
    mov_q, ref_q = _features(fam)
    g = UF.member_groups(fam, 2, 4)
    want = {s: UF.host_unpack_features(m.a_row, m.r_row, fam, s, mov_q, ref_q, g, 2, zone) for s in U.STRATEGIES}
    words, pairs = len(want[U.NEAREST].out), len(fam.mov_code)
    with _Resident(m, fam, mov_q, ref_q, g, 2, zone) as r, _Resident(m, fam, mov_q, ref_q, g, 2, zone) as other:
        out, d2, ref_member = np.full(words + 3, -5, np.int64), np.full(pairs, -5.0), np.full(pairs, -5, np.int64)

        def untouched(rc, code):
            return rc == code and (out == -5).all() and (d2 == -5.0).all() and (ref_member == -5).all()

        def refused(code, **kw):
            kw.setdefault("capacity", pairs)
            return untouched(_raw(m, r, kw.pop("strategy", U.NEAREST), out, d2=d2, ref_member=ref_member, **kw), code)

        def good(s=U.NEAREST):
            _same(m.acc.unpack_features(r.mm, r.rm, NAMES[s], r.feats, r.zone, d2=True, pairs=True), want[s], ("good", s))
            return True

        assert good()
        assert refused(_lib.SAME_EINVAL, out_words=words - 1)
        assert refused(_lib.SAME_EINVAL, feats=other.feats)                  # features made for other members
        assert refused(_lib.SAME_EINVAL, zone=other.zone)                    # a zone made for other features
        assert refused(_lib.SAME_EINVAL, capacity=-1)
        assert refused(_lib.SAME_EINVAL, strategy=2)                         # the unpack call's own: an unknown strategy,
        assert refused(_lib.SAME_EINVAL, mm=r.rm)                            # members of the other section,
        fresh = W.MergeAccumulator(m.ctx)
        try:
            fresh.begin(16)
            assert refused(_lib.SAME_EINVAL, acc=fresh)                      # an accumulator before its finish
        finally:
            fresh.close()
        assert good() and good(U.DISTRIBUTE)
        made = []
        try:
            # one moving member's X is NaN, on a row a final row names: infeasible under NEAREST alone
            xy = fam.mov_xy.copy()
            xy[fam.mov_off[int(m.a_row[9])], 0] = np.nan
            nan_m = W.DeviceMembers(m.frames.dmov, fam.mov_off, xy, fam.mov_code)
            made.append(nan_m)
            nan_f = W.DeviceUnpackFeatures(nan_m, r.rm, mov_q, ref_q, g, 2)
            made.append(nan_f)
            nan_z = W.DeviceUnpackZone(nan_f, *zone)
            made.append(nan_z)
            assert refused(_lib.SAME_ERANGE, mm=nan_m, feats=nan_f, zone=nan_z)
            assert good()                                                    # the sums the refused call counted are cleared
            assert refused(_lib.SAME_ERANGE, mm=nan_m, feats=nan_f, zone=None)
            assert good()
            # a flagged pair's REFERENCE member XY is not finite: under DISTRIBUTE (which reads no XY) the zone call's own refusal,
            # found by the flag kernel before anything is binned; without a zone nobody reads the XY and the call answers
            j = int(want[U.DISTRIBUTE].ref_member[7])
            rxy = fam.ref_xy.copy()
            rxy[j, 1] = np.inf
            inf_r = W.DeviceMembers(m.frames.dref, fam.ref_off, rxy, fam.ref_code)
            made.append(inf_r)
            inf_f = W.DeviceUnpackFeatures(r.mm, inf_r, mov_q, ref_q, g, 2)
            made.append(inf_f)
            inf_z = W.DeviceUnpackZone(inf_f, None, None, zone[2])
            made.append(inf_z)
            assert refused(_lib.SAME_ERANGE, strategy=U.DISTRIBUTE, rm=inf_r, feats=inf_f, zone=inf_z)
            assert good(U.DISTRIBUTE) and good()
            plain = UF.host_unpack_features(m.a_row, m.r_row, fam, U.DISTRIBUTE, mov_q, ref_q, g, 2)
            rc = _raw(m, r, U.DISTRIBUTE, out, rm=inf_r, feats=inf_f, zone=None)
            assert rc == 0 and np.array_equal(out[:len(plain.out)], plain.out) and (out[len(plain.out):] == -5).all()
            out[:] = -5
            with pytest.raises(_lib.SameHipError, match="not finite") as e:
                m.acc.unpack_features(r.mm, inf_r, "distribute", inf_f, inf_z)
            assert e.value.code == _lib.SAME_ERANGE
            # a final row's members against an empty reference list
            counts = np.diff(fam.ref_off)
            keep = np.ones(len(fam.ref_xy), bool)
            row = int(m.r_row[5])
            keep[fam.ref_off[row]:fam.ref_off[row + 1]] = False
            counts[row] = 0
            hollow = W.DeviceMembers(m.frames.dref, np.concatenate(([0], np.cumsum(counts))), fam.ref_xy[keep], fam.ref_code[keep])
            made.append(hollow)
            hollow_f = W.DeviceUnpackFeatures(r.mm, hollow, mov_q, ref_q[keep], g, 2)
            made.append(hollow_f)
            for s in U.STRATEGIES:
                assert refused(_lib.SAME_ERANGE, strategy=s, rm=hollow, feats=hollow_f, zone=None), s
            assert good() and good(U.DISTRIBUTE)
        finally:
            for h in reversed(made):
                h.close()
        with pytest.raises(ValueError, match="strategy must be one of"):
            m.acc.unpack_features(r.mm, r.rm, "closest", r.feats)
