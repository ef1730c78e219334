"""same_merge_acc_score_features and the same_score_features_* / same_feature_zone_* calls (csrc/window_score_feature.hip) driven at the
library against tests/feature_check.py's `host_features` -- plain numpy, nothing of libsame_hip in it -- on merged accumulators
(tests/test_gpu_score_library.py's `_merged` recipe) over sections and feature matrices the tests make themselves.  Every assertion is
exact equality: the int64 words of `out`, and the bits of out_d2.

The inputs: final rows 0, 1, 63, 64, 65, 257 and about 5000; column counts 0, 1, 63, 64, 65 and 300 a side; 1, 2, 64 and 256 groups with
rows in none, and no group array; every value +2**30 and every value -2**30 in one group; an all-zero column; sections grown past the last
matched row; feature_check's zone families; the call twice and between score, detail and map calls, with the runtime calls
include/same_hip.h states; every refusal it states, with `out` untouched.  No test passes a non-finite XY to a zone call."""
import contextlib
import ctypes
import itertools
import types

import numpy as np
import pandas as pd
import pytest

import feature_check as C
from test_gpu_score_library import ONE_WINDOW, _joint_codes, _merged, _relabelled, _spent, _synthetic  # noqa: F401

pytestmark = pytest.mark.gpu

COLUMN_COUNTS = (0, 1, 63, 64, 65, 300)


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
        yield types.SimpleNamespace(acc=done, ctx=done.ctx, n_final=done.n_final,
                                    job=types.SimpleNamespace(a_row=empty, r_row=empty, mov_xy=frames.mov_sec.xy.copy(), ref_xy=frames.ref_sec.xy.copy()))
    finally:
        if own:
            frames.close()


@contextlib.contextmanager
def _accumulator(n):
    """a merged accumulator of n final rows: identical frames of n cells under one neighbour keep every cell on itself; one row: a
    frame of 70 cells all but one of which lie 1500 away from every reference cell; none: no window collected"""
    if n == 0:
        ref, mov, cols = _synthetic(70, 5)
        with _merged_without_a_window(ref, mov, cols, ONE_WINDOW) as m:
            yield m
        return
    if n == 1:
        # seventy moving copies of reference cell 0 in a blob around it, every other reference cell beyond the radius: the window's
        # matching gives a reference cell one match
        ref, _mov, cols = _synthetic(70, 5)
        ref = ref.copy()
        ref.loc[ref.index[0], ["X", "Y"]] = (1000.0, 1000.0)
        mov = pd.concat([ref.iloc[[0]]] * 70, ignore_index=True)
        blob = np.random.default_rng(6).uniform(-5.0, 5.0, (70, 2))
        mov["X"], mov["Y"], mov["Cell_Num_Old"] = 1000.0 + blob[:, 0], 1000.0 + blob[:, 1], np.arange(70)
        mov["cell_type"] = np.asarray(cols)[np.arange(70) % len(cols)]        # (a job wants both frames to name the same types)
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


@contextlib.contextmanager
def _sections(m, ref_xy=None, grow=(0, 0), seed=0):
    """sections of the accumulator's context over the job's rows (`grow` more on each side, which no final row names): the moving one
    scattered, the reference one at `ref_xy` (None: scattered), label codes all 0"""
    from same_amd import windows as W

    n_mov, n_ref = len(m.job.mov_xy) + grow[0], len(m.job.ref_xy) + grow[1]
    rng = np.random.default_rng(seed)
    mov_xy = rng.random((n_mov, 2)) * 2000
    ref_xy = rng.random((n_ref, 2)) * 2000 if ref_xy is None else np.ascontiguousarray(ref_xy, np.float64)
    assert ref_xy.shape == (n_ref, 2) and np.isfinite(ref_xy).all()
    made = []
    try:
        for xy in (mov_xy, ref_xy):
            made.append(W.DeviceSection(W.Section(xy, np.zeros((len(xy), 1))), np.float64, m.ctx))
            made[-1].set_label_codes(np.zeros(len(xy), np.int32))
        yield made[0], made[1], ref_xy
    finally:
        for h in reversed(made):
            h.close()


def _flat(words):
    return np.concatenate([np.asarray(words[k], np.int64).reshape(-1) for k in ("counts", "rows", "sums", "bin_rows", "bin_sums") if k in words])


def _check(m, dmov, dref, ref_xy, mov_q, ref_q, group_of, G, zone=None, tag="", calls=1):
    """the call on these inputs (zone: feature_check's Zone or None) against the statement, `calls` times -> the words"""
    from same_amd import windows as W

    n_mov = len(dmov.section.xy)
    want, want_d2 = C.host_features(m.job.a_row, m.job.r_row, n_mov, mov_q, ref_q, group_of, G, ref_xy,
                                    None if zone is None else (zone.mov_flags, zone.ref_flags, zone.d2_edges))
    feats = W.DeviceScoreFeatures(dmov, dref, mov_q if mov_q.shape[1] else None, ref_q if ref_q.shape[1] else None, group_of, G)
    dz = None
    try:
        if zone is not None:
            dz = W.DeviceFeatureZone(feats, zone.mov_flags, zone.ref_flags, zone.d2_edges)
        for q in range(calls):
            words, d2 = m.acc.score_features(dmov, dref, feats, dz, d2=True)
            got = _flat(words)
            assert got.dtype == np.int64 and got.shape == want.shape, (tag, got.shape, want.shape)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (tag, q, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
            if zone is not None:
                assert C.same_bits(d2, want_d2), (tag, q, np.flatnonzero(~(np.isnan(d2) & np.isnan(want_d2)) & (d2 != want_d2))[:8].tolist())
            else:
                assert d2 is None
    finally:
        if dz is not None:
            dz.close()
        feats.close()
    return words


def _default_features(n_mov, n_ref, F_m=3, F_r=2, seed=1):
    return C.quantize(C.float_columns(n_mov, F_m, seed))[0], C.quantize(C.float_columns(n_ref, F_r, seed + 1))[0]


# ---- 1. final rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_final_rows_at_the_wave_edges_and_none(n):
    with _accumulator(n) as m:
        print("final rows:", m.n_final)
        assert m.n_final == n == len(m.job.a_row)
        with _sections(m) as (dmov, dref, _xy):
            n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
            mov_q, ref_q = _default_features(n_mov, n_ref)
            g = C.groups(n_mov, 2, 4)
            w = _check(m, dmov, dref, None, mov_q, ref_q, g, 2, tag=("no zone", n), calls=2)
            assert w["counts"][0] == n and w["rows"].sum() == n
            for name, zone in C.zone_families(m.job.a_row, m.job.r_row, n_mov, n_ref):
                with _sections(m, zone.ref_xy) as (dm, dr, xy):
                    w = _check(m, dm, dr, xy, mov_q, ref_q, g, 2, zone, tag=(name, n))
                    assert w["bin_rows"].sum() == w["counts"][3]


def test_all_zone_families_on_257_and_on_five_thousand_final_rows(mid, big):
    for m in (mid, big):
        n_mov, n_ref = len(m.job.mov_xy), len(m.job.ref_xy)
        mov_q, ref_q = _default_features(n_mov, n_ref)
        assert not mov_q[:, 0].any()                          # the all-zero column
        g = C.groups(n_mov, 3, 5)
        seen = {}
        for name, zone in C.zone_families(m.job.a_row, m.job.r_row, n_mov, n_ref):
            with _sections(m, zone.ref_xy) as (dmov, dref, xy):
                w = _check(m, dmov, dref, xy, mov_q, ref_q, g, 3, zone, tag=(name, m.n_final), calls=2)
                seen[name] = (w["counts"].tolist(), w["bin_rows"].tolist())
        print(m.n_final, seen)
        n = m.n_final
        assert seen["no zone pair"][0][2] == 0 and seen["one zone point"][0][2:] == [1, n] and seen["every pair both"][0][2:] == [n, n]
        assert seen["NULL flags"][0][2:] == [n, n] and seen["every pair both"][1][-1] == n
        assert len(seen["B = 1"][1]) == 2 and len(seen["B = 64"][1]) == 65 and seen["3-4-5"][1][0] > 0


# ---- 2. columns, groups, values ------------------------------------------------------------------------------------------------------------
def test_every_pair_of_column_counts(mid):
    with _sections(mid) as (dmov, dref, _xy):
        n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
        g = C.groups(n_mov, 5, 6)
        for F_m, F_r in itertools.product(COLUMN_COUNTS, COLUMN_COUNTS):
            if F_m + F_r:
                _check(mid, dmov, dref, None, C.int_columns(n_mov, F_m, F_m), C.int_columns(n_ref, F_r, 100 + F_r), g, 5, tag=(F_m, F_r))


def test_column_counts_across_the_tiles_on_five_thousand_rows_with_a_zone(big):
    n_mov, n_ref = len(big.job.mov_xy), len(big.job.ref_xy)
    zone = dict(C.zone_families(big.job.a_row, big.job.r_row, n_mov, n_ref))["scattered"]
    g = C.groups(n_mov, 7, 7)
    with _sections(big, zone.ref_xy) as (dmov, dref, xy):
        for F_m, F_r in ((0, 1), (1, 0), (63, 65), (64, 64), (65, 63), (300, 0), (0, 300), (300, 300), (1, 64)):
            _check(big, dmov, dref, xy, C.int_columns(n_mov, F_m, F_m), C.int_columns(n_ref, F_r, 100 + F_r), g, 7, zone, tag=(F_m, F_r))


@pytest.mark.parametrize("G", [1, 2, 64, 256, None])
def test_groups_with_rows_in_none_and_no_group_array(big, G):
    with _sections(big) as (dmov, dref, _xy):
        n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
        mov_q, ref_q = C.int_columns(n_mov, 66, 1), C.int_columns(n_ref, 3, 2)
        g = None if G is None else C.groups(n_mov, G, G)
        w = _check(big, dmov, dref, None, mov_q, ref_q, g, G or 1, tag=("groups", G))
        if G is None:
            assert w["rows"].tolist() == [big.n_final, 0] and w["counts"][1] == big.n_final
        else:
            assert w["rows"][-1] > 0 and w["counts"][1] == big.n_final - w["rows"][-1] and (w["rows"][:G] > 0).sum() >= min(G, 60)


@pytest.mark.parametrize("sign", [1, -1])
def test_every_value_at_the_end_of_the_range_in_one_group(big, sign):
    """5000 x 2**30 is beyond 32 bits by twelve: a 32-bit step anywhere on the sum path shows"""
    with _sections(big) as (dmov, dref, _xy):
        n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
        mov_q, ref_q = np.full((n_mov, 65), sign * C.Q_MAX, np.int32), np.full((n_ref, 2), -sign * C.Q_MAX, np.int32)
        zone = C.Zone(None, None, None, np.array([-1.0, np.inf]))         # every pair zone and subset: d2 = 0, one bin
        w = _check(big, dmov, dref, _xy, mov_q, ref_q, None, 1, zone, tag=("saturated", sign))
        assert w["sums"][0, 0] == sign * big.n_final * C.Q_MAX == w["bin_sums"][0, 0] and abs(int(w["sums"][0, 0])) > 2**42
        assert w["sums"][0, -1] == -sign * big.n_final * C.Q_MAX and w["bin_rows"].tolist() == [big.n_final, 0]


def test_sections_grown_past_the_last_matched_row(big):
    for grow in ((5000, 0), (0, 777), (5000, 777)):
        with _sections(big, grow=grow, seed=3) as (dmov, dref, xy):
            n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
            mov_q, ref_q = _default_features(n_mov, n_ref, 5, 4)
            rng = np.random.default_rng(8)
            zone = C.Zone(xy, rng.integers(0, 4, n_mov).astype(np.uint8), rng.integers(0, 4, n_ref).astype(np.uint8), C.EDGES)
            w = _check(big, dmov, dref, xy, mov_q, ref_q, C.groups(n_mov, 4, 9), 4, zone, tag=("grown", grow), calls=2)
            assert 0 < w["counts"][2] < big.n_final and 0 < w["counts"][3] < big.n_final


# ---- 3. the protocol -----------------------------------------------------------------------------------------------------------------------
def test_the_call_twice_between_score_detail_and_map_calls_and_what_it_asks_of_the_runtime(big):
    from same_amd import windows as W

    m = big
    n_mov, n_ref = len(m.job.mov_xy), len(m.job.ref_xy)
    zone = dict(C.zone_families(m.job.a_row, m.job.r_row, n_mov, n_ref))["scattered"]
    mov_q, ref_q = _default_features(n_mov, n_ref, 70, 3)
    g = C.groups(n_mov, 6, 2)
    want, want_d2 = C.host_features(m.job.a_row, m.job.r_row, n_mov, mov_q, ref_q, g, 6, zone.ref_xy, (zone.mov_flags, zone.ref_flags, zone.d2_edges))
    want_plain, _none = C.host_features(m.job.a_row, m.job.r_row, n_mov, mov_q, ref_q, g, 6)
    with _sections(m, zone.ref_xy) as (dmov, dref, _xy):
        made = [W.DeviceScoreFeatures(dmov, dref, mov_q, ref_q, g, 6)]
        try:
            feats = made[0]
            made.append(W.DeviceFeatureZone(feats, zone.mov_flags, zone.ref_flags, zone.d2_edges))
            dz = made[1]
            made.append(W.DeviceScoreDetail(dmov, None, 1, 2, None))
            made.append(W.DeviceScoreMap(dmov, dref, None, True, m.ctx))
            detail, smap = made[2], made[3]
            score0 = m.acc.score(dmov, dref, None)
            detail0 = m.acc.score_detail(dmov, dref, None, detail)
            map0 = m.acc.score_map(dmov, dref, None, detail, smap)
            m.acc.score_features(dmov, dref, feats, dz, d2=True)               # (whatever this first call lays is laid)
            log = []
            for q, (z, d2) in enumerate(((dz, True), (dz, True), (None, False), (dz, False), (None, False))):
                s0 = m.ctx.stats()
                words, dist = m.acc.score_features(dmov, dref, feats, z, d2=d2)
                log.append(_spent(m.ctx, s0))
                assert np.array_equal(_flat(words), want if z is not None else want_plain), q
                assert dist is None if not d2 else C.same_bits(dist, want_d2), q
                # the other readers between the calls: their words unchanged, and nothing laid again
                s0 = m.ctx.stats()
                assert m.acc.score(dmov, dref, None).tolist() == score0.tolist()
                again = m.acc.score_detail(dmov, dref, None, detail)
                assert all(np.array_equal(again[k], detail0[k]) for k in detail0)
                counts, marks = m.acc.score_map(dmov, dref, None, detail, smap)
                assert counts.tolist() == map0[0].tolist() and np.array_equal(marks, map0[1])
                assert _spent(m.ctx, s0)[1] == 0
            print(log)
            # what the header states: (launches, fills, copies, waits)
            assert log == [(4, 0, 3, 2), (4, 0, 3, 2), (1, 0, 1, 1), (4, 0, 2, 2), (1, 0, 1, 1)]
            # more words than any call before: the sums' buffer is laid again, one fill; the zone's is not
            wide = W.DeviceScoreFeatures(dmov, dref, C.int_columns(n_mov, 301, 1), C.int_columns(n_ref, 302, 2), C.groups(n_mov, 256, 1), 256)
            made.append(wide)
            wide_zone = W.DeviceFeatureZone(wide, zone.mov_flags, zone.ref_flags, zone.d2_edges)
            made.append(wide_zone)
            s0 = m.ctx.stats()
            m.acc.score_features(dmov, dref, wide, wide_zone)
            assert _spent(m.ctx, s0) == (4, 1, 2, 2)
            s0 = m.ctx.stats()
            words, _d = m.acc.score_features(dmov, dref, feats, dz)
            assert _spent(m.ctx, s0) == (4, 0, 2, 2) and np.array_equal(_flat(words), want)
        finally:
            for h in reversed(made):
                h.close()


def test_no_final_row_asks_nothing_of_the_runtime():
    with _accumulator(0) as m:
        with _sections(m) as (dmov, dref, xy):
            from same_amd import windows as W

            n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
            mov_q, ref_q = _default_features(n_mov, n_ref)
            feats = W.DeviceScoreFeatures(dmov, dref, mov_q, ref_q, None, 1)
            zone = W.DeviceFeatureZone(feats, None, None, C.EDGES)
            try:
                for z in (None, zone):
                    s0 = m.ctx.stats()
                    words, d2 = m.acc.score_features(dmov, dref, feats, z, d2=True)
                    assert _spent(m.ctx, s0) == (0, 0, 0, 0) and not _flat(words).any() and (d2 is None or np.isnan(d2).all())
            finally:
                zone.close()
                feats.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_the_create_calls_refuse_what_the_header_states(mid):
    from same_amd import _lib
    from same_amd import windows as W

    lib, lock = mid.ctx.lib, mid.ctx.lock
    with _sections(mid) as (dmov, dref, _xy):
        n_mov, n_ref = len(dmov.section.xy), len(dref.section.xy)
        mq, rq = np.zeros((n_mov, 2), np.int32), np.zeros((n_ref, 2), np.int32)
        g = np.zeros(n_mov, np.int32)

        def create(mov_q=mq, F_m=2, ref_q=rq, F_r=2, group_of=g, n_groups=1):
            h = ctypes.c_void_p()
            ptr = lambda v: None if v is None else v.ctypes.data
            with lock:
                rc = lib.same_score_features_create(dmov.handle, dref.handle, ptr(mov_q), F_m, ptr(ref_q), F_r, ptr(group_of), n_groups, ctypes.byref(h))
            assert rc == 0 or not h.value
            if h.value:
                with lock:
                    lib.same_score_features_destroy(h)
            return rc

        assert create() == 0
        assert create(None, 0, None, 0) == create(F_m=-1) == create(F_r=-1) == _lib.SAME_EINVAL
        assert create(F_m=4096, F_r=1) == create(None, 2) == create(ref_q=None) == _lib.SAME_EINVAL
        assert create(n_groups=0) == create(n_groups=257) == _lib.SAME_EINVAL
        for bad in (2**30 + 1, -2**30 - 1, 2**31 - 1, -2**31):
            for side in (0, 1):
                q = (mq, rq)[side].copy()
                q[-1, -1] = bad
                assert (create(mov_q=q) if side == 0 else create(ref_q=q)) == _lib.SAME_ERANGE, (bad, side)
        ends = mq.copy()
        ends[0, 0], ends[-1, -1] = 2**30, -2**30
        assert create(mov_q=ends) == 0
        for bad_group in (1, 2**31 - 1):
            gg = g.copy()
            gg[n_mov // 2] = bad_group
            assert create(group_of=gg) == _lib.SAME_ERANGE
        assert create(group_of=np.full(n_mov, -5, np.int32)) == 0 and create(group_of=None, n_groups=256) == 0
        with pytest.raises(_lib.SameHipError):
            W.DeviceScoreFeatures(dmov, dref, None, None, None, 1)
        with pytest.raises(ValueError):
            W.DeviceScoreFeatures(dmov, dref, mq[:-1], rq, None, 1)
        feats = W.DeviceScoreFeatures(dmov, dref, mq, rq, g, 1)
        try:
            def zone(edges, n_edges=None):
                h = ctypes.c_void_p()
                e = None if edges is None else np.ascontiguousarray(edges, np.float64)
                with lock:
                    rc = lib.same_feature_zone_create(feats.handle, None, None, None if e is None else e.ctypes.data,
                                                      len(e) if n_edges is None else n_edges, ctypes.byref(h))
                assert rc == 0 or not h.value
                if h.value:
                    with lock:
                        lib.same_feature_zone_destroy(h)
                return rc

            assert zone([0.0, 1.0]) == zone([0.0, 0.0, np.inf, np.inf]) == zone(np.arange(65.0)) == zone([-np.inf, np.inf]) == 0
            assert zone([0.0]) == zone(np.arange(66.0)) == zone(None, 2) == _lib.SAME_EINVAL
            assert zone([0.0, np.nan]) == zone([np.nan, 1.0]) == zone([0.0, 2.0, 1.0]) == _lib.SAME_EINVAL
            with pytest.raises(ValueError):
                W.DeviceFeatureZone(feats, np.zeros(n_mov + 1, np.uint8), None, [0.0, 1.0])
        finally:
            feats.close()


def test_the_call_refuses_what_the_header_states_and_leaves_out_untouched(big):
    from same_amd import _lib
    from same_amd import windows as W

    m = big
    lib, lock = m.ctx.lib, m.ctx.lock
    n_mov, n_ref = len(m.job.mov_xy), len(m.job.ref_xy)
    half_m, half_r = n_mov // 2, n_ref // 2
    assert m.job.a_row.max() >= half_m and m.job.r_row.max() >= half_r
    mov_q, ref_q = _default_features(n_mov, n_ref)
    want, want_d2 = C.host_features(m.job.a_row, m.job.r_row, n_mov, mov_q, ref_q, None, 1, m.job.ref_xy, (None, None, C.EDGES))
    words = W.score_feature_words(1, 5, 3)
    made = []

    def call(acc, dm, dr, feats, zone, n_words=words, d2=True):
        out, dist = np.full(words, -7, np.int64), np.full(n_mov, -7.0)
        with lock:
            rc = lib.same_merge_acc_score_features(acc, dm.handle, dr.handle, None if feats is None else feats.handle,
                                                   None if zone is None else zone.handle, out.ctypes.data, n_words, dist.ctypes.data if d2 else None)
        return rc, out, dist

    with _sections(m, m.job.ref_xy) as (dmov, dref, _xy), _sections(m, m.job.ref_xy, seed=1) as (dmov2, dref2, _xy2):
        try:
            feats, other = W.DeviceScoreFeatures(dmov, dref, mov_q, ref_q, None, 1), W.DeviceScoreFeatures(dmov2, dref2, mov_q, ref_q, None, 1)
            made += [feats, other]
            zone, other_zone = W.DeviceFeatureZone(feats, None, None, C.EDGES), W.DeviceFeatureZone(other, None, None, C.EDGES)
            made += [zone, other_zone]
            rc, out, dist = call(m.acc.handle, dmov, dref, feats, zone)
            assert rc == 0 and np.array_equal(out, want) and C.same_bits(dist, want_d2)
            refused = [("other sections' features", (dmov, dref, other, None)), ("another moving section", (dmov2, dref, feats, None)),
                       ("another reference section", (dmov, dref2, feats, None)), ("a zone of other features", (dmov, dref, feats, other_zone)),
                       ("no features", (dmov, dref, None, None))]
            for name, args in refused:
                rc, out, dist = call(m.acc.handle, *args)
                assert rc == _lib.SAME_EINVAL and (out == -7).all() and (dist == -7.0).all(), name
            for short in (words - 1, 0, W.score_feature_words(1, 5)):                  # (enough without the zone, not with it)
                rc, out, dist = call(m.acc.handle, dmov, dref, feats, zone, n_words=short)
                assert rc == _lib.SAME_EINVAL and (out == -7).all() and (dist == -7.0).all(), short
            assert call(None, dmov, dref, feats, zone)[0] == _lib.SAME_EINVAL
            with lock:
                assert lib.same_merge_acc_score_features(m.acc.handle, dmov.handle, dref.handle, feats.handle, None, None, words, None) == _lib.SAME_EINVAL
            # sections of half the rows: final rows name rows outside them -- with a zone and without
            for xy_m, xy_r, name in ((half_m, n_ref, "half the moving rows"), (n_mov, half_r, "half the reference rows")):
                short_m = types.SimpleNamespace(ctx=m.ctx, job=types.SimpleNamespace(mov_xy=m.job.mov_xy[:xy_m], ref_xy=m.job.ref_xy[:xy_r]))
                with _sections(short_m) as (dm, dr, _x):
                    f = W.DeviceScoreFeatures(dm, dr, mov_q[:xy_m], ref_q[:xy_r], None, 1)
                    z = W.DeviceFeatureZone(f, None, None, C.EDGES)
                    try:
                        for with_zone in (z, None):
                            rc, out, dist = call(m.acc.handle, dm, dr, f, with_zone)
                            assert rc == _lib.SAME_ERANGE and (out == -7).all() and (dist == -7.0).all(), (name, with_zone is not None)
                    finally:
                        z.close()
                        f.close()
                # ... and the next call reads as ever
                rc, out, dist = call(m.acc.handle, dmov, dref, feats, zone)
                assert rc == 0 and np.array_equal(out, want) and C.same_bits(dist, want_d2), name
            # what same_merge_acc_score refuses: an accumulator before its finish, after plain, after load -- with a zone and without
            fresh = W.MergeAccumulator(m.ctx)
            try:
                def refused_by(acc, state):
                    for with_zone in (zone, None):
                        s0 = m.ctx.stats()
                        rc, out, dist = call(acc.handle, dmov, dref, feats, with_zone)
                        assert rc == _lib.SAME_EINVAL and (out == -7).all() and (dist == -7.0).all(), (state, with_zone is not None)
                        assert _spent(m.ctx, s0) == (0, 0, 0, 0), state          # refused before any device call

                refused_by(fresh, "made")
                fresh.begin(16)
                refused_by(fresh, "begun")
                W.plain_accumulators([fresh])
                refused_by(fresh, "plain")
                z4 = np.zeros(4, np.int32)
                fresh.load(np.arange(4), np.arange(4), np.zeros(4, np.uint8), z4, z4, z4, 4, 4)
                refused_by(fresh, "loaded")
                _counts, rest = W.resolve_accumulators([fresh], None, None)
                refused_by(fresh, "loaded and resolved")
                fresh.finish(rest["row"])
                assert fresh.n_final == 4
                refused_by(fresh, "loaded and finished")
            finally:
                fresh.close()
            # ... a section without label codes, on either side
            for side in (0, 1):
                xy = (m.job.mov_xy, m.job.ref_xy)[side]
                bare = W.DeviceSection(W.Section(np.ascontiguousarray(xy), np.zeros((len(xy), 1))), np.float64, m.ctx)
                try:
                    bf = W.DeviceScoreFeatures(bare if side == 0 else dmov, dref if side == 0 else bare, mov_q, ref_q, None, 1)
                    bz = W.DeviceFeatureZone(bf, None, None, C.EDGES)
                    try:
                        for with_zone in (bz, None):
                            rc, out, dist = call(m.acc.handle, bare if side == 0 else dmov, dref if side == 0 else bare, bf, with_zone)
                            assert rc == _lib.SAME_EINVAL and (out == -7).all() and (dist == -7.0).all(), (side, with_zone is not None)
                    finally:
                        bz.close()
                        bf.close()
                finally:
                    bare.close()
            # ... and after all of them one good call
            rc, out, dist = call(m.acc.handle, dmov, dref, feats, zone)
            assert rc == 0 and np.array_equal(out, want) and C.same_bits(dist, want_d2)
            rc, out, dist = call(m.acc.handle, dmov, dref, feats, None)
            want_plain = C.host_features(m.job.a_row, m.job.r_row, n_mov, mov_q, ref_q, None, 1)[0]
            assert rc == 0 and np.array_equal(out[:len(want_plain)], want_plain) and (out[len(want_plain):] == -7).all() and np.isnan(dist).all()
        finally:
            for h in reversed(made):
                h.close()
