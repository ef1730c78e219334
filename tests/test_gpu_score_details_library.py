"""same_merge_acc_score_detail (csrc/window_score_detail.hip) driven at the library against tests/score_details_check.py's
`host_detail_counts` -- plain numpy from include/same_hip.h's statement of the words, nothing of libsame_hip in it -- on the two merged
accumulators tests/test_gpu_score_library.py builds (`tiny`: one window, fewer than 64 rows; `large`: more than 512 rows, not a multiple
of 64) and on sections the tests make themselves.  Every assertion is exact equality of the int64 words.

The families (score_details_check.py; tests/test_score_details_cpu.py checks each has its property): label counts 1 and at the cap, label
codes negative and beyond L, group counts 1 and at the cap, no row in a group, one group holding all, groups of one row, group_of NULL,
triangle counts at the wave and block edges and 0, 1 / 2 / 17 type columns, NaN / infinite / tied type rows, no label naming a column;
then score and detail calls interleaved on one accumulator, a moving section larger than any scored before, the stated runtime-call
counts and the refusals."""
import contextlib
import ctypes

import numpy as np
import pytest

import score_check as S
import score_details_check as D
from test_gpu_score_library import ONE_WINDOW, _merged, _spent, _synthetic, large, tiny  # noqa: F401 (large, tiny: fixtures)

pytestmark = pytest.mark.gpu

RULES = [(False, 0.5, 1), (True, 0.5, 1), (True, 1.0 / 3.0, 2)]


@contextlib.contextmanager
def _resident(m, d, detail=True):
    """the Detail's inputs as sections of their own on the accumulator's context -- type matrices of the Detail's width, label codes
    set --, the triangles as a DeviceCallerTris (None: none) and the DeviceScoreDetail"""
    from same_amd import windows as W

    made = []
    try:
        inp = d.inp
        for xy, code, types in ((inp.mov_xy, inp.code_m, d.mov_types), (inp.ref_xy, inp.code_r, d.ref_types)):
            made.append(W.DeviceSection(W.Section(xy, np.ascontiguousarray(types, np.float64)), np.float64, m.ctx))
            made[-1].set_label_codes(np.ascontiguousarray(code, np.int32))
        tris = None
        if inp.tris is not None:
            made.append(W.DeviceCallerTris(made[0], inp.tris, m.ctx))
            tris = made[-1]
        det = None
        if detail:
            made.append(W.DeviceScoreDetail(made[0], d.group_of, d.n_groups, d.n_labels, d.col_of_label))
            det = made[-1]
        yield made[0], made[1], tris, det
    finally:
        for h in reversed(made):                  # the triangulation and the detail before their section
            h.close()


def _flat(split):
    return np.concatenate((split["confusion"].reshape(-1), [split["unlabelled"]], split["groups"].reshape(-1), split["strict"], split["weak"],
                           [split["untyped"]]))


def _check(m, name, d, rules=RULES):
    with _resident(m, d) as (dmov, dref, tris, det):
        for ignore_same in (True, False):
            for rule in (rules if ignore_same else rules[:1]):
                got = _flat(m.acc.score_detail(dmov, dref, tris, det, ignore_same, *rule))
                want = D.host_detail_counts(m.job.a_row, m.job.r_row, d, ignore_same, *rule)
                assert got.dtype == np.int64 and got.tolist() == want.tolist(), (name, ignore_same, rule, np.flatnonzero(got != want)[:20].tolist())
    return got


# ---- 1. the families ---------------------------------------------------------------------------------------------------------------------
N_LARGE = 1 + 2 + 2 + 6 + len(D.TRI_COUNTS) + len(D.TYPE_COLUMNS) + 4 + 2 + 1


@pytest.mark.parametrize("which", range(N_LARGE))
def test_every_family_on_the_large_accumulator(large, which):   # noqa: F811
    if not hasattr(large, "detail_families"):
        large.detail_families = D.all_families(large.job)
    assert len(large.detail_families) == N_LARGE
    name, d = large.detail_families[which]
    got = _check(large, name, d)
    print(name, "L", d.n_labels, "G", d.n_groups, "words", len(got), "non-zero", int(np.count_nonzero(got)))


def test_every_family_on_the_tiny_accumulator(tiny):   # noqa: F811
    for name, d in D.small_families(tiny.job):
        got = _check(tiny, name, d, RULES[:2])
        print("tiny", name, "non-zero words", int(np.count_nonzero(got)))


# ---- 2. create's checks ------------------------------------------------------------------------------------------------------------------
def test_counts_beyond_the_caps_and_values_out_of_range_are_refused_on_the_host(tiny):   # noqa: F811
    from same_amd import _lib
    from same_amd import windows as W

    d = D.plain(tiny.job)
    n = len(d.inp.mov_xy)
    with _resident(tiny, d, detail=False) as (dmov, _dref, _tris, _det):
        lib, ctx = tiny.ctx.lib, tiny.ctx
        group, col = np.zeros(n, np.int32), np.zeros(D.MAX_LABELS + 1, np.int32)

        def create(group_of, n_groups, n_labels, col_of):
            h = ctypes.c_void_p()
            with ctx.lock:
                s0 = ctx.stats()
                rc = lib.same_score_detail_create(dmov.handle, None if group_of is None else group_of.ctypes.data, n_groups, n_labels,
                                                  None if col_of is None else col_of.ctypes.data, ctypes.byref(h))
                assert _spent(ctx, s0) == (0, 0, 0, 0)
                if h.value:
                    lib.same_score_detail_destroy(h)
            return rc, bool(h.value)

        for args in ((group, 1, D.MAX_LABELS + 1, col), (group, D.MAX_GROUPS + 1, 3, col), (group, 0, 3, col), (group, 1, -1, col),
                     (None, -2, 3, None)):
            assert create(*args) == (_lib.SAME_EINVAL, False), args[1:3]
        T = d.mov_types.shape[1]
        for bad_group in (np.where(np.arange(n) == n - 1, 4, 0).astype(np.int32), np.full(n, 2**31 - 1, np.int32)):
            assert create(bad_group, 4, 3, col) == (_lib.SAME_ERANGE, False)
        for bad_col in (np.array([0, T, 1], np.int32), np.array([0, -2, 1], np.int32)):
            assert create(group, 1, 3, bad_col) == (_lib.SAME_ERANGE, False)
        assert create(np.full(n, -(2**31), np.int32), D.MAX_GROUPS, D.MAX_LABELS, np.full(D.MAX_LABELS, T - 1, np.int32)) == (0, True)
        assert create(None, 1, 0, None) == (0, True)
        with pytest.raises(ValueError):
            W.DeviceScoreDetail(dmov, group[:-1], 1, 3, None)
        with pytest.raises(ValueError):
            W.DeviceScoreDetail(dmov, None, 1, 3, col[:2])


# ---- 3. interleaving, the work buffers' life, the call budget -----------------------------------------------------------------------------
def test_score_and_detail_calls_alternate_on_one_accumulator_within_the_stated_calls():
    """a fresh accumulator: detail, score, detail, detail without triangles, score, detail at the groups' cap (more words: the bins are
    laid again, one fill), detail over a moving section 5000 rows larger (the score work buffer is laid again, two fills), score over the
    own section again, detail -- each equal to its host statement, which is its stand-alone result; (launches, fills, copies, waits) as
    include/same_hip.h states: (3, ., 1, 1) with triangles, (1, ., 1, 1) without"""
    with _merged(*_synthetic(200, 7), ONE_WINDOW) as m:
        job = m.job
        base = D.plain(job)
        bare = base._replace(inp=base.inp._replace(tris=None))
        wide = dict(D.group_families(job))["G at the cap"]
        big = D.grown(job)
        steps = [("detail", base, 3), ("score", base, 0), ("detail", base, 0), ("detail", bare, 0), ("score", base, 0), ("detail", wide, 1),
                 ("detail", base, 0), ("detail", big, 2), ("score", base, 0), ("detail", base, 0), ("score", big, 0), ("detail", wide, 0)]
        with contextlib.ExitStack() as stack:
            resident = {id(d): stack.enter_context(_resident(m, d)) for d in (base, bare, wide, big)}
            for step, (what, d, fills) in enumerate(steps):
                dmov, dref, tris, det = resident[id(d)]
                for rule in RULES[:2]:
                    s0 = m.ctx.stats()
                    if what == "score":
                        got = m.acc.score(dmov, dref, tris, True, *rule)
                        inp = d.inp
                        want = S.host_counts(job.a_row, job.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.code_r, inp.tris, True, *rule)[0]
                    else:
                        got = _flat(m.acc.score_detail(dmov, dref, tris, det, True, *rule))
                        want = D.host_detail_counts(job.a_row, job.r_row, d, True, *rule)
                    spent = _spent(m.ctx, s0)
                    print(step, what, d.n_groups, spent)
                    assert got.tolist() == want.tolist(), (step, what, rule)
                    with_tris = d.inp.tris is not None and len(d.inp.tris) > 0
                    assert spent == (3 if with_tris else 1, fills if rule == RULES[0] else 0, 1, 1), (step, what, rule, spent)


def test_no_rows_and_no_triangles_ask_nothing_of_the_runtime(tiny):   # noqa: F811
    """an empty triangulation is one launch; out_words one short is SAME_EINVAL before anything runs, out untouched"""
    from same_amd import _lib

    d = D.plain(tiny.job)
    d = d._replace(inp=d.inp._replace(tris=np.zeros((0, 3), np.int32)))
    with _resident(tiny, d) as (dmov, dref, tris, det):
        s0 = tiny.ctx.stats()
        got = _flat(tiny.acc.score_detail(dmov, dref, tris, det))
        assert _spent(tiny.ctx, s0)[0] == 1 and got.tolist() == D.host_detail_counts(tiny.job.a_row, tiny.job.r_row, d).tolist()
        out = np.full(det.n_words, -7, np.int64)
        with tiny.ctx.lock:
            s0 = tiny.ctx.stats()
            rc = tiny.ctx.lib.same_merge_acc_score_detail(tiny.acc.handle, dmov.handle, dref.handle, tris.handle, det.handle, 1, 0, 0.5, 1,
                                                          out.ctypes.data, det.n_words - 1)
        assert rc == _lib.SAME_EINVAL and (out == -7).all() and _spent(tiny.ctx, s0) == (0, 0, 0, 0)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_out_and_the_accumulator_as_they_were(large):   # noqa: F811
    """same_merge_acc_score's list -- sections of half the rows (SAME_ERANGE), a triangulation made for another section, no detail, a
    NaN threshold, an accumulator before its finish (SAME_EINVAL) -- and a detail made for another section; `out` untouched, and the
    next score and detail calls count as ever"""
    from same_amd import _lib
    from same_amd import windows as W

    job = large.job
    base = D.plain(job)
    half_m, half_r = len(base.inp.mov_xy) // 2, len(base.inp.ref_xy) // 2
    assert job.a_row.max() >= half_m and job.r_row.max() >= half_r
    small_tris = base.inp.tris[(base.inp.tris < half_m).all(axis=1)]
    short_mov = base._replace(inp=S.Inputs(base.inp.mov_xy[:half_m], base.inp.ref_xy, base.inp.code_m[:half_m], base.inp.code_r, small_tris),
                              group_of=base.group_of[:half_m], mov_types=base.mov_types[:half_m])
    short_ref = base._replace(inp=base.inp._replace(ref_xy=base.inp.ref_xy[:half_r], code_r=base.inp.code_r[:half_r]),
                              ref_types=base.ref_types[:half_r])
    want = D.host_detail_counts(job.a_row, job.r_row, base)
    lib, ctx = large.ctx.lib, large.ctx

    def call(acc, dm, dr, tr, det, threshold=0.5):
        out = np.full(D.out_words(base.n_labels, base.n_groups), -7, np.int64)
        with ctx.lock:
            rc = lib.same_merge_acc_score_detail(acc.handle, dm.handle, dr.handle, None if tr is None else tr.handle,
                                                 None if det is None else det.handle, 1, 0, threshold, 1, out.ctypes.data, len(out))
        return rc, out.tolist()

    untouched = [-7] * D.out_words(base.n_labels, base.n_groups)
    with _resident(large, base) as (dmov, dref, tris, det):
        assert _flat(large.acc.score_detail(dmov, dref, tris, det)).tolist() == want.tolist()
        for name, d in (("half the moving rows", short_mov), ("half the reference rows", short_ref),
                        ("half the moving rows, no triangles", short_mov._replace(inp=short_mov.inp._replace(tris=None)))):
            with _resident(large, d) as (dm, dr, tr, dt):
                assert call(large.acc, dm, dr, tr, dt) == (_lib.SAME_ERANGE, untouched), name
                # made for another section: the detail, the triangulation
                assert call(large.acc, dmov, dref, tris, dt) == (_lib.SAME_EINVAL, untouched), name
                if tr is not None:
                    assert call(large.acc, dmov, dref, tr, det) == (_lib.SAME_EINVAL, untouched), name
            assert _flat(large.acc.score_detail(dmov, dref, tris, det)).tolist() == want.tolist(), name
            got = large.acc.score(dmov, dref, tris)
            inp = base.inp
            assert got.tolist() == S.host_counts(job.a_row, job.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.code_r, inp.tris)[0].tolist()
        assert call(large.acc, dmov, dref, tris, None) == (_lib.SAME_EINVAL, untouched)
        assert call(large.acc, dmov, dref, tris, det, float("nan")) == (_lib.SAME_EINVAL, untouched)
        fresh = W.MergeAccumulator(ctx)
        try:
            assert call(fresh, dmov, dref, tris, det) == (_lib.SAME_EINVAL, untouched)
        finally:
            fresh.close()
        # sections without label codes
        bare = W.DeviceSection(W.Section(base.inp.mov_xy, np.ascontiguousarray(base.mov_types)), np.float64, ctx)
        try:
            assert call(large.acc, bare, dref, None, det) == (_lib.SAME_EINVAL, untouched)
        finally:
            bare.close()
        assert _flat(large.acc.score_detail(dmov, dref, tris, det)).tolist() == want.tolist()
