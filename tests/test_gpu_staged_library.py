"""same_collapse_candidates, same_greedy_disjoint (csrc/match.hip), same_window_count (csrc/sweep.hip) and same_eager_signs (csrc/tri.hip)
driven through same_amd.ops against tests/staged_check.py's statements -- plain numpy float64 and Python from the reference's text, nothing
of libsame_hip in them -- on inputs the product routes never make.  Every input is exact before its single sqrt or division (integer
coordinates up to 2**20; cross products that are one coordinate), so every comparison is equality in every bit: flags, perimeters, totals,
selections, round counts, masks, counts and signs; NaN equals NaN in the values.  No tolerance anywhere.

The families (staged_check.py; tests/test_staged_check_cpu.py checks each has its property and that planted wrong kernels are caught on
them).  On the library as it was before this module, three of these tests failed on an MI355X, as read from the code beforehand, and no
other: the non-finite corners (the r_max rule took its maximum pairwise, which drops a leading NaN edge and lets a later one through, where
the reference's Python max does the opposite: 20 of 60 flags) and the two zeros under same_greedy_disjoint and under same_greedy_match,
which shares the key (it put -0.0 before +0.0, where the reference's sort finds them equal and keeps list order)."""
import ctypes

import numpy as np
import pytest

import staged_check as S

pytestmark = pytest.mark.gpu
SAME_OK = 0                                                         # include/same_hip.h


@pytest.fixture(scope="module")
def ctx():
    from same_amd import _lib

    return _lib.default_context(0)


def _bits(got, want, what):
    """equal in dtype, shape and every bit (NaN equal to NaN in float values), with the first places that differ in the message"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == "f"):
        g, w = got.reshape(-1), want.reshape(-1)
        where = np.flatnonzero(~((g == w) | ((g != g) & (w != w))))
        raise AssertionError((what, f"{len(where)} of {len(g)} differ", [(int(i), g[i].item(), w[i].item()) for i in where[:8]]))


def _family(families, name):
    return dict(families)[name]


# ---- same_collapse_candidates -----------------------------------------------------------------------------------------------------------------
def _collapse(case, ctx):
    from same_amd import ops
    from same_amd.triangles import cos_threshold

    enabled, thr = cos_threshold(case.min_angle_deg)                # as metacell_utils obtains the kernel's threshold
    return ops.collapse_candidates(case.xy, case.tris, case.r_max, enabled, thr, case.type_id, case.size, case.max_size, ctx=ctx)


COLLAPSE = S.collapse_families()


@pytest.mark.parametrize("family", [name for name, _cases in COLLAPSE])
def test_collapse_candidates_equal_the_statement(ctx, family):
    for name, case in _family(COLLAPSE, family):
        flag, perim, total = _collapse(case, ctx)
        want_flag, want_perim, want_total = S.host_collapse(case)
        print(family, name, len(case.tris), "triangles:", int((flag & 1).sum()), "valid,", int((flag >> 1).sum()), "candidates")
        _bits(flag, want_flag, (family, name, "flag"))
        _bits(perim, want_perim, (family, name, "perimeter"))
        _bits(total, want_total, (family, name, "total"))


def test_collapse_candidates_index_edges(ctx):
    """Tr = 0 (with points, and with n = 0) returns without touching the outputs; a vertex out of range on either side is SAME_ERANGE with
    the outputs untouched, and the next call is exact"""
    from same_amd import _lib

    case = S.collapse_sizes()[2][1]
    n, Tr = len(case.xy), len(case.tris)
    xy, type_id, size = np.ascontiguousarray(case.xy), np.ascontiguousarray(case.type_id, np.int32), np.ascontiguousarray(case.size)
    flag, perim, total = np.full(Tr, 0xA5, np.uint8), np.full(Tr, -7.0), np.full(Tr, -7.0)

    def call(n_points, tris):
        tris = np.ascontiguousarray(tris, np.int32)
        with ctx.lock:
            return ctx.lib.same_collapse_candidates(ctx.handle, xy.ctypes.data, n_points, tris.ctypes.data, len(tris), 1, 700.0, 1, 0.9,
                                                    type_id.ctypes.data, size.ctypes.data, 4.0, flag.ctypes.data, perim.ctypes.data,
                                                    total.ctypes.data)

    untouched = lambda: (flag == 0xA5).all() and (perim == -7.0).all() and (total == -7.0).all()
    assert call(n, np.zeros((0, 3))) == SAME_OK and untouched()
    assert call(0, np.zeros((0, 3))) == SAME_OK and untouched()
    for bad in (n, -1, 2**31 - 1, -2**31):
        tris = case.tris.copy()
        tris[Tr - 1, 1] = bad
        assert call(n, tris) == _lib.SAME_ERANGE and untouched(), bad
    assert call(n - 1, case.tris) == _lib.SAME_ERANGE and untouched()                  # the last point is named by the last triangle
    got = _collapse(case, ctx)
    for g, w, what in zip(got, S.host_collapse(case), ("flag", "perimeter", "total")):
        _bits(g, w, ("after the refused calls", what))


# ---- same_greedy_disjoint ---------------------------------------------------------------------------------------------------------------------
DISJOINT = S.disjoint_families()


@pytest.mark.parametrize("family", [name for name, _cases in DISJOINT])
def test_greedy_disjoint_equals_the_sequential_scan(ctx, family):
    """the selection equals the reference's sort and scan; the rounds equal those of the local-minimum rule the header states"""
    from same_amd import ops

    for name, case in _family(DISJOINT, family):
        selected, rounds = ops.greedy_disjoint(case.items, case.keys, case.n_nodes, ctx=ctx)
        _also, want_rounds = S.local_minimum_rounds(case)
        print(family, name, len(case.items), "items:", int(selected.sum()), "selected in", rounds, "rounds")
        _bits(selected, S.host_disjoint(case), (family, name, "selected"))
        assert rounds == want_rounds, (family, name, rounds, want_rounds)
        if family == "chain":
            assert rounds == S.CHAIN // 2
        if family in ("star", "disjoint_items"):
            assert rounds == 1 and selected.sum() == (1 if family == "star" else len(case.items))


def test_greedy_disjoint_with_no_items(ctx):
    from same_amd import _lib, ops

    selected, rounds = ops.greedy_disjoint(np.zeros((0, 3), np.int32), np.zeros(0), 10, ctx=ctx)
    assert selected.shape == (0,) and rounds == 0
    rounds = ctypes.c_int(-7)
    with ctx.lock:
        assert ctx.lib.same_greedy_disjoint(ctx.handle, None, None, 0, 0, None, ctypes.byref(rounds)) == SAME_OK and rounds.value == 0
    items, keys, out = np.array([(0, 1, 2), (2, 3, 10)], np.int32), np.zeros(2), np.full(2, 0xA5, np.uint8)
    with ctx.lock:                                                  # a vertex that is n_nodes: refused, nothing written
        rc = ctx.lib.same_greedy_disjoint(ctx.handle, items.ctypes.data, keys.ctypes.data, 2, 10, out.ctypes.data, ctypes.byref(rounds))
    assert rc == _lib.SAME_ERANGE and (out == 0xA5).all()


def test_greedy_match_finds_the_two_zeros_equal(ctx):
    """same_greedy_match shares the kernels' key: rows that all want column 0 at costs +0.0, -0.0, +0.0, -0.0 -- the reference's stable sort
    (src/init_helpers.py:111-112) keeps list order among them, so the first pair wins; and a random problem whose costs are one zero or the
    other, against the sequential scan"""
    from same_amd import ops

    rng = np.random.default_rng(38)
    star = (np.column_stack((np.arange(4), np.zeros(4))).astype(np.int32), np.array([0.0, -0.0, 0.0, -0.0]), 4, 1)
    edges = np.unique(rng.integers(0, 40, (600, 2)), axis=0).astype(np.int32)
    edges = edges[rng.permutation(len(edges))]
    for name, (pairs, costs, n_m, n_r) in (("star", star), ("random", (edges, np.where(rng.random(len(edges)) < 0.5, 0.0, -0.0), 40, 40))):
        match, _rounds = ops.greedy_match(pairs, costs, n_m, n_r, np.ones(n_m, np.uint8), ctx=ctx)
        want, used = np.full(n_m, -1, np.int32), set()
        for p in sorted(range(len(pairs)), key=costs.tolist().__getitem__):
            i, j = int(pairs[p, 0]), int(pairs[p, 1])
            if want[i] < 0 and j not in used:
                want[i] = p
                used.add(j)
        _bits(match, want, ("greedy_match", name))


# ---- same_window_count ------------------------------------------------------------------------------------------------------------------------
WINDOWS = S.window_families()


@pytest.mark.parametrize("family", [name for name, _cases in WINDOWS])
def test_window_counts_and_masks_equal_the_statement(ctx, family):
    """with and without the mask: the mask in layout [n_boxes][n], the counts its row sums both times"""
    from same_amd import ops

    for name, case in _family(WINDOWS, family):
        want = S.host_window_mask(case)
        counts = ops.window_count(case.xy, case.boxes, ctx=ctx)
        counts_too, mask = ops.window_count(case.xy, case.boxes, want_mask=True, ctx=ctx)
        _bits(mask, want, (family, name, "mask"))
        _bits(counts, want.sum(axis=1).astype(np.int64), (family, name, "counts"))
        _bits(counts_too, counts, (family, name, "counts beside the mask"))
    print(family, len(_family(WINDOWS, family)), "cases")


def test_window_count_empty_inputs_and_the_oracle(ctx, oracle):
    from same_amd import _lib, ops

    case = S.window_sizes()[-2][1]                                  # 1000 points, 5 boxes
    counts = ops.window_count(np.zeros((0, 2)), case.boxes, ctx=ctx)
    assert counts.dtype == np.int64 and counts.tolist() == [0] * len(case.boxes)
    out = np.full(3, -7, np.int64)
    xy = np.ascontiguousarray(case.xy)
    with ctx.lock:
        assert ctx.lib.same_window_count(ctx.handle, xy.ctypes.data, len(xy), None, 0, out.ctypes.data, None) == SAME_OK
    assert out.tolist() == [-7] * 3                                 # no boxes: returns, nothing written
    counts, mask = ops.window_count(case.xy, case.boxes, want_mask=True, ctx=ctx)
    for b, box in enumerate(case.boxes):
        want = oracle.window_mask(case.xy, *box)
        assert np.array_equal(mask[b], want) and counts[b] == want.sum(), b


# ---- same_eager_signs -------------------------------------------------------------------------------------------------------------------------
EAGER = S.eager_families()


@pytest.mark.parametrize("family", [name for name, _cases in EAGER])
def test_eager_signs_equal_the_statement(ctx, family):
    from same_amd import ops

    for name, case in _family(EAGER, family):
        got = ops.eager_signs(case.rxy, case.tris, case.cand, ctx=ctx)
        want = S.host_eager_signs(case)                             # the expected signs come from the statement, none is written here
        print(family, name, got.size, "signs:", {int(v): int((got == v).sum()) for v in np.unique(got)})
        _bits(got, want, (family, name))
        if family == "vertex_orders":
            assert got.reshape(-1)[:6].tolist() == [S.order_parity(o) for o in S.ORDERS]


def test_eager_signs_refuses_bad_k_and_candidates(ctx):
    """k = 0, k > SAME_MAX_KNN, a candidate that is n_r (or below -1), a triangle row that is n_m: an error code and the output untouched"""
    from same_amd import _lib, ops

    case = S.missing_candidates()[0][1]
    rxy, tris, cand = np.ascontiguousarray(case.rxy), np.ascontiguousarray(case.tris, np.int32), np.ascontiguousarray(case.cand, np.int32)
    out = np.full(len(tris) * 27, 0x5A, np.int8)

    def call(tris, cand, k, n_r=len(rxy)):
        with ctx.lock:
            return ctx.lib.same_eager_signs(ctx.handle, rxy.ctypes.data, n_r, tris.ctypes.data, len(tris), cand.ctypes.data, len(case.cand), k,
                                            out.ctypes.data)

    assert call(tris, cand, 0) == _lib.SAME_EINVAL and (out == 0x5A).all()
    assert call(tris, cand, -1) == _lib.SAME_EINVAL and (out == 0x5A).all()
    assert call(tris, cand, _lib.MAX_KNN + 1) == _lib.SAME_EINVAL and (out == 0x5A).all()
    for bad in (len(rxy), -2, 2**31 - 1):
        wrong = cand.copy()
        wrong[4, 2] = bad
        assert call(tris, wrong, 3) == _lib.SAME_ERANGE and (out == 0x5A).all(), bad
    assert call(tris, cand, 3, n_r=len(rxy) - 1) == _lib.SAME_ERANGE and (out == 0x5A).all()   # the last reference row is a candidate
    wrong = tris.copy()
    wrong[7, 0] = len(case.cand)
    assert call(wrong, cand, 3) == _lib.SAME_ERANGE and (out == 0x5A).all()
    _bits(ops.eager_signs(case.rxy, case.tris, case.cand, ctx=ctx), S.host_eager_signs(case), "after the refused calls")
