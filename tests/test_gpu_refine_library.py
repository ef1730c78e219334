"""same_refine_matching and same_refine_matching_cap (csrc/refine.hip) driven at the LIBRARY on hostile windows and triangle lists, and the
batched form of the same kernels inside same_window_filter_finish[_cap], against the host statement of the round rule
(tests/refine_check.py, tests/refine_capacity_check.py) -- a fan whose search runs one move a round past every edge of the host form's
round chunks, with round caps on and beside those edges; references contested by deltas that differ in fp64 and are equal as floats;
deltas that are f32 subnormals and deltas beyond float's range; duplicate, collinear and twice-cornered triangles, shuffled rows and
corners, a list five times the cells, none; pairs in any order; cell and slot counts on the block edges, more references than cells and
the empty calls; fractional sizes, signed costs, capacities filled to the limit.  The matching, rounds, moves, settled and the extra
matches are equal, the objectives bit for bit wherever every sum is exact.  The inputs come from tests/refine_hostile_check.py;
tests/test_refine_hostile_check_cpu.py proves without a GPU that each has the property its case is about, and that a kernel wrong in one
of eight ways would give another answer."""
import numpy as np
import pytest

import finish_check as F
import refine_capacity_check as rcc
import refine_check as rc
import refine_hostile_check as H

pytestmark = pytest.mark.gpu

FIRST_ROUNDS = 4            # csrc/refine.h


def _args(kw):
    return (kw["pairs"], kw["costs"], kw["unmatched"], kw["n"], kw["n_r"], kw["triangles"], kw["axy"], kw["ref_xy"], kw["size"],
            kw["delaunay_penalty"])


def _device(kw, start, cap, ctx=None):
    from same_amd import ops

    if H.is_cap(kw):
        return ops.refine_matching_cap(*_args(kw), kw["limit"], kw["penalty_coeff"], cap, start, ctx=ctx)
    return ops.refine_matching(*_args(kw), cap, start, ctx=ctx)


def _bits(x):
    return np.float64(x).view(np.int64)


def _is(got, want, name, exact):
    """the device's (matching, stats) is the statement's: objectives bit for bit where every sum is exact, else at the suite's rel=1e-12
    (the device reduces in a fixed tree, the statement sums in sequence)"""
    (m, st), (wm, wst) = got, want
    print(name, {k: v for k, v in st.items()}, "statement", {k: v for k, v in wst.items() if k != "trace"})
    assert m.dtype == np.int32 and np.array_equal(m, wm), name
    keys = ("rounds", "moves", "settled") + (("ref_extra_matches",) if "ref_extra_matches" in wst else ())
    assert set(st) == set(keys) | {"objective_start", "objective"}, name
    assert tuple(st[k] for k in keys) == tuple(wst[k] for k in keys), name
    for k in ("objective_start", "objective"):
        if exact:
            assert _bits(st[k]) == _bits(wst[k]), (name, k, st[k], wst[k])
        else:
            assert st[k] == pytest.approx(wst[k], rel=1e-12), (name, k)


def _same_bits(a, b):
    """two device answers are one: the matching and every stats word, the objectives as bits"""
    assert np.array_equal(a[0], b[0]) and set(a[1]) == set(b[1])
    assert all(_bits(a[1][k]) == _bits(b[1][k]) if isinstance(a[1][k], float) else a[1][k] == b[1][k] for k in a[1]), (a[1], b[1])


def _nothing(got, extra):
    """a call without cells launches nothing: an empty matching, every stats word 0 (settled too) and both objectives 0.0"""
    m, st = got
    assert m.dtype == np.int32 and len(m) == 0
    assert st == dict(rounds=0, moves=0, settled=0, objective_start=0.0, objective=0.0, **({"ref_extra_matches": 0} if extra else {}))
    assert _bits(st["objective_start"]) == 0 and _bits(st["objective"]) == 0


@pytest.mark.parametrize("name", H.NAMES)
def test_host_form_is_the_statement(name):
    """Every family of tests/refine_hostile_check.NAMES through the entry point its kwargs ask for, twice.  The plain families again
    through the _cap entry point with every limit 1, at penalty_coeff 0 and 100: the plain call bit for bit."""
    kw, start, cap = H.case(name)
    want = H.statement(name)
    got = _device(kw, start, cap)
    if kw["n"] == 0:
        _nothing(got, H.is_cap(kw))
    else:
        _is(got, want, name, name in H.DYADIC)
    _same_bits(_device(kw, start, cap), got)
    if not H.is_cap(kw):
        for pc in (0.0, 100.0):
            m, st = _device(dict(kw, limit=np.ones(kw["n_r"], np.int32), penalty_coeff=pc), start, cap)
            assert st.pop("ref_extra_matches") == 0
            _same_bits((m, st), got)


def test_one_context_large_small_large():
    """513 cells, then 3 cells in the buffers the 513 sized, then the 513 again, on ONE context of their own: each its own statement's,
    the third call's answer the first's"""
    from same_amd import _lib

    ctx = _lib.Context()
    try:
        big, small = "size/n=513", "empty/3-3-3-1"
        first = _device(*H.case(big), ctx=ctx)
        _is(first, H.statement(big), big, True)
        _is(_device(*H.case(small), ctx=ctx), H.statement(small), small, True)
        third = _device(*H.case(big), ctx=ctx)
        _same_bits(third, first)
        cap_big = "size/n=600,n_r=3"
        _is(_device(*H.case(cap_big), ctx=ctx), H.statement(cap_big), cap_big, True)
        _nothing(_device(*H.case("empty/0-5-0-0"), ctx=ctx), False)
        _is(_device(*H.case(small), ctx=ctx), H.statement(small), small, True)
    finally:
        ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, kw, start, cap):
    """the library call itself, as same_amd.ops makes it -> (return code, the match_pair buffer after the call)"""
    from same_amd import ops

    pairs, costs, unm = ops.as_c(kw["pairs"], np.int32).reshape(-1, 2), ops.as_c(kw["costs"], np.float64), ops.as_c(kw["unmatched"], np.float64)
    tris, axy, rxy = ops._tris(kw["triangles"]), ops.as_c(kw["axy"], np.float64), ops.as_c(kw["ref_xy"], np.float64)
    size = ops.as_c(kw["size"], np.float64)
    name, extra, words = "same_refine_matching", (), 5
    if H.is_cap(kw):
        limit = ops.as_c(kw["limit"], np.int32)
        name, extra, words = "same_refine_matching_cap", (limit.ctypes.data, float(kw["penalty_coeff"])), 6
    out = np.array(start, dtype=np.int32, copy=True)
    st = np.full(words, -7, np.int64)
    with ctx.lock:
        code = getattr(ctx.lib, name)(ctx.handle, pairs.ctypes.data, costs.ctypes.data, len(pairs), unm.ctypes.data, kw["n"], kw["n_r"],
                                      tris.ctypes.data, len(tris), axy.ctypes.data, rxy.ctypes.data, size.ctypes.data,
                                      float(kw["delaunay_penalty"]), *extra, int(cap), out.ctypes.data, st.ctypes.data)
    return code, out, st


def _refusals():
    """name -> (kwargs, start, rounds_cap, the code) : one thing wrong with a window the library otherwise accepts"""
    from same_amd import _lib

    kw, start, cap = H.case("size/n=200,n_r=57")
    kw, start = dict(kw), np.array(start)
    plain = {k: v for k, v in kw.items() if k not in ("limit", "penalty_coeff")}
    pairs, tris, n, n_r = np.array(kw["pairs"]), np.array(kw["triangles"]), kw["n"], kw["n_r"]
    EINVAL, ERANGE = _lib.SAME_EINVAL, _lib.SAME_ERANGE

    def edit(a, at, value):
        a = np.array(a)
        a[at] = value
        return a

    # two cells with a pair each to one reference, neither holding it at the start
    by_ref = {}
    for p, (i, j) in enumerate(pairs.tolist()):
        by_ref.setdefault(j, []).append((i, p))
    j2, ((ia, pa), (ib, pb), (ic, pc)) = next((j, v[:3]) for j, v in by_ref.items() if len(v) >= 3)
    twice = edit(edit(np.full(n, -1, np.int32), ia, pa), ib, pb)
    thrice = edit(twice, ic, pc)
    out = {}
    for tag, base in (("", plain), ("cap: ", kw)):
        out[tag + "a (row, column) pair twice"] = (dict(base, pairs=edit(pairs, 1, pairs[0])), start, cap, EINVAL)
        out[tag + "a pair's column = n_r"] = (dict(base, pairs=edit(pairs, (5, 1), n_r)), start, cap, EINVAL)
        out[tag + "a pair's row = -1"] = (dict(base, pairs=edit(pairs, (5, 0), -1)), start, cap, EINVAL)
        out[tag + "a pair's row = n"] = (dict(base, pairs=edit(pairs, (len(pairs) - 1, 0), n)), start, cap, EINVAL)
        out[tag + "a start pair on another cell's row"] = (base, edit(start, 0, int(np.flatnonzero(pairs[:, 0] == 1)[0])), cap, EINVAL)
        out[tag + "a start pair = P"] = (base, edit(start, 3, len(pairs)), cap, EINVAL)
        out[tag + "a start pair = -2"] = (base, edit(start, 3, -2), cap, EINVAL)
        out[tag + "a triangle index = n"] = (dict(base, triangles=edit(tris, (len(tris) - 1, 2), n)), start, cap, ERANGE)
        out[tag + "a triangle index = -1"] = (dict(base, triangles=edit(tris, (0, 0), -1)), start, cap, ERANGE)
        out[tag + "rounds_cap 0"] = (base, start, 0, EINVAL)
        for bad in (-1.0, float("nan"), float("inf")):
            out[tag + f"delaunay_penalty {bad}"] = (dict(base, delaunay_penalty=bad), start, cap, EINVAL)
    out["a start that holds a reference twice"] = (plain, twice, cap, EINVAL)
    out["cap: a start that holds a reference of limit 1 twice"] = (dict(kw, limit=edit(kw["limit"], j2, 1)), twice, cap, EINVAL)
    out["cap: a start that holds a reference of limit 2 three times"] = (dict(kw, limit=edit(kw["limit"], j2, 2)), thrice, cap, EINVAL)
    for bad in (-1.0, float("nan")):
        out[f"cap: penalty_coeff {bad}"] = (dict(kw, penalty_coeff=bad), start, cap, EINVAL)
    for bad in (0, rcc.MAX_LIMIT + 1):
        out[f"cap: a limit of {bad}"] = (dict(kw, limit=edit(kw["limit"], n_r - 1, bad)), start, cap, EINVAL)
    return out, (dict(kw, limit=edit(kw["limit"], j2, 3)), thrice, cap)


def test_refusals_leave_the_matching_and_the_context_as_they_were():
    """Every refusal comes back with its code before any device work (refine_host checks its arguments, the pair list, the start and the
    triangle indices before it touches the device), leaves match_pair as it was, and the next valid call on that context -- the 200-cell
    window, and a fan across a chunk edge -- gives its statement's answer.  The start that fills a reference to its limit of 3 exactly is
    accepted."""
    from same_amd import _lib

    refusals, (ok_kw, ok_start, ok_cap) = _refusals()
    assert len(refusals) == 2 * 13 + 7
    ctx = _lib.Context()
    try:
        after = ("size/n=200,n_r=57", "fan/40/cap=17")
        for q, (what, (kw, start, cap, code)) in enumerate(refusals.items()):
            got, out, st = _raw(ctx, kw, start, cap)
            assert got == code, (what, got, ctx.lib.same_last_error(ctx.handle).decode())
            assert np.array_equal(out, start) and np.all(st == -7), what
            name = after[q % 2]
            _is(_device(*H.case(name), ctx=ctx), H.statement(name), (what, "then", name), True)
        got, out, st = _raw(ctx, ok_kw, ok_start, ok_cap)
        assert got == 0
        wm, wst = H.run(ok_kw, ok_start, ok_cap)
        assert np.array_equal(out, wm) and tuple(st[:3]) == (wst["rounds"], wst["moves"], wst["settled"]) and st[5] == wst["ref_extra_matches"]
    finally:
        ctx.close()


# ---- the batched window form -------------------------------------------------------------------------------------------------------------
def _filter_args(filt, oracle):
    """the filter's arguments as the product passes them (the threshold is the oracle's)"""
    from same_amd.triangles import cos_threshold

    radius, angle, same = filt
    en, thr = cos_threshold(angle)
    assert (en, thr) == tuple(oracle.cos_threshold(angle))
    return (radius, en, thr, F.near_tol(angle, oracle)[2], same)


def _pair_index(pairs, match, n):
    pair_of = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs)}
    return np.array([pair_of[(i, int(match[i]))] if match[i] >= 0 else -1 for i in range(n)], np.int32)


@pytest.mark.parametrize("mode_name", list(H.BATCH_MODES))
def test_ten_windows_in_one_finish_call(oracle, mode_name):
    """ONE filter_finish_windows call per mode over the ten windows of refine_hostile_check.batch_section() (two launch groups): windows
    of 37 to 120 cells at their own blockIdx.y, one without triangles, one without a kept cell, the knife window, and the dense tenth
    whose search goes on past the rounds enqueued up front while the others settle at once.  Every finished window: the statement's
    matching, rounds, moves and settled from the window's greedy start on the window's own arrays; the objective the model's formula;
    under capacity the extra matches and the limits.  Then every window finished alone: the batched record and matching."""
    from same_amd import windows as W
    from same_amd.window_mode import WindowMode

    case = H.batch_section()
    params = H.BATCH_MODES[mode_name]
    mode = WindowMode.from_params(dict(params))
    assert (mode.refine, mode.rounds, mode.delaunay_penalty) == (params["hip_refine"], H.BATCH_ROUNDS, H.BATCH_DELAUNAY_PENALTY)
    mov = W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"])
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov, "float64"), W.DeviceSection(ref, "float64")
    states = [W.DeviceWindow() for _ in case["boxes"]]
    fargs = _filter_args(F.BATCH_FILTER, oracle)
    tris = list(case["tris"])
    try:
        counts = W.stage_windows(states, dmov, dref, list(case["boxes"]), case["radius"], case["k"], case["coeff"])
        greedy = W.filter_finish_windows(states, tris, *fargs, F.PENALTY)
        finished = [w for w, r in enumerate(greedy) if not r[2] and counts[w][2] > 0]
        assert sorted(set(range(len(states))) - set(finished)) == sorted((F.BATCH_KNIFE, F.BATCH_NO_KEPT))
        starts = {w: states[w].fetch(W._W_MATCH).copy() for w in finished}
        assert all(st.refine is None for st in states)
        res = W.filter_finish_windows(states, tris, *fargs, F.PENALTY, mode=mode)
        batched, rounds, moves = {}, {}, {}
        for w, st in enumerate(states):
            kept, added, near, row, flag, stats = res[w]
            if w == F.BATCH_KNIFE:
                assert near > 0 and row is None and flag is None and stats is None
                assert (st.refine["rounds"], st.refine["moves"], st.refine["settled"]) == (0, 0, 0), "no search ran: its words are empty"
                continue
            if w == F.BATCH_NO_KEPT:
                assert counts[w][2:] == (0, 0) and (kept, added, near) == (0, 0, 0) and len(row) == 0 and len(flag) == 0
                assert set(stats.values()) == {0}
                assert (st.refine["rounds"], st.refine["moves"], st.refine["objective_start"], st.refine["objective"]) == (0, 0, 0.0, 0.0)
                continue
            assert (kept, added, near) == greedy[w][:3] and near == 0
            pairs, costs = st.fetch(W._W_PAIRS), st.fetch(W._W_COSTS)
            rows, rows_r, match = st.fetch(W._W_ALIGNED_ROWS), st.fetch(W._W_ROWS_R), st.fetch(W._W_MATCH)
            ktris = st.fetch(W._W_TRIANGLES) if kept + added else np.zeros((0, 3), np.int32)
            n, n_r = len(rows), len(rows_r)
            assert n == counts[w][2] == len(match) and len(ktris) == kept + added and (w != F.BATCH_NO_TRIANGLES or len(ktris) == 0)
            size, axy, rxy = case["size"][rows], case["mov_xy"][rows], case["ref_xy"][rows_r]
            more = H.mode_kwargs(mode_name, n_r)
            if mode.capacity is not None:
                assert np.array_equal(W.window_ref_limits(ref.size[rows_r], pairs, mode.capacity), more["limit"])
            mp, start = _pair_index(pairs, match, n), _pair_index(pairs, starts[w], n)
            wm, wst = H.run(H.window_kwargs(pairs, costs, size, ktris, axy, rxy, **more), start, mode.rounds)
            rec = st.refine
            print("window", w, "n", n, "n_r", n_r, "triangles", len(ktris), rec, "statement", {k: v for k, v in wst.items() if k != "trace"})
            assert np.array_equal(mp, wm), w
            assert (rec["rounds"], rec["moves"], rec["settled"]) == (wst["rounds"], wst["moves"], wst["settled"]), w
            assert np.array_equal(row, np.where(match >= 0, rows_r[np.maximum(match, 0)], -1)), w
            if mode.capacity is None:
                obj = rc.lazy_objective(pairs, costs, n, ktris, axy, rxy, size, mp, F.PENALTY, mode.delaunay_penalty)
                assert set(rec) == {"rounds", "moves", "settled", "objective_start", "objective"}
                assert np.bincount(match[match >= 0], minlength=n_r).max(initial=0) <= 1
            else:
                obj, extra = rcc.model_objective(pairs, costs, n, ktris, axy, rxy, size, mp, F.PENALTY, mode.delaunay_penalty,
                                                 mode.capacity[2])
                cnt = np.bincount(match[match >= 0], minlength=n_r)
                assert rec["ref_extra_matches"] == wst["ref_extra_matches"] == extra == int(np.maximum(cnt - 1, 0).sum())
                assert np.all(cnt <= more["limit"])
            assert rec["objective"] == pytest.approx(obj, rel=1e-9) and rec["objective"] == pytest.approx(wst["objective"], rel=1e-9)
            assert rec["objective_start"] == pytest.approx(wst["objective_start"], rel=1e-9) and rec["objective"] <= rec["objective_start"]
            batched[w] = (dict(rec), match.copy(), row.copy(), flag.copy(), dict(stats))
            rounds[w], moves[w] = rec["rounds"], rec["moves"]
        assert sorted(batched) == finished
        assert rounds[H.BATCH_DENSE] > FIRST_ROUNDS and all(r <= 2 for w, r in rounds.items() if w != H.BATCH_DENSE), rounds
        assert sum(m > 0 for m in moves.values()) >= 5 and (mode_name == "capacity/1" or moves[0] == 0), moves
        for w, st in enumerate(states):
            kept, added, near, row, flag, stats = W.filter_finish_windows([st], [tris[w]], *fargs, F.PENALTY, mode=mode)[0]
            assert (kept, added, near) == res[w][:3], w
            if w in batched:
                rec, match, brow, bflag, bstats = batched[w]
                assert st.refine == rec and np.array_equal(st.fetch(W._W_MATCH), match), w
                assert np.array_equal(row, brow) and np.array_equal(flag, bflag) and stats == bstats, w
            elif w == F.BATCH_KNIFE:
                assert near > 0 and row is None and flag is None and stats is None
            else:
                assert len(row) == 0 and len(flag) == 0 and set(stats.values()) == {0}
    finally:
        for st in states:
            st.close()
        dmov.close()
        dref.close()
