"""same_delaunay_filtered and same_window_delaunay (csrc/delaunay_dev.hip) driven at the LIBRARY against the plain host statement of
the call (tests/delaunay_dev_check.candidates: scipy's triangles that pass the slack screen, owner first, counter-clockwise, by owner,
then q, then r -- ARRAY equal): tiny sets, sizes on a scan block's edge, a grid that doubles, one row of cells, coordinates on both
sides of 0 and on cell boundaries, every capacity answered on one side and refused with its bit on the other, coordinates that are
not finite, settings without a bound, small angle thresholds, and three ladders that open an exactly degenerate configuration rung by
rung -- a rung may be refused, an answered rung must be exactly right.  The window call: the families side by side in one section, in
batches in order, reversed, over two launch groups with skipped windows between, at SAME_WINDOW_BATCH_MAX, and again on states staged
before on other boxes; per window the status, the count and -- the way the triangles on the device are observed -- the whole finish
from the device's candidates against the finish of a fresh staging from the statement's triangles handed over as host simplices.
The inputs come from tests/delaunay_dev_check.py; tests/test_delaunay_dev_check_cpu.py proves without a GPU that each has the property
its case is about."""
import ctypes
import functools

import numpy as np
import pytest

import delaunay_dev_check as D

pytestmark = pytest.mark.gpu


def _W():
    from same_amd import windows as W

    return W


def _guard():
    from same_amd import delaunay

    return delaunay.GUARD


def _settings(angle):
    from same_amd.triangles import cos_threshold

    return cos_threshold(angle)


# ---- the set call ------------------------------------------------------------------------------------------------------------------
def _call(ctx, xy, radius, angle_enabled, cos_thr, n=None):
    """same_delaunay_filtered itself, not the Python wrapper -> (return code, status, triangles written, *out_n_tris)"""
    pts = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(pts) if n is None else n
    out = np.full((max(2 * n, 1), 3), -7, np.int32)
    n_tris, status = ctypes.c_int64(-1), ctypes.c_int(-1)
    with ctx.lock:
        rc = ctx.lib.same_delaunay_filtered(ctx.handle, pts.ctypes.data, n, float(radius), int(angle_enabled), float(cos_thr), float(_guard()),
                                            out.ctypes.data, len(out), ctypes.byref(n_tris), ctypes.byref(status))
    assert n_tris.value >= 0 and (out[n_tris.value:] == -7).all()              # nothing written past the count
    return rc, status.value, out[:n_tris.value].copy(), n_tris.value


def _call_family(ctx, name):
    f = D.family(name)
    return _call(ctx, f["xy"], f["radius"], *_settings(f["angle"]))


@functools.lru_cache(maxsize=None)
def _fresh(name):
    """the family's answer from a context of its own: no slot has held anything before"""
    from same_amd import _lib

    ctx = _lib.Context(0)
    try:
        return _call_family(ctx, name)
    finally:
        ctx.close()


def _held_to(name, answer, expect, bit, want):
    rc, status, tris, n_tris = answer
    print(name, "status", status, "triangles", n_tris)
    assert rc == 0, (name, rc)
    if expect == D.ANSWER:
        assert status == 0, (name, status)
    elif expect == D.REFUSE:
        assert status & bit and status > 0 and n_tris == 0, (name, status, n_tris)
    elif status:
        assert status == bit and n_tris == 0, (name, status, n_tris)       # a refusal may carry the named bit only
    if status == 0:
        D.same_candidates(tris, want)


@pytest.mark.parametrize("name", D.NAMES)
def test_set_call_is_held_to_its_tag(name):
    """every family through same_delaunay_filtered: answered and ARRAY equal to the statement, refused with its bit, or -- small angles,
    the ladders' middle rungs -- either; a ladder's rung 0 is refused and its top rung answered"""
    expect, bit = D.expectation(name)
    want = None if name.startswith("nonfinite/") else D.statement_of(name)
    _held_to(name, _fresh(name), expect, bit, want)


@pytest.mark.parametrize("case", D.settings_cases(), ids=[c[0] for c in D.settings_cases()])
def test_settings_without_a_bound_and_sets_without_a_triangle(case):
    from same_amd import _lib

    _tag, n, radius, en, thr, status = case
    rc, got, _tris, n_tris = _call(_lib.default_context(0), D.uniform(257, 3257)[:n], radius, en, thr)
    assert (rc, got, n_tris) == (0, status, 0)
    assert (D.FEW_POINTS, D.NO_ANGLE, D.NONFINITE, D.IN_DOUBT, D.OVERFLOW) == (_lib.SAME_DD_FEW_POINTS, _lib.SAME_DD_NO_ANGLE,
                                                                                 _lib.SAME_DD_NONFINITE, _lib.SAME_DD_IN_DOUBT, _lib.SAME_DD_OVERFLOW)


def test_one_contexts_slots_at_shrinking_and_growing_sizes_and_after_refusals():
    """hull1024, small n = 3, nb129 (refused), nb128, sparse, own33 (refused), own32 on ONE context: every answer is the one a context
    of its own gave"""
    from same_amd import _lib

    ctx = _lib.Context(0)
    try:
        for name in D.CALL_ORDER + D.CALL_ORDER[::-1]:
            got, fresh = _call_family(ctx, name), _fresh(name)
            expect, bit = D.expectation(name)
            _held_to(name, got, expect, bit, D.statement_of(name))
            assert got[0] == fresh[0] and (got[1] == 0) == (fresh[1] == 0) and np.array_equal(got[2], fresh[2]), name
    finally:
        ctx.close()


# ---- the window call ---------------------------------------------------------------------------------------------------------------
_DEVICE, _SIMPLICES, _WANT, _HOST_FINISH = {}, {}, {}, {}


def _device(sec):
    key = id(sec)
    if key not in _DEVICE:
        W = _W()
        mov = W.Section(sec["mov_xy"], sec["types_m"], sec["type_id"], sec["size"])
        ref = W.Section(sec["ref_xy"], sec["types_r"], None, None)
        _DEVICE[key] = (W.DeviceSection(mov, np.float64), W.DeviceSection(ref, np.float64), sec)       # (the section is held: its id stays its own)
    return _DEVICE[key][:2]


def _rows(sec, w):
    return np.arange(sec["first"][w], sec["first"][w + 1])


def _want(sec, w, radius, angle):
    """the statement of window w of the section at the call's settings, made once; None for a window without a triangle"""
    key = (id(sec), w, radius, angle)
    if key not in _WANT:
        xy = sec["mov_xy"][_rows(sec, w)]
        if len(xy) < 3 or sec["names"][w] == D.NO_CELL:
            _WANT[key] = None
        else:
            if (id(sec), w) not in _SIMPLICES:
                _SIMPLICES[(id(sec), w)] = D.scipy_simplices(xy)
            _WANT[key] = D.candidates(xy, radius, angle, _SIMPLICES[(id(sec), w)])
    return _WANT[key]


def _expectation(sec, w, radius, angle):
    name = sec["names"][w]
    if name.startswith("batch/"):
        return (D.REFUSE, D.FEW_POINTS) if sec["sizes"][w] < 3 else (D.ANSWER, 0)
    return D.window_expectation(name, radius, angle)


def _finish_args(radius, angle):
    en, thr = _settings(angle)
    return (radius, en, thr, float(8 * np.spacing(abs(thr))), True, D.WINDOW_PENALTY)


def _record(st, res):
    kept, added, near, row, flag, stats = res
    tris = st.fetch(_W()._W_TRIANGLES) if not near and kept + added else None
    return dict(kept=kept, added=added, near=near, row=row, flag=flag, stats=stats, tris=tris)


def _same_record(got, want, tag):
    assert (got["kept"], got["added"], got["near"]) == (want["kept"], want["added"], want["near"]), (tag, got["kept"], got["added"], got["near"])
    assert got["stats"] == want["stats"], (tag, got["stats"], want["stats"])
    for key in ("row", "flag", "tris"):
        assert (got[key] is None) == (want[key] is None) and (got[key] is None or np.array_equal(got[key], want[key])), (tag, key)


def _host_finish(sec, w, radius, angle):
    """a FRESH staging of the window's box finished with the statement's triangles as host simplices, made once"""
    key = (id(sec), w, radius, angle)
    if key not in _HOST_FINISH:
        W = _W()
        dmov, dref = _device(sec)
        st = W.DeviceWindow()
        try:
            st.stage(dmov, dref, sec["boxes"][w], sec["radius"], sec["k"], sec["coeff"])
            _HOST_FINISH[key] = _record(st, W.filter_finish_windows([st], [_want(sec, w, radius, angle)], *_finish_args(radius, angle))[0])
        finally:
            st.close()
    return _HOST_FINISH[key]


def _run(states, sec, order, radius, angle, tag):
    """stage states[slot] on the box of window order[slot], ONE same_window_delaunay over them, every slot held to its window's
    expectation; ONE device-source finish over the answered ones, each against the host finish of its statement"""
    W = _W()
    dmov, dref = _device(sec)
    states = states[:len(order)]
    counts = W.stage_windows(states, dmov, dref, [sec["boxes"][w] for w in order], sec["radius"], sec["k"], sec["coeff"])
    en, thr = _settings(angle)
    status, n_tris = W.triangulate_windows(states, radius, en, thr, _guard())
    answered = []
    for slot, w in enumerate(order):
        name, want = sec["names"][w], _want(sec, w, radius, angle)
        expect, bit = _expectation(sec, w, radius, angle)
        s, k = int(status[slot]), int(n_tris[slot])
        print(tag, "slot", slot, name, "cells", counts[slot][2], "status", s, "triangles", k)
        kept_rows = _rows(sec, w) if name != D.NO_CELL else _rows(sec, w)[:0]
        assert counts[slot][2] == len(kept_rows) and np.array_equal(states[slot].fetch(W._W_ALIGNED_XY), sec["mov_xy"][kept_rows]), (tag, slot, name)
        if expect == D.ANSWER:
            assert s == 0, (tag, slot, name, s)
        elif expect == D.REFUSE:
            assert s & bit and s > 0 and k == 0, (tag, slot, name, s, k)
            assert s == bit or bit != D.FEW_POINTS, (tag, slot, name, s)
        elif s:
            assert s & ~bit == 0 and k == 0, (tag, slot, name, s, k)
        if s == 0:
            assert k == len(want), (tag, slot, name, k, len(want))
            answered.append(slot)
    if answered:
        res = W.filter_finish_windows([states[slot] for slot in answered], None, *_finish_args(radius, angle))
        for slot, r in zip(answered, res):
            _same_record(_record(states[slot], r), _host_finish(sec, order[slot], radius, angle), (tag, slot, sec["names"][order[slot]]))
    return status


def _states(n):
    W = _W()
    return [W.DeviceWindow() for _ in range(n)]


def _close(states):
    for st in states:
        st.close()


@pytest.mark.parametrize("radius,angle", D.WINDOW_SETTINGS)
def test_window_batch_in_order_and_reversed(radius, angle):
    """the families' windows, the 2-cell window and the window without a kept cell in ONE call (three launch groups), in the section's
    order and reversed (the skipped windows first: every later window's status comes from another slot of the copy-back)"""
    sec = D.window_section()
    order = list(range(len(sec["names"])))
    states = _states(len(order))
    try:
        status = _run(states, sec, order, radius, angle, "in order")
        back = _run(states, sec, order[::-1], radius, angle, "reversed")
        assert np.array_equal(status == 0, back[::-1] == 0)
        assert len(order) > 2 * D.LAUNCH_WINDOWS and np.count_nonzero(status == 0) >= 12
    finally:
        _close(states)


def test_window_batch_of_nine_and_of_ten():
    """nine windows: a refused one in slots 0 and 8, the window without a kept cell in slot 4; then a tenth, so that the nine that reach
    the kernels are two launch groups and the last status is read from a slot one lower than the window's own"""
    sec = D.window_section()
    nine = [D.window_index(n) for n in ("nb129", "nb128", "small/3", "own32", D.NO_CELL, "edges/257", "small/8", "sparse", "own33")]
    states = _states(10)
    try:
        status = _run(states, sec, nine, 25.0, 10.0, "nine")
        assert status[0] & D.OVERFLOW and status[8] & D.OVERFLOW and status[4] == D.FEW_POINTS and not status[[1, 2, 3, 5, 6]].any()
        status = _run(states, sec, nine + [D.window_index("edges/255")], 25.0, 10.0, "ten")
        assert status[0] & D.OVERFLOW and status[8] & D.OVERFLOW and status[4] == D.FEW_POINTS and status[9] == 0
    finally:
        _close(states)


def test_window_batch_at_the_batch_maximum():
    """SAME_WINDOW_BATCH_MAX windows of 50 to 300 points, every third one a box of 2 cells: 43 sets in six launch groups of mixed sizes"""
    sec = D.batch_section()
    states = _states(D.WINDOW_BATCH_MAX)
    try:
        status = _run(states, sec, list(range(D.WINDOW_BATCH_MAX)), 25.0, 15.0, "batch max")
        assert np.array_equal(status != 0, np.arange(D.WINDOW_BATCH_MAX) % 3 == 2)
    finally:
        _close(states)


def test_windows_staged_again_on_other_boxes():
    """the first batch; every state staged again on another family's box, larger or smaller, after an answer or a refusal (dd_work and
    dd_tris are reused, only the head is zeroed); then the first batch again"""
    sec = D.window_section()
    order = list(range(len(sec["names"])))
    states = _states(len(order))
    try:
        first = _run(states, sec, order, 25.0, 10.0, "first")
        for shift in (7, 16):
            moved = order[shift:] + order[:shift]
            sizes = np.diff(sec["first"])
            assert (sizes[moved] > sizes[order]).any() and (sizes[moved] < sizes[order]).any()
            _run(states, sec, moved, 25.0, 10.0, f"moved by {shift}")
        again = _run(states, sec, order, 25.0, 10.0, "again")
        assert np.array_equal(first == 0, again == 0)
    finally:
        _close(states)
