"""same_amd.window_mode.WindowMode on the CPU: the value's fields and what it derives for the library, the combinations it refuses, its
constructor from optim_params against the three checks it composes, what the window path hands the library's finish calls for every
mode (a stub library records the calls: nothing reaches a device), and the decoding of a window's stats words."""
import ctypes
import threading
import types

import numpy as np
import pytest

from test_assign_cpu import _frames

CAP = (3, None, 7.0)                     # (max_matches, multiplier, penalty_coeff): the multiplier None is the library's 0
# (incumbent, refine) -> (has a capacity, finish_width, refinish_width, the finish call, the re-finish call)
MODES = {
    ("greedy", None): (False, 15, 15, "same_window_filter_finish", "same_window_refinish"),
    ("greedy", "local"): (False, 15, 15, "same_window_filter_finish", "same_window_refinish"),
    ("greedy", "capacity"): (True, 16, 16, "same_window_filter_finish_cap", "same_window_refinish_cap"),
    ("assignment", None): (False, 15, 15, "same_window_filter_finish", "same_window_refinish"),
    ("assignment", "local"): (False, 15, 15, "same_window_filter_finish", "same_window_refinish"),
    ("assignment", "capacity"): (True, 16, 16, "same_window_filter_finish_cap", "same_window_refinish_cap"),
    ("transport", None): (True, 17, 15, "same_window_filter_finish_cap", "same_window_refinish"),
    ("transport", "capacity"): (True, 17, 16, "same_window_filter_finish_cap", "same_window_refinish_cap"),
}
CODES = {"greedy": 0, "assignment": 1, "transport": 2}
ROUNDS, DP = 9, 2.5


def make(incumbent, refine):
    from same_amd.window_mode import WindowMode

    search = {} if refine is None else dict(refine=refine, rounds=ROUNDS, delaunay_penalty=DP)
    return WindowMode(incumbent, capacity=CAP if MODES[incumbent, refine][0] else None, **search)


@pytest.mark.parametrize("incumbent, refine", list(MODES))
def test_the_eight_modes(incumbent, refine):
    from same_amd.window_mode import WindowMode

    has_cap, finish_width, refinish_width, _f, _r = MODES[incumbent, refine]
    mode = make(incumbent, refine)
    assert (mode.incumbent, mode.refine, mode.capacity) == (incumbent, refine, CAP if has_cap else None)
    assert (mode.rounds, mode.delaunay_penalty) == ((ROUNDS, DP) if refine else (0, 0.0)) == mode.search_args
    assert mode.incumbent_code == CODES[incumbent]
    assert (mode.finish_width, mode.refinish_width) == (finish_width, refinish_width)
    c = mode.c_capacity()
    if has_cap:
        assert (c.max_matches, c.multiplier, c.penalty_coeff) == (3, 0, 7.0)
        assert WindowMode(incumbent, refine, mode.rounds, mode.delaunay_penalty, (2, 5, 0.0)).c_capacity().multiplier == 5
    else:
        assert c is None
    with pytest.raises(Exception):                   # immutable
        mode.rounds = 1


def test_default_is_greedy_without_a_search():
    from same_amd.window_mode import WindowMode

    assert WindowMode.default() == WindowMode() == make("greedy", None) and WindowMode.default() is WindowMode.default()


@pytest.mark.parametrize("kw, message", [
    (dict(incumbent="transport", refine="local", rounds=4, capacity=CAP), "hip_refine='local' keeps every reference to one match"),
    (dict(incumbent="transport", refine="local", rounds=4), "hip_refine='local' keeps every reference to one match"),
    (dict(incumbent="transport"), "incumbent='transport' needs its capacity, and a refine on it the same one"),
    (dict(incumbent="greedy", capacity=CAP), "capacity goes with incumbent='transport'"),
    (dict(incumbent="assignment", refine="local", rounds=4, capacity=CAP), "capacity goes with incumbent='transport'"),
    (dict(incumbent="greedy", refine="capacity", rounds=4), "needs its capacity"),
    (dict(incumbent="hungarian"), "not a window mode"),
    (dict(refine="global", rounds=4), "not a window mode"),
    (dict(refine="local"), "not a window mode"),                    # a search without rounds
    (dict(rounds=4), "not a window mode"),                          # rounds without a search
])
def test_invalid_combinations_raise(kw, message):
    from same_amd.window_mode import WindowMode

    with pytest.raises(ValueError) as e:
        WindowMode(**kw)
    assert message in str(e.value)


# the parameter dicts of test_assign_cpu, test_refine_cpu, test_refine_capacity_cpu and test_transport_cpu: (optim_params, gurobi_params)
_BAD_CAPACITY = [{"penalty_coeff": -1.0}, {"penalty_coeff": float("nan")}, {"penalty_coeff": float("inf")}, {"penalty_coeff": True},
                 {"max_matches": 0}, {"max_matches": 1.5}, {"max_matches": True}, {"ref_metacell_match_multiplier": 0},
                 {"ref_metacell_match_multiplier": 2.0}, {"ref_metacell_match_multiplier": -3}]
PARAMS = [(None, None), ({}, None), ({"hip_refine": None}, None), ({"hip_incumbent": "greedy", "max_matches": 3}, None),
          ({"hip_incumbent": "assignment"}, None), ({"hip_incumbent": "assignment"}, {"init_big_m": 200.000001}),
          ({"hip_incumbent": "hungarian"}, None), ({"hip_incumbent": "Assignment"}, None), ({"hip_incumbent": None}, None),
          ({"hip_incumbent": "assignment", "max_matches": 2}, None),
          ({"hip_incumbent": "assignment", "no_match_penalty": 100}, {"init_big_m": 200.0}),
          ({"hip_refine": "local"}, None), ({"hip_refine": "local", "hip_refine_rounds": 3, "delaunay_penalty": 0}, None),
          ({"hip_refine": "local", "hip_refine_rounds": np.int64(7), "delaunay_penalty": 2}, None),
          ({"hip_refine": "global"}, None), ({"hip_refine": "Local"}, None), ({"hip_refine": True}, None),
          ({"hip_refine": "local", "hip_refine_rounds": 0}, None), ({"hip_refine": "local", "hip_refine_rounds": -3}, None),
          ({"hip_refine": "local", "hip_refine_rounds": 2.5}, None), ({"hip_refine": "local", "hip_refine_rounds": True}, None),
          ({"hip_refine": "local", "delaunay_penalty": -1.0}, None), ({"hip_refine": "local", "delaunay_penalty": float("nan")}, None),
          ({"hip_refine": "local", "delaunay_penalty": float("inf")}, None),
          ({"hip_refine": "local", "hip_incumbent": "assignment", "delaunay_penalty": -2}, None),
          ({"hip_refine": "local", "hip_incumbent": "assignment"}, None),
          ({"hip_refine": "capacity"}, None), ({"hip_refine": "capacity", "hip_incumbent": "assignment"}, None),
          ({"hip_refine": "capacity", "max_matches": 3, "ref_metacell_match_multiplier": 2, "penalty_coeff": 0, "hip_refine_rounds": 4},
           None),
          ({"hip_incumbent": "transport", "max_matches": 2}, None), ({"hip_incumbent": "transport"}, None),
          ({"hip_incumbent": "transport", "max_matches": 3, "ref_metacell_match_multiplier": 4, "penalty_coeff": 7}, None),
          ({"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2, "hip_refine_rounds": 5}, None),
          ] + [({"hip_refine": "capacity", **bad}, None) for bad in _BAD_CAPACITY] + [
              ({"hip_incumbent": "transport", **bad}, None) for bad in _BAD_CAPACITY]


def test_from_params_agrees_with_the_three_checks():
    from same_amd.incumbent import incumbent_mode, refine_mode, transport_capacity
    from same_amd.window_mode import WindowMode

    _ref, mov = _frames()
    raised = 0
    for op, gp in PARAMS:
        before = None if op is None else dict(op)
        try:                                  # the order sliding_window_incumbent ran them in
            want = (incumbent_mode(op, gp, mov), refine_mode(op), transport_capacity(op))
        except ValueError as e:
            raised += 1
            with pytest.raises(ValueError) as got:
                WindowMode.from_params(op, gp, mov)
            assert str(got.value) == str(e), op
            continue
        incumbent, refine, capacity = want
        mode = WindowMode.from_params(op, gp, mov)
        assert op == before                   # the caller's dict is read, not completed in place
        assert mode.incumbent == incumbent and mode.refine == (op or {}).get("hip_refine")
        assert mode.search_args == ((0, 0.0) if refine is None else refine[:2])
        assert mode.capacity == (refine[2] if refine is not None and len(refine) == 3 else capacity)
        if capacity is not None and refine is not None:
            assert refine[2] == capacity
    assert raised == 16 + 2 * len(_BAD_CAPACITY)
    # valid for each of the three checks, refused as a combination: the text sliding_window_incumbent raised
    with pytest.raises(ValueError, match="hip_refine='local' keeps every reference to one match; on hip_incumbent='transport'"):
        WindowMode.from_params({"hip_incumbent": "transport", "hip_refine": "local", "max_matches": 2}, None, mov)


def test_from_params_completes_the_params_once_and_only_when_needed(monkeypatch):
    from same_amd import window_mode

    calls = []
    inner = window_mode.init_optim_params
    monkeypatch.setattr(window_mode, "init_optim_params", lambda **kw: calls.append(kw) or inner(**kw))
    window_mode.WindowMode.from_params({"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2})
    assert len(calls) == 1
    window_mode.WindowMode.from_params({"radius": 30})                    # greedy, no search: no key to check
    assert len(calls) == 1
    with pytest.raises(ValueError, match="hip_incumbent"):                  # as before: the key's own check comes first
        window_mode.WindowMode.from_params({"hip_incumbent": "hungarian", 3: "not a keyword"})
    assert len(calls) == 1


# ---- the boundary: what reaches the library
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def _stub_window(ctx, handle, kept):
    from same_amd import windows as W

    st = W.DeviceWindow.__new__(W.DeviceWindow)
    st.ctx, st.handle, st.counts, st.n_triangles = ctx, ctypes.c_void_p(handle), (kept + 2, kept + 3, kept, 4 * kept), 0
    return st


@pytest.fixture
def boundary(monkeypatch):
    """-> (stub context, the int64 arrays numpy.zeros made meanwhile: the stats arrays are among them).  The list keeps every one of
    them alive until the test ends, so no two of them ever share an address and `_handed_in` finds exactly the array a pointer names."""
    ctx = types.SimpleNamespace(lib=_StubLib(), lock=threading.Lock(), handle=None, check=lambda rc, name: None)
    made, zeros = [], np.zeros

    def spy(shape, dtype=float, **kw):
        out = zeros(shape, dtype, **kw)
        if out.dtype == np.int64:
            made.append(out)
        return out

    monkeypatch.setattr(np, "zeros", spy)
    return ctx, made


def _handed_in(made, address):
    (array,) = [a for a in made if a.ctypes.data == address]
    return array


@pytest.mark.parametrize("incumbent, refine", list(MODES))
def test_filter_finish_windows_hands_the_library_the_mode(boundary, incumbent, refine):
    from same_amd import _lib
    from same_amd import windows as W

    ctx, made = boundary
    has_cap, width, _rw, entry, _r = MODES[incumbent, refine]
    states = [_stub_window(ctx, 11, 5), _stub_window(ctx, 12, 7)]
    tris = [np.array([[0, 1, 2], [1, 2, 3]], np.int32), np.array([[0, 1, 2]], np.int32)]
    out = W.filter_finish_windows(states, tris, 25.0, 1, 0.5, 1e-9, True, 6.0, mode=make(incumbent, refine))
    ((name, args),) = ctx.lib.calls
    assert name == entry and len(args) == (20 if has_cap else 19)
    assert list(args[0]) == [11, 12] and args[1:3] == (2, _lib.SAME_TRIS_SIMPLICES)
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[4], ctypes.POINTER(ctypes.c_int64)), (3,)), [0, 2, 3])
    assert args[5:12] == (25.0, 1, 0.5, 1e-9, 1, 1, 6.0)
    assert args[12:15] == (CODES[incumbent],) + ((ROUNDS, DP) if refine else (0, 0.0))
    assert all(type(a) is t for a, t in zip(args[12:15], (int, int, float)))
    if has_cap:
        c = args[15]._obj
        assert isinstance(c, _lib.WindowCapacity) and (c.max_matches, c.multiplier, c.penalty_coeff) == (3, 0, 7.0)
    stats = _handed_in(made, args[-2])
    assert stats.shape == (2, width) and _handed_in(made, args[-1]).shape == (2, 4)
    assert [len(o[3]) for o in out] == [5, 7] and [s.n_triangles for s in states] == [0, 0]
    for s in states:                         # an all-zero record, decoded by the mode
        assert (s.assignment is None) == (incumbent == "greedy") and (s.refine is None) == (refine is None)


def test_filter_finish_windows_without_a_mode_is_the_default(boundary):
    from same_amd import windows as W

    ctx, made = boundary
    W.filter_finish_windows([_stub_window(ctx, 11, 5)], [np.array([[0, 1, 2]], np.int32)], 25.0, 1, 0.5, 0.0, True, 6.0)
    ((name, args),) = ctx.lib.calls
    assert name == "same_window_filter_finish" and args[12:15] == (0, 0, 0.0) and _handed_in(made, args[-2]).shape == (1, 15)


@pytest.mark.parametrize("incumbent, refine", list(MODES))
def test_refinish_hands_the_library_the_search_alone(boundary, incumbent, refine):
    from same_amd import _lib

    ctx, made = boundary
    _c, _fw, width, _f, entry = MODES[incumbent, refine]
    st = _stub_window(ctx, 21, 6)
    mp = np.arange(6, dtype=np.int32)
    row, flag, stats = st.refinish(mp, 6.0, make(incumbent, refine))
    ((name, args),) = ctx.lib.calls
    cap = entry.endswith("_cap")
    assert name == entry and len(args) == (9 if cap else 8)
    assert args[0].value == 21 and args[2:5] == (6.0,) + ((ROUNDS, DP) if refine else (0, 0.0))
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_int32)), (6,)), mp)
    if cap:
        c = args[5]._obj
        assert isinstance(c, _lib.WindowCapacity) and (c.max_matches, c.multiplier, c.penalty_coeff) == (3, 0, 7.0)
    assert _handed_in(made, args[-1]).shape == (width,)
    assert len(row) == len(flag) == 6 and set(stats) == set(st.STAT_NAMES) and (st.refine is None) == (refine is None)


# ---- the records
def _record():
    s = np.arange(100, 117, dtype=np.int64)
    s.view(np.float64)[[9, 13, 14]] = (1.5, 2.5, 3.5)
    return s


@pytest.mark.parametrize("incumbent, refine", list(MODES))
def test_records_decode_the_stats_words(incumbent, refine):
    from same_amd import windows as W

    mode = make(incumbent, refine)
    s = _record()[:mode.finish_width]
    asg, rfn = mode.records(s)
    want_asg = None if incumbent == "greedy" else {"rounds": 106, "flags": 108, "objective": 1.5}
    if incumbent == "transport":
        want_asg["ref_extra_matches_start"] = 116
    want_rfn = None if refine is None else {"rounds": 110, "moves": 111, "settled": 112, "objective_start": 2.5, "objective": 3.5}
    if refine is not None and len(s) > 15:
        want_rfn["ref_extra_matches"] = 115
    assert asg == want_asg and rfn == want_rfn
    assert (refine == "capacity") == (rfn is not None and "ref_extra_matches" in rfn)
    assert W._window_records(s, mode) == (asg, rfn)
    # a re-finish runs no start: its narrower record holds the search's words alone
    assert mode.records(_record()[:mode.refinish_width], start=False) == (None, want_rfn)
