"""windows.batch_schedule -- the order of a batch's calls in windows.iter_device_windows, as data -- and the walk's pool of window states,
without a device:
 * the schedules of a few inputs, literally;
 * over every small input, the schedule run through a model of what the library's calls leave of a window's pair list (which variant
   priced it, the knn it is cut to, whether it is pruned, whether it went through the caller's node masks): every set is finished once,
   on the list that is its own;
 * whatever ends a walk -- a refused library call, a triangulator that raises, a consumer that walks away -- every window state the
   walk made is afterwards in its context's cache, once, or closed (the stand-ins of tests/test_window_walk_cpu.py)."""
import itertools
import types

import numpy as np
import pytest

from same_amd import delaunay
from same_amd import windows as W
from test_window_walk_cpu import _State, walk  # noqa: F401  (the fixture)

F = lambda q: ("finish", q)          # noqa: E731
PRUNE, PAIRS = ("priority",), ("caller_pairs",)
FIVE = [(8, 0), (4, 0), (8, 1), (4, 1), (4, 2)]


def test_literal_schedules():
    assert W.batch_schedule(FIVE, [True, False, True], False, False) == [
        F(2), ("prefix", 4), F(3), ("recost", 0), F(0), ("prefix", 4), F(1), ("recost", 2), ("prefix", 4), F(4)]
    # prune and caller: the pair after every prefix and after the recost no prefix follows; nothing before the first finish
    assert W.batch_schedule(FIVE, [True, False, True], True, True) == [
        F(2), ("prefix", 4), PRUNE, PAIRS, F(3), ("recost", 0), PRUNE, PAIRS, F(0), ("prefix", 4), PRUNE, PAIRS, F(1),
        ("recost", 2), ("prefix", 4), PRUNE, PAIRS, F(4)]
    # tests/test_window_walk_cpu.py::test_sets' order
    assert W.batch_schedule([(2, 0), (8, 0), (2, 0), (1, 0)], [False], False, False) == [F(1), ("prefix", 2), F(0), F(2), ("prefix", 1), F(3)]
    assert W.batch_schedule([(4, 0), (4, 1)], [False, False], True, False) == [F(0), F(1)]
    assert W.batch_schedule([(8, 0)], [False], False, False) == [F(0)]
    # the walk's own sets are (knn, mode, penalty, variant): the first and the last entry are read
    assert W.batch_schedule([(2, None, 1.0, 0), (8, None, 1.0, 0)], [False], True, True) == [F(1), ("prefix", 2), PRUNE, PAIRS, F(0)]


def _small_inputs():
    for n_variants in (1, 2, 3):
        one = list(itertools.product((1, 2, 8), range(n_variants)))
        for n_sets in (1, 2, 3, 4):
            for sets in itertools.product(one, repeat=n_sets):
                for layered in itertools.product((False, True), repeat=n_variants):
                    yield sets, layered


def test_every_set_is_finished_once_on_its_own_list():
    """the model: `recost v` -> (v, staged k, unpruned, uncompacted); `prefix k` -> (same v, k, unpruned, uncompacted); `priority` ->
    pruned; `caller_pairs` -> compacted; the front calls leave (a None variant, staged k, pruned if the prune is on, compacted if
    there is a caller)"""
    cases = 0
    for sets, layered in _small_inputs():
        staged = max(k for k, _v in sets)
        for priority, caller in ((False, False), (False, True), (True, False), (True, True)):
            steps = W.batch_schedule(sets, layered, priority, caller)
            v, k, pruned, compacted = None, staged, priority, caller
            finished = []
            for kind, *arg in steps:
                if kind == "recost":
                    assert layered[arg[0]]
                    v, k, pruned, compacted = arg[0], staged, False, False
                elif kind == "prefix":
                    assert arg[0] != k                   # (a prefix at the k the list is at would be a call for nothing)
                    k, pruned, compacted = arg[0], False, False
                elif kind == "priority":
                    assert priority and not pruned
                    pruned = True
                elif kind == "caller_pairs":
                    assert caller and not compacted
                    compacted = True
                else:
                    assert kind == "finish"
                    set_k, set_v = sets[arg[0]]
                    assert (v == set_v) if layered[set_v] else (v is None or not layered[v]), (sets, layered, steps)
                    assert k == set_k and pruned == priority and compacted == caller, (sets, layered, priority, caller, steps)
                    finished.append(arg[0])
            assert sorted(finished) == list(range(len(sets))), (sets, layered, steps)
            assert sum(s[0] == "recost" for s in steps) == len({sv for _k, sv in sets if layered[sv]})
            cases += 1
    assert cases == 4 * sum((3 * n) ** m * 2 ** n for n in (1, 2, 3) for m in (1, 2, 3, 4))


# ---- the pool of window states --------------------------------------------------------------------------------------------------------
NINE = [dict(box=(float(q % 5), 0.0, 0.0, 0.0), window_id=q) for q in range(9)]        # (windows 2 and 7 are staged without pairs)


class Refused(Exception):
    pass


@pytest.fixture
def counted(monkeypatch, walk):  # noqa: F811
    """-> (run, check): `run` the walk fixture's over NINE with a context of its own; `check()` after it: every state made is in the
    context's cache or closed, none twice -> (made, cached, closed)"""
    made, closed, ctx = [], [], types.SimpleNamespace()

    class Counted(_State):
        def __init__(self, ctx=None):
            super().__init__(ctx)
            made.append(self)

        def close(self):
            closed.append(self)

    monkeypatch.setattr(W, "DeviceWindow", Counted)

    def check():
        cache = ctx._device_windows
        assert len(made) == len(cache) + len(closed)
        assert len({id(s) for s in cache + closed}) == len(cache) + len(closed) and {id(s) for s in cache + closed} == {id(s) for s in made}
        return len(made), len(cache), len(closed)

    return (lambda **kw: walk(plan=NINE, ctx=ctx, **kw)), check


def test_a_refused_library_call_leaves_every_state_with_the_context(counted, monkeypatch):
    run, check = counted
    calls, real = [], W.priority_windows

    def priority_windows(states):
        calls.append(len(states))
        if len(calls) == 3:
            raise Refused("same_window_priority_pairs")
        return real(states)

    monkeypatch.setattr(W, "priority_windows", priority_windows)
    with pytest.raises(Refused):
        run(priority=True)
    assert calls == [2, 2, 2] and check() == (4, 4, 0)


def test_a_triangulator_that_raises_leaves_every_state_with_the_context(counted):
    run, check = counted

    class Fifth(delaunay.Triangulator):
        def submit(self, points, key=None):
            if key == 4:
                raise Refused("submit")
            return delaunay.Ticket(self, points, simplices=np.array([[0, 1, 2]], np.int32), native=False)

    with pytest.raises(Refused):
        run(triangulator=Fifth())
    assert check() == (4, 4, 0)


def test_an_abandoned_walk_leaves_every_state_with_the_context(counted):
    run, check = counted

    def first_only(generator):
        first = next(generator)
        generator.close()
        return [first]

    _log, results, _c = run(take=first_only)
    assert results[0].window["window_id"] == 0 and check() == (2, 2, 0)


def test_a_context_keeps_what_one_pass_needs(counted):
    """a finished walk: the same invariant; and a second pass over the context makes no state"""
    run, check = counted
    run()
    first = check()
    run()
    assert check() == first and first[2] == 0
