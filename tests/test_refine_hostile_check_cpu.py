"""tests/refine_hostile_check.py without a GPU: every family has the property its case in tests/test_gpu_refine_library.py is about, every
wrong statement of the round rule gives another answer on the family that is named for it, every run of the oracle lowers the objective or
keeps it round by round and stays within its limits, and the batch's windows do what the batched test needs of them."""
import numpy as np
import pytest

import finish_check as F
import refine_capacity_check as rcc
import refine_check as rc
import refine_hostile_check as H

FIRST_ROUNDS = 4            # csrc/refine.h: the rounds a finish call enqueues before its first look


def _f32(d):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(d)


def test_names_are_the_issues_families():
    assert len(H.NAMES) == len(set(H.NAMES)) and set(H.DYADIC) | set(H.NOT_DYADIC) == set(H.NAMES)
    assert [H.case(f"fan/40/cap={c}")[2] for c in H.FAN_CAPS] == [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 10 ** 12]
    for name in H.NAMES:
        kw, start, _cap = H.case(name)
        again = H._BUILD[name]()
        assert all(np.array_equal(kw[k], again[0][k]) for k in kw) and np.array_equal(start, again[1]), name      # seeded
        assert kw["n"] <= 600 and len(start) == kw["n"]


@pytest.mark.parametrize("name", H.DYADIC)
def test_dyadic_families_sum_exactly(name):
    kw, _start, _cap = H.case(name)
    step = 2.0 ** -30
    for k in ("costs", "unmatched", "size"):
        assert np.array_equal(np.round(np.asarray(kw[k]) / step) * step, kw[k]) and np.all(np.abs(kw[k]) < 2.0 ** 10), (name, k)
    assert np.array_equal(np.round(kw["size"]), kw["size"])
    assert kw["delaunay_penalty"] in (5.0, 2.0 ** -12) and kw.get("penalty_coeff", 0.0) in H.PENALTY_COEFFS


@pytest.mark.parametrize("name", H.NAMES)
def test_every_run_moves_and_never_raises_the_objective(name):
    kw, start, cap = H.case(name)
    match, st = H.statement(name)
    assert (st["moves"] > 0) or name in H.EMPTY_NAMES, "every family but the empty calls makes a move"
    assert st["rounds"] <= cap and (st["settled"] == 1 or st["rounds"] == cap)
    assert len(st["trace"]) == st["rounds"] + 1 and all(b <= a for a, b in zip(st["trace"], st["trace"][1:])), st["trace"]
    assert st["objective"] == st["trace"][-1] and np.isfinite(st["objective"])
    prob = H.problem(kw)
    if H.is_cap(kw):
        count = prob.counts(list(match))                  # (asserts count <= limit)
        assert all(c <= l for c, l in zip(count, prob.limit)) and st["ref_extra_matches"] == sum(max(0, c - 1) for c in count)
    else:
        prob.owners(list(match))                          # (asserts one-to-one)
    if kw["n"] == 0:
        assert (st["rounds"], st["moves"], st["objective_start"], st["objective"]) == (0, 0, 0.0, 0.0)


def test_the_fan_runs_one_move_a_round_across_every_chunk_edge():
    for m, name in ((40, "fan/40/cap=1000000000000"), (300, "fan/300")):
        kw, _start, _cap = H.case(name)
        prob = H.problem(kw)
        assert len(prob.inc[0]) == m and all(0 in prob.tris[t] for t in range(m)), "a hub of degree m, in every footprint"
        _match, st = H.statement(name)
        assert (st["rounds"], st["moves"], st["settled"]) == (m + 1, m + 1, 1)
        assert st["trace"][-1] > sum(np.asarray(kw["costs"])), "triangles are flipped at the end: the hub's walk counts"
    for cap in H.FAN_CAPS:
        _match, st = H.statement(f"fan/40/cap={cap}")
        assert (st["rounds"], st["moves"], st["settled"]) == ((cap, cap, 0) if cap < 41 else (41, 41, 1))
    # the host form's chunks are 16, 32, 64, ...: the caps sit on, before and after the first three edges, and 41 rounds need three
    assert {15, 16, 17, 47, 48, 49} <= set(H.FAN_CAPS) and 16 + 32 > 41 > 16


def test_contested_deltas_are_equal_as_floats_and_differ_in_fp64():
    kw, start, _cap = H.case("contested/50")
    m = 50
    d = H.deltas_of_round_one(kw, start)
    assert len(d) == kw["n"] == 4 * m
    for j in range(2 * m):
        i, k = 2 * j, 2 * j + 1
        assert d[k] < d[i] < 0.0
        assert (_f32(d[i]) == _f32(d[k])) == (j < m)
    match, _st = H.statement("contested/50")
    pairs = np.asarray(kw["pairs"])
    assert all(match[2 * j + 1] < 0 for j in range(m)), "near-ties go to the lower cell"
    assert sum(match[2 * j] >= 0 for j in range(m)) > m // 2
    assert all(match[2 * j] < 0 for j in range(m, 2 * m)) and sum(match[2 * j + 1] >= 0 for j in range(m, 2 * m)) > m // 2
    assert np.array_equal(pairs[:, 0], np.arange(4 * m))


def test_scaled_keys_are_subnormal_and_beyond_range():
    tiny = 2.0 ** -126
    kw, start, _cap = H.case("scaled/-140")
    d = np.array(list(H.deltas_of_round_one(kw, start).values()))
    assert len(d) > 10 and np.all(_f32(d) != 0.0) and np.all(np.abs(_f32(d).astype(np.float64)) < tiny)
    assert len(np.unique(_f32(d))) > 10, "distinct subnormal keys"
    kw, start, _cap = H.case("scaled/130")
    d = np.array(list(H.deltas_of_round_one(kw, start).values()))
    assert len(d) > 10 and np.all(np.isfinite(d)) and np.all(np.isneginf(_f32(d)))
    small, plain, big = (H.statement(f"scaled/{e}") for e in H.SCALES)
    assert H.answer(*small) == H.answer(*plain) and (plain[1]["rounds"], plain[1]["moves"]) == (7, 50)
    assert H.answer(*big) != H.answer(*plain), "with every key tied the cell decides: another search"


def test_triangle_lists_are_what_their_names_say():
    base, _start, _cap = H.case("triangles/as is")
    n = base["n"]
    key = lambda t: sorted(map(tuple, np.sort(np.asarray(t), axis=1).tolist()))
    shuf = H.case("triangles/shuffled")[0]["triangles"]
    assert key(shuf) == key(base["triangles"]) and not np.array_equal(shuf, base["triangles"])
    assert not np.array_equal(np.sort(shuf, axis=1), shuf), "corners not in ascending order"
    assert H.answer(*H.statement("triangles/shuffled")) == H.answer(*H.statement("triangles/as is")), "only the triangle set matters"
    dbl = key(H.case("triangles/doubled")[0]["triangles"])
    counts = np.unique(np.array(dbl), axis=0, return_counts=True)[1]
    assert set(counts.tolist()) == {2, 3} and len(counts) == len(base["triangles"]) and (counts == 3).sum() == -(-len(counts) // 3)
    twice = np.asarray(H.case("triangles/corner twice")[0]["triangles"])
    rep = (twice[:, 0] == twice[:, 1]) | (twice[:, 1] == twice[:, 2]) | (twice[:, 0] == twice[:, 2])
    assert rep.sum() == 240
    moved = H.statement("triangles/corner twice")[0] != H.case("triangles/corner twice")[1]
    assert moved[np.unique(twice[rep])].any(), "a cell that moves is named twice by a triangle"
    assert len(H.case("triangles/long")[0]["triangles"]) == 5 * n and len(H.case("triangles/none")[0]["triangles"]) == 0
    assert H.statement("triangles/long")[1]["rounds"] > 16


def test_a_sign_zero_triangle_is_incident_to_a_cell_that_moves():
    kw, start, _cap = H.case("triangles/collinear")
    prob = H.problem(kw)
    flat = [t for t in range(len(prob.tris)) if prob.sign[t] == 0]
    assert len(flat) > 50 and all(len(set(prob.tris[t])) == 3 for t in flat), "collinear, not repeated, corners"
    moved = set(np.flatnonzero(H.statement("triangles/collinear")[0] != start).tolist())
    assert any(set(prob.tris[t]) & moved for t in flat)


def test_shuffled_pairs_are_not_grouped_and_the_start_is_renumbered():
    kw, start, _cap = H.case("pairs/shuffled")
    base, bstart, _cap = H.case("triangles/as is")
    rows = np.asarray(kw["pairs"])[:, 0]
    assert (np.diff(rows) < 0).sum() > 100, "the library's `where` is not the identity"
    on = start >= 0
    assert np.array_equal(on, bstart >= 0) and np.array_equal(np.asarray(kw["pairs"])[start[on]], np.asarray(base["pairs"])[bstart[on]])
    assert np.array_equal(rows[start[on]], np.flatnonzero(on))


def test_sizes_sit_on_the_block_edges():
    assert [H.case(f"size/n={n}")[0]["n"] for n in H.SIZES] == [255, 256, 257, 511, 512, 513]
    shapes = [(H.case(f"size/n={n},n_r={r}")[0]["n"], H.case(f"size/n={n},n_r={r}")[0]["n_r"]) for n, r in H.CAP_SIZES]
    assert shapes == [(200, 56), (200, 57), (5, 1000), (600, 3)] and 200 + 56 == 256
    assert [tuple(len(H.case(n)[0][k]) if k in ("pairs", "triangles") else H.case(n)[0][k] for k in ("n", "n_r", "pairs", "triangles"))
            for n in H.EMPTY_NAMES] == list(H.EMPTY)
    _m, st = H.statement("size/n=600,n_r=3")
    assert st["settled"] == 0 and st["rounds"] == 64, "a cap that is reached inside the fourth chunk (16 + 32 + 16)"


def test_fractional_sizes_make_the_order_of_f_count():
    kw, start, _cap = H.case("fractional")
    assert set(np.unique(kw["size"]).tolist()) == set(H.FRACTIONS)
    _sizes, order, by_corners, by_index = H._order_gadget(kw["delaunay_penalty"])
    assert by_corners != by_index and order != (0, 1, 2)
    c = kw["n"] - 7
    prob = H.problem(kw)
    assert [prob.tris[t] for t in prob.inc[c]] == sorted(prob.tris[t] for t in prob.inc[c]) and prob.inc[c] != sorted(prob.inc[c])
    m = [int(p) for p in start]
    (d_un, *_u), (d_a, _s, p_a, *_a), (d_b, _s2, p_b, *_b) = prob.moves(m, prob.owners(m), c)
    assert d_a == by_corners and d_b == min(by_corners, by_index) and d_un > 0.0
    match, _st = H.statement("fractional")
    assert match[c] == (p_a if by_corners <= by_index else p_b)
    assert np.any(np.asarray(kw["costs"]) * 2.0 ** 20 % 1.0 != 0.0), "costs not dyadic"


def test_signed_costs_and_capacity_starts():
    assert (np.asarray(H.case("signed")[0]["costs"]) < 0).sum() > 100
    kw, start, _cap = H.case("capacity/filled")
    prob = H.problem(kw)
    count = prob.counts(list(start))
    full = [j for j in range(prob.n_r) if prob.limit[j] > 1 and count[j] == prob.limit[j]]
    assert len(full) >= H.LEAVERS + 5, "references filled to their limit exactly"
    match, st = H.statement("capacity/filled")
    after = prob.counts(list(match))
    lead = prob.n_r - 3 * H.LEAVERS
    assert all((count[lead + 3 * g], after[lead + 3 * g]) == (2, 1) for g in range(H.LEAVERS)), "one leaver went, one stayed"
    for pc in H.PENALTY_COEFFS:
        for fam in ("contested", "fan"):
            kw, _s, _c = H.case(f"capacity/{fam}/pc={pc}")
            assert set(np.unique(kw["limit"]).tolist()) == set(H.LIMITS) and kw["penalty_coeff"] == pc
    assert H.statement("capacity/contested/pc=0.0")[1]["ref_extra_matches"] > 10
    assert H.statement("capacity/contested/pc=100.0")[1]["ref_extra_matches"] == 0
    m1, s1 = H.statement("capacity/contested/pc=100.0")
    m0, s0 = H.statement("contested/50")
    assert H.answer(m1, s1) == H.answer(m0, s0), "a capacity too dear to use: the one-to-one search"


@pytest.mark.parametrize("wrong", H.WRONG)
def test_each_wrong_statement_is_told_apart_by_its_family(wrong):
    name = H.TOLD_BY[wrong]
    kw, start, cap = H.case(name)
    assert H.is_cap(kw) or wrong != "old reference not claimed"
    got = H.answer(*H.run(kw, start, cap, wrong=wrong))
    assert got != H.answer(*H.statement(name)), (wrong, name)
    assert H.answer(*H.run(kw, start, cap)) == H.answer(*H.statement(name)) and rc._key is rcc._key and rc._key.__module__ == "refine_check"


def test_limit_one_is_the_plain_statement():
    """what the GPU test asks of the library holds of the oracle: with every limit 1 the capacity statement is the plain one"""
    for name in ("contested/50", "triangles/long", "fan/40/cap=17"):
        kw, start, cap = H.case(name)
        for pc in (0.0, 100.0):
            got = H.run(dict(kw, limit=np.ones(kw["n_r"], np.int32), penalty_coeff=pc), start, cap)
            assert H.answer(*got) == H.answer(*H.statement(name)) and got[1]["objective"] == H.statement(name)[1]["objective"]


def test_the_batch_has_a_window_that_runs_on_and_windows_that_settle_at_once(oracle):
    case = H.batch_section()
    base = F.batch_section()
    assert len(case["boxes"]) == F.BATCH_WINDOWS + 1 == H.BATCH_DENSE + 1
    rows = len(base["mov_xy"])
    assert np.array_equal(case["mov_xy"][:rows], base["mov_xy"]) and np.array_equal(case["ref_xy"][:len(base["ref_xy"])], base["ref_xy"])
    wins = [H.cpu_window(case, w, oracle) for w in range(len(case["boxes"]))]
    assert [w for w, x in enumerate(wins) if x is None] == sorted((F.BATCH_KNIFE, F.BATCH_NO_KEPT))
    assert len(wins[F.BATCH_NO_TRIANGLES][0][3]) == 0
    for name in H.BATCH_MODES:
        rounds, moves = {}, {}
        for w, x in enumerate(wins):
            if x is None:
                continue
            arrays, start = x
            _m, st = H.run(H.window_kwargs(*arrays, **H.mode_kwargs(name, len(arrays[5]))), start, H.BATCH_ROUNDS)
            rounds[w], moves[w] = st["rounds"], st["moves"]
            assert st["settled"] == 1
        print(name, rounds, moves)
        assert rounds[H.BATCH_DENSE] > FIRST_ROUNDS and all(r <= 2 for w, r in rounds.items() if w != H.BATCH_DENSE), (name, rounds)
        assert sum(m > 0 for m in moves.values()) >= 5
        if name != "capacity/1":
            assert moves[0] == 0, "a window that makes no move"
