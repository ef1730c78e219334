"""The input families of tests/finish_check.py, checked WITHOUT a GPU: every family has the property its GPU test of the window finish
call (same_window_filter_finish / same_window_refinish, csrc/window_finish.hip with csrc/match.hip's greedy rounds) is about -- a scan
sized to a block edge, equal smallest perimeters, cosines on the threshold, a chain of 200 greedy rounds, rows on the penalty, cells
with both flag bits -- by proof with the oracle, not by luck.  And the evidence that a kernel wrong in one of six ways fails the GPU
test: each deliberately wrong statement gives another answer than the right one on at least one family."""
import numpy as np
import pytest

import caller_check as C
import finish_check as F

DTYPES = ("float64", "float32")
ALL_TAGS = tuple(f"edge/{name}" for name in F.EDGE_LISTS) + F.TAGS
_CACHE = {}


def _window(tag, dtype, oracle):
    """(section, triangles, filter settings, the arrays as staged on the host, the statement) of a tag, worked out once"""
    key = (tag, dtype)
    if key not in _CACHE:
        case, tris, filt = F.window_of(tag, oracle)
        skey = (id(case), dtype)
        if skey not in _CACHE:
            _CACHE[skey] = F.cpu_staged(case, oracle, dtype)
        staged = _CACHE[skey]
        start = _CACHE.get((skey, "start"))
        want = F.of_case(case, staged, tris, filt, oracle, start=start)
        if want["near"] == 0:
            _CACHE[(skey, "start")] = want["start"]
        _CACHE[key] = (case, tris, filt, staged, want)
    return _CACHE[key]


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_every_row_is_a_kept_cell_and_near_is_zero_but_on_the_knife(oracle, tag):
    case, tris, filt, staged, want = _window(tag, "float64", oracle)
    n = len(case["mov_xy"])
    assert np.array_equal(staged["rows"], np.arange(n)) and tris.min() >= 0 and tris.max() < n
    assert np.bincount(staged["pairs"][:, 0], minlength=n).min() >= 1
    assert (want["near"] > 0) == (tag in F.NEAR_TAGS)
    if tag in F.NEAR_TAGS:
        assert want["row"] is None and want["flag"] is None and want["stats"] is None
    # the numpy restatement of the add-back and of the greedy start is the oracle's (the reference's) on this window
    again = F.restated(case, staged, tris, filt, oracle)
    assert again["near"] == want["near"] and np.array_equal(again["tris"], want["tris"])
    if want["near"] == 0:
        assert F.same_answer(again, want) and again["rounds"] == want["stats"]["greedy_rounds"]


def test_edge_lists_have_exact_row_counts_and_all_four_classes(oracle):
    case = F.edge_section()
    lists = F.edge_lists(oracle)
    assert len(case["mov_xy"]) == 16385 and len(case["tris"]) > 2 * 16385 - 600
    for m in F.EDGE_TRIANGLES:
        tris = lists[f"Tr={m}"]
        assert len(tris) == m
        cls, _p, _c = oracle.tri_classify(case["mov_xy"], tris, C.RADIUS, 15, case["type_id"])
        want = _window(f"edge/Tr={m}", "float64", oracle)[4]
        if m >= 255:
            assert set(np.unique(cls).tolist()) == {0, 1, 2, 3}
            assert want["kept"] > 0 and want["added"] > 0
    cls, _p, _c = oracle.tri_classify(case["mov_xy"], lists["all kept"], C.RADIUS, 15, case["type_id"])
    assert len(cls) == 16385 and not cls.any()
    want = _window("edge/all kept", "float64", oracle)[4]
    assert (want["kept"], want["added"]) == (16385, 0)
    cls, _p, _c = oracle.tri_classify(case["mov_xy"], lists["none kept"], C.RADIUS, 15, case["type_id"])
    assert len(cls) > 257 and cls.all() and set(np.unique(cls).tolist()) == {1, 2, 3}
    want = _window("edge/none kept", "float64", oracle)[4]
    assert want["kept"] == 0 and want["added"] > 256
    # the whole list crosses the look-back window of 64 scan blocks of 256
    assert F.EDGE_TRIANGLES[-1] > 64 * 256


@pytest.mark.parametrize("n", F.EDGE_NODES)
def test_one_type_sections_every_node_asks_and_a_triangle_comes_once(oracle, n):
    case, tris, filt, staged, want = _window(f"edge/n={n}", "float64", oracle)
    assert len(staged["rows"]) == n
    f = F.filter_statement(staged["xy"], case["type_id"], tris, filt, oracle)
    assert want["kept"] == 0 and not (f["cls"] == 0).any() and (f["cls"] == 3).any()
    valid = np.zeros(n, bool)
    valid[tris[f["cls"] == 3].reshape(-1)] = True
    assert np.array_equal(f["asks"], valid) and valid.sum() > 0.9 * n          # every node with a valid triangle asks
    # up to three nodes ask for a triangle, it comes once: fewer triangles than asking nodes, and none twice
    assert 0 < want["added"] < valid.sum() and len(np.unique(want["tris"], axis=0)) == want["added"]
    asked = np.bincount(f["best"][f["asks"]], minlength=len(tris))
    assert asked.max() >= 2 and (asked.max() == 3 or n < 1000)


@pytest.mark.parametrize("tag", [t for t in F.TAGS if t.startswith("lattice/one type")])
def test_lattice_has_equal_smallest_perimeters(oracle, tag):
    case, tris, filt, staged, want = _window(tag, "float64", oracle)
    f = F.filter_statement(staged["xy"], case["type_id"], tris, filt, oracle)
    assert want["added"] > 0 and f["fc_ties"] > 0
    shared = 0
    for v in np.flatnonzero(f["asks"]):
        mine = np.flatnonzero((f["cls"] == 3) & (tris == v).any(axis=1))
        equal = mine[f["perim"][mine] == f["perim"][mine].min()]
        assert f["best"][v] == equal[0]                                        # the first in input order
        shared += len(equal) > 1
    assert shared > 0


def test_order_ties_of_both_kinds_occur(oracle):
    fc = sc = 0
    for tag in F.TAGS:
        want = _window(tag, "float64", oracle)[4]
        if want["near"] == 0:
            fc += want["fc_ties"]
            sc += want["order_ties"] - want["fc_ties"]
    assert fc > 0 and sc > 0
    want = _window("lattice/one type/15", "float64", oracle)[4]
    assert want["fc_ties"] > 0 and want["order_ties"] > want["fc_ties"]


def test_knife_count_and_its_class_one_triangles(oracle):
    case, tris, filt, staged, want = _window("knife", "float64", oracle)
    cls, _p, maxcos = oracle.tri_classify(staged["xy"], tris, *filt[:2], case["type_id"])
    assert want["near"] == F.near_count(cls, maxcos, 45, oracle) > 0
    assert F.near_count(cls, maxcos, 45, oracle, class1_too=True) > want["near"]
    for angle in (15, 30):
        c2, _p, m2 = oracle.tri_classify(staged["xy"], tris, C.RADIUS, angle, case["type_id"])
        assert F.near_count(c2, m2, angle, oracle, class1_too=True) == 0


@pytest.mark.parametrize("rule", ["angle rule", "no angle rule"])
def test_degenerate_list(oracle, rule):
    case, tris, filt, staged, want = _window(f"degenerate/{rule}", "float64", oracle)
    xy = staged["xy"]
    repeated = (tris[:, 0] == tris[:, 1]) | (tris[:, 1] == tris[:, 2]) | (tris[:, 0] == tris[:, 2])
    p = xy[tris]
    area2 = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    assert repeated.sum() >= 100 and (~repeated & (area2 == 0)).sum() >= 100 and (area2 != 0).sum() >= 100
    cls, _p, maxcos = oracle.tri_classify(xy, tris, *filt[:2], case["type_id"])
    assert (maxcos[repeated] == 2.0).all()                                     # corner_cos's "angle 0"
    if rule == "angle rule":
        assert (cls[area2 == 0] != 0).all() and (cls[repeated] != 3).all()   # a degenerate triangle fails the angle test (or is too long)
    else:
        flat = np.flatnonzero((area2 == 0) & ((cls == 0) | (cls == 3)))
        assert len(flat) > 50
    # handed over as kept triangles: source sign 0, nothing of them checked, and their sign is in doubt
    full = F.of_case(case, staged, tris, filt, oracle, prefiltered=True)
    assert (full["signs"][area2 == 0] == 0).all() and full["stats"]["checked"] <= int((area2 != 0).sum())
    assert full["order_ties"] >= int((area2 == 0).sum()) - int(repeated.sum()) and full["fc_ties"] == 0


@pytest.mark.parametrize("n", F.MATCH_CELLS)
def test_matchings(oracle, n):
    case, tris, filt, staged, want = _window(f"match/{n}", "float64", oracle)
    assert n % 4 == F.MATCH_CELLS.index(n) + 1 and len(staged["pairs"]) == n * 2 * n and want["kept"] == len(tris) and want["added"] == 0
    assert len(np.unique(case["ref_xy"], axis=0)) == 2 * n - 2                 # duplicate coordinates in the reference
    out = {}
    for name in F.MATCHINGS:
        mp = F.matching(name, n, want["tris"], staged["pairs"], 2 * n)
        out[name] = F.of_case(case, staged, want["tris"], filt, oracle, prefiltered=True, match_pair=mp)
        assert out[name]["stats"]["greedy_rounds"] == 0
    s = out["none"]
    assert not s["flag"].any() and (s["row"] == -1).all() and set(s["stats"].values()) == {0}
    s = out["identity"]
    assert np.array_equal(s["row"], np.arange(n)) and 0 < s["stats"]["checked"] <= len(tris)
    s = out["mirror"]
    assert (s["flag"] == 3).all() and s["stats"]["flipped"] == s["stats"]["area_flips"] == s["stats"]["checked"] == len(tris)
    assert np.array_equal(s["row"], np.arange(n) + n)
    s = out["two on one"]
    c0, c1 = want["tris"][0][:2]
    both = (want["tris"] == c0).any(axis=1) & (want["tris"] == c1).any(axis=1)
    assert both.any() and s["stats"]["checked"] <= len(tris) - both.sum()      # a reference sign of 0: not checked
    assert s["order_ties"] >= both.sum() and s["row"][c0] == s["row"][c1] == c0
    s = out["one unmatched per triangle"]
    assert s["stats"]["checked"] == 0 and s["stats"]["area_flips"] == 0 and s["stats"]["xy_comparisons"] > 0
    assert 0 < s["stats"]["matched"] < n
    assert ((want["tris"][:, :, None] == np.flatnonzero(s["row"] < 0)[None, None, :]).any(axis=(1, 2))).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_takes_two_hundred_rounds(oracle, dtype):
    case, tris, filt, staged, want = _window("greedy/chain", dtype, oracle)
    assert len(staged["pairs"]) == 399 and len(np.unique(staged["costs"])) == 399
    assert want["stats"]["greedy_rounds"] == 200 >= 130 and want["stats"]["matched"] == 200
    # past 3 + 4 + 8 + 16 + 32 + 64: the batch stays at its maximum for at least one read
    assert want["stats"]["greedy_rounds"] > F.WINDOW_GREEDY_ROUNDS + 4 + 8 + 16 + 32 + F.GREEDY_BATCH_MAX
    assert want["kept"] == len(tris) > 0 and want["stats"]["xy_comparisons"] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_have_equal_costs_that_the_pair_index_decides(oracle, dtype):
    case, tris, filt, staged, want = _window("greedy/ties", dtype, oracle)
    costs = staged["costs"]
    assert len(np.unique(costs)) <= 3 and (costs == 3.0).sum() == 4 * len(staged["rows"])
    wrong = F.round_rule(staged["pairs"], costs, len(staged["rows"]), len(staged["rows_r"]), F.PENALTY * case["size"], tie="high")[0]
    assert not np.array_equal(wrong, want["match_pair"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_penalty_rows_on_above_and_below(oracle, dtype):
    case, tris, filt, staged, want = _window("greedy/penalty", dtype, oracle)
    n = len(staged["rows"])
    assert len(staged["pairs"]) == n and np.array_equal(staged["pairs"][:, 0], np.arange(n))
    costs, limit = staged["costs"], case["penalty"] * case["size"]
    ft = np.float64 if dtype == "float64" else np.float32
    on = costs == limit
    above = costs == np.nextafter(limit.astype(ft), ft(np.inf)).astype(np.float64)
    below = costs == np.nextafter(limit.astype(ft), ft(-np.inf)).astype(np.float64)
    assert on.any() and above.any() and below.any() and (on | above | below | (dtype == "float64")).all()
    for size in (1.0, 2.0, 1.5):                                               # integral sizes and a float one, on the penalty
        assert (on & (case["size"] == size)).any()
    assert np.array_equal(want["match_pair"] >= 0, costs < limit) and np.array_equal(costs < limit, below | ((costs < limit) & ~on & ~above))
    assert (want["match_pair"][on | above] == -1).all() and (want["match_pair"][below] >= 0).all()


def test_batch_windows(oracle):
    case = F.batch_section()
    assert len(case["boxes"]) == F.BATCH_WINDOWS == 9
    for w, box in enumerate(case["boxes"]):
        staged = F.cpu_staged(case, oracle, box=box)
        first = case["first"][w]
        last = case["first"][w + 1] if w + 1 < F.BATCH_WINDOWS else len(case["mov_xy"])
        assert np.array_equal(C.in_box(case["mov_xy"], box), np.arange(first, last)) and len(staged["rows_r"]) > 0
        if w == F.BATCH_NO_KEPT:
            assert len(staged["rows"]) == 0 and len(staged["pairs"]) == 0
            continue
        assert np.array_equal(staged["rows"], np.arange(first, last))
        want = F.of_case(case, staged, case["tris"][w], F.BATCH_FILTER, oracle)
        assert (want["near"] > 0) == (w == F.BATCH_KNIFE)
        assert (len(case["tris"][w]) == 0) == (w == F.BATCH_NO_TRIANGLES)
        if w not in (F.BATCH_KNIFE, F.BATCH_NO_TRIANGLES):
            assert want["kept"] > 0 and want["stats"]["matched"] > 0 and want["stats"]["checked"] > 0
        if w == F.BATCH_NO_TRIANGLES:
            assert want["stats"]["matched"] > 0 and want["stats"]["checked"] == 0 and not want["flag"].any()


# ---- a kernel wrong in one of these ways fails the GPU test: the wrong statement's answer is another one ----------------------------
WRONG = {"the last of equal perimeters": dict(pick="last"), "<= against the penalty": dict(strict=False),
         "an added triangle per asking node": dict(per_node=True), "cost ties to the higher pair index": dict(tie="high"),
         "a flag byte overwritten": dict(flags="overwrite"), "near over class-1 triangles too": dict(class1_too=True)}
CAUGHT_BY = {"the last of equal perimeters": ("lattice/one type/15", "lattice/one type/None"), "<= against the penalty": ("greedy/penalty",),
             "an added triangle per asking node": ("edge/n=257", "edge/Tr=257", "lattice/one type/15"),
             "cost ties to the higher pair index": ("greedy/ties", "lattice/two types/15"), "a flag byte overwritten": ("match/41", "match/42", "match/43"),
             "near over class-1 triangles too": ("knife",)}


@pytest.mark.parametrize("how", sorted(WRONG))
def test_wrong_statement_gives_another_answer(oracle, how):
    for tag in CAUGHT_BY[how]:
        for dtype in DTYPES:
            case, tris, filt, staged, want = _window(tag, dtype, oracle)
            more = {}
            if tag.startswith("match/"):          # the mirror matching: both kinds of writer at every cell
                more = dict(match_pair=F.matching("mirror", len(staged["rows"]), want["tris"], staged["pairs"], len(staged["rows_r"])))
            right = F.restated(case, staged, tris, filt, oracle, **more)
            wrong = F.restated(case, staged, tris, filt, oracle, **more, **WRONG[how])
            assert not F.same_answer(right, wrong), (how, tag, dtype)


# ---- the round rule is the reference's scan ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_round_rule_equals_the_oracle_on_random_pair_lists(oracle, seed):
    pairs, costs, n, n_r, size, penalty = F.random_pair_list(seed)
    want = F.oracle_greedy(pairs, costs, n, n_r, penalty, size, oracle)
    got, rounds = F.round_rule(pairs, costs, n, n_r, penalty * size)
    assert np.array_equal(got, want) and (rounds > 0) == (want >= 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", ["greedy/chain", "greedy/ties", "greedy/penalty"])
def test_round_rule_equals_the_oracle_on_the_greedy_families(oracle, tag, dtype):
    case, tris, filt, staged, want = _window(tag, dtype, oracle)
    n, n_r = len(staged["rows"]), len(staged["rows_r"])
    penalty = case.get("penalty", F.PENALTY)
    got, rounds = F.round_rule(staged["pairs"], staged["costs"], n, n_r, penalty * case["size"])
    assert np.array_equal(got, F.oracle_greedy(staged["pairs"], staged["costs"], n, n_r, penalty, case["size"], oracle))
    assert np.array_equal(got, want["match_pair"]) and rounds == want["stats"]["greedy_rounds"]
