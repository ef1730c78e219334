"""tests/staged_check.py without a GPU: each statement tests/test_gpu_staged_library.py holds a kernel against equals what the project
already trusts on every family (the oracle's `_mc_valid`, `window_mask`, `eager_signs`; for the disjoint scan a second, differently written
loop and the kernels' own local-minimum rule); each family has the property it was made for; and four planted wrong kernels differ from
the statements exactly where the families were made to catch them."""
import numpy as np
import pytest

import staged_check as S


def _same(got, want):
    """bit-for-bit, NaN equal to NaN"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def _differing(families, wrong, right):
    """the names of the families in which some case's `wrong` differs from its `right`"""
    return {family for family, cases in families if any(not _same(wrong(case), right(case)) for _name, case in cases)}


# ---- the statements against what the project trusts -----------------------------------------------------------------------------------------
def test_collapse_validity_equals_the_oracles_mc_valid_on_every_family(oracle):
    for name, case in S.flat(S.collapse_families()):
        flag, perim, total = S.host_collapse(case)
        with np.errstate(all="ignore"):
            want = [oracle._mc_valid(case.xy[tri], case.r_max, case.min_angle_deg) for tri in case.tris]
        assert (flag & 1).astype(bool).tolist() == want, name
        assert not ((flag >> 1) & ~flag & 1).any() and flag.max(initial=0) <= 3, name              # a candidate is valid
        assert perim.dtype == total.dtype == np.float64


def test_the_disjoint_scan_equals_a_second_loop_and_the_local_minimum_rule():
    """the second loop: take the smallest (key, index) among the items left, drop every item that shares a vertex with it, repeat"""
    for name, case in S.flat(S.disjoint_families()):
        want = S.host_disjoint(case)
        left, second = list(range(len(case.items))), np.zeros(len(case.items), bool)
        sets = [set(map(int, it)) for it in case.items]
        while left:
            m = min(left, key=lambda q: (case.keys[q], q))             # tuples compare the keys with ==: the two zeros tie
            second[m] = True
            left = [q for q in left if not (sets[q] & sets[m])]
        assert np.array_equal(want, second), name
        selected, rounds = S.local_minimum_rounds(case)
        assert np.array_equal(want, selected) and (rounds > 0) == (len(case.items) > 0), name
        assert not np.isnan(case.keys).any() and case.items.min() >= 0 and case.items.max() < case.n_nodes, name


def test_the_window_mask_equals_the_oracles_box_by_box(oracle):
    for name, case in S.flat(S.window_families()):
        mask = S.host_window_mask(case)
        assert mask.shape == (len(case.boxes), len(case.xy)) and mask.dtype == bool
        for b in range(0, len(case.boxes), 1 if len(case.boxes) < 50 else 37):
            assert np.array_equal(mask[b], oracle.window_mask(case.xy, *case.boxes[b])), (name, b)


def test_eager_signs_equal_the_oracles(oracle):
    for name, case in S.flat(S.eager_families()):
        want = oracle.eager_signs(case.rxy, case.tris, case.cand)
        assert _same(S.host_eager_signs(case), want), name


# ---- each family has its property -----------------------------------------------------------------------------------------------------------
def test_the_geometry_is_exact_before_every_sqrt_and_division():
    for name, case in S.flat(S.collapse_families()):
        assert S.geometry_is_exact(case.xy, case.tris), name
    assert not S.geometry_is_exact(np.array([(0, 0), (0.5, 0), (0, 1)]), [(0, 1, 2)])
    assert not S.geometry_is_exact(np.array([(0, 0), (2**21, 0), (0, 1)]), [(0, 1, 2)])
    rounding = S.rounding_points()[0][1]
    head = rounding.tris[:len(S.ROUNDING_Y)]
    cross = S.cross_product(*(rounding.rxy[head[:, q]] for q in range(3)))
    assert _same(cross, np.array(S.ROUNDING_Y)) and np.array_equal(np.signbit(cross), np.signbit(S.ROUNDING_Y))    # the cross is y, bit for bit


def test_collapse_families_have_both_answers_where_they_were_made_to():
    fam = dict(S.collapse_families())
    assert [len(case.tris) for _n, case in fam["collapse_sizes"]] == list(S.COLLAPSE_SIZES)
    for _name, case in fam["collapse_sizes"][1:]:
        flag = S.host_collapse(case)[0]
        assert {0, 1, 3} <= set(flag.tolist())
    # zero sides at 10 degrees: (a, a, b) valid, (a, b, b) invalid, (a, b, a) valid, (a, a, a) valid; r_max 4 < |ab| = 5 takes all but (a, a, a)
    zero = {name: (S.host_collapse(case)[0] & 1).tolist() for name, case in fam["zero_sides"]}
    assert zero == {"r_max None": [1, 0, 1, 1], "r_max 10.0": [1, 0, 1, 1], "r_max 5.0": [1, 0, 1, 1], "r_max 4.0": [0, 0, 0, 1]}
    col = {name: (S.host_collapse(case)[0] & 1) for name, case in fam["collinear"]}
    assert not col["min_angle_deg 10"].any() and col["min_angle_deg 0"].all() and 0 < col["min_angle_deg None"].sum() < 18
    # an edge exactly r_max long is valid, one float more than r_max is not
    rmax = {case.r_max: S.host_collapse(case)[0] & 1 for _n, case in fam["rmax_edges"] if case.r_max is not None and case.r_max == case.r_max}
    iso, tri345 = slice(6, 12), slice(0, 6)
    hyp = float(np.sqrt(72.0))
    assert rmax[30.0].all() and not rmax[float(np.nextafter(30.0, 0.0))][tri345].any() and rmax[float(np.nextafter(30.0, 0.0))][iso].all()
    assert rmax[hyp][iso].all() and not rmax[float(np.nextafter(hyp, 0.0))].any() and not rmax[0.0].any() and rmax[S.INF].all()
    assert all((S.host_collapse(case)[0] & 1).all() for _n, case in fam["rmax_edges"] if case.r_max is None or case.r_max != case.r_max)
    # corner angles on and beside 45 degrees: the three thresholds around 45 do not all answer alike, and the infinite thresholds answer as one
    ang = {case.min_angle_deg: S.host_collapse(case)[0] & 1 for _n, case in fam["angle_edges"]}
    below, above = float(np.nextafter(45.0, 0.0)), float(np.nextafter(45.0, 90.0))
    assert ang[None].all() and ang[0].all() and not ang[181].any() and not ang[180].any()
    assert 0 < ang[above].sum() < ang[45].sum() <= ang[below].sum() < len(ang[45])
    assert [m for m in S.MIN_ANGLES if m is not None] == sorted(m for m in S.MIN_ANGLES if m is not None)
    # non-finite corners under r_max: both answers among the NaN corners
    nonfinite = S.host_collapse(fam["nonfinite_corners"][0][1])[0] & 1
    has_nan = np.isnan(fam["nonfinite_corners"][0][1].xy).any(axis=1).reshape(-1, 3).any(axis=1)
    assert 0 < nonfinite[has_nan].sum() < has_nan.sum()
    # the size rule: 3 is a candidate at max_size 3, the float after 3 is not, a NaN total is, and so is everything under a NaN max_size
    rules = dict(fam["size_and_type_rules"])
    flag, _perim, total = S.host_collapse(rules["max_size 3.0"])
    assert (flag & 1).all()
    assert total[0] == 3.0 and total[1] == total[2] == np.nextafter(3.0, 4.0) and np.isnan(total[3]) and np.isnan(total[18])
    assert (flag >> 1).tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1]
    nan_max = S.host_collapse(rules["max_size nan"])[0] >> 1
    assert nan_max.tolist() == [1] * 10 + [0, 0, 0, 1, 0, 1, 1, 1, 1]
    assert len(rules["max_size 3.0"].xy) > rules["max_size 3.0"].tris.max() + 1


def test_disjoint_families_have_their_properties():
    fam = dict(S.disjoint_families())
    assert [len(case.items) for _n, case in fam["disjoint_sizes"]] == list(S.SIZES)
    for _name, case in fam["disjoint_sizes"][3:]:
        assert len(np.unique(case.keys)) < len(case.keys) / 2                                          # heavy ties
    even = np.arange(S.CHAIN) % 2 == 0
    for name, case in fam["chain"]:
        selected, rounds = S.local_minimum_rounds(case)
        assert rounds == S.CHAIN // 2 == 300, name                                               # a round per item taken
        assert np.array_equal(selected, ~even if name == "falling" else even), name
    for name, case in fam["star"]:
        selected, rounds = S.local_minimum_rounds(case)
        first = {"distinct keys": int(np.argmin(case.keys)), "equal keys": 0, "three equal smallest": 70}[name]
        assert rounds == 1 and np.flatnonzero(selected).tolist() == [first], name
    selected, rounds = S.local_minimum_rounds(fam["disjoint_items"][0][1])
    assert rounds == 1 and selected.all()
    repeated = fam["repeated_vertex"][0][1].items
    assert all(((repeated[:, i] == repeated[:, j]) & (repeated[:, i] != repeated[:, 3 - i - j])).any() for i, j in ((0, 1), (0, 2), (1, 2)))
    assert (repeated.max(axis=1) == repeated.min(axis=1)).any()
    many, tight = (case for _n, case in fam["many_nodes"])
    assert many.n_nodes == 100_000 and many.items.max() == 99_999 and many.items.min() > 99_000 and tight.n_nodes == tight.items.max() + 1
    keys = fam["extreme_keys"][0][1].keys
    assert np.isposinf(keys).any() and np.isneginf(keys).any() and (np.abs(keys[keys != 0]) < 2.3e-308).any()
    assert (keys == 0).any() and not np.signbit(keys[keys == 0]).any()
    for _name, case in fam["two_zeros"]:
        zero = case.keys == 0
        assert np.signbit(case.keys[zero]).any() and not np.signbit(case.keys[zero]).all()
    assert np.flatnonzero(S.host_disjoint(fam["two_zeros"][0][1])).tolist() == [0]


def test_window_families_have_their_properties():
    fam = dict(S.window_families())
    assert sorted({len(case.xy) for _n, case in fam["window_sizes"]}) == list(S.WINDOW_SIZES)
    assert sorted({len(case.boxes) for _n, case in fam["window_sizes"]}) == list(S.BOX_COUNTS)
    for name, case in fam["window_sizes"]:
        mask = S.host_window_mask(case)
        assert mask[:, 0].all(), name                                                   # row 0 lies inside every box
        assert len(case.xy) < 4 or 0 < mask.sum() < mask.size, name
    edges = fam["window_edges"][0][1]
    mask = S.host_window_mask(edges)
    at = lambda x, y: int(np.flatnonzero((edges.xy[:, 0] == x) & (edges.xy[:, 1] == y) & ~((edges.xy == 0) & np.signbit(edges.xy)).any(axis=1))[0])
    below = float(np.nextafter(10.0, 0.0))
    plain = mask[0]
    assert plain[at(0, 5)] and plain[at(5, 0)] and plain[at(0, 0)] and plain[at(below, below)]      # on x0, on y0, inside x1 and y1 by one float
    assert not plain[at(10, 5)] and not plain[at(5, 10)] and not plain[at(10, 10)]                # on x1, on y1
    assert not mask[1:6].any()                                                          # x0 == x1, y0 == y1, inverted in x, in y, in both
    everything = mask[6]
    assert everything[at(-S.INF, -S.INF)] and not everything[at(S.INF, 5)] and not everything[at(5, S.INF)] and everything[at(-3, -3)]
    assert not mask[8:15].any()                                                         # empty infinite boxes, NaN bounds
    assert not mask[:, np.isnan(edges.xy).any(axis=1)].any()                            # NaN points are in no box
    assert np.array_equal(mask[16], mask[0])                                            # -0.0 bounds are 0.0 bounds


def test_eager_families_have_their_properties():
    fam = dict(S.eager_families())
    totals = [len(case.tris) * case.cand.shape[1] ** 3 for _n, case in fam["eager_sizes"]]
    assert {1, 255, 256, 257} <= set(totals) and max(totals) > 4000 and {case.cand.shape[1] for _n, case in fam["eager_sizes"]} == {1, 2, 3, 5}
    for (k, _tr), (_name, case) in zip(S.EAGER_SIZES, fam["eager_sizes"]):
        out = S.host_eager_signs(case)
        assert out.shape == (len(case.tris), k, k, k)
        if len(case.tris) > 8:
            assert {-1, 0, 1} <= set(out.reshape(-1).tolist()) and (k == 1) != (2 in out)
        if k == 1:
            assert np.array_equal(case.cand[:, 0], np.arange(len(case.cand)))
    missing = fam["missing_candidates"][0][1]
    out = S.host_eager_signs(missing)
    for t, (a, b, c) in enumerate(missing.tris):          # the layout ((t * k + x) * k + y) * k + z, entry by entry
        for x in range(3):
            for y in range(3):
                for z in range(3):
                    unknown = min(missing.cand[a, x], missing.cand[b, y], missing.cand[c, z]) < 0
                    assert (out.reshape(-1)[((t * 3 + x) * 3 + y) * 3 + z] == 2) == unknown
    assert (out[missing.tris[:, 1] == 5] == 2).all() and all((missing.cand[:5, z] == -1).any() for z in range(3))
    rounding = S.host_eager_signs(S.rounding_points()[0][1]).reshape(-1)
    by_y = dict(zip(map(repr, S.ROUNDING_Y), rounding.tolist()))
    assert {-1, 0, 1} <= set(by_y.values()) and by_y["0.0004"] == 0 and by_y["nan"] == 0 and by_y["1e-320"] == 0 and by_y["0.0015"] == 1
    assert rounding[len(S.ROUNDING_Y):].tolist() == [1, -1, 0, -1]                                   # +inf, -inf, inf - inf, -inf
    orders = S.host_eager_signs(S.vertex_orders()[0][1]).reshape(-1)
    assert orders[:6].tolist() == [S.order_parity(o) for o in S.ORDERS] and not orders[6:].any()


# ---- planted wrong kernels are caught ---------------------------------------------------------------------------------------------------------
def test_a_pairwise_max_differs_on_the_nan_corners_and_nowhere_else():
    families = S.collapse_families()
    wrong = _differing(families, lambda case: S.host_collapse(case, S.pairwise_max)[0], lambda case: S.host_collapse(case)[0])
    assert wrong == {"nonfinite_corners"}
    case = dict(families)["nonfinite_corners"][0][1]
    differ = S.host_collapse(case, S.pairwise_max)[0] != S.host_collapse(case)[0]
    nan_corner = np.isnan(case.xy).any(axis=1).reshape(-1, 3)
    of_nan = differ & nan_corner.any(axis=1)                 # the others: two corners at one infinity, whose edge is inf - inf = NaN
    assert of_nan.any() and not nan_corner[of_nan][:, 0].any() and nan_corner[of_nan][:, 1].any() and nan_corner[of_nan][:, 2].any()
    assert set((S.host_collapse(case)[0][of_nan] & 1).tolist()) == {0, 1}                         # wrong each way round


def test_a_sign_ordered_key_differs_on_the_two_zeros_and_nowhere_else():
    wrong = _differing(S.disjoint_families(), lambda case: S.local_minimum_rounds(case, S.sign_ordered)[0], S.host_disjoint)
    assert wrong == {"two_zeros"}
    star = dict(S.disjoint_families())["two_zeros"][0][1]
    assert np.flatnonzero(S.local_minimum_rounds(star, S.sign_ordered)[0]).tolist() == [1]


def test_a_count_over_padded_lanes_differs_on_the_sizes():
    for name, case in dict(S.window_families())["window_sizes"]:
        excess = S.padded_counts(case) - S.host_window_mask(case).sum(axis=1)
        assert (excess == -len(case.xy) % 256).all() and (excess > 0).all() == (len(case.xy) != 256), name


def test_rounding_half_up_differs_on_the_rounding_points():
    wrong = _differing(S.eager_families(), lambda case: S.host_eager_signs(case, S.round_half_up), S.host_eager_signs)
    assert wrong == {"rounding_points"}
    case = S.rounding_points()[0][1]
    differ = (S.host_eager_signs(case, S.round_half_up) != S.host_eager_signs(case)).reshape(-1)
    ys = [y for y, d in zip(S.ROUNDING_Y, differ) if d]
    assert 0.0005 in ys or 0.0025 in ys, ys                                    # a tie at a half, which rint takes to the even side


@pytest.mark.parametrize("names", [("collapse_families", S.Collapse), ("disjoint_families", S.Disjoint), ("window_families", S.Windows),
                                   ("eager_families", S.Eager)])
def test_the_families_are_the_same_on_every_call(names):
    """seeded: a second call gives the same bits, so the GPU module and this one run the same inputs"""
    maker, kind = names
    for (name, a), (_n, b) in zip(S.flat(getattr(S, maker)()), S.flat(getattr(S, maker)())):
        assert isinstance(a, kind)
        for u, v in zip(a, b):
            assert (u is None and v is None) or np.array_equal(np.asarray(u), np.asarray(v), equal_nan=np.asarray(u).dtype.kind == "f"), name
