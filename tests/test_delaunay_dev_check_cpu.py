"""tests/delaunay_dev_check.py without a GPU: every family has the property it was made for (no triangle in the band where numpy and
devmath.h could differ; neighbour, owner and hull counts on both sides of each capacity; the sparse family's grid doublings; the
host triangulator's answer at four times the guard for every family that must be answered and every ladder's top rung; the ladders'
rung 0 exactly degenerate), the statement is a statement of the reference's filter (the filter keeps over `candidates` what it keeps
over scipy's simplices), and the comparison rejects a kernel's answer that is wrong in each of five ways."""
import numpy as np
import pytest

import delaunay_dev_check as D

ANSWERABLE = D.MUST_ANSWER + D.CAPACITY_REFUSED + D.EITHER_NAMES
WINDOWED = tuple("w/" + name for name in D.WINDOW_NAMES)


def _filter_set(oracle, f, tris):
    kept = oracle.filter_triangles_by_radius(f["xy"], np.asarray(tris), f["radius"], min_angle_deg=f["angle"])
    return {tuple(sorted(int(v) for v in t)) for t in np.asarray(kept).reshape(-1, 3)}


@pytest.mark.parametrize("name", ANSWERABLE + WINDOWED)
def test_statement_is_in_the_calls_form_and_no_triangle_is_in_the_band(oracle, name):
    """band 0 at the family's own settings (the window section's copies: at every setting a window batch runs at); the statement's rows
    start with their smallest index, turn counter-clockwise, come by (owner, min, max) without repeats; the reference's filter keeps
    over them exactly what it keeps over scipy's simplices"""
    f = D.family(name)
    want = D.statement_of(name)
    assert D.band_of(name) == 0
    if name.startswith("w/"):
        assert [D.band_of(name, r, a) for r, a in D.WINDOW_SETTINGS] == [0, 0, 0]
    assert want.dtype == np.int32 and (want[:, 0] < want[:, 1:].min(axis=1)).all() and (D.area2(f["xy"], want) > 0).all()
    key = np.column_stack((want[:, 0], want[:, 1:].min(axis=1), want[:, 1:].max(axis=1))).astype(np.int64)
    flat = (key[:, 0] * len(f["xy"]) + key[:, 1]) * len(f["xy"]) + key[:, 2]
    assert (np.diff(flat) > 0).all()
    simplices = D.simplices_of(name)
    assert {tuple(sorted(r)) for r in want.tolist()} <= {tuple(sorted(r)) for r in simplices.tolist()}
    assert _filter_set(oracle, f, want) == _filter_set(oracle, f, simplices)
    assert np.array_equal(want, D.candidates(f["xy"], f["radius"], f["angle"]))          # (the cached simplices are scipy's of these points)


@pytest.mark.parametrize("name", D.MUST_ANSWER + tuple("w/" + n for n in D.MUST_ANSWER) + tuple(f"ladder/{w}/{len(D.LADDER_EPS) - 1}" for w in D.LADDERS))
def test_host_triangulator_answers_at_four_times_the_guard(name):
    """the condition of the ANSWER tag (and of a ladder's top rung): same_delaunay2d, which shares qhull_margin.h with the device, answers
    at 4 x GUARD -- and its triangles are scipy's"""
    from same_amd import delaunay

    f = D.family(name)
    assert D.expectation(name)[0] == D.ANSWER
    got = delaunay.native_simplices(f["xy"], guard=4 * delaunay.GUARD)
    assert got is not None
    assert {tuple(sorted(r)) for r in got.tolist()} == {tuple(sorted(r)) for r in D.simplices_of(name).tolist()}


def test_small_sets():
    for n in D.SMALL:
        f = D.family(f"small/{n}")
        assert len(f["xy"]) == n and len(D.hull_vertices(f["xy"])) == f["corners"] == (n if n <= 4 else n - 1)
        assert len(D.statement_of(f"small/{n}")) == len(D.simplices_of(f"small/{n}")) == 2 * n - 2 - f["corners"]
        assert np.abs(f["xy"] - D.CENTRE).max() < 12
    s2, _c = D.sides2_maxcos(D.family("small/3")["xy"], [[0, 1, 2]])
    assert (np.abs(np.sqrt(s2) - 10.0) < 2.0).all()


def test_edge_sets_sit_on_the_scan_block():
    assert D.SCAN_NT == 256 and D.EDGES == (255, 256, 257, 513)
    for n in D.EDGES:
        assert len(D.family(f"edges/{n}")["xy"]) == n
    f = D.family("edges/cells256")
    nx, ny, _cw, doublings = D.grid_of(f["xy"], f["radius"])
    assert (nx, ny, doublings) == (16, 16, 0) and nx * ny == D.SCAN_NT
    for name in ("edges/cells256", "w/edges/cells256"):
        assert D.grid_of(D.family(name)["xy"], 25.0)[:2] == (16, 16)


def test_sparse_set_doubles_its_grid():
    """the kernel's own rule: floor(ext / cw) + 1 cells per axis against 2 n + 64"""
    for name in ("sparse", "w/sparse"):
        f = D.family(name)
        ext = f["xy"].max(axis=0) - f["xy"].min(axis=0)
        cw = f["radius"] * (1.0 + 1e-6)
        assert (np.floor(ext[0] / cw) + 1) * (np.floor(ext[1] / cw) + 1) > 2 * len(f["xy"]) + 64
        nx, ny, width, doublings = D.grid_of(f["xy"], f["radius"])
        assert doublings == 4 and abs(width - 192.0) < 1e-3 and nx * ny <= 2 * len(f["xy"]) + 64
        assert len(D.statement_of(name)) == 238
    for name in ("hull1024", "hull1025"):           # (so do the hull sets, twice)
        assert D.grid_of(D.family(name)["xy"], 25.0)[3] == 2


def test_strip_is_one_row_of_cells():
    f = D.family("strip")
    assert len(f["xy"]) == 600 and D.grid_of(f["xy"], f["radius"])[:2] == (240, 1)
    assert D.grid_of(D.family("w/strip")["xy"], 25.0)[1] == 1


@pytest.mark.parametrize("prefix", ["", "w/"])
def test_capacity_pairs_stand_on_both_sides(prefix):
    lo, hi = D.family(prefix + "nb128"), D.family(prefix + "nb129")
    for f, n in ((lo, 128), (hi, 129)):
        d = f["xy"][:, None, :] - f["xy"][None, :, :]
        assert np.sqrt((d * d).sum(-1)).max() < 24.0 and len(f["xy"]) == n + 1
        nb = D.neighbours_above(f["xy"], f["radius"])
        assert nb[0] == n == nb.max() and (nb[1:] < n).all()
    assert D.owner_counts(D.statement_of(prefix + "nb128"), 129).max() == 7 and D.owner_counts(D.statement_of(prefix + "nb129"), 130).max() <= D.OWN_CAP
    assert np.array_equal(lo["xy"] - lo["xy"][0], hi["xy"][:-1] - hi["xy"][0])            # one point more, nothing else
    for name, n in ((prefix + "own32", 32), (prefix + "own33", 33)):
        f, want = D.family(name), D.statement_of(name)
        assert len(want) == n == len(D.simplices_of(name)) and (want[:, 0] == 0).all()          # all pass the screen, all owned by point 0
        assert D.owner_counts(want, n + 1)[0] == n and D.neighbours_above(f["xy"], f["radius"]).max() == n <= D.NB_CAP
    assert 360.0 / 33 > 10.9 > 10.0
    for name, n in ((prefix + "hull1024", 1024), (prefix + "hull1025", 1025)):
        f, want = D.family(name), D.statement_of(name)
        hull = D.hull_vertices(f["xy"])
        assert len(hull) == n and hull.min() == D.HULL_INNER and len(f["xy"]) == D.HULL_INNER + n
        assert len(want) > 1000 and want.max() < D.HULL_INNER                                  # no ring point in a triangle that passes the screen
        assert D.neighbours_above(f["xy"], f["radius"]).max() < D.NB_CAP and D.owner_counts(want, len(f["xy"])).max() < D.OWN_CAP
    assert (D.expectation("nb128"), D.expectation("own32"), D.expectation("hull1024")) == ((D.ANSWER, 0),) * 3
    assert (D.expectation("nb129"), D.expectation("own33"), D.expectation("hull1025")) == ((D.REFUSE, D.OVERFLOW),) * 3


def test_no_other_answerable_family_is_near_a_capacity():
    for name in D.MUST_ANSWER + D.EITHER_NAMES:
        if name in ("nb128", "own32", "hull1024"):
            continue
        f = D.family(name)
        assert D.neighbours_above(f["xy"], f["radius"]).max() < D.NB_CAP - 20, name
        assert D.owner_counts(D.statement_of(name), len(f["xy"])).max() < D.OWN_CAP - 10, name
        assert len(D.hull_vertices(f["xy"])) < 64, name


def test_negative_sets_straddle_zero_and_sit_on_cell_boundaries():
    for name in ("negative/uniform", "negative/cluster"):
        xy = D.family(name)["xy"]
        assert (xy.min(axis=0) < -100).all() and (xy.max(axis=0) > 100).all()
    f = D.family("negative/cluster")
    xy, (x0, y0), cw = f["xy"], f["corner"], f["cw"]
    assert tuple(xy.min(axis=0)) == (x0, y0) and cw == 25.0 * (1.0 + 1e-6) == D.grid_of(xy, 25.0)[2]
    on = xy[-len(D.ON_CELL_EDGES):]
    for (a, b), p in zip(D.ON_CELL_EDGES, on):
        assert a is None or p[0] == x0 + a * cw
        assert b is None or p[1] == y0 + b * cw
    assert sum(a is not None for a, _b in D.ON_CELL_EDGES) >= 4 and sum(b is not None for _a, b in D.ON_CELL_EDGES) >= 4


def test_nonfinite_sets():
    base = D.uniform(257, 3257)
    for how in D.NONFINITE_HOW:
        f = D.family(f"nonfinite/{how}")
        bad = ~np.isfinite(f["xy"])
        assert D.expectation(f"nonfinite/{how}") == (D.REFUSE, D.NONFINITE)
        assert bad.all() if how == "all nan" else (bad.sum() == 1 and np.array_equal(f["xy"][~bad], base[~bad]))
    assert np.isnan(D.family("nonfinite/nan first")["xy"][0]).any() and np.isnan(D.family("nonfinite/nan last")["xy"][-1]).any()
    assert np.isposinf(D.family("nonfinite/+inf")["xy"]).any() and np.isneginf(D.family("nonfinite/-inf")["xy"]).any()


def test_ladders_start_exactly_degenerate_and_open():
    assert D.LADDER_EPS[0] == 0.0 and D.LADDER_EPS[1] == 1e-15 and D.LADDER_EPS[-1] == 1e-3 and len(D.LADDER_EPS) == 14
    for which in D.LADDERS:
        assert D.expectation(f"ladder/{which}/0") == (D.REFUSE, D.IN_DOUBT)
        assert D.expectation(f"ladder/{which}/{len(D.LADDER_EPS) - 1}") == (D.ANSWER, 0)
        assert all(D.expectation(f"ladder/{which}/{r}") == (D.EITHER, D.IN_DOUBT) for r in range(1, len(D.LADDER_EPS) - 1))
        assert all(len(D.family(f"ladder/{which}/{r}")["xy"]) > D.LADDER_GENERIC for r in range(len(D.LADDER_EPS)))
    # (a) the rectangle at rung 0: whole corners, exactly cocircular by integer arithmetic, nothing else in or on the circle
    xy = D.family("ladder/rectangle/0")["xy"]
    corners = [(int(x), int(y)) for x, y in xy[-4:]]
    assert np.array_equal(xy[-4:], np.asarray(corners, np.float64))
    (ax, ay), (bx, by), (cx, cy), (dx, dy) = corners
    rows = [[px - dx, py - dy, (px - dx) ** 2 + (py - dy) ** 2] for px, py in ((ax, ay), (bx, by), (cx, cy))]
    det = (rows[0][0] * (rows[1][1] * rows[2][2] - rows[1][2] * rows[2][1]) - rows[0][1] * (rows[1][0] * rows[2][2] - rows[1][2] * rows[2][0])
           + rows[0][2] * (rows[1][0] * rows[2][1] - rows[1][1] * rows[2][0]))
    assert isinstance(det, int) and det == 0
    assert np.hypot(*(xy[:-4] - (103.0, 104.0)).T).min() > 9.0 > 5.0
    top = D.family(f"ladder/rectangle/{len(D.LADDER_EPS) - 1}")["xy"]
    assert np.hypot(*(top[-2] - (103.0, 104.0))) > 5.0 and np.array_equal(np.delete(top, -2, axis=0), np.delete(xy, -2, axis=0))
    # (b) the duplicate at rung 0: two identical rows
    xy = D.family("ladder/duplicate/0")["xy"]
    assert np.array_equal(xy[-1], xy[D.DUPLICATED]) and len(np.unique(xy, axis=0)) == len(xy) - 1
    assert len(np.unique(D.family("ladder/duplicate/13")["xy"], axis=0)) == len(xy)
    # (c) three hull points on a line with whole coordinates
    xy = D.family("ladder/hull line/0")["xy"]
    assert np.array_equal(xy[-3:], D.HULL_LINE) and (xy[:-3, 1] > 0).all() and (D.HULL_LINE[:, 1] == -6).all()
    assert xy[-2, 1] > D.family("ladder/hull line/13")["xy"][-2, 1]
    assert len(xy) - 2 in D.hull_vertices(D.family("ladder/hull line/13")["xy"])


def test_small_angles_are_the_uniform_family():
    for a in D.SMALL_ANGLES:
        f = D.family(f"angle/{a}")
        assert f["angle"] == a and len(f["xy"]) == 1000 and D.expectation(f"angle/{a}") == (D.EITHER, D.OVERFLOW)


def test_window_section_holds_the_families_apart():
    """whole-number moves, every family alone in its box, the extent under 20 000, every row but the `no cell` ones kept (the reference
    is the point itself), windows of exactly 0, 2 and 3 cells"""
    import caller_check as C

    sec = D.window_section()
    assert sec["mov_xy"].min() >= 0 and sec["mov_xy"].max() < 20000 and sec["ref_xy"].max() < 20000
    for w, name in enumerate(sec["names"]):
        rows = C.in_box(sec["mov_xy"], sec["boxes"][w])
        assert np.array_equal(rows, np.arange(sec["first"][w], sec["first"][w + 1])), name
        if name in D.WINDOW_NAMES:
            f, g = D.family(name), D.family("w/" + name)
            move = g["xy"] - f["xy"]
            assert np.array_equal(sec["mov_xy"][rows], g["xy"])
            assert np.abs(move - np.round(move[0])).max() < 1e-9                  # one whole-number move (up to the sum's rounding)
            assert np.array_equal(sec["ref_xy"][rows], g["xy"])
    sizes = dict(zip(sec["names"], np.diff(sec["first"]).tolist()))
    assert sizes[D.PAIR] == 2 and sizes["small/3"] == 3 and sizes[D.NO_CELL] == 5
    lone = np.arange(sec["first"][-2], sec["first"][-1])
    d = sec["mov_xy"][lone][:, None, :] - sec["ref_xy"][None, :, :]
    assert np.abs(d).sum(-1).min() > 2 * D.WINDOW_RADIUS                       # no reference within the radius: no kept cell
    assert len(C.in_box(sec["ref_xy"], sec["boxes"][-1])) == 5


def test_batch_section():
    sec = D.batch_section()
    assert len(sec["names"]) == D.WINDOW_BATCH_MAX == 64 and D.LAUNCH_WINDOWS == 8
    assert all((n == 2) == (w % 3 == 2) and (n == 2 or 50 <= n <= 300) for w, n in enumerate(sec["sizes"]))
    for w, n in enumerate(sec["sizes"]):
        xy = sec["mov_xy"][sec["first"][w]:sec["first"][w + 1]]
        assert len(xy) == n
        if n > 2:                                  # must be answered: the band, the host at four times the guard, no capacity near
            assert D.band(xy, 25.0, 15.0) == 0 and D.host_answers(xy) and D.neighbours_above(xy, 25.0).max() < D.NB_CAP - 20, w


# ---- the comparison itself -------------------------------------------------------------------------------------------------------------
def test_comparison_rejects_each_wrong_answer():
    name = "edges/257"
    f, want = D.family(name), D.statement_of(name)
    D.same_candidates(want.copy(), want)
    assert D.difference(want.copy(), want) is None

    def broke(got, what):
        assert D.difference(got, want) == what
        with pytest.raises(AssertionError, match=what):
            D.same_candidates(got, want)

    swapped = want.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    broke(swapped, "the row order")
    clockwise = want.copy()
    clockwise[5] = clockwise[5][[0, 2, 1]]
    broke(clockwise, "the orientation")
    rotated = want.copy()
    rotated[7] = rotated[7][[1, 2, 0]]
    broke(rotated, "the owner-first rule")
    broke(np.delete(want, 20, axis=0), "the set")
    # a triangle that passes the screen and is not Delaunay: two neighbouring triangles' shared edge flipped
    from scipy.spatial import Delaunay

    tri = Delaunay(f["xy"])
    have = {tuple(sorted(r)) for r in want.tolist()}
    for s, nbrs in enumerate(tri.neighbors):
        for k, o in enumerate(nbrs):
            if o < 0:
                continue
            a = int(tri.simplices[s][k])
            b = int(next(v for v in tri.simplices[o] if v not in tri.simplices[s]))
            for c in (int(v) for v in tri.simplices[s] if v != a):
                flipped = np.array([[a, b, c]])
                if D.passes_screen(f["xy"], flipped, f["radius"], f["angle"]).all() and tuple(sorted((a, b, c))) not in have:
                    added = D.in_call_order(f["xy"], np.vstack((want, flipped)))
                    assert len(added) == len(want) + 1
                    broke(added, "the set")
                    return
    raise AssertionError("no flipped triangle passes the screen")


def test_comparison_rejects_an_answer_of_another_type():
    want = D.statement_of("small/5")
    assert D.difference(want.astype(np.int64), want) == "the type"
    assert D.difference(want[:, :2], want) == "the type"
    assert D.difference(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32)) is None
