"""The host statement of same_delaunay_filtered / same_window_delaunay (csrc/delaunay_dev.hip) and the point sets its library-level
tests run it on.

`candidates` is the call's whole answer when it answers: scipy's Delaunay triangles that pass the slack screen of the filter (every
squared side below (radius (1 + 1e-9))^2, the largest corner cosine below the threshold + 1e-9), each starting with its smallest index
(its owner), counter-clockwise, sorted by (owner, the smaller of the other two, the larger) -- array equal, not set equal.  `band` counts
the triangles a difference of expression between numpy and devmath.h could decide (a longest side within 1e-6 radius of the radius, a
largest cosine within 1e-6 of the threshold): every family that can be answered has none.  `same_candidates` is the comparison the GPU
test makes, and says what broke: the set, the orientation, the owner-first rule or the row order.

The families are cached and frozen as tests/caller_check.py's are, and tagged with what must happen to them: ANSWER (status 0, the
output equal to `candidates`), REFUSE with a bit of SAME_DD_* (SAME_OK, the bit in the status, no triangle), or EITHER with a bit (a
refusal may carry that bit only, an answer must equal `candidates`).  A family is tagged ANSWER only if the host triangulator, which
shares csrc/qhull_margin.h with the device, answers it at FOUR times the guard (`host_answers`): the factor is room for the device's own
extra rules (its determinant rounding bound, the hull-edge rule) and nobody has measured it.  tests/test_delaunay_dev_check_cpu.py
checks, without a GPU, that each family has the property it was made for; tests/test_gpu_delaunay_library.py drives the library on
them.  Not collected by pytest."""
import functools

import numpy as np

import caller_check as C

SLACK, BAND = 1e-9, 1e-6
NB_CAP, OWN_CAP, SURV_CAP, SCAN_CELLS_CAP, SCAN_NT = 128, 32, 1024, 256, 256      # csrc/delaunay_dev.hip, csrc/scan.h
LAUNCH_WINDOWS, WINDOW_BATCH_MAX = 8, 64                                           # csrc/common.h, include/same_hip.h
FEW_POINTS, NO_ANGLE, NONFINITE, IN_DOUBT, OVERFLOW = 1, 2, 4, 8, 16               # SAME_DD_*
ANSWER, REFUSE, EITHER = "answer", "refuse", "either"
DENSITY = 0.01                                                                     # cfg 5's: cells per unit area


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def _threshold(min_angle_deg):
    from same_amd.triangles import cos_threshold

    return cos_threshold(min_angle_deg)[1]


def _tris(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(-1, 3))


def sides2_maxcos(xy, tri):
    """-> (squared sides (T, 3), largest corner cosine (T,)) of the triangles `tri` over `xy`"""
    p = np.asarray(xy, np.float64)[np.asarray(tri, np.int64).reshape(-1, 3)]
    v1, v2 = p[:, [1, 2, 0]] - p, p[:, [2, 0, 1]] - p
    s2 = (v1 * v1).sum(-1)
    cos = (v1 * v2).sum(-1) / np.sqrt(s2 * (v2 * v2).sum(-1))
    return s2, cos.max(axis=1)


def area2(xy, tri):
    p = np.asarray(xy, np.float64)[np.asarray(tri, np.int64).reshape(-1, 3)]
    return (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])


def scipy_simplices(xy):
    from scipy.spatial import Delaunay

    return Delaunay(np.asarray(xy, np.float64)).simplices


def passes_screen(xy, tri, radius, min_angle_deg):
    s2, maxcos = sides2_maxcos(xy, tri)
    return (s2 < (radius * (1.0 + SLACK)) ** 2).all(axis=1) & (maxcos < _threshold(min_angle_deg) + SLACK)


def in_call_order(xy, tri):
    """the triangles `tri` as the call emits them: smallest index first, counter-clockwise, rows by (first, min, max of the other two)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    tri = np.take_along_axis(tri, (tri.argmin(axis=1)[:, None] + np.arange(3)[None, :]) % 3, axis=1)
    clockwise = area2(xy, tri) < 0
    tri[clockwise] = tri[clockwise][:, [0, 2, 1]]
    return _tris(tri[np.lexsort((tri[:, 1:].max(axis=1), tri[:, 1:].min(axis=1), tri[:, 0]))])


def candidates(xy, radius, min_angle_deg, simplices=None):
    """(k, 3) int32: the call's answer for the points `xy` -- built from scipy.spatial.Delaunay(xy).simplices (or `simplices`, already made)"""
    tri = scipy_simplices(xy) if simplices is None else np.asarray(simplices)
    return in_call_order(xy, tri[passes_screen(xy, tri, radius, min_angle_deg)])


def band(xy, radius, min_angle_deg, simplices=None):
    """scipy triangles whose longest side is within 1e-6 radius of the radius, plus those whose largest cosine is within 1e-6 of the threshold"""
    tri = scipy_simplices(xy) if simplices is None else np.asarray(simplices)
    s2, maxcos = sides2_maxcos(xy, tri)
    longest = np.sqrt(s2.max(axis=1))
    return (int(np.count_nonzero(np.abs(longest - radius) <= BAND * radius))
            + int(np.count_nonzero(np.abs(maxcos - _threshold(min_angle_deg)) <= BAND)))


def _keys(t):
    return [tuple(sorted(r)) for r in np.asarray(t).reshape(-1, 3).tolist()]


def difference(got, want):
    """None when `got` is `want`, array equal; else what broke first: "the set" (a triangle missing, added or twice), "the orientation"
    (a triangle that is its statement's mirror image), "the owner-first rule" (one that does not start with its smallest index), "the row
    order", or "the type" (not (k, 3) int32)"""
    want = _tris(want)
    got = np.asarray(got)
    if got.dtype != np.int32 or got.ndim != 2 or got.shape[1] != 3:
        return "the type"
    if np.array_equal(got, want):
        return None
    gk, wk = _keys(got), _keys(want)
    if len(set(gk)) != len(gk) or set(gk) != set(wk):
        return "the set"
    of = dict(zip(wk, want.tolist()))
    for key, row in zip(gk, got.tolist()):
        w = of[key]
        if row not in (w, w[1:] + w[:1], w[2:] + w[:2]):
            return "the orientation"
    if not (got[:, 0] == got.min(axis=1)).all():
        return "the owner-first rule"
    return "the row order"


def same_candidates(got, want):
    """the GPU test's comparison: exact array equality, or an AssertionError that names what broke"""
    what = difference(got, want)
    assert what is None, f"{what} broke: {len(np.asarray(got))} triangles against the statement's {len(want)}"


# ---- what the CPU test measures of a family --------------------------------------------------------------------------------------------
def grid_of(xy, radius):
    """dd_setup_kernel's grid: cells radius (1 + 1e-6) wide, the width doubled until floor(ext / cw) + 1 cells per axis fit 2 n + 64
    -> (nx, ny, cell width, doublings)"""
    xy = np.asarray(xy, np.float64)
    ext = xy.max(axis=0) - xy.min(axis=0)
    cw = radius * (1.0 + 1e-6)
    for doublings in range(64):
        fx, fy = np.floor(ext[0] / cw) + 1.0, np.floor(ext[1] / cw) + 1.0
        if fx * fy <= 2 * len(xy) + 64:
            return int(fx), int(fy), cw, doublings
        cw *= 2.0
    raise ValueError("no grid")


def neighbours_above(xy, radius):
    """per point p: the points q > p within the screen's radius (the candidate kernel's neighbour list)"""
    from scipy.spatial import cKDTree

    xy = np.asarray(xy, np.float64)
    pairs = cKDTree(xy).query_pairs(radius * 1.001, output_type="ndarray")
    d = xy[pairs[:, 0]] - xy[pairs[:, 1]]
    pairs = pairs[(d * d).sum(axis=1) < (radius * (1.0 + SLACK)) ** 2]
    return np.bincount(pairs.min(axis=1), minlength=len(xy))


def owner_counts(cands, n):
    return np.bincount(np.asarray(cands).reshape(-1, 3)[:, 0], minlength=n)


def hull_vertices(xy):
    from scipy.spatial import ConvexHull

    return ConvexHull(np.asarray(xy, np.float64)).vertices


def host_answers(xy, factor=4.0):
    """the host triangulator answers for the set at `factor` times the guard"""
    from same_amd import delaunay

    return delaunay.native_simplices(np.ascontiguousarray(xy, np.float64), guard=factor * delaunay.GUARD) is not None


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def _family(xy, radius, angle, expect, bit=0, **more):
    return C._frozen(dict(xy=np.ascontiguousarray(xy, np.float64), radius=float(radius), angle=float(angle), expect=expect, bit=bit, **more))


def uniform(n, seed, side=None):
    """the uniform family of tests/test_gpu_device_delaunay.py: n points at cfg 5's density"""
    side = float(np.sqrt(n / DENSITY)) if side is None else side
    return np.random.default_rng(seed).uniform(0, side, (n, 2))


SMALL = (3, 4, 5, 8)
CENTRE = np.array([300.0, 300.0])


def _small(n):
    """n = 3: one near-equilateral triangle of side about 10; n = 4: a convex quadrilateral; n = 5 and 8: a convex polygon of n - 1 corners
    with one point inside; generic coordinates near (300, 300)"""
    rng = np.random.default_rng(3100 + n)
    corners = n if n <= 4 else n - 1
    t = (np.arange(corners) + rng.uniform(-0.15, 0.15, corners)) * 2 * np.pi / corners + 0.3
    r = (10.0 / np.sqrt(3.0) if n == 3 else 9.0) * (1.0 + rng.uniform(-0.05, 0.05, corners))
    xy = CENTRE + np.column_stack((r * np.cos(t), r * np.sin(t)))
    if n > 4:
        xy = np.vstack((xy, CENTRE + rng.uniform(-2.0, 2.0, 2)))
    return _family(xy[rng.permutation(n)], 25, 10, ANSWER, corners=corners)


EDGES = (255, 256, 257, 513)
CELLS_SIDE = 395.0        # 16 x 16 cells of width 25 (1 + 1e-6): a cell count on scan::NT


def _disk(n_disk):
    """point 0 at the centre, n_disk more uniform in a disk of radius 12 around it: every pairwise distance below 24 < radius"""
    rng = np.random.default_rng(4200)
    r, t = 12.0 * np.sqrt(rng.uniform(0, 1, NB_CAP + 1)), rng.uniform(0, 2 * np.pi, NB_CAP + 1)
    xy = np.vstack((CENTRE, CENTRE + np.column_stack((r * np.cos(t), r * np.sin(t)))[:n_disk]))
    return _family(xy, 25, 10, ANSWER if n_disk <= NB_CAP else REFUSE, 0 if n_disk <= NB_CAP else OVERFLOW)


def _ring(n_ring):
    """point 0 at the centre, n_ring points on a ring of radius 10 around it (angle jitter +-0.02 of the spacing, radial jitter +-0.2 %):
    the fan of n_ring triangles around point 0, all its own"""
    rng = np.random.default_rng(4300 + n_ring)
    t = (np.arange(n_ring) + rng.uniform(-0.02, 0.02, n_ring)) * 2 * np.pi / n_ring
    r = 10.0 * (1.0 + rng.uniform(-0.002, 0.002, n_ring))
    xy = np.vstack((CENTRE, CENTRE + np.column_stack((r * np.cos(t), r * np.sin(t)))))
    return _family(xy, 25, 10, ANSWER if n_ring <= OWN_CAP else REFUSE, 0 if n_ring <= OWN_CAP else OVERFLOW)


HULL_INNER, HULL_RADIUS = 900, 2000.0


def _hull(n_ring):
    """900 points uniform in a 300-wide square, then n_ring points on a circle of radius 2000 about its centre (angle jitter +-0.2 of the
    spacing): n_ring hull vertices, every one of them near the hull"""
    rng = np.random.default_rng(4400)
    inner = rng.uniform(0, 300, (HULL_INNER, 2)) + (HULL_RADIUS - 150.0)
    jitter = np.random.default_rng(4401).uniform(-0.2, 0.2, SURV_CAP + 1)[:n_ring]
    t = (np.arange(n_ring) + jitter) * 2 * np.pi / n_ring
    ring = HULL_RADIUS + HULL_RADIUS * np.column_stack((np.cos(t), np.sin(t)))
    return _family(np.vstack((inner, ring)), 25, 15, ANSWER if n_ring <= SURV_CAP else REFUSE, 0 if n_ring <= SURV_CAP else OVERFLOW)


def _sparse():
    """30 clusters of 10 points, sigma 6, centres uniform in [0, 3000)^2, radius 12: far more radius-wide cells than 2 n + 64"""
    rng = np.random.default_rng(4500)
    centres = rng.uniform(0, 3000, (30, 2))
    return _family(np.repeat(centres, 10, axis=0) + rng.normal(0, 6.0, (300, 2)), 12, 10, ANSWER)


def _strip():
    """600 points in a 6000 x 20 strip: one row of cells"""
    rng = np.random.default_rng(4600)
    return _family(np.column_stack((rng.uniform(0, 6000, 600), rng.uniform(0, 20, 600))), 25, 15, ANSWER)


NEGATIVE_N = 1000
ON_CELL_EDGES = ((1, None), (2, None), (6, None), (11, None), (None, 1), (None, 3), (None, 8), (5, 4))     # whole cell widths in x, in y, in both


def _negative_uniform():
    """the uniform family at n = 1000, translated so that the extent straddles 0 in both axes"""
    side = float(np.sqrt(NEGATIVE_N / DENSITY))
    return _family(uniform(NEGATIVE_N, 4700) - side / 2, 25, 15, ANSWER)


def _negative_cluster():
    """the cluster family at n = 1000 around 0; the set's minimum corner is a point of its own, and eight points lie exactly on whole
    multiples of the cell width from it in x, in y or in both (the other coordinate generic: no three of them on a line): the
    boundaries of cell_x and cell_y"""
    rng = np.random.default_rng(4800)
    side = float(np.sqrt(NEGATIVE_N / DENSITY))
    centres = rng.uniform(0, side, (NEGATIVE_N // 20, 2))
    xy = centres[rng.integers(0, len(centres), NEGATIVE_N)] + rng.normal(0, 4.0, (NEGATIVE_N, 2)) - side / 2
    x0, y0 = np.floor(xy.min(axis=0)) - 1.5
    cw = 25.0 * (1.0 + 1e-6)
    free = rng.uniform(40.0, side - 40.0, (len(ON_CELL_EDGES), 2))
    on = np.array([(x0 + (a * cw if a is not None else f[0]), y0 + (b * cw if b is not None else f[1])) for (a, b), f in zip(ON_CELL_EDGES, free)])
    return _family(np.vstack((xy, [(x0, y0)], on)), 25, 15, ANSWER, corner=(x0, y0), cw=cw)


NONFINITE_HOW = ("nan first", "nan last", "nan middle", "+inf", "-inf", "all nan")


def _nonfinite(how):
    """the small uniform set (n = 257) with a coordinate that is not finite"""
    xy = uniform(257, 3257).copy()
    if how == "all nan":
        xy[:] = np.nan
    else:
        at = {"nan first": (0, 0), "nan last": (256, 1), "nan middle": (128, 1), "+inf": (100, 0), "-inf": (101, 1)}[how]
        xy[at] = {"+inf": np.inf, "-inf": -np.inf}.get(how, np.nan)
    return _family(xy, 25, 15, REFUSE, NONFINITE)


SMALL_ANGLES = (2, 3, 5)

LADDER_EPS = (0.0,) + tuple(10.0 ** e for e in range(-15, -2))       # 0, 1e-15, ..., 1e-3
LADDERS = ("rectangle", "duplicate", "hull line")
RECTANGLE = np.array([(100.0, 100.0), (106.0, 100.0), (106.0, 108.0), (100.0, 108.0)])     # sides 6 and 8, diagonal 10: centre (103, 104)
DUPLICATED = 7
HULL_LINE = np.array([(40.0, -6.0), (100.0, -6.0), (160.0, -6.0)])
LADDER_GENERIC = 400


def _generic(seed, keep_out=None):
    """400 generic points uniform in [0, 200)^2, none within `keep_out` = (centre, distance)"""
    xy = np.random.default_rng(seed).uniform(0, 200, (2 * LADDER_GENERIC, 2))
    if keep_out is not None:
        xy = xy[np.hypot(*(xy - keep_out[0]).T) > keep_out[1]]
    return xy[:LADDER_GENERIC]


def _ladder(which, rung):
    """an exactly degenerate configuration inside a generic set of 400 points, opened by LADDER_EPS[rung] times its size:
    rectangle: four whole corners, the circumcircle empty; corner (106, 108) moves outward along the diagonal (size 10);
    duplicate: point 7 a second time; the copy moves away (size 10, a mean spacing);
    hull line: three hull points with whole coordinates on y = -6; the middle one moves outward (size 120)"""
    eps = LADDER_EPS[rung]
    if which == "rectangle":
        extra = RECTANGLE.copy()
        extra[2] += eps * 10.0 * np.array([0.6, 0.8])
        xy = np.vstack((_generic(5100, (np.array([103.0, 104.0]), 9.0)), extra))
    elif which == "duplicate":
        xy = _generic(5200)
        xy = np.vstack((xy, xy[DUPLICATED] + eps * 10.0 * np.array([0.6, 0.8])))
    else:
        extra = HULL_LINE.copy()
        extra[1, 1] -= eps * 120.0
        xy = np.vstack((_generic(5300), extra))
    return _family(xy, 25, 10, EITHER, IN_DOUBT, rung=rung, eps=eps, top=rung == len(LADDER_EPS) - 1)


def _build(name):
    kind, _, rest = name.partition("/")
    if kind == "small":
        return _small(int(rest))
    if kind == "edges" and rest == "cells256":
        return _family(uniform(int(CELLS_SIDE ** 2 * DENSITY), 3999, CELLS_SIDE), 25, 15, ANSWER)
    if kind == "edges":
        return _family(uniform(int(rest), 3000 + int(rest)), 25, 15, ANSWER)
    if kind == "sparse":
        return _sparse()
    if kind == "strip":
        return _strip()
    if kind in ("nb128", "nb129"):
        return _disk(int(kind[2:]))
    if kind in ("own32", "own33"):
        return _ring(int(kind[3:]))
    if kind in ("hull1024", "hull1025"):
        return _hull(int(kind[4:]))
    if name == "negative/uniform":
        return _negative_uniform()
    if name == "negative/cluster":
        return _negative_cluster()
    if kind == "nonfinite":
        return _nonfinite(rest)
    if kind == "angle":
        return _family(uniform(NEGATIVE_N, 4700), 25, int(rest), EITHER, OVERFLOW)
    if kind == "ladder":
        which, _, rung = rest.partition("/")
        return _ladder(which, int(rung))
    if kind == "w":
        return _window_family(rest)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def family(name):
    """-> dict(xy, radius, angle, expect, bit, ...) of a name of NAMES (or "w/" + a name of WINDOW_NAMES: the window section's copy)"""
    return _build(name)


@functools.lru_cache(maxsize=None)
def simplices_of(name):
    s = scipy_simplices(family(name)["xy"])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def statement_of(name, radius=None, angle=None):
    """`candidates` of a family at its own settings (or at another radius / angle), made once"""
    f = family(name)
    out = candidates(f["xy"], f["radius"] if radius is None else radius, f["angle"] if angle is None else angle, simplices_of(name))
    out.setflags(write=False)
    return out


def band_of(name, radius=None, angle=None):
    f = family(name)
    return band(f["xy"], f["radius"] if radius is None else radius, f["angle"] if angle is None else angle, simplices_of(name))


MUST_ANSWER = (tuple(f"small/{n}" for n in SMALL) + tuple(f"edges/{n}" for n in EDGES)
               + ("edges/cells256", "sparse", "strip", "nb128", "own32", "hull1024", "negative/uniform", "negative/cluster"))
CAPACITY_REFUSED = ("nb129", "own33", "hull1025")
CAPACITY_PAIRS = (("nb128", "nb129"), ("own32", "own33"), ("hull1024", "hull1025"))
MUST_REFUSE = CAPACITY_REFUSED + tuple(f"nonfinite/{how}" for how in NONFINITE_HOW)
LADDER_NAMES = tuple(f"ladder/{which}/{rung}" for which in LADDERS for rung in range(len(LADDER_EPS)))
EITHER_NAMES = tuple(f"angle/{a}" for a in SMALL_ANGLES) + LADDER_NAMES
NAMES = MUST_ANSWER + MUST_REFUSE + EITHER_NAMES
CALL_ORDER = ("hull1024", "small/3", "nb129", "nb128", "sparse", "own33", "own32")      # one context's slots: shrinking, growing, refused


def expectation(name, rung_rule=True):
    """(expect, bit) of a family; a ladder's rung 0 must be refused and its top rung answered"""
    f = family(name)
    if name.startswith("ladder/") and rung_rule:
        if f["rung"] == 0:
            return REFUSE, f["bit"]
        if f["top"]:
            return ANSWER, 0
    return f["expect"], f["bit"]


def settings_cases():
    """same_delaunay_filtered's arguments that are refused before a kernel runs: (tag, n points of the small uniform set, radius,
    angle_enabled, cos_thr, the status)"""
    thr = _threshold(15)
    return (("radius inf", 257, np.inf, 1, thr, NO_ANGLE), ("radius 0", 257, 0.0, 1, thr, NO_ANGLE), ("angle off", 257, 25.0, 0, thr, NO_ANGLE),
            ("threshold nan", 257, 25.0, 1, np.nan, NO_ANGLE), ("n = 0", 0, 25.0, 1, thr, FEW_POINTS), ("n = 1", 1, 25.0, 1, thr, FEW_POINTS),
            ("n = 2", 2, 25.0, 1, thr, FEW_POINTS))


# ---- the window section: the families side by side ----------------------------------------------------------------------------------
# Every family that a box can hold (finite coordinates), moved by WHOLE numbers to a place of its own; "pair" is two points of its own
# (a window of 2 cells), small/3 the window of 3; "no cell": five moving points whose references stand 60 away (rows on both sides of
# the box, no kept cell).  Everywhere else the reference section is the moving points themselves: every row in a box is kept.
WINDOW_NAMES = MUST_ANSWER + CAPACITY_REFUSED
WINDOW_RADIUS, WINDOW_K, WINDOW_COEFF, WINDOW_PENALTY = 25.0, 4, 1000.0, 50.0
WINDOW_SETTINGS = ((25.0, 10.0), (12.0, 10.0), (25.0, 15.0))          # the families' own (radius, min_angle_deg)
PAIR, NO_CELL = "pair", "no cell"
_PLACES = {"hull1024": (0, 0), "hull1025": (4200, 0), "sparse": (0, 4300), "strip": (0, 7500), "negative/uniform": (3400, 4300),
           "negative/cluster": (3900, 4300), "edges/cells256": (4400, 4300), "edges/513": (4900, 4300), "edges/255": (5300, 4300),
           "edges/256": (5600, 4300), "edges/257": (5900, 4300), "nb128": (3400, 4800), "nb129": (3500, 4800), "own32": (3600, 4800),
           "own33": (3700, 4800), "small/3": (3800, 4800), "small/4": (3900, 4800), "small/5": (4000, 4800), "small/8": (4100, 4800)}
_PAIR_AT, _NO_CELL_AT = (4250.0, 4850.0), (4400.0, 4850.0)


def _moved(name):
    xy = family(name)["xy"]
    return xy - np.floor(xy.min(axis=0)) + np.asarray(_PLACES[name], np.float64) + 10.0


def _window_family(name):
    f = family(name)
    return _family(_moved(name), f["radius"], f["angle"], f["expect"], f["bit"])


def _box(xy):
    return (float(xy[:, 0].min() - 1), float(xy[:, 0].max() + 1), float(xy[:, 1].min() - 1), float(xy[:, 1].max() + 1))


@functools.lru_cache(maxsize=None)
def window_section():
    """-> dict(mov_xy, ref_xy, types_m, types_r, type_id, size, names, boxes, first): window w = names[w] holds the rows
    first[w] : first[w + 1] of the section, in the family's order, inside boxes[w]"""
    rng = np.random.default_rng(6000)
    parts = [family("w/" + name)["xy"] for name in WINDOW_NAMES]
    pair = np.asarray(_PAIR_AT) + np.array([(0.0, 0.0), (7.3, 4.1)])
    lone = np.asarray(_NO_CELL_AT) + rng.uniform(0, 10, (5, 2))
    mov = np.vstack(parts + [pair, lone])
    ref = mov.copy()
    ref[-5:, 0] += 60.0
    names = WINDOW_NAMES + (PAIR, NO_CELL)
    first = np.concatenate(([0], np.cumsum([len(p) for p in parts] + [2, 5])))
    boxes = [_box(p) for p in parts] + [_box(pair), _box(np.vstack((lone, ref[-5:])))]
    n = len(mov)
    return C._frozen(dict(mov_xy=np.ascontiguousarray(mov), ref_xy=np.ascontiguousarray(ref), types_m=np.zeros((n, 0)), types_r=np.zeros((n, 0)),
                          type_id=rng.integers(0, 3, n).astype(np.int32), size=rng.integers(1, 4, n).astype(np.float64), names=names,
                          boxes=tuple(boxes), first=first, radius=WINDOW_RADIUS, k=WINDOW_K, coeff=WINDOW_COEFF))


def window_index(name):
    return window_section()["names"].index(name)


def window_expectation(name, radius, angle):
    """what same_window_delaunay must say of the window `name` at the call's settings: at the family's own settings its tag; at another
    family's settings either an answer equal to the statement or a refusal for a capacity or a doubt (the CPU test holds the band at 0
    at all of WINDOW_SETTINGS, so an answer is decided by no rounding) -> (expect, bits allowed or asked for)"""
    if name in (PAIR, NO_CELL):
        return REFUSE, FEW_POINTS
    f = family("w/" + name)
    if (f["radius"], f["angle"]) == (radius, angle):
        return f["expect"], f["bit"]
    return EITHER, OVERFLOW | IN_DOUBT


@functools.lru_cache(maxsize=None)
def batch_section():
    """WINDOW_BATCH_MAX windows side by side, 400 apart: every third a box of 2 cells, the others 50 to 300 uniform points at cfg 5's
    density (radius 25, min_angle_deg 15) -> the section as window_section()'s; `sizes`"""
    rng = np.random.default_rng(6400)
    parts, sizes = [], []
    for w in range(WINDOW_BATCH_MAX):
        n = 2 if w % 3 == 2 else int(rng.integers(50, 301))
        xy = rng.uniform(0, np.sqrt(n / DENSITY), (n, 2)) if n > 2 else np.array([(0.0, 0.0), (6.1, 3.7)])
        parts.append(xy + ((w % 16) * 400.0 + 10.0, (w // 16) * 400.0 + 10.0))
        sizes.append(n)
    mov = np.vstack(parts)
    n = len(mov)
    first = np.concatenate(([0], np.cumsum(sizes)))
    return C._frozen(dict(mov_xy=np.ascontiguousarray(mov), ref_xy=mov.copy(), types_m=np.zeros((n, 0)), types_r=np.zeros((n, 0)),
                          type_id=rng.integers(0, 3, n).astype(np.int32), size=rng.integers(1, 4, n).astype(np.float64),
                          names=tuple(f"batch/{w}" for w in range(WINDOW_BATCH_MAX)), boxes=tuple(_box(p) for p in parts), first=first,
                          sizes=tuple(sizes), radius=WINDOW_RADIUS, k=WINDOW_K, coeff=WINDOW_COEFF))
