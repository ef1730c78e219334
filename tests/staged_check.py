"""The host statements of the four staged calls -- same_collapse_candidates and same_greedy_disjoint (csrc/match.hip), same_window_count
(csrc/sweep.hip), same_eager_signs (csrc/tri.hip) -- and the input families their library-level tests run them on.

Each statement is the operation in plain numpy float64 and Python, written from the reference's text: src/metacell_utils.py:234-262
(validity), :400-430 (candidate, perimeter, total), :437-448 (sort and vertex-disjoint scan), src/same.py:293-295 (the half-open box),
src/helpers.py:425-441 (the rounded cross product's sign).  It imports nothing that ends in libsame_hip.

Every finite coordinate of the geometry families is an integer of magnitude <= 2**20, so every difference, product and sum that comes
before a sqrt or a division is exact in float64 (`geometry_is_exact` checks it with Python's integers): fused and unfused arithmetic
agree and the kernel has to equal the statement in every bit.  The eager-sign rounding points have p1 = (0, 0) and p2 = (1, 0), so the
cross product is p3.y exactly.  Non-finite members are compared as numpy computes them.

The families make what the product routes never hand the calls: zero sides, collinear corners, an edge exactly r_max long, an angle on
the threshold, NaN and infinite corners, totals one ulp over max_size; chains that need a round per item, ties across waves, both zeros in
one tie group; points on every edge of a box, padded lanes that would count row 0; cross products that round to zero, tie at a half,
overflow or are NaN.  tests/test_staged_check_cpu.py checks, without a GPU, that each statement equals what the project already trusts,
that each family has the property it was made for and that planted wrong kernels (`pairwise_max`, `sign_ordered`, `padded_counts`,
`round_half_up`) are caught; tests/test_gpu_staged_library.py drives the library against the statements.  Not collected by pytest."""
import collections
import itertools

import numpy as np

Collapse = collections.namedtuple("Collapse", "xy tris type_id size r_max min_angle_deg max_size")
Disjoint = collections.namedtuple("Disjoint", "items keys n_nodes")
Windows = collections.namedtuple("Windows", "xy boxes")
Eager = collections.namedtuple("Eager", "rxy tris cand")

SIZES = (1, 63, 64, 65, 255, 256, 257)         # a wave, a block, and one either side
COLLAPSE_SIZES = SIZES + (769,)
WINDOW_SIZES = SIZES + (1000,)
BOX_COUNTS = (1, 5, 300)
CHAIN = 600                                    # items in the chain: CHAIN / 2 rounds, through the whole 4, 4, 8 ... 64 batch schedule
COORD_MAX = 2**20
NAN, INF = float("nan"), float("inf")
MIN_ANGLES = (None, 0, float(np.nextafter(45.0, 0.0)), 45, float(np.nextafter(45.0, 90.0)), 60, 90, 180, 181)
ROUNDING_Y = (0.0004, -0.0004, 0.0005, -0.0005, float(np.nextafter(0.0005, 0.0)), float(np.nextafter(0.0005, 1.0)),
              -float(np.nextafter(0.0005, 0.0)), -float(np.nextafter(0.0005, 1.0)), 0.0015, -0.0015, 0.0025, -0.0025, 0.0, -0.0, 1e-320, NAN)


# ---- same_collapse_candidates: the statement ---------------------------------------------------------------------------------------------
def corner_angle(p1, p2, p3):
    """src/metacell_utils.py:234-240: the angle at p2 in degrees; a zero side gives 0 / 0 = NaN, which np.clip keeps"""
    v1, v2 = p1 - p2, p3 - p2
    with np.errstate(all="ignore"):
        c = np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2))
        return np.degrees(np.arccos(np.clip(c, -1, 1)))


def python_max(e1, e2, e3):
    """Python's max on three numbers: the first stays unless a later one compares greater, so a leading NaN wins and later ones are skipped"""
    return max(e1, e2, e3)


def pairwise_max(e1, e2, e3):
    """a planted wrong rule: `mx = e1 > e2 ? e1 : e2; mx = mx > e3 ? mx : e3`, which drops a leading NaN and lets a later one through"""
    mx = e1 if e1 > e2 else e2
    return mx if mx > e3 else e3


def triangle_valid(p1, p2, p3, r_max, min_angle_deg, edge_max=python_max):
    """src/metacell_utils.py:242-262"""
    with np.errstate(all="ignore"):
        if r_max is not None and edge_max(np.linalg.norm(p2 - p1), np.linalg.norm(p3 - p2), np.linalg.norm(p1 - p3)) > r_max:
            return False
        if min_angle_deg is not None and min(corner_angle(p2, p1, p3), corner_angle(p1, p2, p3), corner_angle(p1, p3, p2)) < min_angle_deg:
            return False
    return True


def host_collapse(case, edge_max=python_max):
    """-> (flag uint8 [bit0 valid, bit1 candidate: valid, one type id, not total > max_size], perimeter (|a-b| + |b-c|) + |c-a|,
    total size[a] + size[b] + size[c]) per triangle, in a Python loop as src/metacell_utils.py:400-430 runs"""
    xy = np.asarray(case.xy, np.float64).reshape(-1, 2)
    tris = np.asarray(case.tris, np.int64).reshape(-1, 3)
    type_id, size = np.asarray(case.type_id), np.asarray(case.size, np.float64)
    flag, perim, total = np.zeros(len(tris), np.uint8), np.zeros(len(tris)), np.zeros(len(tris))
    with np.errstate(all="ignore"):
        for t, (a, b, c) in enumerate(tris):
            valid = triangle_valid(xy[a], xy[b], xy[c], case.r_max, case.min_angle_deg, edge_max)
            total[t] = size[a] + size[b] + size[c]
            perim[t] = np.linalg.norm(xy[a] - xy[b]) + np.linalg.norm(xy[b] - xy[c]) + np.linalg.norm(xy[c] - xy[a])
            candidate = valid and type_id[a] == type_id[b] == type_id[c] and not total[t] > case.max_size
            flag[t] = valid + 2 * candidate
    return flag, perim, total


def geometry_is_exact(xy, tris):
    """the exactness precondition, in Python's integers: every finite coordinate is an integer of magnitude <= COORD_MAX, and every squared
    length and dot product the statement forms over the finite corners of `tris` is below 2**53"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    finite = xy[np.isfinite(xy)]
    if not (np.all(finite == np.rint(finite)) and np.all(np.abs(finite) <= COORD_MAX)):
        return False
    for tri in np.asarray(tris, np.int64).reshape(-1, 3):
        pts = [tuple(int(v) for v in xy[i]) for i in tri if np.isfinite(xy[i]).all()]
        for p, q, r in itertools.permutations(pts, 3) if len(pts) == 3 else ():
            v1, v2 = (p[0] - q[0], p[1] - q[1]), (r[0] - q[0], r[1] - q[1])
            if max(abs(v1[0] * v2[0] + v1[1] * v2[1]), v1[0] ** 2 + v1[1] ** 2, abs(v1[0] * v2[0]), abs(v1[1] * v2[1])) >= 2**53:
                return False
    return True


# ---- same_collapse_candidates: the families ----------------------------------------------------------------------------------------------
SHAPES = {"3-4-5": ((0, 0), (4, 0), (0, 3)), "5-12-13": ((0, 0), (12, 0), (0, 5)), "right-isosceles": ((0, 0), (1, 0), (0, 1)),
          "thin": ((0, 0), (12, 0), (6, 1)), "obtuse": ((0, 0), (4, 0), (-3, 4))}
ORDERS = tuple(itertools.permutations(range(3)))


def _placed(shape, scale, at, order=(0, 1, 2), turn=0):
    """the shape's corners times `scale`, turned by `turn` quarter turns, moved to `at`, in vertex order `order` -> (3, 2) integers"""
    pts = np.array(SHAPES[shape], np.int64) * scale
    for _ in range(turn % 4):
        pts = np.column_stack((-pts[:, 1], pts[:, 0]))
    return (pts + np.asarray(at, np.int64))[list(order)]


def _own_points(corners, **kw):
    """one Collapse over triangles that share no point: `corners` (Tr, 3, 2); type 0, size 1, no rule unless given"""
    corners = np.asarray(corners, np.float64).reshape(-1, 3, 2)
    n = 3 * len(corners)
    base = dict(xy=corners.reshape(-1, 2), tris=np.arange(n, dtype=np.int32).reshape(-1, 3), type_id=np.zeros(n, np.int32),
                size=np.ones(n), r_max=None, min_angle_deg=None, max_size=3.0)
    base.update(kw)
    return Collapse(**base)


def collapse_sizes(seed=21):
    """Tr at the wave and block edges: a lattice of 3-4-5 and 5-12-13 triangles at scales 1 ... 2**16, mixed with right-isosceles and thin
    ones, every vertex order and quarter turn; r_max between the scales, 10 degrees, types and sizes that make both answers"""
    rng = np.random.default_rng(seed)
    names, scales = ("3-4-5", "5-12-13", "3-4-5", "right-isosceles", "5-12-13", "thin"), (1, 2, 7, 100, 2**10, 2**16)
    out = []
    for Tr in COLLAPSE_SIZES:
        corners = [_placed(names[t % 6], scales[(t // 6) % 6], (37 * (t % 29) - 500, 41 * (t // 29) - 300), ORDERS[t % 6], t // 7)
                   for t in range(Tr)]
        n = 3 * Tr
        type_id = np.repeat(rng.integers(0, 3, Tr), 3).astype(np.int32)
        type_id[rng.choice(n, n // 10, replace=False)] = 7
        out.append((f"{Tr} triangles", _own_points(corners, type_id=type_id, size=rng.integers(1, 3, n).astype(np.float64), r_max=700.0,
                                                   min_angle_deg=10, max_size=4.0)))
    return out


def zero_sides():
    """(a, a, b), (a, b, b), (a, b, a) and (a, a, a) over a = (0, 0), b = (3, 4), with and without r_max; at 10 degrees the statement says
    valid, invalid, valid, valid: which corner's angle is NaN decides"""
    xy = np.array([(0, 0), (3, 4)], np.float64)
    tris = np.array([(0, 0, 1), (0, 1, 1), (0, 1, 0), (0, 0, 0)], np.int32)
    base = Collapse(xy, tris, np.zeros(2, np.int32), np.ones(2), None, 10, 3.0)
    return [(f"r_max {r}", base._replace(r_max=r)) for r in (None, 10.0, 5.0, 4.0)]


def collinear():
    """three points on a line in all six vertex orders: angles of 0 and 180 degrees"""
    corners = [np.array(pts, np.int64)[list(o)] for pts in (((0, 0), (3, 4), (6, 8)), ((0, 0), (1, 0), (5, 0)), ((-7, 2), (-7, 9), (-7, 3)))
               for o in ORDERS]
    rules = ((10, None), (None, 9.0), (0, 100.0), (180, None), (181, None))
    return [(f"min_angle_deg {m}", _own_points(corners, min_angle_deg=m, r_max=r)) for m, r in rules]


def rmax_edges():
    """r_max exactly the longest edge (valid: the rule is >), one float below and above it, and 0, inf, NaN, None; the longest edge in every
    position, and one that is a rounded square root (the right-isosceles hypotenuse)"""
    corners = [_placed(name, 6, (11 * q, -5), o) for q, (name, o) in enumerate(itertools.product(("3-4-5", "right-isosceles"), ORDERS))]
    longest = (30.0, float(np.sqrt(72.0)))
    values = [v for e in longest for v in (e, float(np.nextafter(e, 0.0)), float(np.nextafter(e, INF)))] + [0.0, INF, NAN, None]
    return [(f"r_max {v!r}", _own_points(corners, r_max=v)) for v in values]


def angle_edges():
    """every min_angle_deg of MIN_ANGLES on right-isosceles and 3-4-5 triangles, every order and quarter turn, at several scales: corner
    angles on and beside 45 and 90 degrees, both infinite thresholds of cos_threshold (0 and None: nothing fails; 181: everything does)"""
    corners = [_placed(name, s, (0, 0), o, q) for q, (name, s, o) in
               enumerate(itertools.product(("right-isosceles", "3-4-5", "obtuse"), (1, 3, 7, 1000, 2**18), ORDERS))]
    return [(f"min_angle_deg {m!r}", _own_points(corners, min_angle_deg=m)) for m in MIN_ANGLES]


def nonfinite_corners():
    """one NaN, +inf or -inf coordinate (x or y) at each of the three vertex positions, the two finite corners 5 apart or 20.02... apart
    (either side of r_max = 10), and two corners at the same infinity (inf - inf); under both rules, each alone, and neither.  A NaN corner
    makes the edges (NaN, e, NaN) when it is first, (NaN, NaN, e) when second, (e, NaN, NaN) when last: Python's max keeps a leading NaN and
    skips a later one, so the first two pass any r_max and the last is judged by e"""
    corners = []
    for far, value, col, pos in itertools.product(((3, 4), (20, 1)), (NAN, INF, -INF), (0, 1), range(3)):
        pts = [(0.0, 0.0), tuple(map(float, far))]
        bad = [0.0, 0.0]
        bad[col] = value
        pts.insert(pos, tuple(bad))
        corners.append(pts)
    for value, o in itertools.product((INF, -INF), ORDERS):
        corners.append(np.array([(value, 1.0), (value, 2.0), (0.0, 0.0)])[list(o)])
        corners.append(np.array([(value, value), (value, value), (3.0, 4.0)])[list(o)])
    rules = ((10.0, 10), (10.0, None), (None, 10), (None, None))
    return [(f"r_max {r}, min_angle_deg {m}", _own_points(corners, r_max=r, min_angle_deg=m)) for r, m in rules]


def size_and_type_rules():
    """one valid 3-4-5 triangle per row of a table of (sizes, type ids): totals exactly max_size and one ulp over it, NaN and negative sizes,
    type ids equal pairwise but not all three, negative type ids; then max_size 0 and NaN; arrays with rows no triangle names"""
    over = 1.0 + 2.0**-51                                # 1 + 1 + over == 3 + 2**-51 exactly: the float after 3
    table = [((1, 1, 1), (0, 0, 0)), ((1, 1, over), (0, 0, 0)), ((over, 1, 1), (0, 0, 0)), ((1, 1, NAN), (0, 0, 0)), ((NAN, 1, 1), (0, 0, 0)),
             ((-1, -1, -1), (0, 0, 0)), ((-5, 4, 4), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((-0.0, -0.0, -0.0), (0, 0, 0)), ((2, 2, 2), (0, 0, 0)),
             ((1, 1, 1), (1, 1, 2)), ((1, 1, 1), (2, 1, 1)), ((1, 1, 1), (1, 2, 1)), ((1, 1, 1), (-1, -1, -1)), ((1, 1, 1), (-1, -1, -2)),
             ((1, 1, 1), (-2**31, -2**31, -2**31)), ((1, 1, 1), (2**31 - 1, 2**31 - 1, 2**31 - 1)), ((INF, 1, 1), (0, 0, 0)),
             ((INF, -INF, 1), (0, 0, 0))]
    corners = [_placed("3-4-5", 2, (9 * q, 0), ORDERS[q % 6]) for q in range(len(table))]
    spare = 40                                           # rows after the last one a triangle names
    xy = np.vstack((np.asarray(corners, np.float64).reshape(-1, 2), np.full((spare, 2), NAN)))
    size = np.concatenate((np.array([s for s, _t in table], np.float64).reshape(-1), np.full(spare, NAN)))
    type_id = np.concatenate((np.array([t for _s, t in table], np.int64).reshape(-1), np.arange(spare) + 100)).astype(np.int32)
    base = Collapse(xy, np.arange(3 * len(table), dtype=np.int32).reshape(-1, 3), type_id, size, 100.0, 10, 3.0)
    return [(f"max_size {m!r}", base._replace(max_size=m)) for m in (3.0, 0.0, NAN, -3.0, INF)]


def collapse_families():
    """[(family, [(name, Collapse)])]"""
    return [(f.__name__, f()) for f in (collapse_sizes, zero_sides, collinear, rmax_edges, angle_edges, nonfinite_corners, size_and_type_rules)]


# ---- same_greedy_disjoint: the statement ----------------------------------------------------------------------------------------------------
def host_disjoint(case):
    """src/metacell_utils.py:437-448: list.sort by key (stable: equal keys, the two zeros among them, stay in list order), then one scan that
    takes an item when none of its three vertices is used -> selected (M,) bool.  NaN keys are outside the contract: Python's sort on them is
    not an order"""
    items, keys = np.asarray(case.items, np.int64).reshape(-1, 3).tolist(), np.asarray(case.keys, np.float64).tolist()
    used, selected = set(), np.zeros(len(items), bool)
    for m in sorted(range(len(items)), key=keys.__getitem__):
        a, b, c = items[m]
        if a not in used and b not in used and c not in used:
            selected[m] = True
            used.update((a, b, c))
    return selected


def sign_ordered(keys):
    """a planted wrong key: the doubles' bit patterns in their total order, in which -0.0 comes before +0.0"""
    u = np.asarray(keys, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def local_minimum_rounds(case, order_key=None):
    """the rule the kernels run: in every round, each item alive (no vertex used yet) that is the smallest (key, index) at all three of its
    vertices among the items alive is taken, until none is alive -> (selected, rounds).  `order_key` maps the keys to what is compared
    (default: their values, the two zeros equal)"""
    items, keys = np.asarray(case.items, np.int64).reshape(-1, 3), np.asarray(case.keys, np.float64)
    rank = np.unique(keys if order_key is None else order_key(keys), return_inverse=True)[1].astype(np.int64) * len(items) + np.arange(len(items))
    used, selected, rounds = np.zeros(case.n_nodes, bool), np.zeros(len(items), bool), 0
    alive = np.ones(len(items), bool)
    while True:
        alive &= ~used[items].any(axis=1)
        if not alive.any():
            return selected, rounds
        best = np.full(case.n_nodes, np.iinfo(np.int64).max)
        np.minimum.at(best, items[alive].reshape(-1), np.repeat(rank[alive], 3))
        take = alive & (best[items] == rank[:, None]).all(axis=1)
        selected |= take
        alive &= ~take
        used[items[take].reshape(-1)] = True
        rounds += 1


# ---- same_greedy_disjoint: the families -----------------------------------------------------------------------------------------------------
def _random_items(rng, M, n_nodes):
    """M triples of three different vertices"""
    return np.array([rng.choice(n_nodes, 3, replace=False) for _ in range(M)], np.int32).reshape(-1, 3)


def disjoint_sizes(seed=31):
    """M at the wave and block edges, random triples over M // 4 + 6 nodes, keys with one decimal: heavy ties, within a wave and across"""
    rng = np.random.default_rng(seed)
    return [(f"{M} items", Disjoint(_random_items(rng, M, M // 4 + 6), np.round(rng.gamma(2.0, 0.4, M), 1), M // 4 + 6)) for M in SIZES]


def chain():
    """item m holds {2m, 2m + 1, 2m + 2}: under rising (or equal) keys only the first item alive is a local minimum, so each round takes one
    item and CHAIN / 2 rounds take every other one; falling keys run the chain from its other end"""
    items = (2 * np.arange(CHAIN)[:, None] + np.arange(3)).astype(np.int32)
    rising = np.arange(CHAIN, dtype=np.float64) / 8.0
    return [(name, Disjoint(items, keys, 2 * CHAIN + 1)) for name, keys in (("rising", rising), ("falling", rising[::-1].copy()),
                                                                            ("equal", np.full(CHAIN, 2.5)))]


def star(seed=32):
    """every item holds vertex 0: one is taken, the smallest key or the first among equal ones, in one round"""
    rng = np.random.default_rng(seed)
    M = 300
    items = np.column_stack((np.zeros(M), 1 + 2 * np.arange(M), 2 + 2 * np.arange(M))).astype(np.int32)
    distinct = rng.permutation(M).astype(np.float64)
    tied = np.full(M, 4.0)
    tied[[70, 130, 257]] = 1.0                            # the first of them is in the second wave
    return [(name, Disjoint(items, keys, 2 * M + 1)) for name, keys in (("distinct keys", distinct), ("equal keys", np.full(M, 4.0)),
                                                                        ("three equal smallest", tied))]


def disjoint_items(seed=33):
    """no two items share a vertex: all are taken in one round"""
    rng = np.random.default_rng(seed)
    M = 300
    return [("disjoint", Disjoint(rng.permutation(3 * M).astype(np.int32).reshape(-1, 3), np.round(rng.random(M), 1), 3 * M))]


def repeated_vertex(seed=34):
    """items (a, a, b), (a, b, a), (b, a, a) and (a, a, a) among random ones"""
    rng = np.random.default_rng(seed)
    items = _random_items(rng, 200, 40)
    items[::4, 1] = items[::4, 0]
    items[1::8, 2] = items[1::8, 0]
    items[2::8, 2] = items[2::8, 1]
    items[3::16] = items[3::16, :1]
    return [("repeated", Disjoint(items, np.round(rng.gamma(2.0, 0.4, 200), 1), 40))]


def many_nodes(seed=35):
    """100 000 nodes and 50 items on the top ids; the same items with n_nodes exactly max id + 1"""
    rng = np.random.default_rng(seed)
    items = (100_000 - 1 - _random_items(rng, 50, 30)).astype(np.int32)
    keys = np.round(rng.gamma(2.0, 0.4, 50), 1)
    low = (items - items.min()).astype(np.int32)
    return [("100000 nodes", Disjoint(items, keys, 100_000)), ("max id + 1 nodes", Disjoint(low, keys, int(low.max()) + 1))]


def extreme_keys(seed=36):
    """+inf, -inf, negative values, subnormals of both signs, the largest doubles and one zero, many times each: ties at every one"""
    rng = np.random.default_rng(seed)
    pool = np.array([INF, -INF, -1.5, -1e300, 1e300, 5e-324, -5e-324, 1e-320, -1e-320, 0.0, 1.7976931348623157e308, 2.5, -2.5])
    return [("extremes", Disjoint(_random_items(rng, 400, 90), pool[rng.integers(0, len(pool), 400)], 90))]


def two_zeros(seed=37):
    """+0.0 and -0.0 in one tie group: a star whose first item has +0.0 and whose second has -0.0 (list order takes the first), and random
    triples under keys that are one zero or the other"""
    rng = np.random.default_rng(seed)
    hub = np.column_stack((np.zeros(70), 1 + 2 * np.arange(70), 2 + 2 * np.arange(70))).astype(np.int32)
    keys = np.full(70, 3.0)
    keys[:4] = (0.0, -0.0, 0.0, -0.0)
    signs = np.where(rng.random(300) < 0.5, 0.0, -0.0)
    return [("star", Disjoint(hub, keys, 141)), ("random", Disjoint(_random_items(rng, 300, 80), signs, 80))]


def disjoint_families():
    """[(family, [(name, Disjoint)])]"""
    return [(f.__name__, f()) for f in (disjoint_sizes, chain, star, disjoint_items, repeated_vertex, many_nodes, extreme_keys, two_zeros)]


# ---- same_window_count -----------------------------------------------------------------------------------------------------------------------
def host_window_mask(case):
    """src/same.py:293-295 per box {x0, x1, y0, y1}, half-open -> mask [n_boxes][n] bool; counts are its row sums"""
    xy, boxes = np.asarray(case.xy, np.float64).reshape(-1, 2), np.asarray(case.boxes, np.float64).reshape(-1, 4)
    x, y = xy[None, :, 0], xy[None, :, 1]
    with np.errstate(invalid="ignore"):
        return (x >= boxes[:, 0:1]) & (x < boxes[:, 1:2]) & (y >= boxes[:, 2:3]) & (y < boxes[:, 3:4])


def padded_counts(case, block=256):
    """a planted wrong count: the lanes beyond n, which load row 0 in its stead, are counted with the rest"""
    mask = host_window_mask(case)
    n = mask.shape[1]
    return mask.sum(axis=1) + (-n % block) * mask[:, 0]


def window_sizes(seed=41):
    """n at the wave and block edges times 1, 5 and 300 boxes; integer points in [-60, 60], integer boxes around the origin, where row 0
    lies: it is inside every box, so a padded lane that counted its stand-in load of row 0 shows as an excess"""
    rng = np.random.default_rng(seed)
    out = []
    for n, n_boxes in itertools.product(WINDOW_SIZES, BOX_COUNTS):
        xy = rng.integers(-60, 61, (n, 2)).astype(np.float64)
        xy[0] = 0.0
        lo, hi = -rng.integers(0, 50, (n_boxes, 2)), rng.integers(1, 50, (n_boxes, 2))
        out.append((f"{n} points, {n_boxes} boxes", Windows(xy, np.column_stack((lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1])).astype(np.float64))))
    return out


def window_edges():
    """points on x0, x1, y0, y1, on the corners and one float inside x1 and y1; NaN and infinite points; against a plain box, degenerate and
    inverted ones, infinite ones (which take -inf and leave +inf) and boxes with a NaN bound"""
    below = float(np.nextafter(10.0, 0.0))
    line = (0.0, -0.0, 5.0, below, 10.0, float(np.nextafter(10.0, 20.0)), float(np.nextafter(0.0, -1.0)), -3.0, NAN, INF, -INF)
    xy = np.array(list(itertools.product(line, line)))
    boxes = [(0, 10, 0, 10), (0, 0, 0, 10), (0, 10, 5, 5), (10, 0, 0, 10), (0, 10, 10, 0), (10, 0, 10, 0), (-INF, INF, -INF, INF),
             (-INF, 5, 0, INF), (INF, INF, 0, 10), (-INF, -INF, 0, 10), (NAN, 10, 0, 10), (0, NAN, 0, 10), (0, 10, NAN, 10), (0, 10, 0, NAN),
             (NAN, NAN, NAN, NAN), (0, below, 0, below), (-0.0, 10, -0.0, 10)]
    return [("edges", Windows(xy, np.array(boxes, np.float64)))]


def window_families():
    """[(family, [(name, Windows)])]"""
    return [(f.__name__, f()) for f in (window_sizes, window_edges)]


# ---- same_eager_signs ------------------------------------------------------------------------------------------------------------------------
def cross_product(p1, p2, p3):
    """src/helpers.py:435 before the rounding, operation for operation"""
    return (p2[..., 0] - p1[..., 0]) * (p3[..., 1] - p1[..., 1]) - (p2[..., 1] - p1[..., 1]) * (p3[..., 0] - p1[..., 0])


def numpy_round(x):
    return np.round(x, 3)


def round_half_up(x):
    """a planted wrong rounding: floor(x * 1000 + 0.5) / 1000 takes the ties up"""
    return np.floor(x * 1000.0 + 0.5) / 1000.0


def host_eager_signs(case, rounding=numpy_round):
    """src/helpers.py:425-441 over every combination of candidates: out[t, x, y, z] = sign(round(cross, 3)) of cand[tris[t, 0], x],
    cand[tris[t, 1], y], cand[tris[t, 2], z] as int8 (NaN: 0, the reference's else branch), 2 where any of the three is -1"""
    rxy = np.asarray(case.rxy, np.float64).reshape(-1, 2)
    tris, cand = np.asarray(case.tris, np.int64).reshape(-1, 3), np.asarray(case.cand, np.int64)
    k = cand.shape[1]
    r1, r2, r3 = np.broadcast_arrays(cand[tris[:, 0]][:, :, None, None], cand[tris[:, 1]][:, None, :, None], cand[tris[:, 2]][:, None, None, :])
    known = (r1 >= 0) & (r2 >= 0) & (r3 >= 0)
    if len(rxy) == 0:
        return np.full((len(tris), k, k, k), 2, np.int8)
    with np.errstate(all="ignore"):
        sign = np.sign(rounding(cross_product(rxy[np.where(known, r1, 0)], rxy[np.where(known, r2, 0)], rxy[np.where(known, r3, 0)])))
    return np.where(known, np.where(np.isnan(sign), 0.0, sign), 2.0).astype(np.int8)


EAGER_SIZES = ((1, 1), (1, 255), (1, 256), (1, 257), (1, 3000), (2, 31), (2, 32), (2, 33), (2, 500), (3, 9), (3, 10), (3, 150), (5, 2), (5, 3),
               (5, 33))                                  # (k, Tr): Tr * k**3 on and around 1, 256 and a few thousand


def eager_sizes(seed=51):
    """(k, Tr) of EAGER_SIZES over integer points in [-4, 4] (many crosses exactly zero), one candidate in eight -1; k = 1 with
    cand = arange, the form api._add_spatial_constraints_eager uses for the aligned side"""
    rng = np.random.default_rng(seed)
    out = []
    for k, Tr in EAGER_SIZES:
        n_m, n_r = 40, (40 if k == 1 else 23)
        cand = np.arange(n_m).reshape(-1, 1) if k == 1 else np.where(rng.random((n_m, k)) < 0.125, -1, rng.integers(0, n_r, (n_m, k)))
        out.append((f"k {k}, {Tr} triangles", Eager(rng.integers(-4, 5, (n_r, 2)).astype(np.float64), rng.integers(0, n_m, (Tr, 3)).astype(np.int32),
                                                    cand.astype(np.int32))))
    return out


def missing_candidates():
    """k = 3 over six rows: -1 in each position of a row, in two positions, a whole row of -1; every triple of rows as a triangle"""
    cand = np.array([(0, 1, 2), (-1, 1, 2), (0, -1, 2), (0, 1, -1), (-1, -1, 3), (-1, -1, -1)], np.int32)
    rxy = np.array([(0, 0), (5, 1), (2, 7), (-3, 2)], np.float64)
    return [("missing", Eager(rxy, np.array(list(itertools.product(range(6), repeat=3)), np.int32), cand))]


def rounding_points():
    """p1 = (0, 0), p2 = (1, 0), p3 = (0, y) for y in ROUNDING_Y: the cross is y exactly.  Then crosses that overflow: one product to +inf,
    to -inf, and both (inf - inf = NaN).  k = 1, cand = arange"""
    pts, tris = [(0.0, 0.0), (1.0, 0.0)], []
    for y in ROUNDING_Y:
        tris.append((0, 1, len(pts)))
        pts.append((0.0, y))
    big = len(pts)
    pts += [(1e200, 0.0), (0.0, 1e200), (0.0, -1e200), (1e200, 1e200)]
    tris += [(0, big, big + 1), (0, big, big + 2), (0, big + 3, big + 3), (0, big + 1, big)]
    return [("rounding", Eager(np.array(pts), np.array(tris, np.int32), np.arange(len(pts), dtype=np.int32).reshape(-1, 1)))]


def vertex_orders():
    """one triangle in all six vertex orders: the sign flips with the order's parity; a collinear one: 0 in every order"""
    rxy = np.array([(0, 0), (4, 0), (0, 3), (1, 1), (2, 2), (5, 5)], np.float64)
    tris = [o for o in ORDERS] + [tuple(3 + i for i in o) for o in ORDERS]
    return [("orders", Eager(rxy, np.array(tris, np.int32), np.arange(6, dtype=np.int32).reshape(-1, 1)))]


def order_parity(order):
    """+1 for an even permutation of (0, 1, 2), -1 for an odd one"""
    return 1 if tuple(order) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1


def eager_families():
    """[(family, [(name, Eager)])]"""
    return [(f.__name__, f()) for f in (eager_sizes, missing_candidates, rounding_points, vertex_orders)]


def flat(families):
    """[(family, [(name, case)])] -> [(family: name, case)]"""
    return [(f"{family}: {name}", case) for family, cases in families for name, case in cases]

