"""Hostile inputs for the local search (same_amd/csrc/refine.hip) and the WRONG statements of its rule, for the tests only.

The oracle stays refine_check.refine / refine_capacity_check.refine: nothing here restates the round rule.  `case(name)` gives a family's
window as (kwargs of Problem / CapProblem, start, rounds_cap), seeded and deterministic; `statement(name)` runs the oracle on it once.
Costs, no-match costs, delaunay_penalty and penalty_coeff are multiples of 2^-30 at least (2^-20 but for `contested`) and sizes are
integers in every family of DYADIC: each sum is then exact in fp64 and the objectives compare bit for bit.

`run(kw, start, cap, wrong=...)` runs the oracle with ONE deviation a plausible kernel change would make (WRONG); the CPU test proves that
each gives another answer on the family TOLD_BY names, so a device that made it would fail there.

`batch_section()` is the section of the batched form's test: finish_check's nine windows and a dense tenth one; `window_kwargs` turns a
finished window's own arrays into the oracle's problem under the modes of BATCH_MODES.
"""
import contextlib
import functools
import itertools

import numpy as np

import refine_capacity_check as rcc
import refine_check as rc

Q = 2.0 ** -20
BIG_CAP = 10 ** 12
LIMITS = (1, 2, 3, rcc.MAX_LIMIT)


def _dyadic(x):
    return np.round(np.asarray(x, np.float64) / Q) * Q


def greedy_start(pairs, costs, unmatched, n, n_r, limit=None):
    """cheapest pairs first, a pair only below its cell's no-match cost and while its reference has room (one each without limits)"""
    start = np.full(n, -1, np.int32)
    room = np.ones(n_r, np.int64) if limit is None else np.asarray(limit, np.int64).copy()
    for p in np.argsort(costs, kind="stable"):
        i, j = pairs[p]
        if start[i] < 0 and room[j] > 0 and costs[p] < unmatched[i]:
            start[i], room[j] = p, room[j] - 1
    return start


def _made(kind, n, seed, **more):
    """refine_check.make_problem with its costs rounded to multiples of 2^-20 (the greedy start taken again on them)"""
    kw, _start = rc.make_problem(kind, n, seed=seed, **more)
    kw = dict(kw, costs=_dyadic(kw["costs"]))
    return kw, greedy_start(kw["pairs"], kw["costs"], kw["unmatched"], n, kw["n_r"])


# ---- the families -----------------------------------------------------------------------------------------------------------------------
def fan(m):
    """a hub (cell 0) and m rim cells on a circle, triangles (hub, r, r + 1) all the way round: the hub has degree m, every footprint
    holds the hub's slot, so one move wins per round.  Every cell starts unmatched with one pair, to a reference of its own, cheaper than
    its no-match cost by more than every flip can cost (m * 9 * 2^-12 < 0.7): m + 1 rounds of one move.  Every fifth rim cell's reference
    lies across the hub, so triangles flip on the way."""
    n = m + 1
    ang = 2.0 * np.pi * np.arange(m) / m
    axy = np.vstack(([[0.0, 0.0]], 10.0 * np.column_stack((np.cos(ang), np.sin(ang)))))
    ref_xy = axy.copy()
    ref_xy[1::5] *= -1.0
    size = 1.0 + (np.arange(n) % 3)
    costs = (1.0 + np.random.default_rng(m).permutation(n)) * 2.0 ** -10         # distinct, below 0.3
    rim = 1 + np.arange(m)
    tris = np.column_stack((np.zeros(m, np.int64), rim, 1 + (rim % m))).astype(np.int32)
    pairs = np.column_stack((np.arange(n), np.arange(n))).astype(np.int32)
    kw = dict(pairs=pairs, costs=costs, unmatched=3.0 * size, n=n, n_r=n, triangles=tris, axy=axy, ref_xy=ref_xy, size=size,
              delaunay_penalty=2.0 ** -12)
    return kw, np.full(n, -1, np.int32)


def contested(m):
    """2 m references, each wanted by two unmatched cells i = 2 j < k = 2 j + 1 with one pair each, no-match cost 3.  The first m:
    cost(k) = cost(i) - 2^-30 around 0.5 -- in fp64 k's delta is the lower one, rounded to float the two are equal and the rule gives
    the reference to i.  The other m: cost(k) = cost(i) - 2^-10, so k wins under either rule.  The cells sit on a jittered grid under
    scipy's triangulation, each reference beside its two cells."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(1000 + m)
    n, n_r = 4 * m, 2 * m
    s = int(np.ceil(np.sqrt(n)))
    axy = np.column_stack((np.arange(n) % s, np.arange(n) // s)).astype(np.float64) + rng.normal(0, 0.05, (n, 2))
    ref_xy = 0.5 * (axy[0::2] + axy[1::2]) + rng.normal(0, 0.3, (n_r, 2))
    j = np.arange(n_r)
    ci = 0.5 + j * 2.0 ** -10
    ck = ci - np.where(j < m, 2.0 ** -30, 2.0 ** -10)
    costs = np.column_stack((ci, ck)).reshape(-1)
    pairs = np.column_stack((np.arange(n), np.arange(n) // 2)).astype(np.int32)
    size = np.ones(n)
    kw = dict(pairs=pairs, costs=costs, unmatched=3.0 * size, n=n, n_r=n_r, triangles=Delaunay(axy).simplices.astype(np.int32), axy=axy,
              ref_xy=ref_xy, size=size, delaunay_penalty=5.0)
    return kw, np.full(n, -1, np.int32)


def scaled(e):
    """make_problem("uniform", 257, seed=3) with every cost, no-match cost and the penalty times 2^e (exact): the same search at every e,
    its deltas f32 subnormals at e = -140 and beyond float's range at e = +130 (every key ties, the cell decides)"""
    kw, start = rc.make_problem("uniform", 257, seed=3)
    s = 2.0 ** e
    return dict(kw, costs=kw["costs"] * s, unmatched=kw["unmatched"] * s, delaunay_penalty=kw["delaunay_penalty"] * s), start


@functools.lru_cache(maxsize=None)
def _tri_base():
    return _made("clustered", 300, 5)


def _corner_orders(tris, rng):
    orders = np.array(list(itertools.permutations(range(3))))           # the rotations and the reversals
    return np.take_along_axis(tris, orders[rng.integers(0, 6, len(tris))], axis=1)


def triangle_list(how):
    """one clustered window of 300 cells under a triangle list the host form accepts: as it is / rows shuffled, corners rotated or
    reversed / every triangle twice and a third of them three times / corners named twice added / 5 n triangles / none"""
    kw, start = _tri_base()
    tris, n = np.asarray(kw["triangles"]), kw["n"]
    rng = np.random.default_rng(77)
    if how == "shuffled":
        tris = _corner_orders(tris[rng.permutation(len(tris))], rng)
    elif how == "doubled":
        tris = np.vstack((tris, tris, tris[::3]))
        tris = _corner_orders(tris[rng.permutation(len(tris))], rng)
    elif how == "corner twice":
        a, b = tris[:80, 0], tris[:80, 1]
        tris = np.vstack((tris, np.column_stack((a, a, b)), np.column_stack((a, b, a)), np.column_stack((b, a, a))))
        tris = tris[rng.permutation(len(tris))]
    elif how == "long":
        a = rng.integers(0, n, 5 * n - len(tris))
        more = np.column_stack((a, (a + rng.integers(1, 10, len(a))) % n, (a + rng.integers(10, 20, len(a))) % n))
        tris = np.vstack((tris, more))
        tris = tris[rng.permutation(len(tris))]
        assert len(tris) == 5 * n
    elif how == "none":
        tris = np.zeros((0, 3), np.int32)
    else:
        assert how == "as is"
    return dict(kw, triangles=np.ascontiguousarray(tris, np.int32)), start


def collinear():
    """a lattice window WITHOUT its jitter: the triangulation of the jittered cells (its thin hull triangles now exactly collinear) and
    every third collinear triple along a row, a column or a diagonal -- triangles whose source sign is 0"""
    kw, start = _made("lattice", 300, 6)
    n = kw["n"]
    s = int(np.ceil(np.sqrt(n)))
    axy = np.round(kw["axy"])
    i = np.arange(n)
    rows = i[(i % s <= s - 3) & (i + 2 < n)]
    cols = i[i + 2 * s < n]
    diag = i[(i % s <= s - 3) & (i + 2 * s + 2 < n)]
    more = np.vstack((np.column_stack((rows, rows + 1, rows + 2)), np.column_stack((cols + 2 * s, cols, cols + s)),
                      np.column_stack((diag + s + 1, diag + 2 * s + 2, diag))))[::3]
    tris = np.vstack((kw["triangles"], more))
    tris = tris[np.random.default_rng(78).permutation(len(tris))]
    return dict(kw, axy=axy, triangles=np.ascontiguousarray(tris, np.int32)), start


def shuffled_pairs():
    """triangle_list("as is") with its pair rows in a random order and the start renumbered to match (the library's `order` and `where`
    maps are no longer the identity).  The statement keeps the caller's order within a cell, so it is the oracle ON THIS LIST."""
    kw, start = _tri_base()
    perm = np.random.default_rng(79).permutation(len(kw["pairs"]))
    inv = np.argsort(perm)
    return dict(kw, pairs=kw["pairs"][perm], costs=kw["costs"][perm]), np.where(start >= 0, inv[np.maximum(start, 0)], -1).astype(np.int32)


def sized(n):
    return _made(("uniform", "clustered", "lattice")[n % 3], n, n)


def cap_sized(n, n_r, seed=0, limits=LIMITS, penalty_coeff=2.0 ** -3, fill=False):
    """n cells (make_problem's) and n_r references scattered over them, up to 4 nearest references as pairs, limits drawn from `limits`;
    the start one-to-one (none matched where the cells are fewer than ten: that start would be the optimum), or with `fill` greedy
    within the limits (references filled to their limit exactly)"""
    from scipy.spatial import cKDTree

    kw, _start = rc.make_problem("uniform", n, seed=seed)
    rng = np.random.default_rng(2000 + seed)
    ref_xy = rng.uniform(0, np.sqrt(n), (n_r, 2))
    k = min(4, n_r)
    d, j = cKDTree(ref_xy).query(kw["axy"], k=k)
    pairs = np.column_stack((np.repeat(np.arange(n), k), np.reshape(j, -1))).astype(np.int32)
    costs = _dyadic(np.reshape(d, -1))
    limit = rng.choice(np.asarray(limits, np.int32), n_r)
    start = greedy_start(pairs, costs, kw["unmatched"], n, n_r, limit if fill else None)
    if n < 10:
        start[:] = -1
    return dict(kw, pairs=pairs, costs=costs, n_r=n_r, ref_xy=ref_xy, limit=limit, penalty_coeff=penalty_coeff), start


LEAVERS = 4


def filled():
    """cap_sized(300, 60) from the greedy start within its limits, and beside it LEAVERS references of limit 2 held by two cells each
    that share no triangle; either cell would leave for a free reference of its own at a cost up by less than penalty_coeff.  Both
    count the reference's one penalty as theirs: the leavers' claim on the reference they leave lets one go per round, and the other
    then stays."""
    kw, start = cap_sized(300, 60, seed=4, limits=(1, 2, 3), fill=True)
    n, n_r, P, g = kw["n"], kw["n_r"], len(kw["pairs"]), np.arange(LEAVERS)
    a, o = n + 2 * g, n_r + 3 * g
    pairs = np.column_stack((np.stack((a, a, a + 1, a + 1), 1).reshape(-1), np.stack((o, o + 1, o, o + 2), 1).reshape(-1)))
    costs = np.tile([0.5, 0.5 + 2.0 ** -4, 0.5, 0.5 + 2.0 ** -5], LEAVERS)
    xy = np.column_stack((1000.0 + 10.0 * np.arange(3 * LEAVERS), np.zeros(3 * LEAVERS)))
    out = dict(kw, pairs=np.vstack((kw["pairs"], pairs)).astype(np.int32), costs=np.concatenate((kw["costs"], costs)),
               unmatched=np.concatenate((kw["unmatched"], np.full(2 * LEAVERS, 3.0))), n=n + 2 * LEAVERS, n_r=n_r + 3 * LEAVERS,
               axy=np.vstack((kw["axy"], xy[:2 * LEAVERS])), ref_xy=np.vstack((kw["ref_xy"], xy)),
               size=np.concatenate((kw["size"], np.ones(2 * LEAVERS))),
               limit=np.concatenate((kw["limit"], np.tile([2, 1, 1], LEAVERS))).astype(np.int32))
    return out, np.concatenate((start, P + 2 * np.arange(2 * LEAVERS))).astype(np.int32)


def empty(n, n_r, P, Tr):
    """the smallest calls: cells on a triangle, references across the Y axis, pair p = (p, p) at cost 1/4"""
    axy = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]])[:n]
    ref_xy = (np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [1.0, 1.0], [2.0, 2.0]]) * (-1.0, 1.0))[:n_r]
    pairs = np.column_stack((np.arange(P), np.arange(P))).astype(np.int32)
    tris = np.array([[2, 0, 1]], np.int32)[:Tr]
    size = np.arange(1.0, n + 1.0)
    kw = dict(pairs=pairs, costs=np.full(P, 0.25), unmatched=3.0 * size, n=n, n_r=n_r, triangles=tris, axy=axy, ref_xy=ref_xy, size=size,
              delaunay_penalty=5.0)
    return kw, np.full(n, -1, np.int32)


FRACTIONS = (0.1, 0.3, 0.7, 2.5)


def _order_gadget(dp):
    """sizes of a cell c and of the corners (a_k, b_k) of three triangles (c, a_k, b_k), and an order of the three, such that
    dp * (-w_1 - w_2 - w_3) summed in the order of the sorted corners and summed in that order differ in fp64
    -> (sizes (7,), order, the two deltas)"""
    for sz in itertools.product(FRACTIONS, repeat=7):
        w = [(sz[0] + sz[2 * k + 1]) + sz[2 * k + 2] for k in range(3)]
        for order in itertools.permutations(range(3)):
            by_corners = dp * (((0.0 - w[0]) - w[1]) - w[2])
            by_index = dp * (((0.0 - w[order[0]]) - w[order[1]]) - w[order[2]])
            if by_corners != by_index:
                return np.array(sz), order, by_corners, by_index
    raise AssertionError("no such sizes")


def fractional():
    """a uniform window with sizes from {0.1, 0.3, 0.7, 2.5} and decimal costs (F is a rounded sum: its ORDER counts), and beside it seven
    cells where the order decides a move: cell c holds a reference under which its three triangles flip; pair A unflips all three at
    the same cost (delta = delaunay_penalty * F), pair B keeps them at a cost lower by exactly the smaller of F's two orders' deltas.
    A is considered first and B must be strictly better, so c goes to A or to B by the last bit of F."""
    kw, _start = rc.make_problem("uniform", 300, seed=8)
    rng = np.random.default_rng(80)
    n, n_r, dp = kw["n"], kw["n_r"], kw["delaunay_penalty"]
    size = rng.choice(np.asarray(FRACTIONS), n)
    unm = 3.0 * size
    start = greedy_start(kw["pairs"], kw["costs"], unm, n, n_r)
    gs, order, by_corners, by_index = _order_gadget(dp)
    lo = min(by_corners, by_index)
    held = 2.0 ** np.ceil(np.log2(-lo))                   # c's cost now and on A; B's = held + lo, exact both ways
    assert (held + lo) - held == lo and held + lo >= 0.0
    x0 = 1000.0
    ring = np.array([[x0 + 3.0 * k + h, 0.0] for k in range(3) for h in (0.0, 1.0)])
    axy = np.vstack((kw["axy"], [[x0 + 5.0, 1.0]], ring))
    ref_xy = np.vstack((kw["ref_xy"], [[x0 + 5.0, -1.0], [x0 + 5.0, 1.0], [x0 + 5.5, -1.0]], ring))
    c = n
    tris = np.array([[c, c + 2 * k + 1, c + 2 * k + 2] for k in order], np.int32)
    pairs = np.vstack((kw["pairs"], [[c, n_r], [c, n_r + 1], [c, n_r + 2]], [[c + 1 + q, n_r + 3 + q] for q in range(6)])).astype(np.int32)
    P = len(kw["pairs"])
    costs = np.concatenate((kw["costs"], [held, held, held + lo], np.full(6, 0.25)))
    out = dict(kw, pairs=pairs, costs=costs, unmatched=np.concatenate((unm, np.full(7, 100.0))), n=n + 7, n_r=n_r + 9,
               triangles=np.vstack((kw["triangles"], tris)).astype(np.int32), axy=axy, ref_xy=ref_xy, size=np.concatenate((size, gs)))
    start = np.concatenate((start, [P], P + 3 + np.arange(6))).astype(np.int32)
    return out, start


def signed():
    kw, _start = _made("uniform", 300, 9)
    costs = kw["costs"] - 0.5
    return dict(kw, costs=costs), greedy_start(kw["pairs"], costs, kw["unmatched"], kw["n"], kw["n_r"])


def with_capacity(made, seed, penalty_coeff):
    kw, start = made
    limit = np.random.default_rng(3000 + seed).choice(np.asarray(LIMITS, np.int32), kw["n_r"])
    return dict(kw, limit=limit, penalty_coeff=penalty_coeff), start


FAN_CAPS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, BIG_CAP)
SCALES = (-140, 0, 130)
TRIANGLE_LISTS = ("as is", "shuffled", "doubled", "corner twice", "long", "none")
SIZES = (255, 256, 257, 511, 512, 513)
CAP_SIZES = ((200, 56), (200, 57), (5, 1000), (600, 3))
EMPTY = ((0, 0, 0, 0), (0, 5, 0, 0), (1, 0, 0, 0), (1, 1, 1, 0), (3, 3, 3, 1))
PENALTY_COEFFS = (0.0, 2.0 ** -3, 100.0)

_BUILD = {}
_BUILD.update({f"fan/40/cap={c}": (lambda c=c: (*fan(40), c)) for c in FAN_CAPS})
_BUILD["fan/300"] = lambda: (*fan(300), 400)
_BUILD["contested/50"] = lambda: (*contested(50), 64)
_BUILD.update({f"scaled/{e}": (lambda e=e: (*scaled(e), 32)) for e in SCALES})
_BUILD.update({f"triangles/{how}": (lambda how=how: (*triangle_list(how), 64)) for how in TRIANGLE_LISTS})
_BUILD["triangles/collinear"] = lambda: (*collinear(), 64)
_BUILD["pairs/shuffled"] = lambda: (*shuffled_pairs(), 64)
_BUILD.update({f"size/n={n}": (lambda n=n: (*sized(n), 64)) for n in SIZES})
_BUILD.update({f"size/n={n},n_r={r}": (lambda n=n, r=r: (*cap_sized(n, r, seed=n + r), 64)) for n, r in CAP_SIZES})
_BUILD.update({"empty/" + "-".join(map(str, e)): (lambda e=e: (*empty(*e), 8)) for e in EMPTY})
_BUILD["fractional"] = lambda: (*fractional(), 64)
_BUILD["signed"] = lambda: (*signed(), 64)
for _q, _pc in enumerate(PENALTY_COEFFS):
    _BUILD[f"capacity/contested/pc={_pc}"] = lambda q=_q, pc=_pc: (*with_capacity(contested(50), q, pc), 64)
    _BUILD[f"capacity/fan/pc={_pc}"] = lambda q=_q, pc=_pc: (*with_capacity(fan(40), 10 + q, pc), BIG_CAP)
_BUILD["capacity/filled"] = lambda: (*filled(), 64)

NAMES = tuple(_BUILD)
EMPTY_NAMES = tuple(n for n in NAMES if n.startswith("empty/"))
NOT_DYADIC = tuple(n for n in NAMES if n.startswith("scaled/")) + ("fractional",)
DYADIC = tuple(n for n in NAMES if n not in NOT_DYADIC)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (kwargs of Problem, or of CapProblem where they hold `limit`; start; rounds_cap)"""
    kw, start, cap = _BUILD[name]()
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    start.flags.writeable = False
    return kw, start, cap


def is_cap(kw):
    return "limit" in kw


# ---- the wrong statements: one deviation each -------------------------------------------------------------------------------------------
def _f32_word(delta):
    with np.errstate(over="ignore", under="ignore"):
        return int(np.array([delta], dtype=np.float32).view(np.uint32)[0])


def _ordered(u):
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


def _key_fp64(delta, i):
    return (delta, i)                       # (compared as a tuple: only min and == are taken of a key)


def _key_flushed(delta, i):
    u = _f32_word(delta)
    if (u & 0x7F800000) == 0:               # a subnormal: flushed to a signed zero
        u &= 0x80000000
    return (_ordered(u) << 32) | i


def _key_high_cell(delta, i):
    return (_ordered(_f32_word(delta)) << 32) | (0xFFFFFFFF - i)


KEYS = {"key by the fp64 delta": _key_fp64, "key flushed below 2^-126": _key_flushed, "ties to the higher cell": _key_high_cell}


def _once(kw):
    """duplicate triangles counted once"""
    t = np.sort(np.asarray(kw["triangles"], np.int64).reshape(-1, 3), axis=1)
    return dict(kw, triangles=np.unique(t, axis=0))


class _SignAsGiven:
    """the source sign taken over the corners as given"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        given = (a[5] if len(a) > 5 else kw["triangles"])
        self.sign = [rc._orient(*(self.axy[int(v)] for v in t)) for t in np.asarray(given, np.int64).reshape(-1, 3)]


class _NoSkip:
    """the swap's second cell does not skip the triangles it shares with the first"""

    def _flip_part(self, m, cells, change):
        F = W = 0.0
        for c in cells:
            f, w = super()._flip_part(m, [c], change)
            F, W = F + f, W + w
        return F, W


class _OldNotClaimed:
    """a single move does not claim the reference it leaves (capacity only)"""

    def cap_footprint(self, i, po, pn, k, pk):
        return self.footprint(i, pn, k, pk)


class _ByIndex:
    """each cell's incident triangles in the order of their index, not of their sorted corners"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.inc = [sorted(l) for l in self.inc]


MIXINS = {"sign over the corners as given": _SignAsGiven, "second cell does not skip": _NoSkip,
          "old reference not claimed": _OldNotClaimed, "incidence by triangle index": _ByIndex}
WRONG = tuple(KEYS) + ("duplicates counted once",) + tuple(MIXINS)
# the family on which each wrong statement gives another answer (tests/test_refine_hostile_check_cpu.py proves it)
TOLD_BY = {"key by the fp64 delta": "contested/50", "key flushed below 2^-126": "scaled/-140", "ties to the higher cell": "contested/50",
           "duplicates counted once": "triangles/doubled", "sign over the corners as given": "triangles/shuffled",
           "second cell does not skip": "triangles/as is", "old reference not claimed": "capacity/filled",
           "incidence by triangle index": "fractional"}


@contextlib.contextmanager
def _keyed(fn):
    old = rc._key, rcc._key
    rc._key = rcc._key = fn
    try:
        yield
    finally:
        rc._key, rcc._key = old


def problem(kw, wrong=None):
    base = rcc.CapProblem if is_cap(kw) else rc.Problem
    if wrong == "duplicates counted once":
        kw = _once(kw)
    if wrong in MIXINS:
        base = type("Wrong", (MIXINS[wrong], base), {})
    return base(**kw)


def run(kw, start, cap, wrong=None):
    """the oracle's (matching, stats) -- refine_capacity_check's where kw holds limits -- or with `wrong` (one of WRONG) that deviation's.
    (the oracle's key casts through numpy: beyond float's range that warns, which is silenced here)"""
    assert wrong is None or wrong in WRONG
    prob = problem(kw, wrong)
    refine = rcc.refine if is_cap(kw) else rc.refine
    with np.errstate(over="ignore", under="ignore"), _keyed(KEYS.get(wrong, rc._key)):
        return refine(prob, start, cap)


@functools.lru_cache(maxsize=None)
def statement(name):
    return run(*case(name))


def answer(match, st):
    """what two runs are compared by"""
    return (tuple(int(p) for p in match), st["rounds"], st["moves"], st["settled"])


def deltas_of_round_one(kw, start):
    """{cell: its best move's fp64 delta} at the start"""
    prob = problem(kw)
    m = [int(p) for p in start]
    if is_cap(kw):
        count = prob.counts(m)
        best = {i: prob.cap_best(m, count, i) for i in range(prob.n)}
    else:
        owner = prob.owners(m)
        best = {i: prob.best(m, owner, i) for i in range(prob.n)}
    return {i: b[0] for i, b in best.items() if b is not None}


# ---- the batched window form -------------------------------------------------------------------------------------------------------------
BATCH_DENSE = 9                     # the tenth window's index
BATCH_DELAUNAY_PENALTY, BATCH_MAX_MATCHES = 5.0, 2
# optim_params of the batch's modes; at penalty_coeff 1 most windows hold a reference twice, at 4 only the tenth does and window 0 is
# left as it started
BATCH_MODES = {"local": dict(hip_refine="local", delaunay_penalty=BATCH_DELAUNAY_PENALTY),
               "capacity/1": dict(hip_refine="capacity", delaunay_penalty=BATCH_DELAUNAY_PENALTY, max_matches=BATCH_MAX_MATCHES,
                                  penalty_coeff=1.0),
               "capacity/4": dict(hip_refine="capacity", delaunay_penalty=BATCH_DELAUNAY_PENALTY, max_matches=BATCH_MAX_MATCHES,
                                  penalty_coeff=4.0)}
BATCH_ROUNDS = 32                   # window_mode.REFINE_ROUNDS, the modes' rounds cap


@functools.lru_cache(maxsize=None)
def batch_section():
    """finish_check.batch_section()'s nine windows (one without triangles, one without a kept cell, the knife window) and a tenth box:
    37 cells on a hexagonal patch of step 5 (every angle 60 degrees: the batch's 45-degree rule keeps its triangles, which it would not
    keep of a fan with more than seven rim cells) whose references are the cells jittered by 3.5, most of the spacing.  Every closed
    1-ring reaches across a good part of the patch, so its many improving moves go a few per round: the search there runs on past the
    rounds enqueued up front while the windows beside it settle at once."""
    from scipy.spatial import Delaunay

    import finish_check as F

    base = F.batch_section()
    rng = np.random.default_rng(8)
    x0 = F.BATCH_WINDOWS * F.BATCH_PITCH
    rings, step = 3, 5.0
    hexes = np.array([(step * (a + 0.5 * b), step * np.sqrt(3.0) / 2.0 * b) for a in range(-rings, rings + 1)
                      for b in range(-rings, rings + 1) if abs(a + b) <= rings])
    m = hexes + (x0 + 45.0, 45.0) + rng.normal(0, 0.05, hexes.shape)
    r = m + rng.normal(0, 3.5, m.shape)
    tid = rng.integers(0, 3, len(m)).astype(np.int32)
    size = rng.integers(1, 4, len(m))
    return F._section(np.vstack((base["mov_xy"], m)), np.vstack((base["ref_xy"], r)), np.concatenate((base["type_id"], tid)),
                      size=np.concatenate((base["size"], size)), box=(-1.0, x0 + 100.0, -1.0, 91.0),
                      boxes=base["boxes"] + ((x0, x0 + F.BATCH_PITCH - 10.0, 0.0, 90.0),), tris=base["tris"] + (F._tris(Delaunay(m).simplices),),
                      first=base["first"] + (len(base["mov_xy"]),))


def window_kwargs(pairs, costs, size, triangles, axy, ref_xy, limit=None, penalty_coeff=None):
    """a finished window's own arrays as the kwargs of Problem (or, with limits, of CapProblem) under the batch's modes"""
    import finish_check as F

    n, n_r = len(axy), len(ref_xy)

    kw = dict(pairs=np.asarray(pairs).reshape(-1, 2), costs=costs, unmatched=F.PENALTY * np.asarray(size, np.float64), n=n, n_r=n_r,
              triangles=np.asarray(triangles).reshape(-1, 3), axy=axy, ref_xy=ref_xy, size=size, delaunay_penalty=BATCH_DELAUNAY_PENALTY)
    if limit is not None:
        kw.update(limit=limit, penalty_coeff=penalty_coeff)
    return kw


def mode_kwargs(name, n_r):
    """window_kwargs' last two arguments under a mode of BATCH_MODES: the references carry no sizes, so every limit is max_matches"""
    if name == "local":
        return {}
    return dict(limit=np.full(n_r, BATCH_MAX_MATCHES, np.int32), penalty_coeff=BATCH_MODES[name]["penalty_coeff"])


def cpu_window(case, w, oracle):
    """window w of batch_section() on the host: None where it has no kept cell or comes back near, else (window_kwargs' first six
    arguments, the greedy start as pairs)"""
    import finish_check as F

    st = F.cpu_staged(case, oracle, box=case["boxes"][w])
    if len(st["rows"]) == 0:
        return None
    want = F.of_case(case, st, case["tris"][w], F.BATCH_FILTER, oracle)
    if want["near"]:
        return None
    return (st["pairs"], st["costs"], case["size"][st["rows"]], want["tris"], st["xy"], case["ref_xy"][st["rows_r"]]), want["match_pair"]
