"""The host statement of same_merge_acc_score (csrc/window_score.hip) and the input families its library-level tests run it on.

`host_counts` is the call in plain numpy float64, written from the reference's text (src/eval_utils.py:116-121 the area, :160-166 the flip
rule, :199-211 the node rule) and include/same_hip.h's statement of the eight counts.  It imports nothing that ends in libsame_hip.

The families make what the product route never hands the call: areas that are exactly zero, NaN, infinite or decided by the last rounding,
label codes below zero, thousands of triangles around one row, a moving section larger than any scored before.  Each takes a `Job` (the
final rows of a merged accumulator and the job's own XY and joint label codes) and returns `Inputs` or a list of named `Inputs`.
tests/test_score_check_cpu.py checks, without a GPU, that each family has the property it was made for; tests/test_gpu_score_library.py
drives the library against `host_counts` on them.  Not collected by pytest."""
import collections
from fractions import Fraction

import numpy as np

Job = collections.namedtuple("Job", "a_row r_row mov_xy ref_xy code_m code_r")
Inputs = collections.namedtuple("Inputs", "mov_xy ref_xy code_m code_r tris")

TRI_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 769)
FAN = 3000                     # triangles around each hub row
GROWN_ROWS = 5000
# the node-local rule's points: thresholds at, just above and far from the hubs' ratios, and min_flips at and beyond the rule's edge
THRESHOLDS = (0.0, 0.5, float(np.nextafter(0.5, 1.0)), 1.0 / 3.0, 1.0, 1.5, -1.0, float("inf"))
MIN_FLIPS = (0, 1, 2, -3, 2**62 - 1)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def signed_area(p1, p2, p3):
    """src/eval_utils.py:116-121, its operations in its order, one IEEE operation each (numpy fuses nothing)"""
    return 0.5 * (p1[..., 0] * (p2[..., 1] - p3[..., 1]) + p2[..., 0] * (p3[..., 1] - p1[..., 1]) + p3[..., 0] * (p1[..., 1] - p2[..., 1]))


def host_triangles(a_row, r_row, mov_xy, ref_xy, code_m, tris, ignore_same):
    """per triangle of `tris` (rows of the moving section): (all three corners matched, same type and skipped, flipped, area before, area
    after); the flags of a triangle that is not all matched are False and its after-area NaN"""
    mov_xy, ref_xy = np.asarray(mov_xy, np.float64).reshape(-1, 2), np.asarray(ref_xy, np.float64).reshape(-1, 2)
    tris = np.zeros((0, 3), np.int64) if tris is None else np.asarray(tris, np.int64).reshape(-1, 3)
    match_of = np.full(len(mov_xy), -1, np.int64)
    match_of[np.asarray(a_row, np.int64)] = np.asarray(r_row, np.int64)
    m = match_of[tris]
    matched = (m >= 0).all(axis=1)
    c = np.asarray(code_m, np.int64)[tris]
    same = matched & bool(ignore_same) & (c[:, 0] >= 0) & (c[:, 0] == c[:, 1]) & (c[:, 0] == c[:, 2])       # a negative code equals nothing
    with np.errstate(all="ignore"):
        before = signed_area(mov_xy[tris[:, 0]], mov_xy[tris[:, 1]], mov_xy[tris[:, 2]])
        mm = np.where(m >= 0, m, 0)
        after = np.where(matched, signed_area(ref_xy[mm[:, 0]], ref_xy[mm[:, 1]], ref_xy[mm[:, 2]]), np.nan)
        s0, s1 = np.sign(before), np.sign(after)                 # the sign of NaN is NaN: unequal to everything, itself included
        flipped = matched & (s0 != s1) & (s0 != 0) & (s1 != 0)
    return matched, same, flipped, before, after


def node_rule(n_tri, n_flip, node_local, majority_threshold, min_flips):
    """src/eval_utils.py:187-200 per node, in Python's own numbers: ints compared as ints, the share a float64 quotient"""
    out = np.zeros(len(n_tri), bool)
    for i, (t, f) in enumerate(zip(np.asarray(n_tri).tolist(), np.asarray(n_flip).tolist())):
        if node_local:
            out[i] = t > 0 and f >= min_flips and (f / t) >= majority_threshold
        else:
            out[i] = f > 0
    return out


def host_counts(a_row, r_row, mov_xy, ref_xy, code_m, code_r, tris, ignore_same=True, node_local=False, majority_threshold=0.5,
                min_flips=1):
    """-> (the eight counts of include/same_hip.h as int64, node_tri, node_flip per moving row).  `tris` None: no triangle counts.
    A repeated corner counts once per occurrence; a final row's moving cell is counted under the node rule once."""
    a_row, r_row = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    code_m, code_r = np.asarray(code_m, np.int64), np.asarray(code_r, np.int64)
    n_mov = len(np.asarray(mov_xy).reshape(-1, 2))
    assert len(np.unique(a_row)) == len(a_row) and (len(a_row) == 0 or (0 <= a_row.min() and a_row.max() < n_mov))
    node_tri, node_flip = np.zeros(n_mov, np.int64), np.zeros(n_mov, np.int64)
    counts = np.zeros(8, np.int64)
    counts[0] = len(a_row)
    counts[1] = np.count_nonzero((code_m[a_row] >= 0) & (code_m[a_row] == code_r[r_row]))
    if tris is not None and len(tris):
        t = np.asarray(tris, np.int64).reshape(-1, 3)
        matched, same, flipped, _b, _a = host_triangles(a_row, r_row, mov_xy, ref_xy, code_m, t, ignore_same)
        np.add.at(node_tri, t[matched & ~same].reshape(-1), 1)
        np.add.at(node_flip, t[flipped & ~same].reshape(-1), 1)
        counts[2:7] = len(t), matched.sum(), same.sum(), flipped.sum(), (flipped & ~same).sum()
        counts[7] = np.count_nonzero(node_rule(node_tri[a_row], node_flip[a_row], node_local, majority_threshold, min_flips))
    return counts, node_tri, node_flip


def exact_sign(p1, p2, p3):
    """the sign of the area expression over the rationals (what correct rounding of the whole expression keeps)"""
    f = lambda v: Fraction(float(v))
    s = f(p1[0]) * (f(p2[1]) - f(p3[1])) + f(p2[0]) * (f(p3[1]) - f(p1[1])) + f(p3[0]) * (f(p1[1]) - f(p2[1]))
    return (s > 0) - (s < 0)


# ---- the families ------------------------------------------------------------------------------------------------------------------------
def _delaunay(xy):
    from scipy.spatial import Delaunay

    return Delaunay(xy).simplices.astype(np.int32)


def _copies(job):
    return job.mov_xy.copy(), job.ref_xy.copy(), job.code_m.copy(), job.code_r.copy()


def _once(job):
    """positions in the final rows whose reference row no other final row names (their mapped XY can be set row by row)"""
    _u, inverse, count = np.unique(job.r_row, return_inverse=True, return_counts=True)
    return np.flatnonzero(count[inverse] == 1)


def own(job):
    """the job's XY and joint codes, the Delaunay triangulation of the moving XY"""
    return Inputs(*_copies(job), _delaunay(job.mov_xy))


def mirrored(job):
    """ref X negated: every term of the after-area changes its sign exactly, so the after-area does"""
    mov, ref, cm, cr = _copies(job)
    ref[:, 0] = -ref[:, 0]
    return Inputs(mov, ref, cm, cr, _delaunay(job.mov_xy))


def line(job, seed=11):
    """every matched reference row on the line y = x / 3: seven in ten at an x that is a multiple of 3 (their areas are sums of small
    integers: exactly 0), the rest at a random x, where y is rounded and the area is whatever the roundings leave"""
    rng = np.random.default_rng(seed)
    mov, ref, cm, cr = _copies(job)
    rows = np.unique(job.r_row)
    x = np.where(rng.random(len(rows)) < 0.7, 3.0 * rng.integers(-300, 300, len(rows)), rng.uniform(-900.0, 900.0, len(rows)))
    ref[rows] = np.column_stack((x, x / 3.0))
    return Inputs(mov, ref, cm, cr, _delaunay(job.mov_xy))


def degenerate(job, seed=12):
    """own's triangles, then: triangles (a, a, b) and (a, b, a); moving triples on a line of small integers (before-area exactly 0); one
    triangle 300 times over, made to flip; triangles of unmatched rows alone (where the job has three)"""
    rng = np.random.default_rng(seed)
    mov, ref, cm, cr = _copies(job)
    tris = _delaunay(job.mov_xy)
    a = job.a_row.astype(np.int32)
    first = next(t for t in tris if np.isin(t, job.a_row[_once(job)]).all())          # its mapped XY: the moving triangle, X negated
    at = {int(r): i for i, r in enumerate(job.a_row)}
    for v in first:
        ref[job.r_row[at[int(v)]]] = (-mov[v, 0], mov[v, 1])
    pick = rng.permutation(a[~np.isin(a, first)])
    n_line = min(60, len(pick) // 6)
    on_line = pick[:3 * n_line].reshape(-1, 3)
    for q, t in enumerate(on_line):
        mov[t] = [(7 * q, 5 * q), (7 * q + 2, 5 * q + 2), (7 * q + 5, 5 * q + 5)]
    pairs = pick[3 * n_line:3 * n_line + 2 * min(60, len(pick) // 6)].reshape(-1, 2)
    twice = np.vstack((np.column_stack((pairs[:, 0], pairs[:, 0], pairs[:, 1])), np.column_stack((pairs[:, 0], pairs[:, 1], pairs[:, 0]))))
    lost = np.setdiff1d(np.arange(len(mov)), job.a_row).astype(np.int32)
    alone = lost[:3 * min(50, len(lost) // 3)].reshape(-1, 3)
    return Inputs(mov, ref, cm, cr, np.vstack((tris, twice, on_line, np.repeat(first[None], 300, axis=0), alone)).astype(np.int32))


def nonfinite(job, seed=13):
    """NaN, +inf and -inf over both XY (one row in twenty-five each, X or Y or both), and sixteen matched pairs of rows at (+-0.0, +-0.0)
    with every triangle among the first eight of them: areas that are +0.0 or -0.0"""
    rng = np.random.default_rng(seed)
    mov, ref, cm, cr = _copies(job)
    tris = _delaunay(job.mov_xy)
    for xy in (mov, ref):
        for value in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(xy), max(2, len(xy) // 25), replace=False)
            cols = rng.integers(0, 3, len(rows))
            xy[rows[cols != 1], 0] = value
            xy[rows[cols != 0], 1] = value
    zeros = rng.choice(_once(job), min(16, len(_once(job))), replace=False)
    signs = np.array([[0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]])
    for q, i in enumerate(zeros):
        mov[job.a_row[i]] = signs[q % 4]
        ref[job.r_row[i]] = signs[(q // 4 + q) % 4]
    z = job.a_row[zeros[:8]]
    among = np.array([(z[i], z[j], z[k]) for i in range(len(z)) for j in range(len(z)) for k in range(len(z)) if i != j != k != i][:200])
    return Inputs(mov, ref, cm, cr, np.vstack((tris, among.reshape(-1, 3))).astype(np.int32))


def _slivers(rng, n):
    """n triangles at offset 1e6 with side 1e-4, the third corner on the line through the first two plus 1e-10 noise -> (n, 3, 2)"""
    p1 = 1e6 + rng.random((n, 2))
    theta = rng.uniform(0.0, 2.0 * np.pi, n)
    d = 1e-4 * np.column_stack((np.cos(theta), np.sin(theta)))
    p2 = p1 + d
    p3 = p1 + rng.uniform(0.2, 0.8, n)[:, None] * d + 1e-10 * rng.standard_normal((n, 2))
    return np.stack((p1, p2, p3), axis=1)


def cancellation(job, seed=14):
    """disjoint triples of matched rows whose reference rows are named once, each a sliver far from the origin on both sides: the sign of
    the area is decided by the roundings of the reference's operation order; the triangles are these triples alone"""
    rng = np.random.default_rng(seed)
    mov, ref, cm, cr = _copies(job)
    pos = rng.permutation(_once(job))
    pos = pos[:3 * (len(pos) // 3)].reshape(-1, 3)
    mov[job.a_row[pos]] = _slivers(rng, len(pos))
    ref[job.r_row[pos]] = _slivers(rng, len(pos))
    return Inputs(mov, ref, cm, cr, job.a_row[pos].astype(np.int32))


def hub(job, seed=15):
    """two hub rows, each the first corner of FAN triangles (hub, rim, rim') over rim pairs of its own, FAN / pairs triangles per pair;
    the mapped positions of a pair are the moving positions -- or those of each other, which turns every triangle of the pair over.
    Half of the first hub's pairs are swapped (n_flip / n_tri == 0.5 exactly), a third of the second's (1 / 3); the hubs' codes are
    no rim's, so no triangle is skipped.  -> (Inputs, (first hub row, second hub row))"""
    rng = np.random.default_rng(seed)
    mov, ref, cm, cr = _copies(job)
    pos = rng.permutation(_once(job))
    pairs = next(p for p in (150, 60, 30, 12, 6) if 4 * p + 2 <= len(pos))
    tris, hubs = [], []
    for h, share in ((0, 2), (1, 3)):
        use = pos[h * (2 * pairs + 1):(h + 1) * (2 * pairs + 1)]
        centre, rim = use[0], use[1:].reshape(pairs, 2)
        c = np.array([400.0 * h, -250.0])
        angle = 2.0 * np.pi * (np.arange(2 * pairs).reshape(pairs, 2) + 0.25) / (2 * pairs)
        at = c + 10.0 * np.stack((np.cos(angle), np.sin(angle)), axis=-1)               # (pairs, 2, 2), counter-clockwise
        mov[job.a_row[centre]] = ref[job.r_row[centre]] = c
        mov[job.a_row[rim]] = at
        swapped = np.arange(pairs) < pairs // share
        ref[job.r_row[rim]] = np.where(swapped[:, None, None], at[:, ::-1], at)
        cm[job.a_row[centre]] = 1000 + h
        fan = np.column_stack((np.full(pairs, job.a_row[centre]), job.a_row[rim]))
        tris.append(np.tile(fan, (FAN // pairs, 1)))
        hubs.append(int(job.a_row[centre]))
    return Inputs(mov, ref, cm, cr, np.vstack(tris).astype(np.int32)), tuple(hubs)


def codes(job, seed=16):
    """own's XY and triangles under other codes -> [(name, Inputs)]"""
    rng = np.random.default_rng(seed)
    base = own(job)
    n_m, n_r = len(base.code_m), len(base.code_r)
    out = [("all equal", base._replace(code_m=np.full(n_m, 3, np.int32), code_r=np.full(n_r, 3, np.int32))),
           ("all distinct", base._replace(code_m=np.arange(n_m, dtype=np.int32), code_r=(n_m + np.arange(n_r)).astype(np.int32)))]
    cm, cr = base.code_m.copy(), base.code_r.copy()
    cm[rng.choice(n_m, n_m // 5, replace=False)] = rng.choice([-1, -2, -7, -2**31], n_m // 5)
    cr[rng.choice(n_r, n_r // 5, replace=False)] = rng.choice([-1, -2], n_r // 5)
    both = rng.choice(len(job.a_row), len(job.a_row) // 5, replace=False)
    cm[job.a_row[both]] = cr[job.r_row[both]] = -1
    matched, _s, _f, _b, _a = host_triangles(job.a_row, job.r_row, base.mov_xy, base.ref_xy, cm, base.tris, True)
    cm[base.tris[matched][:40].reshape(-1)] = -1                                      # triangles whose three corners are all -1
    out.append(("negative", base._replace(code_m=cm, code_r=cr)))
    top = np.int32(2**31 - 1)                                                             # the labels 0 and 1 become one, the largest code
    out.append(("largest", base._replace(code_m=np.where(base.code_m <= 1, top, base.code_m).astype(np.int32),
                                         code_r=np.where(base.code_r <= 1, top, base.code_r).astype(np.int32))))
    return out


def tri_counts(job):
    """the first k triangles of own at the block and wave edges (as many as own has), and no triangulation at all -> [(name, Inputs)]"""
    base = own(job)
    ks = sorted({min(k, len(base.tris)) for k in TRI_COUNTS})
    return [(f"{k} triangles", base._replace(tris=base.tris[:k])) for k in ks] + [("no triangulation", base._replace(tris=None))]


def grown(job, seed=17):
    """the moving section with GROWN_ROWS rows appended -- no final row names them --; own's triangles, then triangles of one, two and
    three of the new rows"""
    rng = np.random.default_rng(seed)
    base = own(job)
    n = len(base.mov_xy)
    mov = np.vstack((base.mov_xy, rng.uniform(base.mov_xy.min(), base.mov_xy.max(), (GROWN_ROWS, 2))))
    cm = np.concatenate((base.code_m, rng.integers(0, 3, GROWN_ROWS).astype(np.int32)))
    new = (n + rng.permutation(GROWN_ROWS)).astype(np.int32)
    old = rng.choice(job.a_row, (1500, 2)).astype(np.int32)
    mixed = np.vstack((np.column_stack((new[:1500], old)), np.column_stack((old[:, 0], new[1500:3000], new[3000:4500])),
                       new[-498:].reshape(-1, 3), np.column_stack((old[:500, 0], np.full(500, n + GROWN_ROWS - 1, np.int32), old[:500, 1]))))
    return Inputs(mov, base.ref_xy, cm, base.code_r, np.vstack((base.tris, mixed[rng.permutation(len(mixed))])).astype(np.int32))


def all_families(job):
    """[(name, Inputs)] of every family, in the issue's order"""
    out = [(f.__name__, f(job)) for f in (own, mirrored, line, degenerate, nonfinite, cancellation)]
    out.append(("hub", hub(job)[0]))
    out += [(f"codes: {name}", inp) for name, inp in codes(job)]
    out += [(f"tri_counts: {name}", inp) for name, inp in tri_counts(job)]
    out.append(("grown", grown(job)))
    return out


def small_families(job):
    """what a job of fewer rows than a block is run on"""
    out = [(f.__name__, f(job)) for f in (own, mirrored, degenerate)]
    return out + [(f"tri_counts: {name}", inp) for name, inp in tri_counts(job)]


def synthetic_job(n=1500, n_matched=1200, seed=0, n_types=6, jitter=4.0):
    """final rows without an accumulator: a random injective match of `n_matched` of `n` rows, the reference a jittered, shuffled copy"""
    rng = np.random.default_rng(seed)
    mov = rng.uniform(0.0, 400.0, (n, 2))
    perm = rng.permutation(n)
    ref = np.empty_like(mov)
    ref[perm] = mov + jitter * rng.standard_normal((n, 2))
    code_m = rng.integers(0, n_types, n).astype(np.int32)
    code_r = np.empty(n, np.int32)
    code_r[perm] = np.where(rng.random(n) < 0.85, code_m, (code_m + 1) % n_types)
    a_row = np.sort(rng.choice(n, n_matched, replace=False)).astype(np.int32)
    return Job(a_row, perm[a_row].astype(np.int32), mov, ref, code_m, code_r)
