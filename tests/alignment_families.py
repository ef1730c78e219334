"""Seeded (query, template) point families for eval_utils.check_alignment (csrc/align.hip), each built for one branch of the kernel's
grid and early stop, and the two labellings the geometry tests run them under.  No tests in here.

Labellings.  "random": 5 labels drawn at random on both sides.  "rank": the rank probe -- template codes are the template's row
numbers, and a query's code is the row of its exact k-th nearest template point (the match bit must be True) or of its (k+1)-th (it
must be False), both from one cKDTree query at k + 1; every undoubted row's bit then depends on where exactly the k-th boundary falls.
"""
import math
from dataclasses import dataclass

import numpy as np

ALL_KS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 63, 64)
LABELLINGS = ("random", "rank")
ABSENT = -5   # a query code no template row carries (the (k+1)-th probe where the template has only k rows)
NT, NQ = 2000, 1500
WORKERS = 8


@dataclass(frozen=True)
class Family:
    name: str
    branch: str          # what in align.hip it is there for
    qxy: np.ndarray
    txy: np.ndarray
    degenerate: bool = False   # rows in doubt are expected (exact ties, or d2 outside the range of a double)


def _rng(name, seed):
    return np.random.default_rng([seed, *name.encode()])


def _inside_and_near(rng, txy, n_q, lo, hi):
    """70 % uniform in [lo, hi], 30 % a template point moved by about a tenth of the mean spacing"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    n_near = (3 * n_q) // 10
    u = lo + rng.random((n_q - n_near, 2)) * (hi - lo)
    step = 0.1 * max(hi - lo) / math.sqrt(len(txy))
    near = txy[rng.integers(0, len(txy), n_near)] + rng.normal(0.0, 1.0, (n_near, 2)) * step
    return np.concatenate((u, near))


def _line(name, axis, n_q, n_t, seed):
    rng = _rng(name, seed)
    t = np.empty((n_t, 2))
    t[:, axis] = rng.random(n_t) * 1000.0
    t[:, 1 - axis] = 37.25
    q = np.empty((n_q, 2))
    q[:, axis] = rng.random(n_q) * 1100.0 - 50.0
    q[:, 1 - axis] = 37.25 + np.where(rng.random(n_q) < 0.5, 0.0, rng.normal(0.0, 30.0, n_q))   # half of them on the line itself
    return q, t


def _hline(n_q, n_t, seed):
    return _line("hline", 0, n_q, n_t, seed)


def _vline(n_q, n_t, seed):
    return _line("vline", 1, n_q, n_t, seed)


def _single_point(n_q, n_t, seed):
    rng = _rng("single_point", seed)
    return rng.normal(0.0, 5.0, (n_q, 2)) + (3.5, -2.25), np.tile((3.5, -2.25), (n_t, 1))


def _aniso(n_q, n_t, seed):
    rng = _rng("aniso", seed)
    t = rng.random((n_t, 2)) * (1e6, 1.0)
    q = _inside_and_near(rng, t, n_q, (-1e4, -2.0), (1.01e6, 3.0))
    return q, t


def _offset(name, off, ext):
    def gen(n_q, n_t, seed):
        rng = _rng(name, seed)
        t = off + rng.random((n_t, 2)) * ext
        return _inside_and_near(rng, t, n_q, (off - 0.05 * ext,) * 2, (off + 1.05 * ext,) * 2), t
    return gen


CLUSTER_AT, CLUSTER_SIDE, CLUSTER_BOX = np.array((3000.25, -1234.75)), 1.0, 1e4   # the cluster's share of the box: 2.5e-9


def _cluster_outliers(n_q, n_t, seed):
    rng = _rng("cluster_outliers", seed)
    n_c = (9 * n_t) // 10
    t = np.concatenate((CLUSTER_AT + rng.random((n_c, 2)) * CLUSTER_SIDE, (rng.random((n_t - n_c, 2)) * 2 - 1) * CLUSTER_BOX))
    n_in, n_ring = (4 * n_q) // 10, n_q // 5
    q_in = CLUSTER_AT + rng.random((n_in, 2)) * 3 * CLUSTER_SIDE - CLUSTER_SIDE
    ang, dist = rng.random(n_ring) * 2 * math.pi, 10.0 ** (rng.random(n_ring) * 4)
    q_ring = CLUSTER_AT + 0.5 * CLUSTER_SIDE + np.column_stack((np.cos(ang), np.sin(ang))) * dist[:, None]
    q_far = (rng.random((n_q - n_in - n_ring, 2)) * 2 - 1) * CLUSTER_BOX
    return np.concatenate((q_in, q_ring, q_far)), t


OUTSIDE_EXT = 100.0


def _outside(n_q, n_t, seed):
    """queries beyond each side and each corner of the template's box, from 1e-9 extents outside to 1e3 extents away"""
    rng = _rng("outside", seed)
    t = rng.random((n_t, 2)) * OUTSIDE_EXT
    t[:4] = ((0, 0), (OUTSIDE_EXT, 0), (0, OUTSIDE_EXT), (OUTSIDE_EXT, OUTSIDE_EXT))   # pins the box
    dirs = [(sx, sy) for sx in (-1, 0, 1) for sy in (-1, 0, 1) if (sx, sy) != (0, 0)]
    d = np.array(dirs)[np.arange(n_q) % 8]
    away = OUTSIDE_EXT * 10.0 ** (rng.random((n_q, 2)) * 12 - 9)
    along = rng.random((n_q, 2)) * OUTSIDE_EXT
    q = np.where(d < 0, -away, np.where(d > 0, OUTSIDE_EXT + away, along))
    return q, t


def _scale(name, s):
    def gen(n_q, n_t, seed):
        rng = _rng(name, seed)
        return rng.random((n_q, 2)) * s, rng.random((n_t, 2)) * s
    return gen


def _lattice(n_q, n_t, seed):
    rng = _rng("lattice", seed)
    side = math.isqrt(n_t - 1) + 1
    gx, gy = np.meshgrid(np.arange(side, dtype=float), np.arange(side, dtype=float))
    t = np.column_stack((gx.ravel(), gy.ravel()))[:n_t]   # the last lattice row may be short
    base = rng.integers(0, side - 1, (n_q, 2)).astype(float)
    kind = np.arange(n_q) % 4   # on a lattice point, an edge midpoint, a cell centre, anywhere
    shift = np.select([kind[:, None] == 0, kind[:, None] == 1, kind[:, None] == 2], [(0.0, 0.0), (0.5, 0.0), (0.5, 0.5)],
                      rng.random((n_q, 2)))
    return base + shift, t


def _duplicates(n_q, n_t, seed):
    """every distinct template point one, two or three times over, so that for every k some k-th neighbour has a twin"""
    rng = _rng("duplicates", seed)
    distinct = rng.random((n_t, 2)) * 100.0
    t = np.repeat(distinct, rng.integers(1, 4, n_t), axis=0)[:n_t]
    return rng.random((n_q, 2)) * 100.0, t[rng.permutation(len(t))]


def _uniform(name, side=100.0):
    def gen(n_q, n_t, seed):
        rng = _rng(name, seed)
        return rng.random((n_q, 2)) * side, rng.random((n_t, 2)) * side
    return gen


# name -> (generator, branch, degenerate, default n_q, default n_t)
_SPEC = {
    "hline": (_hline, "w * h == 0 (gy == 1); with 6000 points the ext / 4096 floor on the cell for k <= 4", False, NQ, 6000),
    "vline": (_vline, "w * h == 0 (gx == 1)", False, NQ, NT),
    "single_point": (_single_point, "ext == 0: one cell, every distance equal", True, NQ, NT),
    "aniso": (_aniso, "a 1e6 : 1 box: area = ext^2 / n, one row of cells", False, NQ, NT),
    "offset_1e9": (_offset("offset_1e9", 1e9, 50.0), "the ldexp(mag, -40) term of the slack at ~1e-3 of a cell", False, NQ, NT),
    "offset_4e6": (_offset("offset_4e6", 4e6, 1e-3), "the ldexp(mag, -40) term of the slack at ~0.2 of a cell", False, NQ, NT),
    "cluster_outliers": (_cluster_outliers, "nine tenths of the template in one cell, the rest rings away", False, NQ, NT),
    "outside": (_outside, "queries beyond the four sides and corners: the clamped start cell and the ox / oy terms", False, NQ, NT),
    "scale_1e150": (_scale("scale_1e150", 1e150), "d2 near 1e300, still finite", False, NQ, NT),
    "scale_1e160": (_scale("scale_1e160", 1e160), "d2 overflows: d_k is inf and isfinite(dk) leaves the row to the host", True, NQ, NT),
    "scale_1e-150": (_scale("scale_1e-150", 5e-151), "every d2 below ALIGN_ABS: B is the whole template", True, NQ, NT),
    "lattice": (_lattice, "exact distance ties", True, NQ, NT),
    "duplicates": (_duplicates, "coincident template points", True, NQ, NT),
}
for _n in ALL_KS:   # n_t == k at the largest k that runs (found == k exactly at the `all` exit); n_t in {1, 2} among them
    _SPEC[f"nt_{_n}"] = (_uniform(f"nt_{_n}"), f"n_t == {_n}: the `all` exit with found == k", False, 300, _n)
BLOCK_NQ = (1, 63, 64, 65, 255, 256, 257)
for _n in BLOCK_NQ:
    _SPEC[f"nq_{_n}"] = (_uniform(f"nq_{_n}"), f"n_q == {_n}: the last block of 64 (LDS list) or 256 threads", False, _n, NT)

NAMES = tuple(_SPEC)
DEGENERATE = tuple(n for n in NAMES if _SPEC[n][2])
SIZE_NAMES = ("aniso", "offset_1e9", "offset_4e6", "cluster_outliers", "outside")
SIZE_KS = (1, 2, 5, 7, 9, 63)
_cache = {}


def family(name, n_q=None, n_t=None, seed=20):
    key = (name, n_q, n_t, seed)
    if key not in _cache:
        gen, branch, degenerate, dq, dt = _SPEC[name]
        q, t = gen(n_q or dq, n_t or dt, seed)
        q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
        assert q.shape == (n_q or dq, 2) and t.shape == (n_t or dt, 2) and np.isfinite(q).all() and np.isfinite(t).all()
        _cache[key] = Family(name, branch, q, t, degenerate)
    return _cache[key]


def ks_of(fam, ks=ALL_KS):
    return tuple(k for k in ks if k <= len(fam.txy))


def neighbours(fam, k):
    """cKDTree's k + 1 nearest template rows of every query, (n_q, k + 1); the row count n_t where scipy finds none"""
    from scipy.spatial import cKDTree

    kk = min(k + 1, len(fam.txy))
    with np.errstate(all="ignore"):
        _, idx = cKDTree(fam.txy).query(fam.qxy, k=list(range(1, kk + 1)), workers=WORKERS)
    if kk == k:
        idx = np.column_stack((idx, np.full(len(idx), len(fam.txy), idx.dtype)))
    return idx


def labels(fam, k, labelling, seed=5):
    """-> (qcode, tcode int32, expected match bit of a decided row or None)"""
    rng = _rng(fam.name + labelling, seed * 1000 + k)
    n_q, n_t = len(fam.qxy), len(fam.txy)
    if labelling == "random":
        return rng.integers(0, 5, n_q).astype(np.int32), rng.integers(0, 5, n_t).astype(np.int32), None
    idx = neighbours(fam, k)
    at_k = rng.random(n_q) < 0.5
    row = np.where(at_k, idx[:, k - 1], idx[:, k])
    qcode = np.where(row < n_t, row, ABSENT).astype(np.int32)
    return qcode, np.arange(n_t, dtype=np.int32), at_k


def restatement(fam, qcode, tcode, k):
    """the reference's rule with one vectorised cKDTree query -> (match (n_q,) bool, nearest template row (k == 1) or None)"""
    from scipy.spatial import cKDTree

    with np.errstate(all="ignore"):
        _, idx = cKDTree(fam.txy).query(fam.qxy, k=k, workers=WORKERS)
    if k == 1:
        return tcode[idx] == qcode, idx
    return (tcode[idx] == qcode[:, None]).any(axis=1), None


def frames(fam, qcode, tcode):
    import pandas as pd

    q = pd.DataFrame({"X": fam.qxy[:, 0], "Y": fam.qxy[:, 1], "cell_type": qcode.astype(np.int64)})
    t = pd.DataFrame({"X": fam.txy[:, 0], "Y": fam.txy[:, 1], "cell_type": tcode.astype(np.int64)})
    return q, t


def grid_of(txy, k):
    """align_geometry of csrc/align.hip in Python floats (the same IEEE doubles) -> dict(cell, gx, gy, floored, grew)"""
    x0, y0, x1, y1 = txy[:, 0].min(), txy[:, 1].min(), txy[:, 0].max(), txy[:, 1].max()
    n = len(txy)
    w, h = float(x1 - x0), float(y1 - y0)
    ext = max(w, h)
    cell, gx, gy, floored, grew = 1.0, 1, 1, False, 0
    if ext > 0.0 and math.isfinite(ext):
        per_cell = max(1.0, 0.5 * k)
        with np.errstate(over="ignore"):
            area = float(max(np.float64(w) * h, np.float64(ext) * ext / n))
            dense = float(np.sqrt(np.float64(area) * per_cell / n))
        cell = max(dense, ext / 4096.0)
        floored = cell > dense
        while True:
            gx, gy = (int(math.floor(w / cell)) + 1, int(math.floor(h / cell)) + 1) if math.isfinite(cell) else (1, 1)
            if gx * gy <= 2 * n + 16:
                break
            cell *= 1.25
            grew += 1
    return {"cell": cell, "gx": gx, "gy": gy, "x0": float(x0), "y0": float(y0), "floored": floored, "grew": grew}
