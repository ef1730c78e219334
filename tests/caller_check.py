"""Plain host statements and deterministic input builders for tests of the window path's two front calls at the LIBRARY
(csrc/window_caller.hip: same_window_caller_tris; csrc/window_priority.hip: same_window_priority_pairs) at the shapes the product route
never produces: boxes over more than 64 cells of a section's grid, grids that cut through boxes, launch groups that mix the two
candidate paths, scans sized to a block edge, rows of 65 and 200 pairs with exactly equal distances, one reference 700 rows bid for.
tests/test_window_front_calls_cpu.py checks on these very inputs, without a GPU, that each has the property it was built for; GPU
tests that drive the library calls against the statements take their inputs from here.  Not collected by pytest."""
import functools

import numpy as np

RADIUS, KNN = 12.0, 6
NEAR_MARGIN = 1e-9            # no cosine of any input lies this close to the angle threshold: the call compacts (near == 0)


def window_statement(rows_kept, job_rows, xy, type_id, pairs, costs, radius, min_angle_deg, ignore_same_type, oracle):
    """csrc/window_caller.hip in numpy, for one window: `rows_kept` the ascending section rows of its kept aligned cells as staged,
    `job_rows` the job's triangles as section rows in the caller's order, `xy` / `type_id` of the kept cells, `pairs` (P, 2) over the kept
    cells (rows ascending) with their `costs`.
    -> (selected triangles in the caller's order and corner order, as indices into the kept cells as staged; valid mask over them; kept
    cells left; renumbered pairs; their costs; renumbered triangles left)"""
    n = len(rows_kept)
    job_rows = np.asarray(job_rows).reshape(-1, 3)
    # select + remap: all three rows among the kept cells; the caller's order, the caller's corners
    at = np.minimum(np.searchsorted(rows_kept, job_rows), max(n - 1, 0))
    inside = (rows_kept[at] == job_rows).all(axis=1) if n else np.zeros(len(job_rows), bool)
    sel = at[inside]
    # node mask: every triangle that passes the side and the angle test, before the same-type test
    cls, _perim, _maxcos = oracle.tri_classify(xy, sel, radius, min_angle_deg, type_id if ignore_same_type else None)
    valid = np.zeros(n, bool)
    valid[sel[(cls == 0) | (cls == 3)].reshape(-1)] = True
    # second compaction
    new = np.cumsum(valid) - 1
    left = sel[valid[sel].all(axis=1)] if len(sel) else sel
    tris2 = new[left]
    keep_pair = valid[pairs[:, 0]]
    pairs2 = np.column_stack((new[pairs[keep_pair, 0]], pairs[keep_pair, 1]))
    return sel, valid, int(valid.sum()), pairs2, np.asarray(costs)[keep_pair], tris2


def filtered_after(xy, type_id, valid, tris2, radius, min_angle_deg, ignore_same_type, oracle):
    """the unchanged filter on the smaller window (no node of it is unconstrained any more) -> kept triangles, in the reference's order"""
    import pandas as pd

    frame = pd.DataFrame({"cell_type": type_id[valid]})
    kept, gone = oracle.filter_triangles_by_radius(xy[valid], tris2, radius, aligned_df=frame, ignore_same_type_triangles=ignore_same_type,
                                                   remove_unconstrained_nodes=True, min_angle_deg=min_angle_deg)
    assert not gone
    return np.asarray(kept, dtype=np.int64).reshape(-1, 3)


def near_count(xy, sel, radius, min_angle_deg, oracle, margin=NEAR_MARGIN):
    """selected triangles that pass the side test and whose largest cosine lies within `margin` of the angle threshold"""
    en, thr = oracle.cos_threshold(min_angle_deg)
    if not en or not np.isfinite(thr) or len(sel) == 0:
        return 0
    cls, _perim, maxcos = oracle.tri_classify(xy, sel, radius, min_angle_deg, None)
    return int(np.count_nonzero((cls != 1) & (np.abs(maxcos - thr) <= margin)))


def in_box(xy, box):
    """np.flatnonzero of the reference's four comparisons (src/same.py:293-295)"""
    x0, x1, y0, y1 = box
    return np.flatnonzero((xy[:, 0] >= x0) & (xy[:, 0] < x1) & (xy[:, 1] >= y0) & (xy[:, 1] < y1))


def host_stage(mov_xy, ref_xy, box, radius, k, oracle):
    """same_window_stage's rows and pair list on the host: -> (section rows of the kept aligned cells, reference rows in the box, pairs
    (P, 2) int64 over (kept cell, reference of the window), rows ascending)"""
    rows_m, rows_r = in_box(mov_xy, box), in_box(ref_xy, box)
    if len(rows_m) == 0 or len(rows_r) == 0:
        return rows_m[:0], rows_r, np.zeros((0, 2), np.int64)
    idx, _d2, cnt = oracle.knn_prune(mov_xy[rows_m], ref_xy[rows_r], radius, k)
    kept = cnt > 0
    a, col = np.nonzero(idx[kept] >= 0)
    return rows_m[kept], rows_r, np.column_stack((a, idx[kept][a, col])).astype(np.int64)


def fitted_grid(grid, xy):
    """same_section_bin's grid for a caller's (x0, y0, cell_w, cell_h): whole cells from the origin down to the lowest finite row ->
    (x0, y0, cell_w, cell_h, nx, ny)"""
    ok = np.isfinite(xy).all(axis=1)
    out = []
    for origin, width, v in ((grid[0], grid[2], xy[ok, 0]), (grid[1], grid[3], xy[ok, 1])):
        lo, hi = float(v.min()), float(v.max())
        shift = np.ceil((origin - lo) / width) if origin > lo else 0.0
        while origin - shift * width > lo:
            shift += 1.0
        o = origin - shift * width
        n = max(1, int(np.floor((hi - o) / width) + 1.0))
        while not o + n * width > hi:
            n += 1
        out.append((o, n))
    return out[0][0], out[1][0], float(grid[2]), float(grid[3]), out[0][1], out[1][1]


def cells_covered(box, grid, xy):
    """cells of the section's grid a box covers (csrc/section.hip cover_of): the window leaves the cell-run path above 64"""
    gx0, gy0, cw, ch, nx, ny = fitted_grid(grid, xy)

    def span(lo, hi, origin, width, n):
        if not lo < hi or not hi > origin or not lo < origin + n * width:
            return 0
        c0 = 0 if lo <= origin else min(n - 1, int(np.floor((lo - origin) / width)))
        c1 = n - 1 if hi >= origin + n * width else min(n - 1, int(np.floor((hi - origin) / width)))
        if c1 > c0 and origin + c1 * width >= hi:
            c1 -= 1
        return c1 - c0 + 1

    return span(box[0], box[1], gx0, cw, nx) * span(box[2], box[3], gy0, ch, ny)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def shuffled_triangulation(xy, rng, thin=0.0):
    """scipy's Delaunay thinned by `thin`, shuffled, corners rotated: a caller's list"""
    from scipy.spatial import Delaunay

    tri = Delaunay(xy).simplices
    tri = tri[rng.random(len(tri)) >= thin]
    tri = tri[rng.permutation(len(tri))]
    tri = np.take_along_axis(tri, (np.arange(3)[None, :] + rng.integers(0, 3, len(tri))[:, None]) % 3, axis=1)
    return np.ascontiguousarray(tri, dtype=np.int32)


# ---- the caller call's base case ---------------------------------------------------------------------------------------------------
GRIDS = {"cell 75": (0.0, 0.0, 75.0, 75.0), "cell 25": (0.0, 0.0, 25.0, 25.0), "cell 40 off origin": (-7.3, 11.1, 40.0, 40.0),
         "one cell": (0.0, 0.0, 1000.0, 1000.0), "60 x 17": (0.0, 0.0, 60.0, 17.0)}
N_BASE = 6000
EMPTY_BOX = (590.0, 660.0, -5.0, 15.0)       # rows of both sections, none within the radius of another: staged, no kept cell
BESIDE_BOX = (310.0, 320.0, 0.0, 10.0)       # beside the data: no row of either section


@functools.lru_cache(maxsize=None)
def base_case():
    """6 000 moving points uniform in [0, 300)^2 with 3 type codes, a jittered copy as the reference; the triangulation scipy's Delaunay
    thinned by ~30 %, shuffled, corners rotated.  Behind them (rows >= 6 000, in no box of the 300 x 300 square): a clump of 40 moving
    rows and, 30 away, a clump of 40 reference rows -- EMPTY_BOX holds both and keeps nothing --, and one moving row without finite
    coordinates, named by four more triangles at the head of the list (it is in no cell of any grid, and in no window)."""
    rng = np.random.default_rng(2026)
    xy = rng.uniform(0, 300, (N_BASE, 2))
    tris = shuffled_triangulation(xy, rng, thin=0.3)
    ref = xy + rng.normal(0, 0.5, xy.shape)
    mov_xy = np.vstack((xy, rng.uniform(0, 10, (40, 2)) + (600.0, 0.0), [(np.nan, 5.0)]))
    ref_xy = np.vstack((ref, rng.uniform(0, 10, (40, 2)) + (640.0, 0.0), [(np.inf, 5.0)]))
    n = len(mov_xy)
    bad = n - 1
    head = np.array([[bad, 3, 4], [bad, 10, 11], [20, bad, 21], [30, 31, bad]], np.int32)
    return _frozen(dict(mov_xy=mov_xy, ref_xy=ref_xy, type_id=rng.integers(0, 3, n).astype(np.int32), types_m=rng.gamma(0.3, 30.0, (n, 4)),
                        types_r=rng.gamma(0.3, 30.0, (n, 4)), size=rng.integers(1, 4, n).astype(np.float64),
                        tris=np.ascontiguousarray(np.vstack((head, tris))), n_unbinned=2))


def _kept_without_triangle(case, oracle):
    """a box small enough that it holds kept cells but no whole triangle: the first 7 x 7 box around a moving point that does"""
    xy = case["mov_xy"]
    for p in range(200):
        x, y = xy[p]
        box = (float(x) - 3.5, float(x) + 3.5, float(y) - 3.5, float(y) + 3.5)
        rows, _r, _pairs = host_stage(xy, case["ref_xy"], box, RADIUS, KNN, oracle)
        if len(rows) and not np.isin(case["tris"], rows).all(axis=1).any():
            return box
    raise AssertionError("no such box among the first 200 points")


def base_boxes(oracle):
    """the boxes of the grid-independence test: the whole section, an interior 100 x 100, a sliver 2 wide, a box beside the data, a box
    with kept cells and no whole triangle"""
    return {"whole": (0.0, 300.0, 0.0, 300.0), "interior": (100.0, 200.0, 100.0, 200.0), "sliver": (150.0, 152.0, 0.0, 300.0),
            "beside": BESIDE_BOX, "no triangle": _kept_without_triangle(base_case(), oracle)}


def mixed_boxes(oracle):
    """23 boxes for ONE call on the cell-25 grid: whole-job-path boxes (> 64 cells), cell-run boxes, boxes without kept cells and boxes
    without a whole triangle, interleaved so that every launch group of 8 mixes them -> [(kind, box)]"""
    small = _kept_without_triangle(base_case(), oracle)
    rng = np.random.default_rng(23)
    out = []
    for q in range(23):
        kind = ("job", "cells", "empty", "no triangle")[q % 4]
        if kind == "job":            # at least 9 x 8 cells of 25
            x0, y0 = rng.uniform(0, 60, 2)
            box = (float(x0), float(x0 + rng.uniform(226, 240)), float(y0), float(y0 + rng.uniform(201, 240)))
        elif kind == "cells":        # at most 5 x 5 cells of 25, cutting through them
            x0, y0 = rng.uniform(0, 200, 2)
            box = (float(x0), float(x0 + rng.uniform(20, 99)), float(y0), float(y0 + rng.uniform(20, 99)))
        elif kind == "empty":
            box = EMPTY_BOX
        else:
            box = small
        out.append((kind, box))
    return out


# ---- sections whose every row is kept: the scans sized to a block edge ---------------------------------------------------------------
EDGE_ROWS = (255, 256, 257, 16385)
EDGE_TRIANGLES = (1, 255, 256, 257, 513, 16384, 16385)


@functools.lru_cache(maxsize=None)
def edge_case(n):
    """`n` points at the base case's density, the reference the moving points themselves: every row is kept (its own copy is 0 away), so the
    kept-cell count of the full box is `n` exactly.  The grid has 10 x 10 cells or more: the full box takes the whole-job path, where the
    candidates are the list's first m triangles exactly.  Two label codes, drawn independently on the two sides (the prune's scan)."""
    rng = np.random.default_rng(7000 + n)
    side = 300.0 * np.sqrt(n / N_BASE)
    xy = rng.uniform(0, side, (n, 2))
    return _frozen(dict(mov_xy=xy, ref_xy=xy.copy(), type_id=rng.integers(0, 3, n).astype(np.int32), types_m=rng.gamma(0.3, 30.0, (n, 4)),
                        types_r=rng.gamma(0.3, 30.0, (n, 4)), size=np.ones(n), tris=shuffled_triangulation(xy, rng), side=side,
                        grid=(0.0, 0.0, side / 10.0, side / 10.0), box=(-1.0, side + 1.0, -1.0, side + 1.0),
                        code_m=rng.integers(0, 2, n).astype(np.int32), code_r=rng.integers(0, 2, n).astype(np.int32)))


def edge_counts(n):
    """the triangle counts m to cut the list of edge_case(n) to: every block edge the list reaches, and the whole list"""
    total = len(edge_case(n)["tris"])
    return [m for m in EDGE_TRIANGLES if m <= total] + ([total] if n == EDGE_ROWS[-1] else [])


# ---- the prune's inputs --------------------------------------------------------------------------------------------------------------
TIE_K = {1: 1.5, 4: 1.5, 8: 3.2, 64: 10.0, 65: 10.0, 200: 20.0}       # k -> a radius at which interior rows fill k
TIE_BOX = (-10.0, 110.0, -10.0, 110.0)


def labels_of(codes):
    """labels whose `==` is the codes' rule: equal non-negative codes compare equal, a negative code (NaN) equals nothing"""
    return np.where(codes < 0, np.nan, codes.astype(np.float64))


@functools.lru_cache(maxsize=None)
def tie_case():
    """600 references on an integer lattice of spacing 2, the moving points on the half-step lattice -- four references exactly
    equidistant from every row, and whole shells of equal distances behind them -- plus a second layer of exact duplicates of every third
    moving point.  Two label codes; about one row in six has code -1 (a label that equals nothing), independently on the two sides."""
    rng = np.random.default_rng(77)
    gx, gy = np.meshgrid(np.arange(25) * 2.0, np.arange(24) * 2.0, indexing="ij")
    ref = np.column_stack((gx.ravel(), gy.ravel()))
    hx, hy = np.meshgrid(np.arange(24) * 2.0 + 1.0, np.arange(23) * 2.0 + 1.0, indexing="ij")
    half = np.column_stack((hx.ravel(), hy.ravel()))
    mov = np.vstack((half, half[::3]))
    code = lambda n: np.where(rng.random(n) < 1 / 6, -1, rng.integers(0, 2, n)).astype(np.int32)
    return _frozen(dict(mov_xy=mov, ref_xy=ref, types_m=rng.gamma(0.3, 30.0, (len(mov), 3)), types_r=rng.gamma(0.3, 30.0, (len(ref), 3)),
                        code_m=code(len(mov)), code_r=code(len(ref))))


CONTENTION_ROWS, CONTENTION_BOX, CONTENTION_RADIUS, CONTENTION_K = 700, (-10.0, 10.0, -10.0, 10.0), 5.0, 4


@functools.lru_cache(maxsize=None)
def contention_case():
    """700 moving rows within 0.5 of ONE reference that carries their label, eight references of the other label on a ring 3 away: every
    row's nearest is the one reference and every row bids for it"""
    rng = np.random.default_rng(700)
    ang, rad = rng.uniform(0, 2 * np.pi, CONTENTION_ROWS), rng.uniform(0.01, 0.5, CONTENTION_ROWS)
    mov = np.column_stack((rad * np.cos(ang), rad * np.sin(ang)))
    ring = np.arange(8) * (np.pi / 4)
    ref = np.vstack(([(0.0, 0.0)], np.column_stack((3.0 * np.cos(ring), 3.0 * np.sin(ring)))))
    return _frozen(dict(mov_xy=mov, ref_xy=ref, types_m=rng.gamma(0.3, 30.0, (len(mov), 3)), types_r=rng.gamma(0.3, 30.0, (len(ref), 3)),
                        code_m=np.zeros(len(mov), np.int32), code_r=np.array([0] + [1] * 8, np.int32)))


@functools.lru_cache(maxsize=None)
def base_codes():
    """two label codes for the base case's sections (some rows -1), for the prune's batch of 23 and the chain priority -> caller -> finish"""
    rng = np.random.default_rng(99)
    n = len(base_case()["mov_xy"])
    code = lambda: np.where(rng.random(n) < 0.1, -1, rng.integers(0, 2, n)).astype(np.int32)
    return _frozen(dict(code_m=code(), code_r=code()))


def priority_boxes():
    """23 boxes for ONE prune call: windows with pairs of very different sizes; in the middle of the launch groups windows whose box holds
    rows of both sections and no pair (EMPTY_BOX) and windows whose box holds nothing (BESIDE_BOX) -> [(kind, box)]"""
    rng = np.random.default_rng(123)
    out = []
    for q in range(23):
        kind = "no pairs" if q % 8 in (1, 4) else ("nothing" if q % 8 in (2, 5) else "pairs")
        if kind == "pairs":
            x0, y0 = rng.uniform(0, 250, 2)
            box = (float(x0), float(x0 + rng.uniform(3, 120)), float(y0), float(y0 + rng.uniform(3, 120)))
        else:
            box = EMPTY_BOX if kind == "no pairs" else BESIDE_BOX
        out.append((kind, box))
    out[0] = ("pairs", (0.0, 300.0, 0.0, 300.0))
    return out


def costs_of(staged_pairs, staged_costs, pairs, n_ref):
    """the staged cost of every pair of `pairs` (a pair is named once in a staged list)"""
    key = staged_pairs[:, 0].astype(np.int64) * n_ref + staged_pairs[:, 1]
    order = np.argsort(key, kind="stable")
    want = np.asarray(pairs)[:, 0].astype(np.int64) * n_ref + np.asarray(pairs)[:, 1]
    at = np.searchsorted(key[order], want)
    assert len(np.unique(key)) == len(key) and np.array_equal(key[order][at], want)
    return staged_costs[order][at]
