"""The host statement of same_window_filter_finish / same_window_refinish (csrc/window_finish.hip, with the greedy rounds of
csrc/match.hip behind it) and the input families its library-level tests run it on.

`statement` is one window's whole answer -- filter counts and the emitted triangles in the reference's order, `near`, signs, weights, the
greedy start and its productive rounds, matched rows, flag bytes, the eight stats, the two order-tie counters -- from the window's arrays
AS STAGED (fetched from the device, or `cpu_staged` here), a triangle list, the filter settings and the penalty.  It uses only the oracle
(the C restatement of the reference) and numpy.  The filter's add-back, the greedy round rule and the tie counters are stated a second
time in plain numpy (`emit`, `round_rule`, `filter_ties`, `sweep_ties`): the first two take the switches of the deliberately WRONG
statements tests/test_finish_check_cpu.py holds against the right one.

The families are small sections of their own, cached and frozen as tests/caller_check.py does.  Every moving row of a family is a kept
cell of its box (the CPU test proves it), so a triangle list over the section's rows is a list over the window's kept cells.  Sections
without type columns (T = 0) are staged with dist_ct_coeff = 1000: the distance coefficient is 1000 * 0.001 == 1.0 in both cost types
and a cost is the pair's L1 distance itself.  tests/test_finish_check_cpu.py checks, without a GPU, that each family has the property
it was made for; tests/test_gpu_finish_library.py drives the library against `statement` on them.  Not collected by pytest."""
import functools
import itertools

import numpy as np

import caller_check as C

PENALTY = 50.0
EDGES = ((0, 1), (0, 2), (1, 2))
STAT_NAMES = ("checked", "flipped", "xy_comparisons", "xy_violations", "xy_triangles", "area_flips", "greedy_rounds", "matched")
EDGE_TRIANGLES = (1, 255, 256, 257, 16385)
EDGE_NODES = (255, 256, 257, 16385)
MATCH_CELLS = (41, 42, 43)                        # n = 1, 2, 3 (mod 4): the last flag word is partly padding
MATCHINGS = ("none", "identity", "mirror", "two on one", "one unmatched per triangle")
WINDOW_GREEDY_ROUNDS, GREEDY_BATCH_MAX = 3, 64    # csrc/window_finish.hip, csrc/common.h


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _tris(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(-1, 3))


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def near_tol(angle, oracle):
    """(angle_enabled, threshold, tolerance) as the product passes them: tol = 8 * spacing(|thr|), 0 with a non-finite threshold"""
    en, thr = oracle.cos_threshold(angle)
    return en, thr, (float(8 * np.spacing(abs(thr))) if (en and np.isfinite(thr)) else 0.0)


def near_count(cls, maxcos, angle, oracle, class1_too=False):
    """triangles of class != 1 with |maxcos - thr| <= tol; `class1_too`: the WRONG count over every triangle"""
    en, thr, tol = near_tol(angle, oracle)
    if not en or not np.isfinite(thr):
        return 0
    hit = np.abs(maxcos - thr) <= tol
    return int(np.count_nonzero(hit if class1_too else hit & (cls != 1)))


def emit(cls, perim, tris, n, readd, pick="first", per_node=False):
    """src/helpers.py:331-389 over the classes, in numpy: the class-0 triangles ascending, then -- `readd` -- for every node without a kept
    triangle and with a valid one, ascending, its same-type triangle of smallest perimeter (the FIRST in input order among equal ones),
    unless an earlier node brought it.  -> (indices into `tris` in emitted order, kept count, best triangle per node or -1, asking nodes).
    The wrong statements: pick="last" (the last of equal perimeters), per_node=True (a triangle per asking node)."""
    kept = np.flatnonzero(cls == 0)
    best, asks = np.full(n, -1, np.int64), np.zeros(n, bool)
    if not readd:
        return kept, len(kept), best, asks
    has_kept, any_valid = np.zeros(n, bool), np.zeros(n, bool)
    has_kept[tris[kept].reshape(-1)] = True
    any_valid[tris[(cls == 0) | (cls == 3)].reshape(-1)] = True
    t3 = np.flatnonzero(cls == 3)
    v, t = tris[t3].reshape(-1).astype(np.int64), np.repeat(t3, 3)
    order = np.lexsort((t if pick == "first" else -t, perim[t], v))
    vs = v[order]
    head = np.flatnonzero(np.r_[True, vs[1:] != vs[:-1]]) if len(vs) else np.zeros(0, np.int64)
    best[vs[head]] = t[order][head]
    asks = ~has_kept & any_valid & (best >= 0)
    want = best[np.flatnonzero(asks)]
    if not per_node and len(want):
        want = want[np.sort(np.unique(want, return_index=True)[1])]
    return np.concatenate((kept, want)), len(kept), best, asks


def filter_ties(cls, perim, tris, best, asks):
    """FC_TIES, filter_emit_kernel's expression: class-3 triangles with a corner that asks, whose best triangle is another one and whose
    perimeter is within 1.8e-15 (relative) of that one's"""
    t3 = np.flatnonzero(cls == 3)
    if len(t3) == 0:
        return 0
    v = tris[t3]
    b = np.maximum(best[v], 0)
    tie = asks[v] & (best[v] != t3[:, None]) & (np.abs(perim[t3][:, None] - perim[b]) <= 1.8e-15 * perim[b])
    return int(np.count_nonzero(tie.any(axis=1)))


def _in_doubt(p):
    """devmath::sign_in_doubt over (T, 3, 2), its operations in its order"""
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    v = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    side = np.fmax(np.fmax(np.abs(b[:, 0] - a[:, 0]) + np.abs(b[:, 1] - a[:, 1]), np.abs(c[:, 0] - a[:, 0]) + np.abs(c[:, 1] - a[:, 1])),
                   np.abs(c[:, 0] - b[:, 0]) + np.abs(c[:, 1] - b[:, 1]))
    reach = np.fmax(np.fmax(np.abs(a[:, 0]), np.abs(b[:, 0])), np.abs(c[:, 0])) + side
    return np.abs(v) <= 3.6e-15 * reach * side


def sweep_ties(axy, rxy, tris, match):
    """SC_TIES, window_sweeps_kernel's expression: triangles with an edge matched at both ends whose ends share a coordinate on either
    side, or -- all three matched -- whose sign is in doubt on either side"""
    if len(tris) == 0:
        return 0
    m = match[tris]
    a = axy[tris]
    r = np.where((m >= 0)[:, :, None], rxy[np.maximum(m, 0)], 0.0)
    ties = np.zeros(len(tris), bool)
    for p, q in EDGES:
        both = (m[:, p] >= 0) & (m[:, q] >= 0)
        ties |= both & ((a[:, p, 0] == a[:, q, 0]) | (a[:, p, 1] == a[:, q, 1]) | (r[:, p, 0] == r[:, q, 0]) | (r[:, p, 1] == r[:, q, 1]))
    ties |= (m >= 0).all(axis=1) & (_in_doubt(a) | _in_doubt(r))
    return int(np.count_nonzero(ties))


def row_minimum(pairs, costs, n):
    best = np.full(n, np.inf)
    np.minimum.at(best, pairs[:, 0], costs)
    return best


def round_rule(pairs, costs, n, n_r, unmatched, strict=True, tie="low"):
    """csrc/match.hip's round rule, vectorised: rows whose minimum cost does not beat `unmatched` never enter (row_prefer_kernel's strict
    `<`); per round every pair alive that is the minimum under (cost, pair index) at BOTH of its ends is taken; the two zeros are one
    cost.  -> (pair index per row or -1, productive rounds).  The wrong statements: strict=False (`<=`), tie="high" (the higher index)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    i, j = pairs[:, 0], pairs[:, 1]
    c = np.asarray(costs, np.float64) + 0.0
    best = row_minimum(pairs, c, n)
    prefer = best < unmatched if strict else best <= unmatched
    alive = prefer[i]
    used_a, used_r = np.zeros(n, bool), np.zeros(n_r, bool)
    match_pair = np.full(n, -1, np.int32)
    rounds = 0
    while True:
        alive &= ~used_a[i] & ~used_r[j]
        idx = np.flatnonzero(alive)
        if len(idx) == 0:
            return match_pair, rounds
        order = idx[np.lexsort((idx if tie == "low" else -idx, c[idx]))]
        min_a, min_r = np.full(n, -1, np.int64), np.full(n_r, -1, np.int64)
        ua, fa = np.unique(i[order], return_index=True)
        ur, fr = np.unique(j[order], return_index=True)
        min_a[ua], min_r[ur] = order[fa], order[fr]
        sel = idx[(min_a[i[idx]] == idx) & (min_r[j[idx]] == idx)]
        assert len(sel)             # the smallest pair alive always qualifies
        rounds += 1
        match_pair[i[sel]] = sel
        used_a[i[sel]] = True
        used_r[j[sel]] = True
        alive[sel] = False


def oracle_greedy(pairs, costs, n, n_r, penalty, size, oracle):
    """oracle.compute_mip_start_pairs(init_method="greedy") -> pair index per row or -1"""
    chosen, _un = oracle.compute_mip_start_pairs(valid_pairs=np.asarray(pairs, np.int64).reshape(-1, 2), costs=costs, n_aligned=n, n_ref=n_r,
                                                 aligned_sizes=size, no_match_penalty=penalty, max_matches=1,
                                                 init_method="greedy", verbose=False)
    mp = np.full(n, -1, np.int32)
    for a, _r, p in chosen:
        mp[a] = p
    return mp


def tail(axy, size, rxy, rows_r, tris, pairs, match_pair, oracle, flags="or"):
    """the matched rows and the one pass over the kept triangles under `match_pair` -> dict(signs, weights, row, flag, stats without the
    rounds, sc_ties).  flags="overwrite": the WRONG flag byte, the last kind of writer wins."""
    n = len(axy)
    tris = _tris(tris)
    mp = np.asarray(match_pair, np.int64)
    match = np.where(mp >= 0, np.asarray(pairs, np.int64).reshape(-1, 2)[np.maximum(mp, 0), 1] if len(pairs) else -1, -1).astype(np.int32)
    row = np.where(match >= 0, np.asarray(rows_r)[np.maximum(match, 0)] if len(rows_r) else -1, -1).astype(np.int32)
    sign, weight = oracle.tri_sign_weight(axy, np.asarray(size, np.float64), tris)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["matched"] = int(np.count_nonzero(mp >= 0))
    flag = np.zeros(n, np.uint8)
    if len(tris):
        checked, viol, _f = oracle.orient_sweep(tris, sign, rxy, match)
        _edge, _tflag, pflag, counts = oracle.xyorder_sweep(axy, rxy, tris, match)
        _before, _after, _m3, flipped = oracle.area_flip(axy, rxy, tris, match)
        flip_node = np.zeros(n, np.uint8)
        flip_node[tris[flipped.astype(bool)].reshape(-1)] = 1
        flag = (pflag.astype(np.uint8) & 1) | (flip_node << 1) if flags == "or" else np.where(flip_node != 0, 2, pflag & 1).astype(np.uint8)
        stats.update(checked=int(checked), flipped=len(viol), xy_comparisons=int(counts[0]), xy_violations=int(counts[1]),
                     xy_triangles=int(counts[2]), area_flips=int(np.count_nonzero(flipped)))
    return dict(signs=sign.astype(np.int8), weights=weight, row=row, flag=flag, stats=stats, match=match,
                sc_ties=sweep_ties(np.asarray(axy), np.asarray(rxy), tris.astype(np.int64), match.astype(np.int64)))


def filter_statement(xy, type_id, tris, filt, oracle):
    """the filter of one window: -> dict(kept, added, near, out = emitted triangles in the reference's order, fc_ties, cls, perim,
    maxcos); `filt` = (radius, min_angle_deg, ignore_same_type)"""
    import pandas as pd

    radius, angle, same = filt
    tris = _tris(tris)
    use_type = bool(same) and type_id is not None
    cls, perim, maxcos = oracle.tri_classify(xy, tris, radius, angle, type_id if use_type else None)
    frame = pd.DataFrame({"cell_type": np.asarray(type_id)}) if use_type else None
    out = oracle.filter_triangles_by_radius(xy, tris, radius, aligned_df=frame, ignore_same_type_triangles=use_type, min_angle_deg=angle)
    out = _tris(out)
    kept = int(np.count_nonzero(cls == 0))
    _idx, _k, best, asks = emit(cls, perim, tris.astype(np.int64), len(xy), use_type)
    return dict(kept=kept, added=len(out) - kept, near=near_count(cls, maxcos, angle, oracle), out=out, cls=cls, perim=perim, maxcos=maxcos,
                fc_ties=filter_ties(cls, perim, tris.astype(np.int64), best, asks) if use_type else 0, best=best, asks=asks)


def statement(staged, rxy, type_id, size, tris, filt, penalty, oracle, prefiltered=False, match_pair=None, start=None):
    """One window's answer.  `staged`: dict(rows, rows_r, xy, pairs, costs) as staged; `rxy` the XY of `rows_r`; `type_id` / `size` of the
    kept cells; `tris` the simplices (or, `prefiltered`, the kept triangles); `match_pair` given: a re-finish under that matching (no
    start, rounds 0); `start`: the (match_pair, rounds) of an earlier statement of the same staged window, not worked out again.
    -> dict(kept, added, near, tris, signs, weights, match_pair, row, flag, stats, order_ties); with near != 0 only
    the filter's part (row, flag, stats None; order_ties the filter's count)."""
    n, n_r = len(staged["rows"]), len(staged["rows_r"])
    pairs, costs = staged["pairs"].astype(np.int64), staged["costs"]
    if prefiltered or len(_tris(tris)) == 0:
        f = dict(kept=len(_tris(tris)), added=0, near=0, out=_tris(tris), fc_ties=0)
    else:
        f = filter_statement(staged["xy"], type_id, tris, filt, oracle)
    out = dict(kept=f["kept"], added=f["added"], near=f["near"], tris=f["out"], order_ties=f["fc_ties"], fc_ties=f["fc_ties"], row=None, flag=None,
               stats=None)
    if f["near"]:
        return out
    size = np.asarray(size, np.float64)
    rounds = 0
    if match_pair is None and start is not None:
        match_pair, rounds = start
    elif match_pair is None:
        match_pair = oracle_greedy(pairs, costs, n, n_r, penalty, size, oracle)
        ruled, rounds = round_rule(pairs, costs, n, n_r, penalty * size)
        assert np.array_equal(ruled, match_pair)
    t = tail(staged["xy"], size, rxy, staged["rows_r"], f["out"], pairs, match_pair, oracle)
    t["stats"]["greedy_rounds"] = rounds
    out.update(match_pair=np.asarray(match_pair, np.int32), signs=t["signs"], weights=t["weights"], row=t["row"], flag=t["flag"],
               stats=t["stats"], order_ties=f["fc_ties"] + t["sc_ties"], match=t["match"], start=(match_pair, rounds))
    return out


def restated(case, staged, tris, filt, oracle, penalty=None, pick="first", per_node=False, strict=True, tie="low", flags="or", class1_too=False,
             match_pair=None):
    """The window's answer a second time, the filter's add-back and the greedy start from the numpy statements (`emit`, `round_rule`)
    instead of the oracle's -- with every switch at its default it is `statement`'s answer, with one switch thrown the answer of a kernel
    that is wrong in that way.  -> dict(near, tris, match_pair, rounds, row, flag, stats)"""
    rows = staged["rows"]
    n, n_r = len(rows), len(staged["rows_r"])
    tid = None if case.get("type_id") is None else case["type_id"][rows]
    size = np.asarray(case["size"][rows], np.float64)
    penalty = case.get("penalty", PENALTY) if penalty is None else penalty
    radius, angle, same = filt
    tris = _tris(tris)
    use_type = bool(same) and tid is not None
    cls, perim, maxcos = oracle.tri_classify(staged["xy"], tris, radius, angle, tid if use_type else None)
    idx, _kept, _best, _asks = emit(cls, perim, tris.astype(np.int64), n, use_type, pick, per_node)
    rounds = 0
    if match_pair is None:
        match_pair, rounds = round_rule(staged["pairs"], staged["costs"], n, n_r, penalty * size, strict, tie)
    t = tail(staged["xy"], size, case["ref_xy"][staged["rows_r"]], staged["rows_r"], tris[idx], staged["pairs"], match_pair, oracle, flags)
    t["stats"]["greedy_rounds"] = rounds
    return dict(near=near_count(cls, maxcos, angle, oracle, class1_too), tris=tris[idx], match_pair=match_pair, rounds=rounds, row=t["row"],
                flag=t["flag"], stats=t["stats"])


def same_answer(a, b):
    """two `restated` answers (or one and a `statement` without a near window) agree in everything both hold"""
    return (a["near"] == b["near"] and np.array_equal(a["tris"], b["tris"]) and np.array_equal(a["match_pair"], b["match_pair"])
            and np.array_equal(a["row"], b["row"]) and np.array_equal(a["flag"], b["flag"]) and a["stats"] == b["stats"])


def cpu_staged(case, oracle, dtype="float64", box=None):
    """the window's arrays as the stage call leaves them, on the host (caller_check.host_stage + oracle.pair_cost_arrays in `dtype`)"""
    box = case["box"] if box is None else box
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, case["radius"], case["k"], oracle)
    xy, rxy = case["mov_xy"][rows], case["ref_xy"][rows_r]
    costs = oracle.pair_cost_arrays(case["types_m"][rows], case["types_r"][rows_r], xy, rxy, pairs, case["coeff"],
                                    dtype=np.dtype(dtype)).astype(np.float64) if len(pairs) else np.zeros(0)
    return dict(rows=rows, rows_r=rows_r, xy=np.ascontiguousarray(xy), pairs=pairs.astype(np.int32), costs=costs)


def of_case(case, staged, tris, filt, oracle, penalty=None, **how):
    """`statement` of a family's window from its arrays as staged"""
    rows = staged["rows"]
    tid = None if case.get("type_id") is None else case["type_id"][rows]
    return statement(staged, case["ref_xy"][staged["rows_r"]], tid, case["size"][rows], tris, filt, case.get("penalty", PENALTY) if penalty is None
                     else penalty, oracle, **how)


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def _section(mov, ref, type_id, size=None, types=None, box=None, radius=C.RADIUS, k=C.KNN, coeff=1000.0, **more):
    mov, ref = np.ascontiguousarray(mov, np.float64), np.ascontiguousarray(ref, np.float64)
    tm, tr = types if types is not None else (np.zeros((len(mov), 0)), np.zeros((len(ref), 0)))
    if box is None:
        both = np.vstack((mov, ref))
        box = (float(both[:, 0].min() - 1), float(both[:, 0].max() + 1), float(both[:, 1].min() - 1), float(both[:, 1].max() + 1))
    return _frozen(dict(mov_xy=mov, ref_xy=ref, types_m=tm, types_r=tr, type_id=None if type_id is None else np.asarray(type_id, np.int32),
                        size=np.ones(len(mov)) if size is None else np.asarray(size, np.float64), box=box, radius=radius, k=k, coeff=coeff, **more))


PATCH = 8.0         # about two mean spacings of caller_check's density


@functools.lru_cache(maxsize=None)
def edge_section():
    """`edge/Tr`: caller_check.edge_case(16 385)'s points (the reference the moving points themselves: every row kept) and its shuffled,
    corner-rotated triangulation; two types in a chessboard of 8 x 8 patches, so inside a patch triangles are same-type (class 3, nodes
    that ask) and across patch borders they are kept (class 0); the hull brings long sides (class 1) and slivers (class 2)."""
    e = C.edge_case(16385)
    xy = e["mov_xy"]
    tid = ((np.floor(xy[:, 0] / PATCH) + np.floor(xy[:, 1] / PATCH)) % 2).astype(np.int32)
    return _section(xy, xy.copy(), tid, types=(e["types_m"], e["types_r"]), box=e["box"], coeff=1.0, tris=e["tris"])


def edge_lists(oracle):
    """name -> triangle list of edge_section(): the list cut to exactly Tr rows; a list whose every triangle is kept and one with none kept"""
    case = edge_section()
    cls, _p, _c = oracle.tri_classify(case["mov_xy"], case["tris"], case["radius"], 15, case["type_id"])
    out = {f"Tr={m}": case["tris"][:m] for m in EDGE_TRIANGLES}
    out["all kept"] = case["tris"][cls == 0][:16385]
    out["none kept"] = case["tris"][cls != 0]
    return out


@functools.lru_cache(maxsize=None)
def one_type_section(n):
    """`edge/n`: caller_check.edge_case(n)'s points, every cell one type: no triangle is kept, every node with a valid triangle asks"""
    e = C.edge_case(n)
    return _section(e["mov_xy"], e["mov_xy"].copy(), np.zeros(n, np.int32), types=(e["types_m"], e["types_r"]), box=e["box"], coeff=1.0,
                    tris=e["tris"])


LATTICE, STEP = 6, 3.0


def _lattice_points(shift=(0.0, 0.0)):
    gx, gy = np.meshgrid(np.arange(LATTICE) * STEP, np.arange(LATTICE) * STEP, indexing="ij")
    return np.column_stack((gx.ravel() + shift[0], gy.ravel() + shift[1]))


@functools.lru_cache(maxsize=None)
def lattice_section(two_types=False, shift=(0.0, 0.0)):
    """`lattice` / `knife` / `greedy/ties`: 36 moving points on a 6 x 6 lattice of step 3; 49 references on the 7 x 7 lattice half a
    step off, so the four references around a cell are at L1 distance 3 exactly, the eight behind them at 6 (T = 0: equal costs); the
    triangle list: every triple of lattice points that is not collinear, shuffled, corners rotated -- the 45-degree corners of the
    right-angled ones have a cosine within the tolerance of min_angle_deg = 45's threshold, and the smallest perimeter of every node is
    shared by several triangles exactly.  two_types: the types in columns of two."""
    rng = np.random.default_rng(36)
    mov = _lattice_points(shift)
    gx, gy = np.meshgrid(np.arange(LATTICE + 1) * STEP - STEP / 2, np.arange(LATTICE + 1) * STEP - STEP / 2, indexing="ij")
    ref = np.column_stack((gx.ravel() + shift[0], gy.ravel() + shift[1]))
    tri = np.array(list(itertools.combinations(range(len(mov)), 3)), np.int64)
    p = mov[tri] - np.asarray(shift)
    area2 = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    collinear = tri[area2 == 0]
    tri = tri[area2 != 0]
    tri = tri[rng.permutation(len(tri))]
    tri = np.take_along_axis(tri, (np.arange(3)[None, :] + rng.integers(0, 3, len(tri))[:, None]) % 3, axis=1)
    tid = ((np.arange(len(mov)) // LATTICE) // 2 % 2).astype(np.int32) if two_types else np.zeros(len(mov), np.int32)
    return _section(mov, ref, tid, tris=_tris(tri), collinear=_tris(collinear))


def degenerate_list():
    """`degenerate`: over lattice_section()'s cells -- collinear triples, triangles with a repeated vertex (a, a, b), (a, b, a), (b, a, a), and
    every fifth proper triangle between them"""
    case = lattice_section()
    n = len(case["mov_xy"])
    a = np.arange(n - 1)
    rep = np.vstack((np.column_stack((a, a, a + 1)), np.column_stack((a, a + 1, a)), np.column_stack((a + 1, a, a)), [[3, 3, 3]]))
    parts = [case["collinear"], rep, case["tris"][::5]]
    out = np.vstack(parts)
    return _tris(out[np.random.default_rng(5).permutation(len(out))])


@functools.lru_cache(maxsize=None)
def match_section(n):
    """`match/*`: n moving points; 2 n references: a jittered copy of every moving point (reference i: the `identity` matching; the
    references 7, 8 and 11, 12 share their coordinates), then the moving points' exact mirror images x -> -x (reference n + i).  Radius and k large enough that
    every (cell, reference) is a pair.  The triangles: scipy's Delaunay of the moving points, all kept (no type rule, no angle rule)."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(4100 + n)
    mov = rng.uniform(1.0, 50.0, (n, 2))
    near = mov + rng.normal(0, 0.3, mov.shape)
    near[8], near[12] = near[7], near[11]
    mirror = mov * (-1.0, 1.0)
    return _section(mov, np.vstack((near, mirror)), None, size=rng.integers(1, 4, n), radius=500.0, k=2 * n,
                    tris=_tris(Delaunay(mov).simplices))


def pair_index(pairs, n_ref):
    """(cell, reference of the window) -> index of the pair in the list as staged"""
    key = pairs[:, 0].astype(np.int64) * n_ref + pairs[:, 1]
    order = np.argsort(key, kind="stable")

    def at(cells, refs):
        want = np.asarray(cells, np.int64) * n_ref + np.asarray(refs, np.int64)
        pos = np.searchsorted(key[order], want)
        assert np.array_equal(key[order][pos], want)
        return order[pos].astype(np.int32)

    return at


def matching(name, n, tris, pairs, n_ref):
    """the chosen matchings of `match/*` as pair indices per cell"""
    at = pair_index(pairs, n_ref)
    cells = np.arange(n)
    if name == "none":
        return np.full(n, -1, np.int32)
    if name == "identity":
        return at(cells, cells)
    if name == "mirror":
        return at(cells, cells + n)
    if name == "two on one":                    # the first triangle's first two cells on ONE reference: a reference sign of 0, equal XY at their edge
        return at(cells, np.where(cells == tris[0][1], tris[0][0], cells))
    mp = at(cells, cells)                       # one unmatched per triangle: the first corner of every triangle that has none yet
    off = np.zeros(n, bool)
    for t in tris:
        if not off[t].any():
            off[t[0]] = True
    mp[off] = -1
    return mp


CHAIN = 200


@functools.lru_cache(maxsize=None)
def chain_section():
    """`greedy/chain`: 200 moving and 200 reference points alternating along a line, gap q = 2.0 - 0.004 q; radius 2.5, k = 2: pair q joins
    point q and point q + 1, its cost the gap, strictly falling -- only the last pair alive is the minimum at both of its ends, so every
    round takes ONE pair: 200 rounds.  Every second moving point sits 0.001 above the line (the costs still fall strictly), so that
    consecutive triples of moving points are thin triangles the tail has something to say about."""
    gaps = 2.0 - 0.004 * np.arange(2 * CHAIN - 1)
    x = np.concatenate(([0.0], np.cumsum(gaps)))
    mov = np.column_stack((x[0::2], 0.001 * (np.arange(CHAIN) % 2)))
    ref = np.column_stack((x[1::2], np.zeros(CHAIN)))
    a = np.arange(CHAIN - 2)
    return _section(mov, ref, np.arange(CHAIN) % 3, radius=2.5, k=2, tris=_tris(np.column_stack((a, a + 1, a + 2))))


CHAIN_FILTER = (12.0, None, True)          # the filter's own radius: the thin triangles are kept


PENALTY_ROWS = 63
ULP64, ULP32 = 2.0 ** -51, 2.0 ** -22      # of a double / a float in [2, 4)


@functools.lru_cache(maxsize=None)
def penalty_section():
    """`greedy/penalty`: 63 moving rows 40 apart, each with ONE reference within the radius, penalty 3.0.  The L1 distance is exact in
    both cost types and chosen per row (seven kinds, cycling) so that the row's only cost is: size 1: 3.0 == penalty * size; size 2:
    6.0 == penalty * size; size 1.5: 4.5 == penalty * size; size 1: one double ulp above / below 3.0; size 1: one float ulp above /
    below 3.0.  (The double-ulp rows are 3.0 exactly in float costs.)  The strict `<`: a row on the penalty stays unmatched, so does one
    above; one below is matched."""
    kind = np.arange(PENALTY_ROWS) % 7
    size = np.array([1.0, 2.0, 1.5, 1.0, 1.0, 1.0, 1.0])[kind]
    dx = np.array([3.0, 6.0, 4.5, 3.0, 2.5, 3.0, 2.5])[kind]
    dy = np.array([0.0, 0.0, 0.0, ULP64, 0.5 - ULP64, ULP32, 0.5 - ULP32])[kind]
    mov = np.column_stack((40.0 * np.arange(PENALTY_ROWS), np.zeros(PENALTY_ROWS)))
    a = np.arange(PENALTY_ROWS - 2)
    return _section(mov, mov + np.column_stack((dx, dy)), np.arange(PENALTY_ROWS) % 2, size=size, radius=8.0, k=2, penalty=3.0, kind=kind,
                    tris=_tris(np.column_stack((a, a + 1, a + 2))))


PENALTY_FILTER = (500.0, None, False)


BATCH_WINDOWS, BATCH_PITCH = 9, 100.0
BATCH_KNIFE, BATCH_NO_TRIANGLES, BATCH_NO_KEPT = 4, 2, 6
BATCH_FILTER = (C.RADIUS, 45, True)


@functools.lru_cache(maxsize=None)
def batch_section():
    """`batch`: nine windows side by side, 100 apart, for ONE call at min_angle_deg = 45: window 4 the lattice (its corners on the
    threshold: near > 0), window 2 generic points with an empty triangle list, window 6 moving and reference points 30 apart (staged, no
    kept cell), the others 60-120 generic points with three types and scipy's triangulation.  -> the section; `boxes`, `tris` per window
    (over the window's own cells, which are consecutive rows from `first`)."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(909)
    lat = lattice_section(False, (BATCH_KNIFE * BATCH_PITCH + 20.0, 20.0))
    mov, ref, tid, tris, first, boxes = [], [], [], [], [], []
    at = 0
    for w in range(BATCH_WINDOWS):
        x0 = w * BATCH_PITCH
        boxes.append((x0, x0 + BATCH_PITCH - 10.0, 0.0, 90.0))
        first.append(at)
        if w == BATCH_KNIFE:
            m, r, t, tr = lat["mov_xy"], lat["ref_xy"], lat["type_id"], lat["tris"]
        elif w == BATCH_NO_KEPT:
            m, r = rng.uniform(0, 10, (20, 2)) + (x0 + 5.0, 5.0), rng.uniform(0, 10, (20, 2)) + (x0 + 45.0, 5.0)
            t, tr = np.zeros(20, np.int32), np.zeros((0, 3), np.int32)
        else:
            n = int(rng.integers(60, 121))
            m = rng.uniform(0, 60, (n, 2)) + (x0 + 5.0, 5.0)
            r = m + rng.normal(0, 0.8, m.shape)
            t = rng.integers(0, 3, n).astype(np.int32)
            tr = np.zeros((0, 3), np.int32) if w == BATCH_NO_TRIANGLES else _tris(Delaunay(m).simplices)
        mov.append(m); ref.append(r); tid.append(t); tris.append(tr)
        at += len(m)
    mov, ref = np.vstack(mov), np.vstack(ref)
    return _section(mov, ref, np.concatenate(tid), size=rng.integers(1, 4, len(mov)), box=(-1.0, 900.0, -1.0, 91.0), boxes=tuple(boxes),
                    tris=tuple(tris), first=tuple(first))


def random_pair_list(seed):
    """a seeded random pair list for the greedy agreement: costs from a small set (many ties, both zeros), float sizes"""
    rng = np.random.default_rng(seed)
    n, n_r = int(rng.integers(1, 60)), int(rng.integers(1, 60))
    k = int(rng.integers(1, 7))
    pairs = np.array([(a, r) for a in range(n) for r in sorted(rng.choice(n_r, min(k, n_r), replace=False).tolist())], np.int64)
    costs = rng.choice([-0.0, 0.0, 0.5, 1.0, 1.0, 2.0, 2.5, 7.0], len(pairs)) if seed % 2 else rng.uniform(0, 4, len(pairs))
    size = rng.choice([1.0, 2.0, 0.5, 1.25], n)
    return pairs, np.asarray(costs, np.float64), n, n_r, size, float(rng.choice([0.5, 1.0, 2.0, 50.0]))


# ---- the windows of one finish call each: tag -> (section, triangle list, filter settings) ---------------------------------------------
FILTER = (C.RADIUS, 15, True)
EDGE_LISTS = tuple(f"Tr={m}" for m in EDGE_TRIANGLES) + ("all kept", "none kept")
TAGS = (tuple(f"edge/n={n}" for n in EDGE_NODES)
        + tuple(f"lattice/{types}/{angle}" for types in ("one type", "two types") for angle in (15, None))
        + ("knife", "degenerate/angle rule", "degenerate/no angle rule") + tuple(f"match/{n}" for n in MATCH_CELLS)
        + ("greedy/chain", "greedy/ties", "greedy/penalty"))
NEAR_TAGS = ("knife",)


def window_of(tag, oracle=None):
    """-> (section, triangle list, (radius, min_angle_deg, ignore_same_type)) of a tag of TAGS or of "edge/" + a name of EDGE_LISTS"""
    family, _, rest = tag.partition("/")
    if family == "edge" and rest.startswith("n="):
        case = one_type_section(int(rest[2:]))
        return case, case["tris"], FILTER
    if family == "edge":
        return edge_section(), edge_lists(oracle)[rest], FILTER
    if family == "lattice":
        types, _, angle = rest.partition("/")
        case = lattice_section(types == "two types")
        return case, case["tris"], (C.RADIUS, None if angle == "None" else int(angle), True)
    if family == "knife":
        case = lattice_section()
        return case, case["tris"], (C.RADIUS, 45, True)
    if family == "degenerate":
        return lattice_section(), degenerate_list(), (C.RADIUS, 15 if rest == "angle rule" else None, True)
    if family == "match":
        case = match_section(int(rest))
        return case, case["tris"], (500.0, None, False)
    if tag == "greedy/chain":
        return chain_section(), chain_section()["tris"], CHAIN_FILTER
    if tag == "greedy/ties":             # the lattice's equal costs; a short list, no type rule
        case = lattice_section(True)
        return case, case["tris"][:300], (C.RADIUS, None, False)
    if tag == "greedy/penalty":
        return penalty_section(), penalty_section()["tris"], PENALTY_FILTER
    raise KeyError(tag)
