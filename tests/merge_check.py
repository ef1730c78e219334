"""The host statement of the window merge calls (csrc/window_merge.hip: same_window_collect, same_merge_acc_begin / load / resolve /
finish / plain / fetch / columns, same_section_set_codes; csrc/merge.hip's de-duplication behind resolve) and the input families its
library-level tests run it on.

The statement is plain numpy: `collect_rows` (one window's matched cells of its central region, from the window's CURRENT view),
`dedup` (np.lexsort and first occurrence), `resolve` (codes, de-duplication, degrees, the seam rule, the REST list and the direct
table), `finish`, `plain`, `columns` (bit patterns).  Only `winners` calls the product: merge._resolve_rows, the host's graph step,
which the device path leaves to the host as well.  Nothing of libsame_hip goes into it.  Every function takes the switches of the
deliberately WRONG statements tests/test_merge_check_cpu.py holds against the right one.

The row families (for same_merge_acc_load) and the window families (for same_window_collect) are cached and frozen as
tests/caller_check.py does.  tests/test_merge_check_cpu.py checks, without a GPU, that each family has the property it was made for;
tests/test_gpu_merge_library.py drives the library against the statement on them.  Not collected by pytest."""
import functools

import numpy as np

import caller_check as C

PENALTY = 50.0
ROWS = np.dtype([("a_row", "<i4"), ("r_row", "<i4"), ("flags", "u1"), ("wid", "<i4"), ("pos", "<i4"), ("cidx", "<i4")])
REST = np.dtype([("row", "<i4"), ("ac", "<i4"), ("rc", "<i4"), ("wid", "<i4"), ("pos", "<i4"), ("cidx", "<i4"), ("flags", "<u4")])
FINAL = np.dtype([("a_row", "<i4"), ("r_row", "<i4"), ("cidx", "<i4"), ("wid", "<i4"), ("pos", "<i4"), ("flags", "<u4")])
SCAN_NT, SORT_BLOCK, LOOKBACK = 256, 2048, 64         # csrc/scan.h, csrc/merge.hip
LAUNCH_WINDOWS, MAX_EXTRA_COLUMNS = 8, 4              # csrc/common.h, csrc/window_merge.hip
SIZES = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 16385)
WID_EXTREMES = (0, 1, 2 ** 31 - 2, 2 ** 31 - 1)
SPARSE_CODES = 100_000


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def rows_of(a_row, r_row, flags, wid, pos, cidx):
    """the six columns as one record array (scalars are broadcast)"""
    out = np.zeros(len(a_row), ROWS)
    for name, v in zip(ROWS.names, (a_row, r_row, flags, wid, pos, cidx)):
        out[name] = v
    return out


def collect_rows(rows, xy, match_row, flag, trim, wid, pos, upper="open", lower="closed", staged_rows=None):
    """same_window_collect for one window: the cells c ascending with match_row[c] >= 0, tx0 <= x < tx1 and ty0 <= y < ty1 (IEEE
    comparisons: a NaN edge admits nothing) -> (a_row, r_row, flags, wid, pos, cidx) records.  `rows`, `xy`: the window's kept cells
    as it holds them NOW (after a caller's compaction the compacted ones); `match_row`, `flag`: what its last finish / refinish returned.
    The wrong statements: upper="closed", lower="open", `staged_rows` (cidx counted among the cells as STAGED)."""
    tx0, tx1, ty0, ty1 = (np.float64(t) for t in trim)
    x, y = np.asarray(xy, np.float64).reshape(-1, 2).T
    with np.errstate(invalid="ignore"):
        lo = (x >= tx0) & (y >= ty0) if lower == "closed" else (x > tx0) & (y > ty0)
        hi = (x < tx1) & (y < ty1) if upper == "open" else (x <= tx1) & (y <= ty1)
    c = np.flatnonzero((np.asarray(match_row) >= 0) & lo & hi)
    cidx = c if staged_rows is None else np.searchsorted(staged_rows, np.asarray(rows)[c])
    return rows_of(np.asarray(rows)[c], np.asarray(match_row)[c], np.asarray(flag)[c], wid, pos, cidx)


def dedup(viol, wid, ac, rc, tie="earlier", wid_order="unsigned"):
    """src/helpers.py:745-753 on columns: the rows in the stable order by (viol, wid, row), the first row of every (ac, rc) kept, in
    that order -> row numbers.  The wrong statements: tie="later" (the later row wins a full tie), wid_order="signed" (the window id
    doubled into a 32-bit word and compared as signed: ids from 2^30 up sort before 0)."""
    n = len(ac)
    row = np.arange(n, dtype=np.int64)
    w = np.asarray(wid, np.int64)
    if wid_order == "signed":
        w = ((w << 1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
    order = np.lexsort((row if tie == "earlier" else -row, w, np.asarray(viol, bool)))
    pair = (np.asarray(ac, np.int64)[order] << 32) | np.asarray(rc, np.int64)[order]
    _u, first = np.unique(pair, return_index=True)          # first occurrence in the order
    return order[np.sort(first)]


def seam_of(rows, seams, ref_test="closed", aligned_test="half open", out_of_range=True):
    """seam_of of csrc/window_merge.hip per row: `seams` None -> no row; "all" -> every row; (near_start, near_boxes, reach, mov_xy,
    ref_xy): pos outside [0, n_pos) -> seam; an empty range -> not; else any box of the range with the aligned cell in [x0, x1) x
    [y0, y1) or the reference cell in [x0 - reach, x1 + reach] x [y0 - reach, y1 + reach].  The wrong statements: ref_test="half open",
    aligned_test="closed", out_of_range=False."""
    n = len(rows)
    if seams is None:
        return np.zeros(n, bool)
    if isinstance(seams, str):
        assert seams == "all"
        return np.ones(n, bool)
    near_start, near_boxes, reach, mov_xy, ref_xy = seams
    near_start, boxes = np.asarray(near_start, np.int64), np.asarray(near_boxes, np.float64).reshape(-1, 4)
    n_pos, reach = len(near_start) - 1, np.float64(reach)
    out = np.zeros(n, bool)
    for i in range(n):
        p = int(rows["pos"][i])
        if p < 0 or p >= n_pos:
            out[i] = out_of_range
            continue
        ax, ay = mov_xy[rows["a_row"][i]]
        rx, ry = ref_xy[rows["r_row"][i]]
        for x0, x1, y0, y1 in boxes[near_start[p]:near_start[p + 1]]:
            a_in = (ax >= x0 and ay >= y0) and ((ax < x1 and ay < y1) if aligned_test == "half open" else (ax <= x1 and ay <= y1))
            r_hi = (rx <= x1 + reach and ry <= y1 + reach) if ref_test == "closed" else (rx < x1 + reach and ry < y1 + reach)
            if a_in or (rx >= x0 - reach and ry >= y0 - reach and r_hi):
                out[i] = True
                break
    return out


def resolve(rows, codes_a=None, codes_r=None, n_codes_a=None, n_codes_r=None, seams=None, mask=1, **wrong):
    """same_merge_acc_resolve: the cells' codes (codes_x[row], or the row itself), the de-duplication under the violation mask (bit 0
    alone orders), the degree of every code among the survivors, and per survivor: lone (both degrees 1) and not at a seam -> final
    already, row_of[aligned code] = row; else -> REST, in de-duplicated order, flags & 3 plus 4 at a seam.
    -> dict(counts=(rows, kept, rest, final already), rest, row_of, ac, rows).  `wrong`: dedup's and seam_of's switches; mask=3."""
    n = len(rows)
    ac = rows["a_row"].astype(np.int64) if codes_a is None else np.asarray(codes_a, np.int64)[rows["a_row"]]
    rc = rows["r_row"].astype(np.int64) if codes_r is None else np.asarray(codes_r, np.int64)[rows["r_row"]]
    n_a, n_r = max(int(n_codes_a), 1), max(int(n_codes_r), 1)
    assert n == 0 or (0 <= ac.min() and ac.max() < n_a and 0 <= rc.min() and rc.max() < n_r)
    dd = {k: v for k, v in wrong.items() if k in ("tie", "wid_order")}
    sm = {k: v for k, v in wrong.items() if k in ("ref_test", "aligned_test", "out_of_range")}
    assert len(dd) + len(sm) == len(wrong)
    kept = dedup((rows["flags"] & mask) != 0, rows["wid"], ac, rc, **dd) if n else np.zeros(0, np.int64)
    deg_a, deg_r = np.bincount(ac[kept], minlength=n_a), np.bincount(rc[kept], minlength=n_r)
    lone = (deg_a[ac[kept]] == 1) & (deg_r[rc[kept]] == 1)
    seam = seam_of(rows[kept], seams, **sm)
    row_of = np.full(n_a, -1, np.int64)
    done = lone & ~seam
    row_of[ac[kept[done]]] = kept[done]
    left = kept[~done]
    rest = np.zeros(len(left), REST)
    rest["row"], rest["ac"], rest["rc"] = left, ac[left], rc[left]
    for name in ("wid", "pos", "cidx"):
        rest[name] = rows[name][left]
    rest["flags"] = (rows["flags"][left] & 3).astype(np.uint32) | np.where(seam[~done], 4, 0).astype(np.uint32)
    return dict(counts=(n, len(kept), len(left), len(kept) - len(left)), rest=rest, row_of=row_of, ac=ac, rows=rows)


def _final(rows, sel):
    out = np.zeros(len(sel), FINAL)
    for name in ("a_row", "r_row", "cidx", "wid", "pos"):
        out[name] = rows[name][sel]
    out["flags"] = rows["flags"][sel] & 3
    return out


def finish(resolved, winners, order="code"):
    """same_merge_acc_finish: the winners join the direct table; its rows in aligned-code order are the FINAL records.  The wrong
    statement: order="row"."""
    row_of = resolved["row_of"].copy()
    w = np.asarray(winners, np.int64)
    row_of[resolved["ac"][w]] = w
    sel = row_of[row_of >= 0]
    return _final(resolved["rows"], sel if order == "code" else np.sort(sel))


def plain(rows):
    """same_merge_acc_plain: every row a FINAL record, in arrival order"""
    return _final(rows, np.arange(len(rows)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def columns(final, types, mov_xy, ref_xy, extra_m=(), extra_r=()):
    """same_merge_acc_columns: the merged table's columns as bit patterns -> (uint64 (T + 4 + extras + 3, n), uint8 (2, n)): the moving
    rows' T type values, X, Y, the reference rows' X, Y, the extra 8-byte columns of the moving and of the reference rows, cidx, wid
    and pos as int64; then the area-flip bit and the XY-order bit."""
    a, r = final["a_row"].astype(np.int64), final["r_row"].astype(np.int64)
    types = np.ascontiguousarray(types, np.float64).reshape(len(mov_xy), -1)
    cols = [_bits(types[a, q]) for q in range(types.shape[1])]
    cols += [_bits(np.ascontiguousarray(mov_xy, np.float64)[a, q]) for q in (0, 1)] + [_bits(np.ascontiguousarray(ref_xy, np.float64)[r, q]) for q in (0, 1)]
    cols += [_bits(e)[a] for e in extra_m] + [_bits(e)[r] for e in extra_r]
    cols += [final[name].astype(np.int64).view(np.uint64) for name in ("cidx", "wid", "pos")]
    wide = np.array(cols, np.uint64).reshape(len(cols), len(final))
    return wide, np.array([(final["flags"] >> 1) & 1, final["flags"] & 1], np.uint8).reshape(2, len(final))


def block_image(wide, flags, byte_rows="exact"):
    """the output block as the call lays it: the 8-byte columns, then the byte block at column offset n8 * n.  The wrong statement:
    byte_rows="multiple of 8" (the byte block placed as if the row count were rounded up to 8)."""
    n8, n = wide.shape
    at = n8 * 8 * (n if byte_rows == "exact" else (n + 7) // 8 * 8)
    image = np.zeros(at + 2 * n, np.uint8)
    image[:n8 * 8 * n] = wide.reshape(-1).view(np.uint8)
    image[at:] = flags.reshape(-1)
    return image


def split_image(image, n8, n):
    """what a reader of the documented layout takes from a block"""
    return image[:n8 * 8 * n].view(np.uint64).reshape(n8, n), image[n8 * 8 * n:n8 * 8 * n + 2 * n].reshape(2, n)


def winners(rest):
    """the product's step on the REST list: merge._resolve_rows with rows that are de-duplicated already -> accumulator row numbers"""
    from same_amd import merge as M

    if len(rest) == 0:
        return np.zeros(0, np.int32)
    won = M._resolve_rows(rest["ac"].astype(np.int64), rest["rc"].astype(np.int64), (rest["flags"] & 1) != 0, rest["wid"].astype(np.int64),
                          M.already_deduplicated)
    return rest["row"][won].astype(np.int32)


# ---- the row families -----------------------------------------------------------------------------------------------------------------
def mix64(x):
    """the splitmix64 finaliser of csrc/merge.hip on uint64 arrays"""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def table_slots(n):
    """slots of merge.hip's pair table for n rows: the smallest power of two >= 2 n (at least 2)"""
    slots = 2
    while slots < 2 * n:
        slots <<= 1
    return slots


def home_slot(a, r, slots):
    return (mix64((np.asarray(a, np.uint64) << np.uint64(32)) | np.asarray(r, np.uint64)) & np.uint64(slots - 1)).astype(np.int64)


def _family(a, r, flags, wid, n_a, n_r, rng, **more):
    n = len(a)
    return _frozen(dict(a=np.asarray(a, np.int32), r=np.asarray(r, np.int32), flags=np.asarray(flags, np.uint8), wid=np.asarray(wid, np.int32),
                        pos=rng.integers(-2, 9, n).astype(np.int32), cidx=rng.integers(0, 1 << 20, n).astype(np.int32), n_codes_a=int(n_a),
                        n_codes_r=int(n_r), **more))


def _counts(n):
    """n = a sum of proposal counts 2, 3, 4, 2, ... (the tail adjusted so that every count stays in 2..4)"""
    out, rem, i = [], n, 0
    while rem:
        k = (2, 3, 4)[i % 3]
        i += 1
        if rem - k < 2 and rem - k != 0:
            k = rem if rem <= 4 else 2
        out.append(k)
        rem -= k
    return out


def _proposed(n, rng, propose):
    """pairs that stand alone in the graph, pair p proposed counts[p] times with the (flag, window id) lists propose(p, k) gives, the
    rows shuffled -> (a, r, flags, wid, kind per pair, pair of every row)"""
    counts = _counts(n)
    pa, pr = rng.permutation(len(counts)), rng.permutation(len(counts))
    pair = np.repeat(np.arange(len(counts)), counts)
    flags, wid = [], []
    for p, k in enumerate(counts):
        f, w = propose(p, k)
        flags += list(f)
        wid += list(w)
    order = rng.permutation(n)
    pair = pair[order]
    return pa[pair], pr[pair], np.array(flags)[order], np.array(wid, np.int64)[order], len(counts), pair


def _alone(n, rng):
    return _family(rng.permutation(n), rng.permutation(n), rng.integers(0, 4, n), rng.integers(0, 6, n), n, n, rng)


def _one_pair(n, rng):
    return _family(np.full(n, 3), np.full(n, 1), rng.integers(0, 4, n), rng.integers(0, 3, n), 5, 2, rng)


def _keys(n, rng):
    def propose(p, k):
        kind = p % 3
        if kind == 0:           # viol decides: the non-violating row has the LARGEST window id
            return [1, 0, 1, 1][:k], [0, 7, 1, 0][:k]
        v = (p // 3) % 2
        if kind == 1:           # viol equal, the window id decides
            return [v] * k, [5, 2, 9, 4][:k]
        return [v] * k, [3] * k  # all equal: the earlier row

    a, r, f, w, n_pairs, pair = _proposed(n, rng, propose)
    return _family(a, r, f, w, n_pairs, n_pairs, rng, pair=pair, kind=np.arange(n_pairs) % 3)


def _flag_bits(n, rng):
    def propose(p, k):
        kind = p % 4
        if kind == 0:           # proposals that differ ONLY in bit 1, bit 0 clear: one window id, the earlier row wins
            return [2, 0, 2, 0][:k], [4] * k
        if kind == 1:           # ... bit 0 set
            return [1, 3, 1, 3][:k], [4] * k
        if kind == 2:           # bit 1 alone is no violation: the row of the larger window id is not violating and wins over flag 1
            return [1, 2, 3, 1][:k], [0, 6, 1, 2][:k]
        return [int(q) for q in rng.integers(0, 4, k)], [int(q) for q in rng.integers(0, 3, k)]

    a, r, f, w, n_pairs, pair = _proposed(n, rng, propose)
    return _family(a, r, f, w, n_pairs, n_pairs, rng, pair=pair, kind=np.arange(n_pairs) % 4)


def _wid_extremes(n, rng):
    def propose(p, k):
        w = [WID_EXTREMES[q] for q in rng.permutation(4)[:k]]
        return ([0, 1, 0, 1][:k] if p % 5 == 4 else [p % 2] * k), w

    a, r, f, w, n_pairs, pair = _proposed(n, rng, propose)
    return _family(a, r, f, w, n_pairs, n_pairs, rng, pair=pair)


def _sparse_codes(n, rng):
    a, r = rng.choice(np.arange(1, SPARSE_CODES - 1), n, replace=False), rng.choice(np.arange(1, SPARSE_CODES - 1), n, replace=False)
    if n >= 1:
        a[0], r[0] = SPARSE_CODES - 1, 0
    if n >= 2:
        a[-1], r[-1] = 0, SPARSE_CODES - 1
    if n >= 7:
        a[3] = a[2]                       # one aligned code, two references: contested
        a[5], r[5] = a[4], r[4]           # a pair twice
    return _family(a, r, rng.integers(0, 4, n), rng.integers(0, 4, n), SPARSE_CODES, SPARSE_CODES, rng)


PROBE_ROWS, PROBE_PAIRS, PROBE_HOMES, PROBE_CODES = 2048, 200, (4095, 4094), 1024


def _probe_chain(n, rng):
    assert n == PROBE_ROWS
    slots = table_slots(n)
    ga, gr = np.meshgrid(np.arange(PROBE_CODES), np.arange(PROBE_CODES), indexing="ij")
    home = home_slot(ga.ravel(), gr.ravel(), slots)
    a, r = [], []
    for h in PROBE_HOMES:
        at = np.flatnonzero(home == h)[:PROBE_PAIRS]
        assert len(at) == PROBE_PAIRS
        a += [ga.ravel()[at]] * 3
        r += [gr.ravel()[at]] * 3
    fill = n - 3 * PROBE_PAIRS * len(PROBE_HOMES)
    a, r = np.concatenate(a + [PROBE_CODES + np.arange(fill)]), np.concatenate(r + [PROBE_CODES + rng.permutation(fill)])
    order = rng.permutation(n)
    return _family(a[order], r[order], rng.integers(0, 4, n), rng.integers(0, 3, n), PROBE_CODES + fill, PROBE_CODES + fill, rng, slots=slots)


STAR_ARMS, PATH_ROWS = 300, 511
STARS_NATURAL = 2 * STAR_ARMS + PATH_ROWS


def _stars_and_chains(n, rng):
    """(i) aligned code 0 proposed for `arms` references, (ii) reference `arms` proposed for `arms` aligned codes, (iii) a path
    a0-r0-a1-r1-... over the rest of the rows; 300, 300 and 511 at the natural size"""
    arms = STAR_ARMS if n >= STARS_NATURAL else n // 4
    path = n - 2 * arms
    k = np.arange(path)
    a = np.concatenate((np.zeros(arms, np.int64), 1 + np.arange(arms), arms + 1 + (k + 1) // 2))
    r = np.concatenate((np.arange(arms), np.full(arms, arms), arms + 1 + k // 2))
    order = rng.permutation(n)
    return _family(a[order], r[order], rng.integers(0, 4, n), rng.integers(0, 4, n), int(a.max()) + 1, int(r.max()) + 1, rng)


FAMILIES = {"alone": (_alone, SIZES), "one pair": (_one_pair, SIZES[1:]), "keys": (_keys, SIZES[2:]), "flag bits": (_flag_bits, SIZES[2:]),
            "wid extremes": (_wid_extremes, SIZES[2:]), "sparse codes": (_sparse_codes, tuple(n for n in SIZES if n <= 257)),
            "probe chain": (_probe_chain, (PROBE_ROWS,)),
            "stars and chains": (_stars_and_chains, tuple(n for n in SIZES if n >= 255) + (STARS_NATURAL,))}
LOAD_CASES = tuple((name, n) for name, (_make, sizes) in FAMILIES.items() for n in sizes)


@functools.lru_cache(maxsize=None)
def family(name, n):
    make, sizes = FAMILIES[name]
    assert n in sizes
    return make(n, np.random.default_rng(1000 * sorted(FAMILIES).index(name) + n % 997))


def loaded_rows(fam):
    """the rows of a family as the accumulator holds them after same_merge_acc_load"""
    return rows_of(fam["a"], fam["r"], fam["flags"], fam["wid"], fam["pos"], fam["cidx"])


def resolve_family(fam, **wrong):
    return resolve(loaded_rows(fam), None, None, fam["n_codes_a"], fam["n_codes_r"], None, **wrong)


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the window families ---------------------------------------------------------------------------------------------------------------
MATCHINGS = ("none", "all first candidate", "every second cell", "only cells on a trim edge")
TRIMS = ("whole", "lower edges on a cell", "upper edges on a cell", "tx0 == tx1", "inverted", "NaN edge", "infinite", "-0.0 edge")
EDGE_CELLS = (255, 256, 257, 16385)
WINDOWS = ("base/interior", "base/sliver", "zero") + tuple(f"edge/{n}" for n in EDGE_CELLS)


@functools.lru_cache(maxsize=None)
def zero_case():
    """`zero`: 60 moving points on a lattice of step 3 over [-6, 21] x [0, 15] -- a column of cells at x = 0.0 exactly --, every
    reference 0.25 beside its moving point; three type columns"""
    rng = np.random.default_rng(60)
    gx, gy = np.meshgrid(np.arange(10) * 3.0 - 6.0, np.arange(6) * 3.0, indexing="ij")
    mov = np.column_stack((gx.ravel(), gy.ravel()))
    n = len(mov)
    return _frozen(dict(mov_xy=mov, ref_xy=mov + (0.25, 0.0), type_id=rng.integers(0, 3, n).astype(np.int32), types_m=rng.gamma(0.3, 30.0, (n, 3)),
                        types_r=rng.gamma(0.3, 30.0, (n, 3)), size=np.ones(n), box=(-10.0, 30.0, -10.0, 30.0)))


def window_of(tag, oracle=None):
    """-> (section, box) of a tag of WINDOWS"""
    family_, _, rest = tag.partition("/")
    if family_ == "base":
        return C.base_case(), {"interior": (100.0, 200.0, 100.0, 200.0), "sliver": (150.0, 152.0, 0.0, 300.0)}[rest]      # (caller_check.base_boxes)
    if family_ == "zero":
        return zero_case(), zero_case()["box"]
    case = C.edge_case(int(rest))
    return case, case["box"]


def marked_cell(xy):
    """the kept cell a window's edge trims are cut at: the one in the middle of the cells ordered by (x, y) -- but the first at x == 0.0
    if there is one"""
    zero = np.flatnonzero(xy[:, 0] == 0.0)
    return int(zero[len(zero) // 2]) if len(zero) else int(np.lexsort((xy[:, 1], xy[:, 0]))[len(xy) // 2])


def trim_of(kind, box, xy):
    """the trim `kind` of a window with box `box` and kept cells at `xy`; None where the window cannot take it (-0.0 without a cell at
    x == 0.0)"""
    x0, x1, y0, y1 = (float(b) for b in box)
    mx, my = (float(v) for v in xy[marked_cell(xy)])
    if kind == "whole":
        return (x0, x1, y0, y1)
    if kind == "lower edges on a cell":
        return (mx, x1, my, y1)
    if kind == "upper edges on a cell":
        return (x0, mx, y0, my)
    if kind == "tx0 == tx1":
        return (mx, mx, y0, y1)
    if kind == "inverted":
        return (x1, x0, y1, y0)
    if kind == "NaN edge":
        return (x0, x1, float("nan"), y1)
    if kind == "infinite":
        return (-np.inf, np.inf, -np.inf, np.inf)
    assert kind == "-0.0 edge"
    return (-0.0, x1, y0, y1) if mx == 0.0 else None


def matching(name, pairs, xy):
    """pair index per kept cell (-1: none) of a matching of MATCHINGS; `pairs` the window's current list (rows ascending); "last
    candidate" (not in MATCHINGS): the cell's last pair -- another reference wherever the cell has two candidates"""
    n = len(xy)
    cells = np.arange(n)
    first = np.searchsorted(pairs[:, 0], cells, side="left").astype(np.int32)
    assert n == 0 or np.array_equal(pairs[first, 0], cells)          # every kept cell has a pair
    if name == "all first candidate":
        return first
    if name == "last candidate":
        return (np.searchsorted(pairs[:, 0], cells, side="right") - 1).astype(np.int32)
    mp = np.full(n, -1, np.int32)
    if name == "every second cell":
        mp[::2] = first[::2]
    elif name == "only cells on a trim edge" and n:
        mx, my = xy[marked_cell(xy)]
        on = (xy[:, 0] == mx) | (xy[:, 1] == my)
        mp[on] = first[on]
    else:
        assert name == "none" or n == 0
    return mp


def host_view(case, box, oracle, name):
    """a window's current view made on the host, for the CPU test: the host's stage, the matching `name`, a flag byte that cycles
    through 0..3 -> dict(rows, xy, pairs, match_row, flag)"""
    rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, case.get("radius", C.RADIUS), case.get("k", C.KNN), oracle)
    xy = np.ascontiguousarray(case["mov_xy"][rows])
    mp = matching(name, pairs, xy)
    match_row = np.where(mp >= 0, rows_r[pairs[np.maximum(mp, 0), 1]] if len(pairs) else -1, -1).astype(np.int32)
    return dict(rows=rows.astype(np.int32), xy=xy, pairs=pairs, match_row=match_row, flag=(np.arange(len(rows)) % 4).astype(np.uint8))


# ---- the seam plan ---------------------------------------------------------------------------------------------------------------------
SEAM_REACH = 0.75
SEAM_BANDS = 8


@functools.lru_cache(maxsize=None)
def seam_case():
    """48 moving points on a lattice of step 4 (x = 0 .. 20, y = 0 .. 28), every reference 0.25 to the right of its moving point and,
    with radius 1, its only candidate.  A pass collects the lattice band by band (y = 4 b, trim [4 b - 1, 4 b + 1)), band b at plan
    position SEAM_POS[b].  The boxes, per position (aligned x: 0, 4, .. 20; reference x: 0.25, 4.25, .. 20.25):
      0  [4, 12): reach 0 -- the cell ON x0 = 4 is a seam by the aligned test, the cell ON x1 = 12 is not (its reference at 12.25 lies
         outside the closed box too); with reach 0.75 both are, by the reference test
      1  [5, 11.5): the references at 4.25 and 12.25 lie EXACTLY reach = 0.75 outside -- seams by the closed, widened reference test alone
      2  (5, 11.5) one np.nextafter narrower at both ends: those two references are just out of reach
      3  an empty range
      4  two boxes: one far away, one [16, 20) x the band
    band 5 is collected at position -1, band 6 at position n_pos: seams whatever the boxes; band 7 at position 3 again."""
    gx, gy = np.meshgrid(np.arange(6) * 4.0, np.arange(SEAM_BANDS) * 4.0, indexing="ij")
    mov = np.column_stack((gx.ravel(), gy.ravel()))
    rng = np.random.default_rng(48)
    n = len(mov)
    lo, hi = -100.0, 100.0
    boxes = np.array([(4.0, 12.0, lo, hi), (5.0, 11.5, lo, hi), (np.nextafter(5.0, np.inf), np.nextafter(11.5, -np.inf), lo, hi),
                      (500.0, 600.0, lo, hi), (16.0, 20.0, 15.0, 17.0)])
    return _frozen(dict(mov_xy=mov, ref_xy=mov + (0.25, 0.0), type_id=rng.integers(0, 3, n).astype(np.int32), types_m=rng.gamma(0.3, 30.0, (n, 3)),
                        types_r=rng.gamma(0.3, 30.0, (n, 3)), size=np.ones(n), box=(-2.0, 24.0, -2.0, 32.0), radius=1.0, k=2,
                        near_start=np.array([0, 1, 2, 3, 3, 5], np.int32), near_boxes=boxes))


SEAM_POS = (0, 1, 2, 3, 4, -1, 5, 3)
SEAM_N_POS = 5


def seam_trims():
    return [(-2.0, 24.0, 4.0 * b - 1.0, 4.0 * b + 1.0) for b in range(SEAM_BANDS)]


# ---- the columns' section --------------------------------------------------------------------------------------------------------------
COLUMN_ROWS = (1, 7, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def columns_case():
    """caller_check.edge_case(257)'s points, the reference the moving points themselves, with coordinates whose bit patterns a float
    copy would lose: -0.0, the smallest denormal, the smallest normal (coordinates that are not finite lie in no window and never reach a
    table).  `types`: three type columns with -0.0 and denormals among ordinary values (they price the pairs, so they stay finite);
    `layer`: a second type matrix that only the columns call reads -- NaNs with payloads, both infinities, -0.0, denormals; `extra`: eight
    8-byte columns of arbitrary bits (NaN payloads, negative int64 ids among them), four per side."""
    e = C.edge_case(257)
    rng = np.random.default_rng(257)
    xy = e["mov_xy"].copy()
    xy[0], xy[1], xy[2] = (-0.0, 5e-324), (2.2250738585072014e-308, -0.0), (0.5, 0.0)
    n = len(xy)
    types = rng.gamma(0.3, 30.0, (n, 3))
    types[rng.random((n, 3)) < 0.1] = -0.0
    types[rng.random((n, 3)) < 0.1] = 5e-324
    hostile = np.array([0x7FF8000000000123, 0xFFF8DEADBEEF0001, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF], np.uint64).view(np.float64)
    layer = hostile[rng.integers(0, len(hostile), (n, 3))]
    extra = rng.integers(0, 2 ** 64, (8, n), dtype=np.uint64)
    extra[0, :8], extra[4, :8] = hostile.view(np.uint64), np.array([-1, -2 ** 63, -5, 2 ** 62, 0, 1, -2 ** 31, 2 ** 31], np.int64).view(np.uint64)
    return _frozen(dict(mov_xy=xy, ref_xy=xy.copy(), type_id=e["type_id"], types=types, types_r=rng.gamma(0.3, 30.0, (n, 3)), layer=layer,
                        extra=extra, size=np.ones(n), box=e["box"]))


def own_matching(pairs, rows, rows_r):
    """pair index per kept cell of the pair (cell, the reference row of the cell's own number)"""
    want = np.searchsorted(rows_r, rows)
    assert np.array_equal(np.asarray(rows_r)[want], rows)
    key = pairs[:, 0].astype(np.int64) * len(rows_r) + pairs[:, 1]
    order = np.argsort(key, kind="stable")
    at = np.searchsorted(key[order], np.arange(len(rows), dtype=np.int64) * len(rows_r) + want)
    assert np.array_equal(key[order][at], np.arange(len(rows), dtype=np.int64) * len(rows_r) + want)
    return order[at].astype(np.int32)


def trim_for(n, box, xy):
    """a trim of the box that holds exactly the n cells of smallest x (the cells' x are distinct)"""
    xs = np.sort(xy[:, 0])
    assert len(np.unique(xs)) == len(xs)
    return (box[0], box[1] if n >= len(xs) else float(xs[n]), box[2], box[3])
