"""The host statement of same_merge_acc_score_detail (csrc/window_score_detail.hip) and the input families its library-level tests run on.

`host_detail_counts` is the call's whole `out` array in plain numpy, written from include/same_hip.h's statement of the words; the
triangle flags are tests/score_check.py's (`host_triangles`, the reference's area and flip rule in its operation order).  It imports
nothing that ends in libsame_hip.

A family takes a score_check `Job` (the final rows of a merged accumulator, the job's XY and joint label codes) and returns named `Detail`
inputs: score_check's `Inputs`, the rows' groups, the label count, the labels' columns and the two type matrices.
tests/test_score_details_cpu.py checks, without a GPU, that each family has the property it is named for;
tests/test_gpu_score_details_library.py drives the library against `host_detail_counts` on them.  Not collected by pytest."""
import collections

import numpy as np

import score_check as S

MAX_LABELS, MAX_GROUPS, RANKS = 64, 256, 16          # SAME_SCORE_MAX_LABELS, SAME_SCORE_MAX_GROUPS, SAME_SCORE_RANKS
TRI_COUNTS = (0, 63, 64, 65, 255, 256, 257)
TYPE_COLUMNS = (1, 2, 17)

# inp: score_check.Inputs; group_of: int32 per moving row or None; col_of_label: int32 per label or None; mov_types: only its width is
# read (the sections of a job have one T); ref_types: float64 (reference rows, T)
Detail = collections.namedtuple("Detail", "inp group_of n_groups n_labels col_of_label mov_types ref_types")


def out_words(L, G):
    return L * L + 1 + (G + 1) * 8 + 2 * (RANKS + 1) + 1


def parts(out, L, G):
    """the words by name, in the header's order"""
    out = np.asarray(out)
    at = np.cumsum([0, L * L, 1, (G + 1) * 8, RANKS + 1, RANKS + 1, 1])
    assert len(out) == at[-1]
    cut = lambda q: out[at[q]:at[q + 1]]
    return {"confusion": cut(0).reshape(L, L), "unlabelled": int(cut(1)[0]), "groups": cut(2).reshape(G + 1, 8), "strict": cut(3),
            "weak": cut(4), "untyped": int(cut(5)[0])}


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def host_detail_counts(a_row, r_row, d, ignore_same=True, node_local=False, majority_threshold=0.5, min_flips=1):
    """-> same_merge_acc_score_detail's `out` for the final rows (a_row, r_row) under the Detail `d`, int64"""
    inp, L, G = d.inp, int(d.n_labels), int(d.n_groups)
    a_row, r_row = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    code_m, code_r = np.asarray(inp.code_m, np.int64), np.asarray(inp.code_r, np.int64)
    n_mov = len(np.asarray(inp.mov_xy).reshape(-1, 2))
    assert len(np.unique(a_row)) == len(a_row) and (len(a_row) == 0 or (0 <= a_row.min() and a_row.max() < n_mov))
    group = np.zeros(n_mov, np.int64) if d.group_of is None else np.asarray(d.group_of, np.int64)
    assert len(group) == n_mov and (len(group) == 0 or group.max() < G)
    group = np.where(group < 0, G, group)                        # no group: the cross bin
    confusion, groups = np.zeros((L, L), np.int64), np.zeros((G + 1, 8), np.int64)
    strict_hist, weak_hist = np.zeros(RANKS + 1, np.int64), np.zeros(RANKS + 1, np.int64)
    cm, cr = code_m[a_row], code_r[r_row]
    labelled = (cm >= 0) & (cm < L) & (cr >= 0) & (cr < L)
    np.add.at(confusion, (cm[labelled], cr[labelled]), 1)
    unlabelled = int(len(a_row) - labelled.sum())
    np.add.at(groups[:, 0], group[a_row], 1)
    np.add.at(groups[:, 1], group[a_row][(cm >= 0) & (cm == cr)], 1)
    # ranks
    types = np.asarray(d.ref_types, np.float64)
    T = types.shape[1]
    col = np.full(len(a_row), -1, np.int64)
    if d.col_of_label is not None:
        known = (cm >= 0) & (cm < L)
        col[known] = np.asarray(d.col_of_label, np.int64)[cm[known]]
    untyped = 0
    for r, c in zip(r_row.tolist(), col.tolist()):
        row = types[r]
        if c < 0 or np.isnan(row).any():
            untyped += 1
            continue
        others = np.delete(row, c)
        strict_hist[min(int((others > row[c]).sum()), RANKS)] += 1
        weak_hist[min(int((others >= row[c]).sum()), RANKS)] += 1
    assert T == np.asarray(d.mov_types).shape[1]
    # triangles
    if inp.tris is not None and len(inp.tris):
        t = np.asarray(inp.tris, np.int64).reshape(-1, 3)
        matched, same, flipped, _b, _a = S.host_triangles(a_row, r_row, inp.mov_xy, inp.ref_xy, code_m, t, ignore_same)
        g3 = group[t]
        tri_bin = np.where((g3[:, 0] == g3[:, 1]) & (g3[:, 0] == g3[:, 2]), g3[:, 0], G)
        for word, flag in ((2, np.ones(len(t), bool)), (3, matched), (4, same), (5, flipped), (6, flipped & ~same)):
            np.add.at(groups[:, word], tri_bin[flag], 1)
        node_tri, node_flip = np.zeros(n_mov, np.int64), np.zeros(n_mov, np.int64)
        within = tri_bin < G
        np.add.at(node_tri, t[matched & ~same & within].reshape(-1), 1)
        np.add.at(node_flip, t[flipped & ~same & within].reshape(-1), 1)
        violating = S.node_rule(node_tri[a_row], node_flip[a_row], node_local, majority_threshold, min_flips)
        np.add.at(groups[:, 7], group[a_row][violating], 1)
        assert groups[G, 7] == 0
    return np.concatenate((confusion.reshape(-1), [unlabelled], groups.reshape(-1), strict_hist, weak_hist, [untyped])).astype(np.int64)


# ---- the families ------------------------------------------------------------------------------------------------------------------------
def _types(rng, n, T):
    """rows of T distinct values"""
    return np.argsort(rng.random((n, T)), axis=1).astype(np.float64) + rng.random((n, 1))


def quadrants(xy):
    """four groups by the medians of X and Y"""
    xy = np.asarray(xy)
    return ((xy[:, 0] > np.median(xy[:, 0])).astype(np.int32) + 2 * (xy[:, 1] > np.median(xy[:, 1])).astype(np.int32)).astype(np.int32)


def plain(job, inp=None, seed=21, T=6):
    """the job's own codes as labels (L = the largest code + 1), four quadrant groups with one row in eleven in none, T distinct-valued
    type columns, every label naming a column but the last"""
    rng = np.random.default_rng(seed)
    inp = S.own(job) if inp is None else inp
    L = int(max(job.code_m.max(), job.code_r.max())) + 1
    group = quadrants(inp.mov_xy)
    group[::11] = -1
    col = (np.arange(L) % T).astype(np.int32)
    col[-1] = -1
    return Detail(inp, group, 4, L, col, np.zeros((len(inp.mov_xy), T)), _types(rng, len(inp.ref_xy), T))


def label_counts(job, seed=22):
    """L = 1 (every other code is >= L: unlabelled, untyped) and L at the cap with codes over all of 0 .. 63"""
    rng = np.random.default_rng(seed)
    base = plain(job)
    one = base._replace(n_labels=1, col_of_label=np.zeros(1, np.int32))
    inp = base.inp._replace(code_m=rng.integers(0, MAX_LABELS, len(base.inp.code_m)).astype(np.int32),
                            code_r=rng.integers(0, MAX_LABELS, len(base.inp.code_r)).astype(np.int32))
    cap = base._replace(inp=inp, n_labels=MAX_LABELS, col_of_label=(np.arange(MAX_LABELS) % 6).astype(np.int32))
    return [("L = 1", one), ("L at the cap", cap)]


def label_codes(job):
    """score_check's negative and largest codes under the job's own L"""
    base = plain(job)
    return [(f"codes: {name}", base._replace(inp=inp)) for name, inp in S.codes(job) if name in ("negative", "largest")]


def group_families(job, seed=23):
    rng = np.random.default_rng(seed)
    base = plain(job)
    n = len(base.inp.mov_xy)
    ones = np.full(n, -1, np.int32)
    ones[job.a_row[:MAX_GROUPS]] = np.arange(min(MAX_GROUPS, len(job.a_row)), dtype=np.int32)
    return [("G = 1", base._replace(group_of=np.where(base.group_of < 0, -1, 0).astype(np.int32), n_groups=1)),
            ("G at the cap", base._replace(group_of=rng.integers(-1, MAX_GROUPS, n).astype(np.int32), n_groups=MAX_GROUPS)),
            ("every row in no group", base._replace(group_of=np.full(n, -1, np.int32))),
            ("one group holding all", base._replace(group_of=np.full(n, 1, np.int32), n_groups=3)),
            ("groups of one row", base._replace(group_of=ones, n_groups=MAX_GROUPS)),
            ("group_of NULL", base._replace(group_of=None, n_groups=1))]


def tri_counts(job):
    base = plain(job)
    ks = sorted({min(k, len(base.inp.tris)) for k in TRI_COUNTS})
    return [(f"{k} triangles", base._replace(inp=base.inp._replace(tris=base.inp.tris[:k]))) for k in ks]


def type_columns(job, seed=24):
    """T = 1, 2 and 17: with 17 distinct values per row a label's column has up to 16 above it -- the overflow bin"""
    rng = np.random.default_rng(seed)
    base = plain(job)
    out = []
    for T in TYPE_COLUMNS:
        col = rng.integers(-1, T, base.n_labels).astype(np.int32)
        col[0] = T - 1
        out.append((f"T = {T}", base._replace(col_of_label=col, mov_types=np.zeros((len(base.inp.mov_xy), T)),
                                              ref_types=_types(rng, len(base.inp.ref_xy), T))))
    return out


def type_rows(job, seed=25):
    """NaN and infinities over the reference type rows; rows of few distinct values (ties); no label naming a column, by -1 and by NULL"""
    rng = np.random.default_rng(seed)
    base = plain(job)
    hostile = base.ref_types.copy()
    n, T = hostile.shape
    for value in (np.nan, np.inf, -np.inf):
        rows = rng.choice(n, max(2, n // 12), replace=False)
        hostile[rows, rng.integers(0, T, len(rows))] = value
    hostile[rng.choice(n, max(2, n // 30), replace=False)] = np.inf          # every column +inf: weak = T - 1, strict = 0
    ties = rng.integers(0, 3, (n, T)).astype(np.float64)
    ties[::5] = 0.0
    ties[1::7, ::2] = -0.0                                                     # signed zeros compare equal
    return [("NaN and infinities", base._replace(ref_types=hostile)), ("equal columns", base._replace(ref_types=ties)),
            ("col_of_label all -1", base._replace(col_of_label=np.full(base.n_labels, -1, np.int32))),
            ("col_of_label NULL", base._replace(col_of_label=None))]


def grown(job):
    """score_check's moving section of 5000 more rows, the new rows in a group of their own"""
    inp = S.grown(job)
    base = plain(job, inp)
    group = base.group_of.copy()
    group[len(job.mov_xy):] = 4
    return base._replace(group_of=group, n_groups=5)


def all_families(job):
    out = [("plain", plain(job))]
    for family in (label_counts, label_codes, group_families, tri_counts, type_columns, type_rows):
        out += family(job)
    out += [("hostile geometry: " + f.__name__, plain(job, f(job))) for f in (S.degenerate, S.nonfinite)]
    out.append(("grown", grown(job)))
    return out


def small_families(job):
    return [("plain", plain(job))] + group_families(job) + tri_counts(job) + type_columns(job) + type_rows(job)
