"""The host statement of same_merge_acc_unpack_detail (csrc/window_unpack_detail.hip) and the specs its tests bin by.

`host_unpack_detail` is built on tests/unpack_check.py's `host_unpack` -- scipy's cdist, np.tile and linear_sum_assignment from the
reference's text -- with numpy for the bins and the ranks; nothing of libsame_hip is in it.  A spec says what the pairs are binned by:
the number of cell-level labels, the member codes (negative ones and codes at or above the label count among them), the labels' type
columns, the reference members' type rows, the moving rows' groups.  tests/test_unpack_detail_check_cpu.py holds the statement against a
per-pair Python loop, `score_details.label_ranks` / `top_k_counts` and pd.crosstab; tests/test_gpu_unpack_detail_library.py holds the
library call against the statement."""
import collections

import numpy as np

import unpack_check as U

RANKS, MAX_LABELS, MAX_GROUPS = 16, 64, 256

# what the pairs are binned by.  mov_code / ref_code: the members' codes under this spec (the lists and XY are the family's);
# col_of_label None: no label names a column; ref_types None: no type rows; group_of None: no groups object (one group, 0)
Spec = collections.namedtuple("Spec", "name n_labels mov_code ref_code col_of_label ref_types group_of n_groups expects")


def out_words(L, G):
    """SAME_UNPACK_DETAIL_WORDS"""
    return 4 + L * L + 1 + (G + 1) * 2 + 2 * (RANKS + 1) + 1


def parts(out, L, G):
    """the words by name, in the order include/same_hip.h states"""
    at = np.cumsum([0, 4, L * L, 1, (G + 1) * 2, RANKS + 1, RANKS + 1, 1])
    assert len(out) == at[-1] == out_words(L, G)
    cut = lambda q: out[at[q]:at[q + 1]]
    return {"counts": cut(0), "confusion": cut(1).reshape(L, L), "unlabelled": int(cut(2)[0]), "groups": cut(3).reshape(G + 1, 2),
            "strict": cut(4), "weak": cut(5), "untyped": int(cut(6)[0])}


def with_codes(fam, spec):
    """the family's lists and XY under the spec's member codes"""
    return fam._replace(mov_code=spec.mov_code, ref_code=spec.ref_code)


def pairs_of(a_row, fam, ref_member):
    """(flat moving member, moving section row) per pair: the final rows in their order, each row's members in theirs"""
    a_row = np.asarray(a_row, np.int64)
    na = np.diff(fam.mov_off)[a_row]
    row = np.repeat(a_row, na)
    within = np.arange(int(na.sum()), dtype=np.int64) - np.repeat(np.cumsum(na) - na, na)
    mov_member = fam.mov_off[row] + within
    assert len(mov_member) == len(ref_member)
    return mov_member, row


def host_unpack_detail(a_row, r_row, fam, strategy, spec, unpacked=None):
    """-> the int64 words of same_merge_acc_unpack_detail's `out` for the final rows (a_row, r_row), the family's lists under the spec's
    codes, and the spec.  `unpacked`: `host_unpack`'s answer for these lists and XY where it is known already (the pairs do not depend on
    the codes; the agreeing pairs are counted here)."""
    fam = with_codes(fam, spec)
    counts, ref_member = unpacked if unpacked is not None else U.call(fam, a_row, r_row, strategy)
    mov_member, row = pairs_of(a_row, fam, ref_member)
    L, G = spec.n_labels, spec.n_groups
    cm, cr = fam.mov_code[mov_member].astype(np.int64), fam.ref_code[ref_member].astype(np.int64)
    P = len(cm)
    lm, lr = (cm >= 0) & (cm < L), (cr >= 0) & (cr < L)
    agree = (cm >= 0) & (cm == cr)
    confusion = np.zeros(L * L, np.int64)
    np.add.at(confusion, (cm * L + cr)[lm & lr], 1)
    group = np.zeros(P, np.int64) if spec.group_of is None else spec.group_of[row].astype(np.int64)
    group = np.where((group >= 0) & (group < G), group, G)
    groups = np.zeros((G + 1, 2), np.int64)
    np.add.at(groups[:, 0], group, 1)
    np.add.at(groups[:, 1], group[agree], 1)
    strict_hist, weak_hist = np.zeros(RANKS + 1, np.int64), np.zeros(RANKS + 1, np.int64)
    typed = np.zeros(P, bool)
    if spec.col_of_label is not None and spec.ref_types is not None and P:
        T = spec.ref_types.shape[1]
        c = np.where(lm, spec.col_of_label[np.where(lm, cm, 0)], -1).astype(np.int64) if L else np.full(P, -1)
        rows = spec.ref_types[ref_member]
        typed = (c >= 0) & ~np.isnan(rows).any(axis=1)
        at = np.arange(P)
        v = rows[at, np.maximum(c, 0)]
        strict, weak = np.zeros(P, np.int64), np.zeros(P, np.int64)
        with np.errstate(invalid="ignore"):
            for t in range(T):
                other = c != t
                strict += other & (rows[:, t] > v)
                weak += other & (rows[:, t] >= v)
        np.add.at(strict_hist, np.minimum(strict[typed], RANKS), 1)
        np.add.at(weak_hist, np.minimum(weak[typed], RANKS), 1)
    head = np.array([counts[0], P, int(agree.sum()), counts[3]], np.int64)
    return np.concatenate([head, confusion, [P - int((lm & lr).sum())], groups.reshape(-1), strict_hist, weak_hist, [P - int(typed.sum())]]).astype(np.int64)


# ---- the specs -----------------------------------------------------------------------------------------------------------------------------
def hostile_types(rng, m, T):
    """type rows of small integers (ties everywhere), with +-inf, -0.0 beside 0.0 and rows that hold a NaN"""
    t = rng.integers(0, 3, (m, T)).astype(np.float64)
    t[rng.random((m, T)) < 0.08] = -0.0
    t[rng.random((m, T)) < 0.05] = np.inf
    t[rng.random((m, T)) < 0.05] = -np.inf
    nan_rows = rng.random(m) < 0.1
    t[nan_rows, rng.integers(0, T, int(nan_rows.sum()))] = np.nan
    return t


def specs(fam, n_mov, seed=0):
    """[Spec] over a family's members and a moving section of n_mov rows: L in {1, 5, 64}, G in {none, 3, 256}, T in {1, 2, 17}; member
    codes from -1 to L (a negative code and one at the label count on both sides); groups from -1 (no group); type rows with ties,
    infinities, signed zeros and NaNs; labels that name no column; no columns at all; one spec that puts every pair into a single bin"""
    rng = np.random.default_rng(seed)
    m_m, m_r = len(fam.mov_code), len(fam.ref_code)
    def side(L, m):                            # about one code in seven negative, one in seven at the label count
        c, u = rng.integers(0, L, m), rng.random(m)
        return np.where(u < 0.14, -1, np.where(u < 0.28, L, c)).astype(np.int32)

    codes = lambda L: (side(L, m_m), side(L, m_r))
    groups = lambda G: rng.integers(-1, G, n_mov).astype(np.int32)
    cols = lambda L, T: rng.integers(-1, T, L).astype(np.int32)
    out = [Spec("L 1, no groups, T 1", 1, *codes(1), np.zeros(1, np.int32), rng.random((m_r, 1)), None, 1, {"pairs"})]
    c5 = np.array([0, 1, -1, 0, 1], np.int32)
    out.append(Spec("L 5, G 3, T 2, ties", 5, *codes(5), c5, rng.integers(0, 2, (m_r, 2)).astype(np.float64), groups(3), 3,
                    {"pairs", "off-diagonal", "tied"}))
    out.append(Spec("L 64, G 256, T 17, hostile rows", 64, *codes(64), cols(64, 17), hostile_types(rng, m_r, 17), groups(256), 256,
                    {"pairs", "off-diagonal", "tied", "nan"}))
    out.append(Spec("L 5, T 2, hostile rows, no groups", 5, *codes(5), c5, hostile_types(rng, m_r, 2), None, 1,
                    {"pairs", "off-diagonal", "tied", "nan"}))
    out.append(Spec("no label names a column", 5, *codes(5), None, None, groups(3), 3, {"pairs", "off-diagonal", "all untyped"}))
    out.append(Spec("every pair in one bin", 1, np.zeros(m_m, np.int32), np.zeros(m_r, np.int32), np.zeros(1, np.int32), np.full((m_r, 1), 2.5),
                    None, 1, {"pairs", "one bin"}))
    return out


def check_not_vacuous(p, spec, ks=(1, 2, 3)):
    """what the spec was made to show is in the words `p` (parts)"""
    pairs = int(p["counts"][1])
    assert pairs > 0, spec.name
    assert p["confusion"].sum() + p["unlabelled"] == pairs == p["groups"][:, 0].sum() == p["weak"].sum() + p["untyped"], spec.name
    assert p["strict"].sum() == p["weak"].sum() and p["groups"][:, 1].sum() == p["counts"][2], spec.name
    if "off-diagonal" in spec.expects:
        off = p["confusion"] - np.diag(np.diag(p["confusion"]))
        assert (off > 0).sum() >= 2 and p["unlabelled"] > 0, spec.name
    if "tied" in spec.expects:
        assert any(p["strict"][:k].sum() > p["weak"][:k].sum() for k in ks), spec.name
    if "nan" in spec.expects:
        assert p["untyped"] > 0 and p["weak"].sum() > 0, spec.name
    if "all untyped" in spec.expects:
        assert p["untyped"] == pairs, spec.name
    if "one bin" in spec.expects:
        assert p["confusion"].tolist() == [[pairs]] and p["groups"].tolist() == [[pairs, pairs], [0, 0]], spec.name
        assert p["strict"][0] == p["weak"][0] == pairs and p["untyped"] == p["unlabelled"] == 0, spec.name
