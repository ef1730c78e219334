"""The parts of same_amd.sliding_window_score_details (score_details.py, csrc/window_score_detail.hip) that need no GPU: the host statement
tests/score_details_check.py holds the library against, checked on the recorded output of the reference's
check_triangle_violations_within_quadrants (tests/golden/score_details.npz, tools/gen_score_details_golden.py) and for additivity against
tests/score_check.py's `host_counts`; each hostile family for the property it is named for; `top_k_counts` against np.argpartition and
under the best and worst tie orders; `score_table_details` without a triangulation against the statement; the ValueErrors; the ABI
surface.  Every test fails without the feature: the names do not exist.

(`score_table_details` WITH a triangulation calls check_triangle_violations, whose triangle kernel runs on the device: its golden and
additivity tests are in tests/test_gpu_score_details.py.)"""
import os
import re

import numpy as np
import pandas as pd
import pytest

import score_check as S
import score_details_check as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADRANTS = ("top_left", "top_right", "bottom_right", "bottom_left")
FLAGGED = {"top_left": 6, "top_right": 0, "bottom_right": 25, "bottom_left": 22}


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "score_details.npz"))
    return {k: z[k] for k in z.files}


def golden_detail(g):
    """the fixture as a Detail: quadrants as groups in QUADRANTS' order, labels c1..c3 naming their columns"""
    labels = list(g["commonCT"])
    code = lambda a: np.array([labels.index(v) for v in a], np.int32)
    group = np.array([QUADRANTS.index(q) for q in g["mov_quadrant"]], np.int32)
    inp = S.Inputs(g["mov_xy"], g["ref_xy"], code(g["mov_cell_type"]), code(g["ref_cell_type"]), g["tris"])
    return D.Detail(inp, group, 4, 3, np.arange(3, dtype=np.int32), g["mov_types"], g["ref_types"])


# ---- the golden --------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_issue_describes():
    g = golden()
    assert len(g["a_row"]) == len(g["mov_xy"]) == 372 and len(np.unique(g["r_row"])) == 372 and g["tris"].shape == (728, 3)
    q = g["mov_quadrant"][g["tris"]]
    assert int((~((q[:, 0] == q[:, 1]) & (q[:, 0] == q[:, 2]))).sum()) == 81
    flagged = g["triangle_violation"]
    assert flagged.dtype == bool and {k: int(flagged[g["mov_quadrant"][g["a_row"]] == k].sum()) for k in QUADRANTS} == FLAGGED
    match_of = np.full(372, -1)
    match_of[g["a_row"]] = g["r_row"]
    area = lambda xy, t: S.signed_area(xy[t[:, 0]], xy[t[:, 1]], xy[t[:, 2]])
    assert min(np.abs(area(g["mov_xy"], g["tris"])).min(), np.abs(area(g["ref_xy"], match_of[g["tris"]])).min()) >= 1e-9


def test_the_statement_gives_the_references_rows_and_counts_per_quadrant():
    """without the same-type rule and under the any-flip rule the per-group restriction flags exactly the rows the reference's function
    flags: the node word of every quadrant is its count, and the rows themselves are the same"""
    g = golden()
    d = golden_detail(g)
    out = D.parts(D.host_detail_counts(g["a_row"], g["r_row"], d, ignore_same=False), 3, 4)
    assert out["groups"][:4, 7].tolist() == [FLAGGED[q] for q in QUADRANTS] and out["groups"][4, 7] == 0
    assert out["groups"][4, 2] == 81 and out["groups"][:, 2].sum() == 728 and out["groups"][:4, 0].sum() == 372 and out["groups"][4, 0] == 0
    # the rows: corners of a flipped triangle whose corners share a quadrant
    matched, _same, flipped, _b, _a = S.host_triangles(g["a_row"], g["r_row"], g["mov_xy"], g["ref_xy"], d.inp.code_m, g["tris"], False)
    grp = d.group_of[g["tris"]]
    within = (grp[:, 0] == grp[:, 1]) & (grp[:, 0] == grp[:, 2])
    rows = np.zeros(372, bool)
    rows[g["tris"][matched & flipped & within].reshape(-1)] = True
    assert np.array_equal(rows[g["a_row"]], g["triangle_violation"])
    # one group holding all is same_merge_acc_score's record
    whole = d._replace(group_of=None, n_groups=1)
    counts = S.host_counts(g["a_row"], g["r_row"], g["mov_xy"], g["ref_xy"], d.inp.code_m, d.inp.code_r, g["tris"], False)[0]
    assert D.parts(D.host_detail_counts(g["a_row"], g["r_row"], whole, ignore_same=False), 3, 1)["groups"][0].tolist() == counts.tolist()


# ---- additivity and the families ---------------------------------------------------------------------------------------------------------
JOB = S.synthetic_job()


@pytest.mark.parametrize("rule", [(False, 0.5, 1), (True, 0.5, 1), (True, 1.0 / 3.0, 2)])
def test_words_one_to_seven_sum_to_the_score_calls_counts(rule):
    for name, d in D.all_families(JOB):
        for ignore_same in (True, False):
            out = D.host_detail_counts(JOB.a_row, JOB.r_row, d, ignore_same, *rule)
            assert len(out) == D.out_words(d.n_labels, d.n_groups) and out.dtype == np.int64
            p = D.parts(out, d.n_labels, d.n_groups)
            inp = d.inp
            want = S.host_counts(JOB.a_row, JOB.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.code_r, inp.tris, ignore_same, *rule)[0]
            assert p["groups"][:, :7].sum(axis=0).tolist() == want[:7].tolist(), name
            assert p["groups"][d.n_groups, 7] == 0
            assert p["confusion"].sum() + p["unlabelled"] == len(JOB.a_row) == p["strict"].sum() + p["untyped"] == p["weak"].sum() + p["untyped"]
            assert np.trace(p["confusion"]) <= want[1]
            if d.group_of is None or (d.n_groups == 3 and (d.group_of == 1).all()):          # one group holding all: the score call's record
                assert p["groups"][0 if d.group_of is None else 1].tolist() == want.tolist(), name


def test_every_family_has_the_property_it_is_named_for():
    fam = dict(D.all_families(JOB))
    n = len(JOB.a_row)
    part = lambda name: D.parts(D.host_detail_counts(JOB.a_row, JOB.r_row, fam[name]), fam[name].n_labels, fam[name].n_groups)
    base = part("plain")
    assert base["unlabelled"] == 0 and base["untyped"] > 0 and (base["groups"][:, 0] > 0).all() and base["groups"][:4, 7].sum() > 0
    assert base["groups"][4, 2] > 0 and base["strict"].tolist() == base["weak"].tolist()        # distinct values: no ties
    one = part("L = 1")
    assert one["confusion"].shape == (1, 1) and 0 < one["confusion"][0, 0] < n and one["unlabelled"] == n - one["confusion"][0, 0]
    cap = part("L at the cap")
    assert fam["L at the cap"].n_labels == D.MAX_LABELS and (cap["confusion"] > 0).sum() > 1000 and cap["unlabelled"] == 0
    assert part("codes: negative")["unlabelled"] > 0 and part("codes: largest")["unlabelled"] > 0
    assert part("G = 1")["groups"].shape == (2, 8) and part("G = 1")["groups"][1, 0] > 0
    g_cap = part("G at the cap")
    assert g_cap["groups"].shape == (D.MAX_GROUPS + 1, 8) and (g_cap["groups"][:, 0] > 0).sum() > 250 and g_cap["groups"][[0, -2, -1], 0].all() and g_cap["groups"][-1, 2] > g_cap["groups"][:-1, 2].sum()
    none = part("every row in no group")
    assert none["groups"][:4].sum() == 0 and none["groups"][4, 0] == n and none["groups"][4, 5] > 0 and none["groups"][4, 7] == 0
    assert part("one group holding all")["groups"][[0, 2, 3]].sum() == 0
    single = part("groups of one row")
    assert (single["groups"][:-1, 0] == 1).all() and single["groups"][:-1, 2:].sum() == 0       # no triangle has three corners in one row
    assert part("group_of NULL")["groups"][1].sum() == 0
    counts = [int(name.split()[0]) for name in fam if name.endswith(" triangles")]
    assert counts == list(D.TRI_COUNTS)
    for k in counts:
        assert part(f"{k} triangles")["groups"][:, 2].sum() == k
    for T in D.TYPE_COLUMNS:
        p = part(f"T = {T}")
        assert fam[f"T = {T}"].ref_types.shape[1] == T and p["strict"][T:].sum() == 0 and p["strict"][:T].sum() > 0
    assert part("T = 17")["strict"][D.RANKS] > 0 and part("T = 1")["strict"][0] == part("T = 1")["weak"][0] > 0
    hostile = fam["NaN and infinities"].ref_types
    assert np.isnan(hostile).any() and np.isposinf(hostile).any() and np.isneginf(hostile).any() and np.isposinf(hostile).all(axis=1).any()
    assert part("NaN and infinities")["untyped"] > base["untyped"]
    ties = part("equal columns")
    assert ties["strict"].tolist() != ties["weak"].tolist() and ties["weak"][5] > 0
    for name in ("col_of_label all -1", "col_of_label NULL"):
        assert part(name)["untyped"] == n and part(name)["strict"].sum() == 0
    big = fam["grown"]
    assert len(big.inp.mov_xy) == len(JOB.mov_xy) + S.GROWN_ROWS and part("grown")["groups"][4, 2] > 0 and part("grown")["groups"][4, 0] == 0


# ---- top_k_counts ------------------------------------------------------------------------------------------------------------------------
def test_top_k_counts_against_argpartition_on_rows_of_distinct_values():
    from same_amd import top_k_counts

    rng = np.random.default_rng(3)
    columns = [f"t{q}" for q in range(9)]
    rows = np.argsort(rng.random((500, 9)), axis=1).astype(np.float64) * 0.37 - 1.0
    labels = rng.choice(columns + ["other"], 500)
    ks = (1, 2, 3, 9, 16)
    got = top_k_counts(labels, rows, columns, ks)
    named = labels != "other"
    assert got["typed_rows"] == int(named.sum())
    at = np.array([columns.index(v) if v in columns else -1 for v in labels])
    for k in ks:
        kk = min(k, 9)
        top = np.argpartition(-rows, kk - 1, axis=1)[:, :kk]
        assert got[f"top{k}_matches"] == int((named & (top == at[:, None]).any(axis=1)).sum()) and got[f"top{k}_tied"] == 0
    assert list(got) == ["typed_rows"] + [f"top{k}_{w}" for k in ks for w in ("matches", "tied")]


def test_top_k_counts_under_the_best_and_the_worst_tie_order():
    from same_amd import top_k_counts

    rng = np.random.default_rng(4)
    columns = list("abcdef")
    rows = rng.integers(0, 3, (400, 6)).astype(np.float64)
    rows[:5] = np.nan
    labels = rng.choice(columns, 400)
    at = np.array([columns.index(v) for v in labels])
    typed = ~np.isnan(rows).any(axis=1)
    for k in (1, 2, 3):
        got = top_k_counts(labels, rows, columns, [k])
        # a stable descending order after the label's column is moved first (best) or last (worst) among its equals
        hits = {}
        for name, nudge in (("best", 1e-6), ("worst", -1e-6)):
            keyed = rows.copy()
            keyed[np.arange(400), at] += nudge
            order = np.argsort(-keyed, axis=1, kind="stable")[:, :k]
            hits[name] = int((typed & (order == at[:, None]).any(axis=1)).sum())
        assert hits["worst"] == got[f"top{k}_matches"] and hits["best"] == got[f"top{k}_matches"] + got[f"top{k}_tied"]
        assert got[f"top{k}_tied"] > 0 and got["typed_rows"] == 395


# ---- score_table_details without a triangulation ------------------------------------------------------------------------------------------
def _small_study(seed, n=120, n_rows=90):
    """two frames and a table over them: labels a..d (one reference label the moving frame lacks), four regions with missing values"""
    rng = np.random.default_rng(seed)
    cols = ["a", "b", "c", "d"]
    frame = lambda labels, ids: pd.DataFrame({"Cell_Num_Old": ids, "X": rng.random(n) * 50, "Y": rng.random(n) * 50,
                                              "cell_type": rng.choice(labels, n), **{c: rng.integers(0, 4, n).astype(float) for c in cols}})
    ref, mov = frame(cols + ["e"], rng.permutation(n) + 1000), frame(cols[:3] + ["zz"], rng.permutation(n) + 5)
    region = rng.choice(np.array(["n", "e", "s", "w", None], dtype=object), n)
    mov["region"] = region
    a, r = rng.choice(n, n_rows, replace=False), rng.choice(n, n_rows, replace=False)
    table = pd.DataFrame({"Aligned_Cell_Num_Old": mov["Cell_Num_Old"].to_numpy()[a], "Ref_Cell_Num_Old": ref["Cell_Num_Old"].to_numpy()[r],
                          "ref_X": ref["X"].to_numpy()[r], "ref_Y": ref["Y"].to_numpy()[r]})
    return ref, mov, cols, table, a, r


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_score_table_details_without_a_triangulation_equals_the_statement(seed):
    import same_amd
    from same_amd.score_details import checked_groups, joint_labels, label_columns

    ref, mov, cols, table, a, r = _small_study(seed)
    got = same_amd.score_table_details(table, ref, mov, cell_id_col="Cell_Num_Old", commonCT=cols, group_by="region", top_k={1, 2, 3})
    assert isinstance(got, same_amd.ScoreDetails)
    code_m, code_r, labels = joint_labels(mov["cell_type"].to_numpy(), ref["cell_type"].to_numpy())
    group, names = checked_groups("region", mov)
    assert (group < 0).any() and sorted(names) == ["e", "n", "s", "w"] and names == list(pd.unique(mov["region"].dropna()))
    L, G = len(labels), len(names)
    d = D.Detail(S.Inputs(mov[["X", "Y"]].to_numpy(), ref[["X", "Y"]].to_numpy(), code_m, code_r, None), group, G, L,
                 label_columns(labels, cols), mov[cols].to_numpy(), ref[cols].to_numpy())
    want = D.parts(D.host_detail_counts(a, r, d), L, G)
    assert got.confusion.to_numpy().tolist() == want["confusion"].tolist() and got.confusion.to_numpy().dtype == np.int64
    assert list(got.confusion.index) == labels == list(got.confusion.columns) and got.confusion.index.name == "moving_label"
    assert got.groups["group"].tolist() == names and list(got.groups.columns) == ["group", "matched", "type_matches", "accuracy"]
    assert got.groups["matched"].tolist() == want["groups"][:G, 0].tolist() and got.groups["type_matches"].tolist() == want["groups"][:G, 1].tolist()
    assert got.cross["matched"].tolist() == [want["groups"][G, 0]] and got.cross["type_matches"].tolist() == [want["groups"][G, 1]]
    # additivity: groups + cross = score_table's record
    record = same_amd.score_table(table, ref, mov, cell_id_col="Cell_Num_Old")
    assert got.scores.iloc[0].to_dict() == record
    for k in ("matched", "type_matches"):
        assert got.groups[k].sum() + got.cross[k].iloc[0] == record[k]
    top = got.top_k.iloc[0]
    assert top["typed_rows"] == want["weak"].sum() and list(got.top_k.columns) == ["typed_rows"] + [f"top{k}_{w}" for k in (1, 2, 3)
                                                                                                    for w in ("matches", "tied", "accuracy")]
    for k in (1, 2, 3):
        assert top[f"top{k}_matches"] == want["weak"][:k].sum() and top[f"top{k}_tied"] == want["strict"][:k].sum() - want["weak"][:k].sum()
        assert top[f"top{k}_accuracy"] == 100 * (int(top[f"top{k}_matches"]) / len(table))
    plain = same_amd.score_table_details(table, ref, mov, cell_id_col="Cell_Num_Old", commonCT=cols)
    assert plain.groups is None and plain.cross is None and plain.top_k is None and plain.confusion.equals(got.confusion)
    empty = same_amd.score_table_details(pd.DataFrame(), ref, mov, cell_id_col="Cell_Num_Old", commonCT=cols, group_by="region", top_k=[1])
    assert empty.confusion.to_numpy().sum() == 0 and empty.groups["matched"].tolist() == [0] * G and empty.top_k["typed_rows"].tolist() == [0]


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_anything_is_touched():
    import same_amd

    ref, mov, cols, table, _a, _r = _small_study(5)
    run = lambda **kw: same_amd.sliding_window_score_details(ref, mov, cols, **kw)
    for bad in (0, 17, (1, 2.5), "3", (True,), 3, {1: 2}, (-1,)):
        with pytest.raises(ValueError, match="top_k"):
            run(top_k=bad)
        with pytest.raises(ValueError, match="top_k"):
            same_amd.score_table_details(table, ref, mov, cell_id_col="Cell_Num_Old", commonCT=cols, top_k=bad)
    for bad in ("no_such_column", np.zeros(len(mov) - 1), np.zeros((len(mov), 2))):
        with pytest.raises(ValueError, match="group_by"):
            run(group_by=bad)
        with pytest.raises(ValueError, match="group_by"):
            same_amd.score_table_details(table, ref, mov, cell_id_col="Cell_Num_Old", commonCT=cols, group_by=bad)
    with pytest.raises(ValueError, match="score_params"):
        run(group_by="region", score_params={"no_such_key": 1})
    with pytest.raises(ValueError, match="cell_type"):
        same_amd.sliding_window_score_details(ref.drop(columns="cell_type"), mov, cols, group_by="region")
    with pytest.raises(TypeError):
        run(tables=True)
    with pytest.raises(TypeError):
        run(unpack="nearest")


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_the_abi_stays_9():
    from same_amd import _lib, score_details, windows

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in re.sub(r"[ \t]+", " ", header) and _lib.ABI_VERSION == 9
    for name, n_args in (("same_score_detail_create", 6), ("same_score_detail_destroy", 1), ("same_merge_acc_score_detail", 11)):
        assert re.search(rf"\b(int|void)\s+{name}\(", header), name
        assert name in _lib.EXPORTS and len(_lib._PROTOTYPES[name]) == n_args
    assert header.index("int same_merge_acc_score(") < header.index("same_score_detail_create(") < header.index("same_members_create(")
    caps = {k: int(v) for k, v in re.findall(r"#define (SAME_SCORE_MAX_LABELS|SAME_SCORE_MAX_GROUPS|SAME_SCORE_RANKS)\s+(\d+)", header)}
    assert caps == {"SAME_SCORE_MAX_LABELS": _lib.SAME_SCORE_MAX_LABELS, "SAME_SCORE_MAX_GROUPS": _lib.SAME_SCORE_MAX_GROUPS,
                    "SAME_SCORE_RANKS": _lib.SAME_SCORE_RANKS}
    assert caps["SAME_SCORE_MAX_LABELS"] >= 64 and caps["SAME_SCORE_MAX_GROUPS"] >= 256 and caps["SAME_SCORE_RANKS"] == 16
    assert (D.MAX_LABELS, D.MAX_GROUPS, D.RANKS) == (caps["SAME_SCORE_MAX_LABELS"], caps["SAME_SCORE_MAX_GROUPS"], caps["SAME_SCORE_RANKS"])
    assert windows.score_detail_words(5, 7) == D.out_words(5, 7) and score_details.MAX_TOP_K == 16
    split = windows.split_score_detail(np.arange(D.out_words(2, 3)), 2, 3)
    want = D.parts(np.arange(D.out_words(2, 3)), 2, 3)
    assert all(np.array_equal(split[k], want[k]) for k in want)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "same_merge_acc_score_detail") and lib.same_abi_version() == 9
    import same_amd
    for name in ("sliding_window_score_details", "score_table_details", "top_k_counts", "ScoreDetails"):
        assert name in same_amd.__all__ and getattr(same_amd, name) is getattr(score_details, name)
