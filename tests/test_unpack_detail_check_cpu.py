"""The parts of the cell-level score details (same_amd/score_details.py, csrc/window_unpack_detail.hip) that need no GPU: the host
statement tests/unpack_detail_check.py holds the library against, checked against a per-pair Python loop, `score_details.label_ranks` /
`top_k_counts` and pd.crosstab; its sums; `score_unpacked_details` on a small MetaCell study against the notebook's np.argpartition
count; the ValueErrors; the ABI surface.  The tests of the statement (against the loop, `label_ranks` / `top_k_counts` and crosstab)
check the yardstick itself and need nothing of the feature; the tests of `score_unpacked_details`, of the arguments and of the ABI
surface fail without it: the names do not exist."""
import os
import re
import types

import numpy as np
import pandas as pd
import pytest

import unpack_check as U
import unpack_detail_check as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MOV, N_REF, N_FINAL = 90, 80, 60
A_ROW, R_ROW = U.synthetic_rows(N_MOV, N_REF, N_FINAL, seed=5)
FAMILIES = U.families(A_ROW, R_ROW, N_MOV, N_REF, seed=2)


def _loop(a_row, r_row, fam, spec, ref_member):
    """the words pair by pair, in plain Python"""
    L, G, R = spec.n_labels, spec.n_groups, D.RANKS
    confusion, groups = np.zeros((L, L), np.int64), np.zeros((G + 1, 2), np.int64)
    strict_hist, weak_hist = np.zeros(R + 1, np.int64), np.zeros(R + 1, np.int64)
    unlabelled = untyped = pairs = agreeing = 0
    for a in np.asarray(a_row).tolist():
        for i in range(int(fam.mov_off[a]), int(fam.mov_off[a + 1])):
            j = int(ref_member[pairs])
            pairs += 1
            cm, cr = int(spec.mov_code[i]), int(spec.ref_code[j])
            if 0 <= cm < L and 0 <= cr < L:
                confusion[cm, cr] += 1
            else:
                unlabelled += 1
            g = 0 if spec.group_of is None else int(spec.group_of[a])
            g = g if 0 <= g < G else G
            groups[g, 0] += 1
            if cm >= 0 and cm == cr:
                groups[g, 1] += 1
                agreeing += 1
            c = int(spec.col_of_label[cm]) if spec.col_of_label is not None and 0 <= cm < L else -1
            row = None if spec.ref_types is None else spec.ref_types[j]
            if c < 0 or row is None or any(x != x for x in row.tolist()):
                untyped += 1
                continue
            v = row[c]
            strict = sum(1 for t, x in enumerate(row.tolist()) if t != c and x > v)
            weak = sum(1 for t, x in enumerate(row.tolist()) if t != c and x >= v)
            strict_hist[min(strict, R)] += 1
            weak_hist[min(weak, R)] += 1
    return pairs, agreeing, confusion, unlabelled, groups, strict_hist, weak_hist, untyped


@pytest.mark.parametrize("which", range(len(FAMILIES)))
def test_the_statement_equals_a_loop_over_the_pairs_and_its_parts_add_up(which):
    name, fam = FAMILIES[which]
    for strategy in U.STRATEGIES:
        for spec in D.specs(fam, N_MOV, seed=which):
            counts, ref_member = U.call(D.with_codes(fam, spec), A_ROW, R_ROW, strategy)
            out = D.host_unpack_detail(A_ROW, R_ROW, fam, strategy, spec)
            assert out.dtype == np.int64 and len(out) == D.out_words(spec.n_labels, spec.n_groups)
            p = D.parts(out, spec.n_labels, spec.n_groups)
            assert p["counts"].tolist() == counts.tolist(), (name, spec.name)          # host_unpack's, under the spec's codes
            pairs, agreeing, confusion, unlabelled, groups, strict, weak, untyped = _loop(A_ROW, R_ROW, fam, spec, ref_member)
            assert (pairs, agreeing) == (p["counts"][1], p["counts"][2])
            assert np.array_equal(p["confusion"], confusion) and p["unlabelled"] == unlabelled and np.array_equal(p["groups"], groups)
            assert np.array_equal(p["strict"], strict) and np.array_equal(p["weak"], weak) and p["untyped"] == untyped, (name, spec.name)
            D.check_not_vacuous(p, spec)
            # the answer with host_unpack's pairs handed in (another family's codes): the same
            again = D.host_unpack_detail(A_ROW, R_ROW, fam, strategy, spec, unpacked=U.call(fam, A_ROW, R_ROW, strategy))
            assert np.array_equal(again, out)


def test_the_statement_against_label_ranks_top_k_counts_and_crosstab():
    from same_amd.score_details import label_ranks, top_k_counts

    name, fam = FAMILIES[0]
    for spec in D.specs(fam, N_MOV, seed=9)[1:4]:
        L = spec.n_labels
        _counts, ref_member = U.call(fam, A_ROW, R_ROW, U.NEAREST)
        p = D.parts(D.host_unpack_detail(A_ROW, R_ROW, fam, U.NEAREST, spec), L, spec.n_groups)
        mov_member, _row = D.pairs_of(A_ROW, fam, ref_member)
        cm, cr = spec.mov_code[mov_member], spec.ref_code[ref_member]
        # labels "q<code>"; a label names the column "q<first code with that column>"-- written as columns named by position
        T = spec.ref_types.shape[1]
        columns = [f"col{t}" for t in range(T)]
        name_of = lambda code: columns[spec.col_of_label[code]] if 0 <= code < L and spec.col_of_label[code] >= 0 else f"none{code}"
        labels = np.array([name_of(int(c)) for c in cm], dtype=object)
        strict, weak, typed = label_ranks(labels, spec.ref_types[ref_member], columns)
        assert int(typed.sum()) == p["weak"].sum() == len(cm) - p["untyped"]
        assert np.bincount(np.minimum(strict[typed], D.RANKS), minlength=D.RANKS + 1).tolist() == p["strict"].tolist()
        assert np.bincount(np.minimum(weak[typed], D.RANKS), minlength=D.RANKS + 1).tolist() == p["weak"].tolist()
        got = top_k_counts(labels, spec.ref_types[ref_member], columns, (1, 2, 3))
        for k in (1, 2, 3):
            assert got[f"top{k}_matches"] == p["weak"][:k].sum() and got[f"top{k}_tied"] == p["strict"][:k].sum() - p["weak"][:k].sum()
        inside = (cm >= 0) & (cm < L) & (cr >= 0) & (cr < L)
        tab = pd.crosstab(pd.Categorical(cm[inside], categories=range(L)), pd.Categorical(cr[inside], categories=range(L)), dropna=False)
        assert np.array_equal(tab.to_numpy(), p["confusion"]) and p["unlabelled"] == int((~inside).sum())


# ---- score_unpacked_details on a small MetaCell study ---------------------------------------------------------------------------------------
def _small_metacells(seed, n_cells=160, distinct=True):
    """two MetaCell-like objects over `n_cells` cells each (lists of 1 .. 4 members, every cell in one list) and a table of metacell
    matches; type rows of distinct values per row (no tie at any place) or of small integers; a region per moving metacell, some None"""
    rng = np.random.default_rng(seed)
    cols = ["a", "b", "c", "d", "e"]

    def obj(labels, id0):
        ids = rng.permutation(n_cells) + id0
        rows = (np.argsort(rng.random((n_cells, 5)), axis=1) * 0.5 - 0.25) if distinct else rng.integers(0, 3, (n_cells, 5)).astype(float)
        cells = pd.DataFrame({"Cell_Num_Old": ids, "X": rng.random(n_cells) * 90, "Y": rng.random(n_cells) * 90,
                              "cell_type": rng.choice(labels, n_cells), **{c: rows[:, q] for q, c in enumerate(cols)}})
        cuts = np.concatenate(([0], np.cumsum(rng.integers(1, 5, n_cells))))
        cuts = cuts[cuts < n_cells].tolist() + [n_cells]
        order = rng.permutation(ids)
        members = [order[a:b].tolist() for a, b in zip(cuts, cuts[1:])]
        meta = pd.DataFrame({"metacell_id": np.arange(len(members)), "members": members, "X": rng.random(len(members)) * 90,
                             "Y": rng.random(len(members)) * 90, "cell_type": rng.choice(labels, len(members))})
        return types.SimpleNamespace(metacell_df=meta, original_df=cells, original_idx_col="Cell_Num_Old", cell_type_col="cell_type",
                                     metacell_idx_col="metacell_id", x_col="X", y_col="Y")

    ref, mov = obj(cols + ["f"], 1000), obj(cols[:4] + ["zz"], 5)
    mov.metacell_df["region"] = rng.choice(np.array(["n", "e", "s", "w", None], dtype=object), len(mov.metacell_df))
    n_rows = min(len(ref.metacell_df), len(mov.metacell_df)) - 7
    table = pd.DataFrame({"Aligned_metacell_id": np.sort(rng.permutation(len(mov.metacell_df))[:n_rows]),
                          "Ref_metacell_id": rng.permutation(len(ref.metacell_df))[:n_rows]})
    return ref, mov, cols, table


@pytest.mark.parametrize("seed", [0, 1])
def test_score_unpacked_details_top_k_equals_the_notebooks_argpartition_count(seed):
    """examples/luad/reproduce_figures.ipynb cell 13 on the unpacked pairs: the moving cell's label among the k largest type columns of
    the reference CELL -- on rows of distinct values np.argpartition's answer is definite"""
    import same_amd

    ref, mov, cols, table = _small_metacells(seed)
    got = same_amd.score_unpacked_details(table, ref, mov, "distribute", commonCT=cols, group_by="region", top_k=(1, 2, 3))
    assert isinstance(got, same_amd.CellDetails)
    record, cells = same_amd.score_unpacked(table, ref, mov, "distribute")
    n = record["cells_matched"]
    assert n == len(cells) > len(table)
    aligned_ct = cells["Aligned_cell_id"].map(mov.original_df.set_index("Cell_Num_Old")["cell_type"]).to_numpy()
    xen = ref.original_df.set_index("Cell_Num_Old").loc[cells["Ref_cell_id"].to_numpy(), cols].to_numpy()
    row = got.cell_top_k.iloc[0]
    for k in (1, 2, 3):
        top = np.argpartition(-xen, k - 1, axis=1)[:, :k]
        hits = int(sum(ct in [cols[t] for t in tk] for ct, tk in zip(aligned_ct, top)))
        assert row[f"top{k}_matches"] == hits > 0 and row[f"top{k}_tied"] == 0 and row[f"top{k}_accuracy"] == 100 * (hits / n)
    assert row["typed_rows"] == int(np.isin(aligned_ct, cols).sum()) < n
    # confusion: the crosstab of the two label columns
    ref_ct = cells["Ref_cell_id"].map(ref.original_df.set_index("Cell_Num_Old")["cell_type"]).to_numpy()
    tab = pd.crosstab(aligned_ct, ref_ct)
    conf = got.cell_confusion
    assert conf.index.name == "moving_label" and conf.to_numpy().sum() == n and (conf.dtypes == np.int64).all()
    for m_label in tab.index:
        for r_label in tab.columns:
            assert conf.loc[m_label, r_label] == tab.loc[m_label, r_label]
    # groups: a pair is in its metacell row's region
    region = np.repeat(mov.metacell_df["region"].to_numpy()[table["Aligned_metacell_id"].to_numpy()],
                       [len(mov.metacell_df["members"].iloc[a]) for a in table["Aligned_metacell_id"]])
    agree = aligned_ct == ref_ct
    assert list(got.cell_groups.columns) == ["group", "cells_matched", "cell_type_matches", "cell_accuracy"]
    for _q, g in got.cell_groups.iterrows():
        assert g["cells_matched"] == int((region == g["group"]).sum()) and g["cell_type_matches"] == int((agree & (region == g["group"])).sum())
    none = pd.isna(region)
    assert got.cell_cross["cells_matched"].iloc[0] == int(none.sum()) > 0 and got.cell_cross["cell_type_matches"].iloc[0] == int((agree & none).sum())
    assert got.cell_groups["cells_matched"].sum() + int(none.sum()) == n == record["cells_matched"]
    assert got.cell_groups["cell_type_matches"].sum() + int((agree & none).sum()) == record["cell_type_matches"]
    # without group_by / top_k: None
    bare = same_amd.score_unpacked_details(table, ref, mov, "distribute", commonCT=cols)
    assert bare.cell_groups is None and bare.cell_cross is None and bare.cell_top_k is None
    pd.testing.assert_frame_equal(bare.cell_confusion, conf, check_exact=True)


def test_score_unpacked_details_counts_ties_and_an_empty_table():
    import same_amd

    ref, mov, cols, table = _small_metacells(3, distinct=False)
    got = same_amd.score_unpacked_details(table, ref, mov, "distribute", commonCT=cols, top_k=(1, 2))
    assert got.cell_top_k["top1_tied"].iloc[0] > 0 and got.cell_top_k["top2_tied"].iloc[0] > 0
    empty = same_amd.score_unpacked_details(table.iloc[:0], ref, mov, "distribute", commonCT=cols, group_by="region", top_k=(1,))
    assert empty.cell_confusion.to_numpy().sum() == 0 and empty.cell_groups["cells_matched"].sum() == 0
    assert empty.cell_top_k["typed_rows"].iloc[0] == 0 and np.isnan(empty.cell_top_k["top1_accuracy"].iloc[0])


# ---- arguments, the ABI surface --------------------------------------------------------------------------------------------------------------
def test_bad_unpack_arguments_raise_before_a_job_or_a_device_is_touched(monkeypatch):
    import same_amd
    from same_amd import scores, variants

    touched = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a job was made"))
    monkeypatch.setattr(scores, "sliding_window_variants", touched)
    monkeypatch.setattr(variants, "sliding_window_variants", touched)
    ref, mov, cols, _table = _small_metacells(4)
    with pytest.raises(ValueError, match="unpack must be None or one of"):
        same_amd.sliding_window_score_details(ref, mov, cols, unpack="bogus")
    with pytest.raises(ValueError, match="reads MetaCell objects"):
        same_amd.sliding_window_score_details(ref.metacell_df, mov.metacell_df, cols, unpack="nearest")
    lacking = types.SimpleNamespace(**vars(ref))
    lacking.original_df = ref.original_df.drop(columns="c")
    with pytest.raises(ValueError, match="original_df has no \\['c'\\]"):
        same_amd.sliding_window_score_details(lacking, mov, cols, unpack="nearest", top_k=(1, 2))
    with pytest.raises(ValueError, match="top_k"):
        same_amd.sliding_window_score_details(ref, mov, cols, unpack="nearest", top_k=(0,))
    with pytest.raises(ValueError, match="group_by"):
        same_amd.score_unpacked_details(_table, ref, mov, "distribute", commonCT=cols, group_by="no_such_column")


def test_the_entry_points_are_declared_exported_and_the_abi_stays_9():
    import same_amd
    from same_amd import _lib, windows

    header = re.sub(r"[ \t]+", " ", open(os.path.join(ROOT, "include", "same_hip.h")).read())
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    for name in ("same_unpack_detail_create", "same_unpack_detail_destroy", "same_merge_acc_unpack_detail"):
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    assert header.index("int same_merge_acc_unpack(") < header.index("same_unpack_detail_create(const same_members")
    assert "#define SAME_UNPACK_DETAIL_WORDS(L, G) (4 + (int64_t)(L) * (L) + 1 + ((int64_t)(G) + 1) * 2 + 2 * (SAME_SCORE_RANKS + 1) + 1)" in header
    for L, G in ((0, 1), (1, 1), (5, 3), (64, 256)):
        assert windows.unpack_detail_words(L, G) == D.out_words(L, G) == 4 + L * L + 1 + (G + 1) * 2 + 2 * 17 + 1
        cut = windows.split_unpack_detail(np.arange(D.out_words(L, G)), L, G)
        mine = D.parts(np.arange(D.out_words(L, G)), L, G)
        assert list(cut) == list(mine) == ["counts", "confusion", "unlabelled", "groups", "strict", "weak", "untyped"]
        for k in cut:
            assert np.array_equal(cut[k], mine[k]), k
    assert (D.RANKS, D.MAX_LABELS, D.MAX_GROUPS) == (_lib.SAME_SCORE_RANKS, _lib.SAME_SCORE_MAX_LABELS, _lib.SAME_SCORE_MAX_GROUPS)
    for name in ("CellScoreDetails", "CellDetails", "score_unpacked_details"):
        assert name in same_amd.__all__ and hasattr(same_amd, name), name
    assert same_amd.CellScoreDetails._fields == ("scores", "confusion", "groups", "cross", "top_k", "cell_confusion", "cell_groups",
                                                 "cell_cross", "cell_top_k")
    assert hasattr(windows, "DeviceUnpackDetail") and hasattr(windows.MergeAccumulator, "unpack_detail")
    # the runtime's share, as the header states it: one launch more, three copies, two waits
    assert "exactly ONE launch more than same_merge_acc_unpack" in header and "THREE copies" in header and "TWO waits" in header
