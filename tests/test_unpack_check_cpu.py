"""tests/unpack_check.py's host statement of same_merge_acc_unpack held against the reference-generated fixture, the reference's own
unpack_metacell_matches (where it is mounted), the oracle's solver and the families' claimed properties; `same_amd.score_unpacked`
against the notebook cell written out; the ValueErrors of `sliding_window_scores(unpack=...)`; the ABI surface.  No GPU."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

import unpack_check as U
from conftest import ROOT, load_golden

N_MOV, N_REF, N_FINAL = 700, 650, 600


@pytest.fixture(scope="module")
def rows():
    return U.synthetic_rows(N_MOV, N_REF, N_FINAL, 5)


@pytest.fixture(scope="module")
def fams(rows):
    return U.families(*rows, N_MOV, N_REF, seed=3, library_only=True)


@pytest.fixture(scope="module")
def want(rows, fams):
    """the statement's answer per (family, strategy): computed once"""
    return {(name, s): U.call(fam, *rows, s) for name, fam in fams for s in U.STRATEGIES}


def _golden_metacells(oracle):
    """tests/test_host_rows.py:12-19"""
    from same_amd import synth

    cells = synth.make_cells(900, 3, seed=21)
    a_df = synth.to_frame(cells)
    a_df["Cell_Num_Old"] = np.arange(len(a_df)) * 2 + 5
    r_df = synth.to_frame(synth.make_jittered(cells, seed=22))
    r_df["Cell_Num_Old"] = np.arange(len(r_df)) * 3 + 1
    ma, _, _ = oracle.greedy_triangle_collapse(a_df, max_metacell_size=5, r_max=40, min_angle_deg=10)
    mr, _, _ = oracle.greedy_triangle_collapse(r_df, max_metacell_size=4, r_max=40, min_angle_deg=10)
    return a_df, r_df, ma, mr


def _csr(frame, original):
    lists = frame["members"].tolist()
    off = np.concatenate(([0], np.cumsum([len(m) for m in lists]))).astype(np.int64)
    ids = np.concatenate(lists).astype(np.int64)
    xy = original.set_index("Cell_Num_Old").loc[ids, ["X", "Y"]].to_numpy(dtype=np.float64)
    return off, ids, xy


def test_the_statement_reproduces_the_reference_fixture(oracle):
    g = load_golden("unpack_merge")
    a_df, r_df, ma, mr = _golden_metacells(oracle)
    a_row, r_row = g["mm"][:, 0], g["mm"][:, 1]
    (m_off, m_ids, m_xy), (r_off, r_ids, r_xy) = _csr(ma, a_df), _csr(mr, r_df)
    codes = np.zeros(len(m_ids), np.int32), np.zeros(len(r_ids), np.int32)
    for strategy, key in ((U.NEAREST, "unpack_near_both"), (U.DISTRIBUTE, "unpack_dist_both")):
        counts, ref_member = U.host_unpack(a_row, r_row, m_off, m_xy, codes[0], r_off, r_xy, codes[1], strategy)
        mov_member = np.concatenate([np.arange(m_off[a], m_off[a + 1]) for a in a_row])
        assert np.array_equal(np.column_stack((m_ids[mov_member], r_ids[ref_member])), g[key]), key
        assert counts.tolist() == [len(a_row), len(g[key]), len(g[key]), max(np.diff(m_off)[a_row].max(), np.diff(r_off)[r_row].max())]


def test_the_statement_equals_the_reference(rows, fams, want):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ref_loader import REF_SRC, load_reference

    if not os.path.isdir(REF_SRC):
        pytest.skip("the reference is not mounted")
    ref = load_reference().metacell_utils
    a_row, r_row = rows
    matches = pd.DataFrame({"Aligned_metacell_id": a_row.astype(np.int64), "Ref_metacell_id": r_row.astype(np.int64)})
    for name, fam in fams:
        lists = lambda off: [list(range(int(off[i]), int(off[i + 1]))) for i in range(len(off) - 1)]
        mc_a, mc_r = pd.DataFrame({"members": lists(fam.mov_off)}), pd.DataFrame({"members": lists(fam.ref_off)})
        cells_a = pd.DataFrame(fam.mov_xy, columns=["X", "Y"])
        cells_r = pd.DataFrame(fam.ref_xy, columns=["X", "Y"])
        mov_member = np.concatenate([np.arange(fam.mov_off[a], fam.mov_off[a + 1]) for a in a_row])
        for s, strategy in ((U.DISTRIBUTE, "distribute"), (U.NEAREST, "nearest")):
            got = ref.unpack_metacell_matches(matches, mc_a, mc_r, aligned_df=cells_a, ref_df=cells_r, strategy=strategy)
            counts, ref_member = want[name, s]
            assert got["Aligned_cell_id"].tolist() == mov_member.tolist() and got["Ref_cell_id"].tolist() == ref_member.tolist(), (name, strategy)
            assert counts[1] == len(got)


def test_the_nearest_picks_equal_the_oracle(oracle, rows, fams, want):
    a_row, r_row = rows
    for name, fam in fams:
        na, nr = U.row_sizes(fam, a_row, r_row)
        a_off, r_off = np.concatenate(([0], np.cumsum(na))), np.concatenate(([0], np.cumsum(nr)))
        axy = np.concatenate([fam.mov_xy[fam.mov_off[a]:fam.mov_off[a + 1]] for a in a_row])
        rxy = np.concatenate([fam.ref_xy[fam.ref_off[r]:fam.ref_off[r + 1]] for r in r_row])
        local = oracle.batched_assign(a_off, r_off, axy, rxy)
        assert np.array_equal(np.repeat(fam.ref_off[r_row], na) + local, want[name, U.NEAREST][1]), name


def test_every_family_has_its_property(rows, fams, want):
    a_row, r_row = rows
    by_name = dict(fams)
    assert len(by_name) == 7
    na, nr = U.row_sizes(by_name["grid"], a_row, r_row)
    assert {(a, r) for a, r in zip(na.tolist(), nr.tolist())} == {(a, r) for a in range(1, 7) for r in range(1, 7)}
    assert ((na == 5) & (nr == 2)).any()                    # a tiling that does not divide
    for name, fam in fams:                                   # the strategies differ wherever XY can tell members apart
        d, n = want[name, U.DISTRIBUTE], want[name, U.NEAREST]
        assert d[0][[0, 1, 3]].tolist() == n[0][[0, 1, 3]].tolist() and d[0][1] == np.diff(fam.mov_off)[a_row].sum()
        assert name in ("coincident", "lattice") or not np.array_equal(d[1], n[1]), name
        assert 0 < d[0][2] < d[0][1] and 0 < n[0][2] < n[0][1], name
    assert U.tied_rows(by_name["lattice"], a_row, r_row) > 100 > U.tied_rows(by_name["grid"], a_row, r_row) == 0
    coincident = by_name["coincident"]
    assert np.ptp(coincident.mov_xy) == 0 and np.array_equal(coincident.mov_xy[0], coincident.ref_xy[0])
    assert U.rounded_squares(by_name["offset"], a_row, r_row) > 50 and by_name["offset"].mov_xy.min() >= 1e9
    neg = by_name["negative codes"]
    mov_member = np.concatenate([np.arange(neg.mov_off[a], neg.mov_off[a + 1]) for a in a_row])
    for s in U.STRATEGIES:
        cm, cr = neg.mov_code[mov_member], neg.ref_code[want["negative codes", s][1]]
        assert ((cm < 0) & (cm == cr)).any() and (cm < 0).any() and (cr < 0).any()
        assert want["negative codes", s][0][2] == np.count_nonzero((cm >= 0) & (cm == cr)) < np.count_nonzero(cm == cr)
    empty = by_name["empty moving rows"]
    na, nr = U.row_sizes(empty, a_row, r_row)
    assert (na == 0).sum() >= N_FINAL // 3 and (nr > 0).all() and (np.diff(empty.ref_off) == 0).any()
    na, nr = U.row_sizes(by_name["large lists and 96 x 40"], a_row, r_row)
    assert {(64, 64), (64, 5), (5, 64), (96, 40)} <= set(zip(na.tolist(), nr.tolist()))
    assert want["large lists and 96 x 40", U.NEAREST][0][3] == 96
    product = dict(U.families(*rows, N_MOV, N_REF, seed=3))["large lists"]
    assert max(np.diff(product.mov_off).max(), np.diff(product.ref_off).max()) == 64


def test_a_list_against_an_empty_reference_list_is_refused(rows, fams):
    a_row, r_row = rows
    fam = dict(fams)["grid"]
    counts = np.diff(fam.ref_off).copy()
    counts[r_row[3]] = 0
    off = np.concatenate(([0], np.cumsum(counts)))
    for s in U.STRATEGIES:
        with pytest.raises(ValueError, match="empty reference list"):
            U.host_unpack(a_row, r_row, fam.mov_off, fam.mov_xy, fam.mov_code, off, fam.ref_xy, fam.ref_code, s)


# ---- score_unpacked and the checks of unpack= ------------------------------------------------------------------------------------------
def _objects(missing_label=False):
    """two small MetaCell-like objects whose member lists and labels are made by hand"""
    import types

    rng = np.random.default_rng(8)

    def side(n_cells, n_meta, id0):
        cells = pd.DataFrame({"Cell_Num_Old": id0 + 3 * np.arange(n_cells), "X": rng.uniform(0, 30, n_cells), "Y": rng.uniform(0, 30, n_cells),
                              "cell_type": rng.choice(["a", "b", "c"], n_cells).astype(object)})
        owner = np.sort(rng.integers(0, n_meta, n_cells))
        owner[:n_meta] = np.arange(n_meta)                  # every metacell has a member
        members = [cells["Cell_Num_Old"].to_numpy()[owner == q].tolist() for q in range(n_meta)]
        meta = pd.DataFrame({"metacell_id": np.arange(n_meta), "members": members})
        return types.SimpleNamespace(metacell_df=meta, original_df=cells, original_idx_col="Cell_Num_Old", metacell_idx_col="metacell_id",
                                     x_col="X", y_col="Y", cell_type_col="cell_type")

    ref, mov = side(90, 30, 1000), side(100, 28, 7)
    if missing_label:
        mov.original_df.loc[::5, "cell_type"] = None
        ref.original_df.loc[::4, "cell_type"] = None
    table = pd.DataFrame({"Aligned_metacell_id": np.arange(28), "Ref_metacell_id": rng.permutation(30)[:28]})
    return ref, mov, table


@pytest.mark.parametrize("missing_label", [False, True])
def test_score_unpacked_distribute_is_the_notebook_cell(missing_label):
    """examples/luad/reproduce_figures.ipynb cell 12 written out in pandas ('distribute' touches no kernel); a missing label equals nothing"""
    import same_amd
    from same_amd.metacell_utils import unpack_metacell_matches

    ref, mov, table = _objects(missing_label)
    rec, cells = same_amd.score_unpacked(table, ref, mov, "distribute")
    individual_matches = unpack_metacell_matches(table, mov.metacell_df, ref.metacell_df, aligned_df=mov.original_df, ref_df=ref.original_df,
                                                 strategy="distribute", aligned_original_idx_col="Cell_Num_Old",
                                                 ref_original_idx_col="Cell_Num_Old")
    ct_aligned = mov.original_df.set_index("Cell_Num_Old")["cell_type"]
    ct_ref = ref.original_df.set_index("Cell_Num_Old")["cell_type"]
    individual_matches["aligned_ct"] = individual_matches["Aligned_cell_id"].map(ct_aligned)
    individual_matches["ref_ct"] = individual_matches["Ref_cell_id"].map(ct_ref)
    individual_matches["celltype_match"] = individual_matches["aligned_ct"] == individual_matches["ref_ct"]
    assert list(rec) == ["cells_matched", "cell_type_matches", "cell_accuracy"]
    assert rec["cells_matched"] == len(individual_matches) == 100
    assert rec["cell_type_matches"] == int(individual_matches["celltype_match"].sum()) > 0
    assert rec["cell_accuracy"] == individual_matches["celltype_match"].mean() * 100
    assert cells.equals(individual_matches[["Aligned_cell_id", "Ref_cell_id"]]) and cells.dtypes.tolist() == [np.int64, np.int64]
    if missing_label:
        both_none = individual_matches["aligned_ct"].isna() & individual_matches["ref_ct"].isna()
        assert both_none.any() and not individual_matches["celltype_match"][both_none].any()
    empty, no_cells = same_amd.score_unpacked(table.iloc[:0], ref, mov, "distribute")
    assert empty["cells_matched"] == 0 == empty["cell_type_matches"] and np.isnan(empty["cell_accuracy"]) and len(no_cells) == 0


def test_unpack_is_checked_before_anything_else(monkeypatch):
    import types

    import same_amd
    from same_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    ref, mov, _table = _objects()
    cols = ["a", "b", "c"]
    for df in (ref.metacell_df, mov.metacell_df):
        df["cell_type"] = "a"
    for bad in ("closest", "Nearest", 1, True, ("nearest",)):
        with pytest.raises(ValueError, match="unpack must be None or one of"):
            same_amd.sliding_window_scores(ref, mov, cols, unpack=bad)
    with pytest.raises(ValueError, match="MetaCell objects on both sides: ref has no"):
        same_amd.sliding_window_scores(ref.metacell_df, mov, cols, unpack="nearest")
    with pytest.raises(ValueError, match="MetaCell objects on both sides: moving has no"):
        same_amd.sliding_window_scores(ref, mov.metacell_df, cols, unpack="distribute")
    for field in ("original_df", "original_idx_col"):
        lacking = types.SimpleNamespace(**{k: v for k, v in vars(mov).items() if k != field})
        with pytest.raises(ValueError, match=f"moving has no .*{field}"):
            same_amd.sliding_window_scores(ref, lacking, cols, unpack="nearest")
    no_lists = types.SimpleNamespace(**dict(vars(ref), metacell_df=ref.metacell_df.assign(members=[tuple(m) for m in ref.metacell_df["members"]])))
    no_column = types.SimpleNamespace(**dict(vars(ref), metacell_df=ref.metacell_df.drop(columns="members")))
    for bad in (no_lists, no_column):
        with pytest.raises(ValueError, match="ref.metacell_df has no 'members' column of lists"):
            same_amd.sliding_window_scores(bad, mov, cols, unpack="distribute")


def test_the_abi_surface():
    """additions do not bump the version; the three entry points are in the export table and in the library"""
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert re.search(r"^#define SAME_ABI_VERSION 9$", header, re.M)
    lib = _lib.load()
    for name in ("same_members_create", "same_members_destroy", "same_merge_acc_unpack"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(rf"\b{name}\(", header), name
