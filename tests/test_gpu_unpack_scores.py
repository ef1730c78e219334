"""`same_amd.sliding_window_scores(unpack=...)` as a product: the cell-level keys the device counts from a result's merged rows
(csrc/window_unpack.hip) equal `score_unpacked` of that result's table -- `unpack_metacell_matches` and the two label maps, the notebook
cell of examples/luad/reproduce_figures.ipynb written out here as well --, the unpacked tables equal `unpack_metacell_matches` of the
tables, and what the device does not unpack comes back the same through the tables.  Every comparison is exact."""
import copy
import functools

import numpy as np
import pandas as pd
import pytest

from test_gpu_scores import MC_OP, _records, _same_record
from test_gpu_window_variants import _variants_of

pytestmark = pytest.mark.gpu

SETS = [{}, {"knn": 3, "hip_incumbent": "assignment"}]
CELL_KEYS = ("cells_matched", "cell_type_matches", "cell_accuracy")


@functools.lru_cache(maxsize=None)
def _objects(kind):
    """(reference MetaCell, moving MetaCell, type columns) over about 1500 cells: both sides collapsed at max_metacell_size 3, or the
    moving side at 5 against 4; one original label in nine of the moving side changed, or every cell would sit on a cell of its label"""
    import same_amd
    from same_amd import synth

    cells = synth.make_cells(1500, 3, seed=71)
    r_c = synth.to_frame(cells)
    a_c = synth.to_frame(synth.make_jittered(cells, seed=72))
    a_c["Cell_Num_Old"] = np.arange(len(a_c)) * 2 + 7
    labels = a_c["cell_type"].to_numpy().copy()
    labels[::9] = np.roll(labels, 1)[::9]
    a_c["cell_type"] = labels
    ms_a, ms_r = (3, 3) if kind == "ms3" else (5, 4)
    collapse = lambda df, ms: same_amd.greedy_triangle_collapse(df, max_metacell_size=ms, r_max=40, min_angle_deg=10, return_object=True,
                                                                verbose=False)
    return collapse(r_c, ms_r), collapse(a_c, ms_a), tuple(synth.type_columns(3))


def _notebook_cell(table, mc_ref, mc_mov, strategy):
    """examples/luad/reproduce_figures.ipynb cell 12 -> (len(individual_matches), celltype_match.sum(), celltype_match.mean() * 100, the
    unpacked table)"""
    from same_amd.metacell_utils import unpack_metacell_matches

    individual_matches = unpack_metacell_matches(table, mc_mov.metacell_df, mc_ref.metacell_df, aligned_df=mc_mov.original_df,
                                                 ref_df=mc_ref.original_df, strategy=strategy, aligned_original_idx_col="Cell_Num_Old",
                                                 ref_original_idx_col="Cell_Num_Old")
    cells = individual_matches.copy()
    ct_aligned = mc_mov.original_df.set_index("Cell_Num_Old")["cell_type"]
    ct_ref = mc_ref.original_df.set_index("Cell_Num_Old")["cell_type"]
    individual_matches["aligned_ct"] = individual_matches["Aligned_cell_id"].map(ct_aligned)
    individual_matches["ref_ct"] = individual_matches["Ref_cell_id"].map(ct_ref)
    individual_matches["celltype_match"] = individual_matches["aligned_ct"] == individual_matches["ref_ct"]
    return (len(individual_matches), int(individual_matches["celltype_match"].sum()),
            float(individual_matches["celltype_match"].mean() * 100), cells)


def _held_against_the_host(scores, tables, cell_tables, mc_ref, mc_mov, strategy, tag):
    """every record's cell keys == score_unpacked of its table == the notebook cell; every cell table == unpack_metacell_matches"""
    import same_amd

    records = _records(scores)
    flat = [t for per_set in tables for t in per_set]
    flat_cells = [t for per_set in cell_tables for t in per_set]
    assert len(records) == len(flat) == len(flat_cells) and list(scores.columns[-3:]) == list(CELL_KEYS)
    for q, (rec, table, cells) in enumerate(zip(records, flat, flat_cells)):
        want, want_cells = same_amd.score_unpacked(table, mc_ref, mc_mov, strategy)
        _same_record({k: rec[k] for k in CELL_KEYS}, want, (tag, q))
        n, k, accuracy, nb_cells = _notebook_cell(table, mc_ref, mc_mov, strategy)
        _same_record(want, {"cells_matched": n, "cell_type_matches": k, "cell_accuracy": accuracy}, (tag, q, "notebook"))
        pd.testing.assert_frame_equal(cells, nb_cells, check_exact=True, obj=f"{tag} cell table {q}")
        pd.testing.assert_frame_equal(want_cells, nb_cells, check_exact=True, obj=f"{tag} host cell table {q}")
        assert cells.dtypes.tolist() == [np.int64, np.int64] and 0 < k < n and n > rec["matched"], (tag, q, n, k)
    return records


@pytest.mark.parametrize("kind", ["ms3", "5 against 4"])
@pytest.mark.parametrize("strategy", ["distribute", "nearest"])
def test_cell_level_records_and_tables_equal_the_host_statement(monkeypatch, strategy, kind):
    import same_amd
    from same_amd import windows as W
    from same_amd.scores import RECORD_KEYS

    mc_ref, mc_mov, cols = _objects(kind)
    variants = _variants_of(mc_mov.metacell_df, cols)[:2]
    calls, inner = [], W.MergeAccumulator.unpack

    def counted(self, *a, **k):
        calls.append(a[2])
        return inner(self, *a, **k)

    monkeypatch.setattr(W.MergeAccumulator, "unpack", counted)
    kw = dict(type_variants=variants, param_sets=SETS, optim_params=dict(MC_OP), tables=True)
    scores, tables, cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, **kw)
    assert calls == [strategy] * 4                                      # the device call, once per result
    assert len(same_amd.window_plan(mc_ref.metacell_df[["X", "Y"]].to_numpy(), mc_mov.metacell_df[["X", "Y"]].to_numpy(), MC_OP["window_size"],
                                    MC_OP["overlap"], MC_OP["min_cells_per_window"])) > 1
    records = _held_against_the_host(scores, tables, cell_tables, mc_ref, mc_mov, strategy, (kind, strategy))
    assert any(a != b for a, b in zip(records, records[1:]))
    if kind != "ms3":
        sizes = lambda mc: mc.metacell_df["members"].map(len)
        assert sizes(mc_mov).max() == 5 > sizes(mc_ref).max() == 3       # (a collapse joins three: 1, 3, 5 ... -- 4 admits no more than 3)
        lengths = [(len(mc_mov.metacell_df["members"].iloc[a]), len(mc_ref.metacell_df["members"].iloc[r]))
                   for a, r in zip(tables[0][0]["Aligned_metacell_id"], tables[0][0]["Ref_metacell_id"])]
        assert {(5, 3), (3, 1), (1, 3), (5, 1)} <= set(lengths), sorted(set(lengths))    # tiled, not dividing, plain
    # unpack=None: today's columns and return shape, and the metacell keys do not move
    plain, plain_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), **kw)
    assert list(plain.columns) == ["variant", "set"] + list(RECORD_KEYS) and calls == [strategy] * 4
    pd.testing.assert_frame_equal(scores[plain.columns], plain, check_exact=True)
    for per_set, want in zip(tables, plain_tables):
        for t, w in zip(per_set, want):
            pd.testing.assert_frame_equal(t, w, check_exact=True)


def test_without_tables_nothing_but_the_score_and_the_unpack_call_follow_a_merge(monkeypatch):
    """per result the unpack call asks the runtime for what include/same_hip.h states -- two launches, two copies, two waits, one fill
    when the accumulator's buffer is laid and none after; called again it answers the same; no column is gathered, no row fetched and no
    frame built in the whole run"""
    import same_amd
    from same_amd import incumbent
    from same_amd import windows as W

    mc_ref, mc_mov, cols = _objects("5 against 4")
    kw = dict(param_sets=SETS + [{"knn": 4}], optim_params=dict(MC_OP), workers=1)
    want = {s: _records(same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=s, tables=True, **kw)[0]) for s in ("nearest", "distribute")}
    seen, inner = [], W.MergeAccumulator.unpack

    def twice(self, *a, **k):
        spent = lambda s0, s1: tuple(s1[q] - s0[q] for q in ("launches", "fills", "copies", "waits"))
        s0 = self.ctx.stats()
        first = inner(self, *a, **k)
        s1 = self.ctx.stats()
        second = inner(self, *a, **k)
        seen.append((spent(s0, s1), spent(s1, self.ctx.stats()), first.tolist(), second.tolist()))
        return second

    refuse = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a table was built"))
    monkeypatch.setattr(W.MergeAccumulator, "unpack", twice)
    monkeypatch.setattr(W.MergeAccumulator, "columns", refuse)
    monkeypatch.setattr(W.MergeAccumulator, "final_rows", refuse)
    monkeypatch.setattr(incumbent._TableBuilder, "gather", refuse)
    monkeypatch.setattr(incumbent._TableBuilder, "table_from_device", refuse)
    with same_amd.resident_frames(mc_ref, mc_mov) as frames:
        runs = [(s, same_amd.sliding_window_scores(frames, mc_mov, list(cols), unpack=s, **kw)) for s in ("nearest", "distribute", "nearest")]
    assert len(seen) == 9
    for s, run in runs:
        assert isinstance(run, pd.DataFrame)
        for g, w in zip(_records(run), want[s]):
            _same_record(g, w, ("tables=False", s))
    for first, second, a, b in seen:
        assert second == (2, 0, 2, 2) and first in ((2, 1, 2, 2), (2, 0, 2, 2)) and a == b, (first, second, a, b)
    # the first job's accumulator is the frames' own: laid in the first run, found clean in the later ones
    assert seen[0][0] == (2, 1, 2, 2) and seen[3][0] == (2, 0, 2, 2) and seen[6][0] == (2, 0, 2, 2)


def _changed(mc, members=None, ids=None):
    out = copy.copy(mc)
    out.metacell_df = mc.metacell_df.copy()
    if members is not None:
        out.metacell_df["members"] = members
    if ids is not None:
        out.metacell_df[mc.metacell_idx_col] = ids
    return out


@pytest.mark.parametrize("why", ["no hip_caller_delaunay key", "permuted metacell ids", "a list of 65 members", "a member id the cells lack"])
def test_what_the_device_does_not_unpack_comes_back_the_same_through_the_tables(monkeypatch, why):
    import same_amd
    from same_amd import windows as W

    monkeypatch.setattr(W.MergeAccumulator, "unpack", lambda *a, **k: (_ for _ in ()).throw(AssertionError("unpacked on the device")))
    mc_ref, mc_mov, cols = _objects("ms3")
    op, strategy = dict(MC_OP), "nearest"
    if why == "no hip_caller_delaunay key":
        del op["hip_caller_delaunay"]
    elif why == "permuted metacell ids":
        ids = mc_ref.metacell_df[mc_ref.metacell_idx_col].to_numpy().copy()
        ids[[3, 11]] = ids[[11, 3]]
        mc_ref = _changed(mc_ref, ids=ids)
    elif why == "a list of 65 members":
        members = [list(m) for m in mc_ref.metacell_df["members"]]
        members[5] = mc_ref.original_df["Cell_Num_Old"].to_numpy()[:65].tolist()
        mc_ref = _changed(mc_ref, members=members)
    else:
        members = [list(m) for m in mc_mov.metacell_df["members"]]
        members[4] = members[4] + [10**7]
        mc_mov, strategy = _changed(mc_mov, members=members), "distribute"       # ('nearest' reads the cell's XY: the reference's KeyError)
    scores, tables, cell_tables = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, param_sets=SETS, optim_params=op,
                                                                 tables=True)
    _held_against_the_host(scores, tables, cell_tables, mc_ref, mc_mov, strategy, why)
    without = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack=strategy, param_sets=SETS, optim_params=op)
    pd.testing.assert_frame_equal(without, scores, check_exact=True)


def test_non_finite_member_coordinates_under_nearest():
    """the reference's own error (scipy: "cost matrix is infeasible") from the device's flag; 'distribute' does not read them"""
    import same_amd

    mc_ref, mc_mov, cols = _objects("ms3")
    bad = copy.copy(mc_mov)
    bad.original_df = mc_mov.original_df.copy()
    bad.original_df["X"] = np.nan
    kw = dict(param_sets=SETS[:1], optim_params=dict(MC_OP))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        same_amd.sliding_window_scores(mc_ref, bad, list(cols), unpack="nearest", **kw)
    got = same_amd.sliding_window_scores(mc_ref, bad, list(cols), unpack="distribute", **kw)
    want = same_amd.sliding_window_scores(mc_ref, mc_mov, list(cols), unpack="distribute", **kw)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
