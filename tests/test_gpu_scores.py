"""same_amd.sliding_window_scores as a product and same_merge_acc_score (csrc/window_score.hip) at the library.
Every record the device counts from a result's merged rows equals `score_table` of that result's table -- the host statement, made of
check_triangle_violations and a comparison of labels -- key for key, integers exact and floats bit for bit; the tables are
sliding_window_variants'; the names are tied to the reference's (check_alignment at kNN=1, check_triangle_violations as its notebook calls
it); and with tables=False no table is built.  Every test here fails without the feature: same_amd has no sliding_window_scores."""
import functools
import struct

import numpy as np
import pandas as pd
import pytest

from test_gpu_window_variants import OP, _variants_of
from test_gpu_window_variants import _frames as _variants_frames

pytestmark = pytest.mark.gpu

SETS = [{}, {"knn": 3, "hip_incumbent": "assignment"}, {"delaunay_penalty": 50, "hip_refine": "local"}]
MC_OP = dict(radius=30, knn=6, window_size=200, overlap=50, min_cells_per_window=20, hip_caller_delaunay="device")
CID = "Cell_Num_Old"


@functools.lru_cache(maxsize=None)
def _frames(n=4000, seed=0):
    """the variants tests' frames, one label in twelve of the moving frame's `cell_type` changed (a copy: theirs stay as they are) -- or the
    frame's own types, which ARE its labels, would put every cell on a cell of its label"""
    ref, mov, cols = _variants_frames(n, seed)
    mov = mov.copy()
    rng = np.random.default_rng(seed + 17)
    rows = rng.choice(len(mov), len(mov) // 12, replace=False)
    labels = mov["cell_type"].to_numpy().copy()
    labels[rows] = np.asarray(cols)[(np.searchsorted(np.asarray(cols), labels[rows]) + 1 + rng.integers(0, len(cols) - 1, len(rows))) % len(cols)]
    mov["cell_type"] = labels
    return ref, mov, cols


def _bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _same_record(got, want, tag):
    """key for key, in order; integers exact, floats bit for bit (NaN included)"""
    assert list(got) == list(want), (tag, list(got), list(want))
    for k in want:
        assert type(got[k]) is type(want[k]) and _bits(got[k]) == _bits(want[k]), (tag, k, got[k], want[k])


def _records(scores):
    """the score frame's rows as records without `variant` / `set`, Python numbers"""
    assert all(scores[k].dtype.kind in "fi" for k in scores.columns)
    return [{k: float(scores[k].iloc[i]) if scores[k].dtype.kind == "f" else int(scores[k].iloc[i]) for k in scores.columns[2:]}
            for i in range(len(scores))]


def _simplices(frame):
    from scipy.spatial import Delaunay

    return Delaunay(frame[["X", "Y"]].to_numpy()).simplices.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _plain_tris():
    return _simplices(_frames()[1])


def _scored(ref, mov, cols, op, tag, *, cid=CID, variants=None, sets=None, score_delaunay=None, vertex_col=None, score_params=None,
            host_delaunay="same", **kw):
    """sliding_window_scores(tables=True) -> (the device's records, the host's records of the same tables, the tables); every record is
    asserted to equal score_table of its own table, the frame to be laid out as stated"""
    import same_amd

    scores, tables = same_amd.sliding_window_scores(ref, mov, list(cols), type_variants=variants, param_sets=sets, optim_params=dict(op),
                                                    score_delaunay=score_delaunay, score_delaunay_vertex_col=vertex_col,
                                                    score_params=score_params, tables=True, **kw)
    n_v, n_s = len(variants or [None]), len(sets or [{}])
    assert len(tables) == n_v and all(len(t) == n_s for t in tables) and len(scores) == n_v * n_s
    assert scores["variant"].tolist() == [v for v in range(n_v) for _ in range(n_s)] and scores["set"].tolist() == list(range(n_s)) * n_v
    host_tri = score_delaunay if isinstance(host_delaunay, str) else host_delaunay
    host = [same_amd.score_table(t, ref, mov, cell_id_col=cid, score_delaunay=host_tri, score_delaunay_vertex_col=vertex_col,
                                 score_params=score_params) for per_set in tables for t in per_set]
    got = _records(scores)
    for q, (g, h) in enumerate(zip(got, host)):
        _same_record(g, h, (tag, q))
    return got, host, tables


def _not_vacuous(host, tag):
    for q, h in enumerate(host):
        assert 0 < h["type_matches"] < h["matched"], (tag, q, h)
        assert h["triangles_flipped"] > 0 and h["triangles_same_type_skipped"] > 0 and h["nodes_in_violating_triangles"] > 0, (tag, q, h)
        assert 0 < h["triangles_with_all_matched"] <= h["total_triangles"], (tag, q, h)
    assert any(a != b for a, b in zip(host, host[1:])), tag                       # at least two records of the run differ


@pytest.fixture
def rest_rows(monkeypatch):
    """the rest rows (contested: left to the host's matching) of every merge of the test"""
    from same_amd import windows as W

    seen, inner = [], W.resolve_accumulators

    def resolve(accs, dmov, dref):
        counts, rest = inner(accs, dmov, dref)
        seen.append(len(rest))
        return counts, rest

    monkeypatch.setattr(W, "resolve_accumulators", resolve)
    return seen


# ---- 1. records equal the host statement, three ways -------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one worker", "two workers, a partial last batch"])
def test_records_of_plain_frames_equal_the_host_statement_and_the_tables_are_the_variants(rest_rows, how):
    import same_amd

    ref, mov, cols = _frames()
    variants = _variants_of(mov, cols)
    kw = {}
    if how != "one worker":
        n_windows = len(same_amd.window_plan(ref[["X", "Y"]].to_numpy(), mov[["X", "Y"]].to_numpy(), OP["window_size"], OP["overlap"],
                                             OP["min_cells_per_window"]))
        kw = dict(workers=2, batch=next(b for b in (4, 3, 5) if n_windows % b))
    got, host, tables = _scored(ref, mov, cols, OP, how, variants=variants, sets=SETS, score_delaunay=_plain_tris(), **kw)
    assert len(got) == 9 and any(n > 0 for n in rest_rows)                        # the merge left contested rows for the host
    _not_vacuous(host, how)
    assert len(_plain_tris()) % 256 and len(_plain_tris()) % 64 and all(h["matched"] % 64 and h["matched"] % 256 for h in host[:1])
    want = same_amd.sliding_window_variants(ref, mov, variants, list(cols), param_sets=SETS, optim_params=dict(OP), merge=True, **kw)
    for v in range(3):
        for s in range(3):
            pd.testing.assert_frame_equal(tables[v][s], want[v][s], check_exact=True, obj=f"{how} variant {v} set {s}")
    # without the lists: one variant, one set, nested alike
    one, _h, t1 = _scored(ref, mov, cols, OP, how + " alone", score_delaunay=_plain_tris(), **kw)
    _same_record(one[0], got[0], "alone")
    pd.testing.assert_frame_equal(t1[0][0], tables[0][0], check_exact=True)


def test_records_of_metacell_objects_equal_the_host_statement(rest_rows):
    """the job's own caller triangulation, resident once: no score_delaunay"""
    import same_amd
    from test_gpu_caller_triangulation import _metacells

    ref, mc, cols = _metacells("ms3")
    cid = mc.metacell_idx_col
    variants = _variants_of(mc.metacell_df, cols)
    got, host, tables = _scored(ref, mc, cols, MC_OP, "metacells", cid=cid, variants=variants, sets=SETS,
                                host_delaunay=mc.metacell_delaunay)
    _not_vacuous(host, "metacells")
    assert host[0]["total_triangles"] == len(mc.metacell_delaunay)
    want = same_amd.sliding_window_variants(ref, mc, variants, list(cols), param_sets=SETS, optim_params=dict(MC_OP), merge=True)
    for v in range(3):
        for s in range(3):
            pd.testing.assert_frame_equal(tables[v][s], want[v][s], check_exact=True, obj=f"metacells variant {v} set {s}")
    # tied to the reference's names: the triangle keys are check_triangle_violations' stats, called as reproduce_figures.ipynb cell 21 calls it
    for q, table in enumerate(t for per_set in tables for t in per_set):
        matches = table.copy()
        matches["cell_type"] = mc.metacell_df.loc[matches[f"Aligned_{cid}"], "cell_type"].values
        matches.index = matches[f"Aligned_{cid}"].values
        _df, stats = same_amd.check_triangle_violations(matches, mc, aligned_id_col=f"Aligned_{cid}", ref_id_col=f"Ref_{cid}",
                                                        mapped_x_col="ref_X", mapped_y_col="ref_Y", cell_type_col="cell_type",
                                                        ignore_same_type_triangles=True, verbose=False)
        for k in ("total_triangles", "triangles_with_all_matched", "triangles_same_type_skipped", "triangles_flipped", "percent_flipped",
                  "nodes_in_violating_triangles", "percent_nodes_violating"):
            assert _bits(got[q][k]) == _bits(type(got[q][k])(stats[k])), (q, k, got[q][k], stats[k])
        assert _bits(got[q]["violations"]) == _bits(100 * stats["triangles_flipped"] / stats["total_triangles"])


def test_accuracy_is_check_alignment_at_one_neighbour_on_the_matched_coordinates():
    import same_amd

    ref, mov, cols = _frames()
    rxy = ref[["X", "Y"]].to_numpy()
    assert len(np.unique(rxy, axis=0)) == len(rxy)                                # pairwise distinct: a cell's nearest template cell is itself
    got, _host, tables = _scored(ref, mov, cols, OP, "accuracy", sets=SETS[:2])
    assert list(got[0]) == ["matched", "type_matches", "accuracy"]                # no triangulation to score against
    template = ref.assign(SAME_X=ref["X"], SAME_Y=ref["Y"])
    for q, table in enumerate(tables[0]):
        rows = pd.Index(mov[CID]).get_indexer(table[f"Aligned_{CID}"])
        query = table.assign(SAME_X=table["ref_X"], SAME_Y=table["ref_Y"], cell_type=mov["cell_type"].to_numpy()[rows])
        checked, _mean = same_amd.check_alignment(query, template, xcol="SAME_X", ycol="SAME_Y", ctype_col="cell_type", kNN=1)
        assert _bits(got[q]["accuracy"]) == _bits(float(100 * checked["_1NN_match"].mean())), (q, got[q])
        assert got[q]["type_matches"] == int(checked["_1NN_match"].sum()) and got[q]["matched"] == len(table)


# ---- 2. score_params ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_params", [dict(node_local=True, majority_threshold=0.5), dict(node_local=True, majority_threshold=1.0),
                                          dict(node_local=True, majority_threshold=0.5, min_flips=2), dict(ignore_same_type_triangles=False)],
                         ids=["majority 0.5", "majority 1.0", "two flips", "same type counted"])
def test_score_params_reach_the_kernels(score_params):
    ref, mov, cols = _frames()
    kw = dict(variants=_variants_of(mov, cols)[:2], sets=SETS[:2], score_delaunay=_plain_tris())
    base, _h, _t = _scored(ref, mov, cols, OP, "defaults", **kw)
    got, host, _t = _scored(ref, mov, cols, OP, str(score_params), score_params=score_params, **kw)
    print(score_params, [(h["nodes_in_violating_triangles"], b["nodes_in_violating_triangles"]) for h, b in zip(host, base)])
    assert any(h["nodes_in_violating_triangles"] > 0 for h in host)
    for h, b in zip(host, base):
        assert h["triangles_flipped"] > 0
        if "node_local" in score_params:       # the majority rule is the stricter one
            assert h["nodes_in_violating_triangles"] < b["nodes_in_violating_triangles"] and h["triangles_flipped"] == b["triangles_flipped"]
        else:
            assert h["triangles_same_type_skipped"] == 0 < b["triangles_same_type_skipped"] and h["triangles_flipped"] >= b["triangles_flipped"]


# ---- 3. shapes at which the kernels can go wrong -----------------------------------------------------------------------------------------
def test_one_window_of_fewer_rows_than_a_wave():
    from same_amd import synth

    cells = synth.make_cells(70, 6, seed=5)
    ref, mov = synth.to_frame(cells), synth.to_frame(synth.make_jittered(cells, seed=6))
    op = dict(radius=60, knn=4, window_size=5000, overlap=100, min_cells_per_window=20)
    tris = _simplices(mov)
    got, host, tables = _scored(ref, mov, synth.type_columns(6), op, "70 cells", score_delaunay=tris)
    assert 0 < host[0]["matched"] <= 70 and host[0]["total_triangles"] == len(tris) < 256 and host[0]["triangles_with_all_matched"] > 0
    assert tables[0][0]["window_id"].nunique() == 1


def test_a_triangulation_without_triangles_and_one_that_names_ids_the_frame_lacks():
    ref, mov, cols = _frames()
    none, host, _t = _scored(ref, mov, cols, OP, "no triangles", score_delaunay=np.zeros((0, 3), np.int64))
    assert host[0]["total_triangles"] == 0 and np.isnan(host[0]["violations"]) and host[0]["percent_flipped"] == 0.0
    assert host[0]["nodes_in_violating_triangles"] == 0 and host[0]["type_matches"] > 0
    n = len(mov)
    lost = np.array([[0, 1, n + 5], [n + 7, n + 8, n + 9], [-1, 2, 3]], np.int64)
    base, _h, _t = _scored(ref, mov, cols, OP, "whole", score_delaunay=_plain_tris())
    got, host, _t = _scored(ref, mov, cols, OP, "lost ids", score_delaunay=np.vstack((lost[:1], _plain_tris(), lost[1:])))
    assert host[0]["total_triangles"] == base[0]["total_triangles"] + 3           # total_triangles counts them and nothing else does
    for k in host[0]:
        if k not in ("total_triangles", "violations"):
            assert _bits(host[0][k]) == _bits(base[0][k]), k
    assert host[0]["violations"] < base[0]["violations"]


def test_a_clump_of_moving_cells_far_from_every_reference_cell():
    """the reference cells around a spot are taken out: the moving cells there stay unmatched, and their triangles are not all matched"""
    ref, mov, cols = _frames()
    centre = mov[["X", "Y"]].to_numpy()[len(mov) // 2]
    far = np.hypot(*(ref[["X", "Y"]].to_numpy() - centre).T) > 3 * OP["radius"]
    clump = np.hypot(*(mov[["X", "Y"]].to_numpy() - centre).T) < OP["radius"]
    assert clump.sum() >= 5 and far.sum() > len(ref) - 400
    sparse = ref[far].reset_index(drop=True)
    got, host, tables = _scored(sparse, mov, cols, OP, "clump", sets=SETS[:2], score_delaunay=_plain_tris())
    _not_vacuous(host, "clump")
    for h, table in zip(host, tables[0]):
        assert h["triangles_with_all_matched"] < h["total_triangles"] - clump.sum()
        assert not set(table[f"Aligned_{CID}"]) & set(mov[CID].to_numpy()[clump])


def test_ids_read_through_a_vertex_column():
    """vertex ids that are neither row numbers nor the cell ids"""
    from test_gpu_caller_triangulation import _plain

    ref, mov, tris, cols = _plain()
    vid = mov["vid"].to_numpy()
    got, host, _t = _scored(ref, mov, cols, dict(OP, knn=4), "vid", score_delaunay=vid[tris], vertex_col="vid")
    assert host[0]["total_triangles"] == len(tris) and host[0]["triangles_flipped"] > 0


# ---- 4. tables=False builds no table ------------------------------------------------------------------------------------------------------
def test_without_tables_nothing_but_the_score_call_follows_a_merge(monkeypatch):
    """Per set the score call asks the runtime for what include/same_hip.h states -- three launches, one copy, one wait, no fill once the
    accumulator's work buffer is laid (two fills, once) --; called again on the same accumulator it counts the same (its last kernel left
    the buffer as it found it); no column is gathered and no frame built in the whole run."""
    import same_amd
    from same_amd import incumbent
    from same_amd import windows as W

    ref, mov, cols = _frames()
    variants = _variants_of(mov, cols)[:2]
    with_tables, _host, _t = _scored(ref, mov, cols, OP, "with tables", variants=variants, sets=SETS, score_delaunay=_plain_tris(), workers=1)
    seen, inner = [], W.MergeAccumulator.score

    def twice(self, *a):
        spent = lambda s0, s1: tuple(s1[k] - s0[k] for k in ("launches", "fills", "copies", "waits"))
        s0 = self.ctx.stats()
        first = inner(self, *a)
        s1 = self.ctx.stats()
        second = inner(self, *a)
        seen.append((spent(s0, s1), spent(s1, self.ctx.stats()), first.tolist(), second.tolist()))
        return second

    refuse = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a table was built"))
    monkeypatch.setattr(W.MergeAccumulator, "score", twice)
    monkeypatch.setattr(W.MergeAccumulator, "columns", refuse)
    monkeypatch.setattr(W.MergeAccumulator, "final_rows", refuse)
    monkeypatch.setattr(incumbent._TableBuilder, "gather", refuse)
    monkeypatch.setattr(incumbent._TableBuilder, "table_from_device", refuse)
    with same_amd.resident_frames(ref, mov) as frames:
        runs = [same_amd.sliding_window_scores(frames, mov, list(cols), type_variants=variants, param_sets=SETS, optim_params=dict(OP),
                                               score_delaunay=_plain_tris(), workers=1) for _ in range(2)]
    assert isinstance(runs[0], pd.DataFrame) and len(seen) == 12
    for run in runs:
        for g, w in zip(_records(run), with_tables):
            _same_record(g, w, "tables=False")
    for first, second, a, b in seen:
        assert second == (3, 0, 1, 1) and first in ((3, 2, 1, 1), (3, 0, 1, 1)) and a == b, (first, second, a, b)
    # the first job's accumulator is the frames' own: laid in the first run, found clean in the second
    assert seen[0][0] == (3, 2, 1, 1) and seen[6][0] == (3, 0, 1, 1)


# ---- 5. fallbacks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["host prune", "two triangles of one vertex set", "a missing label"])
def test_inputs_the_device_cannot_score_give_the_same_records_through_the_tables(monkeypatch, why):
    from same_amd import windows as W

    monkeypatch.setattr(W.MergeAccumulator, "score", lambda *a, **k: (_ for _ in ()).throw(AssertionError("scored on the device")))
    ref, mov, cols = _frames(1500, 3)
    op, tris = dict(OP), _simplices(mov)
    if why == "host prune":
        op["ignore_knn_if_matched"] = True
    elif why == "two triangles of one vertex set":
        tris = np.vstack((tris, tris[7:8, ::-1]))
    else:
        mov = mov.copy()
        mov["cell_type"] = mov["cell_type"].astype(object)
        mov.loc[[3, 500, 501], "cell_type"] = None
    got, host, _t = _scored(ref, mov, cols, op, why, sets=SETS[:2], score_delaunay=tris)
    assert host[0]["total_triangles"] == len(tris) and host[0]["triangles_flipped"] > 0 and 0 < host[0]["type_matches"] < host[0]["matched"]


# ---- 6. the library's refusals ----------------------------------------------------------------------------------------------------------------
def test_the_score_call_refuses_what_it_cannot_count():
    from same_amd import _lib
    from same_amd import windows as W
    from same_amd.incumbent import _begin_accumulators, _merge_on_device
    from same_amd.window_api import _WindowJob

    ref, mov, cols = _frames(1500, 3)
    job = _WindowJob(ref, mov, list(cols), None, None, None, dict(OP), None, False, None)
    frames, own = job.device_frames("device")
    other = None
    try:
        accs = _begin_accumulators(job, frames, frames.worker_contexts(1), [0, len(job.todo)], None)
        pos_of = {id(w): pos for pos, w in job.todo}
        collector = lambda states, windows, *_s: accs[0].collect(states, [w["trim"] for w in windows], [w["window_id"] for w in windows],
                                                                 [pos_of[id(w)] for w in windows])
        collected = W.MergeAccumulator(accs[0].ctx)                                # an accumulator that has rows and no finish
        collected.begin(len(mov))
        for dw in frames.windows([w for _p, w in job.todo], collector=collector):
            assert dw.error is None
        ctx, counts = accs[0].ctx, np.full(8, -7, np.int64)

        def call(acc, dmov, dref, tris=None):
            with ctx.lock:
                return ctx.lib.same_merge_acc_score(acc.handle, dmov.handle, dref.handle, None if tris is None else tris.handle, 1, 0, 0.5, 1,
                                                    counts.ctypes.data)

        assert call(accs[0], frames.dmov, frames.dref) == _lib.SAME_EINVAL         # before the merge's finish
        done = _merge_on_device(job, frames, accs, None)
        assert done.n_final > 500
        assert call(done, frames.dmov, frames.dref) == _lib.SAME_EINVAL            # before label codes are set
        frames.label_codes_on_device()
        other = W.DeviceCallerTris(frames.dref, _simplices(ref).astype(np.int32))
        assert call(done, frames.dmov, frames.dref, other) == _lib.SAME_EINVAL     # a triangulation of another section
        assert call(collected, frames.dmov, frames.dref) == _lib.SAME_EINVAL
        assert counts.tolist() == [-7] * 8                                          # out_counts untouched
        with pytest.raises(_lib.SameHipError) as e:
            done.score(frames.dmov, frames.dref, other)
        assert e.value.code == _lib.SAME_EINVAL
        mine = frames.caller_tris(_plain_small(), None)
        got = done.score(frames.dmov, frames.dref, mine)
        assert got[0] == done.n_final and got[2] == len(_plain_small()) and 0 < got[6] <= got[5] <= got[3] and got[1] > 0
        assert np.array_equal(done.score(frames.dmov, frames.dref, mine), got)
        collected.close()
    finally:
        if other is not None:
            other.close()
        if own:
            frames.close()


@functools.lru_cache(maxsize=None)
def _plain_small():
    return _simplices(_frames(1500, 3)[1])
