"""same_merge_acc_score (csrc/window_score.hip) driven at the library against tests/score_check.py's `host_counts` -- plain numpy float64
from the reference's text, nothing of libsame_hip in it -- on sections the tests make themselves: the call only asks that the sections
are on the accumulator's device, carry label codes and that the triangulation was made for the moving one, so one merged accumulator
serves any XY, any codes and any row triples.  Every assertion is exact equality of the eight int64 counts.

The families (score_check.py; tests/test_score_check_cpu.py checks each has its property): areas exactly zero, NaN, infinite, signed zeros,
slivers whose sign the operation order decides, negative and extreme label codes, 3000 triangles around one row at n_flip / n_tri of
exactly 1/2 and 1/3, triangle counts at the wave and block edges, a moving section 5000 rows larger than the one scored before."""
import contextlib
import types

import numpy as np
import pytest

import score_check as S
from test_gpu_scores import OP, _frames, _plain_tris, _records, _same_record

pytestmark = pytest.mark.gpu

RULES = [(False, 0.5, 1)] + [(True, thr, m) for thr in S.THRESHOLDS for m in S.MIN_FLIPS]
ONE_WINDOW = dict(radius=60, knn=4, window_size=5000, overlap=100, min_cells_per_window=20)


def _joint_codes(mov_labels, ref_labels):
    _u, inverse = np.unique(np.concatenate((np.asarray(mov_labels, str), np.asarray(ref_labels, str))), return_inverse=True)
    return inverse[:len(mov_labels)].astype(np.int32), inverse[len(mov_labels):].astype(np.int32)


@contextlib.contextmanager
def _merged(ref, mov, cols, op):
    """a merged accumulator over the frames, without a table (test_the_score_call_refuses_what_it_cannot_count's recipe) -> its handle,
    its context and score_check's Job: the final rows fetched, the job's XY and joint label codes"""
    from same_amd.incumbent import _begin_accumulators, _merge_on_device
    from same_amd.window_api import _WindowJob

    job = _WindowJob(ref, mov, list(cols), None, None, None, dict(op), None, False, None)
    frames, own = job.device_frames("device")
    try:
        accs = _begin_accumulators(job, frames, frames.worker_contexts(1), [0, len(job.todo)], None)
        pos_of = {id(w): pos for pos, w in job.todo}
        collector = lambda states, windows, *_s: accs[0].collect(states, [w["trim"] for w in windows], [w["window_id"] for w in windows],
                                                                 [pos_of[id(w)] for w in windows])
        for dw in frames.windows([w for _p, w in job.todo], collector=collector):
            assert dw.error is None
        done = _merge_on_device(job, frames, accs, None)
        final = done.final_rows()
        code_m, code_r = _joint_codes(mov["cell_type"].to_numpy(), ref["cell_type"].to_numpy())
        yield types.SimpleNamespace(acc=done, ctx=done.ctx, n_windows=len(job.todo), n_final=done.n_final,
                                    job=S.Job(final["a_row"].copy(), final["r_row"].copy(), frames.mov_sec.xy.copy(), frames.ref_sec.xy.copy(),
                                              code_m, code_r))
    finally:
        if own:
            frames.close()


def _synthetic(n, seed):
    from same_amd import synth

    cells = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(cells), _relabelled(synth.to_frame(synth.make_jittered(cells, seed=seed + 1))), synth.type_columns(6)


def _relabelled(frame):
    """one label in nine changed, or every cell would sit on a cell of its own label"""
    labels = frame["cell_type"].to_numpy().copy()
    labels[::9] = np.roll(labels, 1)[::9]
    return frame.assign(cell_type=labels)


@pytest.fixture(scope="module")
def large():
    ref, mov, cols = _frames(1500, 3)
    with _merged(ref, mov, cols, OP) as m:
        print("large:", len(mov), "cells,", m.n_windows, "windows, n_final", m.n_final)
        assert m.n_windows > 1 and m.n_final > 512 and m.n_final % 64 != 0
        yield m


@pytest.fixture(scope="module")
def tiny():
    ref, mov, cols = _synthetic(70, 5)
    mov = mov.copy()
    mov.loc[mov.index[::7], "Y"] += 1500.0             # ten cells with no reference cell within the radius: at most sixty rows
    with _merged(ref, mov, cols, ONE_WINDOW) as m:
        print("tiny:", len(m.job.mov_xy), "moving cells,", m.n_windows, "window, n_final", m.n_final)
        assert m.n_windows == 1 and 0 < m.n_final < 64
        yield m


@pytest.fixture(scope="module")
def middle():
    with _merged(*_synthetic(200, 7), ONE_WINDOW) as m:
        print("middle:", len(m.job.mov_xy), "moving cells,", m.n_windows, "window(s), n_final", m.n_final)
        assert 64 < m.n_final < 256 and m.n_final % 64 != 0
        yield m


@contextlib.contextmanager
def _resident(m, inp):
    """the inputs as sections of their own on the accumulator's context (unbinned beyond the grid a section gives itself), their label
    codes set, the triangles as a DeviceCallerTris of the moving one (None: none)"""
    from same_amd import windows as W

    made = []
    try:
        for xy, code in ((inp.mov_xy, inp.code_m), (inp.ref_xy, inp.code_r)):
            made.append(W.DeviceSection(W.Section(xy, np.zeros((len(xy), 1))), np.float64, m.ctx))
            made[-1].set_label_codes(np.ascontiguousarray(code, np.int32))
        if inp.tris is not None:
            made.append(W.DeviceCallerTris(made[0], inp.tris, m.ctx))
        yield made[0], made[1], (made[2] if inp.tris is not None else None)
    finally:
        for h in reversed(made):                  # a triangulation before its section
            h.close()


def _spent(ctx, s0):
    s1 = ctx.stats()
    return tuple(s1[k] - s0[k] for k in ("launches", "fills", "copies", "waits"))


def _want(m, inp, ignore_same, rule):
    return S.host_counts(m.job.a_row, m.job.r_row, inp.mov_xy, inp.ref_xy, inp.code_m, inp.code_r, inp.tris, ignore_same, *rule)[0]


def _check(m, name, inp, rules=RULES):
    """the call on `inp` under every rule, with and without the same-type rule -> {(ignore_same, rule): counts}"""
    seen = {}
    with _resident(m, inp) as (dmov, dref, tris):
        for ignore_same in (True, False):
            for rule in (rules if ignore_same else rules[:3]):
                got = m.acc.score(dmov, dref, tris, ignore_same, *rule)
                want = _want(m, inp, ignore_same, rule)
                assert got.dtype == np.int64 and got.tolist() == want.tolist(), (name, ignore_same, rule, got.tolist(), want.tolist())
                seen[ignore_same, rule] = got
    return seen


# ---- 1. the families ---------------------------------------------------------------------------------------------------------------------
N_LARGE = 6 + 1 + 4 + (len(S.TRI_COUNTS) + 1) + 1


@pytest.mark.parametrize("which", range(N_LARGE))
def test_every_family_on_the_large_accumulator(large, which):
    if not hasattr(large, "families"):
        large.families = S.all_families(large.job)
    families = large.families
    assert len(families) == N_LARGE
    name, inp = families[which]
    seen = _check(large, name, inp)
    print(name, seen[True, RULES[0]].tolist())
    if name == "hub":       # the first hub row is violating at its own ratio and not a float above it
        half = float(np.nextafter(0.5, 1.0))
        assert seen[True, (True, 0.5, 1)][7] == seen[True, (True, half, 1)][7] + 1
        assert seen[True, (True, 1.0 / 3.0, 1)][7] == seen[True, (True, 0.5, 1)][7] + 1


@pytest.mark.parametrize("which", ["tiny", "middle"])
def test_the_small_accumulators(request, which):
    m = request.getfixturevalue(which)
    for name, inp in S.small_families(m.job):
        seen = _check(m, name, inp)
        print(which, name, seen[True, RULES[0]].tolist())


@pytest.mark.parametrize("n", [256, 257])
def test_final_rows_of_exactly_a_block_and_one_more(n):
    """identical frames, one window, one neighbour: every cell keeps itself, so n_final is n"""
    ref, _mov, cols = _synthetic(n, 9)
    with _merged(ref, _relabelled(ref), cols, dict(ONE_WINDOW, knn=1)) as m:
        print("identical frames of", n, "cells: n_final", m.n_final)
        assert m.n_final == n
        for name, inp in S.small_families(m.job):
            _check(m, name, inp, RULES[:4])


# ---- 2. the work buffer's life -----------------------------------------------------------------------------------------------------------
def test_the_work_buffer_through_a_larger_section_and_back():
    """a fresh accumulator: own with triangles, no triangulation, an empty one, own, grown (laid again for 5000 more rows, which read as
    unmatched), own, mirrored, own -- every step equal to the host statement, every call asking the runtime for what include/same_hip.h
    states: (launches, fills, copies, waits) = (3, 0, 1, 1) with triangles and (1, 0, 1, 1) without, two fills on the calls that lay the
    buffer (the first and grown)"""
    ref, mov, cols = _frames(1500, 3)
    with _merged(ref, mov, cols, OP) as m:
        job = m.job
        base, big, mirror = S.own(job), S.grown(job), S.mirrored(job)
        steps = [("own", base, 2), ("no triangulation", base._replace(tris=None), 0), ("empty", base._replace(tris=np.zeros((0, 3), np.int32)), 0),
                 ("own again", base, 0), ("grown", big, 2), ("own after grown", base, 0), ("mirrored", mirror, 0), ("own at last", base, 0)]
        with contextlib.ExitStack() as stack:
            resident = {id(inp): stack.enter_context(_resident(m, inp)) for _n, inp, _f in steps[:3] + [steps[4], steps[6]]}
            log = []
            for name, inp, fills in steps:
                dmov, dref, tris = resident[id(inp)]
                for rule in (RULES[0], (True, 0.5, 1)):
                    s0 = m.ctx.stats()
                    got = m.acc.score(dmov, dref, tris, True, *rule)
                    spent = _spent(m.ctx, s0)
                    log.append((name, spent, got.tolist()))
                    want = _want(m, inp, True, rule)
                    assert got.tolist() == want.tolist(), (name, rule, got.tolist(), want.tolist())
                    with_tris = inp.tris is not None and len(inp.tris) > 0
                    laid = fills if rule == RULES[0] else 0
                    assert spent == ((3 if with_tris else 1), laid, 1, 1), (name, rule, spent)
            for entry in log:
                print(entry)
        grown_counts = next(c for n, _s, c in log if n == "grown")
        assert grown_counts[2] == len(big.tris) > grown_counts[3] == log[0][2][3]      # the new rows' triangles: resident, never all matched


def test_a_refused_call_leaves_the_accumulator_as_it_was(large):
    """sections of half the rows: final rows name rows outside them, SAME_ERANGE, out_counts untouched -- and the next call counts as ever"""
    from same_amd import _lib

    job = large.job
    base = S.own(job)
    half_m, half_r = len(base.mov_xy) // 2, len(base.ref_xy) // 2
    assert job.a_row.max() >= half_m and job.r_row.max() >= half_r
    small_tris = base.tris[(base.tris < half_m).all(axis=1)]
    short_mov = S.Inputs(base.mov_xy[:half_m], base.ref_xy, base.code_m[:half_m], base.code_r, small_tris)
    short_ref = base._replace(ref_xy=base.ref_xy[:half_r], code_r=base.code_r[:half_r])
    want = _want(large, base, True, RULES[0])
    counts = np.full(8, -7, np.int64)
    with _resident(large, base) as (dmov, dref, tris):
        assert large.acc.score(dmov, dref, tris).tolist() == want.tolist()
        for name, inp in (("half the moving rows", short_mov), ("half the reference rows", short_ref),
                          ("half the moving rows, no triangles", short_mov._replace(tris=None))):
            with _resident(large, inp) as (dm, dr, tr):
                with large.ctx.lock:
                    rc = large.ctx.lib.same_merge_acc_score(large.acc.handle, dm.handle, dr.handle, None if tr is None else tr.handle, 1, 0, 0.5, 1,
                                                            counts.ctypes.data)
            assert rc == _lib.SAME_ERANGE and counts.tolist() == [-7] * 8, (name, rc, counts.tolist())
            for rule in (RULES[0], (True, 0.5, 1)):
                got = large.acc.score(dmov, dref, tris, True, *rule)
                assert got.tolist() == _want(large, base, True, rule).tolist(), (name, rule, got.tolist())


# ---- 3. tied to the product ----------------------------------------------------------------------------------------------------------------
def test_the_products_record_equals_the_host_statement_of_its_table():
    """sliding_window_scores' record against record_from_counts(host_counts(...)) from the table with numpy alone: a yardstick beside
    score_table that no kernel has a part in.  The set allows two matches per reference cell, but at 4000 cells the merged table names no
    reference cell twice (measured: none), so no triangle's mapped corners repeat one: an after-area of exactly 0 is the families' case
    (line, degenerate), not this test's; where one does occur it is checked."""
    import same_amd
    from same_amd.scores import record_from_counts

    ref, mov, cols = _frames()
    sets = [{"hip_incumbent": "transport", "hip_refine": "capacity", "max_matches": 2, "penalty_coeff": 0.5}]
    scores, tables = same_amd.sliding_window_scores(ref, mov, list(cols), param_sets=sets, optim_params=dict(OP), score_delaunay=_plain_tris(),
                                                    tables=True)
    table = tables[0][0]
    cid = "Cell_Num_Old"
    rows_of = lambda frame, ids: np.argsort(frame[cid].to_numpy(), kind="stable")[np.searchsorted(np.sort(frame[cid].to_numpy()), ids)]
    a_row, r_row = rows_of(mov, table[f"Aligned_{cid}"].to_numpy()), rows_of(ref, table[f"Ref_{cid}"].to_numpy())
    assert np.array_equal(mov[cid].to_numpy()[a_row], table[f"Aligned_{cid}"].to_numpy())
    ref_xy = ref[["X", "Y"]].to_numpy(dtype=np.float64)
    assert np.array_equal(ref_xy[r_row], table[["ref_X", "ref_Y"]].to_numpy())
    code_m, code_r = _joint_codes(mov["cell_type"].to_numpy(), ref["cell_type"].to_numpy())
    mov_xy, tris = mov[["X", "Y"]].to_numpy(dtype=np.float64), _plain_tris()
    counts, _nt, _nf = S.host_counts(a_row, r_row, mov_xy, ref_xy, code_m, code_r, tris)
    want = record_from_counts({"matched": counts[0], "type_matches": counts[1], "total_triangles": counts[2],
                               "triangles_with_all_matched": counts[3], "triangles_same_type_skipped": counts[4],
                               "triangles_flipped": counts[6], "nodes_in_violating_triangles": counts[7]})
    _same_record(_records(scores)[0], want, "product")
    matched, _s, flipped, _b, after = S.host_triangles(a_row, r_row, mov_xy, ref_xy, code_m, tris, True)
    match_of = np.full(len(mov), -1, np.int64)
    match_of[a_row] = r_row
    corners = np.sort(match_of[tris[matched]], axis=1)
    repeated = (corners[:, 0] == corners[:, 1]) | (corners[:, 1] == corners[:, 2])
    print("product:", counts.tolist(), "reference cells matched twice:", len(r_row) - len(np.unique(r_row)),
          "triangles whose mapped corners repeat a reference cell:", int(repeated.sum()))
    assert (after[matched][repeated] == 0).all() and not flipped[matched][repeated].any()
    assert counts[6] > 0 and counts[4] > 0 and 0 < counts[1] < counts[0] and counts[3] < counts[2]
