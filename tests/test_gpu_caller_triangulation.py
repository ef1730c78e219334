"""optim_params["hip_caller_delaunay"] = "device": sliding_window_incumbent keeps a caller's triangulation (MetaCell objects,
`moving_delaunay=`) on the device route (csrc/window_caller.hip).  The oracle is the general route on the same inputs, which
tests/test_gpu_run_same.py::test_metacell_flow_equals_reference pins to the reference's own table; where that fixture exists it is the
oracle itself.  Tables: the same rows in the same order, every column bit for bit.  Stats: every integer equal; the float objectives of
the optimal starts and of the search are sums the two routes add up in different orders (one over the device's pair list, one over the
host's compacted copy), so they agree to rel 1e-9 -- the bound the existing tests of these two routes use
(tests/test_gpu_transport.py::test_routes_agree_and_the_objectives_are_ordered) -- and `mip_gap`, a quotient of their difference, to
rel 1e-6 / abs 1e-8 as there."""
import functools

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

KEY = {"hip_caller_delaunay": "device"}
WIN = dict(window_size=200, overlap=50, min_cells_per_window=20)
FLOAT_STATS = ("objective", "mip_objective_start", "mip_objective")


def _run(ref, mov, cols, op, **k):
    import same_amd

    return same_amd.sliding_window_incumbent(ref, mov, commonCT=cols, optim_params=dict(op), return_stats=True, **k)


def _same_tables(got, want, tag=None):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), tag
    for c in want.columns:
        a, b = got[c].to_numpy(), want[c].to_numpy()
        assert a.dtype == b.dtype, (tag, c)
        if a.dtype.kind == "f":
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), (tag, c)


def _same_stats(got, want, tag=None):
    assert len(got) == len(want), tag
    for a, b in zip(got, want):
        assert set(a) == set(b), tag
        for k in a:
            if k == "mip_gap":
                assert a[k] == pytest.approx(b[k], rel=1e-6, abs=1e-8), (tag, k)
            elif k in FLOAT_STATS:
                assert a[k] == pytest.approx(b[k], rel=1e-9, abs=1e-12), (tag, k)
            elif k != "transport_searches":          # (how many searches a start took is the route's own: its pair order)
                assert a[k] == b[k], (tag, k)


def _both(ref, mov, cols, op, tag=None, **k):
    """device route with the key == general route -> (table, stats)"""
    want, wst = _run(ref, mov, cols, op, _route="general", **{q: v for q, v in k.items() if q not in ("batch", "workers")})
    got, gst = _run(ref, mov, cols, dict(op, **KEY), _route="device", **k)
    _same_tables(got, want, tag)
    _same_stats(gst, wst, tag)
    return got, gst


@functools.lru_cache(maxsize=None)
def _metacells(kind):
    """(reference, moving MetaCell, type columns): both sides collapsed at max_metacell_size 3, at 1, or the aligned side only"""
    import same_amd
    from same_amd import synth

    cells = synth.make_cells(2400, 3, seed=71)
    r_c = synth.to_frame(cells)
    a_c = synth.to_frame(synth.make_jittered(cells, seed=72))
    a_c["Cell_Num_Old"] = np.arange(len(a_c)) * 2 + 7
    ms = 1 if kind == "ms1" else 3
    collapse = lambda df: same_amd.greedy_triangle_collapse(df, max_metacell_size=ms, r_max=40, min_angle_deg=10, return_object=True,
                                                            verbose=False)
    mc_a = collapse(a_c)
    if kind == "aligned_only":          # a plain reference frame carries the id column the MetaCell side names (cell_id_col follows it)
        r_c[mc_a.metacell_idx_col] = np.arange(len(r_c)) * 3 + 11
    return (r_c if kind == "aligned_only" else collapse(r_c)), mc_a, tuple(synth.type_columns(3))


@functools.lru_cache(maxsize=None)
def _plain(n=1800, seed=81):
    """(reference frame, moving frame with ids offset by 10^6 and non-contiguous in `vid`, its Delaunay triangulation in row space, cols)"""
    from scipy.spatial import Delaunay
    from same_amd import synth

    cells = synth.make_cells(n, 3, seed=seed)
    r_df = synth.to_frame(cells)
    m_df = synth.to_frame(synth.make_jittered(cells, seed=seed + 1))
    m_df["vid"] = 1_000_000 + np.arange(len(m_df)) * 7 + 3
    return r_df, m_df, Delaunay(m_df[["X", "Y"]].to_numpy()).simplices.astype(np.int64), tuple(synth.type_columns(3))


OP = dict(radius=30, knn=4, **WIN)


def test_without_the_key_the_device_route_still_refuses():
    ref, mc, cols = _metacells("ms3")
    with pytest.raises(ValueError, match="device route does not apply"):
        _run(ref, mc, list(cols), OP, _route="device")
    with pytest.raises(ValueError, match="device route does not apply"):
        _run(ref, mc, list(cols), dict(OP, hip_caller_delaunay="host"), _route="device")


@pytest.mark.parametrize("kind", ["ms3", "ms1", "aligned_only"])
def test_route_equality_on_metacell_objects(kind):
    ref, mc, cols = _metacells(kind)
    cols = list(cols)
    got, st = _both(ref, mc, cols, OP, kind)
    assert 9 <= len(st) <= 20 and len(got) > 300
    for batch in (1, 3, 8, 20):
        for workers in (1, 2):
            _both(ref, mc, cols, OP, (kind, batch, workers), batch=batch, workers=workers)
    _both(ref, mc, cols, OP, (kind, "local indices"), window_local_indices=True)
    _both(ref, mc, cols, dict(OP, ignore_same_type_triangles=False), (kind, "same type off"))
    _both(ref, mc, cols, dict(OP, min_angle_deg=None), (kind, "no angle"), window_local_indices=True)
    # without _route the key alone chooses the device route: the same table
    auto, _st = _run(ref, mc, cols, dict(OP, **KEY))
    _same_tables(auto, got, (kind, "auto"))


def test_fixture_table_through_the_device_route():
    """the `sw_metacell/res_*` record of tests/golden/run_same_mock.npz (the reference's own sliding_window_matching on these MetaCell
    objects), as test_metacell_flow_equals_reference reads it"""
    import same_amd
    from same_amd import synth

    g = load_golden("run_same_mock")
    cells = synth.make_cells(900, 3, seed=61)
    r_c = synth.to_frame(cells)
    a_c = synth.to_frame(synth.make_jittered(cells, seed=62))
    a_c["Cell_Num_Old"] = np.arange(len(a_c)) * 2 + 7
    mc_a = same_amd.greedy_triangle_collapse(a_c, max_metacell_size=4, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    mc_r = same_amd.greedy_triangle_collapse(r_c, max_metacell_size=3, r_max=40, min_angle_deg=10, return_object=True, verbose=False)
    inc = same_amd.sliding_window_incumbent(mc_r, mc_a, commonCT=synth.type_columns(3), window_local_indices=True, _route="device",
                                            optim_params=dict(radius=30, knn=4, window_size=200, overlap=50, min_cells_per_window=20, **KEY),
                                            gurobi_params=dict(init_method="greedy", lazy_allowed_flip_fraction=0.0,
                                                               lazy_max_cuts_per_incumbent=40))
    want_cols = [str(c) for c in g["sw_metacell/res_columns"]]
    assert [c for c in inc.columns] == [c for c in want_cols if c in inc.columns] and set(want_cols) - set(inc.columns) <= {"members"}
    for c in inc.columns:
        if c not in ("filtered_violation", "run_time"):
            want, got = g[f"sw_metacell/res__{c}"], inc[c].to_numpy()
            assert np.array_equal(got.astype(want.dtype) if want.dtype.kind in "fiub" else got.astype(str), want), c


def _thinned(tri, n, seed, fraction):
    """triangles thinned, shuffled, corners rotated"""
    rng = np.random.default_rng(seed)
    keep = rng.random(len(tri)) >= fraction
    t = tri[keep][rng.permutation(int(keep.sum()))]
    rot = rng.integers(0, 3, len(t))
    return np.take_along_axis(t, (np.arange(3)[None, :] + rot[:, None]) % 3, axis=1)


def test_shapes_of_triangulation():
    r_df, m_df, tri, cols = _plain()
    cols = list(cols)
    ids = m_df["vid"].to_numpy()
    # a DataFrame in index space, vertex_col None
    _both(r_df, m_df, cols, OP, "frame/index", moving_delaunay=pd.DataFrame(tri, columns=["a", "b", "c"]))
    # ids offset by 10^6 and non-contiguous, an index that is not the row number
    shuffled = m_df.set_index(np.random.default_rng(3).permutation(len(m_df)) + 50)
    _both(r_df, shuffled, cols, OP, "labels", moving_delaunay=shuffled.index.to_numpy()[tri])
    _both(r_df, m_df, cols, OP, "ids", moving_delaunay=ids[tri], moving_delaunay_vertex_col="vid")
    # ids the frame does not have
    absent = np.vstack([ids[tri[:40]], [[5, 6, 7], [ids[0], ids[1], 999]], ids[tri[40:]]])
    got, st = _both(r_df, m_df, cols, OP, "absent ids", moving_delaunay=absent, moving_delaunay_vertex_col="vid")
    plain, pst = _both(r_df, m_df, cols, OP, "ids", moving_delaunay=ids[tri], moving_delaunay_vertex_col="vid")
    _same_tables(got, plain, "absent ids change nothing")
    # thinned so that many nodes are unconstrained: some windows remove nodes, one removes none.  Which window loses no node under the
    # FULL triangulation is the data's to say (cells at a box's edge keep only the triangles that lie inside the box): the first such
    # window keeps every triangle inside its box, the rest of the section is thinned by 60 %
    from same_amd import windows as W
    inner = W.caller_tris_windows

    def removed_per_window(tag, triangles, opw):
        seen = []

        def spy(states, *a, **k):
            out = inner(states, *a, **k)
            seen.extend(c[1] for c in out)
            return out

        W.caller_tris_windows = spy
        try:
            got, st = _both(r_df, m_df, cols, opw, tag, moving_delaunay=ids[triangles], moving_delaunay_vertex_col="vid", workers=1)
        finally:
            W.caller_tris_windows = inner
        return got, st, seen

    from same_amd.window_api import _WindowJob

    opw = dict(OP, radius=45, min_angle_deg=None)
    full, fst, base = removed_per_window("full", tri, opw)
    plan = _WindowJob(r_df, m_df, cols, None, None, None, opw, None, False, None).plan
    assert len(base) == len(plan) == len(fst) and 0 in base, base
    x0, x1, y0, y1 = plan[base.index(0)]["box"]
    x, y = m_df["X"].to_numpy(), m_df["Y"].to_numpy()
    inside = ((x[tri] >= x0) & (x[tri] < x1) & (y[tri] >= y0) & (y[tri] < y1)).all(axis=1)
    thin = np.vstack([_thinned(tri[~inside], len(m_df), 5, 0.6), tri[inside]])
    got, st, removed = removed_per_window("thinned", thin, opw)
    assert removed[base.index(0)] == 0 and any(r > 0 for r in removed), removed
    assert len(got) < len(full)
    # an empty triangulation: every node is unconstrained, the table is empty, no error
    got, st = _both(r_df, m_df, cols, OP, "empty", moving_delaunay=np.zeros((0, 3), int), moving_delaunay_vertex_col="vid")
    assert len(got) == 0 and st == []
    # one window loses every node among windows that lose none: no triangle touches x < 200, y < 200 (the first window's box)
    hole = tri[~((x[tri] < 205) & (y[tri] < 205)).any(axis=1)]
    got, st = _both(r_df, m_df, cols, OP, "hole", moving_delaunay=ids[hole], moving_delaunay_vertex_col="vid", batch=3)
    assert len(st) == len(pst) - 1
    merged, _ = _both(r_df, m_df, cols, OP, "hole merged", moving_delaunay=ids[hole], moving_delaunay_vertex_col="vid", merge=True)
    assert 0 < len(merged) <= len(got)


@pytest.mark.parametrize("incumbent,refine", [("greedy", None), ("greedy", "local"), ("greedy", "capacity"), ("assignment", None),
                                              ("assignment", "local"), ("assignment", "capacity"), ("transport", None),
                                              ("transport", "capacity")])
@pytest.mark.parametrize("multiplier", [None, 3])
def test_modes(incumbent, refine, multiplier):
    """every start x search `window_mode` allows, on MetaCell references that are shared (penalty_coeff far below a pair's cost); the
    moving side's triangulation is thinned on the left so that cells are removed -- among them the only holders of some metacell
    references, which the limits' frame must still count (`lim` below checks that the case occurs)"""
    ref, mc, cols = _metacells("ms3")
    cols = list(cols)
    mm = 1 if incumbent == "assignment" else 2
    op = dict(OP, max_matches=mm, ref_metacell_match_multiplier=multiplier, penalty_coeff=0.5, hip_incumbent=incumbent)
    if refine is not None:
        op["hip_refine"] = refine
    mdf = mc.metacell_df
    tri = np.asarray(mc.metacell_delaunay)
    pos = pd.Index(mdf[mc.metacell_idx_col]).get_indexer(tri.reshape(-1)).reshape(-1, 3)
    x = mdf["X"].to_numpy()
    left = (x[pos] < 260).any(axis=1)
    thin = np.vstack([tri[~left], _thinned(tri[left], len(mdf), 9, 0.7)])
    kw = dict(moving_delaunay=thin, moving_delaunay_vertex_col=mc.metacell_idx_col)
    got, st = _both(ref, mdf, cols, op, (incumbent, refine, multiplier), **kw)
    assert len(st) >= 9 and len(got) > 100
    if incumbent == "transport" or refine == "capacity":
        key = "ref_extra_matches" if refine == "capacity" else "ref_extra_matches_start"
        assert sum(s[key] for s in st) > 0          # references are shared


def test_a_metacell_reference_named_only_by_removed_cells_still_sets_the_limits():
    """The first window by hand: the LARGEST references (size 3, the corner x, y < 60) are reachable only from aligned cells that the
    caller's triangulation leaves unconstrained (no triangle touches x, y < 100); every second other reference has size 1.5.  With the
    multiplier None the general route reads int(largest size) = 3 from the prune's frame, which still holds the corner: a size-1.5
    reference may take 3 cells.  Were the limits read from the pair list after the removal, int(1.5) = 1 would hold them to one.  Two
    jittered copies of the section are the suitors, so references are shared."""
    from scipy.spatial import Delaunay
    from same_amd import synth

    cells = synth.make_cells(1500, 3, seed=91)
    r_df = synth.to_frame(cells)
    m_df = pd.concat([synth.to_frame(synth.make_jittered(cells, seed=92, drop=0.0)),
                      synth.to_frame(synth.make_jittered(cells, seed=93, drop=0.0))], ignore_index=True)
    m_df["Cell_Num_Old"] = np.arange(len(m_df)) * 3 + 1
    rx, ry = r_df["X"].to_numpy(), r_df["Y"].to_numpy()
    corner = (rx < 60) & (ry < 60)
    assert corner.sum() >= 3
    r_df["size"] = np.where(corner, 3.0, np.where(np.arange(len(r_df)) % 2 == 0, 1.5, 1.0))
    tri = Delaunay(m_df[["X", "Y"]].to_numpy()).simplices
    mx, my = m_df["X"].to_numpy(), m_df["Y"].to_numpy()
    tri = tri[~((mx[tri] < 100) & (my[tri] < 100)).any(axis=1)]          # every aligned cell within reach of the corner goes
    for mult in (None, 3):
        for inc, refine in (("transport", None), ("transport", "capacity"), ("greedy", "capacity")):
            op = dict(OP, max_matches=1, ref_metacell_match_multiplier=mult, penalty_coeff=0.5, hip_incumbent=inc)
            if refine:
                op["hip_refine"] = refine
            _got, st = _both(r_df, m_df, list(synth.type_columns(3)), op, (mult, inc, refine), moving_delaunay=tri, workers=1)
            # the first window uses the capacity that only the prune's frame grants
            assert st[0]["ref_extra_matches" if refine else "ref_extra_matches_start"] > 0, (mult, inc, refine)


def _crowded():
    from same_amd import synth

    cells = synth.make_cells(1500, 3, seed=51)
    r_big = synth.to_frame(cells)
    m_a = synth.to_frame(synth.make_jittered(cells, seed=52))
    m_b = synth.to_frame(synth.make_jittered(cells, seed=53))
    m2 = pd.concat([m_a, m_b], ignore_index=True)
    m2["Cell_Num_Old"] = np.arange(len(m2)) * 3 + 1
    return r_big, m2, synth.type_columns(3)


def _crowded_triangulation(m2):
    from scipy.spatial import Delaunay

    return _thinned(Delaunay(m2[["X", "Y"]].to_numpy()).simplices, len(m2), 13, 0.3)


OP2 = dict(radius=25, knn=6, window_size=100, overlap=4, min_cells_per_window=20)


def test_merge_true_on_the_device_route():
    from same_amd.merge import merge_window_matches_unique_ref

    r_big, m2, cols = _crowded()
    tri = _crowded_triangulation(m2)
    plain, _st = _both(r_big, m2, cols, OP2, "crowded", moving_delaunay=tri)
    want = merge_window_matches_unique_ref([plain])
    assert 300 < len(want) <= len(plain) - 5                # the overlaps do disagree in this job
    one, _st = _both(r_big, m2, cols, OP2, "crowded merged", moving_delaunay=tri, merge=True)
    assert list(one.columns) == list(want.columns) and one.equals(want)


def _sharded_worker(rank, world, out_dir):
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    from test_gpu_caller_triangulation import KEY, OP2, _crowded, _crowded_triangulation
    import same_amd
    from same_amd.dist import MergeChannel
    from same_amd.rendezvous import HostGroup

    r_big, m2, cols = _crowded()
    tri = _crowded_triangulation(m2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), SAME_RDV_DIR=os.path.join(out_dir, "rdv"))
    with HostGroup() as g:
        merged = same_amd.sliding_window_incumbent(r_big, m2, commonCT=cols, optim_params=dict(OP2, **KEY), moving_delaunay=tri, merge=True,
                                                   _route="device", _shard=(rank, world, "block"), _merge_channel=MergeChannel(g))
        g.barrier()
    merged.to_pickle(os.path.join(out_dir, f"merged{rank}.pkl"))


def test_sharded_merge_at_world_two(tmp_path):
    import multiprocessing as mp
    import same_amd
    from same_amd.merge import join_merged_parts

    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_sharded_worker, args=(rank, 2, str(tmp_path))) for rank in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    r_big, m2, cols = _crowded()
    want = same_amd.sliding_window_incumbent(r_big, m2, commonCT=cols, optim_params=dict(OP2), moving_delaunay=_crowded_triangulation(m2),
                                             merge=True, _route="general")
    parts = [pd.read_pickle(tmp_path / f"merged{rank}.pkl") for rank in range(2)]
    assert all(0 < len(p) < len(want) for p in parts)
    assert join_merged_parts(parts).equals(want)


def test_a_cosine_at_the_threshold_is_decided_on_the_host():
    """A triangle whose smallest angle is min_angle_deg to within 1 ulp of the cosine: its window reports `near`, triangles and node mask
    are re-decided with the reference's literal arccos on the host, and the window goes on through the prefiltered forms."""
    from same_amd import windows as W
    from same_amd.triangles import cos_threshold

    r_df, m_df, tri, cols = _plain()
    m_df = m_df.copy()
    _en, thr = cos_threshold(15)
    # three cells of one triangle moved so that the angle at `a` is acos(thr): b on the ray at angle 0, c on the ray at the angle itself
    a, b, c = tri[np.argmin(np.abs(m_df["X"].to_numpy()[tri].mean(axis=1) - 300) + np.abs(m_df["Y"].to_numpy()[tri].mean(axis=1) - 300))]
    ax, ay = m_df.loc[a, "X"], m_df.loc[a, "Y"]
    ang = np.arccos(thr)
    from fractions import Fraction
    import math

    def fma(p, q, r):          # one rounding, as the kernel's fused multiply-add
        return float(Fraction(p) * Fraction(q) + Fraction(r))

    def corner_cos(p1, p2, p3):          # the cosine at p2 in the kernel's own operations (csrc/devmath.h)
        v1x, v1y, v2x, v2y = p1[0] - p2[0], p1[1] - p2[1], p3[0] - p2[0], p3[1] - p2[1]
        n1, n2 = math.sqrt(fma(v1y, v1y, v1x * v1x)), math.sqrt(fma(v2y, v2y, v2x * v2x))
        return fma(v1y, v2y, v1x * v2x) / (n1 * n2)

    found = False
    for scale in np.linspace(8.0, 12.0, 4001):
        bx, by, cx, cy = float(ax + scale), float(ay), float(ax + scale * np.cos(ang)), float(ay + scale * np.sin(ang))
        if abs(corner_cos((bx, by), (float(ax), float(ay)), (cx, cy)) - thr) <= np.spacing(abs(thr)):
            found = True
            break
    assert found
    m_df.loc[b, ["X", "Y"]] = (bx, by)
    m_df.loc[c, ["X", "Y"]] = (cx, cy)
    seen = []
    inner = W.caller_tris_windows

    def spy(states, *args, **k):
        out = inner(states, *args, **k)
        seen.append((k.get("removed") is not None, [o[2] for o in out]))
        return out

    W.caller_tris_windows = spy
    try:
        _both(r_df, m_df, list(cols), OP, "near", moving_delaunay=tri)
        _both(r_df, m_df, list(cols), OP, "near merged", moving_delaunay=tri, merge=True)
    finally:
        W.caller_tris_windows = inner
    assert any(not pre and any(n > 0 for n in near) for pre, near in seen)          # a window reported near ...
    assert any(pre for pre, _near in seen)                                          # ... and came back through the prefiltered form


def test_refusals():
    r_df, m_df, tri, cols = _plain()
    cols = list(cols)
    dup = m_df.copy()
    dup.loc[5, "vid"] = dup.loc[6, "vid"]
    kw = dict(moving_delaunay=dup["vid"].to_numpy()[tri], moving_delaunay_vertex_col="vid")
    want, wst = _run(r_df, dup, cols, OP, _route="general", **kw)
    got, gst = _run(r_df, dup, cols, dict(OP, **KEY), **kw)           # silently the general route
    _same_tables(got, want, "duplicate ids")
    assert gst == wst
    with pytest.raises(ValueError, match="device route does not apply"):
        _run(r_df, dup, cols, dict(OP, **KEY), _route="device", **kw)
    with pytest.raises(ValueError, match="hip_caller_delaunay"):
        _run(r_df, m_df, cols, dict(OP, hip_caller_delaunay="gpu"), moving_delaunay=tri)


def test_library_refuses_bad_arguments_before_any_device_work():
    import ctypes

    from same_amd import _lib
    from same_amd.window_api import _DeviceFrames
    from same_amd.params import init_optim_params

    r_df, m_df, tri, cols = _plain()
    frames = _DeviceFrames(r_df, m_df, list(cols), init_optim_params(**OP))
    try:
        ctx = frames.ctx
        bad = np.ascontiguousarray(tri, dtype=np.int32).copy()
        bad[3, 1] = len(m_df)
        before = ctx.stats()
        h = ctypes.c_void_p()
        rc = ctx.lib.same_caller_tris_create(ctx.handle, frames.dmov.handle, bad.ctypes.data, len(bad), ctypes.byref(h))
        assert rc == _lib.SAME_ERANGE and not h.value
        rc = ctx.lib.same_caller_tris_create(ctx.handle, None, bad.ctypes.data, len(bad), ctypes.byref(h))
        assert rc == _lib.SAME_EINVAL and not h.value
        assert ctx.stats() == before
    finally:
        frames.close()


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(seed):
    """random frames and random thinned / shuffled / rotated triangulations, ids or index labels, random settings"""
    from scipy.spatial import Delaunay
    from same_amd import synth

    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1500, 2600))
    cells = synth.make_cells(n, 3, seed=2000 + seed)
    r_df = synth.to_frame(cells)
    m_df = synth.to_frame(synth.make_jittered(cells, seed=3000 + seed, drop=float(rng.uniform(0.0, 0.2))))
    tri = _thinned(Delaunay(m_df[["X", "Y"]].to_numpy()).simplices, len(m_df), 4000 + seed, float(rng.uniform(0.0, 0.6)))
    op = dict(OP, radius=float(rng.choice([20, 30])), knn=int(rng.integers(2, 7)), min_angle_deg=[15, None, 25][seed % 3],
              ignore_same_type_triangles=bool(seed % 2))
    kw = {}
    if seed % 2:
        m_df["vid"] = rng.permutation(len(m_df)) * 3 + 1_000_000
        kw = dict(moving_delaunay=m_df["vid"].to_numpy()[tri], moving_delaunay_vertex_col="vid")
    else:
        kw = dict(moving_delaunay=tri)
    _both(r_df, m_df, list(synth.type_columns(3)), op, seed, batch=[1, 3, 8, 20][seed % 4], workers=1 + seed % 2,
          merge=seed % 5 == 0, window_local_indices=seed % 5 == 1, **kw)
