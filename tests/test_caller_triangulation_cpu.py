"""The host side of optim_params["hip_caller_delaunay"] = "device" (no GPU needed): the once-per-job preparation of a caller's
triangulation, its refusals, the key's validation, and the REASONING of csrc/window_caller.hip restated in numpy -- select + remap in the
caller's order, the node mask, the second compaction, then the unchanged filter on the smaller window -- against the reference's flow
(src/same.py:1016-1085: remap by a per-window dict, filter with remove_unconstrained_nodes=True, delete, renumber) as same_amd's own
host pieces and the CPU oracle's filter (oracle.filter_triangles_by_radius, src/helpers.py:233-395) run it: the second half of
`prepare_same_inputs(..., aligned_delaunay=...)` step for step, whose own kernels need a GPU.  The kernels themselves are held against
that function's route through sliding_window_incumbent in tests/test_gpu_caller_triangulation.py."""
import numpy as np
import pandas as pd
import pytest


def _frame(n, seed=0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({"X": rng.uniform(0, 100, n), "Y": rng.uniform(0, 100, n), "cell_type": rng.integers(0, 3, n)})


def test_ids_map_to_rows_by_vertex_col_and_by_index_labels():
    from same_amd.window_api import caller_triangulation_rows

    df = _frame(8)
    df["vid"] = [1_000_007, 1_000_000, 1_000_021, 1_000_014, 1_000_035, 1_000_028, 1_000_049, 1_000_042]
    tri_rows = np.array([[0, 1, 2], [2, 1, 3], [7, 5, 6], [4, 0, 3]])
    rows, why = caller_triangulation_rows(df, df["vid"].to_numpy()[tri_rows], "vid")
    assert why is None and rows.dtype == np.int32 and np.array_equal(rows, tri_rows)
    labelled = df.set_index(pd.Index([50, 40, 30, 20, 10, 0, 70, 60]))
    rows, why = caller_triangulation_rows(labelled, pd.DataFrame(labelled.index.to_numpy()[tri_rows], columns=list("abc")), None)
    assert why is None and np.array_equal(rows, tri_rows)
    # integral floats are ids too (the reference's dict looks 3 up under 3.0)
    rows, why = caller_triangulation_rows(df.assign(vid=df["vid"].astype(float)), df["vid"].to_numpy()[tri_rows].astype(float), "vid")
    assert why is None and np.array_equal(rows, tri_rows)
    rows, why = caller_triangulation_rows(df, np.zeros((0, 3), int), "vid")
    assert why is None and rows.shape == (0, 3)
    rows, why = caller_triangulation_rows(df, [], None)
    assert why is None and rows.shape == (0, 3)


def test_triangles_naming_absent_ids_go_and_the_order_stays():
    from same_amd.window_api import caller_triangulation_rows
    from same_amd.triangles import _remap_triangles_by_vertex_ids

    df = _frame(6)
    df["vid"] = np.arange(6) * 10 + 5
    tri = np.array([[25, 5, 15], [5, 15, 999], [55, 45, 35], [-3, 5, 15], [35, 15, 5], [15, 25, 45]])
    rows, why = caller_triangulation_rows(df, tri, "vid")
    assert why is None and np.array_equal(rows, [[2, 0, 1], [5, 4, 3], [3, 1, 0], [1, 2, 4]])
    # and it is the reference's own remap (src/same.py:262-290) where that is defined: ids unique
    assert np.array_equal(rows, _remap_triangles_by_vertex_ids(tri, df["vid"].to_numpy()))


def test_every_refusal_names_its_reason():
    from same_amd.params import init_optim_params
    from same_amd.window_api import caller_triangulation_refusal, caller_triangulation_rows

    df = _frame(6)
    df["vid"] = np.arange(6) * 10 + 5
    tri = np.array([[5, 15, 25], [35, 45, 55]])
    assert caller_triangulation_rows(df.assign(vid=[5, 15, 25, 25, 45, 55]), tri, "vid") == (None, "the frame's vertex ids are not unique")
    assert caller_triangulation_rows(df.set_index(pd.Index([0, 1, 1, 2, 3, 4])), tri, None)[1] == "the frame's vertex ids are not unique"
    same_set = np.array([[5, 15, 25], [35, 45, 55], [25, 5, 15]])
    assert caller_triangulation_rows(df, same_set, "vid") == (None, "two triangles have the same vertex set")
    assert caller_triangulation_rows(df, tri + 0.5, "vid") == (None, "the triangulation's vertex ids are not integers")
    assert caller_triangulation_rows(df.assign(vid=df["vid"] + 0.25), tri, "vid") == (None, "the frame's vertex ids are not integers")
    assert caller_triangulation_rows(df.assign(vid=list("abcdef")), tri, "vid") == (None, "the frame's vertex ids are not integers")
    assert caller_triangulation_rows(df, tri, "nope") == (None, "aligned_delaunay_vertex_col missing")
    # the refusal function: the sections' own reasons first, then the priority filter, then the triangulation's
    cols = ["t0", "t1"]
    full = df.assign(t0=1.0, t1=0.0)
    op = init_optim_params()
    assert caller_triangulation_refusal(full, full, cols, op, tri, "vid") is None
    assert caller_triangulation_refusal(full, full.drop(columns=["t1"]), cols, op, tri, "vid") == "a commonCT / coordinate column is missing"
    assert caller_triangulation_refusal(full, full, cols, dict(op, ignore_knn_if_matched=True), tri, "vid") == "ignore_knn_if_matched"
    assert caller_triangulation_refusal(full, full, cols, op, same_set, "vid") == "two triangles have the same vertex set"
    assert caller_triangulation_refusal(full, full.assign(vid=5), cols, op, tri, "vid") == "the frame's vertex ids are not unique"


def test_the_key_is_validated_with_the_other_hip_keys():
    from same_amd.window_mode import WindowMode, caller_delaunay_route

    assert caller_delaunay_route({}) == caller_delaunay_route(None) == caller_delaunay_route({"hip_caller_delaunay": None}) == "host"
    assert caller_delaunay_route({"hip_caller_delaunay": "host"}) == "host"
    assert caller_delaunay_route({"hip_caller_delaunay": "device"}) == "device"
    for bad in ("gpu", "Device", 1, True, b"device"):
        with pytest.raises(ValueError, match="hip_caller_delaunay"):
            WindowMode.from_params({"hip_caller_delaunay": bad})
    assert WindowMode.from_params({"hip_caller_delaunay": "device"}) == WindowMode.default()


def device_front(rows_kept, job_rows, xy, type_id, pairs, radius, min_angle_deg, ignore_same_type, oracle):
    """csrc/window_caller.hip + the filter that follows, in numpy, for one window: `rows_kept` the ascending frame rows of its kept aligned
    cells, `job_rows` the job's triangles as frame rows (caller_triangulation_rows), `pairs` (P, 2) over the kept cells (rows ascending).
    -> (kept triangles renumbered, in the reference's order; removed nodes; renumbered pairs; cells left)"""
    from caller_check import filtered_after, window_statement

    _sel, valid, n_left, pairs2, _costs, tris2 = window_statement(rows_kept, job_rows, xy, type_id, pairs, np.zeros(len(pairs)), radius,
                                                                  min_angle_deg, ignore_same_type, oracle)
    kept = filtered_after(xy, type_id, valid, tris2, radius, min_angle_deg, ignore_same_type, oracle)
    return kept, np.flatnonzero(~valid), pairs2, n_left


def reference_flow(vertex_ids, caller_tris, xy, type_id, pairs, radius, min_angle_deg, ignore_same_type, oracle):
    """src/same.py:1016-1085 for one window's frame: remap by the window's ids, filter with removal, delete, renumber"""
    from same_amd.triangles import _remap_triangles_by_vertex_ids

    n = len(vertex_ids)
    tris = _remap_triangles_by_vertex_ids(caller_tris, vertex_ids)
    frame = pd.DataFrame({"cell_type": type_id})
    kept, gone = oracle.filter_triangles_by_radius(xy, tris, radius, aligned_df=frame, ignore_same_type_triangles=ignore_same_type,
                                                   remove_unconstrained_nodes=True, min_angle_deg=min_angle_deg)
    kept = np.asarray(kept, dtype=np.int64).reshape(-1, 3)
    keep_node = np.ones(n, bool)
    keep_node[sorted(gone)] = False
    new = np.full(n, -1, np.int64)
    new[keep_node] = np.arange(int(keep_node.sum()))
    vp = pairs[keep_node[pairs[:, 0]]]
    kept = kept[keep_node[kept].all(axis=1)] if len(kept) else kept
    return new[kept], np.flatnonzero(~keep_node), np.column_stack((new[vp[:, 0]], vp[:, 1])), int(keep_node.sum()), kept


@pytest.mark.parametrize("seed", range(30))
def test_the_device_front_restated_equals_the_reference_flow(oracle, seed):
    from scipy.spatial import Delaunay
    from same_amd.window_api import caller_triangulation_rows

    rng = np.random.default_rng(500 + seed)
    n_job = int(rng.integers(400, 900))                 # the job's frame; the window is a box of 50-300 of its cells
    xy_job = rng.uniform(0, 100, (n_job, 2))
    ids = rng.permutation(n_job) * 3 + 1_000_000
    job = pd.DataFrame({"X": xy_job[:, 0], "Y": xy_job[:, 1], "vid": ids})
    type_job = rng.integers(0, 3, n_job).astype(np.int32)
    tri = Delaunay(xy_job).simplices
    tri = tri[rng.random(len(tri)) >= rng.uniform(0.0, 0.6)]               # thinned by 0-60 %
    tri = tri[rng.permutation(len(tri))]                                    # shuffled
    tri = np.take_along_axis(tri, (np.arange(3)[None, :] + rng.integers(0, 3, len(tri))[:, None]) % 3, axis=1)    # corners rotated
    caller = ids[tri]
    job_rows, why = caller_triangulation_rows(job, caller, "vid")
    assert why is None and np.array_equal(job_rows, tri)
    want_cells = int(rng.integers(50, 301))
    half = 50.0 * np.sqrt(want_cells / n_job)
    cx, cy = rng.uniform(half, 100 - half, 2)
    in_box = np.flatnonzero((np.abs(xy_job[:, 0] - cx) < half) & (np.abs(xy_job[:, 1] - cy) < half))
    rows_kept = in_box[rng.random(len(in_box)) >= 0.1]                     # (the prune keeps most cells of the box)
    xy, type_id = xy_job[rows_kept], type_job[rows_kept]
    n = len(rows_kept)
    a = np.sort(np.repeat(np.arange(n), 3))
    pairs = np.column_stack((a, rng.integers(0, 40, len(a))))
    radius, angle, same = float(rng.choice([8.0, 12.0, 30.0])), [15, None, 25][seed % 3], bool(seed % 2)
    got_tris, got_gone, got_pairs, got_n = device_front(rows_kept, job_rows, xy, type_id, pairs, radius, angle, same, oracle)
    want_tris, want_gone, want_pairs, want_n, kept_before = reference_flow(ids[rows_kept], caller, xy, type_id, pairs, radius, angle, same,
                                                                           oracle)
    assert np.array_equal(got_tris, want_tris)                              # the kept triangles, in order
    assert np.array_equal(got_gone, want_gone) and got_n == want_n          # the unconstrained set
    assert np.array_equal(got_pairs, want_pairs)                            # the renumbered pairs
    gone = np.zeros(n, bool)
    gone[want_gone] = True
    # no kept triangle names a removed node: every vertex of a kept (or added-back) triangle is valid by construction
    full_kept, _g = oracle.filter_triangles_by_radius(xy, np.searchsorted(rows_kept, tri[np.isin(tri, rows_kept).all(axis=1)]), radius,
                                                      aligned_df=pd.DataFrame({"cell_type": type_id}), ignore_same_type_triangles=same,
                                                      remove_unconstrained_nodes=True, min_angle_deg=angle)
    full_kept = np.asarray(full_kept, dtype=np.int64).reshape(-1, 3)
    assert not gone[full_kept].any() and len(full_kept) == len(kept_before) == len(want_tris)
