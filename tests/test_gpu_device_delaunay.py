"""The window path triangulated on the device (optim_params["hip_delaunay"] = "device", csrc/delaunay_dev.hip) against scipy's
triangulation -- the reference's call (src/same.py:1023) -- followed by the reference's filter (src/helpers.py:298-340): the device's
candidates are scipy's triangles that pass a slack screen of the filter, degenerate sets are refused (never answered wrongly), and the
product function's tables and per-window statistics are the default route's."""
import zlib

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import Delaunay

from oracle import same_oracle as orc

pytestmark = pytest.mark.gpu


def _sorted_set(tris):
    return {tuple(sorted(int(v) for v in t)) for t in np.asarray(tris).reshape(-1, 3)}


def _family(rng, family, n):
    side = float(np.sqrt(n / 0.01))                   # cfg 5's density: 0.01 cells per unit area
    if family == "uniform":
        return rng.uniform(0, side, (n, 2))
    if family == "blobs":
        k = 6                                         # (peak density about cfg 5's: a far denser set overflows a neighbour list and is refused)
        return np.concatenate([rng.normal(c, side / 6, (n // k, 2)) for c in rng.uniform(0.2 * side, 0.8 * side, (k, 2))])
    if family == "clusters":
        centres = rng.uniform(0, side, (n // 20, 2))
        return centres[rng.integers(0, len(centres), n)] + rng.normal(0, 4.0, (n, 2))
    if family == "strips":
        x = rng.uniform(0, side, n)
        return np.column_stack((x, rng.integers(0, 8, n) * side / 8 + rng.normal(0, 3.0, n)))
    if family == "jittered_lattice":
        g = np.arange(0.0, side, 10.0)
        pts = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
        return pts + rng.normal(0, 1.0, pts.shape)
    raise ValueError(family)


@pytest.mark.parametrize("offset", [0.0, 1e6, 1e8])
@pytest.mark.parametrize("family", ["uniform", "blobs", "clusters", "strips", "jittered_lattice"])
@pytest.mark.parametrize("radius,angle", [(25.0, 15.0), (50.0, 15.0), (12.0, 10.0)])
def test_device_candidates_are_scipys_triangles_that_pass_the_filter(family, offset, radius, angle):
    from same_amd import _lib, delaunay

    rng = np.random.default_rng(zlib.crc32(repr((family, offset, radius, angle)).encode()))
    xy = np.ascontiguousarray(_family(rng, family, 3000) + offset)
    got, status = delaunay.device_filtered_triangles(xy, radius, angle, with_status=True)
    if got is None:
        # far from the origin Qhull's own allowance grows with the coordinates (and refusing is always allowed there); near it these
        # generic sets are refused only where a list outgrows its buffer (dense clusters), never for a sign in doubt
        assert offset >= 1e6 or status == _lib.SAME_DD_OVERFLOW, (family, offset, status)
        return
    simplices = Delaunay(xy).simplices
    kept = _sorted_set(orc.filter_triangles_by_radius(xy, simplices, radius, min_angle_deg=angle))
    cand = _sorted_set(got)
    assert len(cand) == len(got)                                                   # no triangle twice
    assert kept <= cand <= _sorted_set(simplices)                                  # a superset of the kept ones, all of them Qhull's
    assert _sorted_set(orc.filter_triangles_by_radius(xy, got, radius, min_angle_deg=angle)) == kept
    P = xy[got]
    area2 = (P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0])
    assert (area2 > 0).all()                                                       # counter-clockwise
    assert (got[:, 0] < got[:, 1:].min(axis=1)).all() and (np.diff(got[:, 0]) >= 0).all()   # by owner (the smallest corner)


def test_degenerate_sets_are_refused():
    from same_amd import delaunay

    rng = np.random.default_rng(7)
    lattice = np.stack(np.meshgrid(np.arange(0.0, 300.0, 10.0), np.arange(0.0, 300.0, 10.0)), -1).reshape(-1, 2)
    base = rng.uniform(0, 400, (1500, 2))
    duplicated = np.concatenate([base, base[rng.choice(len(base), 40, replace=False)]])
    t = np.linspace(0, 2 * np.pi, 9)[:-1]
    ring = np.column_stack((200 + 10 * np.cos(t), 200 + 10 * np.sin(t)))
    rings = np.concatenate([base[np.hypot(base[:, 0] - 200, base[:, 1] - 200) > 40], ring])
    line = np.column_stack((np.arange(0.0, 400.0, 7.0), np.full(58, -5.0)))
    collinear = np.concatenate([base, line])
    for name, xy in (("lattice", lattice), ("duplicates", duplicated), ("cocircular", rings), ("collinear", collinear)):
        assert delaunay.device_filtered_triangles(np.ascontiguousarray(xy), 25.0, 10.0) is None, name
    assert delaunay.device_filtered_triangles(base, 25.0, None) is None           # no angle threshold: no circumradius bound
    assert delaunay.device_filtered_triangles(base[:2], 25.0, 15.0) is None       # fewer than 3 points


def _frames(rng, n, side, integer_ref=False):
    T = 4
    rxy = rng.uniform(0, side, (n, 2))
    mxy = rxy[rng.random(n) < 0.93] + rng.normal(0, 1.5, (1, 2))
    mxy = mxy + rng.normal(0, 1.0, mxy.shape)
    if integer_ref:
        rxy = np.round(rxy)
    out = []
    for xy in (rxy, mxy):
        df = pd.DataFrame(rng.gamma(0.3, 30.0, (len(xy), T)), columns=[f"t{q}" for q in range(T)])
        df.insert(0, "Y", xy[:, 1])
        df.insert(0, "X", xy[:, 0])
        df["cell_type"] = rng.choice(np.array(["a", "b", "c"], dtype=object), len(xy))
        df["Cell_Num_Old"] = rng.permutation(len(xy)) * 2 + 5
        out.append(df)
    return out[0], out[1], [f"t{q}" for q in range(T)]


@pytest.mark.parametrize("integer_ref", [False, True])
def test_tables_with_the_device_triangulation_are_the_tables_with_scipy(integer_ref):
    """`sliding_window_incumbent`, merged and plain, with the per-window statistics: hip_delaunay = 'device' gives the very tables of
    the default.  Generic coordinates: no window refused or re-finished; reference cells on whole coordinates: windows count order
    ties and are finished again with scipy's simplices -- same tables still."""
    import same_amd
    from same_amd import delaunay

    rng = np.random.default_rng(11 + integer_ref)
    r_df, m_df, cols = _frames(rng, 30000, 900.0, integer_ref)
    op = dict(radius=12, knn=6, window_size=200, overlap=40, min_cells_per_window=10, hip_cost_dtype="float32")
    resident = same_amd.resident_frames(r_df, m_df)
    try:
        for merge in (True, False):
            want = same_amd.sliding_window_incumbent(resident, resident, commonCT=cols, optim_params=dict(op), merge=merge,
                                                     return_stats=True)
            got = same_amd.sliding_window_incumbent(resident, resident, commonCT=cols, optim_params=dict(op, hip_delaunay="device"),
                                                    merge=merge, return_stats=True)
            st = delaunay.last_device_stats()
            assert len(want[0]) > 15000 and got[0].equals(want[0]) and list(got[0].columns) == list(want[0].columns)
            assert got[1] == want[1] and len(want[1]) >= 25
            assert st["submitted"] == len(want[1]), st
            if integer_ref:
                assert st["refinished"] > 0, st
            else:
                assert st["refused"] == 0 and st["refinished"] == 0, st
    finally:
        resident.close()


def test_fuzz_tables_device_route():
    """seeded fuzz: small frames of several shapes (generic, clustered, whole-number reference cells, a coarse aligned lattice), both
    routes' merged tables and statistics identical"""
    import same_amd

    for seed in range(6):
        rng = np.random.default_rng(500 + seed)
        n, side = int(rng.integers(2000, 8000)), float(rng.uniform(200, 600))
        r_df, m_df, cols = _frames(rng, n, side, integer_ref=seed % 3 == 2)
        if seed % 3 == 1:
            for df in (r_df, m_df):
                df["X"] = np.round(df["X"] / 3) * 3 + rng.normal(0, 0.4, len(df))
        op = dict(radius=float(rng.choice([8.0, 12.0, 20.0])), knn=int(rng.integers(3, 9)), window_size=int(rng.choice([100, 150])),
                  overlap=20, min_cells_per_window=5, min_angle_deg=float(rng.choice([10.0, 15.0])))
        with same_amd.resident_frames(r_df, m_df) as res:
            for merge in (True, False):
                want = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op), merge=merge, return_stats=True)
                got = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op, hip_delaunay="device"), merge=merge,
                                                        return_stats=True)
                assert got[0].equals(want[0]) and got[1] == want[1], (seed, merge)


def test_answered_batch_from_the_device_source_uploads_no_simplices():
    """the device's candidates never cross the bus: the device finish call makes one copy fewer than the same finish with the
    simplices from the host (their upload), and the match it computes is the same"""
    from same_amd import _lib, synth
    from same_amd import windows as W
    from same_amd.triangles import cos_threshold

    ctx = _lib.default_context(0)
    ref = synth.make_cells(4000, 4, seed=3)
    mov = synth.make_jittered(ref, seed=4)
    tid = np.unique(mov["cell_type"], return_inverse=True)[1].astype(np.int32)
    rs, ms = W.Section(ref["xy"], ref["types"], None, None), W.Section(mov["xy"], mov["types"], tid, mov["size"])
    dref, dmov = W.DeviceSection(rs, np.float64, ctx), W.DeviceSection(ms, np.float64, ctx)
    st = W.DeviceWindow(ctx)
    en, thr = cos_threshold(15)
    box = [(-1e9, 1e9, -1e9, 1e9)]
    try:
        W.stage_windows([st], dmov, dref, box, 25.0, 8, 1.0)
        status, n_tris = W.triangulate_windows([st], 25.0, en, thr, 16.0)
        assert status[0] == 0 and n_tris[0] > 0
        before = ctx.stats()
        dev = W.filter_finish_windows([st], None, 25.0, en, thr, 0.0, True, 100.0)[0]
        dev_copies = ctx.stats()["copies"] - before["copies"]
        host_tris = Delaunay(st.fetch(W._W_ALIGNED_XY)).simplices
        W.stage_windows([st], dmov, dref, box, 25.0, 8, 1.0)
        before = ctx.stats()
        host = W.filter_finish_windows([st], [host_tris], 25.0, en, thr, 0.0, True, 100.0)[0]
        host_copies = ctx.stats()["copies"] - before["copies"]
        assert dev_copies + 1 == host_copies, (dev_copies, host_copies)
        assert dev[0] == host[0] and dev[1] == host[1]
        if not st.order_ties:
            assert np.array_equal(dev[3], host[3]) and np.array_equal(dev[4], host[4]) and dev[5] == host[5]
    finally:
        st.close()
        dref.close()
        dmov.close()


def test_cfg5_1m_cells_device_triangulation_gives_the_same_merged_table():
    """BASELINE config 5 at full size through the product function, window merge included, triangulated on the device and by scipy:
    the merged tables and every window's counters are identical"""
    import same_amd
    from same_amd import delaunay, synth

    T = 8
    ref = synth.make_cells(1_000_000, T, seed=0)
    mov = synth.make_jittered(ref, seed=1)
    r_df, m_df = synth.to_frame(ref), synth.to_frame(mov)
    r_df["Cell_Num_Old"], m_df["Cell_Num_Old"] = np.arange(len(r_df)), np.arange(len(m_df))
    cols = synth.type_columns(T)
    op = dict(radius=25, knn=8, no_match_penalty=100, hip_cost_dtype="float32", window_size=1200, overlap=300, min_cells_per_window=10)
    with same_amd.resident_frames(r_df, m_df) as res:
        want, want_stats = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op), merge=True, return_stats=True)
        got, got_stats = same_amd.sliding_window_incumbent(res, res, commonCT=cols, optim_params=dict(op, hip_delaunay="device"),
                                                           merge=True, return_stats=True)
    st = delaunay.last_device_stats()
    assert len(want) > 900_000 and got.equals(want) and got_stats == want_stats
    assert st["submitted"] == len(want_stats) > 100 and st["refused"] <= st["submitted"] // 10, st
