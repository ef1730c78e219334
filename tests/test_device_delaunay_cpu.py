"""The device triangulation route (optim_params["hip_delaunay"] = "device", csrc/delaunay_dev.hip) on the CPU: the mode switch, the
ABI surface, and the premise the route is built on -- the filter's kept triangles are exactly the triangles that pass the filter and
have an empty circumcircle -- stated in numpy and held against the reference's filter over scipy's triangulation."""
import ctypes
import os
import zlib

import numpy as np
import pytest
from scipy.spatial import Delaunay, cKDTree

from oracle import same_oracle as orc


def test_mode_accepts_device_from_params_and_environment(monkeypatch):
    from same_amd import delaunay

    monkeypatch.delenv("SAME_DELAUNAY", raising=False)
    assert delaunay.mode({"hip_delaunay": "device"}) == "device"
    assert delaunay.mode({"hip_delaunay": "DEVICE"}) == "device"
    assert delaunay.mode(None) == "qhull"
    monkeypatch.setenv("SAME_DELAUNAY", "device")
    assert delaunay.mode({}) == "device"
    assert delaunay.mode({"hip_delaunay": "native"}) == "native"          # the parameter wins over the environment
    for bad in ("gpu", "scipy", "devices"):
        with pytest.raises(ValueError):
            delaunay.mode({"hip_delaunay": bad})


def test_abi9_entry_points_are_exported_and_declared():
    from same_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "same_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("same_window_delaunay", "same_window_filter_finish", "same_delaunay_filtered"):
        assert name in _lib.EXPORTS
        assert f"int {name}(" in header
        assert hasattr(lib, name)
    for name in ("same_window_filter_finish_device", "same_window_set_incumbent", "same_window_incumbent_result", "same_window_set_refine",
                 "same_window_refine_result"):       # folded into same_window_filter_finish (ABI 9)
        assert name not in _lib.EXPORTS and not hasattr(lib, name)
    for name in ("SAME_DD_FEW_POINTS", "SAME_DD_NO_ANGLE", "SAME_DD_NONFINITE", "SAME_DD_IN_DOUBT", "SAME_DD_OVERFLOW",
                 "SAME_TRIS_SIMPLICES", "SAME_TRIS_KEPT", "SAME_TRIS_DEVICE", "SAME_WINDOW_STATS"):
        assert f"#define {name} {getattr(_lib, name)}" in " ".join(header.split())


def _local_rule(xy, radius, min_angle_deg):
    """every triangle (sorted triple) whose sides are < radius, whose angles are >= min_angle_deg (the reference's expressions,
    src/helpers.py:278-319) and whose circumcircle holds no other point -- no triangulation anywhere"""
    tree = cKDTree(xy)
    out = set()
    for p in range(len(xy)):
        nb = sorted(q for q in tree.query_ball_point(xy[p], radius) if q > p)
        for a in range(len(nb)):
            for b in range(a + 1, len(nb)):
                tri = (p, nb[a], nb[b])
                P = xy[list(tri)]
                sides = [np.linalg.norm(P[1] - P[0]), np.linalg.norm(P[2] - P[1]), np.linalg.norm(P[0] - P[2])]
                if max(sides) >= radius:
                    continue
                ok = True
                for c in range(3):
                    v1, v2 = P[(c + 1) % 3] - P[c], P[(c + 2) % 3] - P[c]
                    cosv = np.clip(np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2)), -1.0, 1.0)
                    ok &= np.degrees(np.arccos(cosv)) >= min_angle_deg
                if not ok:
                    continue
                (ax, ay), (bx, by), (cx, cy) = P
                d = 2 * (ax * (by - cy) + bx * (cy - ay) + cx * (ay - by))
                ux = ((ax * ax + ay * ay) * (by - cy) + (bx * bx + by * by) * (cy - ay) + (cx * cx + cy * cy) * (ay - by)) / d
                uy = ((ax * ax + ay * ay) * (cx - bx) + (bx * bx + by * by) * (ax - cx) + (cx * cx + cy * cy) * (bx - ax)) / d
                r2 = (ax - ux) ** 2 + (ay - uy) ** 2
                near = [s for s in tree.query_ball_point((ux, uy), np.sqrt(r2) * (1 + 1e-9)) if s not in tri]
                if all((xy[s, 0] - ux) ** 2 + (xy[s, 1] - uy) ** 2 > r2 for s in near):
                    out.add(tri)
    return out


@pytest.mark.parametrize("family", ["uniform", "blobs", "jittered_lattice"])
@pytest.mark.parametrize("radius,angle", [(25.0, 15.0), (50.0, 15.0), (12.0, 10.0)])
def test_local_rule_is_the_filter_of_the_triangulation(family, radius, angle):
    """the premise of the device route, pinned without a GPU: as SETS, the filter's kept triangles of scipy's triangulation are the
    triangles the local rule finds (generic sets at cfg 5's density, the reference datasets' radius / angle pairs)"""
    rng = np.random.default_rng(zlib.crc32(repr((family, radius, angle)).encode()))
    side = 160.0
    if family == "uniform":
        xy = rng.uniform(0, side, (256, 2))
    elif family == "blobs":
        xy = np.concatenate([rng.normal(c, 12.0, (64, 2)) for c in rng.uniform(30, side - 30, (4, 2))])
    else:
        g = np.arange(0.0, side, 10.0)
        xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2) + rng.normal(0, 1.5, (len(g) ** 2, 2))
    xy = np.ascontiguousarray(xy)
    kept = orc.filter_triangles_by_radius(xy, Delaunay(xy).simplices, radius, min_angle_deg=angle)
    want = {tuple(sorted(int(v) for v in t)) for t in kept}
    assert len(want) > 20
    assert _local_rule(xy, radius, angle) == want
