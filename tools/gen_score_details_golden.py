"""Record tests/golden/score_details.npz by RUNNING THE REFERENCE (build container only; not part of `gen_golden.py all`).

Run:  python3 -B tools/gen_score_details_golden.py

Inputs: the synthetic example's two frames as the reference ships them (examples/synthetic/data/query.csv and ref.csv: XY, `cell_type`,
the type columns c1..c3, `quadrant`), the moving (query) frame's scipy triangulation, and a one-to-one matching made here with numpy and
scipy only: linear_sum_assignment on the Euclidean XY distance plus 3.0 where the two labels differ, pairs further apart than 5 forbidden.
Recorded output: the `triangle_violation` column the reference's check_triangle_violations_within_quadrants
(src/synthetic_datagen.py:1314-1418) returns for that matching -- the function is imported and called, nothing of it is copied.  The
fixture holds arrays only.

The reference flags a triangle by the PRODUCT of its two signed areas, the package by their signs; the two part only where a product
underflows to zero, so the generator asserts that no all-matched triangle has |area| < 1e-9 on either side."""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT = os.environ.get("SAME_REFERENCE_ROOT", "/root/reference")
OUT = os.environ.get("SAME_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
COLUMNS = ("c1", "c2", "c3")
LABEL_PENALTY, MAX_DISTANCE, FORBIDDEN = 3.0, 5.0, 1e6


def load_datagen():
    """src/synthetic_datagen.py loaded by path; its plotting and kernel imports, which the function called here never touches, are
    stubbed where they are absent"""
    path = os.path.join(REF_ROOT, "src", "synthetic_datagen.py")
    if not os.path.isfile(path):
        raise RuntimeError(f"reference not mounted at {REF_ROOT}; fixtures can only be generated in the build container")
    sys.dont_write_bytecode = True
    for name, attrs in (("matplotlib", {}), ("matplotlib.pyplot", {}), ("sklearn", {}), ("sklearn.gaussian_process", {}),
                        ("sklearn.gaussian_process.kernels", {"RBF": None})):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.__path__ = []
            for k, v in attrs.items():
                setattr(mod, k, v)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("_same_reference_synthetic_datagen", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def signed_area(p):
    """(n, 3, 2) corners -> (n,) signed areas"""
    return 0.5 * ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))


def main():
    import pandas as pd
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import Delaunay
    from scipy.spatial.distance import cdist

    datagen = load_datagen()
    data = os.path.join(REF_ROOT, "examples", "synthetic", "data")
    mov, ref = pd.read_csv(os.path.join(data, "query.csv"), index_col=0), pd.read_csv(os.path.join(data, "ref.csv"), index_col=0)
    mov_xy, ref_xy = mov[["X", "Y"]].to_numpy(np.float64), ref[["X", "Y"]].to_numpy(np.float64)
    tris = Delaunay(mov_xy).simplices.astype(np.int32)

    dist = cdist(mov_xy, ref_xy)
    cost = dist + LABEL_PENALTY * (mov["cell_type"].to_numpy()[:, None] != ref["cell_type"].to_numpy()[None, :])
    cost[dist > MAX_DISTANCE] = FORBIDDEN
    rows, cols = linear_sum_assignment(cost)
    keep = cost[rows, cols] < FORBIDDEN
    a_row, r_row = rows[keep].astype(np.int32), cols[keep].astype(np.int32)
    assert len(np.unique(r_row)) == len(r_row)

    matched = np.full(len(mov), -1, np.int64)
    matched[a_row] = r_row
    full = (matched[tris] >= 0).all(axis=1)
    smallest = min(float(np.abs(signed_area(mov_xy[tris[full]])).min()), float(np.abs(signed_area(ref_xy[matched[tris[full]]])).min()))
    assert smallest >= 1e-9, smallest

    matches = pd.DataFrame({"aligned_idx": a_row.astype(np.int64), "ref_idx": r_row.astype(np.int64), "X": mov_xy[a_row, 0],
                            "Y": mov_xy[a_row, 1], "ref_X": ref_xy[r_row, 0], "ref_Y": ref_xy[r_row, 1]})
    carrier = types.SimpleNamespace(metacell_delaunay=tris, metacell_df=mov.reset_index(drop=True))
    with contextlib.redirect_stdout(io.StringIO()):
        flagged = datagen.check_triangle_violations_within_quadrants(matches, carrier)["triangle_violation"].to_numpy(dtype=bool)

    quadrant = mov["quadrant"].to_numpy().astype(str)
    same_quadrant = (quadrant[tris] == quadrant[tris[:, :1]]).all(axis=1)
    out = {"commonCT": np.array(COLUMNS), "mov_xy": mov_xy, "ref_xy": ref_xy,
           "mov_cell_type": mov["cell_type"].to_numpy().astype(str), "ref_cell_type": ref["cell_type"].to_numpy().astype(str),
           "mov_types": mov[list(COLUMNS)].to_numpy(np.float64), "ref_types": ref[list(COLUMNS)].to_numpy(np.float64),
           "mov_quadrant": quadrant, "ref_quadrant": ref["quadrant"].to_numpy().astype(str), "tris": tris, "a_row": a_row, "r_row": r_row,
           "triangle_violation": flagged}
    path = os.path.join(OUT, "score_details.npz")
    np.savez_compressed(path, **out)
    per = {q: int(flagged[quadrant[a_row] == q].sum()) for q in pd.unique(quadrant)}
    print(f"wrote {path}: {len(a_row)} of {len(mov)} cells matched, {len(tris)} triangles, {int((~same_quadrant).sum())} cross-quadrant, "
          f"smallest |area| {smallest:.3g}, flagged per quadrant {per}")


if __name__ == "__main__":
    main()
