"""Record tests/golden/check_alignment.npz by RUNNING THE REFERENCE (build container only; not part of `gen_golden.py all`).

Run:  python3 -B tools/gen_golden_alignment.py

The reference's eval_utils.check_alignment (src/eval_utils.py:6-53) runs as-is on small query / template frames of the families
below, for kNN 1, 3 and 8 where the template is large enough.  The fixture holds each case's inputs (coordinates; labels as
(kind, text), tests/alignment_check.py) and, per kNN, the reference's match column, its score and -- kNN == 1 -- its
`_1NN_match_ctype` column; or the name of the exception it raised.  same_amd.eval_utils.check_alignment must reproduce them exactly.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alignment_check import decode_labels, encode_labels  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.environ.get("SAME_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
KS = (1, 3, 8)
TIE_FAMILIES = ("lattice", "duplicates")   # families whose rows include exact distance ties


def _types(rng, n, t=6):
    return np.array([f"T{i}" for i in rng.integers(0, t, n)], dtype=object)


def _argmax_type(g, prefix, names, suffix=""):
    m = np.stack([np.asarray(g[f"{prefix}__{c}{suffix}"], np.float64) for c in names], 1)
    return np.array([names[i] for i in m.argmax(1)], dtype=object)


def cases():
    """(name, query xy, query labels, template xy, template labels)"""
    rng = np.random.default_rng(2024)
    yield "uniform", rng.random((1500, 2)) * 100, _types(rng, 1500), rng.random((1200, 2)) * 100, _types(rng, 1200)
    gx, gy = np.meshgrid(np.arange(30.0), np.arange(30.0))
    lat = np.column_stack([gx.ravel(), gy.ravel()])
    hx, hy = np.meshgrid(np.arange(29.0) + 0.5, np.arange(29.0) + 0.5)
    qlat = np.vstack([np.column_stack([hx.ravel(), hy.ravel()]), lat[rng.choice(len(lat), 200, replace=False)] + [0.5, 0.0]])
    yield "lattice", qlat, _types(rng, len(qlat), 3), lat, _types(rng, len(lat), 3)
    base = rng.random((300, 2)) * 50
    dup = np.vstack([base, base[rng.permutation(300)]])
    qd = np.vstack([rng.random((400, 2)) * 50, base[:200]])
    yield "duplicates", qd, _types(rng, len(qd), 4), dup, _types(rng, len(dup), 4)
    t = rng.random((300, 2)) * 10
    qf = np.vstack([rng.random((60, 2)) * 10 + [1e5, 0.0], rng.random((60, 2)) * 10 - [0.0, 3e4], rng.random((60, 2)) * 40 - 15,
                    [[-1e6, -1e6], [1e6, 1e6], [5.0, -2e5]]])
    yield "far", qf, _types(rng, len(qf), 4), t, _types(rng, len(t), 4)
    tc = np.vstack([rng.random((600, 2)) * 1.0, rng.random((200, 2)) * 200 - 100])
    qc = np.vstack([rng.random((300, 2)) * 1.0, rng.random((200, 2)) * 200 - 100])
    yield "cluster", qc, _types(rng, len(qc), 5), tc, _types(rng, len(tc), 5)
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_tongue.npz"))
    names = [c for c in ("Endothelial cells", "Epithelial cells", "Fibroblasts", "Lymphoid cells", "Myeloid cells")]
    yield ("tongue", np.column_stack([g["mer__transformed_x"], g["mer__transformed_y"]]), _argmax_type(g, "mer", names),
           np.column_stack([g["prot__transformed_x"], g["prot__transformed_y"]]), _argmax_type(g, "prot", names))
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_heart.npz"))
    names = [str(c)[:-len("_percentage")] for c in g["ref_columns"] if str(c).endswith("_percentage")]
    yield ("heart", np.column_stack([g["query__spot_x"], g["query__spot_y"]]), _argmax_type(g, "query", names, "_percentage"),
           np.column_stack([g["ref__spot_x"], g["ref__spot_y"]]), _argmax_type(g, "ref", names, "_percentage"))
    t = rng.random((800, 2)) * 60
    yield "same_coords", t.copy(), _types(rng, 800, 4), t, _types(rng, 800, 4)
    lab_t = np.array([1, True, None, float("nan"), "1", 2.0, "a", 0], dtype=object)
    lab_q = np.array([1.0, 1, None, float("nan"), "1", 1, True, 2, "a", False, None, 0.0], dtype=object)
    tl = np.column_stack([np.arange(8.0), np.zeros(8)])
    ql = np.column_stack([[0, 1, 2, 3, 0, 4, 0, 5, 6, 7, 3, 7.2], np.full(12, 0.1)])
    yield "labels", ql, lab_q, tl, lab_t
    yield "empty", np.zeros((0, 2)), np.zeros(0, dtype=object), rng.random((50, 2)), _types(rng, 50)
    yield "knn_gt_n", rng.random((5, 2)), _types(rng, 5), rng.random((4, 2)), _types(rng, 4)


def frames(q_xy, q_lab, t_xy, t_lab):
    import pandas as pd

    q = pd.DataFrame({"X": q_xy[:, 0], "Y": q_xy[:, 1]})
    q["cell_type"] = pd.Series(q_lab, dtype=object)
    t = pd.DataFrame({"X": t_xy[:, 0], "Y": t_xy[:, 1]})
    t["cell_type"] = pd.Series(t_lab, dtype=object)
    return q, t


def main():
    ref = load_reference(with_run_same=False)
    out = {}
    names = []
    for name, q_xy, q_lab, t_xy, t_lab in cases():
        names.append(name)
        out[f"{name}_q_xy"], out[f"{name}_t_xy"] = np.asarray(q_xy, np.float64), np.asarray(t_xy, np.float64)
        out[f"{name}_q_kind"], out[f"{name}_q_text"] = encode_labels(q_lab)
        out[f"{name}_t_kind"], out[f"{name}_t_text"] = encode_labels(t_lab)
        q, t = frames(q_xy, decode_labels(out[f"{name}_q_kind"], out[f"{name}_q_text"]), t_xy,
                      decode_labels(out[f"{name}_t_kind"], out[f"{name}_t_text"]))
        ks = [k for k in KS if k <= max(len(t_xy), 1)] if name != "knn_gt_n" else [5]
        out[f"{name}_ks"] = np.array(ks, np.int64)
        for k in ks:
            try:
                df, score = ref.eval_utils.check_alignment(q, t, "X", "Y", kNN=k)
            except Exception as e:   # noqa: BLE001 -- the exception's type is what is recorded
                out[f"{name}_k{k}_error"] = np.array(type(e).__name__)
                print(f"[{name} k={k}] {type(e).__name__}")
                continue
            col = df[f"_{k}NN_match"]
            out[f"{name}_k{k}_match"] = col.to_numpy().astype(np.uint8)
            out[f"{name}_k{k}_match_dtype"] = np.array(str(col.dtype))
            out[f"{name}_k{k}_score"] = np.array([score], np.float64)
            if k == 1:
                out[f"{name}_k1_ctype_kind"], out[f"{name}_k1_ctype_text"] = encode_labels(df["_1NN_match_ctype"].to_numpy())
            print(f"[{name} k={k}] {len(q)} x {len(t)}: score {score}")
    out["cases"] = np.array(names)
    out["tie_families"] = np.array(TIE_FAMILIES)
    path = os.path.join(OUT, "check_alignment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
