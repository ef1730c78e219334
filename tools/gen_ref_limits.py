"""Record tests/golden/ref_match_limits.npz by RUNNING THE REFERENCE (build container only; not part of `gen_golden.py all`).

Run:  python3 -B tools/gen_ref_limits.py

The reference's add_basic_constraints_optimized (src/helpers.py:102-161) runs as-is against the recording stand-in for the solver API
(tests/fake_gurobipy.py) on small post-KNN frames -- with and without reference metacells, sizes integer and not -- for
max_matches 1 / 3 and ref_metacell_match_multiplier None / 1 / 2.  The fixture holds each frame's reference sizes, the pairs, and the
right-hand side of every `max_matches_{j}` constraint it emitted (j, limit): what same_amd.api.ref_match_limits must give.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_gurobipy as fg  # noqa: E402

fg.install()
from ref_loader import load_reference  # noqa: E402

OUT = os.environ.get("SAME_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
MAX_MATCHES = (1, 3)
MULTIPLIERS = (None, 1, 2)


def frames():
    """(name, ref sizes or None for a frame without a size column, pairs) of a few post-KNN frames"""
    import pandas as pd  # noqa: F401

    rng = np.random.default_rng(7)
    n_a, n_r = 30, 20
    pairs = np.stack([np.repeat(np.arange(n_a), 3), rng.integers(0, n_r, 3 * n_a)], 1)
    pairs = np.unique(pairs, axis=0)
    yield "single", np.ones(n_r), pairs                        # every size 1: no metacells
    yield "nosize", None, pairs                                # no size column
    meta = np.ones(n_r)
    meta[::3] = [3, 5, 2, 4, 3, 6, 2][: len(meta[::3])]
    yield "meta", meta, pairs                                  # some metacells, the largest 6
    yield "allmeta", rng.integers(2, 5, n_r).astype(np.float64), pairs     # both sides collapsed: every reference a metacell
    frac = np.ones(n_r)
    frac[1::4] = 2.5                                           # a non-integer largest size: int() of it
    yield "frac", frac, pairs


def main():
    import pandas as pd

    ref = load_reference(with_run_same=False)
    ref.helpers.GRB = fg.GRB
    ref.helpers.quicksum = fg.quicksum
    out = {}
    names = []
    for name, sizes, pairs in frames():
        n_r = int(pairs[:, 1].max()) + 1
        n_a = int(pairs[:, 0].max()) + 1
        r_df = pd.DataFrame({"X": np.arange(n_r, dtype=np.float64), "Y": np.zeros(n_r)})
        if sizes is not None:
            r_df["size"] = sizes[:n_r]
        out[f"{name}_has_size"] = np.array(sizes is not None)
        out[f"{name}_size"] = np.asarray(sizes[:n_r] if sizes is not None else np.ones(n_r), dtype=np.float64)
        out[f"{name}_pairs"] = pairs.astype(np.int64)
        names.append(name)
        for mm in MAX_MATCHES:
            for mult in MULTIPLIERS:
                model = fg.Model("limits")
                x = model.addVars(len(pairs), vtype=fg.GRB.BINARY, lb=0, ub=1, name="x")
                pv = model.addVars(n_r, vtype=fg.GRB.CONTINUOUS, lb=0, ub=1000, name="penalty")
                nv = model.addVars(n_a, vtype=fg.GRB.CONTINUOUS, lb=0, ub=1, name="no_match")
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    ref.helpers.add_basic_constraints_optimized(model, [tuple(map(int, p)) for p in pairs], n_r, n_a, mm, x, pv, nv,
                                                                aligned_df=None, ref_df=r_df, ref_metacell_match_multiplier=mult)
                rows = [(int(cn[len("max_matches_"):]), -float(c.expr.const)) for cn, c in model.constrs
                        if cn and cn.startswith("max_matches_")]
                out[f"{name}_mm{mm}_mult{mult}"] = np.array(rows, dtype=np.float64)
    out["frames"] = np.array(names)
    out["max_matches"] = np.array(MAX_MATCHES)
    out["multipliers"] = np.array(["None" if m is None else str(m) for m in MULTIPLIERS])
    path = os.path.join(OUT, "ref_match_limits.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} frames x {len(MAX_MATCHES) * len(MULTIPLIERS)} settings")


if __name__ == "__main__":
    main()
