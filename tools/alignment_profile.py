"""Time eval_utils.check_alignment at 1M x 1M (uniform random query and template, 12 labels), kNN 1 and 8: the whole call (host
label coding, upload, grid build, kernel, host resolution of the rows in doubt, column assembly) and its row counts.  For the
kernel's own time run it once more under `rocprofv3 --kernel-trace --stats -- python tools/alignment_profile.py --reps 1` (a run of
its own).  Prints one JSON line per kNN."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(n, seed=3):
    rng = np.random.default_rng(seed)
    types = np.array([f"type_{i}" for i in range(12)], dtype=object)
    q = pd.DataFrame({"X": rng.random(n) * 5000, "Y": rng.random(n) * 5000, "cell_type": types[rng.integers(0, 12, n)]})
    t = pd.DataFrame({"X": rng.random(n) * 5000, "Y": rng.random(n) * 5000, "cell_type": types[rng.integers(0, 12, n)]})
    return q, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--knn", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    from same_amd import _lib
    from same_amd.eval_utils import _label_codes, check_alignment

    q, t = frames(a.n)
    ctx = _lib.default_context()
    for k in a.knn:
        check_alignment(q, t, "X", "Y", kNN=k, ctx=ctx)            # warm-up: scratch growth, code load
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, score, st = check_alignment(q, t, "X", "Y", kNN=k, ctx=ctx, return_stats=True)
            walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        _label_codes(q["cell_type"].to_numpy(), t["cell_type"].to_numpy())
        codes_s = time.perf_counter() - t0
        print(json.dumps({"n_query": a.n, "n_template": a.n, "kNN": k, "wall_s_median": float(np.median(walls)), "wall_s_min": min(walls),
                          "label_coding_s": codes_s, "score": float(score), **st}), flush=True)


if __name__ == "__main__":
    main()
