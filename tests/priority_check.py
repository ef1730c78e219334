"""A plain host statement of the DEVICE rule of the cell-type-priority prune (csrc/window_priority.hip), for the tests: the per-row
stable rank by d = sqrt(dx*dx + dy*dy), then the lowest-row claim of each row's nearest reference.  Not collected by pytest."""
import numpy as np


def device_rule(pairs, axy, rxy, code_m, code_r):
    """pairs (P, 2): (aligned row, reference row), rows ascending, any order inside a row (the staged order).  code_m / code_r: joint label
    codes per aligned / reference row (eval_utils._label_codes).  -> (filtered pairs (n, 2) int64, rows that kept one pair, rows that
    kept all): what same_amd.knn.priority_filter gives for labels with these codes."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = len(pairs)
    if P == 0:
        return pairs, 0, 0
    assert np.all(pairs[1:, 0] >= pairs[:-1, 0])
    rows, start = np.unique(pairs[:, 0], return_index=True)
    prow = np.append(start, P)
    dx, dy = axy[pairs[:, 0], 0] - rxy[pairs[:, 1], 0], axy[pairs[:, 0], 1] - rxy[pairs[:, 1], 1]
    d = np.sqrt(dx * dx + dy * dy)
    rank = np.empty(P, np.int64)
    for a in range(len(rows)):                       # 1. the stable rank of every pair in its row: #{q : d_q < d_p or (d_q == d_p and q < p)}
        dr, q = d[prow[a]:prow[a + 1]], np.arange(prow[a + 1] - prow[a])
        rank[prow[a]:prow[a + 1]] = ((dr[None, :] < dr[:, None]) | ((dr[None, :] == dr[:, None]) & (q[None, :] < q[:, None]))).sum(axis=1)
    claim = np.full(len(rxy), np.iinfo(np.int32).max, np.int64)
    near = np.empty(len(rows), np.int64)
    for a in range(len(rows)):                       # 2. the claims: min over the bidding rows
        p = prow[a] + int(np.flatnonzero(rank[prow[a]:prow[a + 1]] == 0)[0])
        near[a] = j = pairs[p, 1]
        cm, cr = code_m[rows[a]], code_r[j]
        if cm == cr and cm >= 0:
            claim[j] = min(claim[j], a)
    wins = claim[near] == np.arange(len(rows))
    keep = np.where(wins, 1, np.diff(prow))          # 3. the compaction
    new_prow = np.concatenate(([0], np.cumsum(keep)))
    out = np.full((int(new_prow[-1]), 2), -1, np.int64)
    for a in range(len(rows)):
        for p in range(prow[a], prow[a + 1]):
            if not wins[a] or rank[p] == 0:
                out[new_prow[a] + (0 if wins[a] else rank[p])] = pairs[p]
    assert (out >= 0).all()
    return out, int(wins.sum()), int(len(rows) - wins.sum())
