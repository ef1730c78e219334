"""The transport start's problem (optim_params["hip_incumbent"] = "transport", csrc/assign.hip) stated on the host, three ways that share
no code with ops.sparse_transport_host: its objective, an exhaustive enumeration for tiny problems, and scipy's dense
linear_sum_assignment on the expanded matrix.

The problem: every aligned row takes one of its pairs or its no-match column; reference j takes at most limit[j] rows; the cost is
pair costs + no-match costs + penalty_coeff * sum_j max(0, count_j - 1) -- the model of src/same.py:1191-1196 without its triangle
term, under the constraints of src/helpers.py:102-161."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

BIG_M = 1e9


def objective(mp, pairs, costs, unmatched, n_r, pc):
    """the cost of a matching (pair index per row, -1 = unmatched), counted reference by reference"""
    total, count = 0.0, np.zeros(n_r, np.int64)
    for i, p in enumerate(np.asarray(mp).tolist()):
        if p < 0:
            total += float(unmatched[i])
        else:
            assert int(pairs[p, 0]) == i, "a row's pair is its own"
            total += float(costs[p])
            count[pairs[p, 1]] += 1
    return total + float(pc) * float(np.maximum(count - 1, 0).sum()), count


def within_limits(mp, pairs, n_a, n_r, limit):
    """a row's pair is its own, and no reference holds more rows than its limit -> the counts"""
    mp = np.asarray(mp)
    m = mp >= 0
    assert len(mp) == n_a and np.all(mp[m] < len(pairs))
    assert np.array_equal(pairs[mp[m], 0], np.flatnonzero(m))
    count = np.bincount(pairs[mp[m], 1], minlength=n_r)
    assert np.all(count <= np.asarray(limit)), "a reference holds more rows than its limit"
    return count


def brute_force(pairs, costs, unmatched, n_a, n_r, limit, pc):
    """the minimum over EVERY feasible matching (tiny problems only) -> (objective, one matching that reaches it)"""
    options = [[-1] + [p for p in range(len(pairs)) if pairs[p, 0] == i] for i in range(n_a)]
    best, best_mp = np.inf, None
    for mp in itertools.product(*options):
        obj, count = objective(mp, pairs, costs, unmatched, n_r, pc)
        if np.all(count <= limit) and obj < best:
            best, best_mp = obj, np.array(mp, np.int32)
    return best, best_mp


def dense_transport(pairs, costs, unmatched, n_a, n_r, limit, pc):
    """linear_sum_assignment on the expanded dense matrix: reference j as min(limit[j], n_a) columns, the columns after its first
    penalty_coeff dearer, a no-match column per row, big-M elsewhere -> pair index per row, -1 = unmatched"""
    copies = np.minimum(np.asarray(limit, np.int64), n_a)
    first = np.concatenate(([0], np.cumsum(copies)))
    n_cols = int(first[-1])
    mat = np.full((n_a, n_cols + n_a), BIG_M)
    for p, (i, j) in enumerate(pairs.tolist()):
        for t in range(int(copies[j])):
            mat[i, first[j] + t] = costs[p] + (pc if t else 0.0)
    mat[np.arange(n_a), n_cols + np.arange(n_a)] = unmatched
    rows, cols = linear_sum_assignment(mat)
    col_ref = np.repeat(np.arange(n_r), copies)
    lookup = {(int(i), int(j)): p for p, (i, j) in enumerate(pairs.tolist())}
    out = np.full(n_a, -1, np.int32)
    for i, c in zip(rows.tolist(), cols.tolist()):
        if c < n_cols and mat[i, c] < BIG_M * 0.5:
            out[i] = lookup[(i, int(col_ref[c]))]
    return out


def random_limits(rng, n_r, wide=0.05):
    """limits from 1..4, a few of 1001 (the bound of p_j + 1)"""
    limit = rng.integers(1, 5, n_r).astype(np.int32)
    limit[rng.random(n_r) < wide] = 1001
    return limit
