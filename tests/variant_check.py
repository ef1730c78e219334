"""A plain host statement of csrc/window_recost.hip (same_window_recost) and the inputs of its tests.  The statement: a staged window's
pair list keeps its rows, pairs and reference numbers, and its costs are `oracle.pair_cost_arrays` over the staged pairs
(tests/caller_check.host_stage) with the VARIANT's moving rows, in the cost type.  tests/test_window_variants_cpu.py checks on these very
inputs, without a GPU, that they hold the shapes the kernel can go wrong at; tests/test_gpu_window_variants.py holds the library against
a window freshly staged from a section made with the variant's matrix.  Not collected by pytest."""
import functools

import numpy as np

import caller_check as C
import knn_prefix_check as K

LDS_MIN_PAIRS = 64 * 64        # a launch group whose largest staged list has this many pairs takes the LDS form (where its block fits)
LDS_BYTES = 65536


def recost(case_xy_m, case_xy_r, types_v, types_r, rows, rows_r, pairs, w, dtype, oracle):
    """the costs of the staged `pairs` ((P, 2) over (kept cell, reference of the window)) priced from `types_v`, the variant's (n, T)
    matrix over the moving SECTION's rows: float64 (P,), float costs widened -- what SAME_WINDOW_COSTS hands out"""
    dt = np.dtype(dtype)
    if len(pairs) == 0:
        return np.zeros(0, np.float64)
    A, R = np.ascontiguousarray(types_v[rows]).astype(dt), np.ascontiguousarray(types_r[rows_r]).astype(dt)
    axy, rxy = case_xy_m[rows].astype(dt), case_xy_r[rows_r].astype(dt)
    return oracle.pair_cost_arrays(A, R, axy, rxy, pairs, w, dtype=dt).astype(np.float64)


def lds_waves(T, itemsize):
    """waves per block of the LDS form for T type columns of `itemsize` bytes (cost.hip's rule); 0: the block does not fit"""
    per_wave = (64 * (T | 1) * itemsize + 64 * 4 + 7) & ~7
    return min(4, LDS_BYTES // per_wave)


def takes_lds(T, itemsize, most_pairs):
    return T >= 2 and lds_waves(T, itemsize) >= 1 and most_pairs >= LDS_MIN_PAIRS


def variants_of(types_m, seed):
    """two variants of a moving section's type matrix: L1 noised (every entry moved, none negative), L2 the rows reversed and the columns
    rolled by one -> (L1, L2), float64 C-contiguous"""
    rng = np.random.default_rng(seed)
    l1 = np.ascontiguousarray(np.abs(types_m * (1.0 + 0.25 * rng.standard_normal(types_m.shape)) + rng.uniform(0.01, 1.0, types_m.shape)))
    l2 = np.ascontiguousarray(np.roll(types_m[::-1], 1, axis=1))
    return l1, l2


# ---- the T family: small sections of their own -------------------------------------------------------------------------------------------
T_VALUES = (1, 2, 3, 4, 20, 63, 64, 65, 200, 300)       # 200: the LDS block fits in float and not in double; 300: in neither
T_ROWS, T_SIDE, T_RADIUS, T_KBIG = 400, 60.0, 12.0, 16


@functools.lru_cache(maxsize=None)
def t_case(T):
    """400 moving points uniform in [0, 60)^2, the reference the points themselves (every row in a box is kept, and at k = 1 a window's pair
    count is its row count exactly), T type columns drawn independently on the two sides"""
    rng = np.random.default_rng(9000 + T)
    xy = rng.uniform(0, T_SIDE, (T_ROWS, 2))
    return C._frozen(dict(mov_xy=xy, ref_xy=xy.copy(), types_m=rng.gamma(0.3, 30.0, (T_ROWS, T)), types_r=rng.gamma(0.3, 30.0, (T_ROWS, T))))


def _box_of_first(xy, m):
    """the box that holds exactly the m points of smallest x"""
    xs = np.sort(xy[:, 0])
    return (-1.0, float((xs[m - 1] + xs[m]) / 2), -1.0, T_SIDE + 1.0)


def t_windows(T):
    """-> [(name, box, k)]: the whole section at k = 16 (enough pairs for the LDS form), windows of exactly 63, 65 and 127 pairs (k = 1:
    fewer than 64; 1 and 63 mod 64), a box beside the data (nothing)"""
    xy = t_case(T)["mov_xy"]
    return [("big", (-1.0, T_SIDE + 1.0, -1.0, T_SIDE + 1.0), T_KBIG), ("63", _box_of_first(xy, 63), 1), ("65", _box_of_first(xy, 65), 1),
            ("127", _box_of_first(xy, 127), 1), ("nothing", (T_SIDE + 10.0, T_SIDE + 20.0, 0.0, 10.0), 1)]


def families(oracle):
    """-> [(tag, case, box, radius, k)]: the T family's windows, then the base / tie / contention / edge families of
    tests/knn_prefix_check.py at the k they are staged at"""
    out = [(f"T{T}/{name}", t_case(T), box, T_RADIUS, k) for T in T_VALUES for name, box, k in t_windows(T)]
    return out + [(f"K/{tag}", case, box, radius, k) for tag, case, box, radius, k in K.families(oracle)]


def family(oracle, tag):
    return next(f for f in families(oracle) if f[0] == tag)


def tags():
    """the families' tags without an oracle (the parametrisation of the GPU tests)"""
    return [f"T{T}/{name}" for T in T_VALUES for name in ("big", "63", "65", "127", "nothing")] + \
           [f"K/{t}" for t in ("base/whole", "base/interior", "base/sliver", "base/beside", "base/no triangle", "base/empty", "tie",
                               "contention", "edge/255", "edge/256", "edge/257", "edge/16385")]
