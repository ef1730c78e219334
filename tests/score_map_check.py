"""The host statement of same_merge_acc_score_map (csrc/window_score_map.hip) and the input families its library-level tests add to
tests/score_check.py's.

`host_marks` is the call in plain numpy: `score_check.host_counts` for the eight counts and the node counters (imported as it is), the
node rule per moving row, the truth comparison, and the reference's rank rule (examples/luad/reproduce_figures.ipynb cell 13: is the
moving cell's label among the k largest type columns of the reference cell -- stated as the two counts include/same_hip.h states, how many
OTHER columns hold a value > and >= the label's, in float64; a NaN anywhere in the row ranks nothing).  It imports nothing that ends in
libsame_hip.

The families make what the product route never hands the call: moving sections cut to the last matched row and grown past the wave and
block edges, truth arrays that are all unknown, all right, all wrong, type rows with exact ties, signed zeros, infinities and NaN, more
columns than a rank byte counts, labels that name no column.  tests/test_score_map_check_cpu.py checks, without a GPU, that each has the
property it was made for; tests/test_gpu_score_map_library.py drives the library against `host_marks` on them.  Not collected by pytest."""
import numpy as np

import score_check as S

# same_cell_mark, as include/same_hip.h lays it out
MARK = np.dtype([("ref_row", np.int32), ("node_tri", np.uint32), ("node_flip", np.uint32), ("flags", np.uint8), ("rank_strict", np.uint8),
                 ("rank_weak", np.uint8), ("reserved", np.uint8)])
MATCHED, TYPE_MATCH, CONSIDERED, VIOLATING, TRUTH_KNOWN, ON_TRUTH, RANKED = 1, 2, 4, 8, 16, 32, 64
UNRANKED, RANK_TOP = 255, 254
SIZE_STEPS = (0, 1, 63, 64, 65, 257, 5000)         # rows beyond the smallest moving section that holds the final rows
TYPE_COUNTS = (1, 2, 20, 300)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def host_ranks(label_col, row):
    """(strict, weak) of type column `label_col` in the float64 type row `row`, or None: the label names no column, a NaN in the row"""
    row = np.asarray(row, np.float64)
    if label_col < 0 or label_col >= len(row) or np.isnan(row).any():
        return None
    v = row[label_col]
    others = np.delete(row, label_col)
    return int(np.count_nonzero(others > v)), int(np.count_nonzero(others >= v))


def host_marks(a_row, r_row, mov_xy, ref_xy, code_m, code_r, tris, truth=None, col_of_label=None, ref_types=None, ignore_same=True,
               node_local=False, majority_threshold=0.5, min_flips=1):
    """-> (marks: MARK per moving row; the ten counts of include/same_hip.h as int64; what one call adds to the tally, int64 (rows, 4)).
    `truth`: int per moving row, -1 unknown (None: all unknown); `col_of_label`: the type column per label code (None: no ranks);
    `ref_types`: float64 (reference rows, T)."""
    counts8, node_tri, node_flip = S.host_counts(a_row, r_row, mov_xy, ref_xy, code_m, code_r, tris, ignore_same, node_local,
                                                 majority_threshold, min_flips)
    a_row, r_row = np.asarray(a_row, np.int64), np.asarray(r_row, np.int64)
    code_m, code_r = np.asarray(code_m, np.int64), np.asarray(code_r, np.int64)
    n = len(code_m)
    truth = np.full(n, -1, np.int64) if truth is None else np.asarray(truth, np.int64)
    assert len(truth) == n == len(np.asarray(mov_xy).reshape(-1, 2))
    marks = np.zeros(n, MARK)
    marks["ref_row"] = -1
    marks["rank_strict"] = marks["rank_weak"] = UNRANKED
    marks["flags"] = np.where(truth >= 0, TRUTH_KNOWN, 0)
    violating = S.node_rule(node_tri[a_row], node_flip[a_row], node_local, majority_threshold, min_flips)
    tally = np.zeros((n, 4), np.int64)
    for q, (a, r) in enumerate(zip(a_row.tolist(), r_row.tolist())):
        m = marks[a]
        flags = int(m["flags"]) | MATCHED
        agree = code_m[a] >= 0 and code_m[a] == code_r[r]
        flags |= TYPE_MATCH if agree else 0
        flags |= CONSIDERED if node_tri[a] > 0 else 0
        flags |= VIOLATING if violating[q] else 0
        flags |= ON_TRUTH if truth[a] == r else 0
        m["ref_row"], m["node_tri"], m["node_flip"] = r, node_tri[a], node_flip[a]
        if col_of_label is not None and 0 <= code_m[a] < len(col_of_label):
            got = host_ranks(int(col_of_label[code_m[a]]), ref_types[r])
            if got is not None:
                flags |= RANKED
                m["rank_strict"], m["rank_weak"] = min(got[0], RANK_TOP), min(got[1], RANK_TOP)
        m["flags"] = flags
        tally[a] = (1, agree, violating[q], truth[a] == r)
    counts = np.zeros(10, np.int64)
    counts[:8] = counts8
    counts[7] = np.count_nonzero(violating)             # (host_counts leaves it 0 without a triangle; so does the node rule)
    counts[8] = np.count_nonzero(truth[a_row] >= 0)
    counts[9] = np.count_nonzero(truth[a_row] == r_row)
    return marks, counts, tally


# ---- the families ------------------------------------------------------------------------------------------------------------------------
def smallest_rows(job):
    """rows of the smallest moving section that holds the final rows"""
    return int(np.max(job.a_row)) + 1


def resized(inp, job, rows, seed=21):
    """`inp` (score_check.Inputs) with a moving section of `rows` rows: cut -- the triangles that name a row beyond it dropped -- or grown
    by rows no final row names, scattered over the section's extent under codes 0 .. 2"""
    assert rows >= smallest_rows(job)
    n = len(inp.mov_xy)
    if rows <= n:
        tris = None if inp.tris is None else inp.tris[(inp.tris < rows).all(axis=1)]
        return inp._replace(mov_xy=inp.mov_xy[:rows].copy(), code_m=inp.code_m[:rows].copy(), tris=tris)
    rng = np.random.default_rng(seed)
    lo, hi = np.nanmin(inp.mov_xy[np.isfinite(inp.mov_xy).all(axis=1)]), np.nanmax(inp.mov_xy[np.isfinite(inp.mov_xy).all(axis=1)])
    return inp._replace(mov_xy=np.vstack((inp.mov_xy, rng.uniform(lo, hi, (rows - n, 2)))),
                        code_m=np.concatenate((inp.code_m, rng.integers(0, 3, rows - n).astype(np.int32))))


def sizes(job):
    """[(name, Inputs)]: score_check's own inputs over moving sections of the smallest size and that size plus SIZE_STEPS"""
    base, least = S.own(job), smallest_rows(job)
    return [(f"smallest + {k}", resized(base, job, least + k)) for k in SIZE_STEPS]


def truths(job, n_mov, n_ref):
    """[(name, int32 truth per moving row)]: all unknown; the match itself where there is one and row 0 elsewhere (known on unmatched
    rows too); the match shifted by one (every known truth is wrong); the last reference row everywhere"""
    match = np.zeros(n_mov, np.int64)
    match[job.a_row] = job.r_row
    shifted = np.full(n_mov, -1, np.int64)
    shifted[job.a_row] = (job.r_row.astype(np.int64) + 1) % n_ref
    return [("all unknown", np.full(n_mov, -1, np.int32)), ("the match", match.astype(np.int32)), ("shifted by one", shifted.astype(np.int32)),
            ("the last row", np.full(n_mov, n_ref - 1, np.int32))]


def type_rows(n_ref, T, seed=22):
    """float64 (n_ref, T) type rows in blocks of eight rows: 0 random; 1 every column equal (all ties: strict 0, weak T - 1); 2 values
    from {0.25, 0.5} (ties with strict < weak); 3 signed zeros alone; 4 +inf in some columns; 5 -inf in some; 6 a NaN somewhere;
    7 descending 1, 1/2, 1/3 ... (column c has strict rank c: past 254 for T = 300)"""
    rng = np.random.default_rng(seed)
    rows = rng.random((n_ref, T))
    kind = np.arange(n_ref) % 8
    rows[kind == 1] = 0.125
    rows[kind == 2] = rng.choice([0.25, 0.5], (int((kind == 2).sum()), T))
    rows[kind == 3] = rng.choice([0.0, -0.0], (int((kind == 3).sum()), T))
    for k, value in ((4, np.inf), (5, -np.inf), (6, np.nan)):
        at = np.flatnonzero(kind == k)
        hit = rng.random((len(at), T)) < max(0.3, 1.0 / T)
        hit[np.arange(len(at)), rng.integers(0, T, len(at))] = True
        block = rows[at]
        block[hit] = value
        rows[at] = block
    rows[kind == 7] = 1.0 / np.arange(1, T + 1)
    return rows


def label_columns(n_labels, T, seed=23):
    """int32 column per label code: label 0 names column T - 1, the last label names none, the rest random columns or none"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(-1, T, n_labels).astype(np.int32)
    cols[0], cols[-1] = T - 1, -1
    return cols


def golden_eval_study(g):
    """tests/golden/eval_tri.npz (test_oracle_golden.eval_inputs' arrays) as a result table over two frames -> (table, ref, moving,
    triangulation, id column, per table row its row of the moving frame).  The moving frame carries the golden's ids and XY, each cell
    the label of the LAST table row that names it (the reference's dicts keep that one); the table's mapped XY are the golden's; the
    reference frame only lends its ids."""
    import pandas as pd

    cid = "node"
    ids, o_id = np.asarray(g["ids"]), np.asarray(g["o_id"])
    rows = pd.Index(ids).get_indexer(o_id)
    assert (rows >= 0).all()
    labels = np.full(len(ids), "unmatched", dtype=object)
    labels[rows] = np.asarray(g["o_type"]).astype(object)            # (a later row overwrites an earlier one)
    moving = pd.DataFrame({"X": g["mxy"][:, 0], "Y": g["mxy"][:, 1], "cell_type": labels, cid: ids})
    n_ref = int(np.max(g["o_ref"])) + 1
    ref = pd.DataFrame({"X": np.zeros(n_ref), "Y": np.zeros(n_ref), "cell_type": np.full(n_ref, "c1", dtype=object), cid: np.arange(n_ref)})
    table = pd.DataFrame({f"Aligned_{cid}": o_id, f"Ref_{cid}": np.asarray(g["o_ref"]), "ref_X": np.asarray(g["o_mx"]), "ref_Y": np.asarray(g["o_my"])})
    return table, ref, moving, np.asarray(g["tri_ids"]), cid, rows
