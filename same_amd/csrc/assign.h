// assign.h -- the optimal-assignment incumbent (assign.hip) as the window path (window_finish.hip) and the host-buffer entry point
// (same_sparse_assign) launch it.
#pragma once
#include "window_internal.h"

namespace asg {

constexpr int32_t MAX_LIMIT = 1001;       // count_j <= 1 + the upper bound 1000 of p_j (src/same.py:1117)

// one problem: rows 0..n-1 with their pairs a contiguous run prow[i] .. prow[i+1] of the pair list (column = pairs[2 p + 1] in
// 0..n_r-1, each column at most once per row), the row's no-match column n_r + i
struct AssignArgs {
    const int32_t *prow = nullptr, *pairs = nullptr;
    const double *cost = nullptr;
    const double *unm = nullptr;          // no-match cost per row, or null: penalty * size[i]
    const double *size = nullptr;
    double penalty = 0.0;
    int64_t n = 0, n_r = 0, max_pops = 0;
    uint8_t *alive = nullptr;             // or null: the greedy rule's pair flags, cleared (match_rows_kernel reads them)
    int32_t *match_pair = nullptr;        // [n] out: the pair of each row, -1 = its no-match column
    unsigned long long *res = nullptr;    // [4] ([5]: transport) out: searches, columns finalized, flags (!= 0: not certified), objective (fp64 bits)
    // the work arrays (lay): per column (n_r + n) ...
    int32_t *col_row = nullptr, *pred = nullptr, *mark = nullptr, *list = nullptr, *done = nullptr, *ppair = nullptr;
    double *v = nullptr, *d = nullptr, *ec = nullptr;
    // ... per row
    int32_t *row_col = nullptr;
    double *rc = nullptr;
    // the transport form (set before lay): reference j takes up to limit[j] rows (1 .. 1001), each after its first priced pc; the
    // shared columns n_r + n + j (capacity limit[j] - 1) extend the per-column arrays; res gains a fifth word, sum_j max(0, count_j - 1)
    bool transport = false;
    double pc = 0.0;
    int32_t *limit = nullptr;             // [n_r] the caller's (or refine.hip's limits kernel's) before the launch
    int32_t *cnt = nullptr;               // [n_r] holders of each shared column; its list: col_row = head, then ...
    int32_t *nxt = nullptr, *prv = nullptr;   // ... [n] the links through the rows
};

// the work arrays of `a` (n, n_r set) as the next takes of a buffer's layout (win::Carver: measured, then placed)
void lay(AssignArgs &a, win::Carver &cv);
int64_t default_max_pops(int64_t n, int64_t n_r, int64_t P, bool transport = false);
// the solve and its certificate for up to SAME_LAUNCH_WINDOWS problems of one form: two launches, no wait
int launch(same_ctx *ctx, const AssignArgs *jobs, int n_w);

}  // namespace asg
