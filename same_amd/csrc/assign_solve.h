// assign_solve.h -- the small optimal assignment of unpack_metacell_matches(strategy='nearest'), ONE statement for the two kernels that
// solve it: batched_assign_kernel (match.hip: problems from host buffers) and unpack_solve_kernel (window_unpack.hip: one problem per
// final row of a merge, where the rows are).
//
// src/metacell_utils.py:711-761 solves, per metacell match, linear_sum_assignment on cdist(aligned members, ref members) with the ref
// columns tiled ceil(n_a/n_r) times when there are more aligned than ref members.  One lane solves one problem start to finish with its
// work arrays in a private slice of a global buffer; the algorithm is scipy's shortest-augmenting-path solver (Crouse 2016) step for step
// -- same scan order of the remaining columns, same "prefer a free column among equal minima" rule, same dual updates in the same fp64
// operation order -- so ties resolve exactly as in the reference.  rows <= cols always holds here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace assign_solve {

// columns of the (tiled) cost matrix of na aligned against nref reference members (nref > 0)
__host__ __device__ inline int64_t columns(int64_t na, int64_t nref) { return na <= nref ? nref : nref * ((na + nref - 1) / nref); }

// The private work slice of one problem, in 8-byte words:
//   cost[na*nc] u[na] v[nc] spc[nc] | path, row4col, remaining [nc] col4row[na] (int32) | SR[na] SC[nc] (bytes)
__host__ __device__ inline int64_t slice_words(int64_t na, int64_t nc) {
    return na * nc + na + 2 * nc + (3 * nc + na + 1) / 2 + (na + nc + 7) / 8;
}

// The assignment of na > 0 aligned members (XY at axy[2 * i]) to nref > 0 reference members (XY at rxy[2 * j]) in the slice `work`
// (slice_words(na, columns(na, nref)) words): -> col4row[na] inside the slice, the TILED column each aligned member got (% nref: the
// reference member), or null when no finite augmenting path exists (NaN / inf coordinates: scipy raises "cost matrix is infeasible").
__device__ inline const int *solve(int na, int nref, const double *__restrict__ axy, const double *__restrict__ rxy, double *__restrict__ work) {
    const int nc = (int)columns(na, nref);
    double *cost = work, *u = cost + (int64_t)na * nc, *v = u + na, *spc = v + nc;
    int *path = reinterpret_cast<int *>(spc + nc), *row4col = path + nc, *remaining = row4col + nc, *col4row = remaining + nc;
    uint8_t *SR = reinterpret_cast<uint8_t *>(col4row + na), *SC = SR + na;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int i = 0; i < na; ++i) {
        const double ax = axy[2 * i], ay = axy[2 * i + 1];
        for (int j = 0; j < nref; ++j) {
            const double dx = ax - rxy[2 * j], dy = ay - rxy[2 * j + 1];
            const double d = sqrt(dx * dx + dy * dy);  // cdist euclidean: s = dx*dx; s += dy*dy; sqrt (contraction is off)
            for (int jj = j; jj < nc; jj += nref) cost[(int64_t)i * nc + jj] = d;
        }
        u[i] = 0.0;
        col4row[i] = -1;
    }
    for (int j = 0; j < nc; ++j) { v[j] = 0.0; row4col[j] = -1; path[j] = -1; }
    for (int cur = 0; cur < na; ++cur) {
        double min_val = 0.0;
        int num_remaining = nc, sink = -1, i = cur;
        for (int it = 0; it < nc; ++it) { remaining[it] = nc - it - 1; SC[it] = 0; spc[it] = inf; }
        for (int r = 0; r < na; ++r) SR[r] = 0;
        while (sink == -1) {
            int index = -1;
            double lowest = inf;
            SR[i] = 1;
            const double ui = u[i];
            for (int it = 0; it < num_remaining; ++it) {
                const int j = remaining[it];
                const double r = min_val + cost[(int64_t)i * nc + j] - ui - v[j];
                double s = spc[j];
                if (r < s) { path[j] = i; spc[j] = s = r; }
                if (s < lowest || (s == lowest && row4col[j] == -1)) { lowest = s; index = it; }
            }
            min_val = lowest;
            if (index < 0 || min_val == inf) return nullptr;  // NaN / inf coordinates: no finite augmenting path (scipy raises)
            const int j = remaining[index];
            if (row4col[j] == -1) sink = j; else i = row4col[j];
            SC[j] = 1;
            remaining[index] = remaining[--num_remaining];
        }
        u[cur] += min_val;
        for (int r = 0; r < na; ++r)
            if (SR[r] && r != cur) u[r] += min_val - spc[col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (SC[j]) v[j] -= min_val - spc[j];
        int j = sink;
        for (;;) {
            const int r = path[j];
            row4col[j] = r;
            const int t = col4row[r];
            col4row[r] = j;
            j = t;
            if (r == cur) break;
        }
    }
    return col4row;
}

}  // namespace assign_solve
