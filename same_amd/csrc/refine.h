// refine.h -- the local search on the window's lazy-model objective (refine.hip) as the window path (window_finish.hip) and the
// host-buffer entry point (same_refine_matching) launch it.
#pragma once
#include "window_internal.h"

namespace rfn {

// the search's control words (on the device; the window path keeps them in its finish block, so they come back with it):
// productive rounds, moves applied, settled (a round found no winner), winners of the round in progress, blocks of the apply launch
// done, objective at the start and now (fp64 bits), sum_j max(0, count_j - 1) of the matching the objective was last taken of
enum { RC_ROUNDS = 0, RC_MOVES = 1, RC_SETTLED = 2, RC_WIN = 3, RC_DONE = 4, RC_OBJ0 = 5, RC_OBJ = 6, RC_EXTRA = 7, RC_COUNT = 8 };
constexpr int32_t MAX_LIMIT = 1001;       // count_j <= 1 + the upper bound 1000 of p_j (src/same.py:1117)

constexpr int FIRST_ROUNDS = 4;          // rounds enqueued before the first look (cfg 5: at most 2 productive + the settling one)
constexpr double EPS = 0x1p-40;          // a move improves when delta < -EPS * scale (the assignment certificate's bound)

// a cell's proposal: key (~0 = none), its new pair (-1 = unmatched), the swap partner (-1 = none), the partner's new pair and the
// cell's pair when it proposed (-1 = unmatched)
struct Prop {
    unsigned long long key;
    int32_t p_i, k, p_k, p_o;
};

// one problem: cells 0..n-1 with their pairs a contiguous run prow[i] .. prow[i+1] (reference = pairs[2 p + 1] in 0..n_r-1, each
// reference at most once per cell); the kept triangles over the cells; the start matching (pair per cell, -1 = none), which holds
// every reference at most its limit times.  Limits: limit_in[n_r] (host form), or from the reference section's sizes (the window
// path: rsize non-null, the model's rule src/helpers.py:102-161 over the references the pairs name), or 1 each (one-to-one).
struct RefineArgs {
    const int32_t *prow = nullptr, *pairs = nullptr;
    const double *cost = nullptr;         // per pair
    const double *unm = nullptr;          // no-match cost per cell, or null: penalty * size[i]
    const double *size = nullptr;         // per cell (triangle weights)
    double penalty = 0.0, dp = 0.0;       // no-match penalty (unm null), delaunay_penalty
    const double *axy = nullptr;          // [n][2]
    const double *ref_xy = nullptr;       // reference XY, row ref_row[p] of pair p (ref_row null: row pairs[2 p + 1])
    const int32_t *ref_row = nullptr;
    const int32_t *tris = nullptr;        // [cap_tr][3]
    const unsigned long long *dTr = nullptr;   // or null: cap_tr triangles
    int64_t n = 0, n_r = 0, cap_tr = 0, cap = 0;
    const int32_t *start = nullptr;       // [n]
    unsigned long long *ctrl = nullptr;   // [RC_COUNT], zeroed by the setup
    double pc = 0.0;                      // penalty_coeff: the price of every match of a reference after its first
    const int32_t *limit_in = nullptr;    // [n_r] matches each reference may take (1 .. MAX_LIMIT), or null: see above
    const double *rsize = nullptr;        // the window path's capacity: reference section sizes, at ref_rows[j] for reference j and
    const int32_t *ref_rows = nullptr;    // at ref_row[p] for pair p's; P pairs
    int64_t P = 0, max_matches = 1, multiplier = 0;   // multiplier 0 = None (the frame's largest size)
    const int32_t *lim_row = nullptr;     // the frame the limits are read over when it is not the pair list's own: lim_P reference rows
    int64_t lim_P = 0;                    // (a window whose unconstrained nodes went: the pair list as staged)
    // the work arrays (lay)
    int32_t *match = nullptr;             // [n] the search's matching (its result)
    int32_t *count = nullptr;             // [n_r] cells holding each reference
    long long *hsum = nullptr;            // [n_r] sum of their ids: THE holder where count is 1 (the only swap partners)
    int32_t *limit = nullptr;             // [n_r]
    int32_t *tsort = nullptr;             // [cap_tr][3] corners sorted ascending
    int8_t *tsign = nullptr;              // [cap_tr] source sign over the sorted corners
    double *tw = nullptr;                 // [cap_tr] weight: size sum over the sorted corners
    uint8_t *q = nullptr;                 // [cap_tr] q_t under the current matching (refreshed before every round)
    unsigned *deg = nullptr, *cur = nullptr;   // [n] incident triangles, fill cursor
    int32_t *off = nullptr;               // [n + 1] incidence offsets
    int32_t *inc = nullptr;               // [3 cap_tr] incident triangles per cell, by sorted corners
    unsigned long long *st = nullptr;     // scan words of the offsets
    unsigned long long *slot[2] = {nullptr, nullptr};   // [n + n_r] claim slots (cells, then references), by round parity
    Prop *best = nullptr;                 // [n]
};

// the work arrays of `a` (n, n_r, cap_tr set) as the next takes of a buffer's layout (win::Carver: measured, then placed)
void lay(RefineArgs &a, win::Carver &cv);
// the search for up to SAME_LAUNCH_WINDOWS problems, enqueue only.  setup: the matching from `start`, the incidence lists, the
// objective at the start; rounds: `rounds` more rounds (each returns at once once its window settled or reached its cap), then the
// objective now
int launch_setup(same_ctx *ctx, const RefineArgs *jobs, int n_w);
// the window path's limits alone (rsize, ref_row, ref_rows, P, n_r, max_matches, multiplier -> limit[n_r]; nothing else of a job is
// read): for the transport start, which runs before the search's setup (assign.hip)
int launch_limits(same_ctx *ctx, const RefineArgs *jobs, int n_w);
int launch_rounds(same_ctx *ctx, const RefineArgs *jobs, int n_w, int rounds);

}  // namespace rfn
