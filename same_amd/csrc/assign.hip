// assign.hip -- the optimal-assignment incumbent: the reference's init_method="hungarian" MIP start (src/init_helpers.py:135-175)
// solved on its sparse form, with no size cap (the reference's dense n_aligned x (n_ref + n_aligned) matrix gives up above
// init_hungarian_max_n, :136-142).
//
// Rows are the window's kept aligned cells, columns its reference cells plus one PRIVATE no-match column per row (column n_r + i, cost
// no_match_penalty * size[i] -- the fp64 product row_prefer_kernel forms -- or the caller's `unmatched[i]`).  Every row is assigned; a
// row on its no-match column is unmatched (:163-175).  With every no-match cost below big_m / 2 this is the reference's dense big-M
// problem (the caller checks that).
//
// The method: successive shortest augmenting paths with Jonker-Volgenant potentials, one WAVE per window.
//   * dual start: v = 0; every row takes the argmin of its row (a pair beats the no-match column only when strictly cheaper; among pairs
//     the first in pair order).  A reference column wanted by several rows goes to the lowest row; the others start free.  Every
//     matched edge then has reduced cost 0 and every edge a reduced cost >= 0: the state is optimal for the rows it matches.
//   * each free row, in row order, is one Dijkstra search on reduced costs c_rk - v_k - (c_r,m(r) - v_m(r)).  Its own no-match column is
//     always free, so the search is bounded by that edge and stays local.  Columns are finalized by (distance, column index); a free
//     column ends the search (early: a free column reached at the distance just finalized, the lowest such).  The path is flipped and
//     every finalized column's potential moves by d_k - d_sink (<= 0; free columns keep v = 0).
//   * searches run one after another inside the kernel (no host round trip), so the answer depends on nothing but the input.
// A window's work arrays live in global memory (sized by its own counts: no list can outgrow them).  A cap on the columns finalized
// (`max_pops`), an empty frontier (NaN costs) or a failed certificate flags the window; the caller then solves it on the host.
//
// certificate_kernel checks the answer edge by edge, no-match edges included: each row holds a column that holds it back, the row's
// recorded cost is its edge's, every reduced cost is >= -delta and free reference columns have v = 0, where
//   delta = 2^-40 (|c_rk| + |v_k| + |c_r,m(r)| + |v_m(r)|)
// bounds the fp64 rounding the potentials gather over a window's searches (each update is one rounded difference of path sums).
//
// The TRANSPORT form (AssignArgs::limit set; same_sparse_assign_cap, SAME_INCUMBENT_TRANSPORT) is the model without its triangle term:
// reference j may take up to limit[j] rows, each after its first priced `pc` (penalty_coeff) -- a convex surcharge, so splitting j in
// two columns is exact: its SLOT column j (capacity 1, edge cost c_ij: the columns above) and its SHARED column n_r + n + j (capacity
// limit[j] - 1, edge cost c_ij + pc; no column where the limit is 1).  Every unit of the shared column costs pc more than the slot, so
// an optimum fills the slot first and count_j rows on j cost pc * max(0, count_j - 1) whichever tier they sit on.  The shared columns
// come after the no-match columns: the order among the columns above, ties included, is untouched.  In the search a column is a sink
// while it has ROOM (fewer holders than its capacity) and keeps v = 0 that long; a full column, once finalized, relaxes every one of its
// holders (a list per shared column, threaded through the rows: col_row = its head, nxt / prv); the path flip moves one holder from
// each column on the path to the next, so only the sink's count grows.  Same dual start (a second-tier edge is never strictly cheaper
// than its first-tier twin).  With every limit 1 no shared column exists and every step is the one-to-one kernel's: the same match,
// searches and objective bits.  The certificate also checks the lists (every row is reached from the head of the column it holds within
// `limit` steps; a column's list has `cnt` members, all holding it), cnt <= capacity, v = 0 on columns with room and v <= delta on full
// ones (the surcharge a full column earns is never a bonus), and the reduced costs of both tiers.
#include "assign.h"

namespace {

constexpr int WAVE = 64;
constexpr int32_t NO_OWNER = 0x7fffffff;

__device__ __forceinline__ double wave_min(double x) {
    for (int o = WAVE / 2; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ double wave_sum(double x) {
    for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ double no_match_cost(const asg::AssignArgs &a, int64_t i) {
    return a.unm ? a.unm[i] : a.penalty * a.size[i];
}

// CAP: the transport form (shared columns S0 .. S0 + n_r - 1 behind the slot and no-match columns)
template <bool CAP>
__global__ __launch_bounds__(WAVE) void assign_kernel(win::Batch<asg::AssignArgs> b) {
    const asg::AssignArgs &a = b.w[blockIdx.y];
    const int lane = threadIdx.x;
    const int64_t n = a.n, n_r = a.n_r, S0 = n_r + n, C = CAP ? S0 + n_r : S0;
    if (n == 0) {
        if (lane == 0) {
            a.res[0] = a.res[1] = a.res[2] = a.res[3] = 0;
            if (CAP) a.res[4] = 0;
        }
        return;
    }
    const int64_t P = a.prow[n];
    for (int64_t k = lane; k < C; k += WAVE) {
        a.col_row[k] = -1;
        a.v[k] = 0.0;
        a.mark[k] = 0;
        a.pred[k] = NO_OWNER;
    }
    if (CAP)
        for (int64_t j = lane; j < n_r; j += WAVE) a.cnt[j] = 0;
    // a column with room is a sink (a shared column: fewer holders than limit - 1)
    auto room = [&](int32_t k) { return !CAP || k < S0 ? a.col_row[k] < 0 : a.cnt[k - S0] < a.limit[k - S0] - 1; };
    if (a.alive)
        for (int64_t p = lane; p < P; p += WAVE) a.alive[p] = 0;
    __syncthreads();
    // dual start: every row on its row minimum
    for (int64_t i = lane; i < n; i += WAVE) {
        double best = no_match_cost(a, i);
        int64_t bj = n_r + i;
        int32_t bp = -1;
        for (int32_t p = a.prow[i]; p < a.prow[i + 1]; ++p) {
            const double c = a.cost[p];
            if (c < best) {
                best = c;
                bj = a.pairs[2 * (int64_t)p + 1];
                bp = p;
            }
        }
        a.row_col[i] = (int32_t)bj;
        a.rc[i] = best;
        a.match_pair[i] = bp;
        if (bj < n_r) atomicMin(&a.pred[bj], (int32_t)i);
        else a.col_row[bj] = (int32_t)i;
    }
    __syncthreads();
    for (int64_t i = lane; i < n; i += WAVE) {
        const int32_t j = a.row_col[i];
        if (j < n_r) {
            if (a.pred[j] == (int32_t)i) {
                a.col_row[j] = (int32_t)i;
            } else {
                a.row_col[i] = -1;
                a.match_pair[i] = -1;
            }
        }
    }
    __syncthreads();

    unsigned long long searches = 0, pops = 0, flags = 0;
    int32_t stamp = 0;
    const unsigned long long lt_mask = (1ull << lane) - 1;   // lanes below this one
    for (int64_t base = 0; base < n && !flags; base += WAVE) {
        const int64_t i = base + lane;
        unsigned long long todo = __ballot(i < n && a.row_col[i] < 0);
        while (todo && !flags) {
            const int32_t i0 = (int32_t)(base + __builtin_ctzll(todo));
            todo &= todo - 1;
            ++searches;
            ++stamp;
            const int32_t s_front = 2 * stamp, s_done = 2 * stamp + 1;
            int64_t L = 0, F = 0;      // frontier length, columns finalized
            double ub = __builtin_inf(), d_sink = 0.0;
            int32_t sink = -1;
            // relax row r's edges (pairs, then its no-match column) from distance `off`; a free column reached at distance <= `early`
            // (the distance just finalized: nothing can come closer) ends the search at once -- the lowest such column
            auto relax = [&](int32_t r, double off, double early) {
                // (CAP: the row's pairs once more behind its no-match column, as edges to the shared columns)
                const int32_t lo = a.prow[r], deg = a.prow[r + 1] - lo, cnt = CAP ? 2 * deg + 1 : deg + 1;
                int32_t early_k = NO_OWNER;
                for (int32_t e0 = 0; e0 < cnt; e0 += WAVE) {
                    const int32_t e = e0 + lane;
                    bool fresh = false, upd = false;
                    int32_t k = -1;
                    double nd = __builtin_inf();
                    bool edge = e < cnt;
                    int32_t pp = -1;
                    double c = 0.0;
                    if (edge) {
                        if (e < deg) {
                            pp = lo + e;
                            k = a.pairs[2 * (int64_t)pp + 1];
                            c = a.cost[pp];
                        } else if (e == deg) {
                            k = (int32_t)(n_r + r);
                            c = no_match_cost(a, r);
                        } else {
                            pp = lo + e - deg - 1;
                            const int32_t j = a.pairs[2 * (int64_t)pp + 1];
                            edge = a.limit[j] > 1;
                            k = (int32_t)(S0 + j);
                            c = a.cost[pp] + a.pc;
                        }
                    }
                    if (edge) {
                        const int32_t mk = a.mark[k];
                        nd = off + (c - a.v[k]);
                        if (mk != s_done && nd <= ub) {
                            fresh = mk != s_front;
                            upd = fresh || nd < a.d[k];
                            if (upd) {
                                a.d[k] = nd;
                                a.pred[k] = r;
                                a.ec[k] = c;
                                a.ppair[k] = pp;
                                a.mark[k] = s_front;
                            }
                        }
                    }
                    const bool free_col = upd && room(k);
                    const unsigned long long nb = __ballot(fresh);
                    if (fresh) a.list[L + __builtin_popcountll(nb & lt_mask)] = k;
                    L += __builtin_popcountll(nb);
                    ub = fmin(ub, wave_min(free_col ? nd : __builtin_inf()));
                    int32_t ek = free_col && nd <= early ? k : NO_OWNER;
                    for (int o = WAVE / 2; o > 0; o >>= 1) ek = min(ek, __shfl_xor(ek, o));
                    early_k = min(early_k, ek);
                }
                __syncthreads();
                return early_k;
            };
            relax(i0, 0.0, -__builtin_inf());
            for (;;) {
                if (L == 0 || ++pops > (unsigned long long)a.max_pops) {   // no free column reachable (NaN costs), or the cap
                    flags |= L == 0 ? 1 : 2;
                    break;
                }
                double bd = __builtin_inf();
                int32_t bk = NO_OWNER;
                int64_t bpos = -1;
                for (int64_t x = lane; x < L; x += WAVE) {
                    const int32_t k = a.list[x];
                    const double dk = a.d[k];
                    if (dk < bd || (dk == bd && k < bk)) {
                        bd = dk;
                        bk = k;
                        bpos = x;
                    }
                }
                for (int o = WAVE / 2; o > 0; o >>= 1) {
                    const double od = __shfl_xor(bd, o);
                    const int32_t ok = __shfl_xor(bk, o);
                    const int64_t op = __shfl_xor(bpos, o);
                    if (od < bd || (od == bd && ok < bk)) {
                        bd = od;
                        bk = ok;
                        bpos = op;
                    }
                }
                if (bk == NO_OWNER) {              // only NaN distances left
                    flags |= 1;
                    break;
                }
                --L;
                if (lane == 0) {
                    a.list[bpos] = a.list[L];
                    a.mark[bk] = s_done;
                    a.done[F] = bk;
                }
                ++F;
                __syncthreads();
                if (room(bk)) {
                    sink = bk;
                    d_sink = bd;
                    break;
                }
                int32_t ek = relax(a.col_row[bk], bd - (a.rc[a.col_row[bk]] - a.v[bk]), bd);
                if (CAP && bk >= S0)          // a full shared column: its other holders too, in list order (each counts as a pop)
                    for (int32_t r = a.nxt[a.col_row[bk]]; r >= 0 && ek == NO_OWNER && ++pops <= (unsigned long long)a.max_pops; r = a.nxt[r])
                        ek = relax(r, bd - (a.rc[r] - a.v[bk]), bd);
                if (ek != NO_OWNER) {
                    sink = ek;
                    d_sink = a.d[ek];
                    if (lane == 0) {
                        a.mark[ek] = s_done;
                        a.done[F] = ek;
                    }
                    ++F;
                    __syncthreads();
                    break;
                }
            }
            if (flags) break;
            // flip the path, then move the finalized columns' potentials
            if (lane == 0) {
                int32_t j = sink;
                for (int64_t steps = 0;; ++steps) {
                    if (steps > F) {
                        flags |= 1;
                        break;
                    }
                    const int32_t r = a.pred[j], prev = a.row_col[r];
                    if (CAP && prev >= S0) {        // r leaves its shared column's list (the next step brings that column a holder)
                        const int32_t pr = a.prv[r], nx = a.nxt[r];
                        if (pr >= 0) a.nxt[pr] = nx;
                        else a.col_row[prev] = nx;
                        if (nx >= 0) a.prv[nx] = pr;
                        --a.cnt[prev - S0];
                    }
                    a.row_col[r] = j;
                    if (CAP && j >= S0) {           // ... and joins j's at its head
                        const int32_t h = a.col_row[j];
                        a.nxt[r] = h;
                        a.prv[r] = -1;
                        if (h >= 0) a.prv[h] = r;
                        ++a.cnt[j - S0];
                    }
                    a.col_row[j] = r;
                    a.rc[r] = a.ec[j];
                    a.match_pair[r] = a.ppair[j];
                    if (r == i0) break;
                    j = prev;
                }
            }
            for (int64_t f = lane; f < F; f += WAVE) {
                const int32_t k = a.done[f];
                a.v[k] += a.d[k] - d_sink;
            }
            flags = __shfl(flags, 0);
            __syncthreads();
        }
    }
    double obj = 0.0;
    for (int64_t i = lane; i < n; i += WAVE) obj += a.rc[i];
    obj = wave_sum(obj);
    double extra = 0.0;                   // sum_j max(0, count_j - 1): whole numbers, exact in fp64
    if (CAP) {
        for (int64_t j = lane; j < n_r; j += WAVE) extra += (double)max(0, (a.col_row[j] >= 0) + a.cnt[j] - 1);
        extra = wave_sum(extra);
    }
    if (lane == 0) {
        a.res[0] = searches;
        a.res[1] = pops;
        a.res[2] = flags;
        a.res[3] = (unsigned long long)__double_as_longlong(obj);
        if (CAP) a.res[4] = (unsigned long long)extra;
    }
}

// the certificate: rows (blockIdx.x < row blocks) and reference columns (the blocks after them); any failure sets bit 2 of res[2]
template <bool CAP>
__global__ __launch_bounds__(256) void certificate_kernel(win::Batch<asg::AssignArgs> b, unsigned row_blocks) {
    const asg::AssignArgs &a = b.w[blockIdx.y];
    const int64_t n = a.n, n_r = a.n_r, S0 = n_r + n, C = CAP ? S0 + n_r : S0;
    if (CAP && n == 0) return;                 // (nothing was laid out or solved)
    bool bad = false;
    if (blockIdx.x < row_blocks) {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        const int32_t m = a.row_col[i], mp = a.match_pair[i];
        bool held = m >= 0 && m < C;
        if (held && CAP && m >= S0) {          // a shared column lists the row: back along the list to its head, `limit` steps at most
            int32_t r = (int32_t)i;
            for (int32_t steps = a.limit[m - S0]; steps > 0 && r >= 0 && r < n && a.prv[r] >= 0; --steps) r = a.prv[r];
            held = r >= 0 && r < n && a.prv[r] < 0 && a.col_row[m] == r;
        } else if (held) {
            held = a.col_row[m] == (int32_t)i;
        }
        if (!held) {
            bad = true;
        } else {
            const double cm = a.rc[i], vm = a.v[m], h = cm - vm;
            const double cnm = no_match_cost(a, i);
            if (mp >= 0) {
                bad = mp < a.prow[i] || mp >= a.prow[i + 1];
                if (!bad) {
                    const int32_t j = a.pairs[2 * (int64_t)mp + 1];
                    if (CAP && m >= S0) bad = m != S0 + j || a.limit[j] <= 1 || !(a.cost[mp] + a.pc == cm);
                    else bad = j != m || !(a.cost[mp] == cm);
                }
            } else {
                bad = m != n_r + i || !(cnm == cm);
            }
            for (int32_t p = a.prow[i]; p <= a.prow[i + 1] && !bad; ++p) {
                const bool nm = p == a.prow[i + 1];
                const int64_t k = nm ? n_r + i : a.pairs[2 * (int64_t)p + 1];
                const double c = nm ? cnm : a.cost[p], vk = a.v[k];
                const double red = (c - vk) - h;
                const double tol = 0x1p-40 * (fabs(c) + fabs(vk) + fabs(cm) + fabs(vm));
                bad = !(red >= -tol);
                if (CAP && !nm && !bad && a.limit[k] > 1) {       // the pair's second tier
                    const double c2 = c + a.pc, v2 = a.v[S0 + k];
                    bad = !((c2 - v2) - h >= -0x1p-40 * (fabs(c2) + fabs(v2) + fabs(cm) + fabs(vm)));
                }
            }
        }
    } else {
        const int64_t j = (int64_t)(blockIdx.x - row_blocks) * blockDim.x + threadIdx.x;
        if (j >= n_r) return;
        const int32_t r = a.col_row[j];
        bad = r < 0 ? a.v[j] != 0.0 : (r >= n || a.row_col[r] != (int32_t)j);
        if (CAP && !bad) {
            // the slot column's surcharge is no bonus; the shared column: its list has cnt members, all holding it, cnt within the
            // capacity, v = 0 with room and no bonus without
            if (r >= 0) bad = !(a.v[j] <= 0x1p-40 * (fabs(a.v[j]) + fabs(a.rc[r])));
            const int32_t cnt = a.cnt[j], cap = a.limit[j] - 1, k = (int32_t)(S0 + j);
            int32_t seen = 0, prev = -1;
            double scale = 0.0;
            bool ok = cnt >= 0 && cnt <= cap;
            for (int32_t q = a.col_row[k]; ok && q >= 0; ++seen) {
                ok = q < n && seen < cnt && a.row_col[q] == k && a.prv[q] == prev;
                if (!ok) break;
                scale = fmax(scale, fabs(a.rc[q]));
                prev = q;
                q = a.nxt[q];
            }
            ok = ok && seen == cnt;
            if (ok) ok = cnt < cap ? a.v[k] == 0.0 : a.v[k] <= 0x1p-40 * (fabs(a.v[k]) + scale);
            bad = bad || !ok;
        }
    }
    if (bad) atomicOr(&a.res[2], 4ull);
}

}  // namespace

namespace asg {

void lay(AssignArgs &a, win::Carver &cv) {
    // sized by the counts themselves (rfn::lay gives every array one element at least)
    // (the transport form: a shared column per reference behind them, the holder lists' links per row)
    const size_t C = (size_t)(a.n + a.n_r) + (a.transport ? (size_t)a.n_r : 0);
    for (int32_t **p : {&a.col_row, &a.pred, &a.mark, &a.list, &a.done, &a.ppair}) *p = cv.take<int32_t>(C);
    a.row_col = cv.take<int32_t>((size_t)a.n);
    for (double **p : {&a.v, &a.d, &a.ec}) *p = cv.take<double>(C);
    a.rc = cv.take<double>((size_t)a.n);
    if (a.transport) {
        for (int32_t **p : {&a.limit, &a.cnt}) *p = cv.take<int32_t>((size_t)a.n_r);
        for (int32_t **p : {&a.nxt, &a.prv}) *p = cv.take<int32_t>((size_t)a.n);
    }
}

int64_t default_max_pops(int64_t n, int64_t n_r, int64_t P, bool transport) {
    // every search finalizes at most n_r + n columns; a window that needs more than this many in all is left to the host.  The
    // transport form: n_r shared columns and P second-tier edges more, and every holder a full shared column relaxes counts as one
    return transport ? 64 * (n + 2 * n_r + 2 * P) + 4096 : 64 * (n + n_r + P) + 4096;
}

int launch(same_ctx *ctx, const AssignArgs *jobs, int n_w) {
    if (n_w <= 0) return SAME_OK;
    win::Batch<AssignArgs> bt{};
    int64_t max_n = 0, max_r = 0;
    for (int q = 0; q < n_w; ++q) {
        REQUIRE(ctx, jobs[q].transport == jobs[0].transport);
        bt.w[q] = jobs[q];
        max_n = std::max(max_n, jobs[q].n);
        max_r = std::max(max_r, jobs[q].n_r);
    }
    const unsigned rb = win::grid_for(max_n);
    const dim3 cert(rb + win::grid_for(max_r), (unsigned)n_w);
    if (jobs[0].transport) {        // (a launch's problems are of one form)
        SAME_LAUNCH(ctx, assign_kernel<true>, dim3(1, (unsigned)n_w), dim3(WAVE), 0, bt);
        SAME_LAUNCH(ctx, certificate_kernel<true>, cert, dim3(256), 0, bt, rb);
    } else {
        SAME_LAUNCH(ctx, assign_kernel<false>, dim3(1, (unsigned)n_w), dim3(WAVE), 0, bt);
        SAME_LAUNCH(ctx, certificate_kernel<false>, cert, dim3(256), 0, bt, rb);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace asg

// ref_limit null: the one-to-one problem (same_sparse_assign, four stats words); else the transport form (five)
static int assign_host(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m, int64_t n_r,
                       const int32_t *ref_limit, double penalty_coeff, int32_t *out_match_pair, int64_t *out_stats) {
    REQUIRE(ctx, ctx != nullptr);
    REQUIRE(ctx, P >= 0 && n_m >= 0 && n_r >= 0 && n_m + n_r < ((int64_t)1 << 30) && P < ((int64_t)1 << 31) - 1);
    REQUIRE(ctx, !ref_limit || (n_m + 2 * n_r < ((int64_t)1 << 30) && P < ((int64_t)1 << 30)));      // shared columns, second-tier edges
    REQUIRE(ctx, (P == 0 || (pairs && costs)) && (n_m == 0 || (unmatched && out_match_pair)) && out_stats);
    const int n_res = ref_limit ? 5 : 4;
    if (ref_limit) {
        REQUIRE(ctx, penalty_coeff >= 0.0 && penalty_coeff - penalty_coeff == 0.0);
        for (int64_t j = 0; j < n_r; ++j) REQUIRE(ctx, ref_limit[j] >= 1 && ref_limit[j] <= asg::MAX_LIMIT);
    }
    // the pairs by row (stable), each (row, column) once
    same_pair_csr by_row;
    SAME_TRY(same_pairs_by_row(ctx, pairs, costs, P, n_m, n_r, &by_row));
    const std::vector<int32_t> &order = by_row.order;
    SAME_TRY(same_use(ctx));
    asg::AssignArgs a{};
    a.n = n_m;
    a.n_r = n_r;
    a.transport = ref_limit != nullptr;
    a.pc = penalty_coeff;
    a.max_pops = asg::default_max_pops(n_m, n_r, P, a.transport);
    int32_t *d_prow, *d_pairs;
    double *d_cost, *d_unm;
    auto lay = [&](win::Carver cv) {       // (one element more than each input: no array is empty)
        a.prow = d_prow = cv.take<int32_t>((size_t)n_m + 1);
        a.pairs = d_pairs = cv.take<int32_t>((size_t)P * 2 + 2);
        a.cost = d_cost = cv.take<double>((size_t)P + 1);
        a.unm = d_unm = cv.take<double>((size_t)n_m + 1);
        a.match_pair = cv.take<int32_t>((size_t)n_m + 1);
        a.res = cv.take<unsigned long long>(5);
        asg::lay(a, cv);
        return cv.off;
    };
    char *d = nullptr;
    SAME_TRY(slot_as(ctx, SL_OUT0, lay(win::Carver()), &d));
    lay(win::Carver(d));
    SAME_COPY(ctx, d_prow, by_row.prow.data(), by_row.prow.size() * 4, hipMemcpyHostToDevice);
    if (P) {
        SAME_COPY(ctx, d_pairs, by_row.csr.data(), (size_t)P * 8, hipMemcpyHostToDevice);
        SAME_COPY(ctx, d_cost, by_row.ccsr.data(), (size_t)P * 8, hipMemcpyHostToDevice);
    }
    if (n_m) SAME_COPY(ctx, d_unm, unmatched, (size_t)n_m * 8, hipMemcpyHostToDevice);
    if (ref_limit && n_r) SAME_COPY(ctx, a.limit, ref_limit, (size_t)n_r * 4, hipMemcpyHostToDevice);
    SAME_TRY(asg::launch(ctx, &a, 1));
    std::vector<int32_t> mp((size_t)n_m);
    unsigned long long res[5] = {};
    if (n_m) SAME_COPY(ctx, mp.data(), a.match_pair, (size_t)n_m * 4, hipMemcpyDeviceToHost);
    SAME_COPY(ctx, res, a.res, (size_t)n_res * 8, hipMemcpyDeviceToHost);
    SAME_WAIT(ctx);
    for (int64_t i = 0; i < n_m; ++i) out_match_pair[i] = mp[(size_t)i] >= 0 ? order[(size_t)mp[(size_t)i]] : -1;
    for (int q = 0; q < n_res; ++q) out_stats[q] = (int64_t)res[q];
    return SAME_OK;
}

extern "C" int same_sparse_assign(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                                  int64_t n_r, int32_t *out_match_pair, int64_t *out_stats) {
    return assign_host(ctx, pairs, costs, P, unmatched, n_m, n_r, nullptr, 0.0, out_match_pair, out_stats);
}

extern "C" int same_sparse_assign_cap(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched,
                                      int64_t n_m, int64_t n_r, const int32_t *ref_limit, double penalty_coeff, int32_t *out_match_pair,
                                      int64_t *out_stats) {
    REQUIRE(ctx, ctx != nullptr && (n_r <= 0 || ref_limit));
    static const int32_t none = 1;       // (n_r == 0: no limits to read, still the transport form)
    return assign_host(ctx, pairs, costs, P, unmatched, n_m, n_r, ref_limit ? ref_limit : &none, penalty_coeff, out_match_pair, out_stats);
}
