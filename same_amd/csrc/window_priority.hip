// window_priority.hip -- the cell-type-priority prune on the window path (src/knn_utils.py:28-78, switched at src/same.py:974-976, with
// the frames resident).  The reference walks the aligned rows in ascending order carrying the set of references already claimed: a row
// whose NEAREST reference has its cell type and is not yet claimed keeps only that pair and claims it; every other row keeps all its
// pairs, each row re-sorted by distance with a stable sort (:40-49).  Only nearest references are ever claimed, and only by such rows, so
// the walk has a closed form (same_amd.knn.priority_filter): among the rows whose nearest reference j has their type the LOWEST gets j.
// Per batch of staged windows, one call and one wait (same_window_priority_pairs):
//   rank + claim   one thread per pair: d = sqrt(dx*dx + dy*dy) in fp64, every operation rounded to nearest (the host's np.sqrt((ax-rx)**2 +
//                  (ay-ry)**2); NOT np.linalg.norm's fused form, devmath.h); the pair's stable rank in its row = #{q : d_q < d_p or (d_q ==
//                  d_p and q < p)}.  The rank-0 pair is the row's nearest: where its reference carries the row's label (equal non-negative
//                  label codes) the row bids for it with atomicMin(claim[j], row).
//   keep counts    a row is a winner iff claim[its nearest] is the row itself: it keeps one pair, every other row all of its pairs; one
//                  ordered scan (scan.h) of the counts gives the new pair offsets.
//   scatter        one thread per pair: a kept pair goes to new_prow[row] + rank (a winner's nearest to new_prow[row]), with its reference
//                  row and its cost, into a SECOND set of arrays (the window's `prio` buffer); the window's pointers are turned to them.
// The aligned side is untouched (every kept cell keeps a pair) and the reference side is NOT compacted again (:78 returns the frames it
// got): the pair list as staged stays where it is and stays what as_staged() answers (window_state.h).  The batch is driven by
// window_stage.hip's driver (window_internal.h).
#include <climits>

#include "window_internal.h"

namespace {

using namespace devmath;
using namespace win;
using scan::Pair;

// per window of a launch
struct PrioArgs {
    int64_t n, n_r;                    // kept aligned cells, reference rows in the box
    PairList src, dst;                 // the list as staged; the filtered list (the `prio` buffer: room for src.P pairs)
    const int32_t *rows_ua;
    const double *axy, *ref_xy;        // XY of the kept cells; XY of the reference SECTION
    const int32_t *code_m, *code_r;    // label codes per section row
    int32_t *claim, *near, *rank;      // [n_r] lowest bidding row; [n] the row's nearest reference in the window; [src.P] stable rank in the row
    unsigned long long *st, *counts;   // scan words; the window's count block: [3] pairs left, [4] rows that kept one pair
};

__global__ __launch_bounds__(256) void prio_init_kernel(Batch<PrioArgs> b) {
    const PrioArgs &w = b.w[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < w.n_r) w.claim[j] = INT_MAX;
    if (j < w.n) w.near[j] = -1;                  // (every kept row has a rank-0 pair that overwrites it; -1 names no reference)
}

__global__ __launch_bounds__(256) void prio_rank_kernel(Batch<PrioArgs> b) {
    const PrioArgs &w = b.w[blockIdx.y];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.src.P) return;
    const int32_t a = w.src.pairs[2 * p];
    if (a < 0 || a >= w.n) return;
    const int32_t *__restrict__ jsec0 = w.src.jsec;
    const double2_t m = ld2(w.axy, a);
    // correctly rounded by contract: the products and the sum are separate IEEE operations (-ffp-contract=off), and __builtin_sqrt is
    // llvm.sqrt.f64 without the `afn` flag (-fno-fast-math), which LLVM defines as the IEEE-754 square root -- round to nearest even
    auto dist = [&](int64_t q) {
        const double2_t r = ld2(w.ref_xy, jsec0[q]);
        const double dx = m.x - r.x, dy = m.y - r.y;
        return __builtin_sqrt(dx * dx + dy * dy);
    };
    const double d = dist(p);
    int32_t rank = 0;
    for (int64_t q = w.src.prow[a], e = w.src.prow[a + 1]; q < e; ++q) {
        if (q == p) continue;
        const double dq = dist(q);
        rank += (dq < d || (dq == d && q < p)) ? 1 : 0;
    }
    w.rank[p] = rank;
    if (rank == 0) {
        const int32_t j = w.src.pairs[2 * p + 1];
        w.near[a] = j;
        const int32_t cm = w.code_m[w.rows_ua[a]], cr = w.code_r[jsec0[p]];
        if (cm == cr && cm >= 0 && j >= 0 && j < w.n_r) atomicMin(&w.claim[j], a);
    }
}

__device__ __forceinline__ bool prio_wins(const PrioArgs &w, int64_t a) {
    const int32_t j = w.near[a];
    return j >= 0 && j < w.n_r && w.claim[j] == (int32_t)a;
}

// the rows' new pair offsets: scan of the keep counts
__global__ __launch_bounds__(scan::NT) void prio_rows_kernel(Batch<PrioArgs> b) {
    __shared__ scan::Shared sh;
    const PrioArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n);
    if ((int)blockIdx.x >= nb || w.n == 0) return;
    const int64_t n = w.n;
    const int32_t *__restrict__ prow0 = w.src.prow;
    auto val = [&](int64_t a) {
        if (a >= n) return Pair{0u, 0u};
        const bool win = prio_wins(w, a);
        return Pair{win ? 1u : 0u, win ? 1u : (unsigned)(prow0[a + 1] - prow0[a])};
    };
    Pair through;
    const Pair off = scan::exclusive(w.st, (int)blockIdx.x, val, sh, &through);
    const int64_t a = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    const bool last = (int)blockIdx.x == nb - 1;
    rows_tail(w.dst, w.counts, a < n, a, off, last, n, through);
    if (last && threadIdx.x == 0) w.counts[4] = through.a;
}

__global__ __launch_bounds__(256) void prio_scatter_kernel(Batch<PrioArgs> b) {
    const PrioArgs &w = b.w[blockIdx.y];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.src.P) return;
    const int32_t a = w.src.pairs[2 * p];
    if (a < 0 || a >= w.n) return;
    const bool win = prio_wins(w, a);
    const int32_t r = w.rank[p];
    if (win && r != 0) return;
    const int64_t dst = (int64_t)w.dst.prow[a] + (win ? 0 : r);
    if (dst >= w.src.P) return;                   // (ranks are a permutation of the row's places: never taken)
    move_pair(w.dst, dst, a, w.src, p);
}

using PrioPlan = ListPlan<PrioArgs>;

// One window's `prio` buffer laid out; no launch.
int prepare_priority(same_window *w, PrioPlan *pp) {
    same_ctx *ctx = w->ctx;
    const int64_t n = w->cur.n_ua, P0 = w->cur.list.P, n_r = w->n_r;
    PrioArgs &a = pp->a;
    a = PrioArgs{};
    size_t zero_bytes = 0;
    auto lay = [&](Carver c) {
        a.st = scan::arg(c.scan_words(n));          // zeroed head: the scan words
        zero_bytes = c.off;
        a.near = c.take<int32_t>((size_t)n);
        a.claim = c.take<int32_t>((size_t)n_r);
        a.rank = c.take<int32_t>((size_t)P0);
        a.dst.prow = c.take<int32_t>((size_t)n + 1);
        a.dst.pairs = c.take<int32_t>((size_t)P0 * 2);
        a.dst.jsec = c.take<int32_t>((size_t)P0);
        a.dst.cost64 = c.take<double>((size_t)P0);
        return c.off;
    };
    SAME_TRY(ensure(ctx, w->prio, lay(Carver())));
    lay(Carver(w->prio.p));
    pp->zero = ZeroArgs{{w->prio.p, nullptr}, {zero_bytes, 0}};
    a.n = n;
    a.n_r = n_r;
    a.src = w->cur.list;
    a.rows_ua = w->cur.rows_ua;
    a.axy = w->cur.axy_c;
    a.ref_xy = w->ref->xy;
    a.code_m = w->mov->label_codes;
    a.code_r = w->ref->label_codes;
    a.counts = w->cur.counts;
    return SAME_OK;
}

int launch_priority(same_ctx *ctx, PrioPlan *const *pps, int n_w) {
    Batch<PrioArgs> b{};
    ListGrid g;
    SAME_TRY(begin_group(ctx, pps, n_w, &b, &g));
    int64_t max_r = 0;
    for (int q = 0; q < n_w; ++q) max_r = std::max(max_r, b.w[q].n_r);
    SAME_LAUNCH(ctx, prio_init_kernel, dim3(grid_for(std::max(max_r, g.max_n)), g.nw), dim3(256), 0, b);
    SAME_LAUNCH(ctx, prio_rank_kernel, dim3(grid_for(g.max_P), g.nw), dim3(256), 0, b);
    SAME_LAUNCH(ctx, prio_rows_kernel, dim3(scan::blocks_for(g.max_n), g.nw), dim3(scan::NT), 0, b);
    SAME_LAUNCH(ctx, prio_scatter_kernel, dim3(grid_for(g.max_P), g.nw), dim3(256), 0, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace

extern "C" {

int same_section_set_label_codes(same_section *s, const int32_t *codes) {
    if (!s) return SAME_EINVAL;
    same_ctx *ctx = s->ctx;
    REQUIRE(ctx, codes || s->n == 0);
    SAME_TRY(same_use(ctx));
    if (s->label_codes) {
        HIP_TRY(ctx, hipDeviceSynchronize());     // windows of other contexts may still be reading the old codes
        (void)hipFree(s->label_codes);
        s->label_codes = nullptr;
    }
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&s->label_codes), (size_t)std::max<int64_t>(s->n, 1) * sizeof(int32_t)));
    if (s->n) {
        HIP_TRY(ctx, hipMemcpyAsync(s->label_codes, codes, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SAME_OK;
}

int same_window_priority_pairs(same_window *const *windows, int n_windows, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, out_counts);
    for (int i = 0; i < n_windows; ++i) {
        const same_window *w = windows[i];
        REQUIRE(ctx, w->is_staged() && w->mov && w->ref);
        REQUIRE(ctx, w->mov->label_codes && w->ref->label_codes);
        REQUIRE(ctx, w->may_prune());
        // the sections' grids as the window was staged over them (a shared hold each: same_section_bin swaps under the exclusive one)
        for (const same_section *sec : {w->mov, w->ref}) {
            same_section *s = const_cast<same_section *>(sec);
            std::shared_lock<std::shared_mutex> hold(s->grid_lock);
            REQUIRE(ctx, s->bins == (sec == w->mov ? w->bins_m : w->bins_r));
        }
    }
    for (int q = 0; q < 4 * n_windows; ++q) out_counts[q] = 0;
    SAME_TRY(same_use(ctx));
    std::vector<PrioPlan> plans((size_t)n_windows);
    std::vector<int> live;
    int rc = SAME_OK;
    for (int i = 0; i < n_windows && rc == SAME_OK; ++i) {
        same_window *w = windows[i];
        if (!w->pairs_possible() || w->cur.list.P == 0 || w->cur.n_ua == 0) continue;       // no pairs: nothing to rank, nothing launched
        rc = prepare_priority(w, &plans[(size_t)i]);
        if (rc == SAME_OK) live.push_back(i);
    }
    // ONE wait for the batch: per group the zeroing and the four kernels, then every window's count block into the head of its pinned
    // block, where the stage call left the staged counts
    if (rc == SAME_OK)
        rc = for_each_group(plans, live, [&](PrioPlan *const *pps, const int *at, int n_g) {
            SAME_TRY(launch_priority(ctx, pps, n_g));
            Back back[SAME_LAUNCH_WINDOWS];
            for (int q = 0; q < n_g; ++q) back[q] = Back{windows[at[q]], windows[at[q]]->cur.counts, 64};
            return copy_back_group(ctx, back, n_g, "priority prune copy back");
        });
    if (rc != SAME_OK) return fail_batch(ctx, windows, live, rc);
    if (!live.empty()) SAME_WAIT(ctx);
    for (int i : live) {
        same_window *w = windows[i];
        const PrioArgs &a = plans[(size_t)i].a;
        const unsigned long long *tot = static_cast<const unsigned long long *>(w->host);
        const int64_t P = (int64_t)tot[3], one = (int64_t)tot[4];
        REQUIRE(ctx, P >= a.n && P <= a.src.P && one >= 0 && one <= a.n && (int64_t)tot[2] == a.n);
        PairList left = a.dst;
        left.P = P;
        w->pruned(a.src, left);
        int64_t *counts = out_counts + 4 * i;
        counts[0] = a.src.P;
        counts[1] = P;
        counts[2] = one;
        counts[3] = a.n - one;
    }
    return SAME_OK;
}

}  // extern "C"
