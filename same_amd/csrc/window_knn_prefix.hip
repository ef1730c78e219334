// window_knn_prefix.hip -- a staged window's pair list at a SMALLER k, derived from the list as staged instead of staged again
// (same_window_knn_prefix).  The prune keeps an aligned row when any reference lies within the radius, whatever k is, and orders a row's
// candidates by (squared distance, reference row) ascending -- a total order (knn.hip:1-13).  The list a stage call at k' <= k leaves is
// therefore, row by row, the first min(k', count) pairs of the list staged at k: the same kept aligned cells, the same reference rows in
// the box (a pair's reference number is its place among THOSE, window_stage.hip), the same costs.  Per batch of staged windows:
//   row offsets    one ordered scan (scan.h) of min(k', count) over the kept rows gives the new pair offsets and the new pair count
//   scatter        one thread per staged pair: a pair whose place in its row is below k' goes to new_prow[row] + place with its reference
//                  number, its reference's section row and its cost -- copied, never recomputed -- into a SECOND set of arrays (the
//                  window's `kpre` buffer); the window's pointers are turned to them.
// The aligned side is untouched, so a triangulation held for the window stays valid.  The list as staged stays where the stage call put it
// (win::State::sk): every prefix is derived from it, and a prefix at the staged k turns the window back to it without a launch.  What the
// call leaves and invalidates -- the window a stage call at k' leaves; a window same_window_caller_tris compacted turned back first, the
// caller's work HELD for same_window_caller_pairs -- is the knn_prefix row of window_state.h's table.  Turning back and pushing the cut
// list through the held mask are two calls, not one fused kernel, because the staged prefix must exist as a list of its own: the frame of
// the _cap calls' reference limits, SAME_WINDOW_STAGED_PAIRS and `ref_idx` are read over the pair list AS STAGED AT THAT k -- rows of
// removed nodes included -- not over the compacted one, and a priority prune may come between the two.
#include "window_internal.h"

namespace {

using namespace win;
using scan::Pair;

// per window of a launch
struct PrefixArgs {
    int64_t n, cap;                    // kept aligned cells, pairs the prefix buffer holds (>= the prefix's count)
    int k;
    PairList src, dst;                 // the list as staged; the prefix (the `kpre` buffer)
    unsigned long long *st, *counts;   // scan words; the window's count block: [3] pairs
};

__device__ __forceinline__ unsigned prefix_keep(const PrefixArgs &w, int64_t a) {
    const int32_t c = w.src.prow[a + 1] - w.src.prow[a];
    return (unsigned)(c < 0 ? 0 : (c < w.k ? c : w.k));
}

// the rows' new pair offsets: scan of min(k, count)
__global__ __launch_bounds__(scan::NT) void prefix_rows_kernel(Batch<PrefixArgs> b) {
    __shared__ scan::Shared sh;
    const PrefixArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n);
    if ((int)blockIdx.x >= nb || w.n == 0) return;
    const int64_t n = w.n;
    auto val = [&](int64_t a) { return a < n ? Pair{1u, prefix_keep(w, a)} : Pair{0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st, (int)blockIdx.x, val, sh, &through);
    const int64_t a = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    const bool last = (int)blockIdx.x == nb - 1;
    rows_tail(w.dst, w.counts, a < n, a, off, last, n, through);
    if (last && threadIdx.x == 0) w.counts[4] = 0;       // (a priority prune's count: a freshly staged window has none)
}

__global__ __launch_bounds__(256) void prefix_scatter_kernel(Batch<PrefixArgs> b) {
    const PrefixArgs &w = b.w[blockIdx.y];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.src.P) return;
    const int32_t a = w.src.pairs[2 * p];
    if (a < 0 || a >= w.n) return;
    const int64_t place = p - w.src.prow[a];        // the pair's place in its row: the stage call wrote a row's pairs in the prune's order
    if (place < 0 || place >= w.k) return;
    const int64_t dst = (int64_t)w.dst.prow[a] + place;
    if (dst >= w.cap) return;                     // (the offsets are the scan of min(k, count): never taken)
    move_pair(w.dst, dst, a, w.src, p);
}

using PrefixPlan = ListPlan<PrefixArgs>;

// One window's `kpre` buffer laid out; no launch.
int prepare_prefix(same_window *w, int k, PrefixPlan *pp) {
    same_ctx *ctx = w->ctx;
    const int64_t n = w->cur.n_ua, P0 = w->sk.P, cap = std::min<int64_t>(P0, n * (int64_t)k);
    PrefixArgs &a = pp->a;
    a = PrefixArgs{};
    size_t zero_bytes = 0;
    auto lay = [&](Carver c) {
        a.st = scan::arg(c.scan_words(n));          // zeroed head: the scan words
        zero_bytes = c.off;
        a.dst.prow = c.take<int32_t>((size_t)n + 1);
        a.dst.pairs = c.take<int32_t>((size_t)cap * 2);
        a.dst.jsec = c.take<int32_t>((size_t)cap);
        a.dst.cost64 = c.take<double>((size_t)cap);
        return c.off;
    };
    SAME_TRY(ensure(ctx, w->kpre, lay(Carver())));
    lay(Carver(w->kpre.p));
    pp->zero = ZeroArgs{{w->kpre.p, nullptr}, {zero_bytes, 0}};
    a.n = n;
    a.cap = cap;
    a.k = k;
    a.src = w->sk;
    a.counts = w->cur.counts;
    return SAME_OK;
}

int launch_prefix(same_ctx *ctx, PrefixPlan *const *pps, int n_w) {
    Batch<PrefixArgs> b{};
    ListGrid g;
    SAME_TRY(begin_group(ctx, pps, n_w, &b, &g));
    SAME_LAUNCH(ctx, prefix_rows_kernel, dim3(scan::blocks_for(g.max_n), g.nw), dim3(scan::NT), 0, b);
    SAME_LAUNCH(ctx, prefix_scatter_kernel, dim3(grid_for(g.max_P), g.nw), dim3(256), 0, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace

extern "C" {

int same_window_knn_prefix(same_window *const *windows, int n_windows, int k, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, out_counts && k >= 1);
    for (int i = 0; i < n_windows; ++i) {
        const same_window *w = windows[i];
        REQUIRE(ctx, w->may_prefix(k));
    }
    SAME_TRY(same_use(ctx));
    return restage_batch<PrefixPlan>(
        ctx, windows, n_windows, k, "k-NN prefix copy back", out_counts,
        [&](same_window *w, PrefixPlan *pp, bool *needs) {
            // no pairs: every k leaves the same (empty) list; the staged k: the list as staged, no launch
            *needs = w->pairs_possible() && w->sk.P != 0 && w->cur.n_ua != 0 && k != w->k_staged;
            return *needs ? prepare_prefix(w, k, pp) : SAME_OK;
        },
        [&](PrefixPlan *const *pps, int n_g) { return launch_prefix(ctx, pps, n_g); },
        [&](const same_window *w, const PrefixPlan &pp, PairList *cut) {
            const unsigned long long *tot = static_cast<const unsigned long long *>(w->host);
            REQUIRE(ctx, (int64_t)tot[3] >= pp.a.n && (int64_t)tot[3] <= pp.a.cap && (int64_t)tot[2] == pp.a.n);
            *cut = pp.a.dst;
            return SAME_OK;
        });
}

}  // extern "C"
