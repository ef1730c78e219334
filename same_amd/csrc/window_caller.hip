// window_caller.hip -- a CALLER's triangulation on the window path (src/same.py:425-435, :1016-1085 with the frames resident; MetaCell
// inputs bring theirs).  Once per job: the triangulation as rows of the moving section, binned by the section's grid cell of each
// triangle's first corner (same_caller_tris).  Per batch of staged windows, one call and one wait (same_window_caller_tris):
//   select + remap   the triangles of the cells the window's box covers, merged ascending by their number (window_rows_kernel: the
//                    caller's order); a triangle belongs to the window iff its three rows are among the window's kept aligned cells
//                    (three lower bounds in the ascending kept rows), its corners become indices into them, in the caller's corner
//                    order; an ordered compaction (scan.h) lays the window's triangles end to end.  O(window), whatever the job's size.
//   node mask        has_valid_triangle of src/helpers.py:323-325: set by every triangle that passes the side and angle tests, before
//                    the same-type test.  Kept cells without it are the unconstrained nodes (:357-358).
//   second compaction (src/same.py:1055-1085) the kept cells without the unconstrained ones -- rows, XY, sizes, type codes, kept index --
//                    their pairs and costs, pair rows renumbered by the mask's prefix sum; the triangles without those that name a removed
//                    node (none of them passes the tests: the filter that follows would drop them anyway), corners renumbered.
// The compacted arrays live in the window's `caller` buffer and the window is turned to them (win::State::compacted): everything after
// this call -- the filter with the same-type re-add (which then meets no unconstrained node, :370), start, search, sweeps, collect -- is the
// unchanged window path on the smaller window (same_window_filter_finish with SAME_TRIS_CALLER).  The REFERENCE side stays the prune's.
// A parameter sweep over knn (same_window_caller_pairs).  Which rows a window keeps, which of the caller's triangles are its own, the node
// mask and the renumbering do not depend on k: only the pair list behind the mask does, and the second compaction (whole rows of pairs
// go) commutes with the k-NN prefix (every row is cut to its first min(k, count) pairs).  After same_window_knn_prefix turned the
// compacted window back and HELD the caller's work (win::Held), one call per batch pushes the window's CURRENT pair list through the held mask:
//   row offsets    one ordered scan (scan.h) over the staged kept cells of valid[v] ? row count : 0 gives the new pair offsets and count
//   scatter        one thread per pair of the current list: a pair of a row that stays goes to new_prow[newidx[row]] + place, its row
//                  renumbered, its reference number, its reference's section row and its cost copied -- loads and stores run along
//                  the pair index (the per-row loop of caller_cells_kernel, which also moves the aligned side, is not repeated)
// into the pair arrays of `caller`, which were sized for the list as staged.  The window is then, array for array, the one a stage call
// at k (+ the priority prune) + same_window_caller_tris leaves.  What either call requires, leaves and invalidates: window_state.h's table.
// Both calls are batches of window_stage.hip's driver (window_internal.h); a failed batch of either leaves its live windows un-staged.
#include "window_internal.h"

namespace {

using namespace devmath;
using namespace win;
using scan::Pair;

// per window of a launch
struct CallerArgs {
    // select + remap
    const uint32_t *cand;              // the candidates' triangle numbers ascending, or null: every triangle of the job, q = its number
    int64_t n_cand;
    const int32_t *tris;               // the job's triangles [.][3], section rows
    const int32_t *rows0;              // kept aligned rows as staged, ascending
    int64_t n0;                        // kept cells as staged
    int32_t *tmp, *sel;                // [n_cand][3] remapped (first corner -1: not the window's); the window's triangles in order
    unsigned long long *st_sel, *st_cell, *st_tri, *dcount;     // scan words; [0] selected [1] removed [2] near
    // node mask
    const double *axy0;
    const int32_t *type0;              // or null: no same-type rule
    uint8_t *valid;                    // [n0]
    // second compaction
    const unsigned long long *counts0;
    const int32_t *ua0;
    const double *size0;
    PairList src, dst;                 // the window's list; the list without the removed nodes' rows, rows renumbered
    unsigned long long *counts;
    int32_t *newidx, *ua, *rows, *type_c, *out;
    double *axy, *size;
};

__device__ __forceinline__ int32_t place_of(const int32_t *__restrict__ rows, int64_t n, int32_t row) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rows[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo < n && rows[lo] == row ? (int32_t)lo : -1;
}

// candidate -> its corners as indices into the window's kept cells, or -1 in the first corner
__global__ __launch_bounds__(256) void caller_remap_kernel(Batch<CallerArgs> b) {
    const CallerArgs &w = b.w[blockIdx.y];
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n_cand) return;
    const int64_t t = w.cand ? (int64_t)w.cand[q] : q;
    const int32_t a = place_of(w.rows0, w.n0, w.tris[3 * t]);
    int32_t bb = -1, c = -1;
    if (a >= 0) bb = place_of(w.rows0, w.n0, w.tris[3 * t + 1]);
    if (bb >= 0) c = place_of(w.rows0, w.n0, w.tris[3 * t + 2]);
    const bool in = a >= 0 && bb >= 0 && c >= 0;
    w.tmp[3 * q] = in ? a : -1;
    w.tmp[3 * q + 1] = bb;
    w.tmp[3 * q + 2] = c;
}
// the window's triangles end to end, in candidate (= the caller's) order
__global__ __launch_bounds__(scan::NT) void caller_select_kernel(Batch<CallerArgs> b) {
    __shared__ scan::Shared sh;
    const CallerArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n_cand);
    if ((int)blockIdx.x >= nb || w.n_cand == 0) return;
    const int64_t n = w.n_cand;
    const int32_t *__restrict__ tmp = w.tmp;
    auto val = [&](int64_t q) { return Pair{q < n && tmp[3 * q] >= 0 ? 1u : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st_sel, (int)blockIdx.x, val, sh, &through);
    const int64_t q = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (q < n && tmp[3 * q] >= 0) {
        w.sel[3 * (int64_t)off.a] = tmp[3 * q];
        w.sel[3 * (int64_t)off.a + 1] = tmp[3 * q + 1];
        w.sel[3 * (int64_t)off.a + 2] = tmp[3 * q + 2];
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) w.dcount[0] = through.a;
}
// has_valid_triangle (src/helpers.py:323-325) and the knife-edge cosines, as filter_classify_kernel counts them
__global__ __launch_bounds__(256) void caller_mask_kernel(Batch<CallerArgs> b, double radius, int angle_enabled, double cos_thr, int near_enabled,
                                                           double tol) {
    const CallerArgs &w = b.w[blockIdx.y];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((int64_t)blockIdx.x * blockDim.x >= w.n_cand) return;
    bool near = false;
    if (t < w.n_cand && t < (int64_t)w.dcount[0]) {
        const int32_t a = w.sel[3 * t], bb = w.sel[3 * t + 1], d = w.sel[3 * t + 2];
        const int32_t *__restrict__ type_id = w.type0;
        const TriClass r = classify_triangle(ld2(w.axy0, a), ld2(w.axy0, bb), ld2(w.axy0, d), radius, angle_enabled, cos_thr,
                                             type_id && type_id[a] == type_id[bb] && type_id[bb] == type_id[d]);
        near = near_enabled && r.cls != 1 && fabs(r.maxcos - cos_thr) <= tol;
        if (r.cls == 0 || r.cls == 3) { w.valid[a] = 1; w.valid[bb] = 1; w.valid[d] = 1; }
    }
    const unsigned long long nb = __ballot(near);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&w.dcount[2], (unsigned long long)__builtin_popcountll(nb));
}
// the kept cells that stay, their pairs behind them (src/same.py:1055-1075): scan + scatter in one launch, as window_scatter_kernel
__global__ __launch_bounds__(scan::NT) void caller_cells_kernel(Batch<CallerArgs> b) {
    __shared__ scan::Shared sh;
    const CallerArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n0);
    if ((int)blockIdx.x >= nb || w.n0 == 0) return;
    const int64_t n = w.n0;
    const uint8_t *__restrict__ valid = w.valid;
    const int32_t *__restrict__ prow0 = w.src.prow;
    auto val = [&](int64_t v) { return v < n && valid[v] ? Pair{1u, (unsigned)(prow0[v + 1] - prow0[v])} : Pair{0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st_cell, (int)blockIdx.x, val, sh, &through);
    const int64_t v = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (v < n) {
        const bool stays = valid[v] != 0;
        w.newidx[v] = stays ? (int32_t)off.a : -1;
        if (stays) {
            const int64_t a = off.a;
            w.ua[a] = w.ua0[v];
            w.rows[a] = w.rows0[v];
            const double2_t p = ld2(w.axy0, v);
            w.axy[2 * a] = p.x;
            w.axy[2 * a + 1] = p.y;
            w.size[a] = w.size0[v];
            w.type_c[a] = w.type0 ? w.type0[v] : 0;
            w.dst.prow[a] = (int32_t)off.p;
            int64_t pp = off.p;
            for (int32_t p0 = prow0[v]; p0 < prow0[v + 1]; ++p0, ++pp) move_pair(w.dst, pp, (int32_t)a, w.src, p0);
        }
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) {
        w.counts[0] = w.counts0[0];
        w.counts[1] = w.counts0[1];
        w.counts[2] = through.a;
        w.counts[3] = through.p;
        w.dst.prow[through.a] = (int32_t)through.p;
        w.dcount[1] = (unsigned long long)n - through.a;
    }
}
// the triangles whose corners all stay, renumbered, in order (src/same.py:1076-1078)
__global__ __launch_bounds__(scan::NT) void caller_tris_kernel(Batch<CallerArgs> b) {
    __shared__ scan::Shared sh;
    const CallerArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n_cand);
    if ((int)blockIdx.x >= nb || w.n_cand == 0) return;
    const int64_t n = (int64_t)w.dcount[0];
    const int32_t *__restrict__ sel = w.sel, *__restrict__ newidx = w.newidx;
    auto stays = [&](int64_t t) { return t < n && newidx[sel[3 * t]] >= 0 && newidx[sel[3 * t + 1]] >= 0 && newidx[sel[3 * t + 2]] >= 0; };
    auto val = [&](int64_t t) { return Pair{stays(t) ? 1u : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st_tri, (int)blockIdx.x, val, sh, &through);
    const int64_t t = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (stays(t)) {
        w.out[3 * (int64_t)off.a] = newidx[sel[3 * t]];
        w.out[3 * (int64_t)off.a + 1] = newidx[sel[3 * t + 1]];
        w.out[3 * (int64_t)off.a + 2] = newidx[sel[3 * t + 2]];
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) w.counts[4] = through.a;
}
// the words the host reads beside the four counts: [4] triangles left (above; 0 without candidates), [5] selected, [6] near, [7] removed
__global__ void caller_counts_kernel(Batch<CallerArgs> b) {
    const CallerArgs &w = b.w[blockIdx.x];
    if (threadIdx.x != 0 || w.n0 == 0) return;
    if (w.n_cand == 0) w.counts[4] = 0;
    w.counts[5] = w.dcount[0];
    w.counts[6] = w.dcount[2];
    w.counts[7] = w.dcount[1];
}

struct CallerPlan {
    CallerArgs a{};
    RowsArgs rows{};
    ZeroArgs zero{};
    size_t back_bytes = 0;
    View next;                         // the window's view once the removal counts
    int64_t pair_cap = 0;              // pairs next's pair arrays hold
};

// One window's `caller` buffer laid out; no launch.  The caller holds the moving section's grid lock (shared).
int prepare_caller(same_window *w, const same_caller_tris *ct, bool use_type, CallerPlan *cp) {
    same_ctx *ctx = w->ctx;
    w->restart_caller();
    const int64_t n0 = w->cur.n_ua, P0 = w->cur.list.P, cap_m = w->cap_m;
    // the pair arrays take the list as STAGED (>= any prefix of it, pruned or not): same_window_caller_pairs fills them again per knn
    const int64_t pair_cap = cp->pair_cap = std::max(P0, w->sk.P);
    // the candidates: the triangles binned in the cells the box covers (their number is known here), or every triangle of the job where
    // the box covers more cells than a run takes (rare, as for the rows)
    const Cover cv = cover_of(w->mov, w->box);
    int64_t n_cand = 0;
    if (ct->n_binned) {
        if (!cv.use_runs) n_cand = ct->n_tris;
        else
            for (int cy = cv.cy0; cy < cv.cy0 + cv.ncy; ++cy)
                n_cand += (int64_t)ct->h_starts[(size_t)cy * ct->grid.nx + cv.cx0 + cv.ncx] - (int64_t)ct->h_starts[(size_t)cy * ct->grid.nx + cv.cx0];
    }
    REQUIRE(ctx, n_cand < ((int64_t)1 << 31) - 512);
    CallerArgs &a = cp->a;
    a = CallerArgs{};
    uint32_t *merged = nullptr;
    View &nx = cp->next;
    size_t o_counts = 0;
    auto lay = [&](Carver c) {
        // zeroed head: scan words, the call's counters, the node mask
        a.st_sel = scan::arg(c.scan_words(n_cand));
        a.st_cell = scan::arg(c.scan_words(n0));
        a.st_tri = scan::arg(c.scan_words(n_cand));
        a.dcount = c.take<unsigned long long>(8);
        a.valid = c.take<uint8_t>((size_t)n0);
        cp->zero.bytes[0] = c.off;
        // counts, kept XY, kept rows: contiguous and at the stage block's strides, they take its place in the pinned block in one copy
        o_counts = c.align(256);
        nx.counts = c.pack<unsigned long long>(8);
        nx.axy_c = c.pack<double>((size_t)cap_m * 2);
        nx.rows_ua = c.pack<int32_t>((size_t)cap_m);
        cp->back_bytes = c.off - o_counts;
        merged = c.take<uint32_t>((size_t)n_cand);
        a.tmp = c.take<int32_t>((size_t)n_cand * 3);
        a.sel = c.take<int32_t>((size_t)n_cand * 3);
        a.out = c.take<int32_t>((size_t)n_cand * 3);
        a.newidx = c.take<int32_t>((size_t)n0);
        nx.ua = c.take<int32_t>((size_t)n0);
        nx.type_c = c.take<int32_t>((size_t)n0);
        nx.size_c = c.take<double>((size_t)n0);
        nx.list.prow = c.take<int32_t>((size_t)n0 + 1);
        nx.list.pairs = c.take<int32_t>((size_t)pair_cap * 2);
        nx.list.jsec = c.take<int32_t>((size_t)pair_cap);
        nx.list.cost64 = c.take<double>((size_t)pair_cap);
        return c.off;
    };
    SAME_TRY(ensure(ctx, w->caller, lay(Carver())));
    lay(Carver(w->caller.p));
    cp->zero.p[0] = w->caller.p;
    cp->zero.p[1] = nullptr;
    cp->zero.bytes[1] = 0;
    const bool by_cells = cv.use_runs && n_cand > 0;
    cp->rows = RowsArgs{};
    if (by_cells) {
        cp->rows.dm = RunDesc{ct->order, ct->starts, nullptr, ct->grid.nx, cv.cx0, cv.ncx, cv.cy0, cv.ncy, (int)n_cand, 1, merged, a.dcount + 7};
        cp->rows.blocks_m = cp->rows.blocks = grid_for(n_cand);
    }
    a.cand = by_cells ? merged : nullptr;
    a.n_cand = n_cand;
    a.tris = ct->tris;
    a.rows0 = w->cur.rows_ua;
    a.n0 = n0;
    a.axy0 = w->cur.axy_c;
    a.type0 = use_type ? w->cur.type_c : nullptr;
    a.counts0 = w->cur.counts;
    a.ua0 = w->cur.ua;
    a.size0 = w->cur.size_c;
    a.src = w->cur.list;
    a.dst = nx.list;
    a.counts = nx.counts;
    a.ua = nx.ua;
    a.rows = nx.rows_ua;
    a.type_c = nx.type_c;
    a.axy = nx.axy_c;
    a.size = nx.size_c;
    w->sel_tris = a.sel;
    w->caller_out = a.out;
    return SAME_OK;
}

int launch_caller(same_ctx *ctx, CallerPlan *const *cps, int n_w, bool classify, double radius, int angle_enabled, double cos_thr, double near_tol) {
    Batch<CallerArgs> b{};
    RowsArgs rows[SAME_LAUNCH_WINDOWS];
    int64_t max_cand = 0, max_n = 0;
    for (int q = 0; q < n_w; ++q) {
        b.w[q] = cps[q]->a;
        rows[q] = cps[q]->rows;
        max_cand = std::max(max_cand, cps[q]->a.n_cand);
        max_n = std::max(max_n, cps[q]->a.n0);
    }
    const unsigned nw = (unsigned)n_w;
    if (max_cand) {
        SAME_TRY(launch_rows(ctx, rows, n_w));
        SAME_LAUNCH(ctx, caller_remap_kernel, dim3(grid_for(max_cand), nw), dim3(256), 0, b);
        SAME_LAUNCH(ctx, caller_select_kernel, dim3(scan::blocks_for(max_cand), nw), dim3(scan::NT), 0, b);
        if (classify) {
            const int near_enabled = angle_enabled && cos_thr == cos_thr && cos_thr - cos_thr == 0.0;       // a finite threshold
            SAME_LAUNCH(ctx, caller_mask_kernel, dim3(grid_for(max_cand), nw), dim3(256), 0, b, radius, angle_enabled, cos_thr, near_enabled, near_tol);
        }
    }
    if (max_n) {
        SAME_LAUNCH(ctx, caller_cells_kernel, dim3(scan::blocks_for(max_n), nw), dim3(scan::NT), 0, b);
        if (max_cand) SAME_LAUNCH(ctx, caller_tris_kernel, dim3(scan::blocks_for(max_cand), nw), dim3(scan::NT), 0, b);
        SAME_LAUNCH(ctx, caller_counts_kernel, dim3(nw), dim3(64), 0, b);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

// ---- same_window_caller_pairs: the current pair list through the held mask ------------------------------------------------------------
// per window of a launch
struct PairsArgs {
    int64_t n, cap;                    // kept cells as staged, pairs the output arrays hold
    const uint8_t *valid;
    const int32_t *newidx;
    PairList src, dst;                 // the window's current list; the compacted window's pair arrays (held.cs.list)
    unsigned long long *st, *counts;   // scan words; the compacted window's count block: [3] pairs
};

// the pair offsets of the rows that stay: scan of valid ? row count : 0
__global__ __launch_bounds__(scan::NT) void caller_pair_rows_kernel(Batch<PairsArgs> b) {
    __shared__ scan::Shared sh;
    const PairsArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n);
    if ((int)blockIdx.x >= nb || w.n == 0) return;
    const int64_t n = w.n;
    const uint8_t *__restrict__ valid = w.valid;
    const int32_t *__restrict__ prow0 = w.src.prow;
    auto val = [&](int64_t v) {
        if (v >= n || !valid[v]) return Pair{0u, 0u};
        const int32_t c = prow0[v + 1] - prow0[v];
        return Pair{1u, (unsigned)(c < 0 ? 0 : c)};
    };
    Pair through;
    const Pair off = scan::exclusive(w.st, (int)blockIdx.x, val, sh, &through);
    const int64_t v = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    // (a row that stays: off.a == newidx[v] < n, and prow holds n + 1)
    rows_tail(w.dst, w.counts, v < n && valid[v], off.a, off, (int)blockIdx.x == nb - 1, through.a, through);
}

__global__ __launch_bounds__(256) void caller_pair_scatter_kernel(Batch<PairsArgs> b) {
    const PairsArgs &w = b.w[blockIdx.y];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.src.P) return;
    const int32_t v = w.src.pairs[2 * p];
    if (v < 0 || v >= w.n) return;
    const int32_t a = w.newidx[v];
    if (a < 0 || a >= w.n) return;                // the row went with its node
    const int64_t place = p - w.src.prow[v];        // the pair's place in its row: rows keep their order, and their pairs theirs
    if (place < 0) return;
    const int64_t dst = (int64_t)w.dst.prow[a] + place;
    if (dst >= w.cap) return;                     // (the offsets are the scan of the rows' counts, the list at most the staged one: never taken)
    move_pair(w.dst, dst, a, w.src, p);
}

using PairsPlan = ListPlan<PairsArgs>;

// no buffer is laid out: every pointer is one prepare_caller placed (win::Held), or the window's current list
void prepare_pairs(const same_window *w, PairsPlan *pp) {
    const Held &h = w->held;
    PairsArgs &a = pp->a;
    a = PairsArgs{};
    a.n = w->cur.n_ua;
    a.cap = h.cap;
    a.valid = h.valid;
    a.newidx = h.newidx;
    a.src = w->cur.list;
    a.dst = h.cs.list;
    a.st = h.st;
    a.counts = h.cs.counts;
    // the scan words again (scan::arg may have tagged the pointer: the words themselves start 8-byte aligned)
    void *words = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(h.st) & ~uintptr_t(7));
    pp->zero = ZeroArgs{{words, nullptr}, {scan::status_bytes(a.n), 0}};
}

int launch_pairs(same_ctx *ctx, PairsPlan *const *pps, int n_w) {
    Batch<PairsArgs> b{};
    ListGrid g;
    SAME_TRY(begin_group(ctx, pps, n_w, &b, &g));
    SAME_LAUNCH(ctx, caller_pair_rows_kernel, dim3(scan::blocks_for(g.max_n), g.nw), dim3(scan::NT), 0, b);
    SAME_LAUNCH(ctx, caller_pair_scatter_kernel, dim3(grid_for(g.max_P), g.nw), dim3(256), 0, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace

extern "C" {

int same_caller_tris_create(same_ctx *ctx, const same_section *mov, const int32_t *tris, int64_t n_tris, same_caller_tris **out) {
    REQUIRE(ctx, ctx && out);
    *out = nullptr;
    REQUIRE(ctx, mov && mov->ctx->device == ctx->device && n_tris >= 0 && n_tris < ((int64_t)1 << 31) - 512 && (n_tris == 0 || tris));
    // every corner names a row of the section: nothing on the device depends on an index that was not looked at here
    SAME_TRY(check_index_range(ctx, tris, n_tris * 3, 0, mov->n, "caller triangulation"));
    SAME_TRY(same_use(ctx));
    same_caller_tris *ct = new (std::nothrow) same_caller_tris();
    if (!ct) return SAME_ENOMEM;
    ct->ctx = ctx;
    ct->mov = mov;
    ct->n_tris = n_tris;
    *out = ct;                                    // freed by the caller's destroy on any failure below
    std::vector<int32_t> order;
    {
        // the section's grid as it stands: cell of every row from the section's own binning (rows by cell), then the triangles
        // counting-sorted by the cell of their first corner -- stable, so ascending inside a cell
        same_section *s = const_cast<same_section *>(mov);
        std::shared_lock<std::shared_mutex> hold(s->grid_lock);
        ct->grid = s->grid;
        const size_t cells = (size_t)s->grid.nx * (size_t)s->grid.ny;
        REQUIRE(ctx, s->h_starts.size() >= cells + 1 || s->n_binned == 0);
        std::vector<int32_t> rows_by_cell((size_t)s->n_binned), cell_of((size_t)mov->n, -1);
        if (s->n_binned) {
            HIP_TRY(ctx, hipMemcpyAsync(rows_by_cell.data(), s->order, (size_t)s->n_binned * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (size_t c = 0; c < cells; ++c)
                for (unsigned q = s->h_starts[c]; q < s->h_starts[c + 1]; ++q) cell_of[(size_t)rows_by_cell[q]] = (int32_t)c;
        }
        ct->h_starts.assign(cells + 1, 0u);
        for (int64_t t = 0; t < n_tris; ++t) {
            const int32_t c = cell_of[(size_t)tris[3 * t]];       // (a row without finite coordinates is in no cell, and in no window)
            if (c >= 0) ++ct->h_starts[(size_t)c + 1];
        }
        for (size_t c = 0; c < cells; ++c) ct->h_starts[c + 1] += ct->h_starts[c];
        ct->n_binned = (int64_t)ct->h_starts[cells];
        order.resize((size_t)ct->n_binned);
        std::vector<unsigned> at(ct->h_starts.begin(), ct->h_starts.end() - 1);
        for (int64_t t = 0; t < n_tris; ++t) {
            const int32_t c = cell_of[(size_t)tris[3 * t]];
            if (c >= 0) order[at[(size_t)c]++] = (int32_t)t;
        }
    }
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ct->tris), (size_t)std::max<int64_t>(n_tris, 1) * 12));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ct->order), (size_t)std::max<int64_t>(ct->n_binned, 1) * sizeof(int32_t)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ct->starts), ct->h_starts.size() * sizeof(unsigned)));
    if (n_tris) HIP_TRY(ctx, hipMemcpyAsync(ct->tris, tris, (size_t)n_tris * 12, hipMemcpyHostToDevice, ctx->stream));
    if (ct->n_binned) HIP_TRY(ctx, hipMemcpyAsync(ct->order, order.data(), (size_t)ct->n_binned * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ct->starts, ct->h_starts.data(), ct->h_starts.size() * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_caller_tris_destroy(same_caller_tris *ct) {
    if (!ct) return;
    (void)hipSetDevice(ct->ctx->device);
    (void)hipDeviceSynchronize();                 // windows of other contexts may still be reading it
    if (ct->tris) (void)hipFree(ct->tris);
    if (ct->order) (void)hipFree(ct->order);
    if (ct->starts) (void)hipFree(ct->starts);
    delete ct;
}

int same_window_caller_tris(same_window *const *windows, int n_windows, const same_caller_tris *ct, const uint8_t *removed,
                            const int64_t *removed_offsets, double radius, int angle_enabled, double cos_thr, double near_tol,
                            int ignore_same_type, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, ct && out_counts && ct->ctx->device == ctx->device && !removed == !removed_offsets);
    for (int i = 0; i < n_windows; ++i) {
        const same_window *w = windows[i];
        REQUIRE(ctx, w->may_select() && w->mov == ct->mov);
        if (removed) {
            const int64_t n0 = w->caller_ok ? w->st0.n_ua : w->cur.n_ua;
            REQUIRE(ctx, (i > 0 || removed_offsets[0] == 0) && removed_offsets[i + 1] - removed_offsets[i] == n0);
        }
    }
    for (int q = 0; q < 6 * n_windows; ++q) out_counts[q] = 0;
    SAME_TRY(same_use(ctx));
    const bool prefiltered = removed != nullptr;
    std::vector<CallerPlan> plans((size_t)n_windows);
    std::vector<uint8_t> stays;                   // the host's mask turned round: one byte per kept cell, non-zero = it stays
    if (prefiltered) {
        stays.resize((size_t)removed_offsets[n_windows]);
        for (size_t q = 0; q < stays.size(); ++q) stays[q] = removed[q] ? 0 : 1;
    }
    int rc = SAME_OK;
    std::vector<int> live;
    {
        same_section *s = const_cast<same_section *>(ct->mov);
        std::shared_lock<std::shared_mutex> hold(s->grid_lock);
        const BinGrid &g = s->grid, &h = ct->grid;
        REQUIRE(ctx, g.x0 == h.x0 && g.y0 == h.y0 && g.cw == h.cw && g.ch == h.ch && g.nx == h.nx && g.ny == h.ny);
        for (int i = 0; i < n_windows && rc == SAME_OK; ++i) {
            same_window *w = windows[i];
            if ((w->caller_ok ? w->st0.n_ua : w->cur.n_ua) == 0) continue;     // no kept cell: nothing to select, nothing to remove
            const bool use_type = ignore_same_type && w->has_type;
            rc = prepare_caller(w, ct, use_type, &plans[(size_t)i]);
            if (rc == SAME_OK) live.push_back(i);
        }
    }
    // ONE wait for the batch: per group the zeroing, (the host's masks,) the kernels; then every window's counts, kept XY and kept rows
    // into the head of its pinned block, where the stage call left the staged ones
    if (rc == SAME_OK)
        rc = for_each_group(plans, live, [&](CallerPlan *const *cps, const int *at, int n_g) {
            ZeroArgs zr[SAME_LAUNCH_WINDOWS];
            for (int q = 0; q < n_g; ++q) zr[q] = cps[q]->zero;
            SAME_TRY(launch_zero(ctx, zr, n_g));
            for (int q = 0; q < n_g && prefiltered; ++q) {
                hipError_t e = hipMemcpyAsync(cps[q]->a.valid, stays.data() + removed_offsets[at[q]], (size_t)cps[q]->a.n0, hipMemcpyHostToDevice, ctx->stream);
                ++ctx->stats[SAME_STAT_COPIES];
                if (e != hipSuccess) return same_fail(ctx, SAME_EIO, "node mask", e);
            }
            SAME_TRY(launch_caller(ctx, cps, n_g, !prefiltered, radius, angle_enabled, cos_thr, near_tol));
            Back back[SAME_LAUNCH_WINDOWS];
            for (int q = 0; q < n_g; ++q) back[q] = Back{windows[at[q]], cps[q]->next.counts, cps[q]->back_bytes};
            return copy_back_group(ctx, back, n_g, "caller triangulation copy back");
        });
    if (rc != SAME_OK) return fail_batch(ctx, windows, live, rc);
    if (!live.empty()) SAME_WAIT(ctx);
    bool restored = false;
    for (int i : live) {
        same_window *w = windows[i];
        CallerPlan &cp = plans[(size_t)i];
        const unsigned long long *tot = static_cast<const unsigned long long *>(w->host);
        int64_t *counts = out_counts + 6 * i;
        const int64_t n_ua = (int64_t)tot[2], P = (int64_t)tot[3], n_left = (int64_t)tot[4], n_sel = (int64_t)tot[5], near = (int64_t)tot[6];
        REQUIRE(ctx, n_ua <= w->st0.n_ua && P <= w->st0.list.P && n_left <= n_sel && n_sel <= cp.a.n_cand && (int64_t)tot[7] == w->st0.n_ua - n_ua);
        w->selected(n_sel);
        counts[0] = n_sel;
        counts[1] = (int64_t)tot[7];
        counts[2] = near;
        if (near) {
            // a cosine at the threshold: the mask is the host's to make.  The window stays as staged -- and its pinned block gets the
            // staged counts, XY and rows back (the second call starts from there)
            counts[3] = w->st0.n_ua;
            counts[4] = w->st0.list.P;
            counts[5] = 0;
            const Back staged{w, w->st0.counts, cp.back_bytes};
            SAME_TRY(copy_back_group(ctx, &staged, 1, "caller triangulation copy back", true));
            restored = true;
            continue;
        }
        cp.next.n_ua = n_ua;
        cp.next.list.P = P;
        w->compacted(cp.next, n_left);
        w->held.valid = cp.a.valid;               // what a k-NN prefix holds on to (held.on stays 0: the window IS the compacted one)
        w->held.newidx = cp.a.newidx;
        w->held.st = cp.a.st_cell;
        w->held.back_bytes = cp.back_bytes;
        w->held.cap = cp.pair_cap;
        counts[3] = n_ua;
        counts[4] = P;
        counts[5] = n_left;
    }
    if (restored) SAME_WAIT(ctx);
    return SAME_OK;
}

int same_window_caller_pairs(same_window *const *windows, int n_windows, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, out_counts);
    for (int i = 0; i < n_windows; ++i) {
        const same_window *w = windows[i];
        REQUIRE(ctx, w->may_push_pairs());
        // a held selection -- or a window without kept cells, which same_window_caller_tris had nothing to select for either
        REQUIRE(ctx, w->held.on ? (w->cur.n_ua > 0 && w->cur.list.P <= w->held.cap && w->held.cs.n_ua <= w->cur.n_ua) : w->cur.n_ua == 0);
    }
    for (int q = 0; q < 6 * n_windows; ++q) out_counts[q] = 0;
    SAME_TRY(same_use(ctx));
    std::vector<PairsPlan> plans((size_t)n_windows);
    std::vector<int> live;
    for (int i = 0; i < n_windows; ++i)
        if (windows[i]->held.on) {
            prepare_pairs(windows[i], &plans[(size_t)i]);
            live.push_back(i);
        }
    // ONE wait for the batch: per group the zeroing and the two kernels; then every window's counts, kept XY and kept rows -- the
    // compacted window's, still in `caller` -- into the head of its pinned block, where the prefix call put the staged ones
    const int rc = for_each_group(plans, live, [&](PairsPlan *const *pps, const int *at, int n_g) {
        SAME_TRY(launch_pairs(ctx, pps, n_g));
        Back back[SAME_LAUNCH_WINDOWS];
        for (int q = 0; q < n_g; ++q) back[q] = Back{windows[at[q]], windows[at[q]]->held.cs.counts, windows[at[q]]->held.back_bytes};
        return copy_back_group(ctx, back, n_g, "caller pairs copy back");
    });
    if (rc != SAME_OK) return fail_batch(ctx, windows, live, rc);
    if (!live.empty()) SAME_WAIT(ctx);
    for (int i : live) {
        const same_window *w = windows[i];
        const unsigned long long *tot = static_cast<const unsigned long long *>(w->host);
        REQUIRE(ctx, (int64_t)tot[2] == w->held.cs.n_ua && (int64_t)tot[3] <= w->cur.list.P && (int64_t)tot[3] <= w->held.cap &&
                         (int64_t)tot[4] == w->n_caller && (int64_t)tot[7] == w->cur.n_ua - w->held.cs.n_ua);
    }
    for (int i : live) {
        same_window *w = windows[i];
        const unsigned long long *tot = static_cast<const unsigned long long *>(w->host);
        // as prepare_caller and the end of same_window_caller_tris leave it: st0 the arrays the removal started from
        w->st0 = w->cur;
        View cs = w->held.cs;
        cs.list.P = (int64_t)tot[3];
        w->compacted(cs, w->n_caller);
        int64_t *counts = out_counts + 6 * i;
        counts[0] = w->n_sel;
        counts[1] = w->st0.n_ua - cs.n_ua;
        counts[3] = cs.n_ua;
        counts[4] = cs.list.P;
        counts[5] = w->n_caller;
    }
    return SAME_OK;
}

}  // extern "C"
