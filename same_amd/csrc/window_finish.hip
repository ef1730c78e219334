// window_finish.hip -- same_window_filter_finish: per window the Delaunay simplices in; triangle classes (src/helpers.py:300-330),
// the keep list and the same-type triangles added back so that every node keeps one (src/helpers.py:331-340, :365-389) -- all on the
// device, in the reference's order (a cosine within 8 ulp of the angle threshold is left to the host, which re-decides it with the
// reference's literal arccos and calls again with SAME_TRIS_KEPT: the kept triangles in, no filter); source signs / weights
// (src/same.py:1128-1146), per-row minimum and the greedy MIP start (src/init_helpers.py:104-133) or the optimal assignment (assign.hip),
// optionally refined against the model's flip penalty (refine.hip), the lazy-constraint body under the result (src/same.py:645-669),
// XY-order sweep (src/violationhelper.py:53-117), signed-area flips (src/same.py:1362-1402).  The mode is the call's arguments.
// Back to the host: the matched reference row per kept aligned cell, the per-cell violation flags and a stats record per window.
#include "assign.h"
#include "refine.h"

namespace {

using namespace devmath;
using namespace win;
using scan::Pair;

// ---- triangle filter (src/helpers.py:233-395) on the device ------------------------------------------------------------------
// The filter's kernels take the windows of a batch in one launch each (Batch<FilterArgs>, blockIdx.y = window).  The filter settings
// are the call's: the same for every window.
struct FilterArgs {
    const double *xy;                  // kept aligned cells' XY
    const int32_t *raw;                // the triangulation's simplices
    int64_t Tr, n;                     // triangles, kept aligned cells
    const int32_t *type_id;            // or null
    uint8_t *cls;
    double *perim;
    uint8_t *has_kept, *any_valid;
    unsigned long long *best_p;        // or null (no re-adding)
    unsigned *best_t, *first_v;
    unsigned long long *st_keep, *st_own, *counters;
    int32_t *klist, *nlist, *out;
};

// classes; vertices with a kept triangle, vertices with any valid (kept or same-type) triangle; knife-edge cosines
__global__ __launch_bounds__(256) void filter_classify_kernel(Batch<FilterArgs> b, double radius, int angle_enabled, double cos_thr, int near_enabled,
                                                               double tol) {
    const FilterArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= w.Tr) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t *__restrict__ tris = w.raw, *__restrict__ type_id = w.type_id;
    bool near = false;
    if (t < w.Tr) {
        const int32_t a = tris[3 * t], bb = tris[3 * t + 1], d = tris[3 * t + 2];
        const TriClass r = classify_triangle(ld2(w.xy, a), ld2(w.xy, bb), ld2(w.xy, d), radius, angle_enabled, cos_thr,
                                             type_id && type_id[a] == type_id[bb] && type_id[bb] == type_id[d]);
        w.cls[t] = r.cls;
        w.perim[t] = r.perim;
        near = near_enabled && r.cls != 1 && fabs(r.maxcos - cos_thr) <= tol;
        if (r.cls == 0 || r.cls == 3) {
            w.any_valid[a] = 1; w.any_valid[bb] = 1; w.any_valid[d] = 1;
            if (r.cls == 0) { w.has_kept[a] = 1; w.has_kept[bb] = 1; w.has_kept[d] = 1; }
        }
        // best same-type triangle of every vertex, first pass (src/helpers.py:334-340): the smallest perimeter, as an atomic maximum
        // over the INVERTED bit pattern (perimeters are >= 0: the order of the bits is theirs; zero = none yet, one fill prepares it)
        if (w.best_p && r.cls == 3) {
            const unsigned long long key = ~(unsigned long long)__double_as_longlong(r.perim);
            atomicMax(&w.best_p[a], key); atomicMax(&w.best_p[bb], key); atomicMax(&w.best_p[d], key);
        }
    }
    const unsigned long long nb = __ballot(near);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&w.counters[FC_NEAR], (unsigned long long)__builtin_popcountll(nb));
}
// the kept (class 0) triangles in order; and, second pass of the best same-type triangle: the first triangle in input order among
// a vertex's equal smallest perimeters (an atomic maximum of the inverted triangle index)
__global__ __launch_bounds__(scan::NT) void filter_keep_kernel(Batch<FilterArgs> b) {
    __shared__ scan::Shared sh;
    const FilterArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.Tr);
    if ((int)blockIdx.x >= nb || w.Tr == 0) return;
    const int64_t Tr = w.Tr;
    const uint8_t *__restrict__ cls = w.cls;
    auto val = [&](int64_t t) { return Pair{t < Tr && cls[t] == 0 ? 1u : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st_keep, (int)blockIdx.x, val, sh, &through);
    const int64_t t = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (t < Tr) {
        const uint8_t c = cls[t];
        if (c == 0) w.klist[off.a] = (int32_t)t;
        if (w.best_p && c == 3) {
            const unsigned long long key = ~(unsigned long long)__double_as_longlong(w.perim[t]);
            for (int q = 0; q < 3; ++q) {
                const int32_t v = w.raw[3 * t + q];
                if (w.best_p[v] == key) atomicMax(&w.best_t[v], ~(unsigned)t);
            }
        }
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) w.counters[FC_KEEP] = through.a;
}
// nodes without a kept triangle but with a valid one are walked in ascending order and bring their best triangle along unless an
// earlier node already did (src/helpers.py:365-389): first_v[t] = the first node that asks for t (inverted, zero = nobody) ...
__device__ __forceinline__ bool asks(const uint8_t *has_kept, const uint8_t *any_valid, const unsigned *best_t, int64_t v) {
    return !has_kept[v] && any_valid[v] && best_t[v] != 0u;
}
__global__ __launch_bounds__(256) void filter_first_node_kernel(Batch<FilterArgs> b) {
    const FilterArgs &w = b.w[blockIdx.y];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= w.n || !asks(w.has_kept, w.any_valid, w.best_t, v)) return;
    atomicMax(&w.first_v[~w.best_t[v]], ~(unsigned)v);
}
// ... and the nodes that are the first to ask, compacted in order
__global__ __launch_bounds__(scan::NT) void filter_owner_kernel(Batch<FilterArgs> b) {
    __shared__ scan::Shared sh;
    const FilterArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n);
    if ((int)blockIdx.x >= nb || w.n == 0) return;
    const int64_t n = w.n;
    auto own = [&](int64_t v) { return v < n && asks(w.has_kept, w.any_valid, w.best_t, v) && w.first_v[~w.best_t[v]] == ~(unsigned)v; };
    auto val = [&](int64_t v) { return Pair{own(v) ? 1u : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(w.st_own, (int)blockIdx.x, val, sh, &through);
    const int64_t v = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (own(v)) w.nlist[off.a] = (int32_t)v;
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) w.counters[FC_ADD] = through.a;
}
// the kept triangles in the reference's order: class-0 triangles ascending, then the added-back ones in walk order
__global__ __launch_bounds__(256) void filter_emit_kernel(Batch<FilterArgs> b) {
    const FilterArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= w.Tr) return;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_keep = (int64_t)w.counters[FC_KEEP], n_add = (int64_t)w.counters[FC_ADD];
    if (q == 0) w.counters[FC_TR] = (unsigned long long)(n_keep + n_add);
    // ORDER TIES (FC_TIES, SC_TIES): places where the reference's answer depends on the ORDER Qhull lists triangles or their corners
    // in, not only on which triangles there are -- counted so that a caller whose triangulation is not Qhull's (same_delaunay2d) knows
    // when to ask Qhull after all.  Here: a node that asks for its best same-type triangle and has a second one whose perimeter is
    // within the rounding of a three-term sum (the sum's order is the corners' order; equal perimeters go to the first triangle)
    if (w.best_p && q < w.Tr && w.cls[q] == 3) {
        bool tie = false;
        for (int c = 0; c < 3; ++c) {
            const int32_t v = w.raw[3 * q + c];
            if (!asks(w.has_kept, w.any_valid, w.best_t, v)) continue;
            const int64_t best = (int64_t)~w.best_t[v];
            tie |= best != q && fabs(w.perim[q] - w.perim[best]) <= 1.8e-15 * w.perim[best];
        }
        if (tie) atomicAdd(&w.counters[FC_TIES], 1ull);
    }
    if (q >= n_keep + n_add) return;
    const int64_t t = q < n_keep ? w.klist[q] : (int64_t)~w.best_t[w.nlist[q - n_keep]];
    w.out[3 * q] = w.raw[3 * t];
    w.out[3 * q + 1] = w.raw[3 * t + 1];
    w.out[3 * q + 2] = w.raw[3 * t + 2];
}

// ---- incumbent and sweeps ---------------------------------------------------------------------------------------------------

constexpr int WINDOW_GREEDY_ROUNDS = 3;   // rounds enqueued before the first look (cfg 5: 1-3 productive rounds per window)

// The finish call's kernels take the windows of a batch in one launch each too (Batch<A>, blockIdx.y = window).
// per kept aligned row: minimum pair cost (src/init_helpers.py:118-122; its pairs are a contiguous run of the pair list), whether
// it beats the no-match penalty, the row's pairs enter the greedy rule or not, no match yet
struct PreferArgs {
    const int32_t *prow;
    const double *cost64, *size_c;
    const unsigned long long *dn;
    uint8_t *alive;
    int32_t *match_pair;
    int64_t cap;               // the host's count of kept rows (sizes the launch; *dn is the same number on the device)
};
__global__ __launch_bounds__(256) void row_prefer_kernel(Batch<PreferArgs> b, double penalty) {
    const PreferArgs &w = b.w[blockIdx.y];
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= w.cap || a >= (int64_t)*w.dn) return;
    const int32_t lo = w.prow[a], hi = w.prow[a + 1];
    double best = __builtin_inf();
    for (int32_t p = lo; p < hi; ++p) {
        const double c = w.cost64[p];
        if (c < best) best = c;
    }
    const uint8_t prefer = best < penalty * w.size_c[a];
    for (int32_t p = lo; p < hi; ++p) w.alive[p] = prefer;
    w.match_pair[a] = -1;
}
// pair per row -> matched reference cell: its number in the window (handed out), its section row (the sweeps and the caller); and
// whether the greedy rule is finished: a pair still alive whose end points are both free would be taken by a further round.  The
// rows' pairs are `final_pair` (the local search's result, or the incumbent itself); the greedy rule's state is the incumbent's
struct MatchRowsArgs {
    const int32_t *match_pair, *final_pair, *pairs, *jsec, *prow;
    const uint8_t *alive, *used;
    int64_t n_rows;
    const unsigned long long *dn;
    int32_t *match_loc, *match_row;
    uint8_t *pflag;
    unsigned long long *counters;
};
__global__ __launch_bounds__(256) void match_rows_kernel(Batch<MatchRowsArgs> b) {
    const MatchRowsArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= w.n_rows) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    int open = 0;
    if (i < (int64_t)*w.dn) {
        const int32_t p = w.final_pair[i];
        w.match_loc[i] = p >= 0 ? w.pairs[2 * (int64_t)p + 1] : -1;
        w.match_row[i] = p >= 0 ? w.jsec[p] : -1;
        w.pflag[i] = 0;
        m = p >= 0;
        if (w.match_pair[i] < 0 && !w.used[i])
            for (int32_t q = w.prow[i]; q < w.prow[i + 1]; ++q) open += w.alive[q] && !w.used[w.n_rows + w.pairs[2 * (int64_t)q + 1]];
    }
    const unsigned long long bal = __ballot(m), ob = __ballot(open != 0);
    if ((threadIdx.x & 63) == 0) {
        if (bal) atomicAdd(&w.counters[SC_MATCHED], (unsigned long long)__builtin_popcountll(bal));
        if (ob) atomicAdd(&w.counters[SC_REMAINING], (unsigned long long)__builtin_popcountll(ob));
    }
}
// per-cell flag byte: bit 0 = the XY-order sweep flags the cell (src/violationhelper.py:100-104), bit 1 = the cell is a vertex of a
// triangle whose signed area flips (src/same.py:1464-1469).  Two kinds of writers share a byte, so they OR into its 32-bit word
// (the array is word-aligned and padded to whole words by its carver; flagged cells are the exception, not the rule).
__device__ __forceinline__ void cell_flag_or(uint8_t *flags, int32_t i, unsigned bit) {
    atomicOr(reinterpret_cast<unsigned *>(flags) + (i >> 2), bit << (8 * (i & 3)));
}
// one pass over the kept triangles: source sign and weight (src/same.py:1128-1146), the lazy-constraint body under the incumbent
// (:645-669), the XY-order sweep (src/violationhelper.py:53-117), the signed-area flip (src/same.py:1362-1402; helpers.py:73-77)
struct SweepArgs {
    const int32_t *tris;
    int64_t Tr;                        // the number of triangles, or (dTr != null) the bound the launch is sized by
    const unsigned long long *dTr;
    const double *axy, *size_c, *ref_xy;
    const int32_t *match_row;
    int8_t *sign;
    double *weight;
    uint8_t *pflag;
    unsigned long long *counters;
};
__global__ __launch_bounds__(256) void window_sweeps_kernel(Batch<SweepArgs> b) {
    const SweepArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= w.Tr) return;
    const int32_t *__restrict__ tris = w.tris;
    const double *__restrict__ axy = w.axy, *__restrict__ size_c = w.size_c, *__restrict__ ref_xy = w.ref_xy;
    const int32_t *__restrict__ match_row = w.match_row;
    int8_t *__restrict__ sign = w.sign;
    double *__restrict__ weight = w.weight;
    uint8_t *__restrict__ pflag = w.pflag;
    unsigned long long *__restrict__ counters = w.counters;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t Tr = w.dTr ? (int64_t)*w.dTr : w.Tr;
    int checked = 0, flipped = 0, ncmp = 0, nviol = 0, tv = 0, aflip = 0, ties = 0;
    if (t < Tr) {
        const int32_t v[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
        const int32_t m[3] = {match_row[v[0]], match_row[v[1]], match_row[v[2]]};
        double2_t a[3], r[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            a[q] = ld2(axy, v[q]);
            r[q] = m[q] >= 0 ? ld2(ref_xy, m[q]) : double2_t{0.0, 0.0};
        }
        const int8_t ss = orient_sign(a[0], a[1], a[2]);
        sign[t] = ss;
        weight[t] = size_c[v[0]] + size_c[v[1]] + size_c[v[2]];            // src/same.py:1131-1133
        const bool all3 = m[0] >= 0 && m[1] >= 0 && m[2] >= 0;
        const uint8_t f = orient_flag(ss, all3, r[0], r[1], r[2]);
        checked = f != 0;
        flipped = f == 2;
        const int E[3][2] = {{0, 1}, {0, 2}, {1, 2}};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int p = E[e][0], q = E[e][1];
            if (m[p] >= 0 && m[q] >= 0) {  // both matched (implies >= 2 matched vertices, violationhelper.py:58-60)
                ++ncmp;
                const uint8_t e2 = xyorder_edge(a[p], a[q], r[p], r[q]);
                // equal coordinates at an edge's ends: `<` one way round is not `<` the other way round (order tie, see filter_emit_kernel)
                ties |= a[p].x == a[q].x || a[p].y == a[q].y || r[p].x == r[q].x || r[p].y == r[q].y;
                nviol += ((e2 >> 1) & 1) + ((e2 >> 2) & 1);
                if (e2) { tv = 1; cell_flag_or(pflag, v[p], 1u); cell_flag_or(pflag, v[q], 1u); }
            }
        }
        if (all3) {
            const double bf = signed_area(a[0], a[1], a[2]), af = signed_area(r[0], r[1], r[2]);
            aflip = bf * af < 0.0;                                         // src/same.py:1401
            // a sign within rounding of zero may come out the other way with the corners in another order (order tie)
            ties |= sign_in_doubt(a[0], a[1], a[2]) || sign_in_doubt(r[0], r[1], r[2]);
            if (aflip)
                for (int q = 0; q < 3; ++q) cell_flag_or(pflag, v[q], 2u);
        }
    }
    int vals[7] = {checked, flipped, ncmp, nviol, tv, aflip, ties};
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) vals[q] += __shfl_down(vals[q], off, 64);
    __shared__ int part[4][7];
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 7; ++q) part[threadIdx.x >> 6][q] = vals[q];
    __syncthreads();
    if (threadIdx.x < 7) {      // one atomic per block per counter (integer sums: order-independent); SC_CHECKED .. SC_AFLIP, then SC_TIES
        const int s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s) atomicAdd(&counters[threadIdx.x < 6 ? threadIdx.x : SC_TIES], (unsigned long long)s);
    }
}

// ---- the filter and the finish as enqueue-only halves + their read-backs, so that the two calls can also run as one ----------
struct FilterPlan {
    FilterArgs args{};
    void *zero = nullptr;                     // head of the filter buffer, zeroed with the group's
    size_t zero_bytes = 0;
    unsigned long long *counters = nullptr;   // FC_*
    bool readd = false;
};

// A window's filter buffer laid out (d_simplices: its triangulation, on the device already); no launch, no fill -- those come per GROUP
// of windows (launch_filter, and the zeroing with the finish buffers')
int prepare_filter(same_window *w, const int32_t *d_simplices, int64_t Tr, int ignore_same_type, int ensure_min_triangle_per_node, FilterPlan *plan) {
    same_ctx *ctx = w->ctx;
    const int64_t n = w->cur.n_ua;
    const bool use_type = ignore_same_type && w->has_type;
    plan->readd = use_type && ensure_min_triangle_per_node;
    FilterArgs &a = plan->args;
    a.xy = w->cur.axy_c;
    a.raw = d_simplices;
    a.Tr = Tr;
    a.n = n;
    a.type_id = use_type ? w->cur.type_c : nullptr;
    auto lay = [&](Carver cv) {
        // zeroed head: scan words, counters, vertex marks, inverted minima
        a.st_keep = scan::arg(cv.scan_words(Tr));
        a.st_own = scan::arg(cv.scan_words(n));
        a.counters = plan->counters = cv.take<unsigned long long>(8);
        a.has_kept = cv.take<uint8_t>((size_t)n);
        a.any_valid = cv.take<uint8_t>((size_t)n);
        a.best_p = cv.take<unsigned long long>((size_t)n);
        if (!plan->readd) a.best_p = nullptr;
        a.best_t = cv.take<unsigned>((size_t)n);
        a.first_v = cv.take<unsigned>((size_t)Tr);
        plan->zero_bytes = cv.off;
        a.cls = cv.take<uint8_t>((size_t)Tr);
        a.perim = cv.take<double>((size_t)Tr);
        a.klist = cv.take<int32_t>((size_t)Tr);
        a.nlist = cv.take<int32_t>((size_t)n);
        return cv.off;
    };
    SAME_TRY(ensure(ctx, w->filter, lay(Carver())));
    SAME_TRY(ensure(ctx, w->tris, (size_t)std::max<int64_t>(Tr, 1) * 12));
    lay(Carver(w->filter.p));
    a.out = static_cast<int32_t *>(w->tris.p);
    plan->zero = w->filter.p;
    return SAME_OK;
}

// the filter of a group of prepared windows (<= SAME_LAUNCH_WINDOWS; the settings are the call's, `readd` follows from them and from
// the moving section, so it is the group's): three launches, five when same-type triangles come back
int launch_filter(same_ctx *ctx, FilterPlan *const *plans, int n_w, double radius, int angle_enabled, double cos_thr, double near_tol) {
    Batch<FilterArgs> b{};
    int64_t max_tr = 0, max_n = 0;
    for (int q = 0; q < n_w; ++q) {
        b.w[q] = plans[q]->args;
        max_tr = std::max(max_tr, plans[q]->args.Tr);
        max_n = std::max(max_n, plans[q]->args.n);
    }
    const unsigned nw = (unsigned)n_w;
    const int near_enabled = angle_enabled && cos_thr == cos_thr && cos_thr - cos_thr == 0.0;       // a finite threshold
    SAME_LAUNCH(ctx, filter_classify_kernel, dim3(grid_for(max_tr), nw), dim3(256), 0, b, radius, angle_enabled, cos_thr, near_enabled, near_tol);
    SAME_LAUNCH(ctx, filter_keep_kernel, dim3(scan::blocks_for(max_tr), nw), dim3(scan::NT), 0, b);
    if (plans[0]->readd) {
        SAME_LAUNCH(ctx, filter_first_node_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, b);
        SAME_LAUNCH(ctx, filter_owner_kernel, dim3(scan::blocks_for(max_n), nw), dim3(scan::NT), 0, b);
    }
    SAME_LAUNCH(ctx, filter_emit_kernel, dim3(grid_for(max_tr), nw), dim3(256), 0, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

// what a finish call matches by and does after the incumbent: the call's arguments, the same for every window of it
struct FinishMode {
    int incumbent = SAME_INCUMBENT_GREEDY;
    double no_match_penalty = 0.0;
    int64_t refine_cap = 0;                   // local search rounds at most (refine.hip), 0 = no search
    double delaunay_penalty = 0.0;
    bool capacity = false;                    // the search with the model's reference capacities (the _cap calls) ...
    same_window_capacity cap{1, 0, 0.0};      // ... these (the transport start's too)
    bool has_cap = false;                     // the call brought a capacity (the transport start needs one)
    int stride = SAME_WINDOW_STATS;           // int64 words per window in out_stats
};
int check_mode(same_ctx *ctx, const FinishMode &m) {
    REQUIRE(ctx, m.incumbent == SAME_INCUMBENT_GREEDY || m.incumbent == SAME_INCUMBENT_ASSIGNMENT ||
                     (m.incumbent == SAME_INCUMBENT_TRANSPORT && m.has_cap));
    REQUIRE(ctx, m.refine_cap >= 0 && m.delaunay_penalty >= 0.0 && m.delaunay_penalty - m.delaunay_penalty == 0.0);
    REQUIRE(ctx, m.cap.max_matches >= 1 && m.cap.multiplier >= 0 && m.cap.penalty_coeff >= 0.0 &&
                     m.cap.penalty_coeff - m.cap.penalty_coeff == 0.0);
    return SAME_OK;
}
FinishMode mode_of(int incumbent, double no_match_penalty, int64_t refine_rounds_cap, double delaunay_penalty,
                   const same_window_capacity *capacity, bool wide) {
    FinishMode m{incumbent, no_match_penalty, refine_rounds_cap, delaunay_penalty};
    m.capacity = capacity != nullptr && refine_rounds_cap > 0;
    if (capacity) m.cap = *capacity;
    m.has_cap = capacity != nullptr;
    m.stride = !wide ? SAME_WINDOW_STATS : incumbent == SAME_INCUMBENT_TRANSPORT ? SAME_WINDOW_STATS_TRANSPORT : SAME_WINDOW_STATS_CAP;
    return m;
}
// words of a window's out_stats record after the eight counters: the assignment's flags and objective, the search's record, the
// transport start's sum_j max(0, count_j - 1)
enum { WS_AS_FLAGS = 8, WS_AS_OBJ = 9, WS_REFINE = 10, WS_AS_EXTRA = 16 };

// (FinishBack: the head's zeroed length, the block that comes back and its parts -- window_internal.h)
struct FinishPlan : FinishBack {
    FinishMode mode;
    unsigned long long *zero = nullptr;       // head of the finish buffer: [used | keys | sel | counters | point flags (padded)], then the matched rows
    void *filter_zero = nullptr;              // head of the window's filter buffer when this call filters it (zeroed in the same launch)
    size_t filter_zero_bytes = 0;
    same_greedy_state gs;
    int32_t *match_pair = nullptr;
    int64_t cap_tr = 0;
    const unsigned long long *dTr = nullptr;
    asg::AssignArgs aargs{};                  // the optimal assignment's work arrays (SAME_INCUMBENT_ASSIGNMENT), else unset
    bool refine = false;                      // the local search runs on the incumbent (mode.refine_cap > 0) ...
    rfn::RefineArgs rargs{};                  // ... over these arrays; its control words are counters + SC_REFINE
};

// match rows + the one pass over the triangles, for a group of windows (<= SAME_LAUNCH_WINDOWS) in one launch each
int enqueue_tail(same_ctx *ctx, same_window *const *ws, FinishPlan *const *ps, int n_w) {
    Batch<MatchRowsArgs> mb{};
    Batch<SweepArgs> sb{};
    int64_t max_n = 0, max_tr = 0;
    for (int q = 0; q < n_w; ++q) {
        same_window *w = ws[q];
        FinishPlan *p = ps[q];
        const int64_t n = w->cur.n_ua;
        mb.w[q] = MatchRowsArgs{p->match_pair, p->refine ? p->rargs.match : p->match_pair, w->cur.list.pairs, w->cur.list.jsec, w->cur.list.prow, p->gs.alive, p->gs.used, n, w->cur.counts + 2, w->match_loc, p->match_row, p->pflag,
                                p->counters};
        sb.w[q] = SweepArgs{static_cast<const int32_t *>(w->tris.p), p->cap_tr, p->dTr, w->cur.axy_c, w->cur.size_c, w->ref->xy, p->match_row, w->sign, w->weight,
                            p->pflag, p->counters};
        max_n = std::max(max_n, n);
        max_tr = std::max(max_tr, p->cap_tr);
    }
    if (max_n) SAME_LAUNCH(ctx, match_rows_kernel, dim3(grid_for(max_n), (unsigned)n_w), dim3(256), 0, mb);
    if (max_tr) SAME_LAUNCH(ctx, window_sweeps_kernel, dim3(grid_for(max_tr), (unsigned)n_w), dim3(256), 0, sb);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

// A window's finish buffer laid out, its triangles uploaded (prefiltered form); no launch, no fill -- those come per GROUP of windows
// (launch_finish; p->zero / p->zero_bytes name the head to zero).  cap_tr: the number of triangles, or (dTr != null) the bound the launch is sized by with the number itself on the device
int prepare_finish(same_window *w, const int32_t *host_tris, int64_t cap_tr, const unsigned long long *dTr, const FinishMode &mode,
                   FinishPlan *p) {
    same_ctx *ctx = w->ctx;
    const int64_t n = w->cur.n_ua, P = w->cur.list.P, n_ends = n + w->n_r;
    const size_t tt = (size_t)std::max<int64_t>(cap_tr, 1);
    p->mode = mode;
    p->cap_tr = cap_tr;
    p->dTr = dTr;
    p->gs.float_costs = w->cost_f32 != 0;          // cost64 = (double)float there: the two-launch rounds
    p->aargs = asg::AssignArgs{};
    p->aargs.n = n;
    p->aargs.n_r = w->n_r;
    p->aargs.transport = mode.incumbent == SAME_INCUMBENT_TRANSPORT;
    p->aargs.pc = mode.cap.penalty_coeff;
    p->refine = mode.refine_cap > 0;
    rfn::RefineArgs &r = p->rargs;
    r = rfn::RefineArgs{};
    r.n = n;
    r.n_r = w->n_r;
    r.cap_tr = cap_tr;
    auto lay = [&](Carver cv) {
        p->gs.used = cv.take<uint8_t>((size_t)n_ends);
        p->gs.key[0] = cv.take<unsigned long long>((size_t)n_ends * 2);
        p->gs.idx[0] = cv.take<unsigned>((size_t)n_ends * 2);
        win::lay(*p, cv, n);            // sel, counters, point flags, matched rows: contiguous, they come back in one copy
        p->gs.sel = p->sel;
        p->gs.alive = cv.take<uint8_t>((size_t)std::max<int64_t>(P, 1));
        p->match_pair = cv.take<int32_t>((size_t)n);
        w->match_loc = cv.take<int32_t>((size_t)n);
        w->sign = cv.take<int8_t>(tt);
        w->weight = cv.take<double>(tt);
        if (mode.incumbent != SAME_INCUMBENT_GREEDY) asg::lay(p->aargs, cv);
        if (p->refine) rfn::lay(r, cv);
        return cv.off;
    };
    SAME_TRY(ensure(ctx, w->finish, lay(Carver())));
    SAME_TRY(ensure(ctx, w->tris, tt * 12));
    lay(Carver(w->finish.p));
    p->zero = static_cast<unsigned long long *>(w->finish.p);
    p->gs.key[1] = p->gs.key[0] + n_ends;
    p->gs.idx[1] = p->gs.idx[0] + n_ends;
    w->match_row = p->match_row;
    w->pflag = p->pflag;
    if (p->refine) {
        r.prow = w->cur.list.prow;
        r.pairs = w->cur.list.pairs;
        r.cost = w->cur.list.cost64;
        r.size = w->cur.size_c;
        r.dp = mode.delaunay_penalty;
        r.axy = w->cur.axy_c;
        r.ref_xy = w->ref->xy;
        r.ref_row = w->cur.list.jsec;
        r.tris = static_cast<const int32_t *>(w->tris.p);
        r.dTr = dTr;
        r.cap = mode.refine_cap;
        r.penalty = mode.no_match_penalty;
        if (mode.capacity) {            // the limits from the reference section's sizes (refine_limit_kernel), pricing the extra matches
            r.pc = mode.cap.penalty_coeff;
            r.rsize = w->ref->size;
            r.ref_rows = w->rows_r;
            r.P = P;
            r.lim_row = w->as_staged().jsec;
            r.lim_P = w->as_staged().P;
            r.max_matches = mode.cap.max_matches;
            r.multiplier = mode.cap.multiplier;
        }
        r.start = p->match_pair;
        r.ctrl = p->counters + SC_REFINE;
    }
    REQUIRE(ctx, w->host_finish_off + p->back_bytes <= w->host_filter_off);   // sized by the stage call
    if (host_tris && cap_tr) SAME_COPY(ctx, w->tris.p, host_tris, (size_t)cap_tr * 12, hipMemcpyHostToDevice);
    return SAME_OK;
}

// the local search from the incumbent, for the windows of a group that ask for it: setup and the first rounds (refine.hip)
int enqueue_refine(same_ctx *ctx, FinishPlan *const *ps, int n_w) {
    rfn::RefineArgs jobs[SAME_LAUNCH_WINDOWS];
    int k = 0;
    for (int q = 0; q < n_w; ++q)
        if (ps[q]->refine) jobs[k++] = ps[q]->rargs;
    if (k == 0) return SAME_OK;
    SAME_TRY(rfn::launch_setup(ctx, jobs, k));
    return rfn::launch_rounds(ctx, jobs, k, rfn::FIRST_ROUNDS);
}

// greedy MIP start of a group of prepared windows -- per-row minimum, rows that beat their penalty, the scan's matching (one pair per
// aligned row) -- and the tail: one launch per kernel for the whole group (windows of one batch call share the cost type and the mode)
int launch_finish(same_ctx *ctx, same_window *const *ws, FinishPlan *const *ps, int n_w) {
    const double no_match_penalty = ps[0]->mode.no_match_penalty;
    if (ps[0]->mode.incumbent != SAME_INCUMBENT_GREEDY) {
        // the optimal assignment instead (assign.hip): it writes match_pair, clears the pairs' greedy flags, and leaves searches, flags
        // and objective in the head of `sel` (the greedy rounds' words, unused here), which comes back with the finish block.  The
        // transport form: within the windows' reference limits, which the search's limits kernel works out first
        const bool transport = ps[0]->mode.incumbent == SAME_INCUMBENT_TRANSPORT;
        asg::AssignArgs jobs[SAME_LAUNCH_WINDOWS];
        if (transport) {
            rfn::RefineArgs lim[SAME_LAUNCH_WINDOWS];
            for (int q = 0; q < n_w; ++q) {
                const same_window *w = ws[q];
                const same_window_capacity &c = ps[q]->mode.cap;
                rfn::RefineArgs &r = lim[q];
                r = rfn::RefineArgs{};
                r.rsize = w->ref->size;
                r.ref_row = w->cur.list.jsec;
                r.ref_rows = w->rows_r;
                r.P = w->cur.list.P;
                r.lim_row = w->as_staged().jsec;
                r.lim_P = w->as_staged().P;
                r.n_r = w->n_r;
                r.max_matches = c.max_matches;
                r.multiplier = c.multiplier;
                r.limit = ps[q]->aargs.limit;
            }
            SAME_TRY(rfn::launch_limits(ctx, lim, n_w));
        }
        for (int q = 0; q < n_w; ++q) {
            same_window *w = ws[q];
            FinishPlan *p = ps[q];
            asg::AssignArgs &a = jobs[q];
            a = p->aargs;                     // n, n_r and the work arrays (prepare_finish)
            a.prow = w->cur.list.prow;
            a.pairs = w->cur.list.pairs;
            a.cost = w->cur.list.cost64;
            a.size = w->cur.size_c;
            a.penalty = no_match_penalty;
            a.max_pops = asg::default_max_pops(w->cur.n_ua, w->n_r, w->cur.list.P, transport);
            a.alive = p->gs.alive;
            a.match_pair = p->match_pair;
            a.res = p->gs.sel;
        }
        SAME_TRY(asg::launch(ctx, jobs, n_w));
        SAME_TRY(enqueue_refine(ctx, ps, n_w));
        return enqueue_tail(ctx, ws, ps, n_w);
    }
    Batch<PreferArgs> pb{};
    same_greedy_job jobs[SAME_LAUNCH_WINDOWS];
    int64_t max_n = 0;
    for (int q = 0; q < n_w; ++q) {
        same_window *w = ws[q];
        FinishPlan *p = ps[q];
        pb.w[q] = PreferArgs{w->cur.list.prow, w->cur.list.cost64, w->cur.size_c, w->cur.counts + 2, p->gs.alive, p->match_pair, w->cur.n_ua};
        jobs[q].pairs = w->cur.list.pairs;
        jobs[q].costs = w->cur.list.cost64;
        jobs[q].P = w->cur.list.P;
        jobs[q].n_m = w->cur.n_ua;
        jobs[q].n_r = w->n_r;
        jobs[q].st = p->gs;
        jobs[q].match_pair = p->match_pair;
        max_n = std::max(max_n, w->cur.n_ua);
    }
    if (max_n) SAME_LAUNCH(ctx, row_prefer_kernel, dim3(grid_for(max_n), (unsigned)n_w), dim3(256), 0, pb, no_match_penalty);
    SAME_TRY(same_greedy_rounds_batch_core(ctx, jobs, n_w, 0, WINDOW_GREEDY_ROUNDS));
    SAME_TRY(enqueue_refine(ctx, ps, n_w));
    return enqueue_tail(ctx, ws, ps, n_w);
}

// the finish call's answers: one copy (enqueue_finish_copy), a wait the CALLER makes (one for a whole batch of windows), then
// read_finish: more greedy rounds (and the tail again) when the rounds enqueued up front did not settle the matching
int enqueue_finish_copy(same_window *w, FinishPlan *p) {
    same_ctx *ctx = w->ctx;
    SAME_COPY(ctx, static_cast<char *>(w->host) + w->host_finish_off, reinterpret_cast<const char *>(p->gs.sel), p->back_bytes, hipMemcpyDeviceToHost);
    return SAME_OK;
}

// After a look at the finish block (in the pinned block): when the incumbent changed since (`fresh`: greedy rounds added), the local
// search again from it; more rounds while the search is live and under its cap, in growing chunks, one wait each; then, if any of that
// happened, the tail again and the finish block back.  The search's record goes to out_stats[WS_REFINE ..].
int settle(same_window *w, FinishPlan *p, bool fresh, int64_t *out_stats) {
    same_ctx *ctx = w->ctx;
    char *h = static_cast<char *>(w->host) + w->host_finish_off;
    const unsigned long long *rc = reinterpret_cast<const unsigned long long *>(h + p->o_counters) + SC_REFINE;
    bool redo = fresh;
    if (p->refine) {
        int chunk = rfn::FIRST_ROUNDS;
        if (fresh) {
            SAME_TRY(enqueue_refine(ctx, &p, 1));
            SAME_COPY(ctx, const_cast<unsigned long long *>(rc), p->rargs.ctrl, rfn::RC_COUNT * 8, hipMemcpyDeviceToHost);
            SAME_WAIT(ctx);
        }
        const int64_t cap = p->mode.refine_cap;
        while (!rc[rfn::RC_SETTLED] && (int64_t)rc[rfn::RC_ROUNDS] < cap) {
            chunk = (int)std::min<int64_t>(std::min(2 * chunk, 256), cap - (int64_t)rc[rfn::RC_ROUNDS]);
            SAME_TRY(rfn::launch_rounds(ctx, &p->rargs, 1, chunk));
            SAME_COPY(ctx, const_cast<unsigned long long *>(rc), p->rargs.ctrl, rfn::RC_COUNT * 8, hipMemcpyDeviceToHost);
            SAME_WAIT(ctx);
            ++ctx->stats[SAME_STAT_GREEDY_READBACKS];
            redo = true;
        }
    }
    if (redo) {
        SAME_FILL(ctx, p->counters, 0, SC_REFINE * 8);
        SAME_TRY(enqueue_tail(ctx, &w, &p, 1));
        SAME_COPY(ctx, h, reinterpret_cast<const char *>(p->gs.sel), p->back_bytes, hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
    }
    if (p->refine) {
        int64_t *rf = out_stats + WS_REFINE;
        rf[0] = (int64_t)rc[rfn::RC_ROUNDS];
        rf[1] = (int64_t)rc[rfn::RC_MOVES];
        rf[2] = (int64_t)rc[rfn::RC_SETTLED];
        rf[3] = (int64_t)rc[rfn::RC_OBJ0];          // the objectives as the bits of a double
        rf[4] = (int64_t)rc[rfn::RC_OBJ];
        if (p->mode.stride > SAME_WINDOW_STATS) rf[5] = (int64_t)rc[rfn::RC_EXTRA];   // sum_j max(0, count_j - 1)
    }
    return SAME_OK;
}

int read_finish(same_window *w, FinishPlan *p, int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats, int64_t *out_ties) {
    same_ctx *ctx = w->ctx;
    const int64_t n = w->cur.n_ua, P = w->cur.list.P;
    char *h = static_cast<char *>(w->host) + w->host_finish_off;
    const char *dsel = reinterpret_cast<const char *>(p->gs.sel);
    const unsigned long long *sel = reinterpret_cast<const unsigned long long *>(h);
    const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(h + p->o_counters);
    int rounds = 0;
    bool again = false;      // the incumbent changed after the first look
    if (p->mode.incumbent != SAME_INCUMBENT_GREEDY) {     // no greedy rounds to add: the assignment settled in its one launch
        rounds = (int)sel[0];
        out_stats[WS_AS_FLAGS] = (int64_t)sel[2];
        out_stats[WS_AS_OBJ] = (int64_t)sel[3];             // the bits of a double
        if (p->mode.incumbent == SAME_INCUMBENT_TRANSPORT) out_stats[WS_AS_EXTRA] = (int64_t)sel[4];
    } else if (P) {
        int q = 0;
        while (q < WINDOW_GREEDY_ROUNDS && sel[q] != 0) ++q;
        rounds = q;
        // every enqueued round took something AND a pair could still be taken (counted by match_rows_kernel): a long chain of pre-empting
        // pairs -- keep going in growing batches (one read per batch), then redo the tail
        if (q == WINDOW_GREEDY_ROUNDS && cnt[SC_REMAINING] != 0) {
            int batch = 4;
            for (;;) {
                REQUIRE(ctx, rounds <= P + 1);
                SAME_FILL(ctx, p->gs.sel, 0, (size_t)batch * 8);
                SAME_TRY(same_greedy_rounds_core(ctx, w->cur.list.pairs, w->cur.list.cost64, P, nullptr, n, w->n_r, p->gs, p->match_pair, rounds, batch));
                SAME_COPY(ctx, h, dsel, (size_t)batch * 8, hipMemcpyDeviceToHost);
                SAME_WAIT(ctx);
                ++ctx->stats[SAME_STAT_GREEDY_READBACKS];
                q = 0;
                while (q < batch && sel[q] != 0) ++q;
                rounds += q;
                if (q < batch) break;
                if (batch < SAME_GREEDY_BATCH_MAX) batch *= 2;
            }
            again = true;
        }
    }
    SAME_TRY(settle(w, p, again, out_stats));
    for (int q = 0; q < 8; ++q) out_stats[q] = (int64_t)cnt[q];
    out_stats[SC_ROUNDS] = rounds;
    *out_ties += (int64_t)cnt[SC_TIES];
    memcpy(out_match_row, h + p->o_match_row, (size_t)n * sizeof(int32_t));
    memcpy(out_point_flag, h + p->o_pflag, (size_t)n);
    return SAME_OK;
}

}  // namespace

static int filter_finish(same_window *const *windows, int n_windows, int source, const int32_t *simplices, const int64_t *simplex_offsets,
                         double radius, int angle_enabled, double cos_thr, double near_tol, int ignore_same_type,
                         int ensure_min_triangle_per_node, const FinishMode &mode, int32_t *out_match_row, uint8_t *out_point_flag,
                         int64_t *out_stats, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    SAME_TRY(check_mode(ctx, mode));
    REQUIRE(ctx, source == SAME_TRIS_SIMPLICES || source == SAME_TRIS_KEPT || source == SAME_TRIS_DEVICE || source == SAME_TRIS_CALLER);
    // SAME_TRIS_DEVICE: every window's simplices are the ones same_window_delaunay left on the device for it (no host array; the offsets
    // are those of its counts).  SAME_TRIS_CALLER: the caller's own triangles, as same_window_caller_tris left them over the window's cells
    const bool from_caller = source == SAME_TRIS_CALLER;
    const bool on_device = source == SAME_TRIS_DEVICE || from_caller;
    REQUIRE(ctx, on_device == !simplices && on_device == !simplex_offsets);
    std::vector<int64_t> dd_offsets;
    if (on_device) {
        dd_offsets.assign((size_t)n_windows + 1, 0);
        for (int i = 0; i < n_windows; ++i) {
            REQUIRE(ctx, windows[i]->may_finish_from(from_caller ? FROM_CALLER : FROM_DEVICE));
            dd_offsets[(size_t)i + 1] = dd_offsets[(size_t)i] + (from_caller ? windows[i]->n_caller : windows[i]->n_dd);
        }
        simplex_offsets = dd_offsets.data();
    }
    REQUIRE(ctx, out_counts && out_stats && simplex_offsets[0] == 0);
    int64_t n_cells = 0;
    for (int i = 0; i < n_windows; ++i) {
        const int64_t Tr = simplex_offsets[i + 1] - simplex_offsets[i];
        REQUIRE(ctx, windows[i]->may_finish_from(FROM_HOST) && Tr >= 0 && Tr < ((int64_t)1 << 31) - 512);
        n_cells += windows[i]->cur.n_ua;
    }
    REQUIRE(ctx, n_cells == 0 || (out_match_row && out_point_flag));
    for (int q = 0; q < 4 * n_windows; ++q) out_counts[q] = 0;
    for (int q = 0; q < mode.stride * n_windows; ++q) out_stats[q] = 0;
    SAME_TRY(same_use(ctx));
    if (!on_device)     // (the device's own triangles index the window's kept cells by construction)
        for (int i = 0; i < n_windows; ++i)
            SAME_TRY(check_index_range(ctx, simplices + 3 * simplex_offsets[i], (simplex_offsets[i + 1] - simplex_offsets[i]) * 3, 0,
                                       windows[i]->cur.n_ua, "triangles"));
    struct Item {
        FilterPlan fplan;
        FinishPlan plan;
        bool filtered = false, enqueued = false;
    };
    std::vector<Item> items((size_t)n_windows);
    // ONE wait for the batch.  The call's simplices go up in ONE copy (a scratch slot of the context: they are read by this call's filter
    // only); per window its filter and finish buffers are laid out; then per GROUP of SAME_LAUNCH_WINDOWS windows the zeroing of the
    // buffers' heads, the filter's and the finish's kernels (one launch each for the whole group); then every window's copies back
    const int32_t *d_simplices = nullptr;
    if (source == SAME_TRIS_SIMPLICES && simplex_offsets[n_windows] > 0) {
        int32_t *d = nullptr;
        SAME_TRY(slot_as(ctx, SL_TRIS, (size_t)simplex_offsets[n_windows] * 3, &d));
        SAME_COPY(ctx, d, simplices, (size_t)simplex_offsets[n_windows] * 12, hipMemcpyHostToDevice);
        d_simplices = d;
    }
    int rc = SAME_OK;
    std::vector<same_window *> live;
    std::vector<FinishPlan *> plans;
    std::vector<FilterPlan *> fplans;
    for (int i = 0; i < n_windows && rc == SAME_OK; ++i) {
        same_window *w = windows[i];
        Item &it = items[(size_t)i];
        const int32_t *tri = on_device ? nullptr : simplices + 3 * simplex_offsets[i];
        const int64_t Tr = simplex_offsets[i + 1] - simplex_offsets[i];
        w->results_void();
        if (w->cur.n_ua == 0) continue;
        if (Tr && source != SAME_TRIS_KEPT) {
            const int32_t *raw = from_caller ? w->caller_out : on_device ? static_cast<const int32_t *>(w->dd_tris.p) : d_simplices + 3 * simplex_offsets[i];
            rc = prepare_filter(w, raw, Tr, ignore_same_type, ensure_min_triangle_per_node, &it.fplan);
            if (rc == SAME_OK) rc = prepare_finish(w, nullptr, Tr, it.fplan.counters + FC_TR, mode, &it.plan);
            if (rc == SAME_OK) {
                fplans.push_back(&it.fplan);
                it.plan.filter_zero = it.fplan.zero;
                it.plan.filter_zero_bytes = it.fplan.zero_bytes;
            }
            it.filtered = true;
        } else {
            rc = prepare_finish(w, Tr ? tri : nullptr, Tr, nullptr, mode, &it.plan);     // the caller's kept triangles (or none)
        }
        if (rc == SAME_OK) {
            live.push_back(w);
            plans.push_back(&it.plan);
        }
    }
    for (size_t g = 0; g < live.size() && rc == SAME_OK; g += SAME_LAUNCH_WINDOWS) {      // the heads of both buffers of every window: one launch per group
        ZeroArgs zr[SAME_LAUNCH_WINDOWS];
        const int n_g = (int)std::min<size_t>(SAME_LAUNCH_WINDOWS, live.size() - g);
        for (int q = 0; q < n_g; ++q) {
            const FinishPlan *fp = plans[g + (size_t)q];
            zr[q] = ZeroArgs{{fp->zero, fp->filter_zero}, {fp->zero_bytes, fp->filter_zero_bytes}};
        }
        rc = launch_zero(ctx, zr, n_g);
    }
    // groups of at most SAME_LAUNCH_WINDOWS consecutive windows that agree on what a launch fixes for all of them (windows of one call
    // usually come from one pair of sections: whether same-type triangles come back, the cost type; the mode is the call's)
    for (size_t g = 0, e; g < fplans.size() && rc == SAME_OK; g = e) {
        for (e = g + 1; e < fplans.size() && e - g < SAME_LAUNCH_WINDOWS && fplans[e]->readd == fplans[g]->readd; ++e) {}
        rc = launch_filter(ctx, fplans.data() + g, (int)(e - g), radius, angle_enabled, cos_thr, near_tol);
    }
    for (size_t g = 0, e; g < live.size() && rc == SAME_OK; g = e) {
        for (e = g + 1; e < live.size() && e - g < SAME_LAUNCH_WINDOWS && live[e]->cost_f32 == live[g]->cost_f32; ++e) {}
        rc = launch_finish(ctx, live.data() + g, plans.data() + g, (int)(e - g));
    }
    // the finish block of every window and, beside it, the filter's counters: one launch per group straight into the pinned blocks (or
    // one copy from each buffer where a block is not device-addressable)
    {
        CopyArgs ca[SAME_LAUNCH_WINDOWS];
        int n_g = 0;
        for (int i = 0; i < n_windows && rc == SAME_OK; ++i) {
            same_window *w = windows[i];
            Item &it = items[(size_t)i];
            if (w->cur.n_ua != 0) {
                if (w->host_dev) {
                    ca[n_g++] = CopyArgs{{it.plan.gs.sel, it.filtered ? it.fplan.counters : nullptr},
                                         {w->host_dev + w->host_finish_off, w->host_dev + w->host_filter_off},
                                         {it.plan.back_bytes, it.filtered ? FC_COPIED * sizeof(unsigned long long) : 0}};
                } else {
                    if (it.filtered) {
                        unsigned long long *hf = reinterpret_cast<unsigned long long *>(static_cast<char *>(w->host) + w->host_filter_off);
                        hipError_t e = hipMemcpyAsync(hf, it.fplan.counters, FC_COPIED * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
                        ++ctx->stats[SAME_STAT_COPIES];
                        if (e != hipSuccess) rc = same_fail(ctx, SAME_EIO, "filter counters", e);
                    }
                    if (rc == SAME_OK) rc = enqueue_finish_copy(w, &it.plan);
                }
                it.enqueued = rc == SAME_OK;
            }
            if (rc == SAME_OK && n_g && (n_g == SAME_LAUNCH_WINDOWS || i == n_windows - 1)) {
                rc = launch_copy_back(ctx, ca, n_g);
                n_g = 0;
            }
        }
    }
    if (rc != SAME_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    SAME_WAIT(ctx);
    int64_t cell0 = 0;
    for (int i = 0; i < n_windows; ++i) {
        same_window *w = windows[i];
        Item &it = items[(size_t)i];
        const int64_t Tr = simplex_offsets[i + 1] - simplex_offsets[i];
        int64_t *counts = out_counts + 4 * i, *stats = out_stats + mode.stride * i;
        if (!it.enqueued) {                 // no kept aligned cell: nothing to match, nothing to sweep
            w->finished_with(0);
            continue;
        }
        int32_t *const match_out = out_match_row + cell0;
        uint8_t *const flag_out = out_point_flag + cell0;
        cell0 += w->cur.n_ua;
        if (it.filtered) {
            // the filter's counters first (they are on the host since the batch's one wait): a window with a cosine at the threshold is
            // redone by the caller with SAME_TRIS_KEPT, so nothing of it is read back here (its stats stay 0) -- in particular no further greedy rounds
            // (fills, launches and a wait per batch of rounds) are spent on a matching that is thrown away
            const unsigned long long *hf = reinterpret_cast<const unsigned long long *>(static_cast<const char *>(w->host) + w->host_filter_off);
            const int64_t n_keep = (int64_t)hf[FC_KEEP], n_near = (int64_t)hf[FC_NEAR], n_add = it.fplan.readd ? (int64_t)hf[FC_ADD] : 0;
            counts[0] = n_keep;
            counts[1] = n_add;
            counts[2] = n_near;
            counts[3] = (int64_t)hf[FC_TIES];
            if (n_near) continue;
        } else {
            counts[0] = Tr;
        }
        SAME_TRY(read_finish(w, &it.plan, match_out, flag_out, stats, counts + 3));
        w->finished_with(counts[0] + counts[1]);      // kept + added back (the caller's kept triangles: all of them)
    }
    return SAME_OK;
}

static int refinish(same_window *window, const int32_t *match_pair, const FinishMode &mode, int32_t *out_match_row, uint8_t *out_point_flag,
                    int64_t *out_stats) {
    if (!window) return SAME_EINVAL;
    same_window *w = window;
    same_ctx *ctx = w->ctx;
    SAME_TRY(check_mode(ctx, mode));
    REQUIRE(ctx, w->has_results() && w->cur.n_ua > 0 && match_pair && out_match_row && out_point_flag && out_stats);
    for (int64_t i = 0; i < w->cur.n_ua; ++i) REQUIRE(ctx, match_pair[i] >= -1 && match_pair[i] < w->cur.list.P);
    SAME_TRY(same_use(ctx));
    // the window's kept triangles are still the first w->Tr of its triangle buffer: lay the finish block out for exactly those
    FinishPlan p;
    SAME_TRY(prepare_finish(w, nullptr, w->Tr, nullptr, mode, &p));
    SAME_FILL(ctx, p.zero, 0, p.zero_bytes);
    if (w->cur.list.P) SAME_FILL(ctx, p.gs.alive, 0, (size_t)w->cur.list.P);
    SAME_COPY(ctx, p.match_pair, match_pair, (size_t)w->cur.n_ua * 4, hipMemcpyHostToDevice);
    FinishPlan *pp = &p;
    SAME_TRY(enqueue_refine(ctx, &pp, 1));          // the local search again, from the caller's matching
    SAME_TRY(enqueue_tail(ctx, &w, &pp, 1));
    char *h = static_cast<char *>(w->host) + w->host_finish_off;
    SAME_COPY(ctx, h, reinterpret_cast<const char *>(p.gs.sel), p.back_bytes, hipMemcpyDeviceToHost);
    SAME_WAIT(ctx);
    for (int q = 0; q < mode.stride; ++q) out_stats[q] = 0;
    SAME_TRY(settle(w, &p, false, out_stats));
    const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(h + p.o_counters);
    for (int q = 0; q < 8; ++q) out_stats[q] = (int64_t)cnt[q];
    memcpy(out_match_row, h + p.o_match_row, (size_t)w->cur.n_ua * sizeof(int32_t));
    memcpy(out_point_flag, h + p.o_pflag, (size_t)w->cur.n_ua);
    return SAME_OK;
}

extern "C" {

int same_window_filter_finish(same_window *const *windows, int n_windows, int source, const int32_t *simplices, const int64_t *simplex_offsets,
                              double radius, int angle_enabled, double cos_thr, double near_tol, int ignore_same_type,
                              int ensure_min_triangle_per_node, double no_match_penalty, int incumbent, int64_t refine_rounds_cap,
                              double delaunay_penalty, int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats,
                              int64_t *out_counts) {
    return filter_finish(windows, n_windows, source, simplices, simplex_offsets, radius, angle_enabled, cos_thr, near_tol, ignore_same_type,
                         ensure_min_triangle_per_node, mode_of(incumbent, no_match_penalty, refine_rounds_cap, delaunay_penalty, nullptr, false),
                         out_match_row, out_point_flag, out_stats, out_counts);
}

int same_window_filter_finish_cap(same_window *const *windows, int n_windows, int source, const int32_t *simplices,
                                  const int64_t *simplex_offsets, double radius, int angle_enabled, double cos_thr, double near_tol,
                                  int ignore_same_type, int ensure_min_triangle_per_node, double no_match_penalty, int incumbent,
                                  int64_t refine_rounds_cap, double delaunay_penalty, const same_window_capacity *capacity,
                                  int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats, int64_t *out_counts) {
    return filter_finish(windows, n_windows, source, simplices, simplex_offsets, radius, angle_enabled, cos_thr, near_tol, ignore_same_type,
                         ensure_min_triangle_per_node, mode_of(incumbent, no_match_penalty, refine_rounds_cap, delaunay_penalty, capacity, true),
                         out_match_row, out_point_flag, out_stats, out_counts);
}

int same_window_refinish(same_window *window, const int32_t *match_pair, double no_match_penalty, int64_t refine_rounds_cap,
                         double delaunay_penalty, int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats) {
    // (no incumbent is searched for)
    return refinish(window, match_pair, mode_of(SAME_INCUMBENT_GREEDY, no_match_penalty, refine_rounds_cap, delaunay_penalty, nullptr, false),
                    out_match_row, out_point_flag, out_stats);
}

int same_window_refinish_cap(same_window *window, const int32_t *match_pair, double no_match_penalty, int64_t refine_rounds_cap,
                             double delaunay_penalty, const same_window_capacity *capacity, int32_t *out_match_row,
                             uint8_t *out_point_flag, int64_t *out_stats) {
    return refinish(window, match_pair, mode_of(SAME_INCUMBENT_GREEDY, no_match_penalty, refine_rounds_cap, delaunay_penalty, capacity, true),
                    out_match_row, out_point_flag, out_stats);
}

}  // extern "C"
