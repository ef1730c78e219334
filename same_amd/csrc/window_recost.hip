// window_recost.hip -- a staged window's pair list priced again from ANOTHER type matrix of the moving section (same_window_recost).
// Of everything a window is made of, only the pair costs read the type columns: the row lists, the radius / k prune, the compaction, the
// reference numbers and the triangulation are geometry, the triangle filter and the priority prune read type CODES.  A study that changes
// only the moving frame's type columns (a robustness run over noised types) therefore needs, per variant, not a stage call but the costs
// of the list as staged (win::State::sk) written again -- with the moving rows read from a types layer (same_types_layer, section.hip)
// and everything else where the stage call left it.
//
// The value is the stage call's, bit for bit (cost.hip, padded_cost_kernel / padded_cost_lds_kernel):
//   s = s + |a[t] - r[t]| over t = 0..T-1 in the cost type F, then  w*s + (w*0.001)*(|ax-rx| + |ay-ry|)  with the XY in F, then (double).
// Nothing is contracted or reordered; this file is built with cost.hip's flags.
//
// Per launch the windows of a group (blockIdx.y = window).  A wave owns 64 consecutive pairs of the staged list.  Pair p's moving row is
// rows_ua[pairs[2p]], its reference row jsec[p]: consecutive pairs share their moving row (one cache line, broadcast), the reference rows
// are the gather.  As padded_cost_lds_kernel does, the wave first copies its 64 reference rows into LDS with lanes running ALONG the rows
// (a load instruction covers a few rows' worth of lines instead of 64 different ones) at the odd pitch T|1 (2-way bank aliasing at worst
// when every lane then walks its own row left to right).  Where the block does not fit (64 x (T|1) values outgrow 64 KB from T = 128 in
// double), where T < 2, and for lists too short to fill the card, one lane gathers its own row -- padded_cost_dev's rule; both forms
// evaluate the same expression in the same order.
// The pair count is read on the device (prow[kept cells]); the launch is sized by the host's copy of it.
//
// The call leaves every window in the state same_window_knn_prefix at the staged k leaves (window_state.h's table; the two calls are one
// skeleton, win::restage_batch) -- so the sequence of a knn group (prefix, prune, same_window_caller_pairs) runs on it unchanged.  The slots of the stage call's padded candidate costs (the F values cost64 was widened from) are scratch of that call --
// nothing reads them after its scatter -- and are not rewritten.
#include "window_internal.h"

namespace {

using namespace win;

template <typename F> __device__ __forceinline__ F absf(F x);
template <> __device__ __forceinline__ double absf<double>(double x) { return __builtin_fabs(x); }
template <> __device__ __forceinline__ float absf<float>(float x) { return __builtin_fabsf(x); }

// per window of a launch
struct RecostArgs {
    int64_t n, bound;              // kept aligned cells as staged; the staged pair count as the host knows it (the launch's size)
    const int32_t *rows_ua;        // [n] the kept cells' moving SECTION rows
    PairList list;                 // the list as staged: cost64 is rewritten
    unsigned long long *counts;    // the window's count block: [3] pairs, [4] a priority prune's count
};

// the sections' operands of a launch
template <typename F>
struct RecostOperands {
    const F *A, *R, *axy, *rxy;    // moving types (the layer's or the section's own), reference types, both XY in the cost type
    int T;
    int64_t n_a, n_r;              // rows of the two sections: a row number outside them is never dereferenced
    F w, dcoef;
};

// the window's pair count, read where it lives; block (0, window)'s first thread leaves the count block as a stage call does
__device__ __forceinline__ int64_t staged_pairs(const RecostArgs &wa) {
    int64_t P = wa.n > 0 ? (int64_t)wa.list.prow[wa.n] : 0;
    P = P < 0 ? 0 : (P > wa.bound ? wa.bound : P);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        wa.counts[3] = (unsigned long long)P;
        wa.counts[4] = 0;
    }
    return P;
}

// pair p's moving row, or -1
__device__ __forceinline__ int64_t moving_row(const RecostArgs &wa, int64_t p, int64_t n_a) {
    const int32_t a = wa.list.pairs[2 * p];
    if (a < 0 || a >= wa.n) return -1;
    const int64_t i = wa.rows_ua[a];
    return i >= 0 && i < n_a ? i : -1;
}

template <typename F>
__device__ __forceinline__ F pair_value(const RecostOperands<F> &o, const F *a, const F *r, int64_t i, int64_t j) {
    F s = F(0);
    for (int t = 0; t < o.T; ++t) s = s + absf<F>(a[t] - r[t]);
    const F dc = absf<F>(o.axy[2 * i] - o.rxy[2 * j]) + absf<F>(o.axy[2 * i + 1] - o.rxy[2 * j + 1]);
    return o.w * s + o.dcoef * dc;
}

// one lane per pair, its reference row gathered
template <typename F>
__global__ __launch_bounds__(256) void recost_kernel(RecostOperands<F> o, Batch<RecostArgs> b) {
    const RecostArgs &wa = b.w[blockIdx.y];
    const int64_t P = staged_pairs(wa);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int64_t j = wa.list.jsec[p], i = moving_row(wa, p, o.n_a);
    if (i < 0 || j < 0 || j >= o.n_r) return;
    wa.list.cost64[p] = (double)pair_value<F>(o, o.A + i * o.T, o.R + j * o.T, i, j);
}

// a wave owns 64 consecutive pairs: their reference rows staged in LDS (lanes along the rows, pitch T|1), then a lane per pair
template <typename F>
__global__ __launch_bounds__(256) void recost_lds_kernel(RecostOperands<F> o, Batch<RecostArgs> b) {
    extern __shared__ double lds_raw[];
    const RecostArgs &wa = b.w[blockIdx.y];
    const int64_t P = staged_pairs(wa);
    F *lds = reinterpret_cast<F *>(lds_raw);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int T = o.T, pitch = T | 1;
    F *rows = lds + (size_t)wave * 64 * pitch;
    int *jl = reinterpret_cast<int *>(lds + (size_t)waves * 64 * pitch) + wave * 64;     // after ALL waves' row blocks (4-byte aligned for float rows)
    const int64_t p0 = ((int64_t)blockIdx.x * waves + wave) * 64;
    if (p0 >= P) return;                             // whole wave out of range (wave-uniform)
    const int64_t p = p0 + lane;
    int j = p < P ? wa.list.jsec[p] : -1;
    if (j >= o.n_r) j = -1;
    jl[lane] = j;
    __builtin_amdgcn_wave_barrier();                 // jl is written and read by this wave only
    {   // element e = slot * T + t of the wave's 64 x T block, e = lane, lane + 64, ...: (slot, t) advanced without dividing
        const int ds = 64 / T, dt = 64 - ds * T;
        int sl = lane / T, t = lane - sl * T;
        for (int it = 0; it < T; ++it) {
            const int js = jl[sl];
            rows[sl * pitch + t] = js >= 0 ? o.R[(int64_t)js * T + t] : F(0);
            sl += ds;
            t += dt;
            if (t >= T) { t -= T; ++sl; }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (p >= P || j < 0) return;
    const int64_t i = moving_row(wa, p, o.n_a);
    if (i < 0) return;
    wa.list.cost64[p] = (double)pair_value<F>(o, o.A + i * T, rows + lane * pitch, i, (int64_t)j);
}

struct RecostPlan {
    RecostArgs a{};
};

// a group's launch: padded_cost_dev's rule (cost.hip) for which form runs
template <typename F>
int launch_recost(same_ctx *ctx, RecostPlan *const *pps, int n_w, const same_section *mov, const same_section *ref, const void *types_c, double w) {
    Batch<RecostArgs> b{};
    int64_t most = 0;
    for (int q = 0; q < n_w; ++q) {
        b.w[q] = pps[q]->a;
        most = std::max(most, pps[q]->a.bound);
    }
    if (most == 0) return SAME_OK;
    RecostOperands<F> o{static_cast<const F *>(types_c), static_cast<const F *>(ref->types_c), static_cast<const F *>(mov->xy_c),
                        static_cast<const F *>(ref->xy_c), mov->T, mov->n, ref->n, (F)w, (F)w * F(0.001)};
    const int T = mov->T;
    size_t per_wave = (size_t)64 * (T | 1) * sizeof(F) + 64 * sizeof(int);
    per_wave = (per_wave + 7) & ~size_t(7);
    const int waves = (int)std::min<size_t>(4, (size_t)65536 / per_wave);
    if (T >= 2 && waves >= 1 && most >= 64 * 64)
        SAME_LAUNCH(ctx, recost_lds_kernel<F>, dim3((unsigned)ceil_div(most, 64 * waves), (unsigned)n_w), dim3(64 * waves), waves * per_wave, o, b);
    else
        SAME_LAUNCH(ctx, recost_kernel<F>, dim3((unsigned)ceil_div(most, 256), (unsigned)n_w), dim3(256), 0, o, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace

extern "C" {

int same_window_recost(same_window *const *windows, int n_windows, const same_section *mov, const same_section *ref, const same_types_layer *layer,
                       double dist_ct_coeff, int64_t *out_counts) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, mov && ref && out_counts && mov->T == ref->T && mov->cost_f32 == ref->cost_f32);
    REQUIRE(ctx, !layer || (layer->sec == mov && layer->ctx->device == ctx->device && (mov->T == 0 || mov->n == 0 || layer->types_c)));
    for (int i = 0; i < n_windows; ++i) {
        const same_window *w = windows[i];
        REQUIRE(ctx, w->may_recost() && w->mov == mov && w->ref == ref);
    }
    SAME_TRY(same_use(ctx));
    const void *types_c = layer ? layer->types_c : mov->types_c;
    return restage_batch<RecostPlan>(
        ctx, windows, n_windows, 0, "recost copy back", out_counts,
        [&](same_window *w, RecostPlan *pp, bool *needs) {
            *needs = w->pairs_possible() && w->sk.P != 0 && w->cur.n_ua != 0;
            if (*needs) pp->a = RecostArgs{w->cur.n_ua, w->sk.P, w->cur.rows_ua, w->sk, w->cur.counts};
            return SAME_OK;
        },
        [&](RecostPlan *const *pps, int n_g) {
            return mov->cost_f32 ? launch_recost<float>(ctx, pps, n_g, mov, ref, types_c, dist_ct_coeff)
                                 : launch_recost<double>(ctx, pps, n_g, mov, ref, types_c, dist_ct_coeff);
        },
        [&](const same_window *w, const RecostPlan &, PairList *list) {
            REQUIRE(ctx, (int64_t) static_cast<const unsigned long long *>(w->host)[3] == w->sk.P);
            *list = w->sk;
            return SAME_OK;
        });
}

}  // extern "C"
