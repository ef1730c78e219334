// window_score_detail.hip -- the numbers window_score.hip totals, binned: by label pair, by group of the moving rows, by type rank.
//
// The reference's notebooks read every table three more ways than by its totals: per region (check_triangle_violations_within_quadrants,
// src/synthetic_datagen.py:1314-1418: only triangles whose three corners lie in one region count, and each region is reported alone), per
// label pair (the crosstab behind every accuracy figure) and per type rank (is the moving cell's label among the k largest type columns
// of its matched reference cell).  Everything they read is resident when a set's merge ends -- what same_merge_acc_score reads, the
// rows' groups and the labels' columns (same_score_detail), the reference section's type matrix as the caller gave it (types64).
// same_merge_acc_score_detail has the shape of the score call -- a rows kernel, a triangles kernel where there is a triangle, a nodes
// kernel; one copy, one wait -- and works in the same ScoreWork under the same protocol, so the two alternate on one accumulator.
//
//   detail_rows_kernel    per final row: match_of; its cell of the confusion matrix; its group's rows and type matches; the rank of its
//                         label's column in the reference cell's type row (fp64 comparisons, a NaN in the row: untyped)
//   detail_tris_kernel    per resident triangle: its bin (the corners' common group, else cross); score_tris_kernel's flags into that
//                         bin; the corners' counters over the triangles that are within a group and not skipped
//   detail_nodes_kernel   per final row: violating under the rule -> its group's node word; the row's three words back to idle
//
// Every count is an integer.  A block bins into 32-bit LDS counters sized by the call's own L and G, walks its share of a capped grid
// and then issues ONE 64-bit atomic per bin it has something for (the HIP guide's rule 12: reduce per block first).
#include "window_internal.h"

namespace {

using namespace win;

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 128;      // blocks of a launch: the rest is strided over, so the flushes stay few beside the row work
constexpr int R = SAME_SCORE_RANKS;
// words of a group's record (DETAIL_GROUP_WORDS of them), as same_merge_acc_score's out_counts
enum { W_ROWS = 0, W_TYPE = 1, W_TRIS = 2, W_ALL = 3, W_SAME = 4, W_FLIP = 5, W_FLIP_CONSIDERED = 6, W_NODES = 7 };

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>(ceil_div(n > 0 ? n : 1, NT), MAX_BLOCKS); }

extern __shared__ unsigned lds_bins[];

__device__ __forceinline__ void clear_lds(int words) {
    for (int i = threadIdx.x; i < words; i += NT) lds_bins[i] = 0u;
    __syncthreads();
}
// LDS word i -> global word at(i), one atomic per non-zero word
template <class At>
__device__ __forceinline__ void flush_lds(int words, unsigned long long *__restrict__ bins, At at) {
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += NT) {
        const unsigned v = lds_bins[i];
        if (v) atomicAdd(&bins[at(i)], (unsigned long long)v);
    }
}

// LDS: [L*L confusion | unlabelled | (G+1) x (rows, type matches) | strict[R+1] | weak[R+1] | untyped | bad]
__global__ __launch_bounds__(NT) void detail_rows_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                         const int32_t *__restrict__ code_m, const int32_t *__restrict__ code_r,
                                                         const int32_t *__restrict__ group_of, const int32_t *__restrict__ col_of_label,
                                                         const double *__restrict__ types_r, int T, DetailLayout lay,
                                                         int32_t *__restrict__ match_of, unsigned long long *__restrict__ bins,
                                                         unsigned long long *__restrict__ next_bins, int64_t next_dirty) {
    const int L = lay.L, G = lay.G;
    const int o_unl = L * L, o_grp = o_unl + 1, o_strict = o_grp + 2 * (G + 1), o_weak = o_strict + R + 1, o_unt = o_weak + R + 1,
              o_bad = o_unt + 1, words = o_bad + 1;
    const int64_t stride = (int64_t)gridDim.x * NT, first = (int64_t)blockIdx.x * NT + threadIdx.x;
    for (int64_t i = first; i < next_dirty; i += stride) next_bins[i] = 0ull;        // the set the NEXT call counts into
    clear_lds(words);
    for (int64_t i = first; i < n; i += stride) {
        const int32_t a = rows[i].a_row, r = rows[i].r_row;
        if (!followed(rows[i], n_mov, n_ref)) {
            atomicAdd(&lds_bins[o_bad], 1u);
            continue;
        }
        if (match_of) match_of[a] = r;
        const int32_t cm = code_m[a], cr = code_r[r];
        const bool lm = cm >= 0 && cm < L, lr = cr >= 0 && cr < L;
        atomicAdd(&lds_bins[lm && lr ? cm * L + cr : o_unl], 1u);
        const int g = group_at(group_of, a, G);
        atomicAdd(&lds_bins[o_grp + 2 * g], 1u);
        if (labels_agree(cm, cr)) atomicAdd(&lds_bins[o_grp + 2 * g + 1], 1u);
        const int c = lm && col_of_label ? col_of_label[cm] : -1;
        bool typed = c >= 0 && c < T;
        if (typed) {
            int strict, weak;
            typed = type_rank(types_r + (int64_t)r * T, T, c, strict, weak);
            if (typed) {
                atomicAdd(&lds_bins[o_strict + (strict < R ? strict : R)], 1u);
                atomicAdd(&lds_bins[o_weak + (weak < R ? weak : R)], 1u);
            }
        }
        if (!typed) atomicAdd(&lds_bins[o_unt], 1u);
    }
    flush_lds(words, bins, [=](int i) -> int64_t {
        if (i < o_grp) return i;                                             // confusion, unlabelled: the set's own order
        if (i < o_strict) return lay.groups() + (int64_t)((i - o_grp) >> 1) * DETAIL_GROUP_WORDS + ((i - o_grp) & 1 ? W_TYPE : W_ROWS);
        if (i < o_bad) return lay.strict() + (i - o_strict);                 // strict, weak, untyped
        return lay.bad();
    });
}

// LDS: (G+1) x (resident, all matched, same type, flipped, flipped and not skipped)
__global__ __launch_bounds__(NT) void detail_tris_kernel(const int32_t *__restrict__ tris, int64_t Tr, const int32_t *__restrict__ match_of,
                                                         const int32_t *__restrict__ code_m, const int32_t *__restrict__ group_of,
                                                         int ignore_same, const double *__restrict__ mov_xy, const double *__restrict__ ref_xy,
                                                         DetailLayout lay, unsigned *__restrict__ node_tri, unsigned *__restrict__ node_flip,
                                                         unsigned long long *__restrict__ bins) {
    const int G = lay.G, words = 5 * (G + 1);
    clear_lds(words);
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < Tr; t += stride) {
        const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];        // rows of the moving section (same_caller_tris_create)
        const int ga = group_at(group_of, a, G);
        const int g = ga == group_at(group_of, b, G) && ga == group_at(group_of, c, G) ? ga : G;
        unsigned *mine = lds_bins + 5 * g;
        atomicAdd(&mine[0], 1u);
        TriVerdict v;
        tri_verdict(v, a, b, c, match_of, code_m, ignore_same, mov_xy, ref_xy);
        if (!v.all) continue;
        atomicAdd(&mine[1], 1u);
        if (v.same) atomicAdd(&mine[2], 1u);
        if (v.flipped) atomicAdd(&mine[3], 1u);
        if (v.flipped && !v.same) atomicAdd(&mine[4], 1u);
        if (!v.same && g < G) count_corners(a, b, c, v.flipped, node_tri, node_flip);       // within a group and not skipped
    }
    flush_lds(words, bins, [=](int i) -> int64_t { return lay.groups() + (int64_t)(i / 5) * DETAIL_GROUP_WORDS + W_TRIS + i % 5; });
}

// LDS: (G+1) x (violating nodes)
__global__ __launch_bounds__(NT) void detail_nodes_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                          const int32_t *__restrict__ group_of, int node_local, double majority_threshold,
                                                          int64_t min_flips, DetailLayout lay, int32_t *__restrict__ match_of,
                                                          unsigned *__restrict__ node_tri, unsigned *__restrict__ node_flip,
                                                          unsigned long long *__restrict__ bins) {
    const int G = lay.G, words = G + 1;
    clear_lds(words);
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
        const int32_t a = rows[i].a_row;
        if (!followed(rows[i], n_mov, n_ref)) continue;
        if (node_violating(node_tri[a], node_flip[a], node_local, majority_threshold, min_flips))
            atomicAdd(&lds_bins[group_at(group_of, a, G)], 1u);
        reset_idle(a, match_of, node_tri, node_flip);
    }
    flush_lds(words, bins, [=](int i) -> int64_t { return lay.groups() + (int64_t)i * DETAIL_GROUP_WORDS + W_NODES; });
}

}  // namespace

extern "C" {

int same_score_detail_create(const same_section *mov, const int32_t *group_of, int n_groups, int n_labels, const int32_t *col_of_label,
                             same_score_detail **out) {
    if (!mov || !out) return SAME_EINVAL;
    same_ctx *ctx = mov->ctx;
    *out = nullptr;
    REQUIRE(ctx, n_groups >= 1 && n_groups <= SAME_SCORE_MAX_GROUPS && n_labels >= 0 && n_labels <= SAME_SCORE_MAX_LABELS);
    if (group_of)
        for (int64_t i = 0; i < mov->n; ++i)
            if (group_of[i] >= n_groups) {
                ctx->err = "same_score_detail_create: a group_of value is not below n_groups";
                return SAME_ERANGE;
            }
    if (col_of_label)
        for (int q = 0; q < n_labels; ++q)
            if (col_of_label[q] < -1 || col_of_label[q] >= mov->T) {
                ctx->err = "same_score_detail_create: a col_of_label value is outside [-1, T)";
                return SAME_ERANGE;
            }
    SAME_TRY(same_use(ctx));
    same_score_detail *d = new (std::nothrow) same_score_detail();
    if (!d) return SAME_ENOMEM;
    d->ctx = ctx;
    d->mov = mov;
    d->n_groups = n_groups;
    d->n_labels = n_labels;
    *out = d;                                     // freed by the caller's destroy on any failure below
    if (group_of && mov->n > 0) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d->group_of), (size_t)mov->n * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(d->group_of, group_of, (size_t)mov->n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (col_of_label && n_labels > 0) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d->col_of_label), (size_t)n_labels * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(d->col_of_label, col_of_label, (size_t)n_labels * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_score_detail_destroy(same_score_detail *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (d->group_of) (void)hipFree(d->group_of);
    if (d->col_of_label) (void)hipFree(d->col_of_label);
    delete d;
}

int same_merge_acc_score_detail(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                                const same_score_detail *detail, int ignore_same_type, int node_local, double majority_threshold,
                                int64_t min_flips, int64_t *out, int64_t out_words) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out);
    SAME_TRY(require_score_args(ctx, a, mov, ref, tris, majority_threshold));
    REQUIRE(ctx, detail && detail->mov == mov && detail->ctx->device == ctx->device);
    REQUIRE(ctx, !detail->col_of_label || (ref->T == mov->T && ref->types64));
    DetailLayout lay;
    lay.L = detail->n_labels;
    lay.G = detail->n_groups;
    REQUIRE(ctx, out_words >= lay.out_words());
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, Tr = tris ? tris->n_tris : 0, words = lay.words();
    std::vector<unsigned long long> h((size_t)words, 0ull);
    if (n > 0 || Tr > 0) {
        SAME_TRY(ensure_score_work(ctx, a, std::max<int64_t>(mov->n, 1)));
        WorkSets &ds = a->detail_sets;
        if (!ds.fits(words)) {
            InDoubt laying(ds);
            SAME_TRY(lay_over(ctx, a->detail, a->dw, words));
            SAME_FILL(ctx, a->detail.p, 0, a->dw.bytes);
            ds.laid_anew(words);
        }
        const ScoreWork &sw = a->sw;
        InDoubt doubt_score(a->score_sets), doubt(ds);        // the call works in both buffers
        unsigned long long *bins = a->dw.bins + (size_t)ds.set * a->dw.cap, *next = a->dw.bins + (size_t)(ds.set ^ 1) * a->dw.cap;
        const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
        const size_t lds_rows = (size_t)(lay.L * lay.L + 1 + 2 * (lay.G + 1) + 2 * (R + 1) + 2) * sizeof(unsigned);
        SAME_LAUNCH(ctx, detail_rows_kernel, dim3(blocks_for(std::max(n, ds.dirty))), dim3(NT), lds_rows, fin, n, mov->n, ref->n,
                    mov->label_codes, ref->label_codes, detail->group_of, detail->col_of_label, ref->types64, mov->T, lay,
                    Tr > 0 ? sw.match_of : nullptr, bins, next, ds.dirty);
        if (Tr > 0) {
            SAME_LAUNCH(ctx, detail_tris_kernel, dim3(blocks_for(Tr)), dim3(NT), (size_t)(5 * (lay.G + 1)) * sizeof(unsigned), tris->tris, Tr,
                        sw.match_of, mov->label_codes, detail->group_of, ignore_same_type ? 1 : 0, mov->xy, ref->xy, lay, sw.node_tri,
                        sw.node_flip, bins);
            SAME_LAUNCH(ctx, detail_nodes_kernel, dim3(blocks_for(n)), dim3(NT), (size_t)(lay.G + 1) * sizeof(unsigned), fin, n, mov->n, ref->n,
                        detail->group_of, node_local ? 1 : 0, majority_threshold, min_flips, lay, sw.match_of, sw.node_tri, sw.node_flip,
                        bins);
        }
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h.data(), bins, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
        doubt_score.sound();
        doubt.sound();
        ds.flip(words);
        if (h[(size_t)lay.bad()]) {
            ctx->err = "same_merge_acc_score_detail: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    for (int64_t q = 0; q < lay.out_words(); ++q) out[q] = (int64_t)h[(size_t)q];
    return SAME_OK;
}

}  // extern "C"
