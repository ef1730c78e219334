// window_score.hip -- a merged result reduced to the numbers it is read by, where its rows are: on the device.
//
// The reference's figure notebooks reduce every run to a few numbers: the share of matched cells whose cell type is the type of the
// reference cell they were put on (check_alignment at kNN = 1 on the matched coordinates, src/eval_utils.py:6-53) and
// check_triangle_violations' stats (src/eval_utils.py:66-223) over the moving frame's whole triangulation.  After same_merge_acc_finish
// everything they read is resident: the final rows (moving section row, reference section row), both sections' XY, the joint cell-type
// label codes (same_section_set_label_codes) and the triangulation as section rows (same_caller_tris).  same_merge_acc_score counts
// there -- three kernels on the context's stream, one small copy, one wait -- and no table is made for it.
//
//   score_rows_kernel    per final row: match_of[moving row] = reference row; do the two label codes agree (a negative code equals nothing)
//   score_tris_kernel    per resident triangle: all three corners matched?  the same-type rule on the moving codes; the flip rule of
//                        check_triangle_violations on the moving XY and the matched reference XY; the corners' counters over the
//                        triangles that are not skipped
//   score_nodes_kernel   per final row: is the row's node violating (any flip, or the node-local majority rule); the row's match_of and
//                        counters go back to their idle state (win::ScoreWork, window_internal.h)
//
// What a row, a triangle and a node ARE under the rule is window_internal.h's (the rule's section); these kernels add it up.
// Every count is an integer: a block counts with wave ballots, adds its waves' counts in LDS and issues ONE 64-bit atomic per total it
// has something for; the per-node counters are 32-bit integer atomics.  No float is ever added, so the counts do not depend on the order.
#include "window_internal.h"

namespace {

using namespace win;
using namespace win::score_totals;

constexpr int NT = SCORE_NT;
// (the totals' words and block_totals: window_internal.h, shared with window_score_map.hip)

// match_of null: no triangles to score, nothing reads it
__global__ __launch_bounds__(NT) void score_rows_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                        const int32_t *__restrict__ code_m, const int32_t *__restrict__ code_r,
                                                        int32_t *__restrict__ match_of, unsigned long long *__restrict__ totals,
                                                        unsigned long long *__restrict__ next_totals) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < SCORE_TOTALS) next_totals[threadIdx.x] = 0ull;     // the set the NEXT call counts into
    bool bad = false, agree = false;
    if (i < n) {
        const int32_t a = rows[i].a_row, r = rows[i].r_row;
        bad = !followed(rows[i], n_mov, n_ref);
        if (!bad) {
            if (match_of) match_of[a] = r;
            agree = labels_agree(code_m[a], code_r[r]);
        }
    }
    const bool flag[2] = {bad, agree};
    const int word[2] = {T_BAD, T_TYPE};
    block_totals<2>(flag, word, totals);
}

__global__ __launch_bounds__(NT) void score_tris_kernel(const int32_t *__restrict__ tris, int64_t Tr, const int32_t *__restrict__ match_of,
                                                        const int32_t *__restrict__ code_m, int ignore_same, const double *__restrict__ mov_xy,
                                                        const double *__restrict__ ref_xy, unsigned *__restrict__ node_tri,
                                                        unsigned *__restrict__ node_flip, unsigned long long *__restrict__ totals) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    TriVerdict v;
    if (t < Tr) {
        const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];        // rows of the moving section (same_caller_tris_create)
        tri_verdict(v, a, b, c, match_of, code_m, ignore_same, mov_xy, ref_xy);
        if (v.all && !v.same) count_corners(a, b, c, v.flipped, node_tri, node_flip);
    }
    const bool flag[4] = {v.all, v.same, v.flipped, v.flipped && !v.same};
    const int word[4] = {T_ALL, T_SAME, T_FLIP, T_FLIP_CONSIDERED};
    block_totals<4>(flag, word, totals);
}

__global__ __launch_bounds__(NT) void score_nodes_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                         int node_local, double majority_threshold, int64_t min_flips,
                                                         int32_t *__restrict__ match_of, unsigned *__restrict__ node_tri,
                                                         unsigned *__restrict__ node_flip, unsigned long long *__restrict__ totals) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    bool violating = false;
    if (i < n) {
        const int32_t a = rows[i].a_row;
        if (followed(rows[i], n_mov, n_ref)) {
            violating = node_violating(node_tri[a], node_flip[a], node_local, majority_threshold, min_flips);
            reset_idle(a, match_of, node_tri, node_flip);
        }
    }
    const bool flag[1] = {violating};
    const int word[1] = {T_NODES};
    block_totals<1>(flag, word, totals);
}

}  // namespace

int win::score_phases(same_ctx *ctx, same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                      int ignore_same_type, bool keep_match, unsigned long long *totals, unsigned long long *next) {
    const int64_t n = a->n_final, Tr = tris ? tris->n_tris : 0;
    const ScoreWork &sw = a->sw;
    const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
    SAME_LAUNCH(ctx, score_rows_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, mov->n, ref->n, mov->label_codes, ref->label_codes,
                Tr > 0 || keep_match ? sw.match_of : nullptr, totals, next);
    if (Tr > 0)
        SAME_LAUNCH(ctx, score_tris_kernel, dim3(grid_for(Tr)), dim3(NT), 0, tris->tris, Tr, sw.match_of, mov->label_codes,
                    ignore_same_type ? 1 : 0, mov->xy, ref->xy, sw.node_tri, sw.node_flip, totals);
    return SAME_OK;
}

extern "C" int same_merge_acc_score(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                                    int ignore_same_type, int node_local, double majority_threshold, int64_t min_flips, int64_t *out_counts) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out_counts);
    SAME_TRY(require_score_args(ctx, a, mov, ref, tris, majority_threshold));
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, Tr = tris ? tris->n_tris : 0;
    unsigned long long h[SCORE_TOTALS] = {};
    if (n > 0) {
        SAME_TRY(ensure_score_work(ctx, a, std::max<int64_t>(mov->n, 1)));
        const ScoreWork &sw = a->sw;
        InDoubt doubt(a->score_sets);
        unsigned long long *totals = sw.totals + (size_t)a->score_sets.set * SCORE_TOTALS, *next = sw.totals + (size_t)(a->score_sets.set ^ 1) * SCORE_TOTALS;
        const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
        SAME_TRY(score_phases(ctx, a, mov, ref, tris, ignore_same_type, false, totals, next));
        if (Tr > 0) {
            SAME_LAUNCH(ctx, score_nodes_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, mov->n, ref->n, node_local ? 1 : 0, majority_threshold,
                        min_flips, sw.match_of, sw.node_tri, sw.node_flip, totals);
        }
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
        doubt.sound();
        a->score_sets.flip();
        if (h[T_BAD]) {
            ctx->err = "same_merge_acc_score: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    for (int q = 0; q < SCORE_TOTALS; ++q) out_counts[q] = (int64_t)h[q];     // a set's words [1] and [3 .. 7] are out_counts' own
    out_counts[0] = n;
    out_counts[2] = Tr;
    return SAME_OK;
}
