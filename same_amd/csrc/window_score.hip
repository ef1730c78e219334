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
//                        check_triangle_violations on the moving XY and the matched reference XY (devmath.h: eval_area3, eval_flipped --
//                        match.hip's tri_flip_stats_kernel runs the same two functions); the corners' counters over the triangles that
//                        are not skipped
//   score_nodes_kernel   per final row: is the row's node violating (any flip, or the node-local majority rule); the row's match_of and
//                        counters go back to their idle state (win::ScoreWork, window_internal.h)
//
// Every count is an integer: a block counts with wave ballots, adds its waves' counts in LDS and issues ONE 64-bit atomic per total it
// has something for; the per-node counters are 32-bit integer atomics.  No float is ever added, so the counts do not depend on the order.
#include "window_internal.h"

namespace {

using namespace devmath;
using namespace win;

constexpr int NT = 256;
// words of a set of totals (win::SCORE_TOTALS of them)
enum { T_BAD = 0, T_TYPE = 1, T_ALL = 3, T_SAME = 4, T_FLIP = 5, T_FLIP_CONSIDERED = 6, T_NODES = 7 };

// how many threads of the block hold flag[k] -> totals[word[k]].  Every thread of the block calls it (wave64: four ballots' counts meet
// in LDS), thread k adds total k -- one atomic per block and total, none where the block counted nothing.
template <int K>
__device__ __forceinline__ void block_totals(const bool (&flag)[K], const int (&word)[K], unsigned long long *__restrict__ totals) {
    __shared__ unsigned part[K][NT / 64];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long bal = __ballot(flag[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = (unsigned)__builtin_popcountll(bal);
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned n = 0;
        for (int q = 0; q < NT / 64; ++q) n += part[threadIdx.x][q];
        if (n) atomicAdd(&totals[word[threadIdx.x]], (unsigned long long)n);
    }
}

__device__ __forceinline__ bool row_in(int32_t row, int64_t n) { return (unsigned long long)(long long)row < (unsigned long long)n; }

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
        bad = !row_in(a, n_mov) || !row_in(r, n_ref);         // (rows of other sections: counted, never followed)
        if (!bad) {
            if (match_of) match_of[a] = r;
            const int32_t c = code_m[a];
            agree = c >= 0 && c == code_r[r];
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
    bool all = false, same = false, flipped = false;
    if (t < Tr) {
        const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];        // rows of the moving section (same_caller_tris_create)
        const int32_t ma = match_of[a], mb = match_of[b], mc = match_of[c];
        all = ma >= 0 && mb >= 0 && mc >= 0;
        if (all) {
            if (ignore_same) {
                const int32_t ca = code_m[a];
                same = ca >= 0 && ca == code_m[b] && ca == code_m[c];
            }
            flipped = eval_flipped(eval_area3(ld2(mov_xy, a), ld2(mov_xy, b), ld2(mov_xy, c)),
                                   eval_area3(ld2(ref_xy, ma), ld2(ref_xy, mb), ld2(ref_xy, mc)));
            if (!same) {
                atomicAdd(&node_tri[a], 1u); atomicAdd(&node_tri[b], 1u); atomicAdd(&node_tri[c], 1u);
                if (flipped) { atomicAdd(&node_flip[a], 1u); atomicAdd(&node_flip[b], 1u); atomicAdd(&node_flip[c], 1u); }
            }
        }
    }
    const bool flag[4] = {all, same, flipped, flipped && !same};
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
        if (row_in(a, n_mov) && row_in(rows[i].r_row, n_ref)) {          // (the rows score_rows_kernel followed)
            const unsigned n_tri = node_tri[a], n_flip = node_flip[a];
            // src/eval_utils.py:199-211: any flip, or at least min_flips flips that are at least the threshold's share of the node's triangles
            violating = node_local ? (n_tri > 0 && (int64_t)n_flip >= min_flips && (double)n_flip / (double)n_tri >= majority_threshold)
                                   : n_flip > 0;
            match_of[a] = -1;          // a merge's final rows name a moving row once: nobody else reads or resets these three words
            node_tri[a] = 0u;
            node_flip[a] = 0u;
        }
    }
    const bool flag[1] = {violating};
    const int word[1] = {T_NODES};
    block_totals<1>(flag, word, totals);
}

}  // namespace

extern "C" int same_merge_acc_score(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                                    int ignore_same_type, int node_local, double majority_threshold, int64_t min_flips, int64_t *out_counts) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out_counts && a->resolved == 2 && a->merged && !a->loaded);
    REQUIRE(ctx, mov && ref && mov->ctx->device == ctx->device && ref->ctx->device == ctx->device);
    REQUIRE(ctx, mov->label_codes && ref->label_codes);
    REQUIRE(ctx, !tris || (tris->mov == mov && tris->ctx->device == ctx->device));
    REQUIRE(ctx, majority_threshold == majority_threshold);
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, Tr = tris ? tris->n_tris : 0;
    unsigned long long h[SCORE_TOTALS] = {};
    if (n > 0) {
        SAME_TRY(ensure_score_work(ctx, a, std::max<int64_t>(mov->n, 1)));   // laid for too few rows (or never, or a call failed): laid, filled ONCE
        const ScoreWork &sw = a->sw;
        const int64_t laid = a->score_rows;
        a->score_rows = 0;                                    // until the call is through: what fails half way leaves the buffer in doubt
        unsigned long long *totals = sw.totals + (size_t)a->score_set * SCORE_TOTALS, *next = sw.totals + (size_t)(a->score_set ^ 1) * SCORE_TOTALS;
        const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
        SAME_LAUNCH(ctx, score_rows_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, mov->n, ref->n, mov->label_codes, ref->label_codes,
                    Tr > 0 ? sw.match_of : nullptr, totals, next);
        if (Tr > 0) {
            SAME_LAUNCH(ctx, score_tris_kernel, dim3(grid_for(Tr)), dim3(NT), 0, tris->tris, Tr, sw.match_of, mov->label_codes,
                        ignore_same_type ? 1 : 0, mov->xy, ref->xy, sw.node_tri, sw.node_flip, totals);
            SAME_LAUNCH(ctx, score_nodes_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, mov->n, ref->n, node_local ? 1 : 0, majority_threshold,
                        min_flips, sw.match_of, sw.node_tri, sw.node_flip, totals);
        }
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
        a->score_set ^= 1;
        a->score_rows = laid;
        if (h[T_BAD]) {
            ctx->err = "same_merge_acc_score: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    out_counts[0] = n;
    out_counts[1] = (int64_t)h[T_TYPE];
    out_counts[2] = Tr;
    out_counts[3] = (int64_t)h[T_ALL];
    out_counts[4] = (int64_t)h[T_SAME];
    out_counts[5] = (int64_t)h[T_FLIP];
    out_counts[6] = (int64_t)h[T_FLIP_CONSIDERED];
    out_counts[7] = (int64_t)h[T_NODES];
    return SAME_OK;
}
