// window_score_map.hip -- a merged result per CELL: what window_score.hip reduces to eight numbers, kept per row of the moving section.
//
// The reference's notebooks plot every spatial panel per cell: the matches split into good and bad by `in_violating_triangle`
// (examples/synthetic/reproduce_figures.ipynb, Fig 2e), every moving cell as correct or incorrect (examples/tongue, Fig 4), the pairs
// as in or out of the top k type columns (examples/luad cell 13), the pairs against a ground truth (ground_truth.csv of the synthetic
// benchmark).  When a set's merge ends everything such a column reads is resident: the score call's three work words per moving row
// (match_of, node_tri, node_flip: win::ScoreWork), the joint label codes, the reference type rows, a same_score_detail's col_of_label
// and -- uploaded once -- the truth rows.  same_merge_acc_score_map takes the score call's place for a result:
//
//   score_rows_kernel, score_tris_kernel   the score call's own two phases (win::score_phases, window_score.hip), run as they are
//   map_nodes_kernel                       one lane per MOVING row, in the nodes kernel's place: the row's 16-byte mark (one store), its
//                                          share of the resident tally (32-bit atomics whose result is not used: a sweep's sets may be
//                                          folded in from several worker contexts at once), the row's three work words back to idle, and
//                                          the three totals the rows give -- violating nodes and the two truth totals -- per block
//
// The totals of a map call live in the MAP, not in the accumulator: per calling context a slot of two sets of win::MAP_TOTALS words under
// the protocol of work_sets.h (the rows kernel clears the other set's eight score words, the nodes kernel its two truth words), so the
// call costs no fill and the score call's own sets never flip.  The marks are written to a device buffer of the slot and follow the
// totals in ONE asynchronous copy into the caller's memory (page-locked memory makes it a DMA transfer that the one wait covers).
#include "window_internal.h"

namespace {

using namespace win;
using namespace win::score_totals;

constexpr int NT = SCORE_NT;
enum { T_TRUTH_KNOWN = 8, T_ON_TRUTH = 9 };
static_assert(sizeof(same_cell_mark) == 16 && MAP_TOTALS == SCORE_TOTALS + 2, "the mark is one 16-byte store; a set is the score's and two words");

__device__ __forceinline__ unsigned saturated(int rank) { return rank < 254 ? (unsigned)rank : 254u; }

// marks null: counts and tally only; tally null: no tally; truth null: every row unknown; col_of_label null: no ranks
__global__ __launch_bounds__(NT) void map_nodes_kernel(int64_t n_mov, const int32_t *__restrict__ code_m, const int32_t *__restrict__ code_r,
                                                       const int32_t *__restrict__ truth, const int32_t *__restrict__ col_of_label,
                                                       int n_labels, const double *__restrict__ types_r, int T, int node_local,
                                                       double majority_threshold, int64_t min_flips, int32_t *__restrict__ match_of,
                                                       unsigned *__restrict__ node_tri, unsigned *__restrict__ node_flip,
                                                       uint4 *__restrict__ marks, unsigned *__restrict__ tally,
                                                       unsigned long long *__restrict__ totals, unsigned long long *__restrict__ next_totals) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 2) next_totals[T_TRUTH_KNOWN + threadIdx.x] = 0ull;     // (its other words: score_rows_kernel)
    bool violating = false, known = false, on = false;
    if (i < n_mov) {
        const int32_t r = match_of[i];
        const int32_t t = truth ? truth[i] : -1;
        unsigned flags = t >= 0 ? SAME_MARK_TRUTH_KNOWN : 0u, strict = 255u, weak = 255u, n_tri = 0u, n_flip = 0u;
        if (r >= 0) {                                 // a followed final row names it: r is a row of the reference section
            n_tri = node_tri[i];
            n_flip = node_flip[i];
            reset_idle((int32_t)i, match_of, node_tri, node_flip);
            const int32_t cm = code_m[i];
            const bool agree = labels_agree(cm, code_r[r]);
            violating = node_violating(n_tri, n_flip, node_local, majority_threshold, min_flips);
            known = t >= 0;
            on = r == t;
            flags |= SAME_MARK_MATCHED | (agree ? SAME_MARK_TYPE_MATCH : 0u) | (n_tri > 0 ? SAME_MARK_CONSIDERED : 0u) |
                     (violating ? SAME_MARK_VIOLATING : 0u) | (on ? SAME_MARK_ON_TRUTH : 0u);
            const int c = col_of_label && cm >= 0 && cm < n_labels ? col_of_label[cm] : -1;
            if (c >= 0 && c < T) {
                int s, w;
                if (type_rank(types_r + (int64_t)r * T, T, c, s, w)) {
                    flags |= SAME_MARK_RANKED;
                    strict = saturated(s);
                    weak = saturated(w);
                }
            }
            if (tally) {
                unsigned *mine = tally + 4 * i;
                atomicAdd(&mine[0], 1u);
                if (agree) atomicAdd(&mine[1], 1u);
                if (violating) atomicAdd(&mine[2], 1u);
                if (on) atomicAdd(&mine[3], 1u);
            }
        }
        if (marks) marks[i] = make_uint4((unsigned)r, n_tri, n_flip, flags | strict << 8 | weak << 16);
    }
    const bool flag[3] = {violating, known, on};
    const int word[3] = {T_NODES, T_TRUTH_KNOWN, T_ON_TRUTH};
    block_totals<3>(flag, word, totals);
}

// the calling context's slot of the map (a context's first call takes a free one)
int slot_of(same_ctx *ctx, same_score_map *map, MapSlot **out, int *index) {
    std::lock_guard<std::mutex> hold(map->lock);
    for (int q = 0; q < MAP_SLOTS; ++q)
        if (map->slots[q].owner == ctx || !map->slots[q].owner) {
            map->slots[q].owner = ctx;
            *out = &map->slots[q];
            *index = q;
            return SAME_OK;
        }
    ctx->err = "same_merge_acc_score_map: the map serves no more calling contexts";
    return SAME_ENOMEM;
}

}  // namespace

extern "C" {

int same_score_map_create(same_ctx *ctx, const same_section *mov, const same_section *ref, const int32_t *truth_row, int with_tally,
                          same_score_map **out) {
    if (!ctx || !out) return SAME_EINVAL;
    *out = nullptr;
    REQUIRE(ctx, mov && ref && mov->ctx->device == ctx->device && ref->ctx->device == ctx->device);
    if (truth_row)
        for (int64_t i = 0; i < mov->n; ++i)
            if (truth_row[i] < -1 || truth_row[i] >= ref->n) {
                ctx->err = "same_score_map_create: a truth row is outside [-1, rows of the reference section)";
                return SAME_EINVAL;
            }
    SAME_TRY(same_use(ctx));
    same_score_map *m = new (std::nothrow) same_score_map();
    if (!m) return SAME_ENOMEM;
    m->ctx = ctx;
    m->mov = mov;
    m->ref = ref;
    *out = m;                                     // freed by the caller's destroy on any failure below
    const size_t totals_bytes = (size_t)MAP_SLOTS * 2 * MAP_TOTALS * sizeof(unsigned long long);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->totals), totals_bytes));
    HIP_TRY(ctx, hipMemsetAsync(m->totals, 0, totals_bytes, ctx->stream));
    for (MapSlot &s : m->slots) s.sets.laid_anew(1);
    if (truth_row && mov->n > 0) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->truth_row), (size_t)mov->n * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(m->truth_row, truth_row, (size_t)mov->n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (with_tally) {
        const size_t bytes = (size_t)std::max<int64_t>(mov->n, 1) * 4 * sizeof(unsigned);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->tally), bytes));
        HIP_TRY(ctx, hipMemsetAsync(m->tally, 0, bytes, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_score_map_destroy(same_score_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be adding to it
    if (m->truth_row) (void)hipFree(m->truth_row);
    if (m->tally) (void)hipFree(m->tally);
    if (m->totals) (void)hipFree(m->totals);
    for (MapSlot &s : m->slots) release(s.marks);
    delete m;
}

int same_score_map_tally(same_score_map *m, uint32_t *out_tally, int64_t *out_results) {
    if (!m) return SAME_EINVAL;
    same_ctx *ctx = m->ctx;
    REQUIRE(ctx, !out_tally || m->tally);
    SAME_TRY(same_use(ctx));
    if (out_tally && m->mov->n > 0) {
        SAME_COPY(ctx, out_tally, m->tally, (size_t)m->mov->n * 4 * sizeof(unsigned), hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
    }
    if (out_results) {
        std::lock_guard<std::mutex> hold(m->lock);
        *out_results = m->results;
    }
    return SAME_OK;
}

int same_score_map_reset(same_score_map *m) {
    if (!m) return SAME_EINVAL;
    same_ctx *ctx = m->ctx;
    SAME_TRY(same_use(ctx));
    if (m->tally) {
        SAME_FILL(ctx, m->tally, 0, (size_t)std::max<int64_t>(m->mov->n, 1) * 4 * sizeof(unsigned));
        SAME_WAIT(ctx);
    }
    std::lock_guard<std::mutex> hold(m->lock);
    m->results = 0;
    return SAME_OK;
}

int same_merge_acc_score_map(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                             const same_score_detail *detail, same_score_map *map, int ignore_same_type, int node_local,
                             double majority_threshold, int64_t min_flips, same_cell_mark *out_marks, int64_t *out_counts) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out_counts);
    SAME_TRY(require_score_args(ctx, a, mov, ref, tris, majority_threshold));
    REQUIRE(ctx, map && map->mov == mov && map->ref == ref && map->ctx->device == ctx->device);
    REQUIRE(ctx, !detail || (detail->mov == mov && detail->ctx->device == ctx->device));
    REQUIRE(ctx, !detail || !detail->col_of_label || (ref->T == mov->T && ref->types64));
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, Tr = tris ? tris->n_tris : 0;
    unsigned long long h[MAP_TOTALS] = {};
    if (n > 0 || mov->n > 0) {
        MapSlot *slot = nullptr;
        int at = 0;
        SAME_TRY(slot_of(ctx, map, &slot, &at));
        SAME_TRY(ensure_score_work(ctx, a, std::max<int64_t>(mov->n, 1)));
        unsigned long long *both = map->totals + (size_t)at * 2 * MAP_TOTALS;
        if (!slot->sets.fits(1)) {                // a call failed half way: both sets idle again
            InDoubt laying(slot->sets);
            SAME_FILL(ctx, both, 0, (size_t)2 * MAP_TOTALS * sizeof(unsigned long long));
            slot->sets.laid_anew(1);
        }
        if (out_marks) SAME_TRY(ensure(ctx, slot->marks, (size_t)std::max<int64_t>(mov->n, 1) * sizeof(same_cell_mark)));
        const ScoreWork &sw = a->sw;
        InDoubt doubt_score(a->score_sets), doubt(slot->sets);       // the call works in both
        unsigned long long *totals = both + (size_t)slot->sets.set * MAP_TOTALS, *next = both + (size_t)(slot->sets.set ^ 1) * MAP_TOTALS;
        SAME_TRY(score_phases(ctx, a, mov, ref, tris, ignore_same_type, true, totals, next));
        const bool ranks = detail && detail->col_of_label;
        SAME_LAUNCH(ctx, map_nodes_kernel, dim3(grid_for(mov->n)), dim3(NT), 0, mov->n, mov->label_codes, ref->label_codes, map->truth_row,
                    ranks ? detail->col_of_label : nullptr, ranks ? detail->n_labels : 0, ref->types64, mov->T, node_local ? 1 : 0,
                    majority_threshold, min_flips, sw.match_of, sw.node_tri, sw.node_flip,
                    out_marks ? static_cast<uint4 *>(slot->marks.p) : nullptr, map->tally, totals, next);
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
        if (out_marks && mov->n > 0) SAME_COPY(ctx, out_marks, slot->marks.p, (size_t)mov->n * sizeof(same_cell_mark), hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
        doubt_score.sound();
        doubt.sound();
        slot->sets.flip();
        if (h[T_BAD]) {
            ctx->err = "same_merge_acc_score_map: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    {
        std::lock_guard<std::mutex> hold(map->lock);
        ++map->results;
    }
    for (int q = 0; q < MAP_TOTALS; ++q) out_counts[q] = (int64_t)h[q];       // a set's words [1], [3 .. 7] and [8], [9] are out_counts' own
    out_counts[0] = n;
    out_counts[2] = Tr;
    return SAME_OK;
}

}  // extern "C"
