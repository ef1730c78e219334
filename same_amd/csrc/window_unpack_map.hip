// window_unpack_map.hip -- the cell pairs window_unpack.hip counts, kept per moving CELL: window_score_map.hip's reading at cell level.
//
// The reference's paper-scale notebooks unpack the metacell matches to cells and then plot per CELL: examples/tongue/reproduce_figures.ipynb
// cells 15-16 give every protein cell the coordinates and the predicted type of the RNA cell it was put on and colour every spatial
// panel by cell_type == pred_cell_type; examples/luad cells 12-13 colour the cell pairs as in or out of the top k type columns;
// examples/synthetic/data/ground_truth.csv names true pairs of CELLS.  A metacell has no cell id, its label is not a cell's and its type
// row is a mean over its members, so window_score_map.hip's marks answer none of that.  When a set's merge ends the unpack phases keep the
// cell pairs on the device (win::unpack_run with a win::PairReader), both member lists are resident with their joint label codes
// (same_members), and so are the reference members' type rows and the labels' columns (same_unpack_detail).  same_merge_acc_unpack_map
// takes the unpack call's place for a result, with TWO kernels behind the last solve launch:
//
//   pair_of_kernel        one lane per PAIR: pair_of[moving member] = pair (a negative entry -- the pairs of an infeasible row -- is
//                         skipped).  A merge's final rows name a moving row at most once, so a member has at most one pair.
//   member_marks_kernel   one lane per moving MEMBER: the member's pair, its reference member and that one's section row (row_of_member
//                         over the reference offsets), whether the two codes agree, the rank of its label's column in the reference
//                         MEMBER's type row (win::type_rank), the truth bits; the 16-byte mark built in registers and written with ONE
//                         store; its share of the resident tally (32-bit atomics whose result is not used: a sweep's sets may be folded in
//                         from several worker contexts at once); pair_of[member] back to -1; the two truth totals per block
//                         (win::block_totals: one atomic per block and total)
//
// Kernels of their own, not a tail of the solve kernel, for window_unpack_detail.hip's reason: the solver's lanes are long and divergent,
// this is a short balanced gather of T doubles per member.  One lane per member over an uncapped grid, as map_nodes_kernel's: there are no
// LDS bins whose flushes a cap would save, and block_totals counts a block's lanes once.
//
// What a call works in beside the accumulator's unpack buffer lives in the MAP, per calling context (a slot, as window_score_map.hip's):
// pair_of (idle: -1), two sets of the two truth totals under the protocol of work_sets.h (the marks kernel clears the other set), the
// device buffer the marks are written to and a page-locked host block they are copied into -- the caller's out_marks is written by the
// host, only by a call that succeeds (under NEAREST an infeasible row is known only after the last wait).
#include "window_internal.h"

namespace {

using namespace win;

constexpr int NT = SCORE_NT;
enum { T_TRUTH_KNOWN = 0, T_ON_TRUTH = 1 };
static_assert(sizeof(same_member_mark) == 16, "the mark is one 16-byte store");

__device__ __forceinline__ unsigned saturated(int rank) { return rank < 254 ? (unsigned)rank : 254u; }

__global__ __launch_bounds__(NT) void pair_of_kernel(const int32_t *__restrict__ pair_mov, int64_t pairs, int64_t m_mov,
                                                     int32_t *__restrict__ pair_of) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= pairs) return;
    const int32_t i = pair_mov[p];
    if (i >= 0 && i < m_mov) pair_of[i] = (int32_t)p;     // (negative: an infeasible row's, no pair)
}

// marks null: counts and tally only; tally null: no tally; truth null: every member unknown; col_of_label / types_r null: no ranks
__global__ __launch_bounds__(NT) void member_marks_kernel(int64_t m_mov, int64_t m_ref, int64_t pairs, const int64_t *__restrict__ pair_ref,
                                                          const int64_t *__restrict__ roff, int64_t n_ref,
                                                          const int32_t *__restrict__ mcode, const int32_t *__restrict__ rcode,
                                                          const int32_t *__restrict__ truth, const int32_t *__restrict__ col_of_label,
                                                          int n_labels, const double *__restrict__ types_r, int T,
                                                          int32_t *__restrict__ pair_of, uint4 *__restrict__ marks,
                                                          unsigned *__restrict__ tally, unsigned long long *__restrict__ totals,
                                                          unsigned long long *__restrict__ next_totals) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < UNPACK_MAP_TOTALS) next_totals[threadIdx.x] = 0ull;     // the set the NEXT call counts into
    bool known = false, on = false;
    if (i < m_mov) {
        const int32_t p = pair_of[i];
        const int32_t t = truth ? truth[i] : -1;
        unsigned flags = t >= 0 ? SAME_MARK_TRUTH_KNOWN : 0u, strict = 255u, weak = 255u;
        int32_t j = -1, row = -1, pair = -1;
        if (p >= 0) {
            pair_of[i] = -1;                          // back to idle: nobody else reads or resets this member's word
            const int64_t jj = p < pairs ? pair_ref[p] : -1;
            if (jj >= 0 && jj < m_ref) {
                j = (int32_t)jj;
                pair = p;
                row = (int32_t)row_of_member(roff, n_ref, jj);
                const int32_t cm = mcode[i];
                const bool agree = labels_agree(cm, rcode[jj]);
                known = t >= 0;
                on = j == t;
                flags |= SAME_MARK_MATCHED | (agree ? SAME_MARK_TYPE_MATCH : 0u) | (on ? SAME_MARK_ON_TRUTH : 0u);
                const int c = col_of_label && types_r && cm >= 0 && cm < n_labels ? col_of_label[cm] : -1;
                if (c >= 0 && c < T) {
                    int s, w;
                    if (type_rank(types_r + jj * T, T, c, s, w)) {
                        flags |= SAME_MARK_RANKED;
                        strict = saturated(s);
                        weak = saturated(w);
                    }
                }
                if (tally) {
                    unsigned *mine = tally + 3 * i;
                    atomicAdd(&mine[0], 1u);
                    if (agree) atomicAdd(&mine[1], 1u);
                    if (on) atomicAdd(&mine[2], 1u);
                }
            }
        }
        if (marks) marks[i] = make_uint4((unsigned)j, (unsigned)row, (unsigned)pair, flags | strict << 8 | weak << 16);
    }
    const bool flag[2] = {known, on};
    const int word[2] = {T_TRUTH_KNOWN, T_ON_TRUTH};
    block_totals<2>(flag, word, totals);
}

// the two kernels as win::unpack_run's reader: the calling context's slot of the map, its launches, its copies
struct MarksReader : PairReader {
    same_unpack_map *map = nullptr;
    const same_members *mov = nullptr, *ref = nullptr;
    const same_unpack_detail *detail = nullptr;
    bool want_marks = false;
    UnpackMapSlot *slot = nullptr;
    int at = 0;
    unsigned long long h[UNPACK_MAP_TOTALS] = {};
    bool ran = false;                             // the kernels were enqueued: the marks are the device's

    int lay(same_ctx *ctx) override {
        {
            std::lock_guard<std::mutex> hold(map->lock);
            for (int q = 0; q < MAP_SLOTS && !slot; ++q)
                if (map->slots[q].owner == ctx || !map->slots[q].owner) {
                    map->slots[q].owner = ctx;
                    slot = &map->slots[q];
                    at = q;
                }
        }
        if (!slot) {
            ctx->err = "same_merge_acc_unpack_map: the map serves no more calling contexts";
            return SAME_ENOMEM;
        }
        sets = &slot->sets;
        const int64_t m = std::max<int64_t>(mov->m, 1);
        if (want_marks) {
            SAME_TRY(ensure(ctx, slot->marks, (size_t)m * sizeof(same_member_mark)));
            if (slot->host_bytes < (size_t)m * sizeof(same_member_mark)) {
                if (slot->host_marks) HIP_TRY(ctx, hipHostFree(slot->host_marks));
                slot->host_marks = nullptr;
                slot->host_bytes = 0;
                HIP_TRY(ctx, hipHostMalloc(&slot->host_marks, (size_t)m * sizeof(same_member_mark), hipHostMallocDefault));
                slot->host_bytes = (size_t)m * sizeof(same_member_mark);
            }
        }
        if (sets->fits(m)) return SAME_OK;
        InDoubt laying(*sets);                    // anew, or a call failed half way: pair_of idle and both sets of totals zero again
        SAME_TRY(ensure(ctx, slot->pair_of, (size_t)m * sizeof(int32_t)));
        SAME_FILL(ctx, slot->pair_of.p, 0xFF, (size_t)m * sizeof(int32_t));
        SAME_FILL(ctx, map->totals + (size_t)at * 2 * UNPACK_MAP_TOTALS, 0, (size_t)2 * UNPACK_MAP_TOTALS * sizeof(unsigned long long));
        sets->laid_anew(m);
        return SAME_OK;
    }
    int enqueue(same_ctx *ctx, const DevicePairs &p) override {
        unsigned long long *both = map->totals + (size_t)at * 2 * UNPACK_MAP_TOTALS;
        unsigned long long *totals = both + (size_t)sets->set * UNPACK_MAP_TOTALS, *next = both + (size_t)(sets->set ^ 1) * UNPACK_MAP_TOTALS;
        int32_t *pair_of = static_cast<int32_t *>(slot->pair_of.p);
        const bool ranks = detail && detail->col_of_label && detail->types;
        SAME_LAUNCH(ctx, pair_of_kernel, dim3(grid_for(p.pairs)), dim3(NT), 0, p.mov_member, p.pairs, mov->m, pair_of);
        SAME_LAUNCH(ctx, member_marks_kernel, dim3(grid_for(mov->m)), dim3(NT), 0, mov->m, ref->m, p.pairs, p.ref_member, ref->off, ref->n_rows,
                    mov->code, ref->code, map->truth, ranks ? detail->col_of_label : nullptr, ranks ? detail->n_labels : 0,
                    ranks ? detail->types : nullptr, ranks ? detail->T : 0, pair_of,
                    want_marks ? static_cast<uint4 *>(slot->marks.p) : nullptr, map->tally, totals, next);
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
        if (want_marks && mov->m > 0)
            SAME_COPY(ctx, slot->host_marks, slot->marks.p, (size_t)mov->m * sizeof(same_member_mark), hipMemcpyDeviceToHost);
        ran = true;
        return SAME_OK;
    }
};

}  // namespace

extern "C" {

int same_unpack_map_create(const same_members *mov, const same_members *ref, const int32_t *truth_member, int with_tally,
                           same_unpack_map **out) {
    if (!mov || !out) return SAME_EINVAL;
    same_ctx *ctx = mov->ctx;
    *out = nullptr;
    REQUIRE(ctx, ref && ref->ctx->device == ctx->device);
    if (truth_member)
        for (int64_t i = 0; i < mov->m; ++i)
            if (truth_member[i] < -1 || truth_member[i] >= ref->m) {
                ctx->err = "same_unpack_map_create: a truth member is outside [-1, members of the reference)";
                return SAME_EINVAL;
            }
    SAME_TRY(same_use(ctx));
    same_unpack_map *m = new (std::nothrow) same_unpack_map();
    if (!m) return SAME_ENOMEM;
    m->ctx = ctx;
    m->mov = mov;
    m->ref = ref;
    *out = m;                                     // freed by the caller's destroy on any failure below
    const size_t totals_bytes = (size_t)MAP_SLOTS * 2 * UNPACK_MAP_TOTALS * sizeof(unsigned long long);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->totals), totals_bytes));
    HIP_TRY(ctx, hipMemsetAsync(m->totals, 0, totals_bytes, ctx->stream));
    if (truth_member && mov->m > 0) {
        m->h_truth.assign(truth_member, truth_member + mov->m);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->truth), (size_t)mov->m * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(m->truth, m->h_truth.data(), (size_t)mov->m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (with_tally) {
        const size_t bytes = (size_t)std::max<int64_t>(mov->m, 1) * 3 * sizeof(unsigned);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->tally), bytes));
        HIP_TRY(ctx, hipMemsetAsync(m->tally, 0, bytes, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_unpack_map_destroy(same_unpack_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be adding to it
    if (m->truth) (void)hipFree(m->truth);
    if (m->tally) (void)hipFree(m->tally);
    if (m->totals) (void)hipFree(m->totals);
    for (UnpackMapSlot &s : m->slots) {
        release(s.marks);
        release(s.pair_of);
        if (s.host_marks) (void)hipHostFree(s.host_marks);
    }
    delete m;
}

int same_unpack_map_tally(same_unpack_map *m, uint32_t *out_tally, int64_t *out_results) {
    if (!m) return SAME_EINVAL;
    same_ctx *ctx = m->ctx;
    REQUIRE(ctx, !out_tally || m->tally);
    SAME_TRY(same_use(ctx));
    if (out_tally && m->mov->m > 0) {
        SAME_COPY(ctx, out_tally, m->tally, (size_t)m->mov->m * 3 * sizeof(unsigned), hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
    }
    if (out_results) {
        std::lock_guard<std::mutex> hold(m->lock);
        *out_results = m->results;
    }
    return SAME_OK;
}

int same_unpack_map_reset(same_unpack_map *m) {
    if (!m) return SAME_EINVAL;
    same_ctx *ctx = m->ctx;
    SAME_TRY(same_use(ctx));
    if (m->tally) {
        SAME_FILL(ctx, m->tally, 0, (size_t)std::max<int64_t>(m->mov->m, 1) * 3 * sizeof(unsigned));
        SAME_WAIT(ctx);
    }
    std::lock_guard<std::mutex> hold(m->lock);
    m->results = 0;
    return SAME_OK;
}

int same_merge_acc_unpack_map(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy,
                              const same_unpack_detail *detail, same_unpack_map *map, same_member_mark *out_marks, int64_t *out_counts) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out_counts && mov && ref);
    REQUIRE(ctx, map && map->mov == mov && map->ref == ref && map->ctx->device == ctx->device);
    REQUIRE(ctx, !detail || (detail->ref == ref && detail->ctx->device == ctx->device));
    MarksReader reader;
    reader.map = map;
    reader.mov = mov;
    reader.ref = ref;
    reader.detail = detail;
    reader.want_marks = out_marks != nullptr;
    int64_t counts[4] = {0, 0, 0, 0};
    SAME_TRY(unpack_run(a, mov, ref, strategy, counts, nullptr, 0, &reader));
    if (out_marks && mov->m > 0) {
        if (reader.ran) std::memcpy(out_marks, reader.slot->host_marks, (size_t)mov->m * sizeof(same_member_mark));
        else                                      // no pair: nothing was launched, every member is unmatched
            for (int64_t i = 0; i < mov->m; ++i) {
                const bool known = !map->h_truth.empty() && map->h_truth[(size_t)i] >= 0;
                out_marks[i] = same_member_mark{-1, -1, -1, (uint8_t)(known ? SAME_MARK_TRUTH_KNOWN : 0), 255, 255, 0};
            }
    }
    {
        std::lock_guard<std::mutex> hold(map->lock);
        ++map->results;
    }
    for (int q = 0; q < 4; ++q) out_counts[q] = counts[q];
    out_counts[4] = (int64_t)reader.h[T_TRUTH_KNOWN];
    out_counts[5] = (int64_t)reader.h[T_ON_TRUTH];
    return SAME_OK;
}

}  // extern "C"
