// window_unpack_detail.hip -- the cell pairs window_unpack.hip counts, binned: by label pair, by group of the moving row, by type rank.
//
// The reference's LUAD notebook unpacks the metacell matches to cells (examples/luad/reproduce_figures.ipynb cell 12) and then asks of
// every CELL pair whether the moving cell's label is among the k largest type columns of the reference cell it was put on (cell 13,
// FigS19: np.argpartition over the reference cells' type columns, k = 1, 2, 3).  A metacell's type row is a mean over its members, so
// that is another number than window_score_detail.hip's rank count over the metacell rows.  When a set's merge ends everything the
// notebook reads is resident but the reference members' type rows: same_unpack_detail holds them, with the cell-level labels' columns.
//
// same_merge_acc_unpack_detail runs same_merge_acc_unpack's phases (win::unpack_run: they are stated once, in window_unpack.hip) with
// the pairs kept on the device, and ONE kernel more behind the last solve launch:
//
//   unpack_bins_kernel    one lane per PAIR over a capped grid: its cell of the confusion matrix; its moving row's group (the row found
//                         in the moving members' offsets) and whether the two codes agree; the rank of its label's column in the
//                         reference MEMBER's type row (win::type_rank: detail_rows_kernel's rule); a negative entry -- the pairs of an
//                         infeasible row -- is skipped
//
// shaped as detail_rows_kernel is: 32-bit LDS bins sized by the call's own L and G, ONE 64-bit atomic per non-zero bin and block at the
// end, the other set of the bins' buffer cleared on the way (work_sets.h).  The solver's lanes are long and divergent (O(n^3) a row), the
// binning is a short gather of T doubles per pair that wants its lanes balanced however long the lists are and few flushing blocks:
// hence a kernel of its own, not a tail of the solve kernel.  Every count is an integer.
#include "window_internal.h"

namespace {

using namespace win;

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 128;      // blocks of the launch: the rest is strided over, so the flushes stay few beside the pair work
                                     // (detail_rows_kernel's cap, taken over: not measured against others at any pair count)
constexpr int R = SAME_SCORE_RANKS;

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>(ceil_div(n > 0 ? n : 1, NT), MAX_BLOCKS); }

// words of a set, in the order of same_merge_acc_unpack_detail's `out` behind its four counts
__host__ __device__ inline int64_t bin_words(int L, int G) { return (int64_t)L * L + 1 + 2 * ((int64_t)G + 1) + 2 * (R + 1) + 1; }

extern __shared__ unsigned lds_bins[];

// LDS and a set alike: [L*L confusion | unlabelled | (G+1) x (pairs, codes agree) | strict[R+1] | weak[R+1] | untyped]
__global__ __launch_bounds__(NT) void unpack_bins_kernel(const int64_t *__restrict__ pair_ref, const int32_t *__restrict__ pair_mov,
                                                         int64_t pairs, const int64_t *__restrict__ moff, int64_t n_mov, int64_t m_mov,
                                                         int64_t m_ref, const int32_t *__restrict__ mcode,
                                                         const int32_t *__restrict__ rcode, const int32_t *__restrict__ group_of,
                                                         const int32_t *__restrict__ col_of_label, const double *__restrict__ types_r,
                                                         int T, int L, int G, unsigned long long *__restrict__ bins,
                                                         unsigned long long *__restrict__ next_bins, int64_t next_dirty) {
    const int o_unl = L * L, o_grp = o_unl + 1, o_strict = o_grp + 2 * (G + 1), o_weak = o_strict + R + 1, o_unt = o_weak + R + 1,
              words = o_unt + 1;
    const int64_t stride = (int64_t)gridDim.x * NT, first = (int64_t)blockIdx.x * NT + threadIdx.x;
    for (int64_t i = first; i < next_dirty; i += stride) next_bins[i] = 0ull;        // the set the NEXT call counts into
    for (int i = threadIdx.x; i < words; i += NT) lds_bins[i] = 0u;
    __syncthreads();
    for (int64_t p = first; p < pairs; p += stride) {
        const int64_t j = pair_ref[p], i = pair_mov[p];
        if (j < 0 || i < 0 || j >= m_ref || i >= m_mov) continue;                    // an infeasible row's: no pair (the call is refused)
        const int32_t cm = mcode[i], cr = rcode[j];
        const bool lm = cm >= 0 && cm < L, lr = cr >= 0 && cr < L;
        atomicAdd(&lds_bins[lm && lr ? cm * L + cr : o_unl], 1u);
        const int g = group_at(group_of, row_of_member(moff, n_mov, i), G);
        atomicAdd(&lds_bins[o_grp + 2 * g], 1u);
        if (labels_agree(cm, cr)) atomicAdd(&lds_bins[o_grp + 2 * g + 1], 1u);
        const int c = lm && col_of_label && types_r ? col_of_label[cm] : -1;
        bool typed = c >= 0 && c < T;
        if (typed) {
            int strict, weak;
            typed = type_rank(types_r + j * T, T, c, strict, weak);
            if (typed) {
                atomicAdd(&lds_bins[o_strict + (strict < R ? strict : R)], 1u);
                atomicAdd(&lds_bins[o_weak + (weak < R ? weak : R)], 1u);
            }
        }
        if (!typed) atomicAdd(&lds_bins[o_unt], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += NT) {
        const unsigned v = lds_bins[i];
        if (v) atomicAdd(&bins[i], (unsigned long long)v);
    }
}

// the bins kernel as win::unpack_run's reader: its buffer under work_sets.h's protocol, its one launch, its one copy
struct BinsReader : PairReader {
    same_merge_acc *a;
    const same_members *mov, *ref;
    const same_unpack_detail *detail;
    const same_score_detail *groups;
    int G;
    int64_t words;
    std::vector<unsigned long long> h;

    int lay(same_ctx *ctx) override {
        if (sets->fits(words)) return SAME_OK;
        InDoubt laying(*sets);
        SAME_TRY(lay_over(ctx, a->unpack_bins, a->ubw, words));
        SAME_FILL(ctx, a->unpack_bins.p, 0, a->ubw.bytes);
        sets->laid_anew(words);
        return SAME_OK;
    }
    int enqueue(same_ctx *ctx, const DevicePairs &p) override {
        const int L = detail->n_labels;
        unsigned long long *bins = a->ubw.bins + (size_t)sets->set * a->ubw.cap, *next = a->ubw.bins + (size_t)(sets->set ^ 1) * a->ubw.cap;
        SAME_LAUNCH(ctx, unpack_bins_kernel, dim3(blocks_for(std::max(p.pairs, sets->dirty))), dim3(NT), (size_t)words * sizeof(unsigned),
                    p.ref_member, p.mov_member, p.pairs, mov->off, mov->n_rows, mov->m, ref->m, mov->code, ref->code,
                    groups ? groups->group_of : nullptr, detail->col_of_label, detail->types, detail->T, L, G, bins, next, sets->dirty);
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h.data(), bins, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        counted = words;
        return SAME_OK;
    }
};

}  // namespace

extern "C" {

int same_unpack_detail_create(const same_members *ref, int n_labels, const int32_t *col_of_label, const double *ref_member_types, int T,
                              same_unpack_detail **out) {
    if (!ref || !out) return SAME_EINVAL;
    same_ctx *ctx = ref->ctx;
    *out = nullptr;
    REQUIRE(ctx, n_labels >= 0 && n_labels <= SAME_SCORE_MAX_LABELS && T >= 0);
    REQUIRE(ctx, !col_of_label || (ref_member_types && T > 0));
    if (col_of_label)
        for (int q = 0; q < n_labels; ++q)
            if (col_of_label[q] < -1 || col_of_label[q] >= T) {
                ctx->err = "same_unpack_detail_create: a col_of_label value is outside [-1, T)";
                return SAME_ERANGE;
            }
    SAME_TRY(same_use(ctx));
    same_unpack_detail *d = new (std::nothrow) same_unpack_detail();
    if (!d) return SAME_ENOMEM;
    d->ctx = ctx;
    d->ref = ref;
    d->n_labels = n_labels;
    d->T = T;
    *out = d;                                     // freed by the caller's destroy on any failure below
    if (col_of_label && n_labels > 0) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d->col_of_label), (size_t)n_labels * sizeof(int32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(d->col_of_label, col_of_label, (size_t)n_labels * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (ref_member_types && T > 0 && ref->m > 0) {
        const size_t bytes = (size_t)ref->m * (size_t)T * sizeof(double);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d->types), bytes));
        HIP_TRY(ctx, hipMemcpyAsync(d->types, ref_member_types, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_unpack_detail_destroy(same_unpack_detail *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (d->col_of_label) (void)hipFree(d->col_of_label);
    if (d->types) (void)hipFree(d->types);
    delete d;
}

int same_merge_acc_unpack_detail(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy,
                                 const same_unpack_detail *detail, const same_score_detail *groups, int64_t *out, int64_t out_words) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out && mov && ref);
    REQUIRE(ctx, detail && detail->ref == ref && detail->ctx->device == ctx->device);
    REQUIRE(ctx, !groups || (groups->mov == mov->sec && groups->ctx->device == ctx->device));
    BinsReader reader;
    reader.a = a;
    reader.mov = mov;
    reader.ref = ref;
    reader.detail = detail;
    reader.groups = groups;
    reader.G = groups ? groups->n_groups : 1;
    reader.words = bin_words(detail->n_labels, reader.G);
    reader.sets = &a->unpack_bin_sets;
    REQUIRE(ctx, out_words >= 4 + reader.words);
    reader.h.assign((size_t)reader.words, 0ull);
    int64_t counts[4] = {0, 0, 0, 0};
    SAME_TRY(unpack_run(a, mov, ref, strategy, counts, nullptr, 0, &reader));
    for (int q = 0; q < 4; ++q) out[q] = counts[q];
    for (int64_t q = 0; q < reader.words; ++q) out[4 + q] = (int64_t)reader.h[(size_t)q];
    return SAME_OK;
}

}  // extern "C"
