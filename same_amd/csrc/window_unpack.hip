// window_unpack.hip -- a merged MetaCell result unpacked to cells where its rows are: on the device.
//
// The reference's paper-scale flows match metacells and read the result at cell level: unpack_metacell_matches
// (src/metacell_utils.py:564-766) turns every metacell match (a, r) into one pair per member of a, each with a member of r -- dealt
// round-robin ('distribute', member i takes reference member i % nr) or by the optimal assignment of the members' pairwise distances
// ('nearest', the reference columns tiled when there are more aligned members) -- and the notebooks then count the pairs and those whose
// two cells carry the same label.  After same_merge_acc_finish the matches are resident as final rows (moving section row, reference
// section row); the two sides' member lists, the members' XY and their joint label codes are constant over a study and resident beside
// the sections (same_members).  same_merge_acc_unpack counts there, and writes the pairs only where somebody asks for them.
//
//   unpack_size_kernel    per final row: its pairs (the moving row's members) and, under NEAREST, the solver's work slice
//                         (assign_solve::slice_words) in units of UNPACK_UNIT words; ONE exclusive scan (scan.h) makes them the row's
//                         first pair and the start of its slice; the largest list met, rows outside the members, rows that pair members
//                         with an empty reference list
//   unpack_solve_kernel   one lane per final row: the row's pairs -- under NEAREST by assign_solve::solve, the statement
//                         same_batched_assign's kernel runs, in the lane's slice of a global work buffer --, the flat reference member
//                         of every pair where they are asked for, and the pairs whose two codes agree, one atomic per block
//
// The slices' buffer is bounded: rows whose slices start in [c * budget, (c + 1) * budget) are one launch of the solve kernel, and the
// buffer holds a budget plus one largest slice -- it does not grow with the section.  Every count is an integer.
//
// The phases are stated once, in win::unpack_run: same_merge_acc_unpack is that function, and same_merge_acc_unpack_detail
// (window_unpack_detail.hip) is that function with a win::PairReader -- the pairs then stay on the device, with their moving members
// beside them, and the reader's one kernel bins them between the last solve launch and the call's last wait.
#include "assign_solve.h"
#include "window_internal.h"

#include <cstdlib>

namespace {

using namespace win;

constexpr int NT = scan::NT;
// words of a set of totals
enum { T_PAIRS = 0, T_UNITS = 1, T_TYPE = 2, T_MAX = 3, T_FLAGS = 4 };
enum { F_OUTSIDE = 1u, F_EMPTY_REF = 2u, F_INFEASIBLE = 4u };
constexpr int64_t BUDGET_UNITS = (int64_t)1 << 19;          // 64 MiB of slices per launch of the solve kernel

struct Lists {
    const int64_t *moff, *roff;
    int64_t n_mov, n_ref;
};
struct RowLists {
    int64_t a0 = 0, r0 = 0;
    int na = 0, nr = 0;
    bool inside = false;
};
__device__ __forceinline__ RowLists lists_of(const FinalRec &row, const Lists &l) {
    RowLists out;
    const int32_t a = row.a_row, r = row.r_row;
    out.inside = followed(row, l.n_mov, l.n_ref);
    if (out.inside) {
        out.a0 = l.moff[a];
        out.r0 = l.roff[r];
        out.na = (int)(l.moff[a + 1] - out.a0);
        out.nr = (int)(l.roff[r + 1] - out.r0);
    }
    return out;
}
__host__ __device__ inline unsigned slice_units(int64_t na, int64_t nc) {
    return (unsigned)((assign_solve::slice_words(na, nc) + UNPACK_UNIT - 1) / UNPACK_UNIT);
}
// what the scan adds up per final row: (pairs, units of the solver's slice); a row that yields no pair adds nothing
__device__ __forceinline__ scan::Pair sizes_of(const RowLists &q, int nearest) {
    if (q.na == 0 || q.nr == 0) return scan::Pair{0u, 0u};
    return scan::Pair{(unsigned)q.na, nearest ? slice_units(q.na, assign_solve::columns(q.na, q.nr)) : 0u};
}

__global__ __launch_bounds__(NT) void unpack_size_kernel(const FinalRec *__restrict__ rows, int64_t n, Lists l, int nearest,
                                                         unsigned long long *status, unsigned *__restrict__ pair_off,
                                                         unsigned *__restrict__ work_off, unsigned long long *__restrict__ totals,
                                                         unsigned long long *__restrict__ next_status, int64_t status_words,
                                                         unsigned long long *__restrict__ next_totals) {
    __shared__ scan::Shared sh;
    __shared__ unsigned part_max[NT / 64], part_flags[NT / 64];
    // the set the NEXT call counts into (nobody reads it during this call)
    for (int64_t w = (int64_t)blockIdx.x * NT + threadIdx.x; w < status_words; w += (int64_t)gridDim.x * NT) next_status[w] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < UNPACK_TOTALS) next_totals[threadIdx.x] = 0ull;
    auto val = [&](int64_t i) { return i < n ? sizes_of(lists_of(rows[i], l), nearest) : scan::Pair{0u, 0u}; };
    scan::Pair through;
    const scan::Pair off = scan::exclusive(status, (int)blockIdx.x, val, sh, &through);
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    unsigned most = 0u, flags = 0u;
    if (i < n) {
        const RowLists q = lists_of(rows[i], l);
        pair_off[i] = off.a;
        work_off[i] = off.p;
        most = (unsigned)(q.na > q.nr ? q.na : q.nr);
        flags = (q.inside ? 0u : F_OUTSIDE) | (q.na > 0 && q.nr == 0 ? F_EMPTY_REF : 0u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned m2 = __shfl_xor(most, d, 64), f2 = __shfl_xor(flags, d, 64);
        most = most > m2 ? most : m2;
        flags |= f2;
    }
    if ((threadIdx.x & 63) == 0) { part_max[threadIdx.x >> 6] = most; part_flags[threadIdx.x >> 6] = flags; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < NT / 64; ++q) { most = most > part_max[q] ? most : part_max[q]; flags |= part_flags[q]; }
        if (most) atomicMax(&totals[T_MAX], (unsigned long long)most);
        if (flags) atomicOr(&totals[T_FLAGS], (unsigned long long)flags);
        if (blockIdx.x == gridDim.x - 1) {
            totals[T_PAIRS] = through.a;
            totals[T_UNITS] = through.p;
        }
    }
}

// rows whose slice starts in [lo, lo + span) units (DISTRIBUTE: every row, no slices); out_ref null: only the count; out_mov (with
// out_ref, for a reader of the pairs on the device): the pair's flat moving member too, and -1 in both for the pairs of an infeasible row
__global__ __launch_bounds__(NT) void unpack_solve_kernel(const FinalRec *__restrict__ rows, int64_t n, Lists l, int nearest,
                                                          const double *__restrict__ mxy, const double *__restrict__ rxy,
                                                          const int32_t *__restrict__ mcode, const int32_t *__restrict__ rcode,
                                                          const unsigned *__restrict__ pair_off, const unsigned *__restrict__ work_off,
                                                          int64_t lo, int64_t span, double *__restrict__ slices,
                                                          int64_t *__restrict__ out_ref, int32_t *__restrict__ out_mov,
                                                          unsigned long long *__restrict__ totals) {
    __shared__ unsigned part[NT / 64];
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    unsigned agree = 0u;
    bool infeasible = false;
    if (i < n) {
        const RowLists q = lists_of(rows[i], l);
        const int64_t wo = nearest ? (int64_t)work_off[i] : lo;
        if (q.na > 0 && q.nr > 0 && wo >= lo && wo < lo + span) {
            const int64_t first = pair_off[i];
            const int *col4row = nullptr;
            if (nearest) {
                col4row = assign_solve::solve(q.na, q.nr, mxy + 2 * q.a0, rxy + 2 * q.r0, slices + (wo - lo) * UNPACK_UNIT);
                infeasible = col4row == nullptr;
            }
            if (!infeasible)
                for (int k = 0; k < q.na; ++k) {
                    const int64_t member = q.r0 + (nearest ? col4row[k] : k) % q.nr;
                    agree += labels_agree(mcode[q.a0 + k], rcode[member]) ? 1u : 0u;
                    if (out_ref) out_ref[first + k] = member;
                    if (out_mov) out_mov[first + k] = (int32_t)(q.a0 + k);
                }
            else if (out_mov)                      // a reader of the pairs on the device skips them: nothing of this row is a pair
                for (int k = 0; k < q.na; ++k) {
                    out_ref[first + k] = -1;
                    out_mov[first + k] = -1;
                }
        }
    }
    const bool any_infeasible = __ballot(infeasible) != 0ull;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) agree += __shfl_xor(agree, d, 64);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = agree;
        if (any_infeasible) atomicOr(&totals[T_FLAGS], (unsigned long long)F_INFEASIBLE);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < NT / 64; ++q) agree += part[q];
        if (agree) atomicAdd(&totals[T_TYPE], (unsigned long long)agree);
    }
}

// units of slices one launch of the solve kernel may start (SAME_UNPACK_BUDGET_UNITS: a test switch, as scan::arg's)
int64_t budget_units() {
    const char *e = getenv("SAME_UNPACK_BUDGET_UNITS");
    const long long v = e && e[0] ? atoll(e) : 0;
    return v > 0 ? (int64_t)v : BUDGET_UNITS;
}

}  // namespace

extern "C" {

int same_members_create(const same_section *sec, const int64_t *off, const double *member_xy, const int32_t *member_code, int64_t m,
                        same_members **out) {
    if (!sec || !out) return SAME_EINVAL;
    same_ctx *ctx = sec->ctx;
    *out = nullptr;
    REQUIRE(ctx, off && m >= 0 && m < ((int64_t)1 << 31) && (m == 0 || (member_xy && member_code)));
    const int64_t n = sec->n;
    REQUIRE(ctx, off[0] == 0 && off[n] == m);
    int64_t most = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t count = off[i + 1] - off[i];
        REQUIRE(ctx, count >= 0 && count <= SAME_ASSIGN_MAX_MEMBERS);
        most = std::max(most, count);
    }
    SAME_TRY(same_use(ctx));
    same_members *mb = new (std::nothrow) same_members();
    if (!mb) return SAME_ENOMEM;
    mb->ctx = ctx;
    mb->sec = sec;
    mb->n_rows = n;
    mb->m = m;
    mb->max_count = most;
    *out = mb;                                    // freed by the caller's destroy on any failure below
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&mb->off), (size_t)(n + 1) * sizeof(int64_t)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&mb->xy), mm * 2 * sizeof(double)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&mb->code), mm * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(mb->off, off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (m) {
        HIP_TRY(ctx, hipMemcpyAsync(mb->xy, member_xy, (size_t)m * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(mb->code, member_code, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_members_destroy(same_members *mb) {
    if (!mb) return;
    (void)hipSetDevice(mb->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (mb->off) (void)hipFree(mb->off);
    if (mb->xy) (void)hipFree(mb->xy);
    if (mb->code) (void)hipFree(mb->code);
    delete mb;
}

int same_merge_acc_unpack(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy, int64_t *out_counts,
                          int64_t *out_ref_member, int64_t capacity) {
    return win::unpack_run(a, mov, ref, strategy, out_counts, out_ref_member, capacity, nullptr);
}

}  // extern "C"

namespace win {

// The calls that unpack (same_merge_acc_unpack: reader null; same_merge_acc_unpack_detail: its bins kernel the reader) -- every phase
// stated here alone.  With a reader nothing is written through out_ref_member and out_counts is written only by a call that succeeds.
int unpack_run(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy, int64_t *out_counts,
               int64_t *out_ref_member, int64_t capacity, PairReader *reader) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out_counts && has_merged_rows(a));
    REQUIRE(ctx, strategy == SAME_UNPACK_DISTRIBUTE || strategy == SAME_UNPACK_NEAREST);
    REQUIRE(ctx, mov && ref && mov->ctx->device == ctx->device && ref->ctx->device == ctx->device);
    REQUIRE(ctx, mov->sec == a->pass_mov && ref->sec == a->pass_ref);
    REQUIRE(ctx, !out_ref_member || capacity >= 0);
    REQUIRE(ctx, !reader || !out_ref_member);
    SAME_TRY(same_use(ctx));
    const int nearest = strategy == SAME_UNPACK_NEAREST;
    const int64_t n = a->n_final;
    unsigned long long h[UNPACK_TOTALS] = {};
    if (n > 0) {
        // the largest slice any row of these members can ask for; the scan adds the rows' units in 31 bits
        const int64_t unit_max = slice_units(std::max<int64_t>(mov->max_count, 1), std::max<int64_t>(mov->max_count + ref->max_count, 1));
        REQUIRE(ctx, !nearest || n * unit_max < ((int64_t)1 << 31));
        WorkSets &us = a->unpack_sets;
        if (!us.fits(n)) {
            InDoubt laying(us);
            SAME_TRY(lay_over(ctx, a->unpack, a->uw, n));
            SAME_FILL(ctx, a->unpack.p, 0, a->uw.zero_bytes);
            us.laid_anew(n);
        }
        if (reader) SAME_TRY(reader->lay(ctx));
        WorkSets nobody;
        WorkSets &rs = reader ? *reader->sets : nobody;       // the reader's buffer is in doubt whenever this one is
        const UnpackWork &uw = a->uw;
        InDoubt doubt(us), doubt_reader(rs);
        const int set = us.set;
        unsigned long long *totals = uw.totals + (size_t)set * UNPACK_TOTALS, *next = uw.totals + (size_t)(set ^ 1) * UNPACK_TOTALS;
        const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
        const Lists l{mov->off, ref->off, mov->n_rows, ref->n_rows};
        SAME_LAUNCH(ctx, unpack_size_kernel, dim3(scan::blocks_for(n)), dim3(NT), 0, fin, n, l, nearest, scan::arg(uw.status[set]), uw.pair_off,
                    uw.work_off, totals, uw.status[set ^ 1], (int64_t)uw.status_words, next);
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
        doubt.sound();
        doubt_reader.sound();
        us.flip();                                            // the call's one flip: the phases below work on in the set it counted into
        if (h[T_FLAGS] & F_OUTSIDE) {
            ctx->err = "same_merge_acc_unpack: final rows outside the members' sections";
            return SAME_ERANGE;
        }
        if (h[T_FLAGS] & F_EMPTY_REF) {
            ctx->err = "same_merge_acc_unpack: a final row pairs members with a reference row that has none";
            return SAME_ERANGE;
        }
        const int64_t pairs = (int64_t)h[T_PAIRS], units = (int64_t)h[T_UNITS];
        const bool too_small = out_ref_member && capacity < pairs;
        const bool write = out_ref_member && !too_small && pairs > 0;
        if (pairs > 0) {
            const int64_t budget = budget_units(), chunks = nearest ? std::max<int64_t>((units + budget - 1) / budget, 1) : 1;
            double *slices = nullptr;
            int64_t *dref = nullptr;
            int32_t *dmov = nullptr;
            if (nearest) {
                SAME_TRY(ensure(ctx, a->unpack_slices, (size_t)(chunks > 1 ? budget + unit_max : units) * UNPACK_UNIT * 8));
                slices = static_cast<double *>(a->unpack_slices.p);
            }
            if (write || reader) {
                // [pairs] int64 reference members, then -- for a reader -- [pairs] int32 moving members
                SAME_TRY(ensure(ctx, a->unpack_pairs, (size_t)pairs * (sizeof(int64_t) + (reader ? sizeof(int32_t) : 0))));
                dref = static_cast<int64_t *>(a->unpack_pairs.p);
                if (reader) dmov = reinterpret_cast<int32_t *>(dref + pairs);
            }
            InDoubt solving(us), solving_reader(rs);
            for (int64_t c = 0; c < chunks; ++c)
                SAME_LAUNCH(ctx, unpack_solve_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, l, nearest, mov->xy, ref->xy, mov->code, ref->code,
                            uw.pair_off, uw.work_off, c * budget, budget, slices, dref, dmov, totals);
            HIP_TRY(ctx, hipGetLastError());
            if (reader) SAME_TRY(reader->enqueue(ctx, DevicePairs{dref, dmov, pairs}));
            SAME_COPY(ctx, h, totals, sizeof h, hipMemcpyDeviceToHost);
            SAME_WAIT(ctx);
            solving.sound();
            solving_reader.sound();
            if (reader) rs.flip(reader->counted);             // (whatever the answer: the next call clears what this one counted)
            if (h[T_FLAGS] & F_INFEASIBLE) {
                ctx->err = "same_merge_acc_unpack: a cost matrix is infeasible (non-finite coordinates)";
                return SAME_ERANGE;
            }
            if (write) {
                InDoubt copying(us);
                SAME_COPY(ctx, out_ref_member, dref, (size_t)pairs * sizeof(int64_t), hipMemcpyDeviceToHost);
                SAME_WAIT(ctx);
                copying.sound();
            }
        }
        out_counts[0] = n;
        out_counts[1] = pairs;
        out_counts[2] = (int64_t)h[T_TYPE];
        out_counts[3] = (int64_t)h[T_MAX];
        if (too_small) {
            ctx->err = "same_merge_acc_unpack: out_ref_member holds fewer than out_counts[1] entries";
            return SAME_EINVAL;
        }
        return SAME_OK;
    }
    for (int q = 0; q < 4; ++q) out_counts[q] = 0;
    return SAME_OK;
}

}  // namespace win
