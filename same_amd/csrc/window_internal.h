// window_internal.h -- what the translation units of the device-resident window path share (section.hip, window_stage.hip,
// window_finish.hip, window_merge.hip, window_score.hip, window_score_detail.hip, window_score_map.hip, window_score_feature.hip, window_unpack.hip, window_unpack_detail.hip, window_unpack_feature.hip, window_unpack_map.hip, window_caller.hip, window_priority.hip, window_knn_prefix.hip, window_recost.hip): the resident objects behind the
// opaque handles of include/same_hip.h part 4, the per-launch argument blocks, the device side of a window's pair list, the window's
// logical state (window_state.h: win::State, with the table of what each call requires, leaves and invalidates), the protocol of the merged
// rows' reader calls (work_sets.h: win::WorkSets), the small host helpers and the batch driver of the window calls.
//
// The window path (src/same.py:507-593 with both sections RESIDENT on the device).  A section's columns are uploaded once
// (same_section) and its rows are binned once into a grid of cells (same_section_bin: rows sorted by cell, ascending inside a cell)
// -- SURVEY a13's "one-pass bin".  A BATCH of windows is then two calls (window_stage.hip, window_finish.hip), and a third that
// enqueues only (window_merge.hip: the rows of the windows' central regions appended to the pass's merge accumulator).
//
// Every kernel takes up to SAME_LAUNCH_WINDOWS (8) windows per launch: blockIdx.y = window, the per-window arguments -- pointers into
// the window's OWN buffers, its counts -- travel by value in the kernarg segment (Batch<Args>), the grid is sized by the group's largest
// window and blocks beyond a window's share leave at once.  Nothing a call computes is sized by a number the host has to wait for:
// lists are allocated for the candidates of the covered cells (known from the host's copy of the cell offsets), their true lengths
// stay in a counter block on the device and every kernel reads them there.  same_ctx_stat counts the runtime calls.
//
// WHO MAY TOUCH WHAT -- the threading contract of this path.  A context (same_ctx) is one stream and is used by one thread at a time
// (the Python binding holds Context.lock around every call).  Windows and merge accumulators belong to ONE context.  Sections are
// shared by the worker threads' contexts; two locks guard them:
//
//   same_section::grid_lock  (std::shared_mutex)   guards  grid, order, starts, h_starts, n_binned.
//       shared:     every same_window_stage call, from cover_of() until its last kernel is ENQUEUED (the kernels read `order` /
//                   `starts` by the pointers they were launched with).
//       exclusive:  same_section_bin's swap of the five fields.  It first builds the new index WITHOUT the lock, then takes the lock
//                   (no stage call is between cover_of() and its last enqueue), waits for the DEVICE (hipDeviceSynchronize: kernels
//                   enqueued earlier by any context may still read the old arrays), frees the old arrays and stores the new ones.
//   same_section::lock       (std::mutex)          guards  the table `knn` (radius -> prune index, most recently used first, <= 16).
//       held only for look-ups, insertions and evictions of table entries -- NEVER across device work: an index that is not in the
//       table is built by the calling thread on its own context with the lock released, and inserted afterwards (a thread that lost the
//       race to another builder of the same radius drops its build and takes the winner's).  Entries are shared_ptr: a stage call keeps
//       the index it prunes with until its kernels have finished, so an entry evicted meanwhile is freed by its last user, after
//       the lock is let go (hipFree waits for the device).
//
//   Nothing else of a section changes after same_section_create (xy, types, sizes, type codes, id codes are written once, before the
//   handle is handed out; same_section_set_codes must precede the first collect call that reads the codes, same_section_set_label_codes
//   the first same_window_priority_pairs call).
//   same_section_destroy expects that no call is using the section (it waits for the device, not for threads).
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <utility>
#include <vector>

#include "common.h"
#include "devmath.h"
#include "scan.h"
#include "window_state.h"
#include "work_sets.h"

struct same_knn_index;
extern "C" int same_knn_index_build(same_ctx *ctx, const double *drxy, int64_t n_r, double radius, same_knn_index **out);
extern "C" void same_knn_index_destroy(same_knn_index *ix);

namespace win {

constexpr int MAX_RUN_CELLS = 64;        // cells of a section's grid one window may cover on the cell-run path
constexpr int64_t MAX_GRID_CELLS = (int64_t)1 << 22;
constexpr unsigned OUTSIDE = 0x80000000u;   // flag on a candidate row that fails the box test

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

inline int ensure(same_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.bytes && b.p) return SAME_OK;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    if (b.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.bytes = want;
    return SAME_OK;
}
inline void release(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// A buffer's layout is ONE sequence of typed takes, run twice: without a base it measures (every take answers null, `off` ends at the
// size to ensure), on the allocation it places the pointers -- so a size and its pointers cannot disagree.  take: the array starts on a
// 256-byte boundary and the buffer is padded to the next one; pack: the array starts on `align` bytes and nothing is padded behind it (runs
// that are zeroed or copied back in one piece).  `off`, and what align() answers, are offsets where an offset itself is data.
struct Carver {
    char *base = nullptr;
    size_t off = 0;
    explicit Carver(void *b = nullptr) : base(static_cast<char *>(b)) {}
    size_t align(size_t a) { return off = (off + a - 1) & ~(a - 1); }
    template <class T>
    T *pack(size_t count, size_t a = alignof(T)) {
        const size_t at = align(a);
        off = at + count * sizeof(T);
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    template <class T>
    T *take(size_t count) {
        T *p = pack<T>(count, 256);
        align(256);
        return p;
    }
    unsigned long long *scan_words(int64_t n) { return take<unsigned long long>(scan::status_bytes(n) / 8); }   // status_bytes: 16-byte units
};
// `w` laid over `buf` for n (a lay(Work &, Carver &, int64_t) says how): measured, the buffer ensured, the pointers placed
template <class Work>
int lay_over(same_ctx *ctx, DevBuf &buf, Work &w, int64_t n) {
    Work probe;
    Carver measure;
    lay(probe, measure, n);
    SAME_TRY(ensure(ctx, buf, probe.bytes));
    Carver place(buf.p);
    lay(w, place, n);
    return SAME_OK;
}

inline unsigned grid_for(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, 256); }

// ---- the section's grid of cells -------------------------------------------------------------------------------------------
// cell (cx, cy) = [x0 + cx*cw, x0 + (cx+1)*cw) x [y0 + cy*ch, y0 + (cy+1)*ch): a row belongs to the cell whose edges -- these
// very doubles -- bracket it under the comparisons of src/same.py:293-295, so a box whose edges are cell edges needs no test.
struct BinGrid {
    double x0 = 0.0, y0 = 0.0, cw = 1.0, ch = 1.0;
    int nx = 1, ny = 1;
};
__host__ __device__ inline double cell_edge(double origin, double width, int c) { return origin + (double)c * width; }

// Every kernel of the window calls takes the windows of a batch in ONE launch: blockIdx.y = window, the per-window arguments travel by
// value in the kernarg segment (Batch<A>, at most SAME_LAUNCH_WINDOWS windows); the grid is sized by the largest window and blocks
// beyond a window's own share leave at once.
template <typename A>
struct Batch {
    A w[SAME_LAUNCH_WINDOWS];
};

// the heads of the windows' buffers zeroed in one launch (scan words, counters, marks): up to two 16-byte aligned regions per window
struct ZeroArgs {
    void *p[2];
    size_t bytes[2];
};

struct CopyArgs {
    const void *src[2];
    void *dst[2];
    size_t bytes[2];
};

// One section's share of a window in window_rows_kernel (window_stage.hip): the candidates of the covered cells, merged ascending.  The
// caller's triangulation (window_caller.hip) walks its triangles by cell through the same kernel: `order` then lists triangle numbers.
struct RunDesc {
    const int32_t *order;      // the section's rows by cell
    const unsigned *starts;    // cell offsets into `order`
    const double *xy;          // section XY (box test of the candidates)
    int nx, cx0, ncx, cy0, ncy;   // covered cells: [cx0, cx0 + ncx) x [cy0, cy0 + ncy), ncx * ncy <= MAX_RUN_CELLS
    int n_cand;                // rows in those cells (the host knows the cell offsets)
    int aligned;               // the box is a union of cells: every candidate is inside
    uint32_t *merged;          // out: the candidates ascending by row (| OUTSIDE where the box test fails)
    unsigned long long *count; // out, aligned only: n_cand
};
struct RowsArgs {
    RunDesc dm, dr;
    unsigned blocks_m, blocks;     // blocks [0, blocks_m) walk the moving section's candidates, [blocks_m, blocks) the reference's
    double bx0, bx1, by0, by1;
};

// covered cells of a box in a section's grid, and whether the box is exactly their union (section.hip)
struct Cover {
    int cx0 = 0, ncx = 0, cy0 = 0, ncy = 0;
    int64_t n_cand = 0;
    bool aligned = false, use_runs = false;
};

// counters of the filter: [0] kept (class 0), [1] added back, [2] cosines within `tol` of the threshold, [3] triangles left
enum { FC_KEEP = 0, FC_ADD = 1, FC_NEAR = 2, FC_TR = 3, FC_TIES = 4, FC_COPIED = 5 };
// counters of the finish call: [0] orientation checked, [1] flipped, [2] XY comparisons, [3] XY violations, [4] triangles with
// one, [5] area flips, [6] (host) greedy rounds, [7] matched aligned cells, [8] pairs the greedy rule could still take; from
// SC_REFINE on the local search's control words (refine.h RC_*), which a second pass of the tail leaves as they are
enum { SC_CHECKED = 0, SC_FLIPPED = 1, SC_CMP = 2, SC_VIOL = 3, SC_TVIOL = 4, SC_AFLIP = 5, SC_ROUNDS = 6, SC_MATCHED = 7, SC_REMAINING = 8, SC_TIES = 9,
       SC_REFINE = 16, SC_COUNT = 32 };

// What the finish call copies back in one piece, [sel | counters | point flags | matched rows], and zeroes up to the matched rows:
// laid out here because the stage call sizes the pinned block's share for it (finish_back_bytes) before the finish call places it
struct FinishBack {
    unsigned long long *sel = nullptr, *counters = nullptr;   // [SAME_GREEDY_BATCH_MAX] greedy rounds, [SC_COUNT]
    uint8_t *pflag = nullptr;                                 // [n] padded to whole 16 bytes (its writers OR into 32-bit words)
    int32_t *match_row = nullptr;                             // [n]
    size_t back_off = 0, zero_bytes = 0, back_bytes = 0;      // the region's start, the end of the zeroed head; the region's size
    size_t o_counters = 0, o_pflag = 0, o_match_row = 0;      // from the region's start: where the host finds them in its copy
};
inline void lay(FinishBack &b, Carver &cv, int64_t n) {
    b.back_off = cv.align(256);
    b.sel = cv.take<unsigned long long>(SAME_GREEDY_BATCH_MAX);
    b.o_counters = cv.off - b.back_off;
    b.counters = cv.pack<unsigned long long>(SC_COUNT);
    b.o_pflag = cv.off - b.back_off;
    b.pflag = cv.pack<uint8_t>((size_t)n);
    b.zero_bytes = cv.align(16);
    b.o_match_row = cv.off - b.back_off;
    b.match_row = cv.pack<int32_t>((size_t)n);
    b.back_bytes = cv.off - b.back_off;
}
inline size_t finish_back_bytes(int64_t n) {
    FinishBack b;
    Carver cv;
    lay(b, cv, n);
    return b.back_bytes;
}

// (win::PairList, a window's pair list: window_state.h)
// pair p of `src` becomes pair `at` of `dst` under aligned row a: its reference number, that reference's section row and its cost are
// copied, never recomputed
__device__ __forceinline__ void move_pair(const PairList &dst, int64_t at, int32_t a, const PairList &src, int64_t p) {
    dst.pairs[2 * at] = a;
    dst.pairs[2 * at + 1] = src.pairs[2 * p + 1];
    dst.jsec[at] = src.jsec[p];
    dst.cost64[at] = src.cost64[p];
}

// the tail of a kernel that scans the rows' new pair counts (scan.h): the row's offset (where the thread has a row), and from the
// last block's first thread the end of the last row and the window's pair count (counts[3]) -- the kernel adds its own count words
__device__ __forceinline__ void rows_tail(const PairList &dst, unsigned long long *counts, bool has_row, int64_t row, scan::Pair off, bool last,
                                          int64_t n_rows, scan::Pair through) {
    if (has_row) dst.prow[row] = (int32_t)off.p;
    if (last && threadIdx.x == 0) {
        dst.prow[n_rows] = (int32_t)through.p;
        counts[3] = through.p;
    }
}

}  // namespace win

struct same_section {
    same_ctx *ctx = nullptr;
    int64_t n = 0;
    int T = 0;
    int cost_f32 = 0;
    double *xy = nullptr;     // [n][2]
    void *xy_c = nullptr;     // [n][2] in the cost type (== xy for fp64 costs)
    void *types_c = nullptr;  // [n][T] in the cost type
    double *types64 = nullptr; // [n][T] as the caller gave them (== types_c for fp64 costs): what the result table's type columns are read from
    double *size = nullptr;   // [n]
    int32_t *type_id = nullptr;  // [n] codes of the cell type (equal type <=> equal code), or none
    int32_t *id_codes = nullptr; // [n] rank of the row's cell id among the frame's ids (same_section_set_codes), or none: a row's code is its number
    int64_t n_codes = 0;
    int32_t *label_codes = nullptr; // [n] codes of the cell_type LABELS, joint over the two frames of a job (same_section_set_label_codes), or
                                    // none: equal non-negative codes <=> labels that compare equal (the cell-type-priority prune)
    unsigned long long bins = 0;    // how often the grid below was replaced (under grid_lock): a window remembers the numbers it was staged at
    // the grid of cells (same_section_bin)
    win::BinGrid grid;
    int32_t *order = nullptr;        // [n_binned] rows by cell, ascending inside a cell
    unsigned *starts = nullptr;      // [cells + 1] on the device ...
    std::vector<unsigned> h_starts;  // ... and on the host: a window's candidate count is known without asking the device
    int64_t n_binned = 0;
    // prune indices of this section as the REFERENCE side, one per radius used (built on first use, under the lock: sections are
    // shared by the worker threads' contexts)
    std::mutex lock;
    // most recently used first; at most MAX_KNN_INDICES (the oldest is dropped).  Shared: a stage call holds the index it prunes with
    // until its kernels have finished, so an index dropped from the table meanwhile is freed by its last user
    std::vector<std::pair<double, std::shared_ptr<same_knn_index>>> knn;
    // grid, order, starts, h_starts: read (shared) by every stage call from cover_of() until its kernels are enqueued, replaced
    // (exclusive, after a device-wide wait: kernels enqueued earlier may still be reading the old arrays) by same_section_bin
    std::shared_mutex grid_lock;
};

// A types layer of a section (same_types_layer_create, section.hip): one more (n, T) type matrix for the section's rows, resident like
// the section's own -- the doubles as the caller gave them and, in a float section, their float copy.  Read-only after its creation; it
// must not outlive its section.  Where a call takes a layer, NULL means the section's own types.
struct same_types_layer {
    same_ctx *ctx = nullptr;
    const same_section *sec = nullptr;
    void *types_c = nullptr;   // [n][T] in the section's cost type
    double *types64 = nullptr; // [n][T] (== types_c for fp64 costs)
};

// A window: the buffers and the pinned block its calls work in, and -- the base -- its logical state (window_state.h: which arrays and
// which list are the window's, what holds, and the table of what each call requires, leaves and invalidates).
struct same_window : win::State {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr, *ref = nullptr;
    int cost_f32 = 0, has_type = 0;
    int64_t cap_m = 0, cap_r = 0;                   // candidates of the covered cells: what the lists are sized for
    int64_t n_m = 0, n_r = 0;
    win::DevBuf stage, filter, finish, tris, big_mask, full_m, full_r;
    win::DevBuf dd_work, dd_tris;                   // the device's triangulation (delaunay_dev.hip): work buffer, candidate triangles
    int64_t n_dd = 0;                               // candidate triangles in dd_tris (dd_ok)
    // stage block (beside the stage view's arrays)
    int32_t *rows_m = nullptr, *rows_r = nullptr, *idx = nullptr, *cnt = nullptr;
    // finish block
    int8_t *sign = nullptr;
    double *weight = nullptr;
    int32_t *match_loc = nullptr;
    int32_t *match_row = nullptr;   // [n_ua] section row of the matched reference cell (-1 = none), flag byte per kept cell: what
    uint8_t *pflag = nullptr;       // same_window_collect reads after the finish call
    void *host = nullptr;     // pinned staging for everything that comes back
    char *host_dev = nullptr; // the same block as the device addresses it (null: not addressable -- copies go through the copy engine)
    size_t host_bytes = 0;
    size_t host_finish_off = 0;   // the pinned block: [stage call's copy | finish call's copy | the filter's counters]
    size_t host_filter_off = 0;
    double box[4] = {0.0, 0.0, 0.0, 0.0};
    // the caller's triangulation (window_caller.hip): the window's triangles before / after the removal, the compacted view, the node
    // mask and the renumbering
    win::DevBuf caller;
    int32_t *sel_tris = nullptr, *caller_out = nullptr;
    win::DevBuf prio;                               // the cell-type-priority prune's list (window_priority.hip)
    unsigned long long bins_m = 0, bins_r = 0;      // the sections' `bins` when the window was staged
    win::DevBuf kpre;                               // the k-NN prefix's list (window_knn_prefix.hip)
};

// what every call that leaves a window staged reports of it: aligned rows and reference rows in the box, kept aligned cells, pairs
namespace win {
inline void report_counts(const same_window *w, int64_t *out) {
    out[0] = w->n_m;
    out[1] = w->n_r;
    out[2] = w->cur.n_ua;
    out[3] = w->cur.list.P;
}
}  // namespace win

// A caller's triangulation of a moving section, resident (same_caller_tris_create): section rows per corner, in the caller's order, and
// the triangles binned by the section's grid cell of their FIRST corner (ascending inside a cell) -- a window reads the cells it covers.
// Read-only after its creation: shared by the worker contexts of its device like a section.  Bound to the grid the section had then.
struct same_caller_tris {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr;
    int64_t n_tris = 0, n_binned = 0;
    int32_t *tris = nullptr;         // [n_tris][3]
    win::BinGrid grid;
    int32_t *order = nullptr;        // [n_binned] triangle numbers by cell
    unsigned *starts = nullptr;      // [cells + 1]
    std::vector<unsigned> h_starts;
};

// The members of a section's rows (same_members_create, window_unpack.hip): CSR over the rows, per member the original cell's XY and its
// joint label code.  Read-only after its creation: shared by the worker contexts of its device like a section; it must not outlive it.
struct same_members {
    same_ctx *ctx = nullptr;
    const same_section *sec = nullptr;
    int64_t n_rows = 0, m = 0;
    int64_t max_count = 0;           // the longest list (host: bounds a solver slice)
    int64_t *off = nullptr;          // [n_rows + 1]
    double *xy = nullptr;            // [m][2]
    int32_t *code = nullptr;         // [m]
};

namespace win {

// The work buffers of the merged rows' reader calls, one of each per accumulator, under the protocol of work_sets.h.
//
// The unpack call's (window_unpack.hip), laid for `rows` final rows.  Idle: the scan's look-back words and the totals of BOTH sets zero;
// unpack_size_kernel clears the other set's.  The offsets are written before they are read.
constexpr int UNPACK_TOTALS = 8;         // words of one set of totals (window_unpack.hip names them)
struct UnpackWork {
    unsigned long long *status[2] = {nullptr, nullptr};   // the scan's look-back words, two sets
    unsigned long long *totals = nullptr;                 // [2][UNPACK_TOTALS]
    unsigned *pair_off = nullptr, *work_off = nullptr;    // [rows] the row's first pair; its solver slice, in units of UNPACK_UNIT words
    size_t status_words = 0, zero_bytes = 0, bytes = 0;   // words of one set; the share that is zero between calls; the whole
};
constexpr int64_t UNPACK_UNIT = 16;      // words of 8 bytes a solver slice is a multiple of: offsets scan in 31 bits, slices start on 128 bytes
inline void lay(UnpackWork &u, Carver &cv, int64_t rows) {
    u.status_words = scan::status_bytes(rows) / 8;
    u.status[0] = cv.scan_words(rows);
    u.status[1] = cv.scan_words(rows);
    u.totals = cv.take<unsigned long long>(2 * UNPACK_TOTALS);
    u.zero_bytes = cv.off;
    u.pair_off = cv.take<unsigned>((size_t)rows);
    u.work_off = cv.take<unsigned>((size_t)rows);
    u.bytes = cv.off;
}

// The score call's (window_score.hip), laid for `rows` rows of the moving section.  Idle: match_of -1, the node counters 0, the totals 0;
// the nodes kernel resets what the two kernels before it wrote, per final row, and score_rows_kernel clears the other set of totals.
constexpr int SCORE_TOTALS = 8;          // words of one set of totals; words [1] and [3 .. 7] are what out_counts[1], [3 .. 7] report
struct ScoreWork {
    int32_t *match_of = nullptr;                  // [rows] reference section row the moving row is matched to in the final rows, -1 = none
    unsigned *node_tri = nullptr, *node_flip = nullptr;   // [rows] triangles not skipped the row is a corner of; the flipped ones of them
    unsigned long long *totals = nullptr;         // [2][SCORE_TOTALS] two sets
    size_t ones_bytes = 0, bytes = 0;             // match_of's share, from the buffer's start (filled 0xFF; the rest 0); the whole
};
inline void lay(ScoreWork &s, Carver &cv, int64_t rows) {
    s.match_of = cv.take<int32_t>((size_t)rows);
    s.ones_bytes = cv.off;
    s.node_tri = cv.take<unsigned>((size_t)rows);
    s.node_flip = cv.take<unsigned>((size_t)rows);
    s.totals = cv.take<unsigned long long>(2 * SCORE_TOTALS);
    s.bytes = cv.off;
}

// The detail call's bins (window_score_detail.hip): two sets of `cap` words.  A set holds what include/same_hip.h states of
// same_merge_acc_score_detail's `out`, in its order -- the confusion matrix, `unlabelled`, the groups' records, the two rank histograms,
// `untyped` -- and one word more, the final rows outside the sections.  Idle: every word of both sets zero; detail_rows_kernel clears
// what the call before counted into the other set (WorkSets::dirty words).
constexpr int DETAIL_GROUP_WORDS = 8;    // words of a group's record, in the order of same_merge_acc_score's out_counts
struct DetailWork {
    unsigned long long *bins = nullptr;           // [2][cap]
    int64_t cap = 0;
    size_t bytes = 0;
};
inline void lay(DetailWork &d, Carver &cv, int64_t cap) {
    d.cap = cap;
    d.bins = cv.take<unsigned long long>((size_t)(2 * cap));
    d.bytes = cv.off;
}
// where a set's parts start for L labels, G groups and R = SAME_SCORE_RANKS: the one statement of the layout, host and device
struct DetailLayout {
    int L = 0, G = 0;
    __host__ __device__ int64_t confusion() const { return 0; }
    __host__ __device__ int64_t unlabelled() const { return (int64_t)L * L; }
    __host__ __device__ int64_t groups() const { return unlabelled() + 1; }
    __host__ __device__ int64_t strict() const { return groups() + (int64_t)(G + 1) * DETAIL_GROUP_WORDS; }
    __host__ __device__ int64_t weak() const { return strict() + SAME_SCORE_RANKS + 1; }
    __host__ __device__ int64_t untyped() const { return weak() + SAME_SCORE_RANKS + 1; }
    __host__ __device__ int64_t out_words() const { return untyped() + 1; }       // what the caller's `out` holds
    __host__ __device__ int64_t bad() const { return out_words(); }               // final rows outside the sections
    __host__ __device__ int64_t words() const { return out_words() + 1; }
};

}  // namespace win

// What same_merge_acc_score_detail bins by, resident (same_score_detail_create, window_score_detail.hip): per row of the moving section
// its group, per label code the commonCT column the label names.  Read-only after its creation: shared by the worker contexts of its
// device like a same_caller_tris; it must not outlive its section.
struct same_score_detail {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr;
    int n_groups = 1, n_labels = 0;
    int32_t *group_of = nullptr;     // [mov->n] in [0, n_groups), negative: no group; null: every row in group 0
    int32_t *col_of_label = nullptr; // [n_labels] in [-1, mov->T); null: no label names a column
};

// What same_merge_acc_unpack_detail bins cell pairs by, resident (same_unpack_detail_create, window_unpack_detail.hip): per cell-level
// label code the type column the label names, per reference member its type row.  Read-only after its creation: shared by the worker
// contexts of its device like its members; it must not outlive them.
struct same_unpack_detail {
    same_ctx *ctx = nullptr;
    const same_members *ref = nullptr;
    int n_labels = 0, T = 0;
    int32_t *col_of_label = nullptr; // [n_labels] in [-1, T); null: no label names a column
    double *types = nullptr;         // [ref->m][T] in CSR order; null: no type rows
};

// What same_merge_acc_score_map keeps beside the counts, resident (same_score_map_create, window_score_map.hip): per row of the moving
// section its truth row and -- with a tally -- four counters over the results folded in so far; and what a map call works in that is not
// the accumulator's: per calling context a slot of two sets of totals (the score call's eight words and the two truth totals, under the
// protocol of work_sets.h) and the device buffer the marks are written to before their copy.  The truth rows are read-only and the tally
// is only added to, so the worker contexts of the device share a map; a slot belongs to ONE context, which one thread uses at a time.
namespace win {
constexpr int MAP_TOTALS = 10;           // words of one set: [0 .. 7] the score call's set, [8] matched rows with a known truth, [9] those on it
constexpr int MAP_SLOTS = 32;            // calling contexts a map serves
struct MapSlot {
    const same_ctx *owner = nullptr;
    WorkSets sets;                       // laid: 1 while both sets are idle
    DevBuf marks;                        // [mov->n] same_cell_mark
};
}  // namespace win
struct same_score_map {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr, *ref = nullptr;
    int32_t *truth_row = nullptr;        // [mov->n] reference section row, -1 unknown; null: every row unknown
    unsigned *tally = nullptr;           // [mov->n][4] matched_in, type_match_in, violating_in, on_truth_in; null: no tally
    unsigned long long *totals = nullptr;   // [MAP_SLOTS][2][MAP_TOTALS]
    int64_t results = 0;                 // map calls folded into the tally since the last reset (under `lock`)
    std::mutex lock;                     // guards `slots`' owners and `results`; never held across device work
    win::MapSlot slots[win::MAP_SLOTS];
};

// What same_merge_acc_unpack_map keeps beside the counts, resident (same_unpack_map_create, window_unpack_map.hip): per moving MEMBER its
// truth member (on the device and, for the marks of a result without a pair, on the host) and -- with a tally -- three counters over the
// results folded in so far; and what a call works in that is not the accumulator's: per calling context a slot of pair_of (the member's
// pair, idle -1), two sets of the two truth totals (work_sets.h), the device buffer of the marks and the page-locked block they are copied
// into.  Shared by the worker contexts of the device as same_score_map is; a slot belongs to ONE context.
namespace win {
constexpr int UNPACK_MAP_TOTALS = 2;     // words of one set: matched members with a known truth, those on it
struct UnpackMapSlot {
    const same_ctx *owner = nullptr;
    WorkSets sets;                       // laid: the members pair_of is laid for while it is idle and both sets are zero
    DevBuf pair_of;                      // [mov->m] int32
    DevBuf marks;                        // [mov->m] same_member_mark
    void *host_marks = nullptr;          // page-locked, [mov->m] same_member_mark: where the marks' copy lands
    size_t host_bytes = 0;
};
}  // namespace win
struct same_unpack_map {
    same_ctx *ctx = nullptr;
    const same_members *mov = nullptr, *ref = nullptr;
    int32_t *truth = nullptr;            // [mov->m] flat reference member, -1 unknown; null: every member unknown
    std::vector<int32_t> h_truth;        // the same on the host (empty: every member unknown)
    unsigned *tally = nullptr;           // [mov->m][3] matched_in, type_match_in, on_truth_in; null: no tally
    unsigned long long *totals = nullptr;   // [MAP_SLOTS][2][UNPACK_MAP_TOTALS]
    int64_t results = 0;                 // calls folded in since the last reset (under `lock`)
    std::mutex lock;                     // guards `slots`' owners and `results`; never held across device work
    win::UnpackMapSlot slots[win::MAP_SLOTS];
};

// The rows of one pass over a window plan on one context (window_merge.hip), and what window_score.hip reads of them.
struct same_merge_acc {
    same_ctx *ctx = nullptr;
    // the rows (struct of arrays, capacity `cap`); `dcount[0]` rows so far (device), then the collect call's scratch words
    int64_t cap = 0;
    int32_t *a_row = nullptr, *r_row = nullptr, *wid = nullptr, *pos = nullptr, *cidx = nullptr;
    uint8_t *flags = nullptr;
    unsigned long long *dcount = nullptr;     // [0] rows, [1] pad, [2 .. 2 + SAME_LAUNCH_WINDOWS) per-window counts of the group in flight
    int64_t bound = 0;                        // host: the rows collected since begin cannot exceed this (sum of the windows' kept cells)
    // the seams of this rank's share of the plan (same_merge_acc_begin)
    win::DevBuf near_start, near_boxes, scan_words;   // scan_words: the collect call's look-back words, one run per window of a group
    int n_pos = 0, all_seam = 0;
    double reach = 0.0;
    // resolve / finish
    win::DevBuf work, out;                    // out: the rest list, then (after finish / plain) the FinalRecs, n_final of them
    int32_t *ac = nullptr, *rc = nullptr, *row_of = nullptr;
    unsigned long long *counters = nullptr;   // in `work`: [0] survivors of the de-duplication, [1] rest rows, [2] final rows
    int64_t n_codes_a = 0;
    int64_t n_rows = 0, n_kept = 0, n_rest = 0, n_final = 0;
    int resolved = 0;
    int final_on_host = 0;                    // the final records have been copied to `host` (same_merge_acc_fetch does it on demand)
    int merged = 0;                           // the final rows are a merge's (same_merge_acc_finish): at most one per moving row
    int loaded = 0;                           // the rows came from the host (same_merge_acc_load): their "section rows" ARE the codes
    int64_t loaded_codes_a = 0, loaded_codes_r = 0;
    std::vector<char> host;                   // what the last resolve / finish brought back (fetched by same_merge_acc_fetch)
    // same_merge_acc_score (window_score.hip)
    win::DevBuf score;
    win::ScoreWork sw;                        // laid over `score`
    win::WorkSets score_sets;                 // ... for so many rows of the moving section
    // same_merge_acc_score_detail (window_score_detail.hip): it works in `sw` too (never in its totals: score_sets does not flip)
    win::DevBuf detail;
    win::DetailWork dw;                       // laid over `detail`
    win::WorkSets detail_sets;                // ... for so many words a set
    // same_merge_acc_unpack (window_unpack.hip)
    const same_section *pass_mov = nullptr, *pass_ref = nullptr;   // the sections the pass ran over (same_merge_acc_resolve; null: loaded rows)
    win::DevBuf unpack, unpack_slices, unpack_pairs;   // the work buffer; the solver's slices (bounded); the pairs' reference members
    win::UnpackWork uw;                       // laid over `unpack`
    win::WorkSets unpack_sets;                // ... for so many final rows; a set: look-back words and totals
    // same_merge_acc_unpack_detail (window_unpack_detail.hip): it runs same_merge_acc_unpack's phases in `uw`, and bins the pairs in
    win::DevBuf unpack_bins;                  // (released by same_merge_acc_destroy with the buffers above: a DevBuf added here joins its list)
    win::DetailWork ubw;                      // laid over `unpack_bins`: two sets of so many words
    win::WorkSets unpack_bin_sets;            // ... for so many words a set
    // same_merge_acc_score_features (window_score_feature.hip): the sums, and what a call with a zone works in (that file lays it)
    win::DevBuf feature, zone;
    win::DetailWork fw;                       // laid over `feature`: two sets of so many words
    win::WorkSets feature_sets;               // ... for so many words a set
    win::WorkSets zone_sets;                  // `zone`: for so many final rows and moving rows; a set: look-back words and totals
    // same_merge_acc_unpack_features (window_unpack_feature.hip): it runs same_merge_acc_unpack's phases in `uw`; its sums and zone work
    win::DevBuf unpack_feature, unpack_zone;
    win::DetailWork ufw;                      // laid over `unpack_feature`: two sets of so many words
    win::WorkSets unpack_feature_sets;        // ... for so many words a set
    win::WorkSets unpack_zone_sets;           // `unpack_zone`: for so many pairs; a set: look-back words and totals
};

namespace win {
// the accumulator holds a merge's final rows on the device: what the three reader calls require of it
inline bool has_merged_rows(const same_merge_acc *a) { return a->resolved == 2 && a->merged && !a->loaded; }
// what the score call and the detail call require alike (refusals come before any device call)
inline int require_score_args(same_ctx *ctx, const same_merge_acc *a, const same_section *mov, const same_section *ref,
                              const same_caller_tris *tris, double majority_threshold) {
    REQUIRE(ctx, has_merged_rows(a));
    REQUIRE(ctx, mov && ref && mov->ctx->device == ctx->device && ref->ctx->device == ctx->device);
    REQUIRE(ctx, mov->label_codes && ref->label_codes);
    REQUIRE(ctx, !tris || (tris->mov == mov && tris->ctx->device == ctx->device));
    REQUIRE(ctx, majority_threshold == majority_threshold);
    return SAME_OK;
}
// ... and both begin with: the accumulator's ScoreWork laid for at least `rows` rows of the moving section, two fills where it is laid
inline int ensure_score_work(same_ctx *ctx, same_merge_acc *a, int64_t rows) {
    if (a->score_sets.fits(rows)) return SAME_OK;
    InDoubt laying(a->score_sets);
    SAME_TRY(lay_over(ctx, a->score, a->sw, rows));
    SAME_FILL(ctx, a->score.p, 0xFF, a->sw.ones_bytes);
    SAME_FILL(ctx, static_cast<char *>(a->score.p) + a->sw.ones_bytes, 0, a->sw.bytes - a->sw.ones_bytes);
    a->score_sets.laid_anew(rows);
    return SAME_OK;
}
}  // namespace win

// what comes back: one record per row (include/same_hip.h)
struct RestRec {
    int32_t row, ac, rc, wid, pos, cidx;
    uint32_t flags;               // bit 0 XY-order flag, bit 1 area-flip flag, bit 2 the row is at a seam
};
struct FinalRec {
    int32_t a_row, r_row, cidx, wid, pos;
    uint32_t flags;
};
static_assert(sizeof(RestRec) == SAME_MERGE_REST_BYTES && sizeof(FinalRec) == SAME_MERGE_FINAL_BYTES, "record layouts are part of the ABI");

namespace win {

// ---- check_triangle_violations' rule (src/eval_utils.py:66-223) over a merge's final rows, as the device states it ---------------------
// Each decision of it ONCE, for the kernels of window_score.hip, window_score_detail.hip and window_unpack.hip; how a kernel adds up what
// these answer (ballots, LDS bins) stays its own.  (match.hip's tri_flip_stats_kernel serves the host-buffer call: another matched mask,
// another same-type test.)
__device__ __forceinline__ bool row_in(int32_t row, int64_t n) { return (unsigned long long)(long long)row < (unsigned long long)n; }
// a final row is FOLLOWED where both its rows lie inside their sections (rows of other sections: counted, never followed)
__device__ __forceinline__ bool followed(const FinalRec &row, int64_t n_mov, int64_t n_ref) {
    return row_in(row.a_row, n_mov) && row_in(row.r_row, n_ref);
}
// do two joint label codes agree: a negative code equals nothing
__device__ __forceinline__ bool labels_agree(int32_t a, int32_t b) { return a >= 0 && a == b; }

// the bin of a moving row under `group_of` over G groups (null: every row in group 0): its group, or G -- the bin of the rows without one
__device__ __forceinline__ int group_at(const int32_t *__restrict__ group_of, int64_t row, int G) {
    const int32_t g = group_of ? group_of[row] : 0;
    return g >= 0 && g < G ? g : G;               // (create refused g >= G)
}
// the row of the CSR `off` (n_rows + 1 offsets) that owns member i: the last row whose list starts at or before i and ends behind it
__device__ __forceinline__ int64_t row_of_member(const int64_t *__restrict__ off, int64_t n_rows, int64_t i) {
    int64_t lo = 0, hi = n_rows;                  // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// the rank of type column c in a reference type row of T float64 columns: with v = row[c], how many OTHER columns hold a value > v
// (strict) and how many one >= v (weak) -> whether the row ranks at all: a NaN anywhere in it ranks nothing
__device__ __forceinline__ bool type_rank(const double *__restrict__ row, int T, int c, int &strict, int &weak) {
    const double v = row[c];
    strict = weak = 0;
    bool nan = v != v;
    for (int t = 0; t < T; ++t) {
        const double x = row[t];
        nan |= x != x;
        if (t != c) {
            strict += x > v ? 1 : 0;
            weak += x >= v ? 1 : 0;
        }
    }
    return !nan;
}

// a resident triangle (a, b, c: rows of the moving section): all three corners matched?  then, under ignore_same, the same-type rule on
// the moving codes, and the flip rule on the moving XY and the matched reference XY (devmath.h: eval_area3, eval_flipped).  A triangle
// that is not all matched loads neither codes nor XY.  (Filled in place: returned by value the three flags travel packed, in VGPRs.)
struct TriVerdict {
    bool all = false, same = false, flipped = false;
};
__device__ __forceinline__ void tri_verdict(TriVerdict &v, int32_t a, int32_t b, int32_t c, const int32_t *match_of, const int32_t *code_m,
                                            int ignore_same, const double *mov_xy, const double *ref_xy) {
    using namespace devmath;
    const int32_t ma = match_of[a], mb = match_of[b], mc = match_of[c];
    v.all = ma >= 0 && mb >= 0 && mc >= 0;
    if (!v.all) return;
    if (ignore_same) {
        const int32_t ca = code_m[a];
        v.same = labels_agree(ca, code_m[b]) && labels_agree(ca, code_m[c]);
    }
    v.flipped = eval_flipped(eval_area3(ld2(mov_xy, a), ld2(mov_xy, b), ld2(mov_xy, c)),
                             eval_area3(ld2(ref_xy, ma), ld2(ref_xy, mb), ld2(ref_xy, mc)));
}
// the corners' counters of a triangle that is not skipped
__device__ __forceinline__ void count_corners(int32_t a, int32_t b, int32_t c, bool flipped, unsigned *node_tri, unsigned *node_flip) {
    atomicAdd(&node_tri[a], 1u); atomicAdd(&node_tri[b], 1u); atomicAdd(&node_tri[c], 1u);
    if (flipped) { atomicAdd(&node_flip[a], 1u); atomicAdd(&node_flip[b], 1u); atomicAdd(&node_flip[c], 1u); }
}
// src/eval_utils.py:199-211: any flip, or at least min_flips flips that are at least the threshold's share of the node's triangles
__device__ __forceinline__ bool node_violating(unsigned n_tri, unsigned n_flip, int node_local, double majority_threshold, int64_t min_flips) {
    return node_local ? (n_tri > 0 && (int64_t)n_flip >= min_flips && (double)n_flip / (double)n_tri >= majority_threshold) : n_flip > 0;
}
// moving row a's three words back to idle: a merge's final rows name a moving row once, nobody else reads or resets them
__device__ __forceinline__ void reset_idle(int32_t a, int32_t *match_of, unsigned *node_tri, unsigned *node_flip) {
    match_of[a] = -1;
    node_tri[a] = 0u;
    node_flip[a] = 0u;
}

// words of a set of score totals (SCORE_TOTALS of them) -- in a namespace of their own, which window_score.hip and window_score_map.hip
// open: window_unpack.hip names the words of ITS totals T_... too, and win::unpack_run would read these in their place
namespace score_totals {
enum { T_BAD = 0, T_TYPE = 1, T_ALL = 3, T_SAME = 4, T_FLIP = 5, T_FLIP_CONSIDERED = 6, T_NODES = 7 };
}
constexpr int SCORE_NT = 256;            // threads of a block of the score kernels
// how many threads of the block hold flag[k] -> totals[word[k]].  Every thread of the block calls it (wave64: four ballots' counts meet
// in LDS), thread k adds total k -- one atomic per block and total, none where the block counted nothing.
template <int K>
__device__ __forceinline__ void block_totals(const bool (&flag)[K], const int (&word)[K], unsigned long long *__restrict__ totals) {
    __shared__ unsigned part[K][SCORE_NT / 64];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long bal = __ballot(flag[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = (unsigned)__builtin_popcountll(bal);
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned n = 0;
        for (int q = 0; q < SCORE_NT / 64; ++q) n += part[threadIdx.x][q];
        if (n) atomicAdd(&totals[word[threadIdx.x]], (unsigned long long)n);
    }
}
// window_score.hip: the rows and triangles phases of same_merge_acc_score, once, for the calls that score -- enqueued into the
// accumulator's ScoreWork (laid by the caller), counting into `totals` and clearing SCORE_TOTALS words of `next`.  match_of is written
// where there is a triangle or `keep_match` says a later kernel reads it; the caller's last kernel returns the rows' words to idle.
int score_phases(same_ctx *ctx, same_merge_acc *a, const same_section *mov, const same_section *ref, const same_caller_tris *tris,
                 int ignore_same_type, bool keep_match, unsigned long long *totals, unsigned long long *next);

// window_unpack.hip: the phases of same_merge_acc_unpack, once, for the calls that unpack -- sizes and their scan, the wait for them,
// the solve launches, the call's last wait.  A PairReader rides between the last solve launch and that wait: the pairs then stay on the
// device (reference member int64 and flat moving member int32 per pair, -1 for the pairs of an infeasible row) and nothing of them is
// copied to the host.
struct DevicePairs {
    const int64_t *ref_member = nullptr;     // [pairs] flat index into the reference members' CSR, -1: the row was infeasible
    const int32_t *mov_member = nullptr;     // [pairs] flat index into the moving members' CSR, -1 likewise
    int64_t pairs = 0;
};
struct PairReader {
    WorkSets *sets = nullptr;                // the protocol of the reader's own buffer: in doubt whenever the unpack buffer is
    int64_t counted = 0;                     // words of its set the reader's kernel counted into (enqueue says): the flip's argument
    virtual int lay(same_ctx *ctx) = 0;                               // before the first enqueue: its buffer laid (and filled, if anew)
    virtual int enqueue(same_ctx *ctx, const DevicePairs &p) = 0;     // its launch and its copy back, behind the last solve launch
    virtual ~PairReader() = default;
};
int unpack_run(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy, int64_t *out_counts,
               int64_t *out_ref_member, int64_t capacity, PairReader *reader);

// section.hip
int knn_index_for(same_ctx *ctx, const same_section *ref, double radius, std::shared_ptr<same_knn_index> *out);
Cover cover_of(const same_section *s, const double *box);
// window_stage.hip
int launch_copy_back(same_ctx *ctx, const CopyArgs *regions, int n_w);
int launch_rows(same_ctx *ctx, const RowsArgs *jobs, int n_w);
int launch_zero(same_ctx *ctx, const ZeroArgs *regions, int n_w);
int check_batch(same_window *const *windows, int n_windows, same_ctx **out_ctx);

// ---- the batch driver of the calls that work on staged windows (window_stage.hip) ------------------------------------------------------
// A batch call prepares a plan per window (no launch), lists the windows that have work (`live`, indices into the batch), walks them in
// groups of SAME_LAUNCH_WINDOWS -- per group its launches, then what each window hands back --, and waits ONCE.  A batch that fails
// counts for nothing: fail_batch.
struct Back {                // what one window hands back into the HEAD of its pinned block
    same_window *w;
    const void *src;
    size_t bytes;
};
// a group's hand-backs enqueued: one launch_copy_back for the group, or -- for a window whose pinned block the device cannot address,
// and for every window with `engine` -- one hipMemcpyAsync each (counted).  `what` names the call in the failure's text.
int copy_back_group(same_ctx *ctx, const Back *back, int n_w, const char *what, bool engine = false);
// what was enqueued is waited for; the listed windows of the batch are no longer staged (count blocks and pinned blocks of earlier groups
// are overwritten already); -> rc
int fail_batch(same_ctx *ctx, same_window *const *windows, const std::vector<int> &touched, int rc);
// fn(plans of the group, their indices into the batch, how many) for every group of `live`, until one fails
template <class Plan, class F>
int for_each_group(std::vector<Plan> &plans, const std::vector<int> &live, F &&fn) {
    int rc = SAME_OK;
    for (size_t g = 0; g < live.size() && rc == SAME_OK; g += SAME_LAUNCH_WINDOWS) {
        const int n_g = (int)std::min<size_t>(SAME_LAUNCH_WINDOWS, live.size() - g);
        Plan *pps[SAME_LAUNCH_WINDOWS];
        for (int q = 0; q < n_g; ++q) pps[q] = &plans[(size_t)live[g + (size_t)q]];
        rc = fn(pps, live.data() + g, n_g);
    }
    return rc;
}

// The two calls that leave windows "as a stage call at k leaves them" without staging them (k-NN prefix, recost) are this one batch:
// every window's compaction by a caller's triangulation turned back and held; plan(w, &plan, &live) says whether the window needs a
// launch and plans it; launch(plans, n) enqueues a group's kernels; every live window's count block -- a window turned back: the staged
// counts, XY and rows, its pinned block holds the compacted ones -- goes into the head of its pinned block with the group's launch, a
// window only turned back gets its by the copy engine; ONE wait, and only if anything was enqueued; derived(w, plan, &list) then checks
// the counts that came back for a live window and names the list its kernels wrote (P: count word 3).  Every window ends staged_at k
// (0: its own staged k) with that list, or the list as the stage call put it, and reports its four counts.
template <class Plan, class PlanFn, class LaunchFn, class DerivedFn>
int restage_batch(same_ctx *ctx, same_window *const *windows, int n_windows, int k, const char *what, int64_t *out_counts, PlanFn &&plan,
                  LaunchFn &&launch, DerivedFn &&derived) {
    std::vector<Plan> plans((size_t)n_windows);
    std::vector<char> was_turned((size_t)n_windows), is_live((size_t)n_windows, 0);
    for (int i = 0; i < n_windows; ++i) was_turned[(size_t)i] = windows[i]->hold_caller();
    std::vector<int> live, turned;                // turned: turned back, no launch -- only their pinned blocks are to restore
    int rc = SAME_OK;
    for (int i = 0; i < n_windows && rc == SAME_OK; ++i) {
        bool needs = false;
        rc = plan(windows[i], &plans[(size_t)i], &needs);
        if (rc == SAME_OK && needs) live.push_back(i), is_live[(size_t)i] = 1;
    }
    for (int i = 0; i < n_windows; ++i)
        if (!is_live[(size_t)i] && was_turned[(size_t)i]) turned.push_back(i);
    auto hand_back = [&](const int *at, int n_g, bool engine) {
        Back bk[SAME_LAUNCH_WINDOWS];
        for (int q = 0; q < n_g; ++q) {
            same_window *w = windows[at[q]];
            bk[q] = Back{w, w->cur.counts, was_turned[(size_t)at[q]] ? w->held.back_bytes : 64};
        }
        return copy_back_group(ctx, bk, n_g, what, engine);
    };
    if (rc == SAME_OK)
        rc = for_each_group(plans, live, [&](Plan *const *pps, const int *at, int n_g) {
            SAME_TRY(launch(pps, n_g));
            return hand_back(at, n_g, false);
        });
    if (rc == SAME_OK) rc = for_each_group(plans, turned, [&](Plan *const *, const int *at, int n_g) { return hand_back(at, n_g, true); });
    if (rc != SAME_OK) {                          // (a window turned back above: its pinned block may still be the compacted one)
        live.insert(live.end(), turned.begin(), turned.end());
        return fail_batch(ctx, windows, live, rc);
    }
    if (!live.empty() || !turned.empty()) SAME_WAIT(ctx);
    std::vector<PairList> lists((size_t)n_windows);
    for (int i : live) {
        SAME_TRY(derived(windows[i], plans[(size_t)i], &lists[(size_t)i]));
        lists[(size_t)i].P = (int64_t) static_cast<const unsigned long long *>(windows[i]->host)[3];
    }
    for (int i = 0; i < n_windows; ++i) {
        same_window *w = windows[i];
        w->staged_at(k ? k : w->k_staged, is_live[(size_t)i] ? lists[(size_t)i] : w->sk);
        static_cast<unsigned long long *>(w->host)[3] = (unsigned long long)w->cur.list.P;     // the count block's host copy: the list's
        report_counts(w, out_counts + 4 * i);
    }
    return SAME_OK;
}

// The three calls that derive a pair list from a pair list (priority prune, k-NN prefix, caller pairs) plan alike: the kernels' argument
// block -- `n` rows, the source list `src`, the destination `dst` -- and the head of the destination buffer to zero (the scan's words).
template <class A>
struct ListPlan {
    A a{};
    ZeroArgs zero{};
};
struct ListGrid {            // a group's launch shapes: blockIdx.y windows, the largest row count and source list
    unsigned nw = 0;
    int64_t max_n = 0, max_P = 0;
};
// a group's argument blocks by value, its shapes, its zeroing enqueued
template <class A>
int begin_group(same_ctx *ctx, ListPlan<A> *const *pps, int n_w, Batch<A> *b, ListGrid *g) {
    ZeroArgs zr[SAME_LAUNCH_WINDOWS];
    g->nw = (unsigned)n_w;
    for (int q = 0; q < n_w; ++q) {
        b->w[q] = pps[q]->a;
        zr[q] = pps[q]->zero;
        g->max_n = std::max(g->max_n, pps[q]->a.n);
        g->max_P = std::max(g->max_P, pps[q]->a.src.P);
    }
    return launch_zero(ctx, zr, n_w);
}

}  // namespace win
