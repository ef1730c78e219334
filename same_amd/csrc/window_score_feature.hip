// window_score_feature.hip -- a merged result read as FEATURE SUMS: the matched pairs put two feature matrices side by side, and the sums
// of their rows per group of the moving rows and per bin of the distance to a marked zone are what the means of a study are made from.
//
// The reference's notebooks end every study this way (examples/luad/reproduce_figures.ipynb cells 16-22): the PCF rows and the Xenium rows
// of every matched pair gathered into one table, its mean per moving label (the matrixplot), cdist(X_spatial, zone).min(axis=1) per pair,
// pd.cut of that distance, the mean of a marker set per distance bin over a subset of the pairs.  When a set's merge ends the final rows
// and both sections' XY are resident; the feature matrices, the groups and the masks are constant over the study and uploaded once
// (same_score_features, same_feature_zone).  same_merge_acc_score_features reads them where they are:
//
//   feature_sums_kernel   one wave per run of final rows, a tile of 64 feature columns: lane = column, so a pair's share of a feature row is
//                         one coalesced 256-byte read of int32.  A block keeps int64 sums for 64 bins x 64 columns in LDS (32 KB: four
//                         blocks a CU beside their registers), walks its share of a capped grid and flushes one 64-bit integer atomic per
//                         non-zero sum -- a bin's 64 columns as one 512-byte wave instruction.  blockIdx.y = column tile, blockIdx.z = the
//                         chunk of 64 bins the block sums (up to 257 groups: a block skips the rows of other chunks after their 4-byte
//                         group read).  It runs once with the moving row's group as the bin and, with a zone, once more with the distance
//                         bin of the subset pairs.  The columns are fixed point (include/same_hip.h): integer sums are exact, the same
//                         from run to run and under every grid shape, which no float sum would be.
//   zone_flag_kernel      per final row its two flags, the zone pairs' reference XY compacted by scan.h's scan (zone pairs and subset
//                         pairs are the scan's two counters), the rows outside the sections and the flagged pairs with a non-finite XY
//   (grid.h)              knn.hip's build bins the compacted points: bounding box, counts, scan, scatter
//   zone_walk_kernel      one thread per subset pair: rings of cells out from the pair's cell until a lower bound on everything not walked
//                         exceeds the best d2 (align.hip's unwalked_lb2 at k = 1; no "decided" band: a tie does not change a minimum);
//                         then the bin by the edges, marked for the second run of feature_sums_kernel.  A ring is clipped to the grid and
//                         the ring number is bounded by the grid's extent, whatever the coordinates.
//
// A brute-force LDS-tiled minimum was not measured against the grid (the notebook's shape: 91 684 pairs against 20 009 zone points).
// The sums live in the accumulator under the protocol of work_sets.h: two sets of the call's words, the first kernel clears what the call
// before counted into the other; the zone's scan words and totals likewise.  No other buffer of the accumulator is touched.
#include "grid.h"
#include "window_internal.h"

struct same_score_features {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr, *ref = nullptr;
    int F_m = 0, F_r = 0, n_groups = 1;
    int32_t *mov_q = nullptr, *ref_q = nullptr;   // [mov->n][F_m], [ref->n][F_r]
    int32_t *group_of = nullptr;                  // [mov->n] or null: every row in group 0
};

struct same_feature_zone {
    same_ctx *ctx = nullptr;
    const same_score_features *feats = nullptr;
    uint8_t *mov_flags = nullptr, *ref_flags = nullptr;   // null: every bit set
    double *edges = nullptr;                              // [B + 1]
    int B = 0;
};

namespace {

using namespace win;

constexpr int NT = 256, WAVES = NT / 64, TILE = 64, CHUNK = 64, UNROLL = 4;
constexpr int MAX_BLOCKS = 512;          // blocks of a sums launch, tiles and chunks included: the flushes stay few beside the row work
constexpr int32_t Q_MAX = 1 << 30;
enum { Z_ZONE = 0, Z_SUBSET = 1, Z_BAD = 2, Z_NONFINITE = 3, ZONE_TOTALS = 4 };
static_assert(NT == scan::NT && NT == SCORE_NT, "the flag kernel scans and totals with the score kernels' block");

// the words of a set of sums: include/same_hip.h's `out`, then the final rows outside the sections
struct FeatureLayout {
    int G = 1, F = 1, B = 0;
    int64_t rows() const { return 4; }
    int64_t sums() const { return rows() + G + 1; }
    int64_t bin_rows() const { return sums() + (int64_t)(G + 1) * F; }
    int64_t bin_sums() const { return bin_rows() + (B > 0 ? B + 1 : 0); }
    int64_t out_words() const { return bin_sums() + (B > 0 ? (int64_t)(B + 1) * F : 0); }
    int64_t bad() const { return out_words(); }
    int64_t words() const { return out_words() + 1; }
};

// The zone call's work buffer, laid for `rows` >= final rows, moving rows.  Idle: the scan words and the totals of both sets zero; the
// rest is written before it is read.
struct ZoneWork {
    unsigned long long *status[2] = {nullptr, nullptr}, *totals = nullptr;   // two sets: look-back words, [ZONE_TOTALS]
    uint8_t *flag = nullptr;                      // [rows] per final row: bit 0 zone pair, bit 1 subset pair
    int32_t *bin = nullptr;                       // [rows] per final row: the subset pair's distance bin, -1 no subset pair
    double *zxy = nullptr, *d2 = nullptr;         // [rows][2] the zone pairs' XY, compacted; [rows] per MOVING row
    unsigned *start = nullptr, *rank = nullptr;   // the grid of the zone pairs: [2 * rows + 17], [rows]
    double *sxy = nullptr;                        // [rows][2]
    int32_t *sidx = nullptr;                      // [rows]
    size_t status_words = 0, zero_bytes = 0, bytes = 0;
};
void lay(ZoneWork &z, Carver &cv, int64_t rows) {
    z.status_words = scan::status_bytes(rows) / 8;
    z.status[0] = cv.scan_words(rows);
    z.status[1] = cv.scan_words(rows);
    z.totals = cv.take<unsigned long long>(2 * ZONE_TOTALS);
    z.zero_bytes = cv.off;
    z.flag = cv.take<uint8_t>((size_t)rows);
    z.bin = cv.take<int32_t>((size_t)rows);
    z.zxy = cv.take<double>((size_t)rows * 2);
    z.d2 = cv.take<double>((size_t)rows);
    z.start = cv.take<unsigned>((size_t)rows * 2 + 17);
    z.rank = cv.take<unsigned>((size_t)rows);
    z.sxy = cv.take<double>((size_t)rows * 2);
    z.sidx = cv.take<int32_t>((size_t)rows);
    z.bytes = cv.off;
}

// ---- (a) gather and bin -------------------------------------------------------------------------------------------------------------------
// bin of final row i: bin_of[by_final ? i : its moving row] where that is in [0, n_bins), else `rest` (negative: the row is left out);
// bin_of null: bin 0.  cnt[n_bins], sums[n_bins][F]; `bad` (may be null): the final rows outside the sections.
__global__ __launch_bounds__(NT) void feature_sums_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                          const int32_t *__restrict__ bin_of, int by_final, int n_bins, int rest,
                                                          const int32_t *__restrict__ mov_q, int F_m, const int32_t *__restrict__ ref_q,
                                                          int F_r, unsigned long long *__restrict__ cnt,
                                                          unsigned long long *__restrict__ sums, unsigned long long *__restrict__ bad,
                                                          unsigned long long *__restrict__ next, int64_t next_dirty) {
    __shared__ unsigned long long lds_sum[CHUNK][TILE];
    __shared__ unsigned lds_cnt[CHUNK];
    __shared__ unsigned lds_bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int F = F_m + F_r, col = (int)blockIdx.y * TILE + lane, bin0 = (int)blockIdx.z * CHUNK;
    const bool counts_here = blockIdx.y == 0, bad_here = bad && blockIdx.y == 0 && blockIdx.z == 0;
    if (next) {                                   // the set the NEXT call sums into
        const int64_t blocks = (int64_t)gridDim.x * gridDim.y * gridDim.z;
        const int64_t me = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        for (int64_t i = me * NT + threadIdx.x; i < next_dirty; i += blocks * NT) next[i] = 0ull;
    }
    for (int i = threadIdx.x; i < CHUNK * TILE; i += NT) (&lds_sum[0][0])[i] = 0ull;
    if (threadIdx.x < CHUNK) lds_cnt[threadIdx.x] = 0u;
    if (threadIdx.x == 0) lds_bad = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t i0 = (int64_t)blockIdx.x * WAVES + wave; i0 < n; i0 += stride * UNROLL) {
        int local[UNROLL];
        int32_t q[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {        // the loads of UNROLL rows in flight before the first LDS atomic
            const int64_t i = i0 + (int64_t)u * stride;
            local[u] = -1;
            q[u] = 0;
            if (i >= n) continue;
            const FinalRec rec = rows[i];         // (one address per wave: a broadcast)
            if (!followed(rec, n_mov, n_ref)) {
                if (bad_here && lane == 0) atomicAdd(&lds_bad, 1u);
                continue;
            }
            const int32_t g = bin_of ? bin_of[by_final ? i : (int64_t)rec.a_row] : 0;
            const int bin = g >= 0 && g < n_bins ? g : rest;
            if (bin < bin0 || bin >= bin0 + CHUNK) continue;
            local[u] = bin - bin0;
            if (col < F) q[u] = col < F_m ? mov_q[(int64_t)rec.a_row * F_m + col] : ref_q[(int64_t)rec.r_row * F_r + (col - F_m)];
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (local[u] < 0) continue;
            if (q[u]) atomicAdd(&lds_sum[local[u]][lane], (unsigned long long)(long long)q[u]);     // two's complement: the sum wraps to itself
            if (counts_here && lane == 0) atomicAdd(&lds_cnt[local[u]], 1u);
        }
    }
    __syncthreads();
    for (int b = wave; b < CHUNK && bin0 + b < n_bins; b += WAVES) {
        const unsigned long long v = lds_sum[b][lane];
        if (v && col < F) atomicAdd(&sums[(int64_t)(bin0 + b) * F + col], v);
    }
    if (counts_here && threadIdx.x < CHUNK && bin0 + (int)threadIdx.x < n_bins) {
        const unsigned c = lds_cnt[threadIdx.x];
        if (c) atomicAdd(&cnt[bin0 + threadIdx.x], (unsigned long long)c);
    }
    if (bad_here && threadIdx.x == 0 && lds_bad) atomicAdd(bad, (unsigned long long)lds_bad);
}

dim3 sums_grid(int64_t n, int F, int n_bins) {
    const int64_t tiles = ceil_div(F, TILE), chunks = ceil_div(n_bins, CHUNK);
    const int64_t want = ceil_div(n > 0 ? n : 1, WAVES * UNROLL * 4);            // a wave has a few rounds of rows to walk
    const int64_t x = std::max<int64_t>(1, std::min<int64_t>(want, std::max<int64_t>(MAX_BLOCKS / (tiles * chunks), 8)));
    return dim3((unsigned)x, (unsigned)tiles, (unsigned)chunks);
}

// ---- (b) zone -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pair_flags(const FinalRec &rec, const uint8_t *__restrict__ mov_flags, const uint8_t *__restrict__ ref_flags) {
    return (mov_flags ? mov_flags[rec.a_row] : 3u) & (ref_flags ? ref_flags[rec.r_row] : 3u) & 3u;
}

__global__ __launch_bounds__(NT) void zone_flag_kernel(const FinalRec *__restrict__ rows, int64_t n, int64_t n_mov, int64_t n_ref,
                                                       const uint8_t *__restrict__ mov_flags, const uint8_t *__restrict__ ref_flags,
                                                       const double *__restrict__ ref_xy, unsigned long long *status,
                                                       unsigned long long *__restrict__ next_status, int64_t status_words,
                                                       unsigned long long *__restrict__ totals, unsigned long long *__restrict__ next_totals,
                                                       uint8_t *__restrict__ flag, double *__restrict__ zxy, double *__restrict__ d2_mov) {
    __shared__ scan::Shared sh;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x, all = (int64_t)gridDim.x * NT;
    for (int64_t w = i; w < status_words; w += all) next_status[w] = 0ull;          // what the NEXT call scans and totals in
    if (blockIdx.x == 0 && threadIdx.x < ZONE_TOTALS) next_totals[threadIdx.x] = 0ull;
    if (d2_mov)
        for (int64_t m = i; m < n_mov; m += all) d2_mov[m] = __builtin_nan("");     // (the walk kernel, a later launch, writes the subset pairs')
    auto val = [&](int64_t q) {
        if (q >= n) return scan::Pair{0u, 0u};
        const FinalRec rec = rows[q];
        if (!followed(rec, n_mov, n_ref)) return scan::Pair{0u, 0u};
        const unsigned f = pair_flags(rec, mov_flags, ref_flags);
        return scan::Pair{f & 1u, f >> 1};
    };
    scan::Pair through;
    const scan::Pair off = scan::exclusive(status, (int)blockIdx.x, val, sh, &through);
    bool outside = false, nonfinite = false;
    if (i < n) {
        const FinalRec rec = rows[i];
        unsigned f = 0u;
        if (followed(rec, n_mov, n_ref)) {
            f = pair_flags(rec, mov_flags, ref_flags);
            if (f) {
                const double x = ref_xy[2 * (int64_t)rec.r_row], y = ref_xy[2 * (int64_t)rec.r_row + 1];
                nonfinite = !(__builtin_isfinite(x) && __builtin_isfinite(y));
                if (f & 1u) {
                    zxy[2 * (int64_t)off.a] = x;
                    zxy[2 * (int64_t)off.a + 1] = y;
                }
            }
        } else {
            outside = true;
        }
        flag[i] = (uint8_t)f;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        atomicAdd(&totals[Z_ZONE], (unsigned long long)through.a);
        atomicAdd(&totals[Z_SUBSET], (unsigned long long)through.p);
    }
    const bool fl[2] = {outside, nonfinite};
    const int word[2] = {Z_BAD, Z_NONFINITE};
    block_totals<2>(fl, word, totals);
}

// the grid of the zone pairs as the walk reads it (align.hip's AlignGrid)
struct ZoneGrid {
    GridDesc g;
    double cell;     // 1 / g.inv_cell
    double X1, Y1;   // far edges of the grid
    double slack;    // how far a point can lie outside the nominal box of the cell it was binned in
};
// about one zone point per cell, never more than 2 n + 16 cells; one cell for a box without a finite extent
ZoneGrid zone_geometry(const double box[4], int64_t n) {
    const double x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    const double w = x1 - x0, h = y1 - y0, ext = std::max(w, h);
    ZoneGrid z;
    z.g.x0 = x0;
    z.g.y0 = y0;
    double cell = 1.0;
    int64_t gx = 1, gy = 1;
    if (ext > 0.0 && std::isfinite(ext) && std::isfinite(x0) && std::isfinite(y0)) {
        const double area = std::max(w * h, ext * ext / (double)n);   // a set on a line still gets about a point per cell
        cell = std::max(std::sqrt(area / (double)n), ext / 4096.0);
        for (;;) {
            gx = (int64_t)std::floor(w / cell) + 1;
            gy = (int64_t)std::floor(h / cell) + 1;
            if (gx * gy <= 2 * n + 16) break;
            cell *= 1.25;
        }
    }
    z.g.inv_cell = 1.0 / cell;
    z.g.gx = (int)gx;
    z.g.gy = (int)gy;
    z.cell = cell;
    z.X1 = x0 + (double)gx * cell;
    z.Y1 = y0 + (double)gy * cell;
    const double mag = std::max(std::max(std::fabs(x0), std::fabs(y0)), std::max(std::fabs(x1), std::fabs(y1)));
    z.slack = 1e-9 * cell + std::ldexp(mag, -40);
    return z;
}

// squared lower bound on the distance from q to every point binned outside cells [xlo, xhi] x [ylo, yhi] (clipped to the grid): the
// nearest of the slabs of the grid box beyond the block's sides, each widened by the slack (align.hip's unwalked_lb2)
__device__ __forceinline__ double ring_lb2(const ZoneGrid &z, double qx, double qy, int xlo, int xhi, int ylo, int yhi) {
    const double s = z.slack, gx0 = z.g.x0 - s, gy0 = z.g.y0 - s, gx1 = z.X1 + s, gy1 = z.Y1 + s;
    const double ox = fmax(fmax(gx0 - qx, qx - gx1), 0.0), oy = fmax(fmax(gy0 - qy, qy - gy1), 0.0);
    double lb2 = __builtin_inf();
    if (xhi < z.g.gx - 1) {
        const double dx = fmax(fmax(z.g.x0 + (double)(xhi + 1) * z.cell - s - qx, qx - gx1), 0.0);
        lb2 = fmin(lb2, dx * dx + oy * oy);
    }
    if (xlo > 0) {
        const double dx = fmax(fmax(qx - (z.g.x0 + (double)xlo * z.cell + s), gx0 - qx), 0.0);
        lb2 = fmin(lb2, dx * dx + oy * oy);
    }
    if (yhi < z.g.gy - 1) {
        const double dy = fmax(fmax(z.g.y0 + (double)(yhi + 1) * z.cell - s - qy, qy - gy1), 0.0);
        lb2 = fmin(lb2, ox * ox + dy * dy);
    }
    if (ylo > 0) {
        const double dy = fmax(fmax(qy - (z.g.y0 + (double)ylo * z.cell + s), gy0 - qy), 0.0);
        lb2 = fmin(lb2, ox * ox + dy * dy);
    }
    return lb2;
}
// a query's cell: cell_coord, with a NaN in cell 0
__device__ __forceinline__ int query_cell(double v, double v0, double inv_cell, int g) {
    const double c = __builtin_floor((v - v0) * inv_cell);
    return c >= 0.0 ? (c >= (double)g ? g - 1 : (int)c) : 0;
}

// min over the n_zone binned points of dx*dx + dy*dy (fp64, no contraction: the file's -ffp-contract=off); NaN with no point
__device__ __forceinline__ double nearest_d2(const double *__restrict__ sxy, const unsigned *__restrict__ start, const ZoneGrid &z,
                                             int64_t n_zone, double qx, double qy) {
    if (n_zone <= 0) return __builtin_nan("");
    const GridDesc &g = z.g;
    const int cx = query_cell(qx, g.x0, g.inv_cell, g.gx), cy = query_cell(qy, g.y0, g.inv_cell, g.gy);
    const int last = max(g.gx, g.gy);             // ring `last` covers the grid from any cell: the walk ends there at the latest
    double best = __builtin_inf();
    for (int r = 0; r <= last; ++r) {
        const int xlo = max(cx - r, 0), xhi = min(cx + r, g.gx - 1), ylo = max(cy - r, 0), yhi = min(cy + r, g.gy - 1);
        for (int yy = ylo; yy <= yhi; ++yy) {
            const int64_t rowc = (int64_t)yy * g.gx;
            const bool edge = yy == cy - r || yy == cy + r;
            // a ring row is the whole clipped run on the ring's top and bottom, its two end cells between them
            for (int side = 0; side < 2; ++side) {
                int c0, c1;
                if (edge) {
                    if (side) break;
                    c0 = xlo;
                    c1 = xhi;
                } else {
                    c0 = c1 = side ? cx + r : cx - r;
                    if (c0 < 0 || c0 > g.gx - 1) continue;
                }
                const unsigned b = start[rowc + c0], e = start[rowc + c1 + 1];
                for (unsigned p = b; p < e; ++p) {
                    const double dx = sxy[2 * (int64_t)p] - qx, dy = sxy[2 * (int64_t)p + 1] - qy;
                    const double d2 = dx * dx + dy * dy;
                    best = d2 < best ? d2 : best;
                }
            }
        }
        if (xlo == 0 && ylo == 0 && xhi == g.gx - 1 && yhi == g.gy - 1) break;
        if (best < __builtin_inf() && ring_lb2(z, qx, qy, xlo, xhi, ylo, yhi) * (1.0 - 1e-13) > best) break;
    }
    return best < __builtin_inf() ? best : __builtin_nan("");
}

// one thread per final row: a subset pair's d2 and bin; -1 for every other row
__global__ __launch_bounds__(NT) void zone_walk_kernel(const FinalRec *__restrict__ rows, int64_t n, const uint8_t *__restrict__ flag,
                                                       const double *__restrict__ ref_xy, int64_t n_zone, const double *__restrict__ sxy, const unsigned *__restrict__ start, ZoneGrid z,
                                                       const double *__restrict__ edges, int B, int32_t *__restrict__ bin_of,
                                                       double *__restrict__ d2_mov) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const unsigned f = flag[i];
    if (!(f & 2u)) {
        bin_of[i] = -1;
        return;
    }
    const FinalRec rec = rows[i];                 // (flagged: inside the sections)
    const double d2 = (f & 1u) ? 0.0
                               : nearest_d2(sxy, start, z, n_zone, ref_xy[2 * (int64_t)rec.r_row], ref_xy[2 * (int64_t)rec.r_row + 1]);
    int bin = B;                                  // NaN, and a d2 outside (edges[0], edges[B]]: no bin
    for (int b = 0; b < B; ++b)
        if (d2 > edges[b] && d2 <= edges[b + 1]) {
            bin = b;
            break;
        }
    bin_of[i] = bin;
    if (d2_mov) d2_mov[rec.a_row] = d2;
}

template <class T>
int upload(same_ctx *ctx, T **dst, const T *src, size_t count) {
    if (!src || !count) return SAME_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(dst), count * sizeof(T)));
    HIP_TRY(ctx, hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return SAME_OK;
}

}  // namespace

extern "C" {

int same_score_features_create(const same_section *mov, const same_section *ref, const int32_t *mov_q, int F_m, const int32_t *ref_q, int F_r,
                               const int32_t *group_of, int n_groups, same_score_features **out) {
    if (!mov || !out) return SAME_EINVAL;
    same_ctx *ctx = mov->ctx;
    *out = nullptr;
    REQUIRE(ctx, ref && ref->ctx->device == ctx->device);
    REQUIRE(ctx, F_m >= 0 && F_r >= 0 && (int64_t)F_m + F_r >= 1 && (int64_t)F_m + F_r <= SAME_FEATURE_MAX_COLUMNS);
    REQUIRE(ctx, n_groups >= 1 && n_groups <= SAME_SCORE_MAX_GROUPS);
    REQUIRE(ctx, (mov_q || !F_m || !mov->n) && (ref_q || !F_r || !ref->n));
    const struct { const int32_t *q; int64_t count; } sides[2] = {{mov_q, mov->n * F_m}, {ref_q, ref->n * F_r}};
    for (const auto &s : sides)
        for (int64_t i = 0; i < s.count; ++i)
            if (s.q[i] > Q_MAX || s.q[i] < -Q_MAX) {
                ctx->err = "same_score_features_create: a quantised value is beyond 2^30 in magnitude";
                return SAME_ERANGE;
            }
    if (group_of)
        for (int64_t i = 0; i < mov->n; ++i)
            if (group_of[i] >= n_groups) {
                ctx->err = "same_score_features_create: a group_of value is not below n_groups";
                return SAME_ERANGE;
            }
    SAME_TRY(same_use(ctx));
    same_score_features *f = new (std::nothrow) same_score_features();
    if (!f) return SAME_ENOMEM;
    f->ctx = ctx;
    f->mov = mov;
    f->ref = ref;
    f->F_m = F_m;
    f->F_r = F_r;
    f->n_groups = n_groups;
    *out = f;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &f->mov_q, mov_q, (size_t)(mov->n * F_m)));
    SAME_TRY(upload(ctx, &f->ref_q, ref_q, (size_t)(ref->n * F_r)));
    SAME_TRY(upload(ctx, &f->group_of, group_of, (size_t)mov->n));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_score_features_destroy(same_score_features *f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (f->mov_q) (void)hipFree(f->mov_q);
    if (f->ref_q) (void)hipFree(f->ref_q);
    if (f->group_of) (void)hipFree(f->group_of);
    delete f;
}

int same_feature_zone_create(const same_score_features *feats, const uint8_t *mov_flags, const uint8_t *ref_flags, const double *d2_edges,
                             int n_edges, same_feature_zone **out) {
    if (!feats || !out) return SAME_EINVAL;
    same_ctx *ctx = feats->ctx;
    *out = nullptr;
    REQUIRE(ctx, d2_edges && n_edges >= 2 && n_edges <= SAME_FEATURE_MAX_EDGES);
    for (int q = 0; q < n_edges; ++q) REQUIRE(ctx, d2_edges[q] == d2_edges[q] && (q == 0 || d2_edges[q] >= d2_edges[q - 1]));
    SAME_TRY(same_use(ctx));
    same_feature_zone *z = new (std::nothrow) same_feature_zone();
    if (!z) return SAME_ENOMEM;
    z->ctx = ctx;
    z->feats = feats;
    z->B = n_edges - 1;
    *out = z;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &z->mov_flags, mov_flags, (size_t)feats->mov->n));
    SAME_TRY(upload(ctx, &z->ref_flags, ref_flags, (size_t)feats->ref->n));
    SAME_TRY(upload(ctx, &z->edges, d2_edges, (size_t)n_edges));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_feature_zone_destroy(same_feature_zone *z) {
    if (!z) return;
    (void)hipSetDevice(z->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (z->mov_flags) (void)hipFree(z->mov_flags);
    if (z->ref_flags) (void)hipFree(z->ref_flags);
    if (z->edges) (void)hipFree(z->edges);
    delete z;
}

int same_merge_acc_score_features(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_score_features *feats,
                                  const same_feature_zone *zone, int64_t *out, int64_t out_words, double *out_d2) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out);
    SAME_TRY(require_score_args(ctx, a, mov, ref, nullptr, 0.0));
    REQUIRE(ctx, feats && feats->mov == mov && feats->ref == ref && feats->ctx->device == ctx->device);
    REQUIRE(ctx, !zone || zone->feats == feats);
    FeatureLayout lo;
    lo.G = feats->n_groups;
    lo.F = feats->F_m + feats->F_r;
    lo.B = zone ? zone->B : 0;
    REQUIRE(ctx, out_words >= lo.out_words());
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, words = lo.words();
    const int G = lo.G, F = lo.F, B = lo.B;
    std::vector<unsigned long long> h((size_t)words, 0ull);
    unsigned long long zt[ZONE_TOTALS] = {};
    bool d2_copied = false;
    if (n > 0) {
        WorkSets &fs = a->feature_sets;
        if (!fs.fits(words)) {
            InDoubt laying(fs);
            SAME_TRY(lay_over(ctx, a->feature, a->fw, words));
            SAME_FILL(ctx, a->feature.p, 0, a->fw.bytes);
            fs.laid_anew(words);
        }
        const int64_t z_rows = std::max<int64_t>(std::max(n, mov->n), 1);
        ZoneWork zw;
        if (zone) {
            WorkSets &zs = a->zone_sets;
            if (!zs.fits(z_rows)) {
                InDoubt laying(zs);
                SAME_TRY(lay_over(ctx, a->zone, zw, z_rows));
                SAME_FILL(ctx, a->zone.p, 0, zw.zero_bytes);
                zs.laid_anew(z_rows);
            }
            Carver place(a->zone.p);
            lay(zw, place, a->zone_sets.laid);
        }
        InDoubt doubt(fs), doubt_zone(a->zone_sets);          // (the zone's: in doubt only where the call works in it)
        if (!zone) doubt_zone.sound();
        unsigned long long *bins = a->fw.bins + (size_t)fs.set * a->fw.cap, *next = a->fw.bins + (size_t)(fs.set ^ 1) * a->fw.cap;
        const FinalRec *fin = static_cast<const FinalRec *>(a->out.p);
        SAME_LAUNCH(ctx, feature_sums_kernel, sums_grid(n, F, G + 1), dim3(NT), 0, fin, n, mov->n, ref->n, feats->group_of, 0, G + 1, G,
                    feats->mov_q, feats->F_m, feats->ref_q, feats->F_r, bins + lo.rows(), bins + lo.sums(), bins + lo.bad(), next, fs.dirty);
        if (zone) {
            const int zset = a->zone_sets.set;
            unsigned long long *totals = zw.totals + (size_t)zset * ZONE_TOTALS, *next_totals = zw.totals + (size_t)(zset ^ 1) * ZONE_TOTALS;
            SAME_LAUNCH(ctx, zone_flag_kernel, dim3(scan::blocks_for(n)), dim3(NT), 0, fin, n, mov->n, ref->n, zone->mov_flags, zone->ref_flags,
                        ref->xy, scan::arg(zw.status[zset]), zw.status[zset ^ 1], (int64_t)zw.status_words, totals, next_totals, zw.flag, zw.zxy,
                        out_d2 ? zw.d2 : nullptr);
            HIP_TRY(ctx, hipGetLastError());
            SAME_COPY(ctx, zt, totals, sizeof zt, hipMemcpyDeviceToHost);
            SAME_WAIT(ctx);
            if (zt[Z_BAD] || zt[Z_NONFINITE]) {   // (both buffers stay in doubt: the next call lays them again)
                ctx->err = zt[Z_BAD] ? "same_merge_acc_score_features: final rows outside the sections (the accumulator's pass ran over other sections)"
                                     : "same_merge_acc_score_features: a zone or subset pair's reference XY is not finite";
                return SAME_ERANGE;
            }
            const int64_t n_zone = (int64_t)zt[Z_ZONE];
            double box[4] = {0.0, 0.0, 0.0, 0.0};
            ZoneGrid zg = zone_geometry(box, 1);
            if (n_zone > 0) {
                SAME_TRY(grid_bbox(ctx, zw.zxy, n_zone, box));
                zg = zone_geometry(box, n_zone);
                SAME_TRY(grid_fill(ctx, zw.zxy, n_zone, zg.g, zw.start, zw.rank, zw.sxy, zw.sidx));
            }
            SAME_LAUNCH(ctx, zone_walk_kernel, dim3(grid_for(n)), dim3(NT), 0, fin, n, zw.flag, ref->xy, n_zone, zw.sxy, zw.start, zg, zone->edges, B,
                        zw.bin, out_d2 ? zw.d2 : nullptr);
            SAME_LAUNCH(ctx, feature_sums_kernel, sums_grid(n, F, B + 1), dim3(NT), 0, fin, n, mov->n, ref->n, zw.bin, 1, B + 1, -1, feats->mov_q,
                        feats->F_m, feats->ref_q, feats->F_r, bins + lo.bin_rows(), bins + lo.bin_sums(), nullptr, nullptr, (int64_t)0);
        }
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h.data(), bins, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (zone && out_d2 && mov->n > 0) {
            SAME_COPY(ctx, out_d2, zw.d2, (size_t)mov->n * sizeof(double), hipMemcpyDeviceToHost);
            d2_copied = true;
        }
        SAME_WAIT(ctx);
        doubt.sound();
        fs.flip(words);
        if (zone) {
            doubt_zone.sound();
            a->zone_sets.flip();
        }
        if (h[(size_t)lo.bad()]) {
            ctx->err = "same_merge_acc_score_features: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    if (out_d2 && !d2_copied)
        for (int64_t i = 0; i < mov->n; ++i) out_d2[i] = std::nan("");
    for (int64_t q = 0; q < lo.out_words(); ++q) out[q] = (int64_t)h[(size_t)q];
    out[0] = n;
    out[1] = n - out[lo.rows() + G];
    out[2] = (int64_t)zt[Z_ZONE];
    out[3] = (int64_t)zt[Z_SUBSET];
    return SAME_OK;
}

}  // extern "C"
