// feature_kernels.h -- the kernels that read matched pairs as FEATURE SUMS, stated once for the two calls that do:
// same_merge_acc_score_features (window_score_feature.hip: a pair is a final row, its rows are section rows) and
// same_merge_acc_unpack_features (window_unpack_feature.hip: a pair is a cell pair of win::unpack_run, its rows are members).
//
// A kernel here is templated over WHERE A PAIR COMES FROM (FinalSource, PairSource below): item i of the source is a pair of a moving row
// and a reference row (rows of the two feature matrices, of the flags and -- the reference's -- of the XY), or it is no pair.  Everything
// else -- the tiling, the LDS bins, the flush, the scan, the walk -- does not know which.
//
//   feature_sums_kernel   one wave per run of pairs, a tile of 64 feature columns: lane = column, so a pair's share of a feature row is
//                         one coalesced 256-byte read of int32.  A block keeps int64 sums for 64 bins x 64 columns in LDS (32 KB: four
//                         blocks a CU beside their registers), walks its share of a capped grid and flushes one 64-bit integer atomic per
//                         non-zero sum -- a bin's 64 columns as one 512-byte wave instruction.  blockIdx.y = column tile, blockIdx.z = the
//                         chunk of 64 bins the block sums (up to 257 groups: a block skips the pairs of other chunks after their 4-byte
//                         group read).  The columns are fixed point (include/same_hip.h): integer sums are exact, the same from run to
//                         run and under every grid shape, which no float sum would be.  No 32-bit word holds a sum anywhere.
//   zone_flag_kernel      per item its two flags, the zone pairs' reference XY compacted by scan.h's scan (zone pairs and subset pairs
//                         are the scan's two counters), the items counted as bad and the flagged pairs with a non-finite XY
//   (grid.h)              knn.hip's build bins the compacted points: bounding box, counts, scan, scatter
//   zone_walk_kernel      one thread per subset pair: rings of cells out from the pair's cell until a lower bound on everything not walked
//                         exceeds the best d2 (align.hip's unwalked_lb2 at k = 1; no "decided" band: a tie does not change a minimum);
//                         then the bin by the edges, marked for the second run of feature_sums_kernel.  A ring is clipped to the grid and
//                         the ring number is bounded by the grid's extent, whatever the coordinates.
//
// A brute-force LDS-tiled minimum was not measured against the grid (the notebook's shape: 91 684 pairs against 20 009 zone points).
#pragma once
#include "grid.h"
#include "window_internal.h"

namespace win {
namespace feat {

constexpr int NT = 256, WAVES = NT / 64, TILE = 64, CHUNK = 64, UNROLL = 4;
constexpr int MAX_BLOCKS = 512;          // blocks of a sums launch, tiles and chunks included: the flushes stay few beside the pair work
constexpr int32_t Q_MAX = 1 << 30;
enum { Z_ZONE = 0, Z_SUBSET = 1, Z_BAD = 2, Z_NONFINITE = 3, ZONE_TOTALS = 4 };
static_assert(NT == scan::NT && NT == SCORE_NT, "the flag kernel scans and totals with the score kernels' block");

// ---- where a pair comes from ---------------------------------------------------------------------------------------------------------------
// at(i, a, r): 1 item i is the pair (moving row a, reference row r); 0 it is no pair and nobody counts it; -1 it is no pair and counted
// as bad.  slot(i, a): where the pair's d2 is written, of slots() slots.
struct FinalSource {                              // a merge's final rows: a row outside the sections is bad; d2 per MOVING ROW
    const FinalRec *rows;
    int64_t n, n_mov, n_ref;
    __device__ __forceinline__ int at(int64_t i, int64_t &a, int64_t &r) const {
        const FinalRec rec = rows[i];             // (one address per wave in the sums kernel: a broadcast)
        a = rec.a_row;
        r = rec.r_row;
        return followed(rec, n_mov, n_ref) ? 1 : -1;
    }
    __host__ __device__ int64_t slots() const { return n_mov; }
    __device__ __forceinline__ int64_t slot(int64_t, int64_t a) const { return a; }
};
struct PairSource {                               // win::DevicePairs: rows are flat members; -1 is an infeasible row's; d2 per PAIR
    const int64_t *ref_member;
    const int32_t *mov_member;
    int64_t n, n_mov, n_ref;                      // pairs; members of the two sides
    __device__ __forceinline__ int at(int64_t i, int64_t &a, int64_t &r) const {
        a = mov_member[i];
        r = ref_member[i];
        return a >= 0 && a < n_mov && r >= 0 && r < n_ref ? 1 : 0;
    }
    __host__ __device__ int64_t slots() const { return n; }
    __device__ __forceinline__ int64_t slot(int64_t i, int64_t) const { return i; }
};

// the words of a set of sums: include/same_hip.h's `out`, then the items counted as bad
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

// The zone call's work buffer, laid for `rows` >= items, d2 slots.  Idle: the scan words and the totals of both sets zero; the rest is
// written before it is read.
struct ZoneWork {
    unsigned long long *status[2] = {nullptr, nullptr}, *totals = nullptr;   // two sets: look-back words, [ZONE_TOTALS]
    uint8_t *flag = nullptr;                      // [rows] per item: bit 0 zone pair, bit 1 subset pair
    int32_t *bin = nullptr;                       // [rows] per item: the subset pair's distance bin, -1 no subset pair
    double *zxy = nullptr, *d2 = nullptr;         // [rows][2] the zone pairs' XY, compacted; [rows] per d2 slot
    unsigned *start = nullptr, *rank = nullptr;   // the grid of the zone pairs: [2 * rows + 17], [rows]
    double *sxy = nullptr;                        // [rows][2]
    int32_t *sidx = nullptr;                      // [rows]
    size_t status_words = 0, zero_bytes = 0, bytes = 0;
};
inline void lay(ZoneWork &z, Carver &cv, int64_t rows) {
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
// bin of pair i: bin_of[by_item ? i : its moving row] where that is in [0, n_bins), else `rest` (negative: the pair is left out);
// bin_of null: bin 0.  cnt[n_bins], sums[n_bins][F]; `bad` (may be null): the items counted as bad.
template <class Source>
__global__ __launch_bounds__(NT) void feature_sums_kernel(const Source src, const int32_t *__restrict__ bin_of, int by_item, int n_bins,
                                                          int rest, const int32_t *__restrict__ mov_q, int F_m,
                                                          const int32_t *__restrict__ ref_q, int F_r, unsigned long long *__restrict__ cnt,
                                                          unsigned long long *__restrict__ sums, unsigned long long *__restrict__ bad,
                                                          unsigned long long *__restrict__ next, int64_t next_dirty) {
    __shared__ unsigned long long lds_sum[CHUNK][TILE];
    __shared__ unsigned lds_cnt[CHUNK];
    __shared__ unsigned lds_bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int F = F_m + F_r, col = (int)blockIdx.y * TILE + lane, bin0 = (int)blockIdx.z * CHUNK;
    const bool counts_here = blockIdx.y == 0, bad_here = bad && blockIdx.y == 0 && blockIdx.z == 0;
    const int64_t n = src.n;
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
        for (int u = 0; u < UNROLL; ++u) {        // the loads of UNROLL pairs in flight before the first LDS atomic
            const int64_t i = i0 + (int64_t)u * stride;
            local[u] = -1;
            q[u] = 0;
            if (i >= n) continue;
            int64_t a, r;
            const int is_pair = src.at(i, a, r);
            if (is_pair <= 0) {
                if (is_pair < 0 && bad_here && lane == 0) atomicAdd(&lds_bad, 1u);
                continue;
            }
            const int32_t g = bin_of ? bin_of[by_item ? i : a] : 0;
            const int bin = g >= 0 && g < n_bins ? g : rest;
            if (bin < bin0 || bin >= bin0 + CHUNK) continue;
            local[u] = bin - bin0;
            if (col < F) q[u] = col < F_m ? mov_q[a * F_m + col] : ref_q[r * F_r + (col - F_m)];
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

inline dim3 sums_grid(int64_t n, int F, int n_bins) {
    const int64_t tiles = ceil_div(F, TILE), chunks = ceil_div(n_bins, CHUNK);
    const int64_t want = ceil_div(n > 0 ? n : 1, WAVES * UNROLL * 4);            // a wave has a few rounds of pairs to walk
    const int64_t x = std::max<int64_t>(1, std::min<int64_t>(want, std::max<int64_t>(MAX_BLOCKS / (tiles * chunks), 8)));
    return dim3((unsigned)x, (unsigned)tiles, (unsigned)chunks);
}

// ---- (b) zone -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pair_flags(int64_t a, int64_t r, const uint8_t *__restrict__ mov_flags,
                                               const uint8_t *__restrict__ ref_flags) {
    return (mov_flags ? mov_flags[a] : 3u) & (ref_flags ? ref_flags[r] : 3u) & 3u;
}

template <class Source>
__global__ __launch_bounds__(NT) void zone_flag_kernel(const Source src, const uint8_t *__restrict__ mov_flags,
                                                       const uint8_t *__restrict__ ref_flags, const double *__restrict__ ref_xy,
                                                       unsigned long long *status, unsigned long long *__restrict__ next_status,
                                                       int64_t status_words, unsigned long long *__restrict__ totals,
                                                       unsigned long long *__restrict__ next_totals, uint8_t *__restrict__ flag,
                                                       double *__restrict__ zxy, double *__restrict__ d2_out) {
    __shared__ scan::Shared sh;
    const int64_t n = src.n, n_slots = src.slots();
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x, all = (int64_t)gridDim.x * NT;
    for (int64_t w = i; w < status_words; w += all) next_status[w] = 0ull;          // what the NEXT call scans and totals in
    if (blockIdx.x == 0 && threadIdx.x < ZONE_TOTALS) next_totals[threadIdx.x] = 0ull;
    if (d2_out)
        for (int64_t m = i; m < n_slots; m += all) d2_out[m] = __builtin_nan("");   // (the walk kernel, a later launch, writes the subset pairs')
    auto val = [&](int64_t q) {
        if (q >= n) return scan::Pair{0u, 0u};
        int64_t a, r;
        if (src.at(q, a, r) <= 0) return scan::Pair{0u, 0u};
        const unsigned f = pair_flags(a, r, mov_flags, ref_flags);
        return scan::Pair{f & 1u, f >> 1};
    };
    scan::Pair through;
    const scan::Pair off = scan::exclusive(status, (int)blockIdx.x, val, sh, &through);
    bool outside = false, nonfinite = false;
    if (i < n) {
        int64_t a, r;
        const int is_pair = src.at(i, a, r);
        unsigned f = 0u;
        if (is_pair > 0) {
            f = pair_flags(a, r, mov_flags, ref_flags);
            if (f) {
                const double x = ref_xy[2 * r], y = ref_xy[2 * r + 1];
                nonfinite = !(__builtin_isfinite(x) && __builtin_isfinite(y));
                if (f & 1u) {
                    zxy[2 * (int64_t)off.a] = x;
                    zxy[2 * (int64_t)off.a + 1] = y;
                }
            }
        } else {
            outside = is_pair < 0;
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
inline ZoneGrid zone_geometry(const double box[4], int64_t n) {
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

// min over the n_zone binned points of dx*dx + dy*dy (fp64, no contraction: the library's -ffp-contract=off); NaN with no point
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

// one thread per item: a subset pair's d2 and bin; -1 for every other item
template <class Source>
__global__ __launch_bounds__(NT) void zone_walk_kernel(const Source src, const uint8_t *__restrict__ flag,
                                                       const double *__restrict__ ref_xy, int64_t n_zone, const double *__restrict__ sxy,
                                                       const unsigned *__restrict__ start, ZoneGrid z, const double *__restrict__ edges,
                                                       int B, int32_t *__restrict__ bin_of, double *__restrict__ d2_out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= src.n) return;
    const unsigned f = flag[i];
    if (!(f & 2u)) {
        bin_of[i] = -1;
        return;
    }
    int64_t a, r;
    (void)src.at(i, a, r);                        // (flagged: a pair)
    const double d2 = (f & 1u) ? 0.0 : nearest_d2(sxy, start, z, n_zone, ref_xy[2 * r], ref_xy[2 * r + 1]);
    int bin = B;                                  // NaN, and a d2 outside (edges[0], edges[B]]: no bin
    for (int b = 0; b < B; ++b)
        if (d2 > edges[b] && d2 <= edges[b + 1]) {
            bin = b;
            break;
        }
    bin_of[i] = bin;
    if (d2_out) d2_out[src.slot(i, a)] = d2;
}

// ---- (c) the zone phases, enqueued: flag, the wait for the totals, the grid build, the walk, the sums by bin --------------------------------
// What the two calls do alike between their sums by group and their last copy.  `zt` takes the four totals; SAME_ERANGE with ctx->err
// set where an item is bad or a flagged pair's reference XY is not finite -- found before anything is binned by it.  One launch, one copy
// (32 bytes), one WAIT; where there is a zone pair grid.h's build; two launches.
template <class Source>
int zone_phases(same_ctx *ctx, const char *bad_text, const char *nonfinite_text, const Source &src, const ZoneWork &zw, int zset,
                const uint8_t *mov_flags, const uint8_t *ref_flags, const double *edges, int B, const double *ref_xy, bool want_d2,
                const int32_t *mov_q, int F_m, const int32_t *ref_q, int F_r, unsigned long long *bin_cnt, unsigned long long *bin_sums,
                unsigned long long zt[ZONE_TOTALS]) {
    const int64_t n = src.n;
    unsigned long long *totals = zw.totals + (size_t)zset * ZONE_TOTALS, *next_totals = zw.totals + (size_t)(zset ^ 1) * ZONE_TOTALS;
    SAME_LAUNCH(ctx, zone_flag_kernel<Source>, dim3(scan::blocks_for(n)), dim3(NT), 0, src, mov_flags, ref_flags, ref_xy,
                scan::arg(zw.status[zset]), zw.status[zset ^ 1], (int64_t)zw.status_words, totals, next_totals, zw.flag, zw.zxy,
                want_d2 ? zw.d2 : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    SAME_COPY(ctx, zt, totals, sizeof(unsigned long long) * ZONE_TOTALS, hipMemcpyDeviceToHost);
    SAME_WAIT(ctx);
    if (zt[Z_BAD] || zt[Z_NONFINITE]) {           // (the buffers stay in doubt: the next call lays them again)
        ctx->err = zt[Z_BAD] ? bad_text : nonfinite_text;
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
    SAME_LAUNCH(ctx, zone_walk_kernel<Source>, dim3(grid_for(n)), dim3(NT), 0, src, zw.flag, ref_xy, n_zone, zw.sxy, zw.start, zg, edges, B,
                zw.bin, want_d2 ? zw.d2 : nullptr);
    SAME_LAUNCH(ctx, feature_sums_kernel<Source>, sums_grid(n, F_m + F_r, B + 1), dim3(NT), 0, src, zw.bin, 1, B + 1, -1, mov_q, F_m, ref_q,
                F_r, bin_cnt, bin_sums, nullptr, nullptr, (int64_t)0);
    return SAME_OK;
}

template <class T>
int upload(same_ctx *ctx, T **dst, const T *src, size_t count) {
    if (!src || !count) return SAME_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(dst), count * sizeof(T)));
    HIP_TRY(ctx, hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return SAME_OK;
}

// what same_score_features_create and same_unpack_features_create check of the host matrices before anything is uploaded
inline int check_columns(same_ctx *ctx, const char *who, const int32_t *mov_q, int64_t n_mov, int F_m, const int32_t *ref_q, int64_t n_ref,
                         int F_r, const int32_t *group_of, int n_groups) {
    REQUIRE(ctx, F_m >= 0 && F_r >= 0 && (int64_t)F_m + F_r >= 1 && (int64_t)F_m + F_r <= SAME_FEATURE_MAX_COLUMNS);
    REQUIRE(ctx, n_groups >= 1 && n_groups <= SAME_SCORE_MAX_GROUPS);
    REQUIRE(ctx, (mov_q || !F_m || !n_mov) && (ref_q || !F_r || !n_ref));
    const struct { const int32_t *q; int64_t count; } sides[2] = {{mov_q, n_mov * F_m}, {ref_q, n_ref * F_r}};
    for (const auto &s : sides)
        for (int64_t i = 0; i < s.count; ++i)
            if (s.q[i] > Q_MAX || s.q[i] < -Q_MAX) {
                ctx->err = std::string(who) + ": a quantised value is beyond 2^30 in magnitude";
                return SAME_ERANGE;
            }
    if (group_of)
        for (int64_t i = 0; i < n_mov; ++i)
            if (group_of[i] >= n_groups) {
                ctx->err = std::string(who) + ": a group value is not below n_groups";
                return SAME_ERANGE;
            }
    return SAME_OK;
}
inline int check_edges(same_ctx *ctx, const double *d2_edges, int n_edges) {
    REQUIRE(ctx, d2_edges && n_edges >= 2 && n_edges <= SAME_FEATURE_MAX_EDGES);
    for (int q = 0; q < n_edges; ++q) REQUIRE(ctx, d2_edges[q] == d2_edges[q] && (q == 0 || d2_edges[q] >= d2_edges[q - 1]));
    return SAME_OK;
}

}  // namespace feat
}  // namespace win
