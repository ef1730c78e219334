// align.hip -- the k-nearest-template label check of eval_utils.check_alignment (src/eval_utils.py:6-53), exact against scipy.
//
// The reference asks cKDTree(template).query(query, k) for the k nearest template points of every query point and tests whether the
// query's label is among their labels.  cKDTree does not break distance ties by index: which of several (nearly) equidistant points it
// returns depends on its tree.  So the device decides a row only where that choice cannot matter and leaves the rest to the host
// (same_amd/eval_utils.py), as the triangulator does with Qhull:
//   d2 = dx*dx + dy*dy in fp64 (-ffp-contract=off);  d_k = the k-th smallest d2;
//   B = {d2 within d_k * ALIGN_REL + ALIGN_ABS of d_k} (the boundary group),  S = {d2 below B}.
// Whatever scipy's rounding of the same sums (FMA or not, bounding-box pruning included: a few ulps), its k nearest are all of S and
// k - |S| members of B.  Decided: k > 1 -- label in S (match), label in no member of B (no match), |S| + |B| <= k (match);
// k == 1 -- |S| = 0 and |B| = 1 (the nearest point is unique, and it is written out).  Everything else is in doubt.
//
// Kernel shape: one thread per query.  The template is counting-sorted into a uniform grid (knn.hip's build, grid.h) with about
// max(1, k/2) points per cell; the queries are counting-sorted into the same cells, so the threads of a wave search neighbouring
// cells.  Pass 1 walks square rings of cells out from the query's (clamped) cell and keeps the k smallest d2 (an unrolled insertion
// chain in k registers for k <= 8; for 8 < k <= 64 a k-long chain in LDS, 64-thread blocks); it stops when a lower bound on the
// distance to every cell not yet walked exceeds the top of B -- not merely d_k, or B could be incomplete.  Pass 2 walks the same block again and counts S and B and their label matches.  No
// atomics; the grid and the candidates come from L1/L2.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "grid.h"
#include "same_hip.h"

namespace {

constexpr double ALIGN_REL = 1e-12;    // ~4500 ulps: far above any rounding difference between two evaluations of the same d2
constexpr double ALIGN_ABS = 1e-300;   // squares that reach the subnormal range
constexpr int ALIGN_NT = 256;

struct AlignGrid {
    GridDesc g;
    double cell;     // 1 / g.inv_cell
    double X1, Y1;   // far edges of the grid: x0 + gx * cell, y0 + gy * cell
    double slack;    // how far (beyond) a point can lie outside the nominal box of the cell it was binned in
};

// squared lower bound on the distance from q to every template point binned outside cells [xlo, xhi] x [ylo, yhi] (clipped to the
// grid): the nearest of the (at most four) slabs of the grid box beyond the block's sides, each widened by the slack
__device__ __forceinline__ double unwalked_lb2(const AlignGrid &a, double qx, double qy, int xlo, int xhi, int ylo, int yhi) {
    const double s = a.slack, gx0 = a.g.x0 - s, gy0 = a.g.y0 - s, gx1 = a.X1 + s, gy1 = a.Y1 + s;
    const double ox = fmax(fmax(gx0 - qx, qx - gx1), 0.0), oy = fmax(fmax(gy0 - qy, qy - gy1), 0.0);
    double lb2 = __builtin_inf();
    if (xhi < a.g.gx - 1) {
        const double dx = fmax(fmax(a.g.x0 + (double)(xhi + 1) * a.cell - s - qx, qx - gx1), 0.0);
        lb2 = fmin(lb2, dx * dx + oy * oy);
    }
    if (xlo > 0) {
        const double dx = fmax(fmax(qx - (a.g.x0 + (double)xlo * a.cell + s), gx0 - qx), 0.0);
        lb2 = fmin(lb2, dx * dx + oy * oy);
    }
    if (yhi < a.g.gy - 1) {
        const double dy = fmax(fmax(a.g.y0 + (double)(yhi + 1) * a.cell - s - qy, qy - gy1), 0.0);
        lb2 = fmin(lb2, ox * ox + dy * dy);
    }
    if (ylo > 0) {
        const double dy = fmax(fmax(qy - (a.g.y0 + (double)ylo * a.cell + s), gy0 - qy), 0.0);
        lb2 = fmin(lb2, ox * ox + dy * dy);
    }
    return lb2;
}

// The k smallest d2 seen so far, ascending; an entry enters at its place and the largest drops out.
// K > 0: K = k registers, the insertion chain fully unrolled (k <= 8; a longer list the compiler moves to scratch or LDS).
template <int K>
struct RegList {
    double v[K];
    __device__ __forceinline__ RegList() {
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = __builtin_inf();
    }
    __device__ __forceinline__ void insert(double x, int) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double b = v[i];
            const bool lt = x < b;
            v[i] = lt ? x : b;
            x = lt ? b : x;
        }
    }
    __device__ __forceinline__ double kth(int) const { return v[K - 1]; }
};
// k up to SAME_ALIGN_MAX_KNN: the list in LDS, entry i of lane l at [i][l] (64-thread blocks: conflict-free), a k-long chain
struct LdsList {
    double *col;   // &lds[0][lane]
    __device__ __forceinline__ LdsList(double *lds, int k) : col(lds + (threadIdx.x & 63)) {
        for (int i = 0; i < k; ++i) col[64 * i] = __builtin_inf();
    }
    __device__ __forceinline__ void insert(double x, int k) {
        for (int i = 0; i < k; ++i) {
            const double b = col[64 * i];
            if (x < b) {
                col[64 * i] = x;
                x = b;
            }
        }
    }
    __device__ __forceinline__ double kth(int k) const { return col[64 * (k - 1)]; }
};

template <int K>
struct ListOf { using type = RegList<K>; };
template <>
struct ListOf<0> { using type = LdsList; };

typedef double double2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double d2_at(const double *__restrict__ sxy, unsigned p, double qx, double qy) {
    const double2_t v = *reinterpret_cast<const double2_t *>(sxy + 2 * (int64_t)p);
    const double dx = v.x - qx, dy = v.y - qy;
    return dx * dx + dy * dy;
}

__global__ __launch_bounds__(256) void gather_codes_kernel(const int32_t *__restrict__ code, const int32_t *__restrict__ sidx, int64_t n,
                                                           int32_t *__restrict__ scode) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) scode[p] = code[sidx[p]];
}

// one thread per query, queries in cell order (qsxy / qsidx); out_flag / out_nearest indexed by the query's own row.
// K = 0: the list in LDS (blocks of 64 threads, 64 * k doubles of dynamic LDS)
template <int K>
__global__ __launch_bounds__(ALIGN_NT) void align_kernel(const double *__restrict__ qsxy, const int32_t *__restrict__ qsidx,
                                                         const int32_t *__restrict__ qcode, int64_t n_q, const double *__restrict__ sxy,
                                                         const int32_t *__restrict__ sidx, const int32_t *__restrict__ scode,
                                                         const unsigned *__restrict__ start, AlignGrid a, int k,
                                                         uint8_t *__restrict__ out_flag, int32_t *__restrict__ out_nearest) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_q) return;
    const GridDesc &g = a.g;
    const double2_t q = *reinterpret_cast<const double2_t *>(qsxy + 2 * t);
    const double qx = q.x, qy = q.y;
    const int32_t row = qsidx[t];
    const int32_t code = qcode[row];
    const int cx = cell_coord(qx, g.x0, g.inv_cell, g.gx), cy = cell_coord(qy, g.y0, g.inv_cell, g.gy);

    // pass 1: rings of cells until nothing unwalked can reach B
    extern __shared__ double lds_lists[];
    typename ListOf<K>::type best = [&]() {
        if constexpr (K == 0) return LdsList(lds_lists, k);
        else return RegList<K>();
    }();
    int64_t found = 0;
    double dk = __builtin_inf();
    int xlo, xhi, ylo, yhi;
    for (int r = 0;; ++r) {
        xlo = max(cx - r, 0); xhi = min(cx + r, g.gx - 1);
        ylo = max(cy - r, 0); yhi = min(cy + r, g.gy - 1);
        for (int yy = ylo; yy <= yhi; ++yy) {
            const int64_t rowc = (int64_t)yy * g.gx;
            const bool edge = yy == cy - r || yy == cy + r;
            // a ring row is the whole clipped run on the ring's top and bottom, its two end cells between them
            for (int side = 0; side < 2; ++side) {
                int c0, c1;
                if (edge) {
                    if (side) break;
                    c0 = xlo; c1 = xhi;
                } else {
                    c0 = c1 = side ? cx + r : cx - r;
                    if (c0 < 0 || c0 > g.gx - 1) continue;
                }
                const unsigned b = start[rowc + c0], e = start[rowc + c1 + 1];
                found += e - b;
                const double thr = best.kth(k);   // a d2 not below the current k-th cannot enter the k smallest
                for (unsigned p = b; p < e; ++p) {
                    const double d2 = d2_at(sxy, p, qx, qy);
                    if (d2 < thr) best.insert(d2, k);
                }
            }
        }
        const bool all = xlo == 0 && ylo == 0 && xhi == g.gx - 1 && yhi == g.gy - 1;
        if (found >= k) {
            dk = best.kth(k);
            const double hi = dk + (dk * ALIGN_REL + ALIGN_ABS);
            if (all || unwalked_lb2(a, qx, qy, xlo, xhi, ylo, yhi) * (1.0 - 1e-13) > hi) break;
        } else if (all) {
            break;   // fewer than k points in all: the host does not let this happen
        }
    }

    // pass 2: S, B and their label matches over the walked block (it holds every point up to the top of B)
    uint8_t flag = 0;
    int32_t near = -1;
    if (__builtin_isfinite(dk)) {
        const double m = dk * ALIGN_REL + ALIGN_ABS, lo = dk - m, hi = dk + m;
        int nS = 0, nB = 0;
        bool mS = false, mB = false;
        for (int yy = ylo; yy <= yhi; ++yy) {
            const int64_t rowc = (int64_t)yy * g.gx;
            const unsigned b = start[rowc + xlo], e = start[rowc + xhi + 1];
            for (unsigned p = b; p < e; ++p) {
                const double d2 = d2_at(sxy, p, qx, qy);
                if (d2 <= hi) {
                    const bool eq = scode[p] == code;
                    if (d2 < lo) {
                        ++nS; mS |= eq;
                    } else {
                        ++nB; mB |= eq; near = sidx[p];
                    }
                }
            }
        }
        if (k == 1) {
            if (nS == 0 && nB == 1) flag = SAME_ALIGN_DECIDED | (mB ? SAME_ALIGN_MATCH : 0);
        } else if (mS || (mB && nS + nB <= k)) {
            flag = SAME_ALIGN_DECIDED | SAME_ALIGN_MATCH;
        } else if (!mB) {
            flag = SAME_ALIGN_DECIDED;
        }
    }
    out_flag[row] = flag;
    if (out_nearest) out_nearest[row] = (flag & SAME_ALIGN_DECIDED) ? near : -1;
}

// Cell edge from the template's density and k (about max(1, k/2) points per cell), never more than 2 n + 16 cells (memory O(n)).
AlignGrid align_geometry(const double box[4], int64_t n, int k) {
    const double x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    const double w = x1 - x0, h = y1 - y0, ext = std::max(w, h);
    AlignGrid a;
    a.g.x0 = x0; a.g.y0 = y0;
    double cell = 1.0;
    int64_t gx = 1, gy = 1;
    if (ext > 0.0 && std::isfinite(ext)) {
        const double per_cell = std::max(1.0, 0.5 * k);
        const double area = std::max(w * h, ext * ext / (double)n);   // a set on a line still gets ~per_cell points per cell
        cell = std::max(std::sqrt(area * per_cell / (double)n), ext / 4096.0);
        for (;;) {
            gx = (int64_t)std::floor(w / cell) + 1;
            gy = (int64_t)std::floor(h / cell) + 1;
            if (gx * gy <= 2 * n + 16) break;
            cell *= 1.25;
        }
    }
    a.g.inv_cell = 1.0 / cell;
    a.g.gx = (int)gx; a.g.gy = (int)gy;
    a.cell = cell;
    a.X1 = x0 + (double)gx * cell;
    a.Y1 = y0 + (double)gy * cell;
    // binning rounds (v - x0) * inv_cell: a point can sit a few ulps of the coordinates' magnitude outside its cell's nominal box
    const double mag = std::max(std::max(std::fabs(x0), std::fabs(y0)), std::max(std::fabs(x1), std::fabs(y1)));
    a.slack = 1e-9 * cell + std::ldexp(mag, -40);
    return a;
}

}  // namespace

extern "C" {

int same_check_alignment(same_ctx *ctx, const double *qxy, int64_t n_q, const int32_t *qcode, const double *txy, int64_t n_t,
                         const int32_t *tcode, int k, uint8_t *out_flag, int32_t *out_nearest) {
    REQUIRE(ctx, ctx != nullptr);
    REQUIRE(ctx, n_q >= 0 && n_t >= 0 && k >= 1 && k <= SAME_ALIGN_MAX_KNN);
    if (n_q == 0) return SAME_OK;
    REQUIRE(ctx, k <= n_t && n_t < ((int64_t)1 << 31) && n_q < ((int64_t)1 << 31));
    REQUIRE(ctx, qxy && qcode && txy && tcode && out_flag && (k != 1 || out_nearest));
    for (int64_t i = 0; i < 2 * n_q; ++i) REQUIRE(ctx, std::isfinite(qxy[i]));
    for (int64_t i = 0; i < 2 * n_t; ++i) REQUIRE(ctx, std::isfinite(txy[i]));
    SAME_TRY(same_use(ctx));
    double *dq, *dt;
    int32_t *dqc, *dtc;
    SAME_TRY(up_as(ctx, SL_AXY, qxy, (size_t)n_q * 2, &dq));
    SAME_TRY(up_as(ctx, SL_RXY, txy, (size_t)n_t * 2, &dt));
    SAME_TRY(up_as(ctx, SL_A, qcode, (size_t)n_q, &dqc));
    SAME_TRY(up_as(ctx, SL_R, tcode, (size_t)n_t, &dtc));
    double box[4];
    SAME_TRY(grid_bbox(ctx, dt, n_t, box));
    const AlignGrid a = align_geometry(box, n_t, k);
    const int64_t cells = (int64_t)a.g.gx * a.g.gy;
    // template and queries counting-sorted by template cell
    unsigned *tstart, *trank, *qstart, *qrank;
    double *tsxy, *qsxy;
    int32_t *tsidx, *qsidx, *tscode;
    SAME_TRY(slot_as(ctx, SL_K_START, (size_t)cells + 1, &tstart));
    SAME_TRY(slot_as(ctx, SL_K_RANK, (size_t)n_t, &trank));
    SAME_TRY(slot_as(ctx, SL_K_SXY, (size_t)n_t * 2, &tsxy));
    SAME_TRY(slot_as(ctx, SL_K_SIDX, (size_t)n_t, &tsidx));
    SAME_TRY(slot_as(ctx, SL_TYPE, (size_t)n_t, &tscode));
    SAME_TRY(slot_as(ctx, SL_Q_START, (size_t)cells + 1, &qstart));
    SAME_TRY(slot_as(ctx, SL_Q_RANK, (size_t)n_q, &qrank));
    SAME_TRY(slot_as(ctx, SL_Q_SXY, (size_t)n_q * 2, &qsxy));
    SAME_TRY(slot_as(ctx, SL_Q_SIDX, (size_t)n_q, &qsidx));
    SAME_TRY(grid_fill(ctx, dt, n_t, a.g, tstart, trank, tsxy, tsidx));
    hipLaunchKernelGGL(gather_codes_kernel, dim3((unsigned)ceil_div(n_t, 256)), dim3(256), 0, ctx->stream, dtc, tsidx, n_t, tscode);
    SAME_TRY(grid_fill(ctx, dq, n_q, a.g, qstart, qrank, qsxy, qsidx));
    uint8_t *dflag;
    int32_t *dnear = nullptr;
    SAME_TRY(slot_as(ctx, SL_FLAG0, (size_t)n_q, &dflag));
    if (k == 1) SAME_TRY(slot_as(ctx, SL_MATCH, (size_t)n_q, &dnear));
    const dim3 blocks((unsigned)ceil_div(n_q, ALIGN_NT)), block(ALIGN_NT);
    switch (k) {   // k <= 8: the list is exactly k registers (an unrolled chain, the k-th at a fixed place)
#define ALIGN_CASE(K)                                                                                                                   \
    case K:                                                                                                                             \
        hipLaunchKernelGGL(align_kernel<K>, blocks, block, 0, ctx->stream, qsxy, qsidx, dqc, n_q, tsxy, tsidx, tscode, tstart, a, k, dflag, \
                           dnear);                                                                                                      \
        break;
        ALIGN_CASE(1) ALIGN_CASE(2) ALIGN_CASE(3) ALIGN_CASE(4) ALIGN_CASE(5) ALIGN_CASE(6) ALIGN_CASE(7) ALIGN_CASE(8)
#undef ALIGN_CASE
    default:
        hipLaunchKernelGGL(align_kernel<0>, dim3((unsigned)ceil_div(n_q, 64)), dim3(64), (unsigned)(64 * k * sizeof(double)), ctx->stream,
                           qsxy, qsidx, dqc, n_q, tsxy, tsidx, tscode, tstart, a, k, dflag, dnear);
    }
    HIP_TRY(ctx, hipGetLastError());
    SAME_TRY(same_down(ctx, out_flag, dflag, (size_t)n_q));
    if (k == 1) SAME_TRY(same_down(ctx, out_nearest, dnear, (size_t)n_q * sizeof(int32_t)));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

}  // extern "C"
