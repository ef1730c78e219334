// delaunay_dev.hip -- a6 on the device for the window path, as a LOCAL rule: the kept triangles of the reference's filter are exactly
// the Delaunay triangles that pass it, and a Delaunay triangle (points in general position) is a triangle whose circumcircle holds no
// other point (the empty-circle property).  The filter (src/helpers.py:298-319) drops every triangle with a side >= radius or an angle
// < min_angle, and nothing downstream sees a dropped triangle, so only triangles that pass it are looked for.  Such a triangle has
// circumradius <= radius / (2 sin min_angle) (the smallest angle faces a side shorter than `radius`), so every decision reads a
// bounded neighbourhood: no insertion order, one thread per point (only the points near the hull are looked at as a whole).
//
// Per set of points (a window's kept aligned cells, or a caller's set):
//   setup       one block: the coordinate extent, m = the largest |x| or |y|, the lifted range of z = x*x + y*y (Qhull's 'Qbb'
//               allowance, qhull_margin.h -- the very formula of the host triangulator), the eight extreme points (an octagon inside the
//               hull), a uniform grid of cells at least `radius` wide.
//   bin         a counting sort of the points into the cells (atomic slots, the cell offsets by scan.h's look-back scan, then every cell
//               sorted by point index: the layout does not depend on the order of the atomics).
//   hull        one block: the points near the hull (not deeper inside the octagon than Qhull's allowance), sorted, Andrew's monotone
//               chain; a hull corner within guard x allowance of the chord of its neighbours, or a point that close to a hull edge's line
//               (Qhull could take it for coplanar with the facet through the point at infinity, 'Qz') refuses the set.
//   candidates  point p owns the triangles (p, q, r), p < q < r, q and r within `radius` of p and of each other (a slack screen of the
//               filter's side and angle tests: a superset of what the filter keeps, never a subset); each is tested in-circle against
//               every point in the cells its circumcircle's bounding box (widened to where a point could still be in doubt) touches.
//               A sign counts only when it is beyond doubt twice over: |det| clears its own rounding bound, and the distance of the
//               lifted point from the lifted triangle's plane over Qhull's allowance (qm::judge) clears `guard`.  Some point clearly
//               inside: the candidate is not a Delaunay triangle.  No point inside, every point clearly outside: it is one.  No point
//               clearly inside but one in doubt: the SET is refused (duplicates, cocircular quads, collinear runs end here).
//   emit        the surviving triangles counter-clockwise, by owner, then q, then r (scan offsets over the owners' counts).
// Refused sets (a status, never a fault) go to Qhull as before: fewer than 3 points, no angle threshold (no circumradius bound),
// non-finite coordinates, a sign in doubt, a list longer than its buffer.  Every buffer access is checked against its capacity.
// The filter itself (classes, the keep list, the same-type re-add) stays with same_window_filter_finish's kernels, run on these
// candidates: the exact decisions are made once, with the reference's arithmetic.
#include "qhull_margin.h"
#include "window_internal.h"

namespace {

using namespace devmath;
using namespace win;
using scan::Pair;

constexpr int NB_CAP = 128;           // neighbours q > p within the screen's radius, per owner (cfg 5 at radius 50: ~40 on average)
constexpr int OWN_CAP = 32;           // surviving triangles per owner
constexpr int SURV_CAP = 1024;        // points near the hull, per set
constexpr int SCAN_CELLS_CAP = 256;   // cells one circumcircle's box may touch
constexpr double SIGN_MARGIN = 1e-12; // a determinant is trusted when it clears SIGN_MARGIN x the sum of the |products| it is made of
constexpr double SCREEN_SLACK = 1e-9; // the screen's slack on the side length and on the corner cosine (the filter's near band is 8 ulp)

enum { ST_STATUS = 0, ST_TRIS = 1, ST_WORDS = 8 };

// the set's parameters, written by the setup kernel
struct Par {
    double x0, y0, cw, r2s, delta, w, sc_m;
    qm::Scale sc;
    double ox[8], oy[8];
    int nx, ny, ncell, n_oct;
};

struct Job {
    const double *xy;
    int64_t n, ncell_cap, cap_out;
    unsigned long long *st;           // [ST_WORDS]: status bits, triangles emitted
    unsigned long long *scan_cells, *scan_own;
    unsigned *cell_cnt, *cell_start, *slot, *own_cnt;
    int32_t *cell_of, *sorted, *own_tris, *out;
    Par *par;
};

struct Settings {
    double radius, cos_thr, guard;
};

__device__ __forceinline__ void refuse(const Job &j, unsigned bits) { atomicOr(&j.st[ST_STATUS], (unsigned long long)bits); }
__device__ __forceinline__ unsigned long long status_of(const Job &j) {
    return __hip_atomic_load(&j.st[ST_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cell_x(const Par &p, double x) {
    const double f = std::floor((x - p.x0) / p.cw);
    return !(f >= 0.0) ? 0 : (f >= (double)p.nx ? p.nx - 1 : (int)f);     // NaN: cell 0 (a set with a NaN is refused in setup)
}
__device__ __forceinline__ int cell_y(const Par &p, double y) {
    const double f = std::floor((y - p.y0) / p.cw);
    return !(f >= 0.0) ? 0 : (f >= (double)p.ny ? p.ny - 1 : (int)f);
}

// ---- setup: one block per set ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_min(double v, double *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(sh[0], sh[1]), fmin(sh[2], sh[3]));
}
// the largest value, the smallest index among equals
__device__ __forceinline__ void block_argmax(double &v, int64_t &i, double *shv, int64_t *shi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int64_t oi = __shfl_xor(i, off, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = shv[0];
    i = shi[0];
    for (int q = 1; q < 4; ++q)
        if (shv[q] > v || (shv[q] == v && shi[q] < i)) { v = shv[q]; i = shi[q]; }
}

// directions of the octagon's corners, counter-clockwise from -90 degrees
__device__ __forceinline__ double oct_dir(int k, double x, double y) {
    switch (k) {
        case 0: return -y;
        case 1: return x - y;
        case 2: return x;
        case 3: return x + y;
        case 4: return y;
        case 5: return y - x;
        case 6: return -x;
        default: return -x - y;
    }
}

__global__ __launch_bounds__(256) void dd_setup_kernel(Batch<Job> b, Settings set) {
    const Job &j = b.w[blockIdx.y];
    __shared__ double shv[4];
    __shared__ int64_t shi[4];
    const int64_t n = j.n;
    double mnx = __builtin_inf(), mny = mnx, mxx = mnx, mxy = mnx, zmin = mnx, zmax = mnx, m = mnx;   // all kept as minima
    bool bad = false;
    double ov[8];
    int64_t oi[8];
    for (int k = 0; k < 8; ++k) { ov[k] = -__builtin_inf(); oi[k] = INT64_MAX; }
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = j.xy[2 * i], y = j.xy[2 * i + 1];
        if (!(std::isfinite(x) && std::isfinite(y))) { bad = true; continue; }
        const double z = x * x + y * y;
        mnx = fmin(mnx, x); mxx = fmin(mxx, -x); mny = fmin(mny, y); mxy = fmin(mxy, -y);
        zmin = fmin(zmin, z); zmax = fmin(zmax, -z);
        m = fmin(m, -fmax(std::fabs(x), std::fabs(y)));
        for (int k = 0; k < 8; ++k) {
            const double v = oct_dir(k, x, y);
            if (v > ov[k] || (v == ov[k] && i < oi[k])) { ov[k] = v; oi[k] = i; }
        }
    }
    if (bad) refuse(j, SAME_DD_NONFINITE);
    mnx = block_min(mnx, shv); mxx = -block_min(mxx, shv); mny = block_min(mny, shv); mxy = -block_min(mxy, shv);
    zmin = block_min(zmin, shv); zmax = -block_min(zmax, shv); m = -block_min(m, shv);
    for (int k = 0; k < 8; ++k) block_argmax(ov[k], oi[k], shv, shi);
    if (threadIdx.x != 0) return;
    Par &p = *j.par;
    if (n < 3) { refuse(j, SAME_DD_FEW_POINTS); p.nx = p.ny = p.ncell = 1; p.n_oct = 0; p.x0 = p.y0 = 0.0; p.cw = 1.0; return; }
    p.sc = qm::scale(m, zmin, zmax);
    const double w = fmax(mxx - mnx, mxy - mny);
    p.w = w;
    p.sc_m = m;
    p.x0 = mnx;
    p.y0 = mny;
    p.r2s = (set.radius * (1.0 + SCREEN_SLACK)) * (set.radius * (1.0 + SCREEN_SLACK));
    // cells at least radius wide (a point's screen neighbours lie in the 3 x 3 cells around it), and no more cells than the buffer has
    double cw = set.radius * (1.0 + 1e-6);
    int64_t nx = 1, ny = 1;
    for (int it = 0; it < 64; ++it) {
        const double fx = std::floor((mxx - mnx) / cw) + 1.0, fy = std::floor((mxy - mny) / cw) + 1.0;
        if (fx * fy <= (double)j.ncell_cap) { nx = (int64_t)fx; ny = (int64_t)fy; break; }
        cw *= 2.0;
        nx = 0;
    }
    if (nx == 0 || !(cw > 0.0) || !std::isfinite(cw)) { refuse(j, SAME_DD_OVERFLOW); nx = ny = 1; }
    p.cw = cw;
    p.nx = (int)nx;
    p.ny = (int)ny;
    p.ncell = (int)(nx * ny);
    // Qhull's coplanar band in plain coordinates, and how far inside the octagon a point must lie to be clear of the hull by more
    // (the octagon lies inside the hull; its own cross products round by a few eps x extent)
    p.delta = 4.0 * set.guard * p.sc.allow + 64.0 * qm::EPS * (w + m);
    int c = 0;
    for (int k = 0; k < 8; ++k) {
        const int64_t i = oi[k];
        if (i < 0 || i >= n) continue;
        const double x = j.xy[2 * i], y = j.xy[2 * i + 1];
        if (c > 0 && x == p.ox[c - 1] && y == p.oy[c - 1]) continue;
        if (k == 7 && c > 0 && x == p.ox[0] && y == p.oy[0]) continue;
        p.ox[c] = x;
        p.oy[c] = y;
        ++c;
    }
    p.n_oct = c;
}

// ---- bin: counting sort into the cells -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dd_count_kernel(Batch<Job> b) {
    const Job &j = b.w[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n || j.n < 3) return;
    const Par &p = *j.par;
    const int c = cell_y(p, j.xy[2 * i + 1]) * p.nx + cell_x(p, j.xy[2 * i]);
    j.cell_of[i] = c;
    j.slot[i] = atomicAdd(&j.cell_cnt[c], 1u);
}
__global__ __launch_bounds__(scan::NT) void dd_cell_scan_kernel(Batch<Job> b) {
    __shared__ scan::Shared sh;
    const Job &j = b.w[blockIdx.y];
    if (j.n < 3) return;
    const int64_t nc = j.par->ncell;
    const int nb = (int)scan::blocks_for(nc);
    if ((int)blockIdx.x >= nb) return;
    const unsigned *cnt = j.cell_cnt;
    auto val = [&](int64_t c) { return Pair{c < nc ? cnt[c] : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(j.scan_cells, (int)blockIdx.x, val, sh, &through);
    const int64_t c = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (c < nc) j.cell_start[c] = off.a;
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) j.cell_start[nc] = through.a;
}
__global__ __launch_bounds__(256) void dd_scatter_kernel(Batch<Job> b) {
    const Job &j = b.w[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n || j.n < 3) return;
    const int64_t at = (int64_t)j.cell_start[j.cell_of[i]] + j.slot[i];
    if (at >= 0 && at < j.n) j.sorted[at] = (int32_t)i;
}
// every cell's points by index (a cell holds a handful: insertion sort)
__global__ __launch_bounds__(256) void dd_cell_sort_kernel(Batch<Job> b) {
    const Job &j = b.w[blockIdx.y];
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j.n < 3 || c >= j.par->ncell) return;
    const int64_t lo = j.cell_start[c], hi = j.cell_start[c + 1];
    if (lo < 0 || hi > j.n) return;
    int32_t *s = j.sorted;
    for (int64_t a = lo + 1; a < hi; ++a) {
        const int32_t v = s[a];
        int64_t q = a - 1;
        while (q >= lo && s[q] > v) { s[q + 1] = s[q]; --q; }
        s[q + 1] = v;
    }
}

// ---- hull: one block per set --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cross3(double ax, double ay, double bx, double by, double cx, double cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

__global__ __launch_bounds__(256) void dd_hull_kernel(Batch<Job> b, Settings set) {
    const Job &j = b.w[blockIdx.y];
    if (j.n < 3 || status_of(j)) return;
    const Par &p = *j.par;
    __shared__ double ux[SURV_CAP], uy[SURV_CAP], sx[SURV_CAP], sy[SURV_CAP];
    __shared__ int32_t ui[SURV_CAP], si[SURV_CAP];
    __shared__ int hull[2 * SURV_CAP + 2];
    __shared__ int n_surv, n_hull, verdict;
    if (threadIdx.x == 0) { n_surv = 0; n_hull = 0; verdict = 0; }
    __syncthreads();
    const int n_oct = p.n_oct;
    // the points not clear of the hull: not deeper inside the octagon than delta
    for (int64_t i = threadIdx.x; i < j.n; i += blockDim.x) {
        const double x = j.xy[2 * i], y = j.xy[2 * i + 1];
        bool deep = n_oct >= 3;
        for (int k = 0; k < n_oct && deep; ++k) {
            const int k1 = k + 1 == n_oct ? 0 : k + 1;
            const double ex = p.ox[k1] - p.ox[k], ey = p.oy[k1] - p.oy[k];
            const double len = std::sqrt(ex * ex + ey * ey);
            // (the cross product's own rounding: a few eps of the coordinates' size times the lengths it multiplies)
            deep = cross3(p.ox[k], p.oy[k], p.ox[k1], p.oy[k1], x, y) > p.delta * len + 16.0 * qm::EPS * (p.sc_m + p.w) * (len + 2.0 * p.w);
        }
        if (!deep) {
            const int at = atomicAdd(&n_surv, 1);
            if (at < SURV_CAP) { ux[at] = x; uy[at] = y; ui[at] = (int32_t)i; }
        }
    }
    __syncthreads();
    const int k = n_surv;
    if (k > SURV_CAP || k < 3) {
        if (threadIdx.x == 0) refuse(j, k > SURV_CAP ? SAME_DD_OVERFLOW : SAME_DD_IN_DOUBT);
        return;
    }
    // sorted by (x, y, index): rank by counting
    for (int a = threadIdx.x; a < k; a += blockDim.x) {
        int r = 0;
        for (int c = 0; c < k; ++c)
            r += ux[c] < ux[a] || (ux[c] == ux[a] && (uy[c] < uy[a] || (uy[c] == uy[a] && ui[c] < ui[a])));
        sx[r] = ux[a]; sy[r] = uy[a]; si[r] = ui[a];
    }
    __syncthreads();
    // Andrew's monotone chain (one thread: the points near the hull are few), counter-clockwise, collinear points dropped
    if (threadIdx.x == 0) {
        int h = 0;
        for (int a = 0; a < k; ++a) {
            while (h >= 2 && cross3(sx[hull[h - 2]], sy[hull[h - 2]], sx[hull[h - 1]], sy[hull[h - 1]], sx[a], sy[a]) <= 0.0) --h;
            hull[h++] = a;
        }
        for (int a = k - 2, lo = h + 1; a >= 0; --a) {
            while (h >= lo && cross3(sx[hull[h - 2]], sy[hull[h - 2]], sx[hull[h - 1]], sy[hull[h - 1]], sx[a], sy[a]) <= 0.0) --h;
            hull[h++] = a;
        }
        n_hull = h - 1;       // the first point closes the chain
        if (n_hull < 3) verdict = 1;
    }
    __syncthreads();
    const int h = n_hull;
    if (!verdict) {
        // hull corners against the chord of their neighbours; every point near the hull against every hull edge's line
        for (int t = threadIdx.x; t < h; t += blockDim.x) {
            const int a = hull[(t + h - 1) % h], c = hull[t], d = hull[(t + 1) % h];
            const double area2 = std::fabs(cross3(sx[a], sy[a], sx[c], sy[c], sx[d], sy[d]));
            const double chord = std::sqrt((sx[d] - sx[a]) * (sx[d] - sx[a]) + (sy[d] - sy[a]) * (sy[d] - sy[a]));
            if (!(qm::plain_ratio(area2, chord, p.sc) > set.guard)) atomicOr(&verdict, 1);
        }
        for (int64_t q = threadIdx.x; q < (int64_t)k * h; q += blockDim.x) {
            const int s = (int)(q / h), e = (int)(q % h);
            const int a = hull[e], c = hull[(e + 1) % h];
            if (s == a || s == c) continue;
            const double area2 = std::fabs(cross3(sx[a], sy[a], sx[c], sy[c], sx[s], sy[s]));
            const double edge = std::sqrt((sx[c] - sx[a]) * (sx[c] - sx[a]) + (sy[c] - sy[a]) * (sy[c] - sy[a]));
            if (!(qm::plain_ratio(area2, edge, p.sc) > set.guard)) atomicOr(&verdict, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && verdict) refuse(j, SAME_DD_IN_DOUBT);
}

// ---- candidates: one thread per owner -------------------------------------------------------------------------------------------
__device__ __forceinline__ double max_corner_cos(double2_t a, double2_t b, double2_t c) {
    const double c1 = corner_cos(b, a, c), c2 = corner_cos(a, b, c), c3 = corner_cos(a, c, b);
    return fmax(fmax(c1, c2), c3);
}

__global__ __launch_bounds__(256) void dd_candidate_kernel(Batch<Job> b, Settings set) {
    const Job &j = b.w[blockIdx.y];
    const int64_t pi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= j.n || j.n < 3 || status_of(j)) return;
    const Par &p = *j.par;
    const double *__restrict__ xy = j.xy;
    const int32_t *__restrict__ sorted = j.sorted;
    const unsigned *__restrict__ start = j.cell_start;
    const double2_t P = ld2(xy, pi);
    const int c0 = j.cell_of[pi], cx = c0 % p.nx, cy = c0 / p.nx;
    int32_t nb[NB_CAP];
    int k = 0;
    for (int yy = cy - 1; yy <= cy + 1; ++yy) {
        if (yy < 0 || yy >= p.ny) continue;
        for (int xx = cx - 1; xx <= cx + 1; ++xx) {
            if (xx < 0 || xx >= p.nx) continue;
            const int c = yy * p.nx + xx;
            for (unsigned q = start[c]; q < start[c + 1]; ++q) {
                const int32_t s = sorted[q];
                if (s <= pi) continue;
                const double2_t S = ld2(xy, s);
                const double dx = S.x - P.x, dy = S.y - P.y;
                if (dx * dx + dy * dy >= p.r2s) continue;
                if (k == NB_CAP) { refuse(j, SAME_DD_OVERFLOW); return; }
                nb[k++] = s;
            }
        }
    }
    for (int a = 1; a < k; ++a) {              // ascending: the candidates come by q, then r
        const int32_t v = nb[a];
        int q = a - 1;
        while (q >= 0 && nb[q] > v) { nb[q + 1] = nb[q]; --q; }
        nb[q + 1] = v;
    }
    int32_t *own = j.own_tris + pi * (int64_t)OWN_CAP * 3;
    unsigned count = 0;
    for (int a = 0; a < k; ++a) {
        const double2_t Q = ld2(xy, nb[a]);
        for (int bq = a + 1; bq < k; ++bq) {
            const double2_t R = ld2(xy, nb[bq]);
            const double qx = R.x - Q.x, qy = R.y - Q.y;
            if (qx * qx + qy * qy >= p.r2s) continue;
            if (!(max_corner_cos(P, Q, R) < set.cos_thr + SCREEN_SLACK)) continue;
            // counter-clockwise from p
            double2_t B = Q, C = R;
            int32_t ib = nb[a], ic = nb[bq];
            const double o = cross3(P.x, P.y, Q.x, Q.y, R.x, R.y);
            if (o < 0.0) { B = R; C = Q; ib = nb[bq]; ic = nb[a]; }
            const double dx = B.x - P.x, dy = B.y - P.y, ex = C.x - P.x, ey = C.y - P.y;
            const double bl = dx * dx + dy * dy, cl = ex * ex + ey * ey, d = dx * ey - dy * ex;
            if (!(d > 0.0)) { refuse(j, SAME_DD_IN_DOUBT); return; }     // a screened triangle is never this flat: rounding at work
            const double ucx = (ey * bl - dy * cl) * 0.5 / d, ucy = (dx * cl - ex * bl) * 0.5 / d;
            const double ccx = P.x + ucx, ccy = P.y + ucy, rad = std::sqrt(ucx * ucx + ucy * ucy);
            const double jd = qm::judge(P.x, P.y, dx, dy, ex, ey, p.sc);
            // beyond rad + reach a point is clear of the circle by more than the guard asks (det = 2 area (R^2 - dist^2))
            const double reach = 2.0 * set.guard / (rad * d * jd) + 1e-9 * rad + 1e-12 * (std::fabs(ccx) + std::fabs(ccy));
            const int x_lo = cell_x(p, ccx - (rad + reach)), x_hi = cell_x(p, ccx + (rad + reach));
            const int y_lo = cell_y(p, ccy - (rad + reach)), y_hi = cell_y(p, ccy + (rad + reach));
            if (!(reach < 1e300) || (int64_t)(x_hi - x_lo + 1) * (y_hi - y_lo + 1) > SCAN_CELLS_CAP) { refuse(j, SAME_DD_OVERFLOW); return; }
            bool inside = false, doubt = false;
            for (int yy = y_lo; yy <= y_hi && !inside; ++yy) {
                for (int xx = x_lo; xx <= x_hi && !inside; ++xx) {
                    const int c = yy * p.nx + xx;
                    for (unsigned q = start[c]; q < start[c + 1]; ++q) {
                        const int32_t s = sorted[q];
                        if (s == pi || s == ib || s == ic) continue;
                        const double2_t S = ld2(xy, s);
                        // in-circle of S against (P, B, C), the host triangulator's form (csrc/delaunay.cpp)
                        const double ax_ = P.x - S.x, ay_ = P.y - S.y, bx_ = B.x - S.x, by_ = B.y - S.y, fx = C.x - S.x, fy = C.y - S.y;
                        const double ap = ax_ * ax_ + ay_ * ay_, bp = bx_ * bx_ + by_ * by_, cp = fx * fx + fy * fy;
                        const double det = ax_ * (by_ * cp - bp * fy) - ay_ * (bx_ * cp - bp * fx) + ap * (bx_ * fy - by_ * fx);
                        const double perm = (std::fabs(by_ * cp) + std::fabs(bp * fy)) * std::fabs(ax_) +
                                            (std::fabs(bx_ * cp) + std::fabs(bp * fx)) * std::fabs(ay_) +
                                            (std::fabs(bx_ * fy) + std::fabs(by_ * fx)) * ap;
                        if (!(std::fabs(det) > SIGN_MARGIN * perm) || !(std::fabs(det) * jd > set.guard)) {
                            doubt = true;
                            continue;
                        }
                        if (det > 0.0) { inside = true; break; }
                    }
                }
            }
            if (inside) continue;
            if (doubt) { refuse(j, SAME_DD_IN_DOUBT); return; }
            if (count == OWN_CAP) { refuse(j, SAME_DD_OVERFLOW); return; }
            own[3 * count] = (int32_t)pi;
            own[3 * count + 1] = ib;
            own[3 * count + 2] = ic;
            ++count;
        }
    }
    j.own_cnt[pi] = count;
}

// ---- emit: the owners' triangles end to end, in owner order ----------------------------------------------------------------------
__global__ __launch_bounds__(scan::NT) void dd_emit_kernel(Batch<Job> b) {
    __shared__ scan::Shared sh;
    const Job &j = b.w[blockIdx.y];
    if (j.n < 3) return;
    const int64_t n = j.n;
    const int nb = (int)scan::blocks_for(n);
    if ((int)blockIdx.x >= nb) return;
    const unsigned *cnt = j.own_cnt;
    auto val = [&](int64_t i) { return Pair{i < n ? cnt[i] : 0u, 0u}; };
    Pair through;
    const Pair off = scan::exclusive(j.scan_own, (int)blockIdx.x, val, sh, &through);
    const int64_t i = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (i < n) {
        const unsigned c = cnt[i];
        if (c > (unsigned)OWN_CAP || (int64_t)off.a + c > j.cap_out) {
            refuse(j, SAME_DD_OVERFLOW);
        } else {
            const int32_t *src = j.own_tris + i * (int64_t)OWN_CAP * 3;
            int32_t *dst = j.out + 3 * (int64_t)off.a;
            for (unsigned q = 0; q < 3 * c; ++q) dst[q] = src[q];
        }
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) j.st[ST_TRIS] = through.a;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the work buffer of a set of n points: [zeroed head: status words | cell scan words | cell counts | owner counts | owner scan words]
// then parameters, cell offsets, per-point cell / slot / sorted order, per-owner triangles
// (measured without a base, placed with one; answers the length of the head to zero)
size_t lay(Job &j, Carver cv, size_t *total) {
    const int64_t n = j.n;
    j.ncell_cap = 2 * n + 64;
    j.st = cv.take<unsigned long long>(ST_WORDS);
    j.scan_cells = scan::arg(cv.scan_words(j.ncell_cap));
    j.cell_cnt = cv.take<unsigned>((size_t)j.ncell_cap);
    j.own_cnt = cv.take<unsigned>((size_t)n);
    j.scan_own = scan::arg(cv.scan_words(n));
    const size_t zero_bytes = cv.off;
    j.par = cv.take<Par>(1);
    j.cell_start = cv.take<unsigned>((size_t)j.ncell_cap + 1);
    j.cell_of = cv.take<int32_t>((size_t)n);
    j.slot = cv.take<unsigned>((size_t)n);
    j.sorted = cv.take<int32_t>((size_t)n);
    j.own_tris = cv.take<int32_t>((size_t)n * OWN_CAP * 3);
    *total = cv.off;
    return zero_bytes;
}

// the kernels for up to SAME_LAUNCH_WINDOWS sets (heads already zeroed): nine launches
int launch_group(same_ctx *ctx, const Job *jobs, int n_j, Settings set) {
    Batch<Job> b{};
    int64_t max_n = 0, max_cells = 0;
    for (int q = 0; q < n_j; ++q) {
        b.w[q] = jobs[q];
        max_n = std::max(max_n, jobs[q].n);
        max_cells = std::max(max_cells, jobs[q].ncell_cap);
    }
    const unsigned nw = (unsigned)n_j;
    SAME_LAUNCH(ctx, dd_setup_kernel, dim3(1, nw), dim3(256), 0, b, set);
    SAME_LAUNCH(ctx, dd_count_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, b);
    SAME_LAUNCH(ctx, dd_cell_scan_kernel, dim3(scan::blocks_for(max_cells), nw), dim3(scan::NT), 0, b);
    SAME_LAUNCH(ctx, dd_scatter_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, b);
    SAME_LAUNCH(ctx, dd_cell_sort_kernel, dim3(grid_for(max_cells), nw), dim3(256), 0, b);
    SAME_LAUNCH(ctx, dd_hull_kernel, dim3(1, nw), dim3(256), 0, b, set);
    SAME_LAUNCH(ctx, dd_candidate_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, b, set);
    SAME_LAUNCH(ctx, dd_emit_kernel, dim3(scan::blocks_for(max_n), nw), dim3(scan::NT), 0, b);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

bool settings_answerable(double radius, int angle_enabled, double cos_thr) {
    // no angle threshold (or one so small that it bounds nothing): no circumradius bound, no local rule
    return radius > 0.0 && std::isfinite(radius) && angle_enabled && cos_thr == cos_thr && cos_thr < 0.9999;
}

}  // namespace

extern "C" {

int same_window_delaunay(same_window *const *windows, int n_windows, double radius, int angle_enabled, double cos_thr, double guard,
                         int32_t *out_status, int64_t *out_n_tris) {
    same_ctx *ctx = nullptr;
    SAME_TRY(check_batch(windows, n_windows, &ctx));
    REQUIRE(ctx, out_status && out_n_tris && guard >= 0.0);
    for (int i = 0; i < n_windows; ++i) REQUIRE(ctx, windows[i]->may_triangulate() && windows[i]->cur.n_ua < ((int64_t)1 << 30));
    SAME_TRY(same_use(ctx));
    const bool ok = settings_answerable(radius, angle_enabled, cos_thr);
    const Settings set{radius, cos_thr, guard};
    std::vector<Job> jobs;
    std::vector<size_t> zero_bytes;       // of each job's work buffer
    std::vector<int> at((size_t)n_windows, -1);
    for (int i = 0; i < n_windows; ++i) {
        same_window *w = windows[i];
        w->dd_ok = 0;
        w->n_dd = 0;
        out_status[i] = !ok ? SAME_DD_NO_ANGLE : (w->cur.n_ua < 3 ? SAME_DD_FEW_POINTS : 0);
        out_n_tris[i] = 0;
        if (out_status[i]) continue;
        const int64_t n = w->cur.n_ua, cap_out = 2 * n;
        Job jb{};
        jb.xy = w->cur.axy_c;
        jb.n = n;
        jb.cap_out = cap_out;
        size_t total = 0;
        lay(jb, Carver(), &total);
        SAME_TRY(ensure(ctx, w->dd_work, total));
        SAME_TRY(ensure(ctx, w->dd_tris, (size_t)cap_out * 12));
        zero_bytes.push_back(lay(jb, Carver(w->dd_work.p), &total));
        jb.out = static_cast<int32_t *>(w->dd_tris.p);
        at[(size_t)i] = (int)jobs.size();
        jobs.push_back(jb);
    }
    if (jobs.empty()) return SAME_OK;
    int rc = SAME_OK;
    for (size_t g = 0; g < jobs.size() && rc == SAME_OK; g += SAME_LAUNCH_WINDOWS) {
        const int n_g = (int)std::min<size_t>(SAME_LAUNCH_WINDOWS, jobs.size() - g);
        ZeroArgs zr[SAME_LAUNCH_WINDOWS];
        for (int q = 0; q < n_g; ++q) zr[q] = ZeroArgs{{jobs[g + (size_t)q].st, nullptr}, {zero_bytes[g + (size_t)q], 0}};
        rc = launch_zero(ctx, zr, n_g);
        if (rc == SAME_OK) rc = launch_group(ctx, jobs.data() + g, n_g, set);
    }
    // every set's two status words into the context's pinned block: one copy each, ONE wait for the batch
    unsigned long long *h = static_cast<unsigned long long *>(ctx->pinned);
    for (size_t q = 0; q < jobs.size() && rc == SAME_OK; ++q) {
        hipError_t e = hipMemcpyAsync(h + 2 * q, jobs[q].st, 16, hipMemcpyDeviceToHost, ctx->stream);
        ++ctx->stats[SAME_STAT_COPIES];
        if (e != hipSuccess) rc = same_fail(ctx, SAME_EIO, "device triangulation status", e);
    }
    if (rc != SAME_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    SAME_WAIT(ctx);
    for (int i = 0; i < n_windows; ++i) {
        if (at[(size_t)i] < 0) continue;
        const unsigned long long *s = h + 2 * at[(size_t)i];
        same_window *w = windows[i];
        out_status[i] = (int32_t)(s[0] & 0x7fffffffu);
        if (out_status[i] == 0) {
            w->n_dd = (int64_t)s[1];
            w->triangulated();
            out_n_tris[i] = w->n_dd;
        }
    }
    return SAME_OK;
}

int same_delaunay_filtered(same_ctx *ctx, const double *xy, int64_t n, double radius, int angle_enabled, double cos_thr, double guard,
                           int32_t *out_tris, int64_t cap, int64_t *out_n_tris, int32_t *out_status) {
    if (!ctx) return SAME_EINVAL;
    REQUIRE(ctx, (xy || n == 0) && out_n_tris && out_status && n >= 0 && n < ((int64_t)1 << 30) && cap >= 0 && (out_tris || cap == 0) &&
                     guard >= 0.0);
    *out_n_tris = 0;
    *out_status = !settings_answerable(radius, angle_enabled, cos_thr) ? SAME_DD_NO_ANGLE : (n < 3 ? SAME_DD_FEW_POINTS : 0);
    if (*out_status) return SAME_OK;
    SAME_TRY(same_use(ctx));
    double *dxy = nullptr;
    char *work = nullptr;
    int32_t *dout = nullptr;
    Job jb{};
    jb.n = n;
    jb.cap_out = 2 * n;
    size_t total = 0;
    lay(jb, Carver(), &total);
    SAME_TRY(up_as(ctx, SL_AXY, xy, (size_t)n * 2, &dxy));
    SAME_TRY(slot_as(ctx, SL_X, total, &work));
    SAME_TRY(slot_as(ctx, SL_TRIS, (size_t)(2 * n) * 3, &dout));
    const size_t zero_bytes = lay(jb, Carver(work), &total);
    jb.xy = dxy;
    jb.out = dout;
    SAME_FILL(ctx, work, 0, zero_bytes);
    SAME_TRY(launch_group(ctx, &jb, 1, Settings{radius, cos_thr, guard}));
    unsigned long long *h = static_cast<unsigned long long *>(ctx->pinned);
    SAME_COPY(ctx, h, jb.st, 16, hipMemcpyDeviceToHost);
    SAME_WAIT(ctx);
    *out_status = (int32_t)(h[0] & 0x7fffffffu);
    if (*out_status) return SAME_OK;
    const int64_t count = (int64_t)h[1];
    if (count > cap) return SAME_EINVAL;
    if (count) {
        SAME_COPY(ctx, out_tris, dout, (size_t)count * 12, hipMemcpyDeviceToHost);
        SAME_WAIT(ctx);
    }
    *out_n_tris = count;
    return SAME_OK;
}

}  // extern "C"
