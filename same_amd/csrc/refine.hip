// refine.hip -- a local search that lowers a window's full lazy-model objective (src/same.py:1191-1196) from its incumbent:
//
//   sum_p c_p x_p  +  penalty_coeff sum_j p_j  +  no_match_penalty sum_i size_i n_i  +  delaunay_penalty sum_t w_t q_t
//
// over the window's kept aligned cells, their pairs and the kept triangles.  w_t is the size sum of the triangle's corners (:1128-1134);
// q_t = 1 when the lazy body (:645-669) sees t flip: all three corners matched, neither the source nor the reference sign zero, the
// signs different.  Reference j may hold up to limit_j cells (max_matches, or max_matches * the metacell multiplier; at most 1001, the
// bound of p_j); p_j = max(0, count_j - 1).  With every limit 1 (hip_refine="local") the matching stays one-to-one like both starts and
// p_j = 0.  Each reference keeps its count and the sum of its holders' ids, which names THE holder where the count is 1: only such
// references offer a swap partner.
//
// Moves of one cell i, each evaluated exactly against the current state: to a candidate reference with room (count < limit), from
// unmatched to one, to unmatched, and the swap of the references of two matched cells i < k when both crossed pairs are candidates and
// k holds its reference alone, with room or not (the swap belongs to the lower cell; two cells on one reference never swap).  Per
// candidate the move comes before the swap.  A move's delta only
// involves the triangles incident to the cells it moves and the counts of the references it leaves and takes:
//   delta = delaunay_penalty * F + (new cost terms - old cost terms) + penalty_coeff * (dn - do),  F = sum over those triangles of
// +-w_t where q_t changes, dn = 1 when the new reference is held already, do = 1 when the old one is held twice or more (swaps keep
// every count: dn = do = 0) (F first, in the canonical incidence order, exact for integer sizes; one product; then the cost terms; then
// the penalty).  It improves when delta < -2^-40 * scale, scale = delaunay_penalty * (sum of the w_t looked at) + |new terms| +
// |old terms| + penalty_coeff * (dn + do): rounding never counts as an improvement, so the search cannot cycle.
//
// A ROUND: every cell proposes its best improving move (ties: the first in pair order, unmatching before every pair).  Its key is
// (the delta rounded to float, ordered | cell), and it is written by atomicMin to every slot of its FOOTPRINT: the closed 1-ring of every
// cell it moves in the kept-triangle graph, the references it takes and the one it leaves.  A move whose key is the minimum on all of
// them WINS.  Winners share no triangle and no reference, so their deltas add up exactly (each reference's count changes by one move at
// most) and the objective never goes up -- and the apply kernel updates counts with plain stores.  Under limit 1 no other proposal
// claims a held reference but its holder's, so the old slot changes no round's winners.  The smallest key always wins, so a
// round without a winner is a round without an improving move (SETTLED).  The result depends on the input alone -- not on scheduling or
// block shape -- and only on the SET of triangles: each cell's incident triangles are listed by their sorted corner rows and every sign
// and weight is taken over sorted corners.
//
// Kernels over Batch<RefineArgs> (blockIdx.y = window): setup (init, triangles, incidence scan / fill / sort, objective), then per round
// q_t of every triangle, propose, apply; apply's last block closes the round (rounds, moves, settled).  Rounds of a settled window, or one at its cap, return
// at once, so rounds can be enqueued ahead of any look at the device.
#include "refine.h"

namespace {

using namespace devmath;
using namespace win;
using rfn::Prop;
using rfn::RefineArgs;

constexpr unsigned long long NONE = ~0ull;

__device__ __forceinline__ int32_t col_of(const RefineArgs &w, int32_t p) { return w.pairs[2 * (int64_t)p + 1]; }
__device__ __forceinline__ double2_t ref_of(const RefineArgs &w, int32_t p) { return ld2(w.ref_xy, w.ref_row ? w.ref_row[p] : col_of(w, p)); }
__device__ __forceinline__ double unm_of(const RefineArgs &w, int64_t i) { return w.unm ? w.unm[i] : w.penalty * w.size[i]; }
__device__ __forceinline__ bool room(const RefineArgs &w, int32_t j) { return w.count[j] < w.limit[j]; }
__device__ __forceinline__ unsigned long long ld_ctrl(const RefineArgs &w, int q) {
    return __hip_atomic_load(w.ctrl + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool active(const RefineArgs &w) {
    return w.cap > 0 && !ld_ctrl(w, rfn::RC_SETTLED) && (int64_t)ld_ctrl(w, rfn::RC_ROUNDS) < w.cap;
}
__device__ __forceinline__ int64_t n_tris(const RefineArgs &w) { return w.dTr ? (int64_t)*w.dTr : w.cap_tr; }

// q_t under the current matching with cell ci on pair pi and cell ck on pair pk (ci, ck = -1: unchanged)
__device__ __forceinline__ bool flips(const RefineArgs &w, int32_t t, int32_t ci, int32_t pi, int32_t ck, int32_t pk) {
    const int8_t s = w.tsign[t];
    if (s == 0) return false;
    double2_t r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int32_t v = w.tsort[3 * (int64_t)t + q];
        const int32_t p = v == ci ? pi : (v == ck ? pk : w.match[v]);
        if (p < 0) return false;
        r[q] = ref_of(w, p);
    }
    const int8_t rs = orient_sign(r[0], r[1], r[2]);
    return rs != 0 && rs != s;
}
__device__ __forceinline__ bool has_corner(const RefineArgs &w, int32_t t, int32_t v) {
    const int32_t *c = w.tsort + 3 * (int64_t)t;
    return c[0] == v || c[1] == v || c[2] == v;
}
// the flip part over the triangles of cell c (skipping those with corner `skip`), with ci -> pi and ck -> pk
__device__ __forceinline__ void flip_part(const RefineArgs &w, int32_t c, int32_t skip, int32_t ci, int32_t pi, int32_t ck, int32_t pk,
                                          double &F, double &W) {
    for (int32_t q = w.off[c]; q < w.off[c + 1]; ++q) {
        const int32_t t = w.inc[q];
        if (skip >= 0 && has_corner(w, t, skip)) continue;
        const double wt = w.tw[t];
        W += wt;
        const bool o = w.q[t] != 0, nw = flips(w, t, ci, pi, ck, pk);
        if (o != nw) F += nw ? wt : -wt;
    }
}
struct Delta {
    double d, scale;
};
// cell i from its pair to pair pn (-1 = unmatched); the penalty terms are 0.0 under limit 1, and adding them keeps every bit
__device__ __forceinline__ Delta delta_single(const RefineArgs &w, int32_t i, int32_t pn) {
    double F = 0.0, W = 0.0;
    flip_part(w, i, -1, i, pn, -1, 0, F, W);
    const int32_t po = w.match[i];
    const double nw = pn >= 0 ? w.cost[pn] : unm_of(w, i), old = po >= 0 ? w.cost[po] : unm_of(w, i);
    const int dn = pn >= 0 && w.count[col_of(w, pn)] >= 1, dold = po >= 0 && w.count[col_of(w, po)] >= 2;
    return Delta{w.dp * F + (nw - old) + w.pc * (double)(dn - dold), w.dp * W + (fabs(nw) + fabs(old)) + w.pc * (double)(dn + dold)};
}
// cells i < k exchange their references: i to pair pi, k to pair pk
__device__ __forceinline__ Delta delta_swap(const RefineArgs &w, int32_t i, int32_t pi, int32_t k, int32_t pk) {
    double F = 0.0, W = 0.0;
    flip_part(w, i, -1, i, pi, k, pk, F, W);
    flip_part(w, k, i, i, pi, k, pk, F, W);
    const double nw = w.cost[pi] + w.cost[pk], old = w.cost[w.match[i]] + w.cost[w.match[k]];
    return Delta{w.dp * F + (nw - old), w.dp * W + (fabs(nw) + fabs(old))};
}
__device__ __forceinline__ bool improves(Delta x) { return x.d < -rfn::EPS * x.scale; }
// (delta rounded to float, as an ordered 32-bit word | cell): round-to-nearest is monotone, the cell makes every key distinct
__device__ __forceinline__ unsigned long long key_of(double d, int32_t i) {
    const unsigned u = __float_as_uint((float)d);
    const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned)i;
}

// every slot of a proposal's footprint: f(slot index) for cells (closed 1-rings of the moved cells) and references (n + column)
template <class Fn>
__device__ __forceinline__ bool each_slot(const RefineArgs &w, int32_t i, const Prop &pr, Fn f) {
    bool all = f((int64_t)i);
    for (int32_t q = w.off[i]; q < w.off[i + 1]; ++q) {
        const int32_t *c = w.tsort + 3 * (int64_t)w.inc[q];
        all &= f(c[0]);
        all &= f(c[1]);
        all &= f(c[2]);
    }
    if (pr.k >= 0) {
        all &= f((int64_t)pr.k);
        for (int32_t q = w.off[pr.k]; q < w.off[pr.k + 1]; ++q) {
            const int32_t *c = w.tsort + 3 * (int64_t)w.inc[q];
            all &= f(c[0]);
            all &= f(c[1]);
            all &= f(c[2]);
        }
        all &= f(w.n + col_of(w, pr.p_k));
    }
    if (pr.p_i >= 0) all &= f(w.n + col_of(w, pr.p_i));
    if (pr.k < 0 && pr.p_o >= 0) all &= f(w.n + col_of(w, pr.p_o));
    return all;
}

// ---- setup ---------------------------------------------------------------------------------------------------------------------
// the window path's limits (src/helpers.py:102-161) over the frame of the references its pairs name: one block per window
constexpr int LIM_NT = 1024;
__global__ __launch_bounds__(LIM_NT) void refine_limit_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    if (!w.rsize) return;
    double mx = 0.0;
    bool meta = false;
    const int32_t *__restrict__ frame = w.lim_row ? w.lim_row : w.ref_row;
    const int64_t n_frame = w.lim_row ? w.lim_P : w.P;
    for (int64_t p = threadIdx.x; p < n_frame; p += LIM_NT) {
        const double s = w.rsize[frame[p]];
        meta = meta || s > 1.0;
        mx = fmax(mx, s);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
    const bool any_meta = __syncthreads_or(meta);
    __shared__ double pm[LIM_NT / 64];
    if ((threadIdx.x & 63) == 0) pm[threadIdx.x >> 6] = mx;
    __syncthreads();
    double mult = (double)w.multiplier;
    if (w.multiplier <= 0) {          // None: int(max size) over the frame
        mult = 0.0;
        for (int q = 0; q < LIM_NT / 64; ++q) mult = fmax(mult, pm[q]);
        mult = trunc(mult);
    }
    // every product is of integers; it is compared with MAX_LIMIT, so fp64 is exact wherever it matters
    const double big = fmin(mult * (double)w.max_matches, (double)rfn::MAX_LIMIT);
    const int32_t plain = (int32_t)std::min<int64_t>(w.max_matches, rfn::MAX_LIMIT);
    for (int64_t j = threadIdx.x; j < w.n_r; j += LIM_NT)
        w.limit[j] = any_meta && w.rsize[w.ref_rows[j]] > 1.0 ? (int32_t)big : plain;
}
// the matching from the start, counters and claim slots cleared, no reference held (the limits: given or 1, unless the window's)
__global__ __launch_bounds__(256) void refine_init_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < w.n) {
        w.match[x] = w.start[x];
        w.deg[x] = 0;
        w.cur[x] = 0;
    }
    if (x < w.n_r) {
        w.count[x] = 0;
        w.hsum[x] = 0;
        if (!w.rsize) w.limit[x] = w.limit_in ? w.limit_in[x] : 1;
    }
    if (x < w.n + w.n_r) w.slot[0][x] = w.slot[1][x] = NONE;
    if (x < (int64_t)scan::blocks_for(w.n)) w.st[x] = 0;
    if (x < rfn::RC_COUNT) w.ctrl[x] = 0;
}
// per triangle: corners sorted, sign and weight over them, degrees; per cell: the reference it holds
__global__ __launch_bounds__(256) void refine_tri_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < w.n && w.match[x] >= 0) {
        const int32_t j = col_of(w, w.match[x]);
        atomicAdd(&w.count[j], 1);
        atomicAdd(reinterpret_cast<unsigned long long *>(&w.hsum[j]), (unsigned long long)x);
    }
    if (x >= n_tris(w)) return;
    int32_t a = w.tris[3 * x], c1 = w.tris[3 * x + 1], c2 = w.tris[3 * x + 2], t;
    if (a > c1) { t = a; a = c1; c1 = t; }
    if (c1 > c2) { t = c1; c1 = c2; c2 = t; }
    if (a > c1) { t = a; a = c1; c1 = t; }
    w.tsort[3 * x] = a;
    w.tsort[3 * x + 1] = c1;
    w.tsort[3 * x + 2] = c2;
    w.tsign[x] = orient_sign(ld2(w.axy, a), ld2(w.axy, c1), ld2(w.axy, c2));
    w.tw[x] = w.size[a] + w.size[c1] + w.size[c2];
    atomicAdd(&w.deg[a], 1u);
    atomicAdd(&w.deg[c1], 1u);
    atomicAdd(&w.deg[c2], 1u);
}
__global__ __launch_bounds__(scan::NT) void refine_scan_kernel(Batch<RefineArgs> b) {
    __shared__ scan::Shared sh;
    const RefineArgs &w = b.w[blockIdx.y];
    const int nb = (int)scan::blocks_for(w.n);
    if ((int)blockIdx.x >= nb) return;
    const int64_t n = w.n;
    auto val = [&](int64_t i) { return scan::Pair{i < n ? w.deg[i] : 0u, 0u}; };
    scan::Pair through;
    const scan::Pair off = scan::exclusive(w.st, (int)blockIdx.x, val, sh, &through);
    const int64_t i = (int64_t)blockIdx.x * scan::NT + threadIdx.x;
    if (i < n) w.off[i] = (int32_t)off.a;
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) w.off[n] = (int32_t)through.a;
}
__global__ __launch_bounds__(256) void refine_fill_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tris(w)) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int32_t v = w.tsort[3 * t + q];
        w.inc[w.off[v] + (int32_t)atomicAdd(&w.cur[v], 1u)] = (int32_t)t;
    }
}
// each cell's incident triangles in the order of their sorted corner rows (distinct triangles: distinct keys)
__device__ __forceinline__ bool tri_less(const RefineArgs &w, int32_t s, int32_t t) {
    const int32_t *a = w.tsort + 3 * (int64_t)s, *c = w.tsort + 3 * (int64_t)t;
    if (a[0] != c[0]) return a[0] < c[0];
    if (a[1] != c[1]) return a[1] < c[1];
    if (a[2] != c[2]) return a[2] < c[2];
    return s < t;
}
__global__ __launch_bounds__(256) void refine_sort_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n) return;
    int32_t *l = w.inc + w.off[i];
    const int32_t d = w.off[i + 1] - w.off[i];
    for (int32_t q = 1; q < d; ++q) {
        const int32_t t = l[q];
        int32_t r = q - 1;
        while (r >= 0 && tri_less(w, t, l[r])) {
            l[r + 1] = l[r];
            --r;
        }
        l[r + 1] = t;
    }
}
// the objective of the current matching: one block of OBJ_NT per window, a fixed reduction order
constexpr int OBJ_NT = 1024;
__global__ __launch_bounds__(OBJ_NT) void refine_objective_kernel(Batch<RefineArgs> b, int which) {
    const RefineArgs &w = b.w[blockIdx.y];
    double c = 0.0, f = 0.0;
    unsigned long long e = 0;
    for (int64_t i = threadIdx.x; i < w.n; i += OBJ_NT) c += w.match[i] >= 0 ? w.cost[w.match[i]] : unm_of(w, i);
    const int64_t Tr = n_tris(w);
    for (int64_t t = threadIdx.x; t < Tr; t += OBJ_NT)
        if (flips(w, (int32_t)t, -1, 0, -1, 0)) f += w.tw[t];
    for (int64_t j = threadIdx.x; j < w.n_r; j += OBJ_NT)
        if (w.count[j] > 1) e += (unsigned long long)(w.count[j] - 1);
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_down(c, o, 64);
        f += __shfl_down(f, o, 64);
        e += __shfl_down(e, o, 64);
    }
    __shared__ double pc[OBJ_NT / 64], pf[OBJ_NT / 64];
    __shared__ unsigned long long pe[OBJ_NT / 64];
    if ((threadIdx.x & 63) == 0) {
        pc[threadIdx.x >> 6] = c;
        pf[threadIdx.x >> 6] = f;
        pe[threadIdx.x >> 6] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double cs = 0.0, fs = 0.0;
        unsigned long long es = 0;
        for (int q = 0; q < OBJ_NT / 64; ++q) {
            cs += pc[q];
            fs += pf[q];
            es += pe[q];
        }
        double obj = cs + w.dp * fs;
        if (es) obj += w.pc * (double)es;      // last: a one-to-one matching's objective keeps its bits
        w.ctrl[which] = (unsigned long long)__double_as_longlong(obj);
        w.ctrl[rfn::RC_EXTRA] = es;
    }
}

// ---- rounds ---------------------------------------------------------------------------------------------------------------------
// q_t of every triangle under the matching the round starts from
__global__ __launch_bounds__(256) void refine_flag_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= n_tris(w) || !active(w)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_tris(w)) w.q[t] = flips(w, (int32_t)t, -1, 0, -1, 0);
}
__global__ __launch_bounds__(256) void refine_propose_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    if ((int64_t)blockIdx.x * blockDim.x >= w.n || !active(w)) return;
    const int32_t i = (int32_t)((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= w.n) return;
    Prop best{NONE, -1, -1, -1, -1};
    double bd = 0.0;
    bool found = false;
    const int32_t po = w.match[i];
    auto consider = [&](Delta x, int32_t pn, int32_t k, int32_t pk) {
        if (!improves(x) || (found && !(x.d < bd))) return;
        found = true;
        bd = x.d;
        best.p_i = pn;
        best.k = k;
        best.p_k = pk;
    };
    if (po >= 0) consider(delta_single(w, i, -1), -1, -1, -1);
    const int32_t jo = po >= 0 ? col_of(w, po) : -1;
    for (int32_t p = w.prow[i]; p < w.prow[i + 1]; ++p) {
        if (p == po) continue;
        const int32_t j = col_of(w, p);
        if (room(w, j)) consider(delta_single(w, i, p), p, -1, -1);
        if (po >= 0 && w.count[j] == 1 && w.hsum[j] > i && j != jo) {      // (limit 1: only where there is no room)
            const int32_t o = (int32_t)w.hsum[j];
            for (int32_t q = w.prow[o]; q < w.prow[o + 1]; ++q)
                if (col_of(w, q) == jo) {
                    consider(delta_swap(w, i, p, o, q), p, o, q);
                    break;
                }
        }
    }
    if (found) {
        best.key = key_of(bd, i);
        best.p_o = po;
        unsigned long long *s = w.slot[ld_ctrl(w, rfn::RC_ROUNDS) & 1];
        each_slot(w, i, best, [&](int64_t x) { atomicMin(&s[x], best.key); return true; });
    }
    w.best[i] = best;
}
// winners (their key is the minimum on every slot of their footprint) applied; the other parity's slots cleared for the next round;
// the last block of the window closes the round
__global__ __launch_bounds__(256) void refine_apply_kernel(Batch<RefineArgs> b) {
    const RefineArgs &w = b.w[blockIdx.y];
    const int64_t ns = w.n + w.n_r;
    const unsigned nb = (unsigned)((ns + 255) / 256);        // the window's own blocks (launch: grid_for of the largest)
    if (blockIdx.x >= nb || !active(w)) return;
    const unsigned long long par = ld_ctrl(w, rfn::RC_ROUNDS) & 1;
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool won = false;
    if (x < w.n) {
        const int32_t i = (int32_t)x;
        const Prop pr = w.best[i];
        if (pr.key != NONE) {
            const unsigned long long *s = w.slot[par];
            won = each_slot(w, i, pr, [&](int64_t y) { return s[y] == pr.key; });
            if (won) {         // winners share no reference: plain stores
                if (pr.k >= 0) {
                    const int32_t ji = col_of(w, pr.p_i), jk = col_of(w, pr.p_k);
                    w.match[i] = pr.p_i;
                    w.match[pr.k] = pr.p_k;
                    w.hsum[ji] += (long long)i - pr.k;
                    w.hsum[jk] += (long long)pr.k - i;
                } else {
                    if (pr.p_o >= 0) {
                        const int32_t jo = col_of(w, pr.p_o);
                        w.count[jo] -= 1;
                        w.hsum[jo] -= i;
                    }
                    if (pr.p_i >= 0) {
                        const int32_t jn = col_of(w, pr.p_i);
                        w.count[jn] += 1;
                        w.hsum[jn] += i;
                    }
                    w.match[i] = pr.p_i;
                }
            }
        }
    }
    if (x < ns) w.slot[par ^ 1][x] = NONE;
    const unsigned long long bal = __ballot(won);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&w.ctrl[rfn::RC_WIN], (unsigned long long)__builtin_popcountll(bal));
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&w.ctrl[rfn::RC_DONE], 1ull) == nb - 1) {
            __threadfence();
            const unsigned long long win = atomicAdd(&w.ctrl[rfn::RC_WIN], 0ull);
            if (win) {
                w.ctrl[rfn::RC_ROUNDS] += 1;
                w.ctrl[rfn::RC_MOVES] += win;
            } else {
                w.ctrl[rfn::RC_SETTLED] = 1;
            }
            w.ctrl[rfn::RC_WIN] = 0;
            w.ctrl[rfn::RC_DONE] = 0;
        }
    }
}

}  // namespace

namespace rfn {

void lay(RefineArgs &a, Carver &cv) {
    // every array holds one element at least (asg::lay sizes by the counts themselves)
    const size_t N = (size_t)std::max<int64_t>(a.n, 1), R = (size_t)std::max<int64_t>(a.n_r, 1), T = (size_t)std::max<int64_t>(a.cap_tr, 1);
    a.match = cv.take<int32_t>(N);
    a.count = cv.take<int32_t>(R);
    a.hsum = cv.take<long long>(R);
    a.limit = cv.take<int32_t>(R);
    a.tsort = cv.take<int32_t>(T * 3);
    a.tsign = cv.take<int8_t>(T);
    a.tw = cv.take<double>(T);
    a.q = cv.take<uint8_t>(T);
    a.deg = cv.take<unsigned>(N);
    a.cur = cv.take<unsigned>(N);
    a.off = cv.take<int32_t>(N + 1);
    a.inc = cv.take<int32_t>(T * 3);
    a.st = cv.scan_words(a.n);
    a.slot[0] = cv.take<unsigned long long>(N + R);
    a.slot[1] = cv.take<unsigned long long>(N + R);
    a.best = cv.take<Prop>(N);
}

static Batch<RefineArgs> batch_of(const RefineArgs *jobs, int n_w, int64_t *max_n, int64_t *max_s, int64_t *max_t) {
    Batch<RefineArgs> bt{};
    *max_n = *max_s = *max_t = 0;
    for (int q = 0; q < n_w; ++q) {
        bt.w[q] = jobs[q];
        *max_n = std::max(*max_n, jobs[q].n);
        *max_s = std::max(*max_s, jobs[q].n + jobs[q].n_r);
        *max_t = std::max(*max_t, jobs[q].cap_tr);
    }
    return bt;
}

int launch_limits(same_ctx *ctx, const RefineArgs *jobs, int n_w) {
    if (n_w <= 0) return SAME_OK;
    Batch<RefineArgs> bt{};
    for (int q = 0; q < n_w; ++q) bt.w[q] = jobs[q];
    SAME_LAUNCH(ctx, refine_limit_kernel, dim3(1, (unsigned)n_w), dim3(LIM_NT), 0, bt);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

int launch_setup(same_ctx *ctx, const RefineArgs *jobs, int n_w) {
    if (n_w <= 0) return SAME_OK;
    int64_t max_n, max_s, max_t;
    const Batch<RefineArgs> bt = batch_of(jobs, n_w, &max_n, &max_s, &max_t);
    const unsigned nw = (unsigned)n_w;
    bool by_frame = false;
    for (int q = 0; q < n_w; ++q) by_frame = by_frame || jobs[q].rsize;
    if (by_frame) SAME_LAUNCH(ctx, refine_limit_kernel, dim3(1, nw), dim3(LIM_NT), 0, bt);
    SAME_LAUNCH(ctx, refine_init_kernel, dim3(grid_for(std::max<int64_t>(max_s, 64)), nw), dim3(256), 0, bt);
    SAME_LAUNCH(ctx, refine_tri_kernel, dim3(grid_for(std::max(max_t, max_n)), nw), dim3(256), 0, bt);
    SAME_LAUNCH(ctx, refine_scan_kernel, dim3(scan::blocks_for(max_n), nw), dim3(scan::NT), 0, bt);
    SAME_LAUNCH(ctx, refine_fill_kernel, dim3(grid_for(max_t), nw), dim3(256), 0, bt);
    SAME_LAUNCH(ctx, refine_sort_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, bt);
    SAME_LAUNCH(ctx, refine_objective_kernel, dim3(1, nw), dim3(OBJ_NT), 0, bt, (int)RC_OBJ0);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

int launch_rounds(same_ctx *ctx, const RefineArgs *jobs, int n_w, int rounds) {
    if (n_w <= 0) return SAME_OK;
    int64_t max_n, max_s, max_t;
    const Batch<RefineArgs> bt = batch_of(jobs, n_w, &max_n, &max_s, &max_t);
    const unsigned nw = (unsigned)n_w;
    for (int r = 0; r < rounds; ++r) {
        SAME_LAUNCH(ctx, refine_flag_kernel, dim3(grid_for(max_t), nw), dim3(256), 0, bt);
        SAME_LAUNCH(ctx, refine_propose_kernel, dim3(grid_for(max_n), nw), dim3(256), 0, bt);
        SAME_LAUNCH(ctx, refine_apply_kernel, dim3(grid_for(max_s), nw), dim3(256), 0, bt);
    }
    SAME_LAUNCH(ctx, refine_objective_kernel, dim3(1, nw), dim3(OBJ_NT), 0, bt, (int)RC_OBJ);
    HIP_TRY(ctx, hipGetLastError());
    return SAME_OK;
}

}  // namespace rfn

// ---- the host-buffer form ------------------------------------------------------------------------------------------------------
// ref_limit null: every limit 1 (same_refine_matching); out_stats gets Σ p_j as a sixth word when `extra`
static int refine_host(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m, int64_t n_r,
                       const int32_t *tris, int64_t Tr, const double *axy, const double *ref_xy, const double *size, double delaunay_penalty,
                       const int32_t *ref_limit, double penalty_coeff, int64_t rounds_cap, int32_t *match_pair_inout, int64_t *out_stats,
                       bool extra) {
    REQUIRE(ctx, ctx != nullptr);
    REQUIRE(ctx, P >= 0 && n_m >= 0 && n_r >= 0 && Tr >= 0 && n_m + n_r < ((int64_t)1 << 30) && P < ((int64_t)1 << 31) - 1 &&
                     Tr < ((int64_t)1 << 29));
    REQUIRE(ctx, (P == 0 || (pairs && costs)) && (n_m == 0 || (unmatched && match_pair_inout && axy && size)) && (n_r == 0 || ref_xy) &&
                     (Tr == 0 || tris) && out_stats);
    REQUIRE(ctx, rounds_cap >= 1 && delaunay_penalty >= 0.0 && delaunay_penalty - delaunay_penalty == 0.0);
    REQUIRE(ctx, penalty_coeff >= 0.0 && penalty_coeff - penalty_coeff == 0.0);
    if (ref_limit)
        for (int64_t j = 0; j < n_r; ++j) REQUIRE(ctx, ref_limit[j] >= 1 && ref_limit[j] <= rfn::MAX_LIMIT);
    // the pairs by row (stable: the caller's order inside a row), each (row, column) once; the start within the limits
    same_pair_csr by_row;
    SAME_TRY(same_pairs_by_row(ctx, pairs, costs, P, n_m, n_r, &by_row));
    const std::vector<int32_t> &order = by_row.order, &where = by_row.where;
    std::vector<int32_t> start((size_t)n_m);
    std::vector<int32_t> held((size_t)n_r, 0);
    for (int64_t i = 0; i < n_m; ++i) {
        const int32_t p = match_pair_inout[i];
        REQUIRE(ctx, p >= -1 && p < P && (p < 0 || pairs[2 * (int64_t)p] == i));
        if (p >= 0) {
            const int32_t j = pairs[2 * (int64_t)p + 1];
            if (++held[(size_t)j] > (ref_limit ? ref_limit[j] : 1)) {
                ctx->err = ref_limit ? "invalid argument: the start matching takes a reference more often than its limit"
                                     : "invalid argument: the start matching takes a reference twice";
                return SAME_EINVAL;
            }
        }
        start[(size_t)i] = p >= 0 ? where[(size_t)p] : -1;
    }
    SAME_TRY(check_index_range(ctx, tris, Tr * 3, 0, n_m, "triangles"));
    SAME_TRY(same_use(ctx));
    rfn::RefineArgs a{};
    a.dp = delaunay_penalty;
    a.n = n_m;
    a.n_r = n_r;
    a.cap_tr = Tr;
    a.cap = rounds_cap;
    a.pc = penalty_coeff;
    int32_t *d_prow, *d_pairs, *d_tris, *d_start, *d_lim;
    double *d_cost, *d_unm, *d_size, *d_axy, *d_rxy;
    auto lay = [&](Carver cv) {       // (one element more than each input: no array is empty)
        a.prow = d_prow = cv.take<int32_t>((size_t)n_m + 1);
        a.pairs = d_pairs = cv.take<int32_t>((size_t)P * 2 + 2);
        a.cost = d_cost = cv.take<double>((size_t)P + 1);
        a.unm = d_unm = cv.take<double>((size_t)n_m + 1);
        a.size = d_size = cv.take<double>((size_t)n_m + 1);
        a.axy = d_axy = cv.take<double>((size_t)n_m * 2 + 2);
        a.ref_xy = d_rxy = cv.take<double>((size_t)n_r * 2 + 2);
        a.tris = d_tris = cv.take<int32_t>((size_t)Tr * 3 + 3);
        a.start = d_start = cv.take<int32_t>((size_t)n_m + 1);
        a.ctrl = cv.take<unsigned long long>(rfn::RC_COUNT);
        d_lim = cv.take<int32_t>((size_t)n_r + 1);
        a.limit_in = ref_limit ? d_lim : nullptr;
        rfn::lay(a, cv);
        return cv.off;
    };
    char *d = nullptr;
    SAME_TRY(slot_as(ctx, SL_OUT0, lay(Carver()), &d));
    lay(Carver(d));
    SAME_COPY(ctx, d_prow, by_row.prow.data(), by_row.prow.size() * 4, hipMemcpyHostToDevice);
    if (P) {
        SAME_COPY(ctx, d_pairs, by_row.csr.data(), (size_t)P * 8, hipMemcpyHostToDevice);
        SAME_COPY(ctx, d_cost, by_row.ccsr.data(), (size_t)P * 8, hipMemcpyHostToDevice);
    }
    if (n_m) {
        SAME_COPY(ctx, d_unm, unmatched, (size_t)n_m * 8, hipMemcpyHostToDevice);
        SAME_COPY(ctx, d_size, size, (size_t)n_m * 8, hipMemcpyHostToDevice);
        SAME_COPY(ctx, d_axy, axy, (size_t)n_m * 16, hipMemcpyHostToDevice);
        SAME_COPY(ctx, d_start, start.data(), (size_t)n_m * 4, hipMemcpyHostToDevice);
    }
    if (n_r) SAME_COPY(ctx, d_rxy, ref_xy, (size_t)n_r * 16, hipMemcpyHostToDevice);
    if (n_r && ref_limit) SAME_COPY(ctx, d_lim, ref_limit, (size_t)n_r * 4, hipMemcpyHostToDevice);
    if (Tr) SAME_COPY(ctx, d_tris, tris, (size_t)Tr * 12, hipMemcpyHostToDevice);
    std::vector<int32_t> mp((size_t)n_m);
    unsigned long long ctrl[rfn::RC_COUNT] = {};
    if (n_m) {
        SAME_TRY(rfn::launch_setup(ctx, &a, 1));
        // rounds in growing chunks up to the cap (every enqueued round of a live search either applies moves or settles it); one wait
        // unless the search is still moving after the first chunk
        int64_t chunk = std::min<int64_t>(rfn::FIRST_ROUNDS * 4, rounds_cap);
        for (;;) {
            SAME_TRY(rfn::launch_rounds(ctx, &a, 1, (int)chunk));
            SAME_COPY(ctx, ctrl, a.ctrl, sizeof ctrl, hipMemcpyDeviceToHost);
            SAME_COPY(ctx, mp.data(), a.match, (size_t)n_m * 4, hipMemcpyDeviceToHost);
            SAME_WAIT(ctx);
            if (ctrl[rfn::RC_SETTLED] || (int64_t)ctrl[rfn::RC_ROUNDS] >= rounds_cap) break;
            chunk = std::min<int64_t>(chunk * 2, rounds_cap - (int64_t)ctrl[rfn::RC_ROUNDS]);
        }
    }
    for (int64_t i = 0; i < n_m; ++i) match_pair_inout[i] = mp[(size_t)i] >= 0 ? order[(size_t)mp[(size_t)i]] : -1;
    out_stats[0] = (int64_t)ctrl[rfn::RC_ROUNDS];
    out_stats[1] = (int64_t)ctrl[rfn::RC_MOVES];
    out_stats[2] = (int64_t)ctrl[rfn::RC_SETTLED];
    out_stats[3] = (int64_t)ctrl[rfn::RC_OBJ0];
    out_stats[4] = (int64_t)ctrl[rfn::RC_OBJ];
    if (extra) out_stats[5] = (int64_t)ctrl[rfn::RC_EXTRA];
    return SAME_OK;
}

extern "C" int same_refine_matching(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                                    int64_t n_r, const int32_t *tris, int64_t Tr, const double *axy, const double *ref_xy, const double *size,
                                    double delaunay_penalty, int64_t rounds_cap, int32_t *match_pair_inout, int64_t *out_stats) {
    return refine_host(ctx, pairs, costs, P, unmatched, n_m, n_r, tris, Tr, axy, ref_xy, size, delaunay_penalty, nullptr, 0.0, rounds_cap,
                       match_pair_inout, out_stats, false);
}

extern "C" int same_refine_matching_cap(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched,
                                        int64_t n_m, int64_t n_r, const int32_t *tris, int64_t Tr, const double *axy, const double *ref_xy,
                                        const double *size, double delaunay_penalty, const int32_t *ref_limit, double penalty_coeff,
                                        int64_t rounds_cap, int32_t *match_pair_inout, int64_t *out_stats) {
    REQUIRE(ctx, n_r == 0 || ref_limit);
    return refine_host(ctx, pairs, costs, P, unmatched, n_m, n_r, tris, Tr, axy, ref_xy, size, delaunay_penalty, ref_limit, penalty_coeff,
                       rounds_cap, match_pair_inout, out_stats, true);
}
