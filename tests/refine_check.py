"""Host statement of the window path's local search (same_amd/csrc/refine.hip), for the tests only: the product has no CPU fallback.

The objective is the lazy model's (src/same.py:1191-1196) on a window's kept aligned cells, their pairs and the kept triangles:

    sum_p c_p x_p + penalty_coeff sum_j p_j + no_match_penalty sum_i size_i n_i + delaunay_penalty sum_t w_t q_t

with w_t the size sum of the triangle's corners (:1128-1134) and q_t = 1 when the lazy body (:645-669) sees triangle t flip: all three
corners matched (:649-650), neither the source sign (:1146) nor the reference sign (:658) zero (:663-664), the signs different
(:666-669).  The matching stays one-to-one, so p_j = 0.  `unmatched[i]` is the no-match cost no_match_penalty * size_i.

A round, as the device runs it:
  * every cell i proposes its best improving move against the current state -- to unmatched (first), then, in pair order, each candidate
    pair p != its own: to p when p's reference is free; a swap with the reference's holder k when i is matched, i < k and k has a pair
    to i's reference.  delta = delaunay_penalty * F + (new cost terms - old cost terms), F = the +-w_t of the incident triangles (of i,
    then of k without those of i) whose q_t changes, in the order of their sorted corners; a move improves when
    delta < -2^-40 * scale, scale = delaunay_penalty * (sum of those w_t) + |new terms| + |old terms|.  Ties: the first candidate.
  * its key is (float32(delta) as an ordered word, i); it claims every slot of its footprint (the closed 1-rings of the moved cells, the
    references it takes) by minimum; a move that holds all of them wins.  Winners are applied together; a round with no winner settles
    the search, `rounds_cap` productive rounds end it.
Signs and weights are taken over each triangle's sorted corners, so only the triangle SET matters.
"""
import numpy as np

EPS = 2.0 ** -40


def _orient(a, b, c):
    v = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (v > 0.0) - (v < 0.0)


def _key(delta, i):
    u = int(np.array([delta], dtype=np.float32).view(np.uint32)[0])
    o = (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)
    return (o << 32) | i


class Problem:
    """one window: pairs (P, 2) (cell, reference), costs (P,), unmatched (n,), triangles (T, 3), axy (n, 2), ref_xy (n_r, 2), size (n,)"""

    def __init__(self, pairs, costs, unmatched, n, n_r, triangles, axy, ref_xy, size, delaunay_penalty):
        self.pairs = [(int(i), int(j)) for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)]
        self.cost = [float(c) for c in np.asarray(costs, dtype=np.float64)]
        self.unm = [float(u) for u in np.asarray(unmatched, dtype=np.float64)]
        self.n, self.n_r, self.dp = int(n), int(n_r), float(delaunay_penalty)
        self.axy = [tuple(map(float, p)) for p in np.asarray(axy, dtype=np.float64).reshape(-1, 2)]
        self.rxy = [tuple(map(float, p)) for p in np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)]
        self.size = [float(s) for s in np.asarray(size, dtype=np.float64)]
        self.rows = [[] for _ in range(self.n)]          # pairs of each cell in pair order
        for p, (i, _j) in enumerate(self.pairs):
            self.rows[i].append(p)
        self.tris = [tuple(sorted(int(v) for v in t)) for t in np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
        self.sign = [_orient(self.axy[a], self.axy[b], self.axy[c]) for a, b, c in self.tris]
        self.w = [self.size[a] + self.size[b] + self.size[c] for a, b, c in self.tris]
        inc = [[] for _ in range(self.n)]
        for t, tri in enumerate(self.tris):
            for v in tri:
                inc[v].append(t)
        self.inc = [sorted(l, key=lambda t: (self.tris[t], t)) for l in inc]

    def col(self, p):
        return self.pairs[p][1]

    def flips(self, t, m, change=()):
        if self.sign[t] == 0:
            return False
        ch = dict(change)
        r = []
        for v in self.tris[t]:
            p = ch.get(v, m[v])
            if p < 0:
                return False
            r.append(self.rxy[self.col(p)])
        rs = _orient(*r)
        return rs != 0 and rs != self.sign[t]

    def term(self, i, p):
        return self.cost[p] if p >= 0 else self.unm[i]

    def _flip_part(self, m, cells, change):
        F = W = 0.0
        for q, c in enumerate(cells):
            for t in self.inc[c]:
                if any(prev in self.tris[t] for prev in cells[:q]):
                    continue
                W += self.w[t]
                o, nw = self.flips(t, m), self.flips(t, m, change)
                if o != nw:
                    F += self.w[t] if nw else -self.w[t]
        return F, W

    def delta_single(self, m, i, pn):
        F, W = self._flip_part(m, [i], ((i, pn),))
        nw, old = self.term(i, pn), self.term(i, m[i])
        return self.dp * F + (nw - old), self.dp * W + (abs(nw) + abs(old))

    def delta_swap(self, m, i, pi, k, pk):
        F, W = self._flip_part(m, [i, k], ((i, pi), (k, pk)))
        nw, old = self.cost[pi] + self.cost[pk], self.cost[m[i]] + self.cost[m[k]]
        return self.dp * F + (nw - old), self.dp * W + (abs(nw) + abs(old))

    def moves(self, m, owner, i):
        """every candidate move of cell i in the order it is considered: (delta, scale, new pair, partner, partner's new pair)"""
        out = []
        po = m[i]
        if po >= 0:
            out.append((*self.delta_single(m, i, -1), -1, -1, -1))
        for p in self.rows[i]:
            if p == po:
                continue
            o = owner[self.col(p)]
            if o < 0:
                out.append((*self.delta_single(m, i, p), p, -1, -1))
            elif po >= 0 and o > i:
                q = next((q for q in self.rows[o] if self.col(q) == self.col(po)), None)
                if q is not None:
                    out.append((*self.delta_swap(m, i, p, o, q), p, o, q))
        return out

    def best(self, m, owner, i):
        best = None
        for d, s, pn, k, pk in self.moves(m, owner, i):
            if d < -EPS * s and (best is None or d < best[0]):
                best = (d, pn, k, pk)
        return best

    def footprint(self, i, pn, k, pk):
        cells = {i} | {v for t in self.inc[i] for v in self.tris[t]}
        refs = set()
        if k >= 0:
            cells |= {k} | {v for t in self.inc[k] for v in self.tris[t]}
            refs.add(self.col(pk))
        if pn >= 0:
            refs.add(self.col(pn))
        return [("c", c) for c in cells] + [("r", j) for j in refs]

    def objective(self, m):
        c = sum(self.term(i, m[i]) for i in range(self.n))
        f = sum(self.w[t] for t in range(len(self.tris)) if self.flips(t, m))
        return c + self.dp * f

    def owners(self, m):
        owner = [-1] * self.n_r
        for i, p in enumerate(m):
            if p >= 0:
                assert owner[self.col(p)] < 0, "the matching takes a reference twice"
                owner[self.col(p)] = i
        return owner


def refine(prob, match_pair, rounds_cap):
    """-> (match_pair, {"rounds", "moves", "settled", "objective_start", "objective", "trace": objective after every round})"""
    m = [int(p) for p in match_pair]
    owner = prob.owners(m)
    start = prob.objective(m)
    rounds = moves = settled = 0
    trace = [start]
    while rounds < rounds_cap:
        props = {}
        slots = {}
        for i in range(prob.n):
            b = prob.best(m, owner, i)
            if b is None:
                continue
            d, pn, k, pk = b
            key = _key(d, i)
            props[i] = (key, pn, k, pk)
            for s in prob.footprint(i, pn, k, pk):
                slots[s] = min(slots.get(s, key), key)
        winners = [i for i, (key, pn, k, pk) in props.items() if all(slots[s] == key for s in prob.footprint(i, pn, k, pk))]
        if not winners:
            settled = 1
            break
        for i in winners:
            _key_i, pn, k, pk = props[i]
            if k >= 0:
                m[i], m[k] = pn, pk
                owner[prob.col(pn)], owner[prob.col(pk)] = i, k
            else:
                if m[i] >= 0:
                    owner[prob.col(m[i])] = -1
                if pn >= 0:
                    owner[prob.col(pn)] = i
                m[i] = pn
        rounds += 1
        moves += len(winners)
        trace.append(prob.objective(m))
    return np.array(m, dtype=np.int32), {"rounds": rounds, "moves": moves, "settled": settled, "objective_start": start,
                                         "objective": prob.objective(m), "trace": trace}


def improving_moves(prob, m):
    """every improving move of the four kinds at matching m, enumerated without the round's ownership shortcut (swaps either way round)"""
    m = [int(p) for p in m]
    owner = prob.owners(m)
    out = []
    for i in range(prob.n):
        if m[i] >= 0:
            d, s = prob.delta_single(m, i, -1)
            if d < -EPS * s:
                out.append(("unmatch", i))
        for p in prob.rows[i]:
            if p == m[i]:
                continue
            o = owner[prob.col(p)]
            if o < 0:
                d, s = prob.delta_single(m, i, p)
                if d < -EPS * s:
                    out.append(("move" if m[i] >= 0 else "match", i, p))
            elif m[i] >= 0:
                lo, hi = min(i, o), max(i, o)
                for q in prob.rows[o]:
                    if prob.col(q) == prob.col(m[i]):
                        pl, ph = (p, q) if lo == i else (q, p)
                        d, s = prob.delta_swap(m, lo, pl, hi, ph)
                        if d < -EPS * s:
                            out.append(("swap", lo, hi))
    return out


def lazy_objective(pairs, costs, n_aligned, triangles, axy, ref_xy, size, match_pair, no_match_penalty, delaunay_penalty,
                   penalty_coeff=100.0):
    """src/same.py:1191-1196 evaluated directly for a one-to-one matching: x_p from match_pair, p_j = max(0, matches - 1) = 0, n_i = 1 for
    unmatched cells, q_t from the lazy body (:645-669) over the triangles as given (corner order included), w_t = :1128-1134"""
    pairs, costs = np.asarray(pairs).reshape(-1, 2), np.asarray(costs, dtype=np.float64)
    match_pair = np.asarray(match_pair)
    matching = {int(pairs[p, 0]): int(pairs[p, 1]) for p in match_pair if p >= 0}
    x_term = sum(float(costs[p]) for p in match_pair if p >= 0)
    used = np.bincount([j for j in matching.values()], minlength=1) if matching else np.zeros(1)
    p_term = penalty_coeff * float(np.maximum(used - 1, 0).sum())
    n_term = no_match_penalty * sum(float(size[i]) for i in range(int(n_aligned)) if i not in matching)
    q_term = 0.0
    for a, b, c in np.asarray(triangles).reshape(-1, 3):
        if a not in matching or b not in matching or c not in matching:
            continue
        s_src = np.sign((axy[b][0] - axy[a][0]) * (axy[c][1] - axy[a][1]) - (axy[b][1] - axy[a][1]) * (axy[c][0] - axy[a][0]))
        ra, rb, rc = ref_xy[matching[a]], ref_xy[matching[b]], ref_xy[matching[c]]
        s_ref = np.sign((rb[0] - ra[0]) * (rc[1] - ra[1]) - (rb[1] - ra[1]) * (rc[0] - ra[0]))
        if s_src == 0 or s_ref == 0:
            continue
        if s_src != s_ref:
            q_term += float(size[a] + size[b] + size[c])
    return x_term + p_term + n_term + delaunay_penalty * q_term


def make_problem(kind="uniform", n=60, seed=0, jitter=0.6, k=4, equal_costs=False, delaunay_penalty=5.0, no_match_penalty=3.0):
    """a seeded window for the tests: cells (uniform, clustered or a lattice), references = the cells jittered (folds), the k nearest
    references within reach as pairs, Delaunay triangles of the cells, and the greedy one-to-one start (cheapest pairs first, a pair only
    below its cell's no-match cost).  -> (kwargs of Problem, start match_pair)"""
    from scipy.spatial import Delaunay, cKDTree

    rng = np.random.default_rng(seed)
    if kind == "lattice":
        s = int(np.ceil(np.sqrt(n)))
        g = np.stack(np.meshgrid(np.arange(s), np.arange(s)), -1).reshape(-1, 2)[:n].astype(np.float64)
        axy = g + rng.normal(0, 1e-3, g.shape)           # a lattice off its knife edges (no cocircular quads)
    elif kind == "clustered":
        centers = rng.uniform(0, np.sqrt(n), (max(2, n // 15), 2))
        axy = centers[rng.integers(0, len(centers), n)] + rng.normal(0, 0.6, (n, 2))
    else:
        axy = rng.uniform(0, np.sqrt(n), (n, 2))
    ref_xy = axy + rng.normal(0, jitter, axy.shape)
    size = rng.integers(1, 4, n).astype(np.float64)
    d, j = cKDTree(ref_xy).query(axy, k=min(k, n))
    pairs = np.stack([np.repeat(np.arange(n), j.shape[1]), j.reshape(-1)], 1).astype(np.int32)
    costs = np.round(d.reshape(-1), 6) if not equal_costs else np.ones(len(pairs))
    if equal_costs:
        costs = costs * 0.5
    tris = Delaunay(axy).simplices.astype(np.int32)
    unmatched = no_match_penalty * size
    start = np.full(n, -1, np.int32)
    taken = np.zeros(n, bool)
    for p in np.argsort(costs, kind="stable"):
        i, jj = pairs[p]
        if start[i] < 0 and not taken[jj] and costs[p] < unmatched[i]:
            start[i], taken[jj] = p, True
    kw = dict(pairs=pairs, costs=costs, unmatched=unmatched, n=n, n_r=n, triangles=tris, axy=axy, ref_xy=ref_xy, size=size,
              delaunay_penalty=delaunay_penalty)
    return kw, start
