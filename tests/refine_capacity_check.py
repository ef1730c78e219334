"""Host statement of the window path's local search WITH the model's reference capacities (hip_refine="capacity",
same_amd/csrc/refine.hip), for the tests only: the product has no CPU fallback.  refine_check.py states the one-to-one search
(hip_refine="local"); this file states what changes when reference j may hold up to limit_j cells.

The objective is the lazy model's in full (src/same.py:1191-1196):

    sum_p c_p x_p + penalty_coeff sum_j max(0, count_j - 1) + no_match_penalty sum_i size_i n_i + delaunay_penalty sum_t w_t q_t

subject to count_j <= limit_j (src/helpers.py:102-161; at most 1001, the bound of p_j).  It is evaluated as
(costs + delaunay_penalty * flipped weight), then + penalty_coeff * sum_j max(0, count_j - 1) when that sum is not 0.

A round, as the device runs it -- refine_check.py's, with these changes:
  * "a free reference" is "a reference with room" (count < limit); a swap partner is a reference's ONLY holder (count == 1), so the
    device finds it from the sum of the holders' ids, whether the reference has room or not (per candidate the move is considered
    first, then the swap; under limit 1 only one of them applies); two cells on one reference never swap;
  * a single move from reference o to reference r adds penalty_coeff * (dn - do) to its delta, dn = [r held already], do = [o held twice
    or more], and penalty_coeff * (dn + do) to its scale; a swap keeps every count (no penalty term);
  * a single move's footprint also claims its OLD reference: winners then leave and take disjoint references, and their deltas add up.
Under limit 1 every penalty term is 0.0 and no other proposal claims a held reference but its holder's: refine_check.refine bit for bit.
"""
import numpy as np

from refine_check import EPS, Problem, _key

MAX_LIMIT = 1001


class CapProblem(Problem):
    """Problem plus limit (n_r,) int (each 1 .. 1001) and penalty_coeff"""

    def __init__(self, *args, limit=None, penalty_coeff=0.0, **kw):
        super().__init__(*args, **kw)
        self.limit = [1] * self.n_r if limit is None else [int(v) for v in np.asarray(limit).reshape(-1)]
        assert len(self.limit) == self.n_r and all(1 <= v <= MAX_LIMIT for v in self.limit)
        self.pc = float(penalty_coeff)

    def counts(self, m):
        c = [0] * self.n_r
        for p in m:
            if p >= 0:
                c[self.col(p)] += 1
        assert all(c[j] <= self.limit[j] for j in range(self.n_r)), "the matching takes a reference beyond its limit"
        return c

    def holder(self, m, j):
        """the only cell on reference j"""
        hs = [i for i, p in enumerate(m) if p >= 0 and self.col(p) == j]
        assert len(hs) == 1
        return hs[0]

    def delta_single_cap(self, m, count, i, pn):
        F, W = self._flip_part(m, [i], ((i, pn),))
        po = m[i]
        nw, old = self.term(i, pn), self.term(i, po)
        dn = int(pn >= 0 and count[self.col(pn)] >= 1)
        do = int(po >= 0 and count[self.col(po)] >= 2)
        return self.dp * F + (nw - old) + self.pc * float(dn - do), self.dp * W + (abs(nw) + abs(old)) + self.pc * float(dn + do)

    def cap_moves(self, m, count, i):
        """every candidate move of cell i in the order it is considered: (delta, scale, new pair, partner, partner's new pair)"""
        out = []
        po = m[i]
        if po >= 0:
            out.append((*self.delta_single_cap(m, count, i, -1), -1, -1, -1))
        for p in self.rows[i]:
            if p == po:
                continue
            j = self.col(p)
            if count[j] < self.limit[j]:
                out.append((*self.delta_single_cap(m, count, i, p), p, -1, -1))
            if po >= 0 and count[j] == 1 and j != self.col(po):
                o = self.holder(m, j)
                if o > i:
                    q = next((q for q in self.rows[o] if self.col(q) == self.col(po)), None)
                    if q is not None:
                        out.append((*self.delta_swap(m, i, p, o, q), p, o, q))
        return out

    def cap_best(self, m, count, i):
        best = None
        for d, s, pn, k, pk in self.cap_moves(m, count, i):
            if d < -EPS * s and (best is None or d < best[0]):
                best = (d, pn, k, pk)
        return best

    def cap_footprint(self, i, po, pn, k, pk):
        fp = self.footprint(i, pn, k, pk)
        if k < 0 and po >= 0 and ("r", self.col(po)) not in fp:
            fp.append(("r", self.col(po)))
        return fp

    def extra(self, m):
        return sum(max(0, c - 1) for c in self.counts(m))

    def cap_objective(self, m):
        obj = self.objective(m)
        e = self.extra(m)
        if e:
            obj += self.pc * float(e)
        return obj


def refine(prob, match_pair, rounds_cap):
    """-> (match_pair, {"rounds", "moves", "settled", "objective_start", "objective", "ref_extra_matches", "trace": objective after
    every round})"""
    m = [int(p) for p in match_pair]
    count = prob.counts(m)
    start = prob.cap_objective(m)
    rounds = moves = settled = 0
    trace = [start]
    while rounds < rounds_cap:
        props, slots = {}, {}
        for i in range(prob.n):
            b = prob.cap_best(m, count, i)
            if b is None:
                continue
            d, pn, k, pk = b
            key = _key(d, i)
            props[i] = (key, m[i], pn, k, pk)
            for s in prob.cap_footprint(i, m[i], pn, k, pk):
                slots[s] = min(slots.get(s, key), key)
        winners = [i for i, (key, po, pn, k, pk) in props.items() if all(slots[s] == key for s in prob.cap_footprint(i, po, pn, k, pk))]
        if not winners:
            settled = 1
            break
        for i in winners:
            _key_i, po, pn, k, pk = props[i]
            if k >= 0:
                m[i], m[k] = pn, pk
            else:
                if po >= 0:
                    count[prob.col(po)] -= 1
                if pn >= 0:
                    count[prob.col(pn)] += 1
                m[i] = pn
        assert count == prob.counts(m)
        rounds += 1
        moves += len(winners)
        trace.append(prob.cap_objective(m))
    return np.array(m, dtype=np.int32), {"rounds": rounds, "moves": moves, "settled": settled, "objective_start": start,
                                         "objective": prob.cap_objective(m), "ref_extra_matches": prob.extra(m), "trace": trace}


def model_objective(pairs, costs, n_aligned, triangles, axy, ref_xy, size, match_pair, no_match_penalty, delaunay_penalty, penalty_coeff):
    """src/same.py:1191-1196 evaluated directly for any matching (one pair per aligned cell at most): x_p from match_pair,
    p_j = max(0, count_j - 1), n_i = 1 for unmatched cells, q_t from the lazy body (:645-669) over the triangles as given"""
    from refine_check import lazy_objective

    pairs = np.asarray(pairs).reshape(-1, 2)
    mp = np.asarray(match_pair)
    cols = pairs[mp[mp >= 0], 1]
    extra = int(np.maximum(np.bincount(cols) - 1, 0).sum()) if len(cols) else 0
    # lazy_objective's p term counts the same thing; its matching dict keeps one reference per cell, as here
    return lazy_objective(pairs, costs, n_aligned, triangles, axy, ref_xy, size, match_pair, no_match_penalty, delaunay_penalty,
                          penalty_coeff), extra


def make_cap_problem(kind="uniform", n=60, seed=0, limits=(1, 2, 3, 5), penalty_coeff=1.0, **kw):
    """refine_check.make_problem's window with per-reference limits drawn from `limits` and the given penalty_coeff; the references
    are fewer than the cells (every second one kept), so capacities matter -> (kwargs of CapProblem, one-to-one start)"""
    from refine_check import make_problem

    base, _start = make_problem(kind, n=n, seed=seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    n_r = max(1, n // 2)
    ref_xy = np.asarray(base["ref_xy"])[:n_r]
    from scipy.spatial import cKDTree

    axy = np.asarray(base["axy"])
    k = min(4, n_r)
    d, j = cKDTree(ref_xy).query(axy, k=k)
    d, j = d.reshape(n, -1), j.reshape(n, -1)
    pairs = np.stack([np.repeat(np.arange(n), j.shape[1]), j.reshape(-1)], 1).astype(np.int32)
    costs = np.round(d.reshape(-1), 6)
    if kw.get("equal_costs"):
        costs = np.full(len(pairs), 0.5)
    unmatched = np.asarray(base["unmatched"])
    start = np.full(n, -1, np.int32)
    taken = np.zeros(n_r, bool)
    for p in np.argsort(costs, kind="stable"):
        i, jj = pairs[p]
        if start[i] < 0 and not taken[jj] and costs[p] < unmatched[i]:
            start[i], taken[jj] = p, True
    limit = rng.choice(np.asarray(limits, dtype=np.int32), n_r)
    out = dict(base, pairs=pairs, costs=costs, n_r=n_r, ref_xy=ref_xy, limit=limit, penalty_coeff=penalty_coeff)
    return out, start
