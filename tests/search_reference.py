"""A step-exact restatement of the query kernel (csrc/query.hip, k_query) in plain Python / numpy: test infrastructure.

The walk is a deterministic function of its inputs: tree descent to a leaf, every leaf member pushed to the result list
and the frontier, random starts from the library's counter hash when the leaf is small, then best-first expansion under
    bound = worst + epsilon * (worst - min_distance)        (+inf while the list is short)
with the bound updated after every accepted push.  ``reference_search`` runs it one query at a time in float64 and
reports, next to the answer, what a test needs to know about the run: how many vertices were visited (V), how many
frontier entries were ever below the bound at once (L), and whether any decision of the walk was taken on operands the
float32 kernel may legitimately order the other way (``ambiguous``).

Two arithmetic modes:
  * exact=True ("lattice"): sqeuclidean on integer data with dim * (2R)^2 < 2^24 -- every float32 partial sum of the
    kernel is an exact integer, so distances, bounds and comparisons coincide bit for bit.  Only exact ties are flagged.
  * exact=False ("float"): every distance is an interval [lo, hi] around the float64 value with an a-priori float32
    error radius; a decision on overlapping intervals flags the query.
"""
import bisect
import math
from collections import namedtuple

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")
U24 = 2.0 ** -24
METRIC_CODE = {"sqeuclidean": 0, "euclidean": 0, "cosine": 1, "dot": 2, "inner_product": 3, "correlation": 4, "hellinger": 5}

SearchResult = namedtuple("SearchResult", ["ids", "dists", "radius", "V", "L", "F", "ambiguous", "reason", "used_rng", "trace"])


# ------------------------------------------------------------------------------------------------ the counter hash
def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hash2(seed, a):
    return mix32(seed ^ mix32(a + 0x9E3779B9))


def hash3(seed, a, b):
    return mix32(hash2(seed, a) ^ mix32(b * 0x85EBCA6B + 0xC2B2AE35))


def searcher_seed(rng_state):
    """The searcher's 32-bit seed from the index's int64[3] search_rng_state (1 without a state)."""
    if rng_state is None:
        return 1
    s = [int(v) & 0xFFFFFFFF for v in rng_state]
    return mix32(s[0] ^ mix32(s[1] + 0x9E3779B9) ^ mix32(s[2] + 0x7F4A7C15))


# ------------------------------------------------------------------------------------------------ distances
def _ulp32(v):
    """float32 spacing at |v| (array or scalar, float64 in and out)."""
    a = np.minimum(np.abs(np.asarray(v, np.float64)), FLT_MAX).astype(np.float32)
    with np.errstate(over="ignore"):
        return np.spacing(a).astype(np.float64)


def _unit_rows(x):
    nrm = np.sqrt((x * x).sum(1))
    inv = np.where(nrm > 0.0, 1.0 / np.where(nrm > 0.0, nrm, 1.0), 0.0)
    return x * inv[:, None], nrm > 0.0


class _Distances:
    """Alt-space distances of one query to data rows, as (mid, lo, hi) float64 arrays.

    The error radius is derived from the arithmetic, never measured: gamma = (dp + 4) * 2^-24 times sum |a_i b_i| on the
    Gram value (on sum (a_i - b_i)^2 for sqeuclidean), the same gamma relative on each squared norm, both carried through
    the metric's monotone formula by evaluating it at both ends, plus 4 float32 ulps of the result where the formula has
    a sqrt / divide / log2."""

    def __init__(self, data, metric, exact, codes=None, values=None):
        self.metric, self.exact = metric, exact
        x = np.asarray(data, np.float32).astype(np.float64)
        self.n, self.d = x.shape
        self.gamma = 0.0 if exact else (((self.d + 3) & ~3) + 4) * U24
        self.raw = x
        self.proxy = None
        if codes is not None:  # the walk's rows: codebook values of the uint8 codes
            assert metric == 0 and exact
            self.proxy = np.asarray(values, np.float32).astype(np.float64)[np.asarray(codes)]
        if metric in (0, 1, 3):
            self.rows = x
            self.nz = (x * x).sum(1) > 0.0
        elif metric == 2:
            self.rows, self.nz = _unit_rows(x)
        elif metric == 4:
            self.rows, self.nz = _unit_rows(x - x.mean(1, keepdims=True))
        else:
            self.rows, self.nz = _unit_rows(np.sqrt(x))
        self.norm2 = (self.rows * self.rows).sum(1)

    def tree_query(self, q):
        """The query as the tree descent sees it (cosine / dot: normalised in float32), or None for a dead query."""
        q = np.asarray(q, np.float32).astype(np.float64)
        if self.metric in (1, 2):
            nrm = math.sqrt(float((q * q).sum()))
            if not nrm > 0.0:
                return None
            q = (q / nrm).astype(np.float32).astype(np.float64)
        return q

    def dist_query(self, qt):
        """The query as the distances see it (correlation / hellinger: transformed after the descent), and its flag."""
        if self.metric == 4:
            qt = qt - qt.mean()
        elif self.metric == 5:
            qt = np.sqrt(qt)
        if self.metric in (4, 5):
            rows, nz = _unit_rows(qt[None, :])
            return rows[0], bool(nz[0])
        return qt, bool((qt * qt).sum() > 0.0)

    def __call__(self, q, qnz, ids, rows=None):
        """(mid, lo, hi) of the distances of query q to rows ids."""
        m = self.metric
        a = (self.rows if rows is None else rows)[ids]
        if m == 0:
            diff = a - q
            mid = (diff * diff).sum(1)
            r = self.gamma * mid
            return mid, np.maximum(mid - r, 0.0), mid + r
        g = a @ q
        dg = self.gamma * (np.abs(a) @ np.abs(q))
        if m != 1 and m != 3:
            dg = dg + self.gamma * np.abs(g)  # gamma / 2 relative on each of the two norms
        nz = self.nz[ids]
        if m == 1:  # log2(sqrt(|q|^2 |x|^2) / <q, x>), 0 when the ratio is not above 1
            s = np.sqrt(float((q * q).sum()) * self.norm2[ids])

            def f(s, g):
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = s / g
                    return np.where(g > 0.0, np.where(r > 1.0, np.log2(np.where(r > 1.0, r, 1.0)), 0.0), FLT_MAX)

            mid, lo, hi = f(s, g), f(s * (1.0 - self.gamma), g + dg), f(s * (1.0 + self.gamma), g - dg)
            dead = ~nz
        elif m == 3:  # 1 / <q, x> for a positive product

            def f(g):
                with np.errstate(divide="ignore"):
                    return np.where(g > 0.0, np.minimum(1.0 / np.where(g > 0.0, g, 1.0), FLT_MAX), FLT_MAX)

            mid, lo, hi = f(g), f(g + dg), f(g - dg)
            dead = np.zeros(len(ids), bool)
        elif m == 4:  # 1 - <q, x> on centred unit rows
            mid, lo, hi = np.maximum(1.0 - g, 0.0), np.maximum(1.0 - g - dg, 0.0), np.maximum(1.0 - g + dg, 0.0)
            dead = np.zeros(len(ids), bool)
        else:  # dot / hellinger: -log2 <q, x> on unit rows

            def f(g):
                with np.errstate(divide="ignore", invalid="ignore"):
                    return np.where(g > 0.0, np.maximum(-np.log2(np.where(g > 0.0, g, 1.0)), 0.0), FLT_MAX)

            mid, lo, hi = f(g), f(g + dg), f(g - dg)
            dead = ~nz if qnz else np.ones(len(ids), bool)
        fin_lo, fin_hi = lo < FLT_MAX, hi < FLT_MAX
        lo = np.where(fin_lo, np.maximum(lo - 4.0 * _ulp32(lo), 0.0), lo)
        hi = np.where(fin_hi, hi + 4.0 * _ulp32(hi), hi)
        if m in (4, 5) and not qnz:  # two zero rows are at distance 0
            zero = ~nz
            dead = dead & nz
            mid, lo, hi = np.where(zero, 0.0, mid), np.where(zero, 0.0, lo), np.where(zero, 0.0, hi)
        return np.where(dead, FLT_MAX, mid), np.where(dead, FLT_MAX, lo), np.where(dead, FLT_MAX, hi)


def _to_f32_range(v):
    """A float64 value as the float32 bound would hold it: beyond FLT_MAX it is +inf."""
    return INF if v >= FLT_MAX * (1.0 + 2.0 ** -25) else v


# ------------------------------------------------------------------------------------------------ the walk
class _Walk:
    def __init__(self, n, indptr, indices, tree, dist, min_distance, n_neighbors, k, epsilon, seed, trace):
        self.n, self.indptr, self.indices, self.tree = n, indptr, indices, tree
        self.dist, self.md, self.nn, self.k, self.eps, self.seed = dist, float(np.float32(min_distance)), n_neighbors, k, float(epsilon), seed
        self.exact = dist.exact
        self.want_trace = trace
        self.visited = np.zeros(n, bool)

    def flag(self, why):
        if why not in self.reasons:
            self.reasons.append(why)

    def less(self, a, b, why):
        """a < b for (mid, lo, hi) operands; flags the query when the intervals overlap."""
        if a[2] < b[1]:
            return True
        if a[1] > b[2] or (a[1] == a[2] and b[1] == b[2]):  # apart, or both exact (and then a >= b)
            return False
        self.flag(why)
        return a[0] < b[0]

    def update_bound(self):
        if len(self.r_mid) < self.k:
            self.bound = (INF, INF, INF)
            return
        md, eps = self.md, self.eps
        w, wlo, whi = self.r_mid[-1], self.r_lo[-1], self.r_hi[-1]
        with np.errstate(over="ignore"):
            mid = float(np.float32(w + eps * (w - md)))  # the unique float32 rounding of the exact value (lattice)
        if self.exact:
            self.bound = (mid, mid, mid)
            return
        lo, hi = wlo + eps * (wlo - md), whi + eps * (whi - md)
        lo, hi = lo - 4.0 * float(_ulp32(lo)), hi + 4.0 * float(_ulp32(hi))
        self.bound = (mid, _to_f32_range(lo), _to_f32_range(hi))

    def result_push(self, c):
        """Enters iff it beats the worst entry; lands behind every entry that is not larger; the last one leaves."""
        mid, lo, hi, v = c
        if len(self.r_mid) == self.k:
            if not self.less((mid, lo, hi), (self.r_mid[-1], self.r_lo[-1], self.r_hi[-1]), "d vs worst"):
                return
        pos = bisect.bisect_right(self.r_mid, mid)
        self.r_mid.insert(pos, mid)
        self.r_lo.insert(pos, lo)
        self.r_hi.insert(pos, hi)
        self.r_id.insert(pos, v)
        if len(self.r_mid) > self.k:
            self.r_mid.pop(), self.r_lo.pop(), self.r_hi.pop(), self.r_id.pop()

    def frontier_push(self, c):
        mid, lo, hi, v = c
        # entries below the bound as the kernel's compaction would count them: before this push, under the bound that
        # held when the candidate was accepted
        live = len(self.front) if self.bound[0] == INF else bisect.bisect_left(self.front, (self.bound[0], -1))
        self.L = max(self.L, live)
        bisect.insort(self.front, (mid, v, lo, hi))
        self.F = max(self.F, len(self.front))
        if self.want_trace:
            self.trace.append(("push", mid, self.bound[0]))

    def candidates(self, ids):
        """Marks ids (first occurrences, in order) and returns those that had not been visited."""
        ids = np.asarray(ids, np.int64)
        ids = ids[~self.visited[ids]]
        if len(ids) > 1:
            _, first = np.unique(ids, return_index=True)
            if len(first) < len(ids):
                ids = ids[np.sort(first)]
        self.visited[ids] = True
        self.touched.append(ids)
        return ids

    def run(self, qi, query):
        self.reasons, self.trace, self.touched = [], [], []
        self.r_mid, self.r_lo, self.r_hi, self.r_id = [], [], [], []
        self.front, self.L, self.F, self.used_rng = [], 0, 0, False
        self.bound = (INF, INF, INF)
        self.seen_ids, self.seen_mid, self.expanded, self.n_seeds = [], [], [], 0
        dist, k = self.dist, self.k
        qt = dist.tree_query(query)
        if qt is None:  # a zero query under cosine / dot is skipped
            return
        # ---- tree descent: side 0 iff margin > 0, a margin of (almost) 0 is decided by the hash ----
        ls = le = 0
        if self.tree is not None:
            hyper, offsets, children = self.tree.hyperplanes, self.tree.offsets, self.tree.children
            node = depth = 0
            while children[node, 0] > 0:
                h = hyper[node].astype(np.float64)
                off = float(offsets[node])
                m = float(h @ qt) + off
                rad = dist.gamma * (float(np.abs(h) @ np.abs(qt)) + abs(off))
                if not self.exact and abs(m) <= max(rad, 1e-8):
                    self.flag("tree margin")
                if abs(m) < 1e-8:
                    side = hash3(self.seed, qi, depth) & 1
                    self.used_rng = True
                else:
                    side = 0 if m > 0.0 else 1
                node = int(children[node, side])
                depth += 1
            ls, le = -int(children[node, 0]), -int(children[node, 1])
        q, qnz = dist.dist_query(qt)
        walk_rows = dist.proxy
        self.q, self.qnz = q, qnz

        def push_all(ids, bounded):
            if len(ids) == 0:
                return
            mid, lo, hi = dist(q, qnz, ids, walk_rows)
            self.seen_ids.append(ids)
            self.seen_mid.append(mid)
            order = range(len(ids))
            if bounded and self.bound[2] < INF:  # the bound only shrinks: what is surely not below it now never will be
                order = np.nonzero(lo <= self.bound[2])[0].tolist()
            for j in order:
                c = (float(mid[j]), float(lo[j]), float(hi[j]), int(ids[j]))
                if bounded and not self.less(c, self.bound, "d vs bound"):
                    continue
                self.result_push(c)
                self.frontier_push(c)
                if bounded:
                    self.update_bound()

        # ---- every leaf member, then random starts while the leaf held fewer than min(k, n_neighbors) ----
        n_initial = le - ls
        if n_initial > 0:
            push_all(self.candidates(self.tree.indices[ls:le]), False)
        for j in range(min(k, self.nn) - n_initial):
            u = hash3(self.seed ^ 0x3C6EF372, qi, j) % self.n
            self.used_rng = True
            push_all(self.candidates([u]), False)
        self.n_seeds = sum(len(t) for t in self.touched)
        self.update_bound()
        # ---- best-first: pop the frontier minimum while it is below the bound ----
        while self.front:
            mid, v, lo, hi = self.front.pop(0)
            if self.want_trace:
                self.trace.append(("pop", mid, v))
            # (epsilon = 0: the bound IS the worst entry's distance; a vertex is not below itself)
            if self.eps == 0.0 and len(self.r_id) == k and v == self.r_id[-1]:
                break
            if not self.less((mid, lo, hi), self.bound, "popped vs bound"):
                break
            if self.front:
                nxt = self.front[0]
                if nxt[2] <= hi and nxt[2] < self.bound[2]:
                    self.flag("pop order")  # the two smallest live keys tie (lattice) / overlap (float)
            self.expanded.append(v)
            push_all(self.candidates(self.indices[self.indptr[v]:self.indptr[v + 1]]), True)

    def finish(self, k_out=None):
        """The answer as arrays, the tie checks on it, and the clean-up of the visited marks."""
        dist, k = self.dist, self.k
        ids, mid, lo, hi = list(self.r_id), list(self.r_mid), list(self.r_lo), list(self.r_hi)
        touched = np.concatenate(self.touched) if self.touched else np.zeros(0, np.int64)
        V = int(len(touched))
        self.visited[touched] = False
        seen_ids = np.concatenate(self.seen_ids) if self.seen_ids else np.zeros(0, np.int64)
        seen_mid = np.concatenate(self.seen_mid) if self.seen_mid else np.zeros(0)
        if len(ids) == k and k > 0:
            if self.exact:  # equal distances on both sides of the k-th place among everything visited
                if int((seen_mid == mid[-1]).sum()) > sum(1 for m in mid if m == mid[-1]):
                    self.flag("boundary tie")
        if not self.exact:
            for j in range(len(ids) - 1):  # neighbours in the list whose order float32 may not reproduce
                if hi[j] >= lo[j + 1] and not (lo[j] == hi[j] and lo[j + 1] == hi[j + 1]):
                    self.flag("result order")
        if k_out is not None:  # the rerank: the walk's list in ascending proxy order, pushed by exact distance into k_out
            self.k = k_out
            cand = np.asarray(ids, np.int64)
            self.r_mid, self.r_lo, self.r_hi, self.r_id = [], [], [], []
            if len(cand):
                emid, elo, ehi = dist(self.q, self.qnz, cand, None)
                for j in range(len(cand)):
                    self.result_push((float(emid[j]), float(elo[j]), float(ehi[j]), int(cand[j])))
                if len(self.r_id) == k_out and int((emid == self.r_mid[-1]).sum()) > sum(1 for m in self.r_mid if m == self.r_mid[-1]):
                    self.flag("boundary tie")
            ids, mid, lo, hi = self.r_id, self.r_mid, self.r_lo, self.r_hi
            k = k_out
        out_ids = np.full(k, -1, np.int32)
        out_d = np.full(k, INF, np.float64)
        out_r = np.zeros(k, np.float64)
        m = len(ids)
        out_ids[:m] = ids
        out_d[:m] = mid
        out_r[:m] = np.maximum(np.asarray(hi) - np.asarray(mid), np.asarray(mid) - np.asarray(lo)) if m else 0.0
        trace = None
        if self.want_trace:
            trace = {"events": self.trace, "visited": touched, "seen_ids": seen_ids, "seen_mid": seen_mid, "expanded": list(self.expanded),
                     "seeds": touched[:self.n_seeds]}
        return SearchResult(out_ids, out_d, out_r, V, self.L, self.F, bool(self.reasons), "; ".join(self.reasons), self.used_rng, trace)


def reference_search(data, indptr, indices, tree, metric, min_distance, n_neighbors, queries, k, epsilon, seed_state=None, *,
                     exact=False, codes=None, values=None, rerank_k=None, trace=False):
    """The kernel's walk for every row of ``queries`` (numbered 0.. as in one call of the searcher).

    ``tree`` is a FlatTree (hyperplanes, offsets, children, indices) or None; ``metric`` a name or the library's code;
    ``seed_state`` the int64[3] state the searcher was created with.  ``exact=True`` is the lattice mode.  With ``codes`` /
    ``values`` (uint8 walk, sqeuclidean lattice) the walk keeps ``k`` results by proxy distance to the codebook values and
    reranks them by exact distance into ``rerank_k``.  Returns one SearchResult per query: ids and alt-space distances
    ascending (unfilled: -1 / inf), the error radius of every distance, V, L, F (largest frontier without compaction),
    ``ambiguous`` with its ``reason``, whether a hash draw was used, and with ``trace=True`` the events for a recount."""
    code = METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
    data = np.asarray(data)
    dist = _Distances(data, code, exact, codes, values)
    walk = _Walk(data.shape[0], np.asarray(indptr, np.int64), np.asarray(indices, np.int64), tree, dist, min_distance,
                 int(n_neighbors), int(k), epsilon, searcher_seed(seed_state), trace)
    out = []
    for qi, q in enumerate(np.asarray(queries)):
        walk.k = int(k)
        walk.run(qi, q)
        out.append(walk.finish(rerank_k if codes is not None else None))
    return out


def stack(results):
    """(ids (nq, k) int32, dists (nq, k) float64, radius (nq, k), ambiguous (nq,), V (nq,), L (nq,)) of a result list."""
    return (np.stack([r.ids for r in results]), np.stack([r.dists for r in results]), np.stack([r.radius for r in results]),
            np.array([r.ambiguous for r in results]), np.array([r.V for r in results]), np.array([r.L for r in results]))


def query_distances(data, metric, query, ids, *, exact=False):
    """(distance, error radius) of one query to the rows ``ids`` in the metric's alt space: what the weak check "the
    returned distance is the distance of the returned id" compares with."""
    code = METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
    dist = _Distances(np.asarray(data), code, exact)
    qt = dist.tree_query(query)
    if qt is None:
        return np.full(len(ids), INF), np.zeros(len(ids))
    q, qnz = dist.dist_query(qt)
    mid, lo, hi = dist(q, qnz, np.asarray(ids, np.int64))
    return mid, np.maximum(hi - mid, mid - lo)
