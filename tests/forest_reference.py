"""A step-exact restatement of the random-projection forest (csrc/rpforest.hip, nnd_launch_forest) in float64 numpy: test
infrastructure.

The forest is a deterministic function of the prepared rows and the tree seed; every random choice is the counter hash
(csrc/common.h :26-44).  Leaves come out in depth-first position order, so the leaf array determines every split: the model
re-derives each node's split and compares it with the prefix of the node's positions that the GPU sent left.

What is restated, and from where (rpforest.hip unless said otherwise):
  * rows (csrc/prep.hip): sqeuclidean rows centred on the mean of the rows r * stride, r < n_s = min(n, 65536), stride = n / n_s
    (:19, :261-264; float64 sums, :23-69); cosine / dot / correlation / hellinger rows transformed and scaled to unit length, zero
    rows stay zero (:138-170); inner product rows as given (:117-123).  dp = d rounded up to 32; the padding is zero.
  * hyperplane (k_hyperplane :78-126, k_finish_subtrees :813-847): h = x_l - x_r.  Unit-row metrics (nnd_metric_unit, "angular"):
    h scaled by inv = 1 / |h|, inv = 1 when |h| < 1e-8, offset 0.  Otherwise offset = -h . (x_l + x_r) / 2.
  * side (rp_side :184-193, k_route :1228-1229): |margin| < 1e-8 is a coin, else left (side 0) iff margin > 0.
  * the level passes (level_launch :1921-1971), keyed by POSITION.  A segment's members are in ascending id order (stable
    partitions of an iota, k_scatter :604-613).  Pivots: local indices hash3(seed, a, 2 depth) % len and
    hash3(seed, a, 2 depth + 1) % len, + 1 mod len on a collision (:78-80), a = the segment's first position (tree * n + offset).
    Coin: hash3(seed ^ 0x5bd1e995, key, depth) & 1 where key = the member's position at that level in k_margin (:227) but
    tree * n + POINT ID in k_margin_fused (:281-282) -- the point-major kernel has no position at hand.  Which kernel runs is the
    driver's rule (:1942): fused while it has never been left, S * dp * 2 <= 6 MiB and active_pos * 2 >= 3 n.  (So the level
    passes' coin is not position-keyed throughout; the lattice cases pin which key a level uses.)
    One-sided split (k_seg_count :479, k_scatter :604-608): even offsets left, odd offsets right.
  * the finishers (k_finish_subtrees, every template form), keyed by POINT ID with the per-tree salt
    seedt = seed ^ tree * 0x9E3779B9 (:723, tree = first position / n :684).  Pivots: the two members with the smallest
    hash3(seedt, id, 2 dep) << 32 | id (:793-812).  Coin: hash3(seedt ^ 0x5bd1e995, id, dep) & 1 (:921).  One-sided: every member
    re-drawn by hash3(seedt ^ 0x5bd1e995, id, 2 dep + 1) & 1; if those agree too the first pivot goes left alone (:932-951).  A node
    is a leaf iff not (len > leaf_size and max_depth - dep > 0) (:767); leaves are written in ascending id order (:769-778), the
    leaves that k_children marks (:562-568) are in that order already.
  * which regime (levels_start :1887-1918, k_children :546-569, forest_levels :2032-2053): whole-set mode with n <= FIN_MAX = 2048:
    the roots go to the finisher.  Otherwise a child that can split again stays in the passes iff len > fin_max, else it joins the
    finisher list with its depth.  Tail: after a level, once active_pos * 2 < 3 n and the longest stayer is <= BIG_MAX = 8192 the
    stayers go to the global-memory finisher (same rules; it hands nodes of <= FIN_MAX on to the LDS form).  active_pos counts the
    stayers of ALL trees, so the passes are modelled level by level over all trees.
  * routing mode (csrc/plan.h nnd_plan_routes: n >= 131072, dp <= 256): sample member j is row 16 j + hash2(seed ^ 0x7F4A7C15, j) % 16,
    M = n / 16 (k_gather_sample :1061).  The sample forest is the same machinery on the sample rows: leaf_size 24, fin_max 512,
    ids = sample indices, positions in T * M, recording finisher (one-wave form) with tree = position / M (forest_by_routing
    :2307-2308, record_subtrees :1999-2028).  Its leaves are the cells, in position order, each with its depth (:562-568, :979-983).
    Every point walks the recorded tree (k_route :1175-1242; k_route_top / k_route_bucket are the same walk): coin
    hash3(seed ^ 0x5bd1e995, t * n + i, step) & 1, no one-sided rule, a cell may stay empty.  Cells are finished by the finisher
    rules from the cell's depth (forest_place_finish :2274-2297), tree = position / n.

Arithmetic.  The model evaluates every margin in float64 on float64 prepared rows and attaches an a-priori float32 radius, derived
here and never measured (u = 2^-24, A = sum |h_j x_j|, every bound to first order with the constants rounded up to cover the second):
  * euclidean-style, m = h . x + off with B = sum |h_j (l_j + r_j)| / 2:  h_j = fl(l_j - r_j): u (A + B).  The dot product of dp
    terms in any order, with or without fused multiply-add (rp_exact_quad :173-182, rp_dot4f :1072-1077): dp u A.  The offset's sum
    with fl(l_j + r_j) and the products: (dp + 1) u B.  The final addition: u (A + B).  The prepared rows: fl(x_j - mean_j) moves a
    component by u |x_j| (an error of the mean itself is a translation and moves nothing), and m = (l - r) . (x - (l + r) / 2)
    gives dm = e_x . h + e_l . (x - l) - e_r . (x - r): u (A + sum |l_j| |x_j - l_j| + sum |r_j| |x_j - r_j|).  Together
        radius = (dp + 8) u (A + B) + rho (sum |l_j (x_j - l_j)| + sum |r_j (x_j - r_j)|),   rho = u (centred rows), 0 (rows as given).
  * angular, m = h . x, h = (l - r) / N, N = |l - r|:  fl(l_j - r_j) u, the scaling u, the dot product dp u: (dp + 2) u A.  The
    factor 1 / N is common to all of h and moves m relatively: its sum of squares is ceil(dp / 64) sequential terms per lane, a
    6-level reduction over the lanes and at most 4 partial sums of waves (k_hyperplane :87-101, k_finish_subtrees :816-838), then a
    square root (halves it) and a reciprocal: rho_h = ((ceil(dp / 64) + 10) / 2 + 2) u on |m|.  A prepared unit row is
    x (1 + e_s)(1 + e_j): a common factor from the float32 norm -- prep.hip sums at most max(ceil(d / 64), 4 ceil(dp / 256)) terms per
    lane and reduces over at most 64 lanes (:145-154, :205-213), then square root and reciprocal:
    |e_s| <= ((4 ceil(dp / 256) + 6) / 2 + 2) u = rho_s -- and per-component roundings (transform, product) |e_j| <= 3 u = rho_i.
    On x: rho_s |m| + rho_i A.  On a pivot p in {l, r}: dm = e_p . x / N - m (h . e_p) / N, i.e.
    rho_s |p . x - m (h . p)| / N + rho_i (sum |p_j x_j| + |m| sum |h_j p_j|) / N.  Together
        radius = (dp + 8) u A + (rho_s + rho_h) |m| + sum over both pivots of the two pivot terms.
    0 < N < 2e-8 (the inv = 1 branch within reach): every member of the node is unclear.
  * two pivots with identical prepared rows (identical input rows: the preparation is a function of the row) give h = 0 exactly on
    both sides: margin 0, radius 0, every member a clear coin.
  * exact=True (the lattice): integer rows with dp (2 R)^2 < 2^24 whose prepared form is the integers themselves (inner product, or
    a sampled column mean of exactly zero): every partial sum is an exact (half-)integer, radius 0, nothing is unclear.
The half-precision screening path (rp_band, cellA / cellB) is not modelled: its claim is that outside its band it returns the float32
sign, and that is what a comparison with this model tests.

Ambiguity.  A decision is clear when |m| > 1e-8 + radius (a sign) or |m| < 1e-8 - radius (a coin).  Check mode follows the GPU at
unclear decisions: a node's members occupy positions [a, a + len) in the GPU's order, its left child is a prefix; the model takes the
prefix that ends at a leaf boundary, contains every clear-left member and no clear-right member (the one of the model's own float64
size where several qualify).  No such prefix: a mismatch.  A one-sided verdict that hinges on unclear members is tried both ways.
The sample forest of the routing mode cannot be observed; its decisions take the float64 sign and ``recording_unclear`` counts those
that were unclear, per tree.
"""
from collections import namedtuple

import numpy as np

from tests import metric_util as MU
from tests.search_reference import METRIC_CODE, U24, _unit_rows, searcher_seed

EPS = 1e-8
FIN_MAX, BIG_MAX, FIN_SMALL = 2048, 8192, 512   # rpforest.hip :634-642
ROUTE_MIN_N, ROUTE_MAX_DP, SAMPLE_STRIDE, CELL_LEAF = 131072, 256, 16, 24   # csrc/plan.h nnd_plan_routes, nnd_make_plan
COIN = 0x5bd1e995
M32 = 0xFFFFFFFF
METRIC_NAME = {0: "euclidean", 1: "cosine", 2: "dot", 3: "inner_product", 4: "correlation", 5: "hellinger"}

ForestResult = namedtuple("ForestResult", [
    "leaf_array",           # (n_leaves, max(leaf_size, longest leaf)) int32, -1 padded: the model's forest (check mode: the GPU's, followed)
    "mismatch",             # per tree: None, or a dict (tree, depth, a, len, regime, pivots, reason, members [(id, m64, radius)])
    "decisions", "unclear",  # (member, node) decisions of the observable forest, and how many of them were unclear
    "recording_unclear",    # per tree: unclear decisions of the sample forest (routing mode; zeros otherwise)
    "n_cells",              # cells of the recorded trees (0: whole-set mode)
])


# ------------------------------------------------------------------------------------------------ the counter hash, vectorised
def _mix32v(x):
    x = np.asarray(x, np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def hash2v(seed, a):
    return _mix32v(np.uint64(seed & M32) ^ _mix32v(np.asarray(a, np.uint64) + np.uint64(0x9E3779B9)))


def hash3v(seed, a, b):
    """csrc/common.h nnd_hash3 on arrays (uint64 holding 32-bit words); tests pin it against the scalar hash3 and the header."""
    b = (np.asarray(b, np.uint64) & np.uint64(M32)) * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)
    return _mix32v(hash2v(seed, a) ^ _mix32v(b))


# ------------------------------------------------------------------------------------------------ rows and margins
class Prepared:
    """The prepared rows of csrc/prep.hip in float64, and a margin with its a-priori radius."""

    def __init__(self, data, metric, exact=False):
        self.code = METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
        x = np.asarray(data, np.float32).astype(np.float64)
        self.n, self.d = x.shape
        self.dp = (self.d + 31) & ~31
        self.exact = bool(exact)
        self.angular = self.code in (1, 2, 4, 5)
        self.rho = self.rho_s = self.rho_i = 0.0
        if self.code == 0:
            n_s = min(self.n, 65536)
            stride = self.n // n_s
            mean = x[:n_s * stride:stride].mean(0)
            if exact:
                assert not mean.any(), "lattice: the sampled column mean must be exactly 0"
            self.rows = x - mean
            self.rho = U24
        elif self.code == 3:
            self.rows = x
        else:
            self.rows, _ = _unit_rows(MU.transformed(METRIC_NAME[self.code], x))
            self.rho_s, self.rho_i = ((4 * -(-self.dp // 256) + 6) / 2 + 2) * U24, 3 * U24
            self.rho_h = ((-(-self.dp // 64) + 10) / 2 + 2) * U24
        if exact:
            assert not self.angular, "lattice: rows as given or centred on an exact zero only"
            r = np.abs(x).max() if x.size else 0.0
            assert np.array_equal(x, np.rint(x)) and self.dp * (2 * r) ** 2 < 2 ** 24, "lattice: integer rows, dp (2R)^2 < 2^24"
        self.abs = np.abs(self.rows)

    def take(self, idx):
        """the same preparation restricted to rows ``idx`` (the sample of the routing mode)."""
        p = object.__new__(Prepared)
        p.__dict__.update(self.__dict__)
        p.rows, p.abs, p.n = self.rows[idx], self.abs[idx], len(idx)
        return p

    def margins(self, ids, l, r):
        """(m64, radius) of rows ``ids`` against the hyperplane of the pivot rows l, r (float64 vectors)."""
        x, ax = self.rows[ids], self.abs[ids]
        if np.array_equal(l, r):
            return np.zeros(len(ids)), np.zeros(len(ids))
        v = l - r
        if not self.angular:
            m = x @ v - 0.5 * (v @ (l + r))
            if self.exact:
                return m, np.zeros(len(ids))
            rad = (self.dp + 8) * U24 * (ax @ np.abs(v) + 0.5 * (np.abs(v) @ np.abs(l + r)))
            if self.rho:
                rad = rad + self.rho * (np.abs(x - l) @ np.abs(l) + np.abs(x - r) @ np.abs(r))
            return m, rad
        nn = float(np.sqrt(v @ v))
        h = v if nn < EPS else v / nn
        m = x @ h
        if nn < 2 * EPS:
            return m, np.full(len(ids), np.inf)
        am = np.abs(m)
        rad = (self.dp + 8) * U24 * (ax @ np.abs(h)) + (self.rho_s + self.rho_h) * am
        for p in (l, r):
            rad = rad + (self.rho_s * np.abs(x @ p - m * (h @ p)) + self.rho_i * (ax @ np.abs(p) + am * (np.abs(h) @ np.abs(p)))) / nn
        return m, rad


def tree_seed_of(tree_rng):
    """csrc/common.h nnd_seed_of (handle.hip arm_for_build): the forest's 32-bit seed from the first tree's int64[3] state (= searcher_seed)."""
    return searcher_seed(tree_rng)


def sample_rows(n, seed):
    """k_gather_sample :1061: the rows of the routing mode's sample."""
    j = np.arange(n // SAMPLE_STRIDE, dtype=np.int64)
    return j * SAMPLE_STRIDE + (hash2v(seed ^ 0x7F4A7C15, j) % np.uint64(SAMPLE_STRIDE)).astype(np.int64)


class _Node:
    __slots__ = ("t", "a", "ids", "depth", "dead", "kids", "l", "r")

    def __init__(self, t, a, ids, depth, dead=False):
        self.t, self.a, self.ids, self.depth, self.dead, self.kids = t, a, ids, depth, dead, None


class _Gpu:
    """The GPU's leaf array, per tree: the permutation, every id's position and the leaf boundaries."""

    def __init__(self, la, n, T):
        la = np.asarray(la)
        lens = (la >= 0).sum(1)
        self.ok = bool(np.all((la >= 0) == (np.arange(la.shape[1])[None, :] < lens[:, None]))) and int(lens.sum()) == n * T and lens.min() >= 1
        ends = np.cumsum(lens)
        self.ok = self.ok and all(np.any(ends == n * (t + 1)) for t in range(T))
        self.perm = la[la >= 0].astype(np.int64)
        self.bound = np.zeros(n * T + 1, bool)
        self.pos = np.zeros((T, n), np.int64)
        self.tree_ok = [False] * T
        if self.ok:
            self.bound[0] = True
            self.bound[ends] = True
            for t in range(T):
                p = self.perm[t * n:(t + 1) * n]
                self.tree_ok[t] = bool(np.array_equal(np.sort(p), np.arange(n)))
                if self.tree_ok[t]:
                    self.pos[t, p] = t * n + np.arange(n)


class _View:
    """One run of the level passes and finishers: the whole point set, or the routing mode's sample (record=True)."""

    def __init__(self, model, rows, T, leaf_size, fin_max, record, gpu):
        self.m, self.R, self.n, self.T = model, rows, rows.n, T
        self.leaf_size, self.fin_max, self.record, self.gpu = leaf_size, fin_max, record, gpu


class ForestModel:
    """``ForestModel(x, metric, n_trees, leaf_size, tree_rng, ...).run(gpu_leaf_array=None)``.

    ``routing``: None = the library's rule (n >= 131072 and dp <= 256); True / False force it (the CPU tests run the routing
    machinery at a few thousand points).  Test hooks that build a deliberately WRONG forest in dry-run mode, for the mutation
    tests: ``tree_alias`` {t: t'} lets tree t draw with tree t' 's positions and salt; ``cells_from_depth0`` finishes every cell
    from depth 0."""

    def __init__(self, data, metric, n_trees, leaf_size, tree_rng, max_depth=200, exact=False, routing=None, tree_alias=None,
                 cells_from_depth0=False):
        self.R = data if isinstance(data, Prepared) else Prepared(data, metric, exact)
        self.n, self.T, self.leaf_size, self.max_depth = self.R.n, int(n_trees), int(leaf_size), int(max_depth)
        self.seed = tree_rng if isinstance(tree_rng, int) else tree_seed_of(tree_rng)
        self.routing = (self.n >= ROUTE_MIN_N and self.R.dp <= ROUTE_MAX_DP) if routing is None else bool(routing)
        self.alias = dict(tree_alias or {})
        self.cells_from_depth0 = cells_from_depth0

    # -------------------------------------------------------------------------------------------- bookkeeping
    def _tree(self, t):
        return self.alias.get(t, t)

    def _seedt(self, t):
        return self.seed ^ ((self._tree(t) * 0x9E3779B9) & M32)

    def _fail(self, node, regime, reason, pivots=None, ids=None, m=None, rad=None):
        node.dead = True
        if self._rec_view:  # the sample forest is not observable: nothing to fail
            return
        mem = []
        if ids is not None:
            mem = [(int(i), float(mm), float(rr)) for i, mm, rr in zip(ids[:8], m[:8], rad[:8])]
        rep = dict(tree=node.t, depth=node.depth, a=int(node.a - node.t * self.n), len=len(node.ids), regime=regime, pivots=pivots,
                   reason=reason, members=mem)
        old = self.mismatch[node.t]
        if old is None or (rep["depth"], rep["a"]) < (old["depth"], old["a"]):
            self.mismatch[node.t] = rep

    def _count(self, node, n_dec, n_unclear):
        if self._rec_view:
            self.recording_unclear[node.t] += int(n_unclear)
        elif not node.dead:
            self.decisions += int(n_dec)
            self.unclear += int(n_unclear)

    # -------------------------------------------------------------------------------------------- one split
    def _classify(self, m, rad, coin):
        """(left64, clear): the float64 verdict (True = left) and whether it is clear."""
        am = np.abs(m)
        is_coin = am < EPS
        left64 = np.where(is_coin, coin == 0, m > 0.0)
        clear = (am > EPS + rad) | (am < EPS - rad)
        return left64, clear

    def _follow(self, view, node, left64, clear, allow_empty):
        """The left mask of the node's members: the model's own (dry-run, dead nodes), or the GPU's prefix (check).  None: mismatch."""
        gpu = view.gpu
        ln = len(node.ids)
        if gpu is None or node.dead:
            return left64
        p = gpu.pos[node.t][node.ids] - node.a
        cl, cr = clear & left64, clear & ~left64
        lo = int(p[cl].max()) + 1 if cl.any() else 0
        hi = int(p[cr].min()) if cr.any() else ln
        if not allow_empty:
            lo, hi = max(lo, 1), min(hi, ln - 1)
        if lo > hi:
            return None
        cand = lo + np.flatnonzero(gpu.bound[node.a + lo:node.a + hi + 1])
        if len(cand) == 0:
            return None
        want = int(left64.sum())
        nl = want if want in cand else int(cand[0])
        return p < nl

    def _split(self, view, node, regime, idl, idr, coin, one_sided_rule, allow_empty=False):
        """Children id arrays (left, right) of a node (after a mismatch: the model's own, the node dead).  ``one_sided_rule()`` -> left mask."""
        R, ids = view.R, node.ids
        if regime != "walk":
            node.l, node.r = R.rows[idl], R.rows[idr]
        m, rad = R.margins(ids, node.l, node.r)
        left64, clear = self._classify(m, rad, coin)
        unclear = ~clear
        self._count(node, len(ids), unclear.sum())
        if not self._rec_view:
            self.trace.append((regime, node.t, node.depth, int(node.a - node.t * self.n), len(ids)))
        ln = len(ids)
        left = None
        if not allow_empty:
            cl, cr = int((clear & left64).sum()), int((clear & ~left64).sum())
            hinge = unclear.any() and (cl == 0 or cr == 0)
            sure = not unclear.any() and (cl == 0 or cr == 0)
            if sure or (hinge and (view.gpu is None or node.dead) and int(left64.sum()) in (0, ln)):
                left = one_sided_rule()
                got = self._follow(view, node, left, np.ones(ln, bool), False)
                if got is None:  # (the rest of the subtree is grown without the GPU: the level accounting of the other trees goes on)
                    self._fail(node, regime, "one-sided split: the rule's sides are not the GPU's", (idl, idr), ids, m, rad)
            elif hinge and view.gpu is not None and not node.dead:
                redrawn = one_sided_rule()
                left = self._follow(view, node, redrawn, np.ones(ln, bool), False)  # the GPU saw one side only ...
                if left is None:
                    left = self._follow(view, node, left64, clear, False)          # ... or the unclear members made two
        if left is None:
            left = self._follow(view, node, left64, clear, allow_empty)
            if left is None:
                p = view.gpu.pos[node.t][ids] - node.a
                bad = clear & (left64 != (p < int(left64.sum())))
                sel = np.flatnonzero(bad if bad.any() else clear)
                self._fail(node, regime, "no prefix at a leaf boundary holds every clear-left member and no clear-right member",
                           (idl, idr), ids[sel], m[sel], rad[sel])
                left = self._follow(view, node, left64, clear, allow_empty)  # dead now: the model's own sides
        return ids[left], ids[~left]

    def _leaf(self, view, node):
        """A final leaf (or a cell of the sample forest): ascending ids at [a, a + len)."""
        if view.record:
            return
        ids = node.ids
        self.leaves.append((node.a, ids))
        gpu = view.gpu
        if gpu is not None and not node.dead:
            a, e = node.a, node.a + len(ids)
            if not (gpu.bound[a] and gpu.bound[e]) or gpu.bound[a + 1:e].any():
                self._fail(node, "leaf", "the GPU's leaf boundaries are not [a, a + len)")
            elif not np.array_equal(gpu.perm[a:e], ids):
                self._fail(node, "leaf", "the leaf is not its members in ascending id order")

    # -------------------------------------------------------------------------------------------- the two regimes
    def _split_level(self, view, node, depth, fused):
        ids, ln, a = node.ids, len(node.ids), node.a
        a_draw = a + (self._tree(node.t) - node.t) * view.n  # (tree_alias hook; 0 otherwise)
        li = int(hash3v(self.seed, a_draw, 2 * depth)) % ln
        ri = int(hash3v(self.seed, a_draw, 2 * depth + 1)) % ln
        if ri == li:
            ri = (ri + 1) % ln
        key = self._tree(node.t) * view.n + ids if fused else a_draw + np.arange(ln)
        coin = hash3v(self.seed ^ COIN, key, depth) & np.uint64(1)
        return self._split(view, node, "level", int(ids[li]), int(ids[ri]), coin, lambda: np.arange(ln) % 2 == 0)

    def _finish(self, view, root, dep0):
        """k_finish_subtrees on the segment ``root`` from depth dep0; record mode: returns the recorded subtree in root.kids."""
        seedt = self._seedt(root.t)
        stack = [root]
        root.depth = dep0
        while stack:
            node = stack.pop()
            ids, ln, dep = node.ids, len(node.ids), node.depth
            if not (ln > view.leaf_size and self.max_depth - dep > 0):
                self._leaf(view, node)
                continue
            keys = (hash3v(seedt, ids, 2 * dep) << np.uint64(32)) | ids.astype(np.uint64)
            o = np.argpartition(keys, 1)[:2] if ln > 2 else np.argsort(keys)
            o = o[np.argsort(keys[o])]
            idl, idr = int(ids[o[0]]), int(ids[o[1]])
            coin = hash3v(seedt ^ COIN, ids, dep) & np.uint64(1)

            def redraw(ids=ids, dep=dep, idl=idl):
                left = (hash3v(seedt ^ COIN, ids, 2 * dep + 1) & np.uint64(1)) == 0
                return left if 0 < int(left.sum()) < len(ids) else ids == idl
            kids = self._split(view, node, "finisher", idl, idr, coin, redraw)
            node.kids = [_Node(node.t, node.a, kids[0], dep + 1, node.dead), _Node(node.t, node.a + len(kids[0]), kids[1], dep + 1, node.dead)]
            stack.extend(node.kids)

    def _levels(self, view):
        """forest_levels: the roots of the view's trees, grown; returns them."""
        n, T, dp = view.n, view.T, view.R.dp
        bad = [view.gpu is not None and not view.gpu.tree_ok[t] for t in range(T)]
        roots = [_Node(t, t * n, np.arange(n, dtype=np.int64), 0, bad[t]) for t in range(T)]
        if not (n > view.leaf_size and self.max_depth > 0):
            for r in roots:
                self._leaf(view, r)
            return roots
        if not view.record and n <= view.fin_max:
            for r in roots:
                self._finish(view, r, 0)
            return roots
        segs, fin, depth, active_pos, inv_live = roots, [], 0, T * n, True
        while segs:
            fused = inv_live and len(segs) * dp * 2 <= (6 << 20) and active_pos * 2 >= 3 * n
            inv_live = fused
            can_split = self.max_depth - (depth + 1) > 0
            nxt = []
            for node in segs:
                node.depth = depth
                kids = self._split_level(view, node, depth, fused)
                node.kids = [_Node(node.t, node.a, kids[0], depth + 1, node.dead), _Node(node.t, node.a + len(kids[0]), kids[1], depth + 1, node.dead)]
                for c in node.kids:
                    if can_split and len(c.ids) > view.leaf_size:
                        (nxt if len(c.ids) > view.fin_max else fin).append(c)
                    else:
                        self._leaf(view, c)
            depth += 1
            segs = nxt
            active_pos = sum(len(c.ids) for c in segs)
            if not view.record and segs and active_pos * 2 < 3 * n and max(len(c.ids) for c in segs) <= BIG_MAX:
                fin.extend(segs)
                segs = []
        for node in fin:
            self._finish(view, node, node.depth)
        return roots

    # -------------------------------------------------------------------------------------------- routing mode
    def _walk(self, view, t, rec_root):
        """every point of tree t through the recorded tree; the cells in position order, finished."""
        n = self.n
        stack = [(rec_root, _Node(t, t * n, np.arange(n, dtype=np.int64), 0, view.gpu is not None and not view.gpu.tree_ok[t]))]
        while stack:
            rec, node = stack.pop()
            if rec.kids is None:  # a cell
                self.n_cells += 1
                self.trace.append(("cell", t, rec.depth, int(node.a - t * n), len(node.ids)))
                if len(node.ids):
                    self._finish(view, node, 0 if self.cells_from_depth0 else rec.depth)
                continue
            node.l, node.r, node.depth = rec.l, rec.r, rec.depth
            coin = hash3v(self.seed ^ COIN, self._tree(t) * n + node.ids, rec.depth) & np.uint64(1)
            if len(node.ids) == 0:
                kids = (node.ids, node.ids)
            else:
                kids = self._split(view, node, "walk", None, None, coin, None, allow_empty=True)
            stack.append((rec.kids[0], _Node(t, node.a, kids[0], rec.depth + 1, node.dead)))
            stack.append((rec.kids[1], _Node(t, node.a + len(kids[0]), kids[1], rec.depth + 1, node.dead)))

    def record_tops(self):
        """The sample forest alone (dry-run): its roots; fills ``recording_unclear``."""
        self.recording_unclear = [0] * self.T
        self._rec_view = True
        srow = sample_rows(self.n, self.seed)
        view = _View(self, self.R.take(srow), self.T, CELL_LEAF, FIN_SMALL, True, None)
        roots = self._levels(view)
        self._rec_view = False
        return roots

    # -------------------------------------------------------------------------------------------- entry
    def run(self, gpu_leaf_array=None):
        n, T = self.n, self.T
        self.leaves, self.mismatch = [], [None] * T
        self.trace = []  # (regime, tree, depth, first position in the tree, len) of every split and every cell, for the tests
        self.decisions = self.unclear = self.n_cells = 0
        self.recording_unclear = [0] * T
        self._rec_view = False
        gpu = None
        if gpu_leaf_array is not None:
            gpu = _Gpu(gpu_leaf_array, n, T)
            for t in range(T):
                if not gpu.tree_ok[t]:
                    self.mismatch[t] = dict(tree=t, depth=0, a=0, len=n, regime="partition", pivots=None, members=[],
                                            reason="the tree's rows do not hold every point once")
        if self.routing:
            roots = self.record_tops()
            view = _View(self, self.R, T, self.leaf_size, FIN_MAX, False, gpu)
            for t in range(T):
                self._walk(view, t, roots[t])
        else:
            self._levels(_View(self, self.R, T, self.leaf_size, FIN_MAX, False, gpu))
        self.leaves.sort(key=lambda e: e[0])
        width = max([self.leaf_size] + [len(ids) for _, ids in self.leaves])
        la = np.full((max(len(self.leaves), 1), max(width, 1)), -1, np.int32)
        for i, (_, ids) in enumerate(self.leaves):
            la[i, :len(ids)] = ids
        return ForestResult(la, list(self.mismatch), self.decisions, self.unclear, list(self.recording_unclear), self.n_cells)


def describe(mis):
    """one line per mismatching tree."""
    return "\n".join("tree %(tree)d depth %(depth)d segment [%(a)d, +%(len)d) %(regime)s pivots %(pivots)s: %(reason)s; members (id, m64, radius) %(members)s"
                     % m for m in mis if m is not None)
