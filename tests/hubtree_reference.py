"""A step-exact restatement of the hub search tree of prepare() (csrc/hubtree.hip, entry nnd_hub_tree_build) in numpy: test
infrastructure.

The tree is a deterministic function of the rows and the neighbour graph; the handle's seed never reaches a decision (hubtree.hip
:27-32).  The output is the reference's FlatTree (make_hub_tree + convert_tree_format, rp_trees.py:714-1312, 2926-3049).

What is restated, and from where (hubtree.hip unless said otherwise):
  * rows: ``x_orig`` as given, un-prepared, for EVERY metric (:352-355; search_tree.py make_hub_tree builds the handle with
    NND_FLAG_NO_PREP).  The angular branch is taken by the unit-row metrics cosine, dot, correlation, hellinger (csrc/metric.h :30
    nnd_metric_unit, capi.hip nnd_hub_tree_build); euclidean and inner_product take the euclidean branch.
  * in-degrees over the valid graph entries 0 <= id < n only (search_tree.py compute_global_degrees, csrc/prepare.hip; rp_trees.py:733-737);
    rank order by (-degree, id) (search_tree.py make_hub_tree: a stable argsort of -degree).
  * a node's members are in ascending id order (:51-58 an iota, stable partitions :385-388).  Its hubs are its first min(len, 3) members by
    rank (k_hub_planes :69-79: the head of the rank-ordered segment).  Candidates: the hub pairs (0,1), (0,2), (1,2) in this order (:72);
    a node of 2 has the first only (:125 ncand).
  * planes (k_hub_planes :80-107).  euclidean: h_j = l_j - r_j, off = off - (h_j * (l_j + r_j)) * 0.5 over j ascending.  angular:
    L = sqrt(sum l_j l_j) (j ascending), L = 1 if L < 1e-8f, same for r; v_j = l_j / L - r_j / R; N = sqrt(sum v_j v_j), N = 1 if N < 1e-8f;
    h_j = v_j / N; off = 0.
  * margin (k_hub_margins :128-136): m = off; m = m + h_j * x_j over j ascending.  Side (:141): m > 1e-8f left (0), m < -1e-8f right (1),
    else i & 1 where i is the member's offset in the node's ascending-id order.
  * winner (k_hub_choose :177-192): candidates in order; one with an empty side is skipped; balance = float32(min(nl, nr)) / float32(len);
    a candidate replaces the best only when strictly greater (the first wins a tie); best < 0.1f (float32): the node is a leaf.
  * a node splits iff len > leaf_size and max_depth - depth > 0 (:336 root, :234 and :358 children) and it has a winner; leaf_size < 1 counts
    as 1 (:310).
  * the FlatTree (:396-444): pre-order numbers, the left child is numbered next; a leaf's children = (-start, -end) of its slice of
    ``indices``, its ids ascending (:428-433); leaves keep zero hyperplane rows and offset 0; leaf_size = max(leaf_size, largest leaf)
    (:415, :434).

Two arithmetic modes.

``exact32``: the kernel's documented arithmetic.  Every operation above is ONE correctly rounded float32 operation, in the order above,
vectorised over the members of a node and sequential over the dimension (``m = m + h[j] * x[:, j]`` on float32 arrays: numpy rounds the
product, then the sum); float32 ``sqrt`` and ``/``.  The result is a complete FlatTree; the GPU's must equal it byte for byte.

``check``: the verdict that survives a change of summation order.  It walks the GPU's own tree; a node's members are the ids under it.
Margins are float64 and carry an a-priori float32 radius, derived here and never measured (u = 2^-24, first order, constants rounded up to
cover the second; d terms summed in ANY order, fused or not; rows as given, so there is no centring term):
  * euclidean, m = sum h_j x_j + off, A = sum |h_j x_j|, B = sum |h_j (l_j + r_j)| / 2:  h_j = fl(l_j - r_j) moves both sums: u (A + B).
    The offset: fl(l_j + r_j) and the product u B each, the halving is exact, d subtractions d u B: (d + 2) u B.  The margin: d products u A,
    and d additions whose partial sums are bounded by A + B: d u (A + B).  Together (d + 2) u A + (2 d + 3) u B;
        radius = (d + 8) u A + (2 d + 8) u B.
    h itself is one operation per component and must be equal; the offset alone is held to (d + 8) u B.
  * angular, m = h . x, h = v / N, v = l^ - r^, l^ = l / L:  a computed norm is the true one times (1 + e), |e| <= rho = (d / 2 + 2) u (d
    products and d - 1 additions of non-negative terms: d u on the sum of squares, halved by the root, plus the root's own rounding).  So the
    computed v is (1 + a) l^ - (1 + b) r^ + D with |a|, |b| <= rho and |D_j| <= u (|l^_j| + |r^_j|) (the two quotients) + u |v_j| (the
    difference) <= 2 u (|l^_j| + |r^_j|).  With dm = dv . x / N - m (h . dv) / N, the factor 1 / N (rho |m|), h_j = fl(v_j / N) (u A) and the
    dot product (d u A):
        radius = (d + 8) u A + rho |m| + sum over p in {l^, r^} of (rho |p . x - m (h . p)| + 2 u (sum |p_j x_j| + |m| sum |h_j p_j|)) / N.
    A zero hub row keeps L = 1 and l^ = 0 exactly.  A hub row with 0 < |l| < 2e-8 (the L = 1 branch within reach) makes every member unclear.
    l^ = r^ exactly (identical rows, or rows that differ by a power of two: scaling by 2 is exact in every operation) gives v = 0, N = 1,
    h = 0: margin 0, radius 0, every member a clear parity decision.  Nearly collinear hubs have a small N and the radius grows with 1 / N
    until every member is unclear: nothing needs a special rule.  The radius of h_j itself is the same formula at x = e_j.
  * ``exact=True`` (the lattice): euclidean branch, integer rows with 8 d R^2 < 2^24 (R = max |x_j|): every h_j, product, half-integer
    offset term and partial sum is an exact float32, in any order: radius 0, nothing is unclear.
A decision is clear when m > 1e-8 + radius (left), m < -1e-8 - radius (right) or |m| <= 1e-8 - radius (parity); otherwise it is unclear,
the mode follows the GPU and counts it.  Per candidate the clear members give an interval [lo, hi] for the left count.  At a node the mode
checks that the size and depth rules hold exactly; that a splitting node's hyperplane is one of its candidates; that every clear member lies
on the side the GPU put it; that the choice is a possible winner (every earlier candidate can be strictly worse, every later one no
better, under the intervals; the chosen one's balance is the GPU's own count); that split-or-leaf agrees with the balance against
float32 0.1; that leaves are ascending and leaf_size is the maximum.  Where two candidates share a hyperplane (coinciding hubs) the node
passes if either reading passes.
"""
from collections import namedtuple

import numpy as np

U24 = 2.0 ** -24
EPS32 = np.float32(1e-8)               # hubtree.hip :39 HUB_EPS (rp_trees.py:23)
EPS = float(EPS32)
MIN_BALANCE32 = np.float32(0.1)        # hubtree.hip :40 HUB_MIN_BALANCE (rp_trees.py:798)
PAIRS = ((0, 1), (0, 2), (1, 2))       # hubtree.hip :72
ANGULAR = {"euclidean": False, "sqeuclidean": False, "inner_product": False, "cosine": True, "dot": True, "correlation": True,
           "hellinger": True}          # csrc/metric.h :30 nnd_metric_unit

Tree = namedtuple("Tree", ["hyperplanes", "offsets", "children", "indices", "leaf_size"])
HubResult = namedtuple("HubResult", [
    "tree",       # the FlatTree tables
    "nodes",      # per pre-order node: dict(node, depth, len, hubs, choice (-1 leaf), nl, counts [(nl_c) per candidate])
    "stats",      # dict: one_sided (candidates skipped), parity (member decisions by i & 1), ties (nodes whose best balance two candidates
                  # share), lopsided (leaves made by the balance rule), no_valid (of them: no valid candidate at all), level_segments
                  # {depth: nodes}, mutated (the node a test hook changed, or None)
])
CheckResult = namedtuple("CheckResult", [
    "mismatch",        # list of dicts (node, depth, len, hubs, candidate, reason, members [(id, offset, m64, radius, gpu side)])
    "decisions", "unclear",   # (member, node, candidate) decisions, and how many of them were unclear
    "unclear_nodes",   # pre-order numbers of the nodes with an unclear decision
])


# ------------------------------------------------------------------------------------------------ degrees and ranks
def degrees(neighbor_indices, n):
    idx = np.asarray(neighbor_indices)
    valid = (idx >= 0) & (idx < n)
    return np.bincount(idx[valid].ravel().astype(np.int64), minlength=n)[:n].astype(np.int64)


def rank_order(deg):
    """ids by (-degree, id)."""
    return np.argsort(-np.asarray(deg, np.int64), kind="stable").astype(np.int32)


def _ranks(neighbor_indices, n):
    rank = np.empty(n, np.int64)
    rank[rank_order(degrees(neighbor_indices, n))] = np.arange(n)
    return rank


def _hubs(ids, rank):
    return ids[np.argsort(rank[ids], kind="stable")[:3]]


def _balance32(k, ln):
    return np.float32(k) / np.float32(ln)


# ------------------------------------------------------------------------------------------------ exact32
def _seq_sumsq32(v):
    s = np.float32(0.0)
    for j in range(v.shape[0]):
        s = np.float32(s + np.float32(v[j] * v[j]))
    return s


def plane32(l, r, angular):
    """(h (d) float32, off float32) of the hub rows l, r (float32 vectors), operation for operation as k_hub_planes."""
    d = l.shape[0]
    if not angular:
        h = (l - r).astype(np.float32)
        t = ((h * (l + r).astype(np.float32)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
        o = np.float32(0.0)
        for j in range(d):
            o = np.float32(o - t[j])
        return h, o
    ln, rn = np.sqrt(_seq_sumsq32(l)), np.sqrt(_seq_sumsq32(r))
    if abs(ln) < EPS32:
        ln = np.float32(1.0)
    if abs(rn) < EPS32:
        rn = np.float32(1.0)
    v = ((l / ln).astype(np.float32) - (r / rn).astype(np.float32)).astype(np.float32)
    hn = np.sqrt(_seq_sumsq32(v))
    if abs(hn) < EPS32:
        hn = np.float32(1.0)
    return (v / hn).astype(np.float32), np.float32(0.0)


def margins32(xm, hs, offs):
    """(len, ncand) float32 margins of the member rows xm against the planes hs (ncand, d), offs (ncand): m = m + h_j * x_j, j ascending."""
    m = np.repeat(np.asarray(offs, np.float32)[None, :], xm.shape[0], 0)
    t = np.empty_like(m)
    for j in range(xm.shape[1]):
        np.multiply(xm[:, j:j + 1], hs[None, :, j], out=t)
        np.add(m, t, out=m)
    return m


def sides32(m):
    """0 left / 1 right per (member, candidate); the parity rule on the member's offset."""
    par = (np.arange(m.shape[0]) & 1)[:, None]
    return np.where(m > EPS32, 0, np.where(m < -EPS32, 1, par)).astype(np.int8)


def exact32(data, neighbor_indices, leaf_size=30, max_depth=200, metric="euclidean", mutate=None):
    """The hub tree in the kernel's documented arithmetic.  ``mutate`` builds a deliberately WRONG tree for the planted-error tests:
    (kind, k) changes the k-th node (pre-order) at which the kind applies -- "move": one member of largest |margin| goes to the other
    child; "second_best": a valid candidate of strictly smaller balance (still >= 0.1) is chosen; "split_lopsided": a node whose best
    balance is below 0.1 splits by its best candidate anyway."""
    x = np.ascontiguousarray(data, np.float32)
    n, d = x.shape
    angular = ANGULAR[metric]
    leaf_size, max_depth = max(int(leaf_size), 1), int(max_depth)
    rank = _ranks(neighbor_indices, n)
    hyper, offs, children, nodes = [], [], [], []
    indices = np.full(n, -1, np.int32)
    stats = dict(one_sided=0, parity=0, ties=0, lopsided=0, no_valid=0, level_segments={}, mutated=None)
    kind, left_k = (mutate[0], int(mutate[1])) if mutate else (None, -1)
    zero = np.zeros(d, np.float32)
    leaf_start, max_leaf = 0, leaf_size
    stack = [(np.arange(n, dtype=np.int64), 0, None)]
    while stack:
        ids, depth, patch = stack.pop()
        me, ln = len(nodes), len(ids)
        if patch is not None:
            children[patch[0]][patch[1]] = me
        stats["level_segments"][depth] = stats["level_segments"].get(depth, 0) + 1
        rec = dict(node=me, depth=depth, len=ln, hubs=None, choice=-1, nl=0, counts=[])
        nodes.append(rec)
        choice, left = -1, None
        if ln > leaf_size and max_depth - depth > 0:
            hubs = _hubs(ids, rank)
            rec["hubs"] = [int(h) for h in hubs]
            pairs = [p for p in PAIRS if p[1] < len(hubs)]
            planes = [plane32(x[hubs[a]], x[hubs[b]], angular) for a, b in pairs]
            hs = np.stack([p[0] for p in planes])
            m = margins32(x[ids], hs, [p[1] for p in planes])
            side = sides32(m)
            stats["parity"] += int(((m <= EPS32) & (m >= -EPS32)).sum())
            best, bal_of = np.float32(0.0), []
            for c in range(len(pairs)):
                nl = int((side[:, c] == 0).sum())
                rec["counts"].append(nl)
                if nl == 0 or nl == ln:
                    stats["one_sided"] += 1
                    bal_of.append(None)
                    continue
                bal = _balance32(min(nl, ln - nl), ln)
                bal_of.append(bal)
                if bal > best:
                    best, choice = bal, c
            valid = [c for c in range(len(pairs)) if bal_of[c] is not None]
            if sum(1 for c in valid if bal_of[c] == best) > 1:
                stats["ties"] += 1
            if best < MIN_BALANCE32:
                stats["lopsided"] += 1
                stats["no_valid"] += 0 if valid else 1
                if kind == "split_lopsided" and valid:
                    left_k -= 1
                    if left_k < 0:
                        kind, stats["mutated"] = None, me
                    else:
                        choice = -1
                else:
                    choice = -1
            elif kind == "second_best":
                worse = [c for c in valid if bal_of[c] < best and bal_of[c] >= MIN_BALANCE32]
                if worse:
                    left_k -= 1
                    if left_k < 0:
                        kind, stats["mutated"], choice = None, me, max(worse, key=lambda c: bal_of[c])
            if choice >= 0:
                left = side[:, choice] == 0
                if kind == "move" and min(int(left.sum()), ln - int(left.sum())) >= 2:
                    left_k -= 1
                    if left_k < 0:
                        kind, stats["mutated"] = None, me
                        j = int(np.argmax(np.abs(m[:, choice])))
                        left = left.copy()
                        left[j] = not left[j]
        rec["choice"] = choice
        if choice < 0:
            hyper.append(zero)
            offs.append(np.float32(0.0))
            children.append([-leaf_start, -(leaf_start + ln)])
            indices[leaf_start:leaf_start + ln] = ids
            leaf_start += ln
            max_leaf = max(max_leaf, ln)
            continue
        rec["nl"] = int(left.sum())
        hyper.append(planes[choice][0])
        offs.append(planes[choice][1])
        children.append([-1, -1])
        stack.append((ids[~left], depth + 1, (me, 1)))
        stack.append((ids[left], depth + 1, (me, 0)))
    tree = Tree(np.ascontiguousarray(np.stack(hyper), np.float32), np.asarray(offs, np.float32), np.asarray(children, np.int32).reshape(-1, 2),
                indices, int(max_leaf))
    return HubResult(tree, nodes, stats)


# ------------------------------------------------------------------------------------------------ reading a FlatTree
def layout(tree, n):
    """Per pre-order node of a FlatTree: (depth, a, e, left, right) with [a, e) its slice of ``indices`` and left = -1 for a leaf.
    Returns (rows, None), or (None, (node, reason)) where the tables are not a pre-order tree over n points."""
    ch = np.asarray(tree[2])
    idx = np.asarray(tree[3])
    nn = ch.shape[0]
    if ch.ndim != 2 or ch.shape[1] != 2 or nn < 1 or idx.shape != (n,):
        return None, (0, "table shapes")
    rows = [None] * nn
    counter, leaf_pos = 0, 0
    stack = [(0, 0, -1)]   # (claimed number, depth, parent); a negative claimed number closes node ~number
    while stack:
        me, depth, parent = stack.pop()
        if me < 0:
            rows[~me][2] = leaf_pos
            continue
        if me != counter or me >= nn:
            return None, (max(parent, 0), "children are not numbered in pre-order with the left child next (child %d where %d is due)" % (me, counter))
        counter += 1
        l, r = int(ch[me, 0]), int(ch[me, 1])
        if l <= 0:
            if -l != leaf_pos or -r <= -l or -r > n:
                return None, (me, "a leaf's children are not (-start, -end) of the next slice of indices")
            rows[me] = [depth, leaf_pos, -r, -1, -1]
            leaf_pos = -r
        else:
            if l != me + 1 or r <= l or r >= nn:
                return None, (me, "children (%d, %d) of node %d are not (the next number, a later number)" % (l, r, me))
            rows[me] = [depth, leaf_pos, -1, l, r]
            stack.append((~me, 0, 0))
            stack.append((r, depth + 1, me))
            stack.append((l, depth + 1, me))
    if counter != nn or leaf_pos != n:
        return None, (0, "the tree has %d of %d nodes and %d of %d points" % (counter, nn, leaf_pos, n))
    if not np.array_equal(np.sort(idx), np.arange(n)):
        return None, (0, "indices does not hold every point once")
    return rows, None


def same_tables(a, b):
    """the five tables equal, float tables by their bytes."""
    for p, q in zip(a[:4], b[:4]):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        if p.dtype != q.dtype or p.shape != q.shape or not np.array_equal(p.view(np.uint8), q.view(np.uint8)):
            return False
    return int(a[4]) == int(b[4])


def first_structural_difference(ta, tb, n, stop=()):
    """Walks two FlatTrees together from the root and returns the first node of ``ta`` at which they differ in leaf-or-split or in
    the ids of the left child, or None.  Subtrees under a node of ``ta`` listed in ``stop`` are not compared."""
    ra, ea = layout(ta, n)
    rb, eb = layout(tb, n)
    if ea or eb:
        return dict(node=(ea or eb)[0], reason=(ea or eb)[1])
    stop = set(stop)
    ia, ib = np.asarray(ta[3]), np.asarray(tb[3])
    stack = [(0, 0)]
    while stack:
        a, b = stack.pop()
        if a in stop:
            continue
        da, db = ra[a], rb[b]
        if (da[3] < 0) != (db[3] < 0):
            return dict(node=a, reason="leaf in one tree, split in the other", other=b)
        if da[3] < 0:
            if not np.array_equal(ia[da[1]:da[2]], ib[db[1]:db[2]]):
                return dict(node=a, reason="leaf members differ", other=b)
            continue
        la, lb = ra[da[3]], rb[db[3]]
        if not np.array_equal(np.sort(ia[la[1]:la[2]]), np.sort(ib[lb[1]:lb[2]])):
            return dict(node=a, reason="left children differ", other=b)
        stack.append((da[4], db[4]))
        stack.append((da[3], db[3]))
    return None


# ------------------------------------------------------------------------------------------------ check
class _Rows64:
    def __init__(self, data, angular, exact):
        x32 = np.ascontiguousarray(data, np.float32)
        self.x32, self.x = x32, x32.astype(np.float64)
        self.n, self.d = self.x.shape
        self.angular, self.exact = bool(angular), bool(exact)
        if exact:
            assert not angular, "lattice: the euclidean branch only"
            r = float(np.abs(self.x).max()) if self.x.size else 0.0
            assert np.array_equal(self.x, np.rint(self.x)) and 8 * self.d * r * r < 2 ** 24, "lattice: integer rows, 8 d R^2 < 2^24"

    def plane(self, il, ir):
        """A candidate: dict(h, off, zero, N, lh, rh) in float64."""
        l, r = self.x[il], self.x[ir]
        if not self.angular:
            v = l - r
            return dict(h=v, off=-0.5 * float(v @ (l + r)), B=0.5 * float(np.abs(v) @ np.abs(l + r)), zero=not v.any(), wild=False)
        ln, rn = float(np.sqrt(l @ l)), float(np.sqrt(r @ r))
        wild = 0.0 < ln < 2 * EPS or 0.0 < rn < 2 * EPS
        lh, rh = l / (ln if ln >= EPS else 1.0), r / (rn if rn >= EPS else 1.0)
        v = lh - rh
        nn = float(np.sqrt(v @ v))
        if nn == 0.0:
            return dict(h=v, off=0.0, zero=True, wild=wild, N=1.0, lh=lh, rh=rh)
        return dict(h=v / nn, off=0.0, zero=False, wild=wild, N=nn, lh=lh, rh=rh)

    def margins(self, p, xm):
        """(m64, radius) of the float64 rows xm against the candidate p."""
        k = xm.shape[0]
        if p["wild"]:
            return xm @ p["h"] + p["off"], np.full(k, np.inf)
        if p["zero"]:
            return np.zeros(k), np.zeros(k)
        d, h, ax = self.d, p["h"], np.abs(xm)
        m = xm @ h + p["off"]
        if self.exact:
            return m, np.zeros(k)
        a = ax @ np.abs(h)
        if not self.angular:
            return m, ((d + 8) * a + (2 * d + 8) * p["B"]) * U24
        am, rho = np.abs(m), (d / 2.0 + 2.0) * U24
        rad = (d + 8) * U24 * a + rho * am
        for q in (p["lh"], p["rh"]):
            rad = rad + (rho * np.abs(xm @ q - m * float(h @ q)) + 2 * U24 * (ax @ np.abs(q) + am * float(np.abs(h) @ np.abs(q)))) / p["N"]
        return m, rad

    def is_plane(self, p, il, ir, h_gpu, off_gpu):
        """whether the GPU's hyperplane row and offset are this candidate's."""
        h_gpu = np.asarray(h_gpu, np.float64)
        if not self.angular:
            if not np.array_equal(h_gpu, (self.x32[il] - self.x32[ir]).astype(np.float64)):
                return False
            tol = 0.0 if self.exact else (self.d + 8) * U24 * p["B"]
            return abs(float(off_gpu) - p["off"]) <= tol
        if float(off_gpu) != 0.0:
            return False
        want, rad = self.margins(p, np.eye(self.d))
        return bool(np.all(np.abs(h_gpu - want) <= rad))


def _emin(lo, hi, ln):
    """the smallest min(nl, nr) a candidate can have with nl in [lo, hi]; 0 stands for a one-sided (skipped) candidate."""
    def e(k):
        return 0 if k in (0, ln) else min(k, ln - k)
    return min(e(lo), e(hi))


def check(data, neighbor_indices, leaf_size, max_depth, metric, tree, exact=False):
    """The verdict on a FlatTree ``tree`` (any 5-tuple of the tables) for this input; see the module text."""
    R = _Rows64(data, ANGULAR[metric], exact)
    n, d = R.n, R.d
    leaf_size, max_depth = max(int(leaf_size), 1), int(max_depth)
    hyper, offs, idx = np.asarray(tree[0]), np.asarray(tree[1]), np.asarray(tree[3]).astype(np.int64)
    mismatch, unclear_nodes = [], set()
    decisions = unclear = 0
    rows, err = layout(tree, n)
    if err:
        return CheckResult([dict(node=err[0], depth=-1, len=-1, hubs=None, candidate=None, reason=err[1], members=[])], 0, 0, set())
    if hyper.shape != (len(rows), d) or offs.shape != (len(rows),):
        return CheckResult([dict(node=0, depth=0, len=n, hubs=None, candidate=None, reason="table shapes", members=[])], 0, 0, set())
    rank = _ranks(neighbor_indices, n)

    def fail(me, reason, hubs=None, cand=None, members=()):
        depth, a, e = rows[me][:3]
        mismatch.append(dict(node=me, depth=depth, len=e - a, hubs=hubs, candidate=cand, reason=reason, members=list(members)[:8]))

    largest = (leaf_size, -1)
    for me, (depth, a, e, lc, rc) in enumerate(rows):
        ln = e - a
        ids = np.sort(idx[a:e])
        splittable = ln > leaf_size and max_depth - depth > 0
        if lc < 0:
            if ln > largest[0]:
                largest = (ln, me)
            if not np.array_equal(idx[a:e], ids):
                fail(me, "the leaf's ids are not in ascending order")
            if hyper[me].any() or offs[me] != 0:
                fail(me, "a leaf's hyperplane row and offset are not zero")
        elif not splittable:
            fail(me, "the node splits although len <= leaf_size (%d) or max_depth (%d) is exhausted" % (leaf_size, max_depth))
            continue
        if not splittable:
            continue
        hubs = _hubs(ids, rank)
        hub_list = [int(h) for h in hubs]
        pairs = [p for p in PAIRS if p[1] < len(hubs)]
        xm = R.x[ids]
        par = np.arange(ln) & 1
        cands = []
        for hi_, hj_ in pairs:
            p = R.plane(hubs[hi_], hubs[hj_])
            m, rad = R.margins(p, xm)
            cl, cr, cc = m > EPS + rad, m < -EPS - rad, np.abs(m) <= EPS - rad
            want = np.where(cl, 0, np.where(cr, 1, par))     # the side of every clear member
            clear = cl | cr | cc
            decisions += ln
            nu = int((~clear).sum())
            unclear += nu
            if nu:
                unclear_nodes.add(me)
            lo = int((clear & (want == 0)).sum())
            cands.append(dict(p=p, m=m, rad=rad, want=want, clear=clear, lo=lo, hi=lo + nu, pair=(int(hubs[hi_]), int(hubs[hj_]))))
        if lc < 0:   # a leaf by the balance rule: no candidate may be sure of a balance >= 0.1
            for c, q in enumerate(cands):
                k = _emin(q["lo"], q["hi"], ln)
                if not _balance32(k, ln) < MIN_BALANCE32:
                    fail(me, "a leaf although candidate %d has a valid balance of at least %d / %d >= 0.1" % (c, k, ln), hub_list, c)
                    break
            continue
        gl = np.zeros(n, bool)
        la, le = rows[lc][1], rows[lc][2]
        gl[idx[la:le]] = True
        gside = np.where(gl[ids], 0, 1)
        nl = le - la
        bc = min(nl, ln - nl)
        match = [c for c, q in enumerate(cands) if R.is_plane(q["p"], q["pair"][0], q["pair"][1], hyper[me], offs[me])]
        if not match:
            fail(me, "the hyperplane is none of the node's candidates %s" % [q["pair"] for q in cands], hub_list)
            continue
        reports = []
        for c in match:
            q = cands[c]
            bad = q["clear"] & (q["want"] != gside)
            if bad.any():
                sel = np.flatnonzero(bad)
                reports.append((c, "clear members lie on the other side of candidate %d than the tree puts them" % c,
                                [(int(ids[i]), int(i), float(q["m"][i]), float(q["rad"][i]), int(gside[i])) for i in sel]))
                continue
            if _balance32(bc, ln) < MIN_BALANCE32:
                reports.append((c, "the node splits although its balance %d / %d is below 0.1" % (bc, ln), []))
                continue
            beaten = None
            for c2, q2 in enumerate(cands):
                k = _emin(q2["lo"], q2["hi"], ln)
                if c2 != c and c2 not in match and (k >= bc if c2 < c else k > bc):
                    beaten = (c2, k)
                    break
            if beaten:
                reports.append((c, "candidate %d is chosen with balance %d / %d although candidate %d has at least %d / %d"
                                % (c, bc, ln, beaten[0], beaten[1], ln), []))
                continue
            reports = None
            break
        if reports:
            c, reason, members = reports[0]
            fail(me, reason, hub_list, c, members)
    if int(tree[4]) != largest[0]:
        fail(max(largest[1], 0), "leaf_size is %d, the largest leaf (or the given leaf_size) is %d" % (int(tree[4]), largest[0]))
    return CheckResult(mismatch, decisions, unclear, unclear_nodes)


def describe(mis):
    """one line per mismatch."""
    return "\n".join("node %(node)d depth %(depth)d len %(len)d hubs %(hubs)s candidate %(candidate)s: %(reason)s; members (id, offset, m64, "
                     "radius, side in the tree) %(members)s" % m for m in mis)
