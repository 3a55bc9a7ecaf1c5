"""The shapes at which the hub search tree is compared with tests/hubtree_reference.py: the smallest at which each path of
csrc/hubtree.hip can go wrong.  Shared by tests/test_hubtree_reference_cpu.py, tests/test_gpu_hubtree_exact.py and the generator of
tests/golden/hub_tree_edges.npz.

A case is the rows, a synthetic neighbour graph, leaf_size, max_depth and the metric.  The graph is built directly -- the tree reads
nothing of it but the in-degrees -- so a case chooses its hubs by choosing degrees and needs no NN-descent build.
"""
import functools
from collections import namedtuple

import numpy as np

from tests.util_data import clustered

UNCLEAR_CAP = 1e-3   # at most 1 in 1000 (member, node, candidate) decisions of a case may be unclear: a condition on the case, not a
                     # tolerance (the same cap and meaning as tests/forest_cases.py)
K = 10               # columns of the synthetic graphs

Case = namedtuple("Case", "name x nbr leaf_size max_depth metric exact")


# ------------------------------------------------------------------------------------------------ graphs
def graph(n, seed, hubs=(), holes=False, k=K, spread=None):
    """(n, k) int32 neighbour ids drawn from ``spread`` ids (default n: binomial in-degrees with many ties; fewer: the rest has
    in-degree 0).  ``hubs``: ids in the order of their rank; they get the largest in-degrees, strictly descending.  ``holes``: a
    tenth of the entries is -1 and some are n, n + 7 or 2^31 - 1 (all skipped by the degree count)."""
    rs = np.random.RandomState(seed)
    pool = np.arange(n) if spread is None else rs.choice(n, spread, replace=False)
    g = pool[rs.randint(0, len(pool), (n, k))].astype(np.int32)
    if holes:
        g[rs.uniform(size=g.shape) < 0.1] = -1
        flat = g.reshape(-1)
        flat[rs.choice(flat.size, 9, replace=False)] = np.array([n, n, n + 7, n + 7, 2 ** 31 - 1, n, -5, n + 1, -2 ** 31], np.int32)
    hubs = list(hubs)
    if hubs:
        assert len(set(hubs)) == len(hubs)
        g[np.isin(g, hubs)] = -1
        top = int(np.bincount(g[(g >= 0) & (g < n)].ravel(), minlength=n).max())
        want = [top + 2 * (len(hubs) - i) for i in range(len(hubs))]
        assert sum(want) <= n * (k - 1)
        col = np.concatenate([np.full(w, h, np.int32) for h, w in zip(hubs, want)])
        rows = rs.permutation(n * (k - 1))[:len(col)]      # the last column keeps the drawn entries
        g[rows // (k - 1), rows % (k - 1)] = col
    return np.ascontiguousarray(g)


# ------------------------------------------------------------------------------------------------ lattice rows (euclidean, exact)
def lattice(n, d, seed, lo=-2, hi=2, blocks=False):
    """integer rows in {lo..hi}^d; ``blocks``: runs of 3 to 6 identical rows, shuffled."""
    rs = np.random.RandomState(seed)
    if blocks:
        rows, left = [], n
        while left > 0:
            g = min(int(rs.randint(3, 7)), left)
            rows.append(np.repeat(rs.randint(lo, hi + 1, (1, d)), g, 0))
            left -= g
        x = np.concatenate(rows)[rs.permutation(n)]
    else:
        x = rs.randint(lo, hi + 1, (n, d))
    return np.ascontiguousarray(x, np.float32)


def _tie_root(seed):
    """Root hubs (0,0,z), (2,0,z), (0,2,z) over the four corners {0,2}^2, 80 rows each: candidates (0,1) and (0,2) cut x < 1 and
    y < 1, 160 / 320 each: a tie at the largest balance there is, the first wins.  (1,2) cuts x > y with the 160 diagonal rows on the
    plane, split by parity: no better than the two."""
    rs = np.random.RandomState(seed)
    n = 320
    corners = np.array([[0, 0], [2, 0], [0, 2], [2, 2]])
    x = np.concatenate([corners[rs.permutation(np.repeat(np.arange(4), n // 4))], rs.randint(-1, 2, (n, 1))], 1).astype(np.float32)
    hubs = [int(np.flatnonzero((x[:, 0] == a) & (x[:, 1] == b))[3]) for a, b in ((0, 0), (2, 0), (0, 2))]
    return x, graph(n, seed, hubs)


def _balance_root(n_small, seed):
    """Root hubs H0 = origin cluster, H1 = (6,0,0), H2 = (6,4,0): candidates (0,1) and (0,2) cut the ``n_small`` rows at the origin off
    the 300 (n_small / 300 each: 30 is exactly 10 %, 29 is just below), (1,2) cuts y < 2: H2 alone."""
    rs = np.random.RandomState(seed)
    n = 300
    a = rs.randint(-1, 2, (n_small, 3))
    b = np.stack([rs.randint(6, 10, n - n_small), np.zeros(n - n_small, np.int64), rs.randint(-1, 2, n - n_small)], 1)
    b[0], b[1] = (6, 0, 0), (6, 4, 0)
    x = np.concatenate([a, b]).astype(np.float32)
    perm = rs.permutation(n)
    x = x[perm]
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    return np.ascontiguousarray(x), graph(n, seed, [int(where[0]), int(where[n_small]), int(where[n_small + 1])], holes=True)


def _outlier_hubs(seed):
    """Root: G0 = (-40,0,0) against G1 = (40,0,0) halves the set.  The left half then has the hubs G0, (-44,0,0), (-48,0,0), all beyond
    its bulk at x in [-12, -8]: every candidate cuts off at most two of 150, the node stays a leaf of 150 > leaf_size."""
    rs = np.random.RandomState(seed)
    half = 150
    p = np.concatenate([rs.randint(-12, -7, (half, 1)), rs.randint(-2, 3, (half, 2))], 1)
    q = np.concatenate([rs.randint(8, 13, (half, 1)), rs.randint(-2, 3, (half, 2))], 1)
    p[0], p[1], p[2], q[0] = (-40, 0, 0), (-44, 0, 0), (-48, 0, 0), (40, 0, 0)
    x = np.concatenate([p, q]).astype(np.float32)
    perm = rs.permutation(2 * half)
    where = np.empty(2 * half, np.int64)
    where[perm] = np.arange(2 * half)
    return np.ascontiguousarray(x[perm]), graph(2 * half, seed, [int(where[0]), int(where[half]), int(where[1]), int(where[2])])


# ------------------------------------------------------------------------------------------------ float rows
def _angular_rows(metric, d, seed, n=2000):
    """n rows for the angular branch: two zero rows (one of them the third hub), a pair of collinear hubs (the two highest
    in-degrees: identical rows for dot, whose rows are unit length, else one is twice the other) and a block of five identical rows."""
    rs = np.random.RandomState(seed)
    x = clustered(n, d, 6, 30, seed=seed, nonneg=metric == "hellinger")
    if metric == "dot":
        x = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    ids = rs.choice(n, 9, replace=False)
    h0, h1, z0, z1 = (int(i) for i in ids[:4])
    x[h1] = x[h0] if metric == "dot" else x[h0] * np.float32(2.0)
    x[z0] = 0.0
    x[z1] = 0.0
    x[ids[4:]] = x[ids[4]]
    return np.ascontiguousarray(x), graph(n, seed, [h0, h1, z0], holes=True)


def _offset_pairs(seed, n=2000, pairs=8):
    """Rows on a large common offset, leaf_size 1, with ``pairs`` rows that have a twin one float32 step away in some coordinates.  A
    twin pair ends as a node of two whose true margins (half the squared distance, about 1e-7) are smaller than the float32 error of
    h . x + off at this offset, so both members can land on one side of the only candidate: the node has no valid candidate and stays a
    leaf of 2 > leaf_size."""
    rs = np.random.RandomState(seed)
    d = 4
    x = (4096.0 + 128.0 * rs.standard_normal((n, d))).astype(np.float32)
    ids = rs.choice(n, 2 * pairs, replace=False)
    step = rs.randint(-1, 2, (pairs, d)).astype(np.float32) * np.float32(2.0 ** -11)   # (the float32 spacing in [4096, 8192); two steps below 4096)
    x[ids[pairs:]] = x[ids[:pairs]] + step
    return np.ascontiguousarray(x, np.float32), graph(n, seed)


# ------------------------------------------------------------------------------------------------ the table
def _lat(name, n, d, seed, leaf_size, max_depth=200, holes=False, spread=None, **kw):
    return name, lambda: Case(name, lattice(n, d, seed, **kw), graph(n, seed, holes=holes, spread=spread), leaf_size, max_depth, "euclidean", True)


def _made(name, make, leaf_size, metric="euclidean", exact=False, max_depth=200):
    def build():
        x, g = make()
        return Case(name, x, g, leaf_size, max_depth, metric, exact)
    return name, build


def _float(name, n, d, leaf_size, metric="euclidean", seed=None):
    seed = n + d if seed is None else seed
    return name, lambda: Case(name, clustered(n, d, min(d, 6), 30, seed=seed), graph(n, seed, holes=d % 2 == 1), leaf_size, 200, metric, False)


_TABLE = [
    # ---- lattice, euclidean, exact: every decision is clear, the tree is pinned outright
    _lat("lat-d1-leaf1", 300, 1, 11, 1, lo=-20, hi=20),                    # nodes of 2 and 3; runs of equal values: all-identical subtrees
    _lat("lat-d3-leaf1", 400, 3, 12, 1, holes=True, spread=150),           # 125 distinct rows among 400; degree 0 for most points
    _lat("lat-d4-blocks", 600, 4, 13, 5, holes=True, blocks=True),         # blocks of identical rows; -1 and >= n graph entries
    _lat("lat-d33", 1000, 33, 14, 30),                                     # the default leaf_size; d over a 32-boundary
    _made("lat-tie-root", lambda: _tie_root(15), 30, exact=True),          # two candidates of equal (and best) balance at the root
    _made("lat-balance-exact", lambda: _balance_root(30, 16), 10, exact=True),   # best split exactly 10 %: splits
    _made("lat-balance-below", lambda: _balance_root(29, 16), 10, exact=True),   # 29 / 300: the root is a leaf of 300
    _made("lat-outlier-hubs", lambda: _outlier_hubs(17), 10, exact=True),        # every candidate lopsided one level down
    _lat("lat-depth0", 300, 4, 18, 5, max_depth=0),
    _lat("lat-depth1", 300, 4, 18, 5, max_depth=1),
    _lat("lat-depth3", 300, 4, 18, 5, max_depth=3),
    _lat("lat-one-leaf", 30, 4, 19, 30),                                   # n = leaf_size: the root is a leaf
    _lat("lat-leaf+1", 31, 4, 19, 30),
    # ---- more than 256 segments on a level: k_hub_children's chunks and prefix sums
    _float("segments-n4096", 4096, 8, 3),
    # ---- waves inside one segment, and waves that straddle segment boundaries
    _float("waves-leaf5", 3000, 24, 5, seed=3031),          # (the seed: splitting segments of exactly 64, one on a wave boundary, two off it)
    _float("waves-leaf200", 3000, 24, 200),
    # ---- dimension edges
    _float("d1", 1500, 1, 30), _float("d5", 1500, 5, 30), _float("d17", 1500, 17, 30), _float("d64", 1500, 64, 30),
    _float("d127", 1500, 127, 30), _float("d130", 1500, 130, 30),
    # ---- the angular branch on raw rows
    _made("cosine-d16", lambda: _angular_rows("cosine", 16, 31), 30, "cosine"),
    _made("cosine-d33", lambda: _angular_rows("cosine", 33, 32), 30, "cosine"),
    _made("dot-d16", lambda: _angular_rows("dot", 16, 33), 30, "dot"),
    _made("dot-d33", lambda: _angular_rows("dot", 33, 34), 30, "dot"),
    _made("correlation-d16", lambda: _angular_rows("correlation", 16, 35), 30, "correlation"),
    _made("correlation-d33", lambda: _angular_rows("correlation", 33, 36), 30, "correlation"),
    _made("hellinger-d16", lambda: _angular_rows("hellinger", 16, 37), 30, "hellinger"),
    _made("hellinger-d33", lambda: _angular_rows("hellinger", 33, 38), 30, "hellinger"),
    # ---- float rows small enough for the un-jitted reference (at most 1000 points): both branches in rounded arithmetic
    _float("float-n800-d17", 800, 17, 10),
    _made("cosine-n600-d16", lambda: _angular_rows("cosine", 16, 39, n=600), 10, "cosine"),
    _made("hellinger-n600-d33", lambda: _angular_rows("hellinger", 33, 40, n=600), 10, "hellinger"),
    # ---- inner_product: the euclidean branch under another metric code
    _float("inner-product", 1500, 24, 30, "inner_product"),
    # ---- the one-sided-candidate branch
    _made("offset-pairs", lambda: _offset_pairs(41), 1),
]
_BUILD = dict(_TABLE)
NAMES = [name for name, _ in _TABLE]
LATTICE = [name for name in NAMES if name.startswith("lat-")]
ANGULAR = [name for name in NAMES if name.split("-")[0] in ("cosine", "dot", "correlation", "hellinger")]
DEVICE_ENTRY = ["lat-d4-blocks", "segments-n4096", "cosine-d33"]   # also run with the graph and the rank order on the device


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILD[name]()
    for a in (c.x, c.nbr):
        a.setflags(write=False)
    return c


def small():
    """the cases the un-jitted reference is run on: at most 1000 points."""
    return [name for name in NAMES if case(name).x.shape[0] <= 1000]


def reference_tables(c):
    """make_hub_tree + convert_tree_format of the reference, run un-jitted (oracle/ref_t0.py), on a case: the five FlatTree tables."""
    from oracle import ref_t0
    ref_t0.load_reference()
    from pynndescent import rp_trees as R
    from tests.hubtree_reference import ANGULAR as IS_ANGULAR
    x, nbr = np.array(c.x), np.array(c.nbr)
    tree = R.make_hub_tree(x, nbr, np.array([1, 2, 3], np.int64), leaf_size=c.leaf_size, angular=IS_ANGULAR[c.metric], max_depth=c.max_depth)
    flat = R.convert_tree_format(tree, x.shape[0], x.shape[1])
    return (np.asarray(flat.hyperplanes, np.float32), np.asarray(flat.offsets, np.float32), np.asarray(flat.children, np.int32),
            np.asarray(flat.indices, np.int32), int(flat.leaf_size))
