"""Seeded inputs for the step-exact search tests (tests/test_search_reference_cpu.py, tests/test_gpu_search_exact.py):
data, CSR graph, handcrafted FlatTree, queries and settings per case, and the reference walk on them (cached per process).

Lattice cases: integer data and queries with sum over the columns of (largest |q_j - x_j|)^2 < 2^24, so every float32 sum
of the kernel is exact.  Float cases: loose Gaussian clusters (noise as large as the spread of the centres), which keeps
the share of queries with a float32-ambiguous decision small for the angular metrics."""
import functools
import types

import numpy as np

from pynndescent_amd.search_tree import FlatTree
from tests import search_reference as SR

RNG_STATE = np.array([1234567, -7654321, 424242], np.int64)
LATTICE_CAP, FLOAT_CAP = 0.05, 0.10  # largest share of ambiguous queries a case may have


# ------------------------------------------------------------------------------------------------ builders
def lattice_points(n, d, R, seed, latent=None):
    """Integer points with |v| <= R: uniform, or (latent given) a random linear image of a uniform latent cube whose
    columns each use the whole range -R .. R, so the squared distances spread over as many integers as the lattice allows."""
    rs = np.random.RandomState(seed)
    if latent is None or latent >= d:
        return rs.randint(-R, R + 1, size=(n, d)).astype(np.float32)
    proj = rs.standard_normal((latent, d))
    proj /= np.abs(proj).sum(0, keepdims=True)
    return np.rint(R * (rs.uniform(-1.0, 1.0, size=(n, latent)) @ proj)).astype(np.float32)


def lattice_ok(data, queries, rows=None):
    """The lattice condition for these inputs: the largest possible sum of squared differences is below 2^24."""
    rows = data if rows is None else rows
    span = np.maximum(np.abs(queries.max(0) - rows.min(0)), np.abs(rows.max(0) - queries.min(0))).astype(np.float64)
    whole = np.all(data == np.rint(data)) and np.all(queries == np.rint(queries))
    return bool(whole and float((span * span).sum()) < 2.0 ** 24)


def top_neighbours(score, knn):
    """Ids of the knn largest scores per row, self excluded, best first."""
    s = np.array(score, np.float64)
    np.fill_diagonal(s, -np.inf)
    part = np.argpartition(-s, knn, axis=1)[:, :knn]
    order = np.argsort(-np.take_along_axis(s, part, 1), axis=1, kind="stable")
    return np.take_along_axis(part, order, 1)


def euclid_neighbours(x, knn, block=2000):
    x = x.astype(np.float64)
    n2 = (x * x).sum(1)
    out = np.empty((x.shape[0], knn), np.int64)
    for a in range(0, x.shape[0], block):
        s = 2.0 * x[a:a + block] @ x.T - n2[None, :]
        s[np.arange(s.shape[0]), np.arange(a, a + s.shape[0])] = -np.inf
        part = np.argpartition(-s, knn, axis=1)[:, :knn]
        order = np.argsort(-np.take_along_axis(s, part, 1), axis=1, kind="stable")
        out[a:a + block] = np.take_along_axis(part, order, 1)
    return out


def csr_from_rows(rows):
    indptr = np.zeros(len(rows) + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, np.int32) for r in rows]) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, indices.astype(np.int32)


def symmetric_rows(nbr):
    """Adjacency rows of the symmetrised k-NN graph: a row's own neighbours in order, then its reverse neighbours."""
    n = nbr.shape[0]
    rows = [list(r) for r in nbr.tolist()]
    have = [set(r) for r in rows]
    for i in range(n):
        for j in nbr[i].tolist():
            if i not in have[j]:
                have[j].add(i)
                rows[j].append(i)
    return rows


def kd_tree(points, leaf_size):
    """FlatTree in the searcher's format (internal node: two positive child numbers; leaf: (-start, -end) into
    ``indices``) with axis-aligned hyperplanes: entry 1 in the widest column j and offset -t, t between the two middle
    values of that column (integer data: t = v + 0.5, so no margin is ever 0).  Side 0 holds the values above t."""
    points = np.asarray(points, np.float32)
    n, d = points.shape
    hyper, offs, children, order = [], [], [], []

    def build(ids):
        node = len(hyper)
        hyper.append(np.zeros(d, np.float32))
        offs.append(np.float32(0.0))
        children.append([0, 0])
        split = None
        if len(ids) > leaf_size:
            sub = points[ids]
            for j in np.argsort(-(sub.max(0) - sub.min(0)), kind="stable"):
                v = np.sort(sub[:, j])
                cuts = np.nonzero(v[1:] > v[:-1])[0]  # a cut after position c separates v[c] from v[c + 1]
                if len(cuts) == 0:
                    break
                c = cuts[np.argmin(np.abs(cuts + 1 - len(v) / 2.0))]
                t = np.float32((np.float64(v[c]) + np.float64(v[c + 1])) / 2.0)
                if v[c] <= t < v[c + 1]:
                    split = (int(j), t)
                    break
        if split is None:
            children[node] = [-len(order), -(len(order) + len(ids))]
            order.extend(ids.tolist())
            return node
        j, t = split
        hyper[node][j] = 1.0
        offs[node] = np.float32(-t)
        above = points[ids, j] > t
        c0 = build(ids[above])
        c1 = build(ids[~above])
        children[node] = [c0, c1]
        return node

    build(np.arange(n))
    return FlatTree(np.array(hyper, np.float32), np.array(offs, np.float32), np.array(children, np.int32), np.array(order, np.int32), leaf_size)


def column_tree(col, sizes, d):
    """FlatTree over the DISTINCT integer values ``col`` of column 0 whose leaves, in ascending order of that column,
    have exactly the given sizes."""
    order = np.argsort(col, kind="stable")
    assert sum(sizes) == len(col) and len(np.unique(col)) == len(col)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    hyper, offs, children = [], [], []

    def build(a, b):  # leaves a .. b - 1
        node = len(hyper)
        hyper.append(np.zeros(d, np.float32))
        offs.append(np.float32(0.0))
        children.append([0, 0])
        if b - a == 1:
            children[node] = [-int(starts[a]), -int(starts[b])]
            return node
        m = (a + b) // 2
        t = float(col[order[starts[m] - 1]]) + 0.5  # the largest value of the lower half, plus a half
        hyper[node][0] = 1.0
        offs[node] = np.float32(-t)
        c0 = build(m, b)  # margin > 0: the upper half
        c1 = build(a, m)
        children[node] = [c0, c1]
        return node

    build(0, len(sizes))
    return FlatTree(np.array(hyper, np.float32), np.array(offs, np.float32), np.array(children, np.int32), order.astype(np.int32), max(sizes))


def near_queries(x, nq, spread, R, seed):
    """Integer queries: data points moved by up to ``spread`` per column, kept within +-R."""
    rs = np.random.RandomState(seed)
    q = x[rs.choice(x.shape[0], nq, replace=False)] + rs.randint(-spread, spread + 1, size=(nq, x.shape[1]))
    return np.clip(q, -R, R).astype(np.float32)


def case(name, data, rows, tree, queries, k, epsilon, n_neighbors, metric="sqeuclidean", min_distance=64.0, exact=True, **extra):
    indptr, indices = rows if isinstance(rows, tuple) else csr_from_rows(rows)
    c = types.SimpleNamespace(name=name, data=np.ascontiguousarray(data, np.float32), indptr=indptr, indices=indices, tree=tree,
                              queries=np.ascontiguousarray(queries, np.float32), k=k, epsilon=epsilon, n_neighbors=n_neighbors,
                              metric=metric, min_distance=float(np.float32(min_distance)), exact=exact, rng_state=RNG_STATE,
                              values=None, search_k=None)
    c.__dict__.update(extra)
    return c


# ------------------------------------------------------------------------------------------------ lattice worlds
@functools.lru_cache(maxsize=None)
def _world(n=6000, d=16, R=500, seed=1, knn=15, latent=None):
    x = lattice_points(n, d, R, seed, latent)
    return x, symmetric_rows(euclid_neighbours(x, knn))


@functools.lru_cache(maxsize=None)
def _world_tree(leaf, *world):
    return kd_tree(_world(*world)[0], leaf)


WIDTHS = (1, 10, 63, 64, 65, 128, 129, 200, 256)
EPSILONS = (0.0, 0.125, 0.25, 1.0)


WIDTH_WORLD = (500, 16, 500, 2, 15, 2)  # few points with a wide spread of distances: few exact ties at a pop


def _width_case(k, nn):
    """epsilon = 1 goes with the short lists (a wide search pops hundreds of vertices, and on a lattice of 2^24 distance
    values two of hundreds of live keys tie too often); the long lists cycle through 0, 1/8 and 1/4."""
    x, rows = _world(*WIDTH_WORLD)
    eps = 1.0 if k <= 10 else EPSILONS[(WIDTHS.index(k) + (nn == 30)) % 3]
    return case("width_k%d_nn%d" % (k, nn), x, rows, _world_tree(12, *WIDTH_WORLD), near_queries(x, 40, 60, 500, 100 + k + nn), k, eps, nn)


def _hub_case():
    x, rows = _world()
    rows = [list(r) for r in rows]
    hubs = (11, 2222, 4444)
    far = euclid_neighbours(x[:], 300)
    for h, width in zip(hubs, (65, 128, 300)):
        rows[h] = far[h][:width].tolist()
    rs = np.random.RandomState(5)
    q = near_queries(x, 30, 60, 500, 6)
    q[:15] = np.clip(x[np.repeat(hubs, 5)] + rs.randint(-20, 21, size=(15, 16)), -500, 500)
    return case("graph_hub_rows", x, rows, _world_tree(30), q, 10, 0.25, 15)


def _ragged_case():
    x, rows = _world()
    rows = [list(r) for r in rows]
    for v in range(len(rows)):
        if v % 7 == 0:
            rows[v] = []
        elif v % 5 == 0:
            rows[v] = [v] + rows[v]
        elif v % 11 == 0:
            rows[v] = rows[v] + [rows[v][0]]
    return case("graph_empty_self_duplicate", x, rows, _world_tree(30), near_queries(x, 40, 60, 500, 8), 10, 0.125, 15)


def _island_case(k):
    x = lattice_points(1200, 16, 500, 21)
    tree = kd_tree(x, 12)
    rows = [None] * 1200
    for a in range(0, 1200, 24):  # 24 consecutive points of the tree order: fully connected, no edge to the outside
        grp = tree.indices[a:a + 24].tolist()
        for v in grp:
            rows[v] = [u for u in grp if u != v]
    return case("graph_islands_k%d" % k, x, rows, tree, near_queries(x, 30, 60, 500, 22), k, 0.125, 10)


def _ring_case(k):
    x = lattice_points(500, 16, 500, 31)
    rows = (np.arange(501, dtype=np.int32), ((np.arange(500) + 1) % 500).astype(np.int32))
    return case("graph_ring_k%d" % k, x, rows, None, near_queries(x, 30, 60, 500, 32), k, 1.0, 10)


LEAF_SIZES = (1, 30, 64, 65, 200, 1, 30, 64, 65, 200, 100, 180)


def _leaf_case(k, nn, eps):
    rs = np.random.RandomState(41)
    x = lattice_points(1000, 16, 500, 42)
    x[:, 0] = rs.permutation(np.arange(-500, 500))
    tree = column_tree(x[:, 0], LEAF_SIZES, 16)
    starts = np.concatenate([[0], np.cumsum(LEAF_SIZES)])
    q = []
    for a, b in zip(starts[:-1], starts[1:]):  # three queries that descend to every leaf
        for t in range(3):
            p = x[tree.indices[a + (t * 7) % (b - a)]].copy()
            p[1:] = np.clip(p[1:] + rs.randint(-40, 41, size=15), -500, 500)
            q.append(p)
    return case("tree_leaves_k%d_nn%d" % (k, nn), x, symmetric_rows(euclid_neighbours(x, 15)), tree, np.array(q), k, eps, nn,
                leaf_sizes=LEAF_SIZES)


def _single_leaf_case():
    x = lattice_points(150, 16, 500, 51)
    tree = kd_tree(x, 150)
    assert tree.children.shape == (1, 2)
    return case("tree_single_leaf", x, symmetric_rows(euclid_neighbours(x, 8)), tree, near_queries(x, 30, 60, 500, 52), 10, 0.125, 15)


def _no_tree_case():
    x, rows = _world()
    return case("tree_none", x, rows, None, near_queries(x, 40, 60, 500, 53), 10, 0.25, 15)


def _tiny_leaf_case():
    x = lattice_points(40, 16, 500, 61)
    return case("tree_tiny_leaves_repeated_draws", x, symmetric_rows(euclid_neighbours(x, 5)), kd_tree(x, 2),
                near_queries(x, 30, 60, 500, 62), 30, 0.25, 30)


def _dim_case(d):
    R = {4: 1000, 17: 480, 130: 170, 1000: 60}[d]
    n = 1500 if d == 1000 else 3000
    world = (n, d, R, 70 + d, 15, None if d == 4 else 6)
    x, rows = _world(*world)
    return case("dim_%d" % d, x, rows, _world_tree(30, *world), near_queries(x, 40, max(2, R // 10), R, 71 + d), 10, 0.125, 15)


@functools.lru_cache(maxsize=None)
def _routing_world():
    """20 000 points in 250 well separated clusters of 80.  A row holds the 14 nearest neighbours; every fourth vertex is a
    gateway whose row goes on with 250 vertices from anywhere.  A search pops about as many vertices as lie below its
    bound (few: one cluster), yet visits thousands through the gateways -- wide enough to leave the LDS tier without the
    hundreds of pops that make exact ties likely."""
    rs = np.random.RandomState(81)
    centres = rs.randint(-350, 351, size=(250, 16))
    x = (np.repeat(centres, 80, axis=0) + rs.randint(-100, 101, size=(20000, 16))).astype(np.float32)
    near = euclid_neighbours(x, 14)
    rows = [r for r in near.tolist()]
    for v in range(0, 20000, 4):
        rows[v] = rows[v] + rs.randint(0, 20000, size=250).tolist()
    return x, csr_from_rows(rows), kd_tree(x, 30)


def _routing_case(kind):
    """One searcher, two settings: small searches that must stay on the LDS tier, wide ones that must leave it."""
    x, rows, tree = _routing_world()
    q = near_queries(x, 40, 60, 500, 82)
    if kind == "small":
        return case("routing_small", x, rows, tree, q, 10, 0.125, 10)
    return case("routing_wide", x, rows, tree, q[:20], 64, 1.0, 10)


def _compaction_case():
    """The LDS frontier (512 slots) fills with entries that the shrinking bound has made stale, so the compaction runs
    (several times), while far fewer than 512 entries are ever live and fewer than 3400 vertices are visited: the query
    stays on the LDS tier.  A one-point leaf holds a hub whose row lists 2600 vertices from the farthest to the nearest
    (as seen from the hub): almost every one of them beats the worst entry so far and is pushed; the other rows are a ring."""
    rs = np.random.RandomState(92)
    x = lattice_points(3000, 16, 500, 91, latent=2)
    far_first = np.argsort(-((x[1:].astype(np.float64) - x[0].astype(np.float64)) ** 2).sum(1), kind="stable")[:2600] + 1
    rows = [[(v + 1) % 3000] for v in range(3000)]
    rows[0] = far_first.tolist()
    tree = FlatTree(np.zeros((1, 16), np.float32), np.zeros(1, np.float32), np.array([[0, -1]], np.int32), np.arange(3000, dtype=np.int32), 1)
    q = np.clip(x[0] + rs.randint(-30, 31, size=(30, 16)), -500, 500)
    return case("frontier_compaction", x, rows, tree, q, 64, 0.125, 1)


LATTICE = {}
for _k in WIDTHS:
    for _nn in (10, 30):
        LATTICE["width_k%d_nn%d" % (_k, _nn)] = functools.partial(_width_case, _k, _nn)
LATTICE.update({
    "graph_hub_rows": _hub_case, "graph_empty_self_duplicate": _ragged_case,
    "graph_islands_k200": functools.partial(_island_case, 200), "graph_islands_k10": functools.partial(_island_case, 10),
    "graph_ring_k5": functools.partial(_ring_case, 5), "graph_ring_k10": functools.partial(_ring_case, 10),
    "tree_leaves_k10_nn15": functools.partial(_leaf_case, 10, 15, 0.125), "tree_leaves_k64_nn30": functools.partial(_leaf_case, 64, 30, 0.25),
    "tree_leaves_k200_nn30": functools.partial(_leaf_case, 200, 30, 0.0),
    "tree_single_leaf": _single_leaf_case, "tree_none": _no_tree_case, "tree_tiny_leaves_repeated_draws": _tiny_leaf_case,
    "dim_4": functools.partial(_dim_case, 4), "dim_17": functools.partial(_dim_case, 17), "dim_130": functools.partial(_dim_case, 130),
    "dim_1000": functools.partial(_dim_case, 1000),
    "routing_small": functools.partial(_routing_case, "small"), "routing_wide": functools.partial(_routing_case, "wide"),
    "frontier_compaction": _compaction_case,
})


# ------------------------------------------------------------------------------------------------ float cases
FLOAT_METRICS = ("sqeuclidean", "cosine", "dot", "inner_product", "correlation", "hellinger")


def loose_clusters(n, d, seed, n_clusters=20):
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((n_clusters, d))
    return (centres[rs.randint(0, n_clusters, n)] + 1.0 * rs.standard_normal((n, d))).astype(np.float32)


def _descent_space(x, metric):
    """The rows as the tree descent sees a query of that metric (cosine / dot: unit length)."""
    if metric in ("cosine", "dot"):
        nrm = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
        return (x / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)
    return x


def _score(x, metric):
    x = x.astype(np.float64)
    if metric == "sqeuclidean":
        n2 = (x * x).sum(1)
        return 2.0 * x @ x.T - n2[:, None] - n2[None, :]
    if metric == "inner_product":
        return x @ x.T
    if metric == "correlation":
        x = x - x.mean(1, keepdims=True)
    elif metric == "hellinger":
        x = np.sqrt(x)
    nrm = np.linalg.norm(x, axis=1, keepdims=True)
    u = x / np.where(nrm > 0, nrm, 1.0)
    return u @ u.T


def _float_case(metric, d):
    seed = 200 + 10 * FLOAT_METRICS.index(metric) + d
    pts = loose_clusters(3000 + 60, d, seed)
    if metric == "hellinger":
        pts = np.abs(pts) ** 3  # (spread out: rows of similar non-negative entries are all within a hair of each other)
    x, q = pts[:3000].copy(), pts[3000:].copy()
    if metric == "cosine":
        x[7] = 0.0  # a zero data row: FLT_MAX from every query
    if metric == "dot":
        q[3] = 0.0  # a zero query: skipped, every slot stays -1 / inf
    rows = symmetric_rows(top_neighbours(_score(x, metric), 15))
    if metric == "cosine":
        for v in (100, 200, 300):
            rows[v] = [7] + rows[v]
    md = 0.0 if metric == "inner_product" else (1.0 if metric == "sqeuclidean" else 0.001)
    return case("float_%s_d%d" % (metric, d), x, rows, kd_tree(_descent_space(x, metric), 30), q, 10, 0.125, 15, metric=metric,
                min_distance=md, exact=False)


def _float_dim_case(d):
    pts = loose_clusters(3040, d, 300 + d, n_clusters=12)
    x, q = pts[:3000], pts[3000:]
    return case("float_dim_%d" % d, x, symmetric_rows(top_neighbours(_score(x, "sqeuclidean"), 15)), kd_tree(x, 30), q, 10, 0.125, 15,
                min_distance=0.0001, exact=False)


FLOAT = {"float_%s_d%d" % (m, d): functools.partial(_float_case, m, d) for m in FLOAT_METRICS for d in (12, 24)}
FLOAT.update({"float_dim_1": functools.partial(_float_dim_case, 1), "float_dim_3": functools.partial(_float_dim_case, 3)})


# ------------------------------------------------------------------------------------------------ uint8 walk (lattice)
# the integer codebook: 256 of the integers -512 .. 512, irregularly spaced (with a constant step every proxy distance of a
# query falls into one residue class, which makes exact ties several times as likely)
Q8_VALUES = np.sort(np.random.RandomState(399).choice(np.arange(-512, 513), 256, replace=False)).astype(np.float32)


def _q8_case(d, search_k):
    R = 490 if d < 40 else 300  # (d = 40: two latent dimensions, so the columns' spans stay far below 2 R)
    world = (500, d, R, 400 + d, 15, 2)
    x, rows = _world(*world)
    return case("q8_d%d_sk%d" % (d, search_k), x, rows, _world_tree(30, *world), near_queries(x, 30, 25, R, 401 + d + search_k),
                10, 0.125, 15, values=Q8_VALUES, search_k=search_k)


Q8 = {"q8_d%d_sk%d" % (d, sk): functools.partial(_q8_case, d, sk) for d in (13, 16, 40) for sk in (10, 64, 65, 256)}

ALL = {}
ALL.update(LATTICE)
ALL.update(FLOAT)
ALL.update(Q8)


def quantize(values, x):
    """The codes of the rows: position of the first codebook value that is not below the entry, as uint8."""
    return np.searchsorted(values, x).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def get(name, trace=False):
    """(case, reference results) of a case by name."""
    c = ALL[name]()
    if c.values is not None:
        c.codes = quantize(c.values, c.data)
        res = SR.reference_search(c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.search_k,
                                  c.epsilon, c.rng_state, exact=True, codes=c.codes, values=c.values, rerank_k=c.k, trace=trace)
    else:
        res = SR.reference_search(c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.k, c.epsilon,
                                  c.rng_state, exact=c.exact, trace=trace)
    return c, res


def cap(name):
    return FLOAT_CAP if name in FLOAT else LATTICE_CAP
