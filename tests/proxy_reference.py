"""The step-exact model of the query kernel's float walk with the rerank epilogue (metric code 6, proxy_inner_product), built on
tests/search_reference.py without touching it: test infrastructure.

``_ProxyDistances`` gives the two distances of a code-6 searcher as (mid, lo, hi) intervals: the walk's proxy distance with
its a-priori float32 error (tests/proxy_util.py) and the rerank's -<q, x>.  ``proxy_search`` drives ``_Walk.run`` with
k = search_k and ``_Walk.finish(k_out)``, which pushes the walk's list in ascending proxy order by the rerank distance into
a list of k_out, as the kernel's epilogue does.

``lattice=True``: integer rows and queries with dim * R^2 < 2^24, so every float32 Gram value and norm is an exact integer:
the rerank distances are exact (lo = hi = mid) and only the evaluation of the proxy formula carries an error."""
import numpy as np

from tests import proxy_util as PU
from tests import search_reference as SR


class _ProxyDistances(SR._Distances):
    def __init__(self, data, lattice=False):
        super().__init__(data, 3, False)  # rows as given, like inner product
        self.metric = PU.CODE
        self.lattice = lattice
        if lattice:
            self.gamma = 0.0
        self.proxy = self.rows  # not None: _Walk.run hands it back as `rows` on the walk's calls, finish() passes None
        self.abs_rows = np.abs(self.rows)

    def __call__(self, q, qnz, ids, rows=None):
        a = self.rows[ids]
        g = a @ q
        dg = self.gamma * (self.abs_rows[ids] @ np.abs(q))
        if rows is None:  # the rerank: -<q, x>, neither clamped nor corrected
            return -g, -g - dg, -g + dg
        return PU.proxy_interval(g, dg, float((q * q).sum()), self.norm2[ids], self.gamma)


def proxy_search(data, indptr, indices, tree, min_distance, n_neighbors, queries, k, search_k, epsilon, seed_state=None, *, lattice=False):
    """One SearchResult per query: ids and -<q, x> ascending (unfilled: -1 / inf), the radius of every distance, and the flag."""
    data = np.asarray(data)
    dist = _ProxyDistances(data, lattice)
    walk = SR._Walk(data.shape[0], np.asarray(indptr, np.int64), np.asarray(indices, np.int64), tree, dist, min_distance,
                    int(n_neighbors), int(search_k), epsilon, SR.searcher_seed(seed_state), False)
    out = []
    for qi, q in enumerate(np.asarray(queries)):
        walk.k = int(search_k)
        walk.run(qi, q)
        out.append(walk.finish(int(k)))
    return out


# ------------------------------------------------------------------------------------------------ the search cases
# Shared by tests/test_proxy_cpu.py (the share of flagged queries, no GPU) and tests/test_gpu_proxy_search.py.
import functools  # noqa: E402
import types  # noqa: E402

from tests import search_cases as SC  # noqa: E402

WIDTHS = ((10, 40), (30, 120), (50, 200), (10, 10))  # (k, search_k): one, two and four result entries per lane; beam 1
DIMS = (17, 24)
N, NQ, EPSILON, N_NEIGHBORS, ROW_CAP = 2000, 40, 0.125, 15, 200
SCALE_DECADES, SCALE_TOP, SCALE_SHAPE = 13.0, 1e-3, 0.25


def spread_rows(n, d, seed):
    """Clustered rows shifted into the positive orthant (every inner product is positive: no FLT_MAX ties), each multiplied by
    a factor of its own: SCALE_TOP * 10^(-SCALE_DECADES * u^SCALE_SHAPE), u uniform.  Why: the model flags a query as soon as
    two distances it has to order lie within their float32 error of each other, and a walk that keeps 200 results orders a
    few hundred pairs.  The error of a proxy distance is about 2e-6 relative plus 1e-6 absolute (the log term).  Short rows
    (SCALE_TOP) make every distance, dominated by 1 / sqrt<q, x>, larger than 10, so the absolute part does not count; and the
    exponent's shape spreads the longest tenth of the rows -- a query's nearest few hundred -- over half of the decades, a few
    per cent from one distance to the next, where rows of similar length would put them within a few radii of each other."""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((20, d))
    pts = centres[rs.randint(0, 20, n)] + rs.standard_normal((n, d)) + 4.0
    scale = SCALE_TOP * 10.0 ** (-SCALE_DECADES * rs.uniform(0.0, 1.0, n) ** SCALE_SHAPE)
    return (np.abs(pts) * scale[:, None]).astype(np.float32)


def angular_tree(points, leaf_size, seed):
    """FlatTree in the searcher's format whose hyperplanes pass through the origin: the difference of two members' unit rows,
    offset 0.  A query's margin <h, q> scales with the query's own length alone (a tree that cuts these rows at a coordinate
    value would have offsets of every magnitude down to 1e-15, below the 1e-8 under which the descent draws its side)."""
    from pynndescent_amd.search_tree import FlatTree

    pts = np.asarray(points, np.float64)
    unit = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    rs = np.random.RandomState(seed)
    hyper, children, order = [], [], []

    def build(ids):
        node = len(hyper)
        hyper.append(np.zeros(pts.shape[1], np.float32))
        children.append([0, 0])
        if len(ids) > leaf_size:
            for _ in range(8):
                a, b = rs.choice(len(ids), 2, replace=False)
                h = (unit[ids[a]] - unit[ids[b]]).astype(np.float32)
                side0 = unit[ids] @ h.astype(np.float64) > 0.0
                if min(side0.sum(), (~side0).sum()) >= max(1, len(ids) // 8):
                    hyper[node] = h
                    c0 = build(ids[side0])
                    c1 = build(ids[~side0])
                    children[node] = [c0, c1]
                    return node
        children[node] = [-len(order), -(len(order) + len(ids))]
        order.extend(ids.tolist())
        return node

    build(np.arange(len(pts)))
    return FlatTree(np.array(hyper, np.float32), np.zeros(len(hyper), np.float32), np.array(children, np.int32), np.array(order, np.int32), leaf_size)


@functools.lru_cache(maxsize=None)
def _world(d):
    x = spread_rows(N, d, 600 + d)
    rs = np.random.RandomState(650 + d)  # queries of ordinary length: a margin of the tree descent is far from 0
    q = (np.abs(rs.standard_normal((NQ, d)) * 1.5 + 4.0) * 10.0 ** rs.uniform(-3.0, -2.0, (NQ, 1))).astype(np.float32)
    # the long rows are everybody's neighbours: their rows are cut at ROW_CAP entries, so that a walk visits a few hundred
    # vertices (enough to fill 200 results) instead of the whole set at its first hub
    rows = [r[:ROW_CAP] for r in SC.symmetric_rows(SC.top_neighbours(-PU.proxy_dist(x, x), N_NEIGHBORS))]
    indptr, indices = SC.csr_from_rows(rows)
    nbr = PU.proxy_dist(x, x)
    np.fill_diagonal(nbr, np.inf)
    return x, q, indptr, indices, angular_tree(x, 30, 700 + d), float(np.float32(nbr.min()))


@functools.lru_cache(maxsize=None)
def search_case(d, k, search_k):
    """(case, model results) of one float-walk-with-rerank case."""
    x, q, indptr, indices, tree, md = _world(d)
    case = types.SimpleNamespace(name="proxy_d%d_k%d_sk%d" % (d, k, search_k), data=x, queries=q, indptr=indptr, indices=indices, tree=tree,
                                 min_distance=md, n_neighbors=N_NEIGHBORS, k=k, search_k=search_k, epsilon=EPSILON, rng_state=SC.RNG_STATE)
    return case, proxy_search(x, indptr, indices, tree, md, N_NEIGHBORS, q, k, search_k, EPSILON, SC.RNG_STATE)


SEARCH_CASES = [(d, k, sk) for d in DIMS for k, sk in WIDTHS]


# a lattice: non-negative integer rows and queries with dim * R^2 < 2^24 -- every float32 product, partial sum and norm is an
# exact integer, so the rerank's -<q, x> is exact (bit for bit) and the walk's proxy carries the formula's evaluation error only
LATTICE_N, LATTICE_D, LATTICE_R, LATTICE_K, LATTICE_SEARCH_K = 400, 16, 1000, 10, 30


@functools.lru_cache(maxsize=None)
def lattice_case():
    rs = np.random.RandomState(811)
    centres = np.abs(rs.standard_normal((12, LATTICE_D))) + 0.3
    def draw(n, lo):
        pts = np.abs(centres[rs.randint(0, 12, n)] + 0.6 * rs.standard_normal((n, LATTICE_D)))
        length = LATTICE_R * 10.0 ** rs.uniform(lo, 0.0, (n, 1))
        return np.minimum(np.rint(pts / pts.max(1, keepdims=True) * length), LATTICE_R).astype(np.float32)
    x, q = draw(LATTICE_N, -2.0), draw(NQ, -0.5)
    x[x.sum(1) == 0, 0] = 1.0
    assert LATTICE_D * LATTICE_R ** 2 < 2 ** 24
    rows = SC.symmetric_rows(SC.top_neighbours(-PU.proxy_dist(x, x), N_NEIGHBORS))
    indptr, indices = SC.csr_from_rows(rows)
    nbr = PU.proxy_dist(x, x)
    np.fill_diagonal(nbr, np.inf)
    md = float(np.float32(nbr.min()))
    tree = angular_tree(x, 30, 812)
    case = types.SimpleNamespace(name="proxy_lattice", data=x, queries=q, indptr=indptr, indices=indices, tree=tree, min_distance=md,
                                 n_neighbors=N_NEIGHBORS, k=LATTICE_K, search_k=LATTICE_SEARCH_K, epsilon=EPSILON, rng_state=SC.RNG_STATE)
    return case, proxy_search(x, indptr, indices, tree, md, N_NEIGHBORS, q, LATTICE_K, LATTICE_SEARCH_K, EPSILON, SC.RNG_STATE, lattice=True)
