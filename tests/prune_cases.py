"""The cases of the step-exact pruning tests (tests/test_prune_reference_cpu.py, tests/test_gpu_prune_exact.py), which kernel
form each reaches, and the ambiguity caps.

Which kernel a handle's k selects (csrc/prune.hip nnd_launch_diversify_rows / nnd_launch_diversify_csr): k <= 64 the lane
forms k_diversify_rows / k_diversify_csr (one entry a lane), k 65-256 the LDS forms k_diversify_rows_wide /
k_diversify_csr_wide.  Every kernel gives a wave a row and a workgroup four rows: n is never a multiple of 4, so the last
workgroup has idle waves.  n stays below 65536 (the column mean of the prepared rows is the mean of all rows only there).

Sizes.  A row is an independent walk, so a case needs rows, not volume: 1202 rows are 300 workgroups and give every path of a walk -- first entry pruned, last entry pruned, nothing pruned, ties,
guards -- hundreds of rows.  The one exception is scan_rounds, whose size is the point (see below).

Lattice cases (euclidean, integer coordinates, the point set closed under negation): every pair distance is an exact integer
whatever the summation order, so ids, kept positions, distance bits, stage counts and the final CSR must be EQUAL and no row may be
flagged.  ``ties``: coordinates in [-2, 2]^8 -- distances are small integers, so d(j, c) == d(i, j) and d == w_j are frequent: the
strict `<`.  ``dups``: the same with a fifth of the points repeated -- stored distance 0: the PRUNE_EPS guard, the 0 -> EPS
substitution of k_sg_compact, min_distance.

Float cases: exact k-NN graphs (by the model's own float64 distances, stored as float32; the own vertex included, as the
reference's graphs have it) of clustered data, and the reference-built graphs of tests/golden/search_graph*.npz.

Caps: at most 10 % of the rows of a float case may be flagged or tainted, none on the lattice (descent_cases.FLOAT_CAP).
"""
import os
from collections import namedtuple

import numpy as np

from tests import metric_util as MU
from tests import prune_reference as PR
from tests.descent_cases import FLOAT_CAP, LATTICE_CAP  # noqa: F401
from tests.util_data import clustered

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAN_WORDS = 1024 * 2048   # searchgraph.hip k_sg_scan_single: one round scans 1024 tiles of SG_TILE = 2048 words

# mode: diversify_prob, degree_aware, degree_prune_aggressiveness (the arguments of nnd_search_graph); multiplier is 1.5
Case = namedtuple("Case", ["name", "metric", "k", "n", "d", "data", "graph", "prob", "aware", "aggr", "exact", "seed", "doc"])


def _c(name, metric, k, n, d, data, doc, graph="knn", prob=1.0, aware=False, aggr=1.0, exact=False, seed=77):
    return Case(name, metric, k, n, d, data, graph, prob, aware, aggr, exact, seed, doc)


N, NW = 1202, 1202
LATTICE = {c.name: c for c in [
    _c("lat_k1", "euclidean", 1, N, 8, "ties", "lane forms, rows of one entry: nothing to walk, csr rows of length 1 left alone", exact=True),
    _c("lat_k2", "euclidean", 2, N, 8, "ties", "lane forms, one test a row", exact=True),
    _c("lat_k15", "euclidean", 15, N, 8, "ties", "lane forms at the benchmark's k; exact ties pin the strict <", exact=True),
    _c("lat_k16", "euclidean", 16, N, 8, "holes", "lane forms; -1 tails of every length, a row that is all -1, a row of one entry", exact=True),
    _c("lat_k63", "euclidean", 63, N, 8, "ties", "lane forms, one idle lane: the last kept slot is bit 62", exact=True),
    _c("lat_k64", "euclidean", 64, N, 8, "ties", "lane forms, every lane an entry: kept bit 63, csr rows of 64 (len == 64 ? ~0ull)", exact=True),
    _c("lat_k65", "euclidean", 65, N, 8, "ties", "LDS forms at their smallest k (one entry in the second 64-block)", exact=True),
    _c("lat_k100", "euclidean", 100, N, 8, "ties", "LDS forms, two entries a lane", exact=True),
    _c("lat_k256", "euclidean", 256, NW, 8, "ties", "LDS forms at NND_WIDE_K: every LDS slot an entry", exact=True),
    _c("lat_dups_k15", "euclidean", 15, N, 8, "dups", "lane forms; duplicate points: stored 0 (PRUNE_EPS guard, 0 -> EPS, min_distance)", exact=True),
    _c("lat_dups_k100", "euclidean", 100, N, 8, "dups", "LDS forms; duplicate points", exact=True),
    _c("lat_own_k15", "euclidean", 15, N, 8, "ties", "lane forms; the own vertex as a comparison point: it leads every row at a stored "
       "distance of 1/2 > PRUNE_EPS, and the other stored distances are 2 d + 1, above the true ones -- a recomputed d(j, i) would "
       "prune every entry, the stored d(i, j) none", graph="own", exact=True),
    _c("lat_own_k100", "euclidean", 100, N, 8, "ties", "LDS forms; the own vertex as a comparison point", graph="own", exact=True),
    _c("lat_k15_p50", "euclidean", 15, N, 8, "ties", "lane forms with coins (diversify_prob 0.5)", prob=0.5, exact=True),
    _c("lat_k100_p50", "euclidean", 100, N, 8, "ties", "LDS forms with coins: entries beyond 64, where a * 64 + b collided", prob=0.5, exact=True),
    _c("lat_k15_aware", "euclidean", 15, N, 8, "ties", "lane forms, degree aware (alpha 1, aggressiveness 1)", aware=True, exact=True),
    _c("scan_rounds", "euclidean", 30, 36002, 16, "wide_lattice", "the second round of k_sg_scan_single (carry_s): a constructed graph "
       "whose stored distances lie below every pair distance keeps all n k entries, 2 n k = 2 160 120 > 2 097 152 keyed edges and as "
       "many union entries -- both the m_live and the union_nnz scan take 1055 tiles", graph="unpruned", exact=True),
]}
FLOAT = {c.name: c for c in [
    _c("euclidean_k15", "euclidean", 15, N, 24, "clustered", "lane forms, code 0 (difference form)"),
    _c("euclidean_k15_d130", "euclidean", 15, N, 130, "clustered", "lane forms, dp = 132: a lane sums three terms"),
    _c("cosine_k15", "cosine", 15, N, 24, "clustered", "lane forms, code 1"),
    _c("dot_k15", "dot", 15, N, 16, "metric", "lane forms, code 2; zero rows at FLT_MAX"),
    _c("inner_product_k15", "inner_product", 15, N, 16, "metric", "lane forms, code 3; rows keep their own vertex at 1 / |x|^2 > EPS"),
    _c("correlation_k15", "correlation", 15, N, 16, "metric", "lane forms, code 4; constant rows"),
    _c("hellinger_k15", "hellinger", 15, N, 24, "metric", "lane forms, code 5; zero rows"),
    _c("euclidean_k100", "euclidean", 100, N, 24, "clustered", "LDS forms on float data"),
    _c("euclidean_k15_p50", "euclidean", 15, N, 24, "clustered", "lane forms with coins", prob=0.5),
    _c("euclidean_k100_p50", "euclidean", 100, N, 24, "clustered", "LDS forms with coins", prob=0.5),
    _c("aware_a10_g10", "euclidean", 15, N, 24, "clustered", "degree aware, alpha 1.0, aggressiveness 1.0", aware=True),
    _c("aware_a07_g20", "euclidean", 15, N, 24, "clustered", "degree aware, alpha 0.7, aggressiveness 2.0", prob=0.7, aware=True, aggr=2.0),
    _c("aware_cosine_a07_g10", "cosine", 15, N, 24, "clustered", "degree aware on unit rows, alpha 0.7, aggressiveness 1.0", prob=0.7, aware=True),
    _c("aware_k100_g20", "euclidean", 100, N, 24, "clustered", "degree aware, LDS forms, aggressiveness 2.0", aware=True, aggr=2.0),
]}
# the reference's own recorded runs (tests/golden/search_graph.npz, search_graph_modes.npz): tag -> (file, metric, prob, aware, aggr)
FIXTURES = {
    "euclidean": ("search_graph.npz", "euclidean", 1.0, False, 1.0),
    "cosine": ("search_graph.npz", "cosine", 1.0, False, 1.0),
    "aware_euclidean": ("search_graph_modes.npz", "euclidean", 1.0, True, 2.0),
    "aware_cosine": ("search_graph_modes.npz", "cosine", 1.0, True, 2.0),
}
ALL = dict(FLOAT, **LATTICE)
assert all(c.n % 4 and c.n < 65536 for c in ALL.values())

_DATA, _GRAPH, _PREP = {}, {}, {}


def lattice(n, d, r, seed, dups=False):
    """n integer points of [-r, r]^d, closed under negation (column mean exactly 0); distinct unless ``dups``, which repeats a
    fifth of the half set (the copies and their negatives)."""
    assert n % 2 == 0 and ((d + 3) & ~3) * (2 * r) ** 2 < 2 ** 24
    h = np.random.RandomState(seed).randint(-r, r + 1, size=(4 * n, d))
    h = h[h.any(1)]
    first = h[np.arange(len(h)), (h != 0).argmax(1)]
    h = h * np.sign(first)[:, None]                     # one of every +- pair
    _, keep = np.unique(h, axis=0, return_index=True)
    h = h[np.sort(keep)][: n // 2]
    assert len(h) == n // 2, "the range is too small for %d distinct points" % n
    if dups:
        m = len(h) // 5
        h[-m:] = h[:m]
    x = np.vstack([h, -h]).astype(np.float32)
    assert dups or len(np.unique(x, axis=0)) == n
    return np.ascontiguousarray(x)


def data(case):
    key = (case.data, case.metric, case.n, case.d)
    if key not in _DATA:
        if case.data in ("ties", "holes"):
            x = lattice(case.n, case.d, 2, 5)
        elif case.data == "dups":
            x = lattice(case.n, case.d, 2, 5, dups=True)
        elif case.data == "wide_lattice":
            x = lattice(case.n, case.d, 60, 7)
        elif case.metric == "hellinger":
            # non-negative rows that are not nearly parallel (descent_cases.data: shifted rows make -log2 cancel)
            x = np.maximum(clustered(case.n, case.d, 6, 30, seed=case.n % 89), np.float32(0.0))
            x[[7, 500, 1100]] = 0.0
        elif case.data == "metric":
            x = np.ascontiguousarray(MU.metric_data(case.metric, 2000, case.d, seed=11)[0][:case.n])
            if case.metric == "dot":  # the class hands the build normalised rows
                nrm = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
                x = np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1.0), 0.0).astype(np.float32)
        else:
            x = clustered(case.n, case.d, 6, 30, seed=case.n % 89)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def prepared(case):
    key = (case.data, case.metric, case.n, case.d)
    if key not in _PREP:
        _PREP[key] = PR.Prepared(data(case), case.metric, case.exact)
    return _PREP[key]


def knn_graph(prep, k):
    """The exact k nearest rows of every row by the model's own float64 distances, ties by id, the row itself included at its
    self distance; distances stored as float32."""
    n = prep.n
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k), np.float32)
    allb = np.arange(n)[None, :]
    for s in range(0, n, 512):
        rows = np.arange(s, min(s + 512, n))
        mid = prep.block(rows[None, :], allb)[0][0]
        mid[np.arange(len(rows)), rows] = prep.self_mid[rows]
        d32 = mid.astype(np.float32)
        o = np.argsort(d32, axis=1, kind="stable")[:, :k]   # (stable on ascending ids: ties by id)
        idx[s:s + 512], dist[s:s + 512] = o, np.take_along_axis(d32, o, 1)
    return idx, dist


def graph(case):
    """(idx (n, k) int32, dist (n, k) float32) of the case: the graph the pass is handed."""
    if case.name not in _GRAPH:
        prep = prepared(case)
        n, k = case.n, case.k
        if case.graph == "unpruned":
            # entry j of row i points at i + 1 + 7 j (no own vertex, no pair of reciprocal edges: 2 n k union entries); the stored
            # distances 1/4 + j/64 are exact, above PRUNE_EPS and below 1 <= every distance of two distinct lattice points
            idx = ((np.arange(n)[:, None] + 1 + 7 * np.arange(k)[None, :]) % n).astype(np.int32)
            dist = np.broadcast_to((0.25 + np.arange(k) / 64.0).astype(np.float32), (n, k)).copy()
        else:
            key = (case.data if case.data != "holes" else "ties", case.metric, n, case.d, k)
            if key not in _GRAPH:
                _GRAPH[key] = knn_graph(prep, k)
            idx, dist = (a.copy() for a in _GRAPH[key])
            if case.graph == "own":
                assert (idx[:, 0] == np.arange(n)).all() and (dist[:, 0] == 0).all() and (dist[:, 1:] >= 1).all()
                dist = (2.0 * dist + 1.0).astype(np.float32)
                dist[:, 0] = 0.5
            if case.data == "holes":
                rs = np.random.RandomState(3)
                cut = rs.randint(1, k + 1, n)                  # every row keeps 1 .. k entries
                cut[5], cut[6] = 0, 1                          # a row that is all -1, a row of one entry
                hole = np.arange(k)[None, :] >= cut[:, None]
                idx[hole], dist[hole] = -1, np.inf
        idx.setflags(write=False)
        dist.setflags(write=False)
        _GRAPH[case.name] = (idx, dist)
    return _GRAPH[case.name]


def fixture(tag):
    """(x, prep, idx, dist, the npz) of one recorded reference run."""
    fname, metric, _, _, _ = FIXTURES[tag]
    g = np.load(os.path.join(GOLDEN, fname))
    n, d, latent, ncl, seed = (int(v) for v in g[tag + "_gen"])
    x = clustered(n, d, latent, ncl, seed)
    return x, PR.Prepared(x, metric), g[tag + "_idx"], g[tag + "_dist"], g


def forward_opts(case_or_mode, idx, n_neighbors, multiplier=1.5):
    """The keyword arguments of the forward pass as nnd_search_graph_impl derives them (searchgraph.hip :264-275): for the model's
    diversify_rows; ``builder_opts`` turns them into Builder.diversify's."""
    prob, aware, aggr, seed = case_or_mode.prob, case_or_mode.aware, case_or_mode.aggr, case_or_mode.seed
    if aware:
        return dict(aware=True, degree=PR.compute_degrees(idx), max_degree=PR.forward_max_degree(multiplier, n_neighbors),
                    base_rate=PR.base_rate_of(aggr), alpha=prob, seed=seed)
    return dict(prob=prob, seed=seed)


def builder_forward_opts(case, idx, n_neighbors, multiplier=1.5):
    if case.aware:
        return dict(degree=PR.compute_degrees(idx), degree_aware=True, max_degree=PR.forward_max_degree(multiplier, n_neighbors),
                    aggressiveness=case.aggr, alpha=case.prob, seed=case.seed)
    return dict(prune_probability=case.prob, seed=case.seed)


# ---- the csr kernel alone: constructed rows -------------------------------------------------------------------------
def csr_alone(n, length, seed, repeat=True):
    """A CSR matrix of n rows for Builder.diversify_csr: every fourth row has exactly ``length`` entries (the model walks a row of
    256 in 255 steps: a few hundred such rows are enough), the others 0 .. 8 (rows 1, 2, 3: 0, 1, 2; row 9: length - 1);
    distinct columns a row; integer weights in the range of the lattice's pair distances (so d == w_j happens) -- from a small
    set, so that weights REPEAT (the rank's tie-break by position), or distinct within a row.  Every third row holds its own
    vertex, every fifth three entries of weight 0 (the aware walk skips them)."""
    rs = np.random.RandomState(seed)
    ln = np.where(np.arange(n) % 4 == 0, length, rs.randint(0, 9, n)).astype(np.int64)
    ln[[1, 2, 3, 9]] = [0, 1, 2, length - 1]
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    indices = np.empty(indptr[-1], np.int32)
    data = np.empty(indptr[-1], np.float32)
    for i in range(n):
        cols = rs.choice(n - 1, ln[i], replace=False)
        cols[cols >= i] += 1                                   # not the own vertex ...
        if i % 3 == 0 and ln[i] > 2:
            cols[ln[i] // 2] = i                               # ... except in every third row
        w = (rs.randint(1, 12, ln[i]) * 4 if repeat else rs.choice(np.arange(1, 3 * length), ln[i], replace=False)).astype(np.float32)
        if i % 5 == 0 and ln[i] > 3:
            w[rs.choice(ln[i], 3, replace=False)] = 0.0
        indices[indptr[i]:indptr[i + 1]], data[indptr[i]:indptr[i + 1]] = cols, w
    return indptr, indices, data


def degree_prune_alone(n, max_degree, seed):
    """CSR weights for Builder.degree_prune: rows of length 0, max_degree - 1, max_degree (untouched), max_degree + 1, 64, 65,
    150 and 300 (the e0 loop of k_degree_prune), weights from a small set so that values repeat AT the cut."""
    rs = np.random.RandomState(seed)
    ln = rs.choice([0, max_degree - 1, max_degree, max_degree + 1, 64, 65, 150, 300], n)
    ln[:8] = [0, max_degree - 1, max_degree, max_degree + 1, 64, 65, 150, 300]
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    data = rs.randint(1, 9, indptr[-1]).astype(np.float32) / 4.0
    distinct = np.nonzero(ln == max_degree + 1)[0][::2]       # and rows without repeats: exactly one entry leaves
    for i in distinct:
        data[indptr[i]:indptr[i + 1]] = rs.permutation(max_degree + 1) + 1.0
    return indptr, data
