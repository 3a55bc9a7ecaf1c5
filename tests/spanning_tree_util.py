"""The spanning tree restated in numpy: the definitions the kernels of csrc/cross.hip are held to.

F, labels, core: ``model_forest`` of tests/spanning_util.py.  d(i, j): the float32 rounding of the float64 distance of the rows in
the metric's own space.  For i, j in different components w = max(core(i), core(j), d) in float32, no edge where d is not finite;
key = (bits of w, min(i, j), max(i, j)); the weight between two components is the smallest key over their cross pairs; C is
Kruskal's tree of the components under the key order; tree = F + C."""
import numpy as np
import scipy.sparse as sp

from tests.spanning_util import model_forest


def true_distances(x, metric):
    """(m, m) float32: the float64 distances of the rows, rounded once."""
    x = np.asarray(x, np.float64)
    if metric == "cosine":  # 1 - 2^-v of the alternative cosine v: 0 for two zero rows, 1 for one or a cosine <= 0
        dot, n2 = x @ x.T, (x * x).sum(1)
        na, nb = n2[:, None], n2[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            alt = np.maximum(np.log2(np.sqrt(na * nb) / dot), 0.0)
        alt[(na == 0) | (nb == 0) | (dot <= 0)] = np.inf
        alt[(na == 0) & (nb == 0)] = 0.0
        return (1.0 - np.exp2(-alt)).astype(np.float32)
    sq = np.zeros((x.shape[0], x.shape[0]))
    for t in range(x.shape[1]):
        sq += (x[:, t, None] - x[None, :, t]) ** 2
    return (sq if metric == "sqeuclidean" else np.sqrt(sq)).astype(np.float32)


def model_tree(x, ids, dists, min_samples, metric):
    """``(tree, core, n_components)`` by the definitions (m < 65536: a key is one 64-bit word)."""
    forest, labels, core = model_forest(ids, dists, min_samples)
    m, nc = len(labels), int(labels.max()) + 1
    i, j = np.triu_indices(m, 1)
    d = true_distances(x, metric)[i, j]
    keep = (labels[i] != labels[j]) & np.isfinite(d)
    i, j, d = i[keep], j[keep], d[keep]
    w = np.maximum(np.maximum(core[i], core[j]), np.where(d == 0, np.float32(0), d))
    key = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (i.astype(np.uint64) << np.uint64(16)) | j.astype(np.uint64)
    a, b = np.minimum(labels[i], labels[j]).astype(np.int64), np.maximum(labels[i], labels[j]).astype(np.int64)
    order = np.argsort(a * nc + b, kind="stable")
    starts = np.flatnonzero(np.diff((a * nc + b)[order], prepend=-1))
    best = np.sort(np.minimum.reduceat(key[order], starts)) if len(starts) else []  # the smallest key of every pair of components
    root = list(range(nc))

    def find(c):
        while root[c] != c:
            root[c] = c = root[root[c]]
        return c
    rows, cols, bits = [], [], []
    for k in best:
        lo, hi = int(k >> np.uint64(16)) & 0xFFFF, int(k) & 0xFFFF
        ca, cb = find(labels[lo]), find(labels[hi])
        if ca != cb:
            root[ca] = cb
            rows += [lo, hi]
            cols += [hi, lo]
            bits += [int(k >> np.uint64(32))] * 2
    joins = sp.coo_array((np.array(bits, np.uint32).view(np.float32), (rows, cols)), shape=(m, m))
    f = forest.tocoo()
    at = np.lexsort((np.concatenate([f.col, joins.col]), np.concatenate([f.row, joins.row])))  # (no sum: zero weights are entries)
    r, c, v = (np.concatenate(p)[at] for p in ((f.row, joins.row), (f.col, joins.col), (f.data, joins.data)))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    return sp.csr_array((v.astype(np.float32), c.astype(np.int32), indptr), shape=(m, m)), core, nc


def brute_lists(x, k, metric="euclidean", groups=None):
    """Exact k-lists of the rows, self in column 0; ``groups``: a row lists rows of its own group only (-1 where it has fewer)."""
    d = true_distances(x, metric).astype(np.float64)
    if groups is not None:
        d[groups[:, None] != groups[None, :]] = np.inf
    at = np.arange(len(x))
    d[at, at] = -1.0
    ids = np.argsort(d, axis=1, kind="stable")[:, :k]
    out = np.take_along_axis(d, ids, axis=1)
    out[:, 0] = 0.0
    return np.where(np.isfinite(out), ids, -1).astype(np.int32), np.where(np.isfinite(out), out, 0).astype(np.float32)
