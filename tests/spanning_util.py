"""The spanning forest restated in numpy: the definitions the kernels of csrc/mst.hip are held to, bit for bit, and the
Gaussian-blob k-lists both test files run on."""
import numpy as np
import scipy.sparse as sp

from tests.snn_util import same_bytes  # noqa: F401  (offsets, columns and data bytes)


def blob_lists(m, k, blobs, duplicated=0, seed=3):
    """Exact k-lists of ``blobs`` Gaussian blobs in 4-D, float32, self in column 0; the first ``duplicated`` rows once more."""
    rs = np.random.RandomState(seed)
    x = (50 * rs.standard_normal((blobs, 4))[np.arange(m) % blobs] + rs.standard_normal((m, 4))).astype(np.float32)
    x[m - duplicated:] = x[:duplicated]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1, dtype=np.float32))
    d[np.arange(m), np.arange(m)] = -1.0  # the row itself first, also among duplicates
    ids = np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)
    d[np.arange(m), np.arange(m)] = 0.0
    return ids, np.take_along_axis(d, ids, axis=1)


def live_edges(ids, dists, min_samples):
    """``(i, j, w, core)``: the core distances, and every live place (i, s) with id j as an edge of weight max(core(i), core(j), d)."""
    ids, d = np.asarray(ids).astype(np.int64), np.where(np.asarray(dists) == 0, np.float32(0), np.asarray(dists, dtype=np.float32))
    m, k = ids.shape
    ok = (ids >= 0) & (ids < m) & np.isfinite(d) & (d >= 0)
    ranked = np.sort(np.where(ok, d, np.float32(np.inf)), axis=1)
    count = ok.sum(1)
    core = np.where(count > 0, ranked[np.arange(m), np.clip(np.minimum(min_samples, count) - 1, 0, k - 1)], 0).astype(np.float32)
    if min_samples == 0:
        core[:] = 0
    i, s = np.nonzero(ok & (ids != np.arange(m)[:, None]))
    j = ids[i, s]
    return i, j, np.maximum(np.maximum(core[i], core[j]), d[i, s]), core


def model_forest(ids, dists, min_samples):
    """``(forest, labels, core)`` by the definitions: Kruskal with union-find over the keys (bits of w, min(i, j), max(i, j)) of
    the live places in ascending order, labels by ascending smallest member."""
    m = np.asarray(ids).shape[0]
    i, j, w, core = live_edges(ids, dists, min_samples)
    keys = sorted(zip(w.view(np.uint32).tolist(), np.minimum(i, j).tolist(), np.maximum(i, j).tolist()))
    root, entries = list(range(m)), {}

    def find(a):
        while root[a] != a:
            root[a] = a = root[root[a]]
        return a
    for bits, lo, hi in keys:
        a, b = find(lo), find(hi)
        if a != b:
            root[max(a, b)] = min(a, b)  # (a root is its component's smallest member)
            entries[(lo, hi)] = entries[(hi, lo)] = np.uint32(bits)
    roots = np.array([find(a) for a in range(m)])
    labels = np.unique(roots, return_inverse=True)[1].astype(np.int32)
    at = sorted(entries)
    indptr = np.concatenate([[0], np.cumsum(np.bincount([r for r, _ in at], minlength=m))]).astype(np.int32)
    data = np.array([entries[e] for e in at], dtype=np.uint32).view(np.float32)
    return sp.csr_array((data, np.array([c for _, c in at], dtype=np.int32), indptr), shape=(m, m)), labels, core
