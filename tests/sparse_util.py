"""Helpers of the sparse-input tests: random CSR matrices with the shapes the kernel can go wrong at, the clustered sparse set of
the reference fixture (tests/golden/sparse_input.npz), float64 distances on dense rows, and recall counted by distance."""
import numpy as np
import scipy.sparse as sp


def random_csr(n, d, density, seed, index_dtypes=(np.int32, np.int32), empty_rows=(), full_rows=()):
    """A canonical float32 CSR matrix: each element stored with probability ``density`` (1: every one), values in
    [-2, -0.5] U [0.5, 2] (never zero, so ``toarray()`` shows every stored entry); the rows ``empty_rows`` hold nothing, the rows
    ``full_rows`` everything.  ``index_dtypes``: the dtypes of (indptr, indices)."""
    rs = np.random.RandomState(seed)
    mask = np.ones((n, d), bool) if density >= 1 else rs.random_sample((n, d)) < density
    for r in full_rows:
        mask[r % n] = True
    for r in empty_rows:
        mask[r % n] = False
    dense = np.where(mask, rs.uniform(0.5, 2.0, (n, d)) * rs.choice([-1.0, 1.0], (n, d)), 0.0).astype(np.float32)
    return with_index_dtypes(sp.csr_matrix(dense), index_dtypes), dense


def with_index_dtypes(m, index_dtypes):
    """``m`` with its index arrays in the given (indptr, indices) dtypes (scipy itself hands out either width)."""
    out = sp.csr_matrix(m.shape, dtype=np.float32)
    out.data = np.ascontiguousarray(m.data, np.float32)
    out.indptr = np.ascontiguousarray(m.indptr, index_dtypes[0])
    out.indices = np.ascontiguousarray(m.indices, index_dtypes[1])
    return out


def equality_data(boolean=False):
    """The set of the dense-equality tests: 1500 x 70 at density about 0.1, non-negative, rows 7 and 1499 empty, rows 100 and 900
    equal; 40 query rows, 30 fresh rows and 20 replacement rows of the same kind.  ``boolean``: every stored value is 1."""
    rs = np.random.RandomState(11)

    def rows(n):
        centres = rs.randint(0, 12, n)
        support = np.random.RandomState(5).random_sample((12, 70)) < 0.12  # the clusters' columns
        mask = (support[centres] & (rs.random_sample((n, 70)) < 0.7)) | (rs.random_sample((n, 70)) < 0.02)
        x = np.where(mask, rs.uniform(0.2, 3.0, (n, 70)), 0.0).astype(np.float32)
        return (x != 0).astype(np.float32) if boolean else x

    x = rows(1500)
    x[7] = 0.0
    x[1499] = 0.0
    x[900] = x[100]
    return x, rows(40), rows(30), rows(20)


def fixture_data():
    """The set of the reference fixture: 2000 x 64 clustered non-negative rows at density about 0.15 -- 25 clusters of 12 columns
    each, a row holds each of its cluster's columns with probability 0.75 and any other with 0.02, values around the cluster's
    own level -- every row with at least two entries, and 200 held-out query rows of the same kind.  float32, dense."""
    rs = np.random.RandomState(2024)
    columns = np.stack([rs.choice(64, 12, replace=False) for _ in range(25)])
    level = rs.uniform(0.5, 4.0, (25, 64))

    def rows(n):
        c = rs.randint(0, 25, n)
        mask = rs.random_sample((n, 64)) < 0.02
        own = np.zeros((n, 64), bool)
        np.put_along_axis(own, columns[c], True, axis=1)
        mask |= own & (rs.random_sample((n, 64)) < 0.75)
        for r in np.flatnonzero(mask.sum(1) < 2):
            mask[r, columns[c[r], :2]] = True
        return np.where(mask, level[c] * rs.uniform(0.7, 1.3, (n, 64)), 0.0).astype(np.float32)

    return rows(2000), rows(200)


def true_distances(metric, a, b):
    """float64 distances (the metric's own, not the kernels' space) of the dense rows ``a`` (m, d) to ``b`` (n, d): (m, n).
    Rows without an entry: distance 0 to each other, 1 to every other row (cosine, hellinger, jaccard), as the reference has it."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if metric == "euclidean":
        sq = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
        return np.sqrt(np.maximum(sq, 0.0))
    if metric == "jaccard":
        a, b = (a != 0).astype(np.float64), (b != 0).astype(np.float64)
        both = a @ b.T
        either = a.sum(1)[:, None] + b.sum(1)[None, :] - both
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(either == 0, 0.0, 1.0 - both / either)
    if metric == "hellinger":
        num, na, nb = np.sqrt(a) @ np.sqrt(b).T, a.sum(1)[:, None], b.sum(1)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.sqrt(np.maximum(1.0 - num / np.sqrt(na * nb), 0.0))
    else:
        assert metric == "cosine"
        num, na, nb = a @ b.T, (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            out = 1.0 - num / np.sqrt(na * nb)
    return np.where((na == 0) & (nb == 0), 0.0, np.where((na == 0) | (nb == 0), 1.0, out))


def exact_euclidean(a, b):
    """float64 euclidean distances without the expansion's cancellation: for checking returned distances."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def kth_distance(metric, q, x, k):
    """(nq,) the float64 distance of each row of ``q`` to its k-th nearest row of ``x``."""
    return np.partition(true_distances(metric, q, x), k - 1, axis=1)[:, k - 1]


def recall_by_distance(metric, q, x, ids, kth):
    """Recall counted by distance: an id counts when its float64 distance to the query is at most ``kth`` (that of the true k-th
    neighbour), so ties -- binary rows are full of them -- decide nothing.  ``ids`` (nq, k), -1 for an unfilled place."""
    hits = 0
    for r in range(q.shape[0]):
        got = ids[r][ids[r] >= 0]
        dist = true_distances(metric, q[r:r + 1], x[got])[0]
        hits += int((dist <= kth[r] * (1.0 + 1e-12) + 1e-15).sum())
    return hits / float(ids.shape[0] * ids.shape[1])
