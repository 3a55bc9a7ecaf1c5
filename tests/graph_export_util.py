"""Host model of the graph export (csrc/csr_graph.hip) in numpy / scipy, and the synthetic k-lists its tests run on."""
import numpy as np
import scipy.sparse as sp


def model_csr(ids, vals, n, mode="distance", symmetric=False, drop_self=False):
    """The canonical CSR matrix of the k-lists ``ids`` / ``vals`` (m, k) with ``n`` columns: ``coo_array(...).tocsr()`` of the
    places whose id names a column -- an id outside [0, n) is an empty place like -1 -- (a row never holds an id twice, so
    nothing is summed); ``symmetric``: the union with the transpose, an entry present on both sides holding the smaller float,
    and of two equal floats of different bits (+0.0 and -0.0) the one with the smaller bit pattern: what the kernels' sort by
    (column, value bits) followed by ``b < a ? b : a`` on the neighbours keeps; ``connectivity`` stores 1.0.  No NaN.
    Returns (indptr int64, indices int32, data float32)."""
    ids = np.asarray(ids).astype(np.int64)
    vals = np.asarray(vals, dtype=np.float32)
    m, k = ids.shape
    rows = np.repeat(np.arange(m, dtype=np.int64), k)
    cols, data = ids.ravel(), vals.ravel()
    keep = (cols >= 0) & (cols < n)
    if drop_self:
        keep &= cols != rows
    rows, cols, data = rows[keep], cols[keep], data[keep]
    if symmetric:
        assert m == n
        off = rows != cols  # the diagonal is its own reverse
        rows, cols, data = np.concatenate([rows, cols[off]]), np.concatenate([cols, rows[off]]), np.concatenate([data, data[off]])
        # explicit min-union: sort by (row, column, value, value bits) and keep the first entry of every (row, column)
        # (the float order taken from the bits -- sign and magnitude, +0.0 and -0.0 equal -- so that a subnormal compares as the
        # device compares it even in a process whose host arithmetic flushes subnormals: a -ffast-math library, once loaded, sets that)
        bits = data.view(np.uint32)
        magnitude = (bits & np.uint32(0x7FFFFFFF)).astype(np.int64)
        order = np.lexsort((bits, np.where(bits >> np.uint32(31), -magnitude, magnitude), cols, rows))
        rows, cols, data = rows[order], cols[order], data[order]
        first = np.ones(rows.shape[0], bool)
        first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        rows, cols, data = rows[first], cols[first], data[first]
    if mode == "connectivity":
        data = np.ones_like(data)
    a = sp.coo_array((data, (rows, cols)), shape=(m, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    assert a.nnz == rows.shape[0]  # nothing was summed
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32)


def random_klists(m, k, n, seed, empty=0.15, empty_rows=0.1, id_dtype=np.int32):
    """(m, k) ids drawn without repetition per row from [0, n), positive float32 values, -1 scattered at random places and over
    whole rows.  Needs k <= n."""
    rs = np.random.RandomState(seed)
    ids = np.stack([rs.permutation(n)[:k] for _ in range(m)]).astype(id_dtype)
    vals = (rs.random_sample((m, k)) + 0.01).astype(np.float32)
    ids[rs.random_sample((m, k)) < empty] = -1
    ids[rs.random_sample(m) < empty_rows] = -1
    return ids, vals


def symmetric_values(ids):
    """Values that are a function of the unordered pair, as a distance is: those of (i, j) and of (j, i) agree."""
    ids = np.asarray(ids).astype(np.int64)
    i = np.repeat(np.arange(ids.shape[0], dtype=np.int64)[:, None], ids.shape[1], axis=1)
    lo, hi = np.minimum(i, ids), np.maximum(i, ids)
    h = (lo * 2654435761 + hi * 40503 + 12345) % 1000003
    return (h.astype(np.float64) / 1000003.0 + 0.01).astype(np.float32)


def assert_same_csr(got, want):
    """indptr, indices and data equal bit for bit."""
    for g, w, name in zip(got, want, ("indptr", "indices", "data")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s: shape %s, model %s" % (name, g.shape, w.shape)
        if name == "data":
            assert g.dtype == np.float32
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name
        else:
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), name
