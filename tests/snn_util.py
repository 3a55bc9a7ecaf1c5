"""The shared-neighbour graph restated with Python sets: the definition the kernels of csrc/snn.hip are held to, bit for bit."""
import numpy as np
import scipy.sparse as sp


def model_snn(ids, weight="jaccard", include_self=True, prune=0.0, symmetric=True):
    """``ids`` (m, k): row i is point i, a place outside [0, m) is empty.  O(i): the distinct valid ids of row i other than i;
    N(i) = O(i) | {i} with ``include_self``.  Every i and j in O(i) is an edge of c = |N(i) & N(j)|, u = |N(i) | N(j)|, weight
    float32(c) or float32(c / u) (the quotient taken in float64), stored iff w > 0 and w >= float32(prune).  The symmetric
    form is the union with the transpose.  Returns a canonical ``scipy.sparse.csr_array`` (float32 data, int32 columns)."""
    ids = np.asarray(ids)
    m = ids.shape[0]
    own = [set(int(j) for j in row if 0 <= j < m and j != i) for i, row in enumerate(ids)]
    full = [o | {i} for i, o in enumerate(own)] if include_self else own
    bound, entries = np.float32(prune), {}
    for i in range(m):
        for j in own[i]:
            c = len(full[i] & full[j])
            u = len(full[i]) + len(full[j]) - c
            w = np.float32(c) if weight == "count" else np.float32(c / u)
            if w > 0 and w >= bound:
                entries[(i, j)] = w
                if symmetric:
                    assert entries.setdefault((j, i), w) == w  # a function of the unordered pair of sets
    keys = sorted(entries)
    rows, cols = np.array([r for r, _ in keys], dtype=np.int64), np.array([c for _, c in keys], dtype=np.int32)
    data = np.array([entries[key] for key in keys], dtype=np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    out = sp.csr_array((data, cols, indptr), shape=(m, m))
    out.has_sorted_indices = out.has_canonical_format = True
    return out


def same_bytes(a, b):
    """Two CSR matrices hold the same offsets, columns and bits."""
    return (np.array_equal(a.indptr, b.indptr) and a.indices.astype(np.int32).tobytes() == b.indices.astype(np.int32).tobytes()
            and a.data.dtype == b.data.dtype == np.float32 and a.data.tobytes() == b.data.tobytes())
