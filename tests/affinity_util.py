"""The host model of the perplexity affinities (csrc/affinity.hip): sklearn's _binary_search_perplexity in numpy on the energies
minus the row's smallest, the mean over the scales, P + P.T over the total, in float64 -- and, for the noise floor, in float32."""
import numpy as np
import scipy.sparse as sp


def model_search(ids, dists, n, perplexity=30.0, squared=True, f=np.float64):
    """(betas (m, S), the (m, k) conditional entries): a plain loop over the rows, which do not see each other."""
    m, k = ids.shape
    scales = np.atleast_1d(np.asarray(perplexity, np.float64))
    d = np.asarray(dists, np.float32).astype(f)
    with np.errstate(over="ignore", invalid="ignore"):
        energy = d * d if squared else d
    counts = (ids >= 0) & (ids < n) & np.isfinite(energy)
    if m == n:
        counts &= ids != np.arange(m)[:, None]
    betas, cond = np.zeros((m, len(scales)), f), np.zeros((m, k), f)
    for i in range(m):
        e = energy[i][counts[i]]
        e = e - e.min() if e.size else e
        for s, perp in enumerate(scales):
            target = f(np.log(perp))
            beta, lo, hi = f(1), f(-np.inf), f(np.inf)
            for step in range(100):
                p = np.exp(-beta * e)
                total = max(p.sum(dtype=f), f(1e-8))
                h = np.log(total) + beta * (e * p).sum(dtype=f) / total
                if abs(h - target) <= f(1e-5) or step == 99:  # (no update follows the 100th evaluation)
                    break
                if h > target:
                    lo = beta
                    beta = beta * f(2) if hi == np.inf else (beta + hi) / f(2)
                else:
                    hi = beta
                    beta = beta / f(2) if lo == -np.inf else (beta + lo) / f(2)
            betas[i, s] = beta
            cond[i, counts[i]] += p / total
    return betas, cond / f(len(scales))


def model_matrix(ids, cond, n, symmetrize=True, normalize=True):
    """The conditional entries as a matrix of their type: entries that round to 0 in float32 dropped, P + P.T, over the total."""
    f = cond.dtype.type
    keep = cond.astype(np.float32) != 0
    a = sp.csr_array((cond[keep], (np.nonzero(keep)[0], ids[keep])), shape=(ids.shape[0], n))
    total = cond[keep].sum(dtype=f)
    if symmetrize:
        a = (a + a.T).tocsr()
    if normalize and total > 0:
        a = (a / f(f(2) * total if symmetrize else total)).astype(f)
    a.data[a.data.astype(np.float32) == 0] = 0
    a.eliminate_zeros()
    a.sort_indices()
    return a


def row_entropies(a):
    """The float64 entropy of every row of a CSR matrix whose rows sum to 1 (0 for an empty row)."""
    data = np.asarray(a.data, np.float64)
    h = np.zeros(a.shape[0])
    np.add.at(h, np.repeat(np.arange(a.shape[0]), np.diff(a.indptr)), -data * np.log(data))
    return h
