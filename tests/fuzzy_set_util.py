"""The host model of the fuzzy simplicial set (pynndescent_amd/fuzzy.py, csrc/fuzzy.hip): a plain numpy restatement of UMAP's
smooth_knn_dist, compute_membership_strengths and set operations, in float64 -- and, for the noise floor of the formulation,
the same lines in float32."""
import numpy as np
import scipy.sparse as sp


def model_fuzzy_set(ids, dists, n, lc=1.0, bandwidth=1.0, mix=1.0, set_ops=True, f=np.float64):
    """(csr_array with data of type ``f``, sigmas, rhos float32, the (m, k) weights rounded to float32)."""
    m, k = ids.shape
    d, full = np.asarray(dists, np.float32), (ids >= 0) & (ids < n)
    mean_all = d[full].astype(np.float64).mean() if full.any() else 0.0
    lc = np.float32(lc)
    idx = int(np.floor(lc))
    t, target = np.float32(lc - np.float32(idx)), f(np.log2(k) * bandwidth)
    sigmas, rhos, weights = np.zeros(m, f), np.zeros(m, np.float32), np.zeros((m, k), np.float32)
    for i in range(m):
        row, on = d[i], full[i]
        nz = row[on & (row > 0)]
        if len(nz) >= lc:
            if idx > 0:
                rho = nz[idx - 1]
                if t > np.float32(1e-5):
                    rho = np.float32(rho + np.float32(t * np.float32(nz[idx] - nz[idx - 1])))
            else:
                rho = np.float32(t * nz[0])
        else:
            rho = nz.max() if len(nz) else np.float32(0)
        gap = np.maximum(row[1:][on[1:]].astype(f) - f(rho), f(0))  # (exp(-0 / mid) is the 1 a place at or below rho adds)
        lo, hi, mid = f(0), f(np.inf), f(1)
        for _ in range(64):
            psum = np.exp(-gap / mid).sum(dtype=f)
            if abs(psum - target) < f(1e-5):
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / f(2)
            else:
                lo = mid
                mid = mid * f(2) if hi == np.inf else (lo + hi) / f(2)
        mean = (row[on].astype(np.float64).mean() if on.any() else 0.0) if rho > 0 else mean_all
        sigma = f(max(np.float64(mid), 1e-3 * mean))
        w = np.where(sigma == 0, f(1), np.exp(-np.maximum(row.astype(f) - f(rho), f(0)) / sigma))
        w[~on | (ids[i] == i)] = 0
        sigmas[i], rhos[i], weights[i] = sigma, rho, w
    keep = weights != 0
    a = sp.csr_array((weights[keep].astype(f), (np.nonzero(keep)[0], ids[keep])), shape=(m, n))
    if set_ops:
        p = a.multiply(a.T)
        a = (mix * (a + a.T - p) + (1.0 - mix) * p).tocsr()
        a.data[a.data.astype(np.float32) == 0] = 0
        a.eliminate_zeros()
    a.sort_indices()
    return a, sigmas, rhos, weights


def deviation(got, want, relative):
    """The largest |got - want|, over |want| where ``relative``; 0 for empty arrays."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    if relative:
        err = err / np.maximum(np.abs(np.asarray(want, np.float64)), 1e-300)
    return float(err.max()) if err.size else 0.0
