"""float64 evaluations of the reference's dot / inner_product / correlation / hellinger distances (distances.py:680,
759, 1284, 1387) and the fixture inputs of tests/golden/make_golden_metrics.py.  Test helpers only."""
import numpy as np

from tests.util_data import clustered

FLT_MAX = float(np.finfo(np.float32).max)
NEW_METRICS = ("dot", "inner_product", "correlation", "hellinger")


def metric_data(metric, n=2000, d=16, seed=11):
    """The fixture point set of one metric (rows [0, n) build, the rest are held-out queries): clustered, non-negative
    for hellinger; zero rows for dot / correlation / hellinger and a constant row for correlation."""
    x = clustered(n + 200, d, 6, 24, seed, nonneg=metric == "hellinger")
    if metric == "inner_product":
        x = x + np.float32(0.5)  # mostly positive inner products, some negative ones
    if metric in ("dot", "correlation", "hellinger"):
        x[[7, 500, 1500]] = 0.0
    if metric == "correlation":
        x[[11, 900]] = np.float32(0.3)
        x[[1200]] = np.float32(-2.0)
    return np.ascontiguousarray(x[:n]), np.ascontiguousarray(x[n:])


def alt_dist(metric, a, b):
    """(len(a), len(b)) float64 matrix of the reference's distance in its alternative space."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if metric in ("dot", "inner_product"):
        g = a @ b.T
        with np.errstate(divide="ignore", invalid="ignore"):
            r = -np.log2(g) if metric == "dot" else 1.0 / g
        return np.where(g <= 0.0, FLT_MAX, r)
    if metric == "correlation":
        ac = a - a.mean(1, keepdims=True)
        bc = b - b.mean(1, keepdims=True)
        na, nb = (ac * ac).sum(1), (bc * bc).sum(1)
        g = ac @ bc.T
        with np.errstate(divide="ignore", invalid="ignore"):
            r = 1.0 - g / np.sqrt(np.outer(na, nb))
        r = np.where(g == 0.0, 1.0, r)
        return np.where((na[:, None] == 0.0) & (nb[None, :] == 0.0), 0.0, r)
    if metric == "hellinger":
        g = np.sqrt(a) @ np.sqrt(b).T
        la, lb = a.sum(1), b.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.log2(np.sqrt(np.outer(la, lb)) / g)
        z = (la[:, None] == 0.0) & (lb[None, :] == 0.0)
        one = (la[:, None] == 0.0) | (lb[None, :] == 0.0) | (g <= 0.0)
        return np.where(z, 0.0, np.where(one, FLT_MAX, r))
    raise ValueError(metric)


def transformed(metric, a):
    """float64 rows whose plain inner product the Gram kernels take: centred for correlation, square roots for hellinger
    (dot's normalisation is the caller's: the rows come in as NNDescent hands them over)."""
    a = np.asarray(a, np.float64)
    if metric == "correlation":
        return a - a.mean(-1, keepdims=True)
    if metric == "hellinger":
        return np.sqrt(a)
    return a


def abs_cos(metric, a, b):
    """|cos| of every (a, b) pair in the metric's transformed space (nan for a zero row): where it is small, the float32
    Gram value cancels and a stored distance carries a larger relative error."""
    ta, tb = transformed(metric, a), transformed(metric, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(ta @ tb.T) / np.outer(np.linalg.norm(ta, axis=1), np.linalg.norm(tb, axis=1))


def alt_dist_pairs(metric, a, b):
    """alt_dist of the pairs (a[i], b[i]) for any leading shape: (..., d) x (..., d) -> (...) float64, and their |cos|."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ta, tb = transformed(metric, a), transformed(metric, b)
    g = (ta * tb).sum(-1)
    na, nb = (ta * ta).sum(-1), (tb * tb).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.abs(g) / np.sqrt(na * nb)
        if metric in ("dot", "inner_product"):
            r = -np.log2(g) if metric == "dot" else 1.0 / g
            return np.where(g <= 0.0, FLT_MAX, r), cos
        if metric == "correlation":
            r = np.where(g == 0.0, 1.0, 1.0 - g / np.sqrt(na * nb))
            return np.where((na == 0.0) & (nb == 0.0), 0.0, r), cos
        if metric == "hellinger":
            la, lb = a.sum(-1), b.sum(-1)
            r = np.log2(np.sqrt(la * lb) / g)
            one = (la == 0.0) | (lb == 0.0) | (g <= 0.0)
            return np.where((la == 0.0) & (lb == 0.0), 0.0, np.where(one, FLT_MAX, r)), cos
    raise ValueError(metric)


def correct(metric, d):
    """The reference's correction of alt-space distances (float64)."""
    d = np.asarray(d, np.float64)
    if metric == "dot":
        return 1.0 - np.power(2.0, -d)
    if metric == "inner_product":
        with np.errstate(divide="ignore"):
            return np.where(d >= FLT_MAX, 0.0, -1.0 / d)
    if metric == "hellinger":
        return np.sqrt(1.0 - np.power(2.0, -d))
    return d


def brute_knn(metric, x, q=None, k=10):
    """Exact k nearest rows of x for every row of q (default: x itself, the row included) by the alt distance; ties by id."""
    q = x if q is None else q
    out = np.empty((q.shape[0], k), np.int64)
    for s in range(0, q.shape[0], 512):
        dm = alt_dist(metric, q[s:s + 512], x)
        out[s:s + 512] = np.argsort(dm, axis=1, kind="stable")[:, :k]
    return out


def recall(true_idx, idx):
    k = true_idx.shape[1]
    return float(np.mean([len(set(t) & set(r[:k])) / k for t, r in zip(true_idx, idx)]))


def self_first_share(idx):
    return float(np.mean(idx[:, 0] == np.arange(idx.shape[0])))
