"""Helpers of the tests of the metrics with a linear map (seuclidean, wminkowski with p = 2, mahalanobis): the fixture's
parameters, float64 evaluations of the reference's formulas (distances.py:95-197) on raw rows, and the derived error bound
of the transform kernel.  Test helpers only."""
import numpy as np

from tests import metric_util as MU

METRICS = ("mahalanobis", "seuclidean", "wminkowski")
U = 2.0 ** -24  # unit roundoff of float32


def fixture_data():
    """The fixture rows of tests/golden/make_golden_linear.py: metric_data("euclidean"), 2000 x 16 and 200 queries."""
    return MU.metric_data("euclidean")


def fixture_kwds(x):
    """metric_kwds of the three metrics for the fixture rows ``x``, in the reference's positional order: a fixed SPD VI, V = the
    column variances, a fixed w with one zero entry (and p = 2)."""
    d = x.shape[1]
    rng = np.random.RandomState(5)
    b = rng.standard_normal((d, d))
    vi = b @ b.T / d + 0.5 * np.eye(d)
    w = 0.1 + 2.0 * rng.rand(d)
    w[3] = 0.0
    return {"mahalanobis": {"vinv": vi}, "seuclidean": {"sigma": x.astype(np.float64).var(axis=0)}, "wminkowski": {"w": w, "p": 2.0}}


def quadratic_form(metric, kwds):
    """The float64 symmetric matrix M with distance(x, y)^2 = (x - y)^T M (x - y)."""
    args = list(kwds.values())
    if metric == "mahalanobis":
        vi = np.asarray(args[0], np.float64)
        return (vi + vi.T) / 2.0
    if metric == "seuclidean":
        return np.diag(1.0 / np.asarray(args[0], np.float64))
    if metric == "wminkowski":
        return np.diag(np.asarray(args[0], np.float64))
    raise ValueError(metric)


def true_dist_pairs(metric, kwds, a, b):
    """The metric's float64 formula on raw rows for the pairs (a[..., :], b[..., :])."""
    diff = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    m = quadratic_form(metric, kwds)
    return np.sqrt(np.maximum(np.einsum("...i,ij,...j->...", diff, m, diff), 0.0))


def brute_knn(metric, kwds, x, q=None, k=10):
    """Exact k nearest rows of x for every row of q (default x itself, the row included) in float64; ties by id."""
    x = np.asarray(x, np.float64)
    q = x if q is None else np.asarray(q, np.float64)
    m = quadratic_form(metric, kwds)
    xm = x @ m
    xx = (xm * x).sum(1)
    out = np.empty((q.shape[0], k), np.int64)
    for s in range(0, q.shape[0], 512):
        qs = q[s:s + 512]
        d2 = ((qs @ m) * qs).sum(1)[:, None] - 2.0 * qs @ xm.T + xx[None, :]
        # (the expanded form only ranks; refine the candidates with the difference form, which cancels nothing)
        cand = np.argsort(d2, axis=1, kind="stable")[:, :4 * k]
        exact = true_dist_pairs(metric, kwds, qs[:, None, :], x[cand])
        order = np.lexsort((cand, exact), axis=1)[:, :k]
        out[s:s + 512] = np.take_along_axis(cand, order, axis=1)
    return out


def transform_f64(kind, a32, c32, x32):
    """float64 ``A (x - c)`` of the float32 operands (kind 0: diagonal, 1: dense): exact up to float64 rounding."""
    xc = np.asarray(x32, np.float64) - np.asarray(c32, np.float64)
    a = np.asarray(a32, np.float64)
    return xc * a if kind == 0 else xc @ a.T


def transform_bound(kind, a32, c32, x32):
    """The componentwise bound of the transform kernel's error against ``transform_f64``:

        |Y~_j - Y_j| <= (d + 3) * 2^-24 * sum_k |A_jk| |x_k - c_k|

    Derivation (u = 2^-24, first order): the float32 subtraction rounds x_k - c_k once (relative u); a sum of d products in any
    order rounds each product once and passes it through at most d - 1 additions, or takes d fused steps: at most d further
    factors (1 + u) on every term, d + 1 in all; the float32 rounding of A itself (the factor is computed in float64) adds one
    more where the truth is taken with the float64 A: d + 2.  (d + 3) u covers the second-order terms: (1 + u)^(d+2) - 1 <
    (d + 3) u for every d below 2^20.  No subnormal results: the bound has no absolute term."""
    d = np.asarray(x32).shape[1]
    xc = np.abs(np.asarray(x32, np.float64) - np.asarray(c32, np.float64))
    a = np.abs(np.asarray(a32, np.float64))
    return (d + 3) * U * (xc * a if kind == 0 else xc @ a.T)
